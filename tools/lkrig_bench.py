#!/usr/bin/env python3
"""Moving-neighbourhood space-time kriging (model.name: localkriging) at the benchmark size (B=8, 128x128) on the
MI355X, for a block-10 mask (169 gauges per frame) and a block-8 mask (256 per frame), k in {16, 32, 64} and a temporal half-window
of {0, 2, 4} frames: ms of `forward`, `forward_uq` and `cross_validate_sites` at T = 16 from device events (median over a >= 0.5 s
window after warm-up, fixed variogram), `forward` at T = 16 and T = 64 at k = 32, frames = 2 (time per frame should stay flat where
`stkriging` is cubic or refuses), the variogram fit in front, and `stkriging.forward` on the same T = 16 input for the comparison row.
Then the same kernels in the Lagrangian frame (model.name: locallagkriging) against `localkriging` in the same
process and on the same block-10 input: `forward`, `forward_uq` and `cross_validate_sites` at T = 16 and T = 64, k in {16, 32, 64},
frames in {0, 2} at T = 16 and 2 at T = 64, fixed variogram and a fixed velocity (1.5, -0.5), each with its ratio to `localkriging`.
No time target exists: the numbers are recorded (profiles/README.md).  Prints one JSON line.

usage: python tools/lkrig_bench.py [--b 8] [--hw 128] [--blocks 10 8] [--ks 16 32 64] [--frames 0 2 4] [--only-lag]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from classical_bench import timed  # noqa: E402

FIXED = {"model": "exponential", "fit": False, "nugget": 0.002, "psill": 0.05, "range": 6.0, "time_scale": 2.0}
FIXED_V = {"fit": False, "vy": 1.5, "vx": -0.5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--blocks", type=int, nargs="+", default=[10, 8])
    ap.add_argument("--ks", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--frames", type=int, nargs="+", default=[0, 2, 4])
    ap.add_argument("--only-lag", action="store_true", help="the comparison of locallagkriging with localkriging only")
    a = ap.parse_args()
    from p2igan_bench import _hip
    from p2igan_bench.models import build_generator
    from p2igan_bench.utils import seeded
    _hip.load()
    dev = torch.device("cuda:0")
    b, h, w = a.b, a.hw, a.hw
    res = {"workload": "local_space_time_kriging", "B": b, "H": h, "W": w, "masks": {}}

    def local(k, frames, variogram=FIXED, name="localkriging"):
        return build_generator({"model": {"name": name, "variogram": variogram, "advection": FIXED_V,
                                          "neighbourhood": {"k": k, "frames": frames}}}).to(dev)

    def lag_section():
        """ms of (localkriging, locallagkriging, ratio) per call on the block-10 input."""
        mask = seeded.block_mask(h, w, 10)
        out = {"velocity": [FIXED_V["vy"], FIXED_V["vx"]]}
        for T, frames_list in ((16, (0, 2)), (64, (2,))):
            _, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(b, T, h, w, mask)]
            rows = {}
            for k in a.ks:
                for frames in frames_list:
                    S, G = local(k, frames), local(k, frames, name="locallagkriging")
                    row = {}
                    for what in ("forward", "forward_uq", "cross_validate_sites"):
                        s = timed(lambda: getattr(S, what)(masked, masks))
                        g = timed(lambda: getattr(G, what)(masked, masks))
                        row[f"{what}_ms"] = [s, g, round(g / s, 3)]
                    row["failed_pivots"] = [int(S.last_status.sum()), int(G.last_status.sum())]
                    rows[f"k{k}_frames{frames}"] = row
            out[f"T{T}"] = rows
        return out

    for block in ([] if a.only_lag else a.blocks):
        mask = seeded.block_mask(h, w, block)
        _, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(b, 16, h, w, mask)]
        out = {"gauges_per_frame": int(masks[0, 0].sum()), "T16": {}}
        for k in a.ks:
            for frames in a.frames:
                G = local(k, frames)
                row = {"forward_ms": timed(lambda: G(masked, masks)), "forward_uq_ms": timed(lambda: G.forward_uq(masked, masks)),
                       "cross_validate_sites_ms": timed(lambda: G.cross_validate_sites(masked, masks))}
                row["failed_pivots"] = int(G.last_status.sum())
                out["T16"][f"k{k}_frames{frames}"] = row
        G = local(32, 2, {"model": "exponential", "fit": True})
        out["forward_fit_k32_frames2_T16_ms"] = timed(lambda: G(masked, masks))
        S = build_generator({"model": {"name": "stkriging", "variogram": FIXED}}).to(dev)
        out["stkriging_forward_T16_ms"] = timed(lambda: S(masked, masks))
        _, masked64, masks64 = [x.to(dev) for x in seeded.synthetic_batch(b, 64, h, w, mask)]
        G = local(32, 2)
        out["forward_k32_frames2_T16_ms"] = out["T16"].get("k32_frames2", {}).get("forward_ms") or timed(lambda: G(masked, masks))
        out["forward_k32_frames2_T64_ms"] = timed(lambda: G(masked64, masks64))
        out["points_per_sample_T64"] = int(masks64[0].sum())
        try:
            S(masked64, masks64)
            out["stkriging_forward_T64"] = "ran"
        except ValueError as e:
            out["stkriging_forward_T64"] = f"refused: {e}"
        res["masks"][f"block{block}"] = out
    res["locallagkriging_vs_localkriging_block10"] = lag_section()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
