#!/usr/bin/env python3
"""Space-time ordinary kriging (model.name: stkriging) at the benchmark size (B=8, T=16, 128x128) on the MI355X,
for a block-10 mask (169 gauges per frame, N_st = 2704 points per sample) and a block-8 mask (256 per frame: N_st = 4096, the largest
set that fits max_points): ms per stage from device events (median over a >= 0.5 s window after warm-up) -- gather, variogram bins +
fit, factor, solve, predict -- the whole forward (fitted and fixed variogram), and beside them the per-frame `kriging` forward on the
same inputs.  No time target exists yet: the numbers are recorded (profiles/README.md).  Prints one JSON line.

usage: python tools/stkrig_bench.py [--b 8] [--t 16] [--hw 128] [--blocks 10 8]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=16)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--blocks", type=int, nargs="+", default=[10, 8])
    a = ap.parse_args()
    from p2igan_bench import _hip, ops
    from p2igan_bench.models import build_generator
    from p2igan_bench.utils import seeded
    _hip.load()
    dev = torch.device("cuda:0")
    b, t, h, w = a.b, a.t, a.hw, a.hw
    res = {"workload": "space_time_kriging", "B": b, "T": t, "H": h, "W": w, "masks": {}}
    for block in a.blocks:
        _, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(b, t, h, w, seeded.block_mask(h, w, block))]
        x, m = masked.reshape(b, t, h, w), masks.reshape(b, t, h, w)
        pix, z, info = ops.krig_compact(x, m, ops.KRIG_MAX_CAP)
        n_st = int(info[:b * t].view(b, t).sum(1).max())
        np_ = max(32, (n_st + 31) // 32 * 32)
        lag = (min(h, w) / 2.0) / 16
        out = {"gauges_per_frame": int(info[:b * t].max()), "points_per_sample": n_st, "padded_system": np_}
        stpix, stt, stz, stinfo = ops.stkrig_gather(pix, z, info, b, t, np_)
        _, fit, cand, params = ops.stkrig_variogram(pix, z, info, b, t, 16, 3, lag, 0)
        out["fitted_nugget_psill_range_kappa_sample0"] = [round(v, 6) for v in fit[0, :4].cpu().tolist()]
        out["compact_ms"] = timed(lambda: ops.krig_compact(x, m, ops.KRIG_MAX_CAP))
        out["gather_ms"] = timed(lambda: ops.stkrig_gather(pix, z, info, b, t, np_))
        out["variogram_bins_and_fit_ms"] = timed(lambda: ops.stkrig_variogram(pix, z, info, b, t, 16, 3, lag, 0))
        work = torch.empty(b * np_ * np_, device=dev)
        status = torch.zeros(b, device=dev, dtype=torch.int32)
        alpha = torch.empty(b, np_, device=dev)
        mean = torch.empty(b, device=dev)
        ch = ops.KrigSystems(stpix, stz, stinfo, params, cand, 0, 1, 1, np_, status).chunk(0, b)
        out["factor_ms"] = timed(lambda: ops.stkrig_factor(ch, stt, work))
        out["solve_ms"] = timed(lambda: ops.krig_solve(ch, work, alpha, mean))
        out["predict_ms"] = timed(lambda: ops.stkrig_predict(stpix, stt, alpha, mean, stinfo, params, 0, t, h, w))
        out["failed_pivots"] = int(status.sum())
        del work
        for label, model in (("stkriging_fit", {"name": "stkriging"}), ("stkriging_fixed", {"name": "stkriging", "variogram": FIXED}),
                             ("kriging_fit_per_frame_systems_shared", {"name": "kriging"})):
            G = build_generator({"model": model}).to(dev)
            out[f"forward_{label}_ms"] = timed(lambda: G(masked, masks))
        res["masks"][f"block{block}"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
