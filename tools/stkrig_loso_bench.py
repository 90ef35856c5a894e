#!/usr/bin/env python3
"""Leave-one-site-out cross-validation of space-time kriging at the benchmark size (B=8, T=16, 128x128) on the
MI355X, for section 17's two masks (block-10: 169 sites, N_st = 2704 points per sample; block-8: 256 sites, N_st = 4096): ms per stage
from device events (median over a >= 0.5 s window after warm-up) -- site-major gather, factor, solve, invert, band Gram, site solve --
the whole cross_validate_sites call (fitted and fixed variogram), and beside it the forward of the same model on the same inputs.  No
time target exists yet: the numbers are recorded (profiles/README.md).  Prints one JSON line.

usage: python tools/stkrig_loso_bench.py [--b 8] [--t 16] [--hw 128] [--blocks 10 8]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from classical_bench import timed  # noqa: E402
from stkrig_bench import FIXED  # noqa: E402


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
    res = {"workload": "space_time_kriging_loso", "B": b, "T": t, "H": h, "W": w, "masks": {}}
    for block in a.blocks:
        _, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(b, t, h, w, seeded.block_mask(h, w, block))]
        x, m = masked.reshape(b, t, h, w), masks.reshape(b, t, h, w)
        pix, z, info = ops.krig_compact(x, m, ops.KRIG_MAX_CAP)
        n_st = int(info[:b * t].view(b, t).sum(1).max())
        np_ = max(32, (n_st + 31) // 32 * 32)
        lag = (min(h, w) / 2.0) / 16
        sites = ops.stkrig_gather_sites(pix, z, info, b, t, np_)
        out = {"points_per_sample": n_st, "padded_system": np_, "sites_per_sample": int(sites["nsites"].max())}
        _, _, cand, params = ops.stkrig_variogram(pix, z, info, b, t, 16, 3, lag, 0)
        out["gather_sites_ms"] = timed(lambda: ops.stkrig_gather_sites(pix, z, info, b, t, np_))
        work = torch.empty(b * np_ * np_, device=dev)
        winv = torch.empty(b * np_ * np_, device=dev)
        status = torch.zeros(b, device=dev, dtype=torch.int32)
        alpha = torch.empty(b, np_, device=dev)
        mean = torch.empty(b, device=dev)
        pred, var = torch.zeros_like(z), torch.zeros_like(z)
        ch = ops.KrigSystems(sites["stpix"], sites["stz"], sites["stinfo"], params, cand, 0, 1, 1, np_, status).chunk(0, b)
        out["factor_ms"] = timed(lambda: ops.stkrig_factor(ch, sites["stt"], work))
        out["solve_ms"] = timed(lambda: ops.krig_solve(ch, work, alpha, mean))
        sol = ops.krig_solve(ch, work, alpha, mean)
        out["invert_ms"] = timed(lambda: ops.krig_invert(work, b, np_, winv))
        out["site_gram_ms"] = timed(lambda: ops.stkrig_site_gram(winv, b, np_))
        gram = ops.stkrig_site_gram(winv, b, np_)
        out["site_solve_ms"] = timed(lambda: ops.stkrig_loso(ch, gram, sol, alpha, sites, t, pred, var))
        out["failed_pivots"] = int(status.sum())
        out["points_without_a_prediction"] = int(torch.isnan(pred).sum())
        del work, winv, gram
        for label, model in (("fit", {"name": "stkriging"}), ("fixed", {"name": "stkriging", "variogram": FIXED})):
            G = build_generator({"model": model}).to(dev)
            out[f"cross_validate_sites_{label}_ms"] = timed(lambda: G.cross_validate_sites(masked, masks))
            out[f"forward_{label}_ms"] = timed(lambda: G(masked, masks))
            out[f"loso_scores_{label}"] = {k: round(v, 6) for k, v in G.cross_validate_sites(masked, masks).scores().items()}
        res["masks"][f"block{block}"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
