#!/usr/bin/env python3
"""Lagrangian space-time kriging (model.name: lagkriging) at the benchmark size (B=8, T=16, 128x128, 79 gauges
per frame at fixed sites: N_st = 1264 points per sample) on the MI355X: ms per stage from device events (median over a >= 0.5 s window
after warm-up) -- velocity score + choice, variogram bins + fit, factor, solve, predict -- beside the same stages of `stkriging` on
the same inputs, and the whole forward of both (fitted and given velocity).  No time target exists yet: the numbers are recorded
(profiles/README.md).  Prints one JSON line.

usage: python tools/lagkrig_bench.py [--b 8] [--t 16] [--hw 128] [--gauges 79]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from classical_bench import timed  # noqa: E402

GIVEN = {"fit": False, "vy": 2.5, "vx": -1.5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=16)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--gauges", type=int, default=79)
    a = ap.parse_args()
    from p2igan_bench import _hip, ops
    from p2igan_bench.models import build_generator
    from p2igan_bench.utils import seeded
    _hip.load()
    dev = torch.device("cuda:0")
    b, t, h, w = a.b, a.t, a.hw, a.hw
    _, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(b, t, h, w, seeded.gauge_mask(h, w, a.gauges))]
    x, m = masked.reshape(b, t, h, w), masks.reshape(b, t, h, w)
    pix, z, info = ops.krig_compact(x, m, ops.KRIG_MAX_CAP)
    n_st = int(info[:b * t].view(b, t).sum(1).max())
    np_ = max(32, (n_st + 31) // 32 * 32)
    lag = (min(h, w) / 2.0) / 16
    nhalf, vstep, n_tlags = 8, 0.5, min(3, t - 1)
    pairs = sum((t - u) * a.gauges * a.gauges for u in range(1, n_tlags + 1))
    out = {"workload": "lagrangian_space_time_kriging", "B": b, "T": t, "H": h, "W": w, "gauges_per_frame": int(info[:b * t].max()),
           "points_per_sample": n_st, "padded_system": np_, "velocity_candidates": (2 * nhalf + 1) ** 2, "velocity_pairs_per_sample": pairs}
    stpix, stt, stz, stinfo = ops.stkrig_gather(pix, z, info, b, t, np_)
    score, weight, support, vel, velf, vcand = ops.lagkrig_velocity(pix, z, info, b, t, n_tlags, nhalf, vstep, 1.5 * lag)
    _, fit, cand, params = ops.lagkrig_variogram(pix, z, info, vel, b, t, 16, n_tlags, lag, 0)
    _, sfit, scand, sparams = ops.stkrig_variogram(pix, z, info, b, t, 16, n_tlags, lag, 0)
    out["fitted_velocity_sample0"] = vel[0].cpu().tolist()
    out["fitted_nugget_psill_range_kappa_sample0"] = [round(v, 6) for v in fit[0, :4].cpu().tolist()]
    out["stkriging_fitted_nugget_psill_range_kappa_sample0"] = [round(v, 6) for v in sfit[0, :4].cpu().tolist()]
    out["velocity_ms"] = timed(lambda: ops.lagkrig_velocity(pix, z, info, b, t, n_tlags, nhalf, vstep, 1.5 * lag))
    out["variogram_bins_and_fit_ms"] = timed(lambda: ops.lagkrig_variogram(pix, z, info, vel, b, t, 16, n_tlags, lag, 0))
    out["stkriging_variogram_bins_and_fit_ms"] = timed(lambda: ops.stkrig_variogram(pix, z, info, b, t, 16, n_tlags, lag, 0))
    work = torch.empty(b * np_ * np_, device=dev)
    status = torch.zeros(b, device=dev, dtype=torch.int32)
    alpha = torch.empty(b, np_, device=dev)
    mean = torch.empty(b, device=dev)
    sch = ops.KrigSystems(stpix, stz, stinfo, sparams, scand, 0, 1, 1, np_, status).chunk(0, b)
    ch = ops.KrigSystems(stpix, stz, stinfo, params, cand, 0, 1, 1, np_, status).chunk(0, b)
    out["stkriging_factor_ms"] = timed(lambda: ops.stkrig_factor(sch, stt, work))
    ops.krig_solve(sch, work, alpha, mean)
    out["stkriging_predict_ms"] = timed(lambda: ops.stkrig_predict(stpix, stt, alpha, mean, stinfo, sparams, 0, t, h, w))
    out["stkriging_failed_pivots"] = int(status.sum())
    status.zero_()
    out["factor_ms"] = timed(lambda: ops.lagkrig_factor(ch, stt, velf, work))
    out["solve_ms"] = timed(lambda: ops.krig_solve(ch, work, alpha, mean))
    out["predict_ms"] = timed(lambda: ops.lagkrig_predict(stpix, stt, alpha, mean, stinfo, params, velf, 0, t, h, w))
    out["failed_pivots"] = int(status.sum())
    del work
    for label, model in (("lagkriging_fit", {"name": "lagkriging"}), ("lagkriging_given_velocity", {"name": "lagkriging", "advection": GIVEN}),
                         ("stkriging_fit", {"name": "stkriging"})):
        G = build_generator({"model": model}).to(dev)
        out[f"forward_{label}_ms"] = timed(lambda: G(masked, masks))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
