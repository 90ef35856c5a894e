#!/usr/bin/env python3
"""Probabilistic verification (run_prob: dressed and map scores, 4 thresholds, 4 levels, 12 sigma edges) of a synthetic event
(40 frames x 128 x 128, uint8 truth, f32 prediction and variance map) on the MI355X.
End to end: run_prob from host (numpy) arrays, upload included, and from arrays already on the device; median of --reps runs after
one warm-up, wall clock around a call that ends in the evaluator's host sync.  Per stage: each native call alone on device-resident
inputs, device events around --inner back-to-back launches (ms per launch), median of --reps after one warm-up: the point pass
(sigma^2 = 0, which yields the MSE), the dressed pass (one scalar variance), the map pass and the merge of one pass's records.
Bounds, counted from the shapes: HBM = the bytes one pass reads (prediction, variance, truth, selection table) and writes (records)
at 8 TB/s; fp64 VALU = per scored pixel the device-library calls of the pass (erfc: 3 + thresholds under censoring, exp: 2, sqrt,
divisions) at a nominal 48 / 24 / 16 fp64 operations each plus 90 operations of plain arithmetic, at 78.6 TFLOP/s.  The nominal
costs are estimates, not counts of the library's instructions: the fp64 fraction is an order of magnitude, the HBM one is exact.
Prints one JSON line.

usage: python tools/prob_bench.py [--frames 40] [--hw 128] [--reps 5] [--inner 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd")]

HBM_BYTES_PER_S = 8.0e12
FP64_FLOPS = 78.6e12
C_ERFC, C_EXP, C_DIV, C_PLAIN = 48, 24, 16, 90


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    from p2igan_bench import ops
    from p2igan_bench.evaluation import DEFAULT_THRESHOLDS, ProbEvaluator, run_prob
    if not torch.cuda.is_available():
        raise SystemExit("prob_bench measures on the GPU; none is visible")
    dev = torch.device("cuda")
    S, T = a.hw, a.frames
    rng = np.random.default_rng(77)
    g = np.clip(rng.gamma(0.3, 60.0, size=(T, S, S)), 0.0, 255.0) * (rng.random((T, S, S)) < 0.6)
    truth = np.rint(g).astype(np.uint8)
    var = np.exp(rng.normal(np.log(30.0), 1.0, size=(T, S, S))).astype(np.float32)
    pred = np.maximum(g + np.sqrt(var) * rng.standard_normal((T, S, S)), 0.0).astype(np.float32)
    mask = rng.random((S, S)) < 0.02
    preds, variances = {"krig": pred, "flat": pred}, {"krig": var}

    def run(p, v, t):
        t0 = time.perf_counter()
        res = run_prob(p, v, t, mask, "radar", S)
        return (time.perf_counter() - t0) * 1e3, res

    res = run(preds, variances, truth)[1]                  # warm-up (library load, allocator)
    host = [run(preds, variances, truth)[0] for _ in range(a.reps)]
    pd, vd, td = (torch.from_numpy(x).to(dev) for x in (pred, var, truth))
    torch.cuda.synchronize()
    run({"krig": pd, "flat": pd}, {"krig": vd}, td)
    devt = [run({"krig": pd, "flat": pd}, {"krig": vd}, td)[0] for _ in range(a.reps)]

    ev = ProbEvaluator(S, mask)
    lay, K = ev.layout, len(DEFAULT_THRESHOLDS)
    nw = lay.nf + lay.ni
    nwg = -(-T * S * S // ops.PROB_WG_PIXELS)
    part = torch.empty(nwg * nw, device=dev, dtype=torch.float64)
    acc = torch.zeros(nw, device=dev, dtype=torch.float64)
    mse = res["krig"]["dressed"]["sigma0_sq"]

    def acc_with(v):
        return lambda: ops.prob_accumulate(pd, v, td, (0, 0), (0, 0), (0, 0), S, S, ev._rank, ev._lut, ev.thresholds, ev.xq, ev.halfwidths,
                                           ev.sigma_edges, ev.pit_bins, ev.rel_bins, True, True, part)
    stages = {"point": acc_with(0.0), "dressed": acc_with(mse), "map": acc_with(vd), "merge": lambda: ops.prob_merge(part, lay.nf, lay.ni, acc)}
    stage_ms = {}
    for name, fn in stages.items():
        times = []
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(e0.elapsed_time(e1) / a.inner)
        stage_ms[name] = round(statistics.median(times), 4)
    n = res["krig"]["map"]["n"]
    px = T * S * S
    bytes_map = px * (4 + 4 + 1) + S * S * 4 + nwg * nw * 8
    flop_map = n * ((3 + K) * C_ERFC + 2 * C_EXP + 4 * C_DIV + C_PLAIN)
    out = {"tool": "prob_bench", "frames": T, "hw": S, "thresholds": K, "scored_pixels": n, "workgroups": nwg, "record_words": nw,
           "run_prob_from_host_ms": round(statistics.median(host), 2), "run_prob_from_device_ms": round(statistics.median(devt), 2),
           "spread_from_device_ms": [round(min(devt), 2), round(max(devt), 2)], "runs": a.reps, "inner": a.inner, "stage_ms": stage_ms,
           "map_hbm_bound_ms": round(bytes_map / HBM_BYTES_PER_S * 1e3, 5), "map_fp64_bound_ms": round(flop_map / FP64_FLOPS * 1e3, 5),
           "map_fraction_of_hbm_bound": round(bytes_map / HBM_BYTES_PER_S * 1e3 / stage_ms["map"], 4),
           "map_fraction_of_fp64_bound": round(flop_map / FP64_FLOPS * 1e3 / stage_ms["map"], 4),
           "crps_map": res["krig"]["map"]["CRPS"], "crps_dressed": res["krig"]["dressed"]["CRPS"],
           "crpss_map_vs_dressed": res["krig"]["CRPSS_map_vs_dressed"], "cov90_map": res["krig"]["map"]["coverage"]["0.9"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
