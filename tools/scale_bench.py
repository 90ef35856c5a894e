#!/usr/bin/env python3
"""Scale-aware verification (run_scale: FSS over 4 thresholds x 7 neighbourhood sizes, radial power spectra) of a synthetic test set
at full size (4 methods x 10 events x 240 frames x 128 x 128, uint8 truth, f32 predictions) on the MI355X.
End to end: run_scale from host (numpy) arrays, upload included, and from arrays already on the device; median of --reps runs after
one warm-up, wall clock around a call that ends in the evaluator's host sync.  Per stage: each native call alone over the same
pieces on device-resident inputs, device events around the whole sweep (ms for the whole workload), median of --reps sweeps after
one warm-up.  Prints one JSON line.

usage: python tools/scale_bench.py [--methods 4] [--events 10] [--frames 240] [--hw 128] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--methods", type=int, default=4)
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from p2igan_bench import ops
    from p2igan_bench.evaluation import DEFAULT_SCALES, DEFAULT_THRESHOLDS, ScaleEvaluator, run_scale
    if not torch.cuda.is_available():
        raise SystemExit("scale_bench measures on the GPU; none is visible")
    dev = torch.device("cuda")
    S, T = a.hw, a.frames

    def box3(g):
        p = np.pad(g, ((0, 0), (1, 1), (1, 1)), mode="edge")
        return sum(p[:, dy:dy + S, dx:dx + S] for dy in range(3) for dx in range(3)) / np.float32(9.0)

    keys = [f"event_{i + 1:02d}" for i in range(a.events)]
    truth, preds = {}, {f"m{j}": {} for j in range(a.methods)}
    for i, k in enumerate(keys):
        g = np.clip(np.random.default_rng(900 + i).gamma(0.3, 60.0, size=(T, S, S)), 0.0, 255.0).astype(np.float32)
        b = box3(g)
        truth[k] = np.rint(g).astype(np.uint8)
        for j in range(a.methods):
            w = np.float32((j + 1) / a.methods)
            preds[f"m{j}"][k] = (1 - w) * g + w * b

    def run(p, t):
        t0 = time.perf_counter()
        res = run_scale(p, t, S)
        return (time.perf_counter() - t0) * 1e3, res

    res = run(preds, truth)[1]                          # warm-up (library load, allocator)
    host = [run(preds, truth)[0] for _ in range(a.reps)]
    truth_d = {k: torch.from_numpy(v).to(dev) for k, v in truth.items()}
    preds_d = {m: {k: torch.from_numpy(v).to(dev) for k, v in p.items()} for m, p in preds.items()}
    torch.cuda.synchronize()
    run(preds_d, truth_d)
    devt = [run(preds_d, truth_d)[0] for _ in range(a.reps)]

    # stages: the same pieces (one per method and event), each native call alone
    ev = ScaleEvaluator(S)
    K, N, R = len(DEFAULT_THRESHOLDS), len(DEFAULT_SCALES), S // 2 + 1
    pieces = [(preds_d[m][k], truth_d[k]) for m in preds_d for k in keys]
    part = torch.empty(T, K, 3 * N + 1, device=dev, dtype=torch.int64)
    acc = torch.zeros(K * (3 * N + 1), device=dev, dtype=torch.int64)
    G = torch.empty(T * 4 * S * R, device=dev, dtype=torch.float64)
    psd = torch.empty(T * 2 * S * R, device=dev, dtype=torch.float64)
    P = torch.empty(T, 2, R, device=dev, dtype=torch.float64)
    flag = torch.zeros(T, 2, device=dev, dtype=torch.int32)
    Pall = torch.empty(T * a.events, 2, R, device=dev, dtype=torch.float64)
    fall = torch.zeros(T * a.events, 2, device=dev, dtype=torch.int32)
    lib, st = ops._hip.load(), ops._stream
    order, weight, offsets, count = ev._rings
    tl = (0, 0)

    def rows(p, g):
        for field, x in enumerate((p, g)):
            ops._hip.check(lib.p2i_scale_dft_rows(ops._eval_input(x, tl), T, S, field, ops._ptr(ev._lut), 1, ops._ptr(ev._tw), ops._ptr(G),
                                                  ops._ptr(flag), st()), "rows")

    stages = {
        "fss": lambda p, g: ops.scale_fss(p, g, tl, tl, S, ev._lut, DEFAULT_THRESHOLDS, DEFAULT_SCALES, True, part),
        "fss_merge": lambda p, g: ops.scale_fss_merge(part, acc),
        "dft_rows": rows,
        "dft_cols": lambda p, g: ops._hip.check(lib.p2i_scale_dft_cols(ops._ptr(G), T, S, ops._ptr(ev._tw), ops._ptr(psd), st()), "cols"),
        "rings": lambda p, g: ops._hip.check(lib.p2i_scale_rings(ops._ptr(psd), T, S, ops._ptr(order), ops._ptr(weight), ops._ptr(offsets),
                                                                 ops._ptr(count), R, ops._ptr(P), st()), "rings"),
    }
    stage_ms = {}
    for name, fn in stages.items():
        times = []
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for p, g in pieces:
                fn(p, g)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(e0.elapsed_time(e1))
        stage_ms[name] = round(statistics.median(times), 3)
    times = []
    for rep in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.methods):
            ops.scale_spectrum_merge(Pall, fall)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            times.append(e0.elapsed_time(e1))
    stage_ms["spectrum_merge"] = round(statistics.median(times), 3)
    # the work the algorithm needs, from the shapes: fp64 FMAs of the two dense products, per frame and field
    frames = a.methods * a.events * T
    fma = 2 * frames * (S * R * S * 2 + S * R * S * 4)
    out = {"tool": "scale_bench", "methods": a.methods, "events": a.events, "frames": T, "hw": S, "thresholds": K, "scales": N,
           "run_scale_from_host_ms": round(statistics.median(host), 2), "run_scale_from_device_ms": round(statistics.median(devt), 2),
           "spread_from_device_ms": [round(min(devt), 2), round(max(devt), 2)], "runs": a.reps, "stage_ms": stage_ms,
           "dft_fp64_tflops": round(2 * fma / ((stage_ms["dft_rows"] + stage_ms["dft_cols"]) * 1e-3) / 1e12, 2),
           "fss_thr2_n9_m0": res["m0"]["FSS"]["thr_2"]["n_9"], "lsd_m0": res["m0"]["LSD"], "hf_ratio_m0": res["m0"]["HF_ratio"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
