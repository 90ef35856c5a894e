#!/usr/bin/env python3
"""Object-based verification (run_objects: connected rain objects at 4 absolute levels and the relative one, their population and
SAL) of scale_bench's synthetic test set at full size (4 methods x 10 events x 240 frames x 128 x 128, uint8 truth, f32
predictions) on the MI355X.
End to end: run_objects from host (numpy) arrays, upload included, and from arrays already on the device; median of --reps runs after
one warm-up, wall clock around a call that ends with the scores on the host.  Per stage: each native call alone over the same pieces
on device-resident inputs, device events around the whole sweep (ms for the whole workload), median of --reps sweeps after one
warm-up; the labelling on the LDS path and, for the same crop, on the workspace path; the host's share (the read of the tables and
the float64 scores) as wall clock.  Prints one JSON line.

usage: python tools/objects_bench.py [--methods 4] [--events 10] [--frames 240] [--hw 128] [--reps 3]
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
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from p2igan_bench import ops
    from p2igan_bench.evaluation import DEFAULT_THRESHOLDS, ObjectEvaluator, run_objects
    if not torch.cuda.is_available():
        raise SystemExit("objects_bench measures on the GPU; none is visible")
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
        res = run_objects(p, t, S)
        return (time.perf_counter() - t0) * 1e3, res

    res = run(preds, truth)[1]                          # warm-up (library load, allocator)
    host = [run(preds, truth)[0] for _ in range(a.reps)]
    truth_d = {k: torch.from_numpy(v).to(dev) for k, v in truth.items()}
    preds_d = {m: {k: torch.from_numpy(v).to(dev) for k, v in p.items()} for m, p in preds.items()}
    torch.cuda.synchronize()
    run(preds_d, truth_d)
    devt = [run(preds_d, truth_d)[0] for _ in range(a.reps)]

    # the host's share of a run: the device part alone (the updates, each ending in its host read), then the read-back of the
    # tables and the scores (compute)
    ev = ObjectEvaluator(S)
    split = []
    for _ in range(a.reps + 1):
        ev.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for m in preds_d:
            for k in keys:
                ev.update(m, preds_d[m][k], truth_d[k])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ev.compute()
        split.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    split = split[1:]

    # stages: the same pieces (one per method and event), each native call alone
    L = len(DEFAULT_THRESHOLDS) + 1
    pieces = [(preds_d[m][k], truth_d[k]) for m in preds_d for k in keys]
    q = torch.empty(T * 2 * S * S, device=dev, dtype=torch.int32)
    bits = torch.empty(T * 2 * S * S, device=dev, dtype=torch.int16)
    rec = torch.empty(T, 2, 5, device=dev, dtype=torch.int64)
    lev = torch.empty(T, 2, L, 5, device=dev, dtype=torch.int64)
    counts = torch.empty(T * 2 * L, device=dev, dtype=torch.int64)
    offsets = torch.empty(T * 2 * L + 1, device=dev, dtype=torch.int64)
    lab16 = torch.empty(T * 2 * L * S * S, device=dev, dtype=torch.int16)
    lab32 = torch.empty(T * 2 * L * S * S, device=dev, dtype=torch.int32)
    tl = (0, 0)

    def quantize(p, g):
        for field, x in enumerate((p, g)):
            ops.objects_quantize(x, tl, field, S, ev._lut, DEFAULT_THRESHOLDS, ev.sal_factor, ev.sal_floor, True, q, bits, rec)

    def fill(wide):
        def f(p, g):
            # the fill consumes the labels: label again first (its time is taken off below), then size and fill the table
            labels = lab32 if wide else lab16
            ops.objects_label(bits, T, S, L, 8, labels, wide)
            ops.objects_count(labels, wide, q, T, S, L, lev, counts)
            ops.objects_scan(counts, offsets)
            table = torch.zeros(int(offsets[-1].item()), 6, device=dev, dtype=torch.int64)
            ops.objects_fill(labels, wide, q, T, S, L, offsets, table)
        return f

    lds_ok = S <= ops.OBJECTS_LDS_CROP
    stages = {"quantize": quantize}
    if lds_ok:
        stages["label_lds"] = lambda p, g: ops.objects_label(bits, T, S, L, 8, lab16, False)
        stages["count_lds"] = lambda p, g: ops.objects_count(lab16, False, q, T, S, L, lev, counts)
    stages["label_workspace"] = lambda p, g: ops.objects_label(bits, T, S, L, 8, lab32, True)
    stages["count_workspace"] = lambda p, g: ops.objects_count(lab32, True, q, T, S, L, lev, counts)
    stages["scan"] = lambda p, g: ops.objects_scan(counts, offsets)
    if lds_ok:
        stages["label_count_scan_read_fill_lds"] = fill(False)
    stages["label_count_scan_read_fill_workspace"] = fill(True)
    stage_ms = {}
    for name, fn in stages.items():
        times = []
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for p, g in pieces:
                if name != "quantize" and rep == 0:
                    quantize(p, g)              # the last piece's bits stay for the later stages
                fn(p, g)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(e0.elapsed_time(e1))
        stage_ms[name] = round(statistics.median(times), 3)
    objects = int(offsets[-1].item())
    rel = res["m0"]["levels"]["rel"]
    out = {"tool": "objects_bench", "methods": a.methods, "events": a.events, "frames": T, "hw": S, "levels": L, "connectivity": 8,
           "run_objects_from_host_ms": round(statistics.median(host), 2), "run_objects_from_device_ms": round(statistics.median(devt), 2),
           "spread_from_device_ms": [round(min(devt), 2), round(max(devt), 2)], "runs": a.reps,
           "updates_ms": round(statistics.median(s[0] for s in split), 2),
           "read_and_score_ms": round(statistics.median(s[1] for s in split), 2),
           "stage_ms": stage_ms, "objects_in_last_piece": objects,
           "S_median_rel_m0": rel["S_median"], "A_median_rel_m0": rel["A_median"], "L_median_rel_m0": rel["L_median"],
           "objects_mean_rel_m0": [rel["pred"]["objects_mean"], rel["truth"]["objects_mean"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
