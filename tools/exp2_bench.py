#!/usr/bin/env python3
"""exp2 render of one synthetic event at full size (30 frames x 128 x 128, uint8 truth and observation, 3 methods of f32
predictions, radar mode, 300 mask points) on the MI355X: the event end to end (compute_exp2's index panels from host arrays,
the canvases, the GIF file), the two kernels alone (HIP events around --launches launches, with the bytes they move), and the
numpy restatement of the index pass (tests/exp2_ref.py) on the host's CPU.  With --reference ROOT (a checkout of the reference;
CPU only, matplotlib and PIL needed) the reference's run_exp2 renders the same event for comparison, under the two shims of
tests/golden/make_golden_exp2.py; --no-gpu runs only the CPU parts.  Prints one JSON line and, with --out, writes it there too.

usage: python tools/exp2_bench.py [--frames 30] [--hw 128] [--zoom 2] [--reps 5] [--launches 50] [--reference ROOT] [--no-gpu] [--out F]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd"), os.path.join(ROOT, "tests")]


def reference_seconds(ref_root, preds, truth, obs, mask, hw):
    import types
    import numpy as np
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from p2igan_bench.data import zarr_lite
    if not hasattr(FigureCanvasAgg, "tostring_rgb"):
        FigureCanvasAgg.tostring_rgb = lambda self: np.asarray(self.buffer_rgba())[..., :3].tobytes()

    class Group:                                    # the golden script's stub, restated: that script runs on import
        def __init__(self, path):
            self.g = zarr_lite.Group(path, "r")

        def group_keys(self):
            return []

        def keys(self):
            return self.g.keys()

        def __contains__(self, k):
            return k in self.g.keys()

        def __getitem__(self, k):
            return self.g[k][:]
    sys.modules.setdefault("zarr", types.SimpleNamespace(open=lambda path, mode="r": Group(path)))
    sys.path.insert(0, ref_root)
    import experiments.exp2 as ref_exp2
    import exp2_ref
    with tempfile.TemporaryDirectory() as td:
        pp, tp, op = exp2_ref.write_zarrs(td, preds, truth, obs)
        os.makedirs(os.path.join(td, "out"))
        t0 = time.perf_counter()
        ref_exp2.run_exp2(pp, tp, op, mask, os.path.join(td, "out"), hw, None, 0.0, 0.0, 4, True, "radar")
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--zoom", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import exp2_ref
    from p2igan_bench.utils import seeded

    S, n = a.hw, a.frames
    truth = {"event_01": seeded.exp1_truth(800, n, S, S)}
    obs = {"event_01": seeded.exp1_truth(801, n, S, S)}
    preds = {m: {"event_01": seeded.exp1_pred(8000 + j, truth["event_01"], 8.0 + 10 * j, 0.02, 0.01)} for j, m in
             enumerate(("p2igan", "stdk", "idw"))}
    mask = np.zeros((S, S), bool)
    mask.reshape(-1)[np.random.default_rng(5).choice(S * S, size=min(300, S * S // 4), replace=False)] = True
    out = {"tool": "exp2_bench", "frames": n, "hw": S, "methods": 3, "zoom": a.zoom, "points": int(mask.sum())}

    t0 = time.perf_counter()
    ref = exp2_ref.exp2(preds, truth, obs, mask, S, "radar")
    out["cpu_index_restatement_s"] = round(time.perf_counter() - t0, 4)

    if not a.no_gpu:
        import torch
        from p2igan_bench import ops
        from p2igan_bench.evaluation import (EXP2_IDX_BG, EXP2_IDX_EDGE, compute_exp2, exp2_canvases, exp2_chrome, exp2_layout,
                                             paper_cmap, run_exp2, truth_lut)
        dev = torch.device("cuda")
        with tempfile.TemporaryDirectory() as td:
            def whole():
                t0 = time.perf_counter()
                run_exp2(preds, truth, obs, mask, td, S, None, 0.0, 0.0, 4, zoom=a.zoom)
                return time.perf_counter() - t0

            def index_only():
                t0 = time.perf_counter()
                r = compute_exp2(preds, truth, obs, mask, S)
                return time.perf_counter() - t0, r
            whole()                                             # warm-up (library load, allocator, font)
            out["event_end_to_end_s"] = round(statistics.median(whole() for _ in range(a.reps)), 4)
            out["gif_bytes"] = os.path.getsize(os.path.join(td, "comparison_event_01.gif"))
            runs = [index_only() for _ in range(a.reps)]
            out["index_panels_from_host_s"] = round(statistics.median(t for t, _ in runs), 4)
            res = runs[-1][1]
        ev = res.events[0]
        out["indices_equal_restatement"] = bool(np.array_equal(ev.panels, ref["events"][0]["panels"]))
        def canvases():
            t0 = time.perf_counter()
            c = exp2_canvases(ev, a.zoom)
            return time.perf_counter() - t0, c
        runs = [canvases() for _ in range(a.reps)]
        out["canvases_s"] = round(statistics.median(t for t, _ in runs), 4)
        canv = runs[-1][1]
        lay = exp2_layout(len(ev.labels), S, a.zoom)
        out["canvas"] = [int(canv.shape[1]), int(canv.shape[2])]

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.launches      # microseconds per launch

        bd = torch.from_numpy(paper_cmap()[0]).to(dev)
        lut = torch.from_numpy(truth_lut(True)).to(dev)
        idx = torch.empty(n, S, S, device=dev, dtype=torch.uint8)
        for name, src in (("u8", truth["event_01"][:, 0]), ("f32", preds["p2igan"]["event_01"][:, 0])):
            x = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
            us = timed(lambda: ops.exp2_index(x, (0, 0), S, n, bd, lut, True, idx))
            moved = n * S * S * (x.element_size() + 1)
            out[f"index_{name}_us"] = round(us, 2)
            out[f"index_{name}_gbps"] = round(moved / us / 1e3, 1)
        panels = torch.from_numpy(ev.panels).to(dev)
        chrome = torch.from_numpy(exp2_chrome(ev.labels, S, a.zoom)).to(dev)
        pts = torch.from_numpy(np.ascontiguousarray(ev.points, dtype=np.int32)).to(dev)
        cv = torch.empty(n, lay["height"], lay["pitch"], device=dev, dtype=torch.uint8)
        us = timed(lambda: ops.exp2_compose(panels, a.zoom, 1, pts, chrome, lay["oy"], lay["ox"], lay["step"], EXP2_IDX_BG, EXP2_IDX_EDGE, cv))
        moved = cv.numel() + panels.numel() + chrome.numel()
        out["compose_us"] = round(us, 2)
        out["compose_gbps"] = round(moved / us / 1e3, 1)
        out["compose_bytes"] = int(moved)
        if out.get("event_end_to_end_s"):
            out["index_speedup_vs_restatement"] = round(out["cpu_index_restatement_s"] / out["index_panels_from_host_s"], 1)
    if a.reference:
        out["reference_run_exp2_s"] = round(reference_seconds(a.reference, preds, truth, obs, mask, S), 2)
        if out.get("event_end_to_end_s"):
            out["speedup_vs_reference"] = round(out["reference_run_exp2_s"] / out["event_end_to_end_s"], 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
