#!/usr/bin/env python3
"""The loss family of csrc/loss_ext.hip at the benchmark size (B=8, T=16, 128x128) on the MI355X: each public function of
p2igan_bench.modules.losses, forward and forward+backward, from device events over a >= 1 s window (median of per-call times),
next to the fp32 torch-eager restatement of the reference (tests/losses_ext_ref.py) timed in the same process, call by call in turn.
Kernel times: run under `rocprofv3 --kernel-trace --stats` separately, with --no-eager (profiles/README.md).  Prints one JSON
line; profiles/README.md records a run.

usage: python tools/loss_ext_bench.py [--b 8] [--t 16] [--hw 128] [--min-s 1.0] [--no-eager]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def timed_interleaved(fns, min_s, warm=5):
    """Median device-event time (ms) of each callable of `fns`, the callables taking turns call by call so that all of them see
    the same clocks and the same neighbours on the host; until min_s of timed work per callable on average and >= 20 samples each."""
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    while sum(sum(t) for t in times.values()) < min_s * 1e3 * len(fns) or len(next(iter(times.values()))) < 20:
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: round(statistics.median(t), 4) for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=16)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--no-eager", action="store_true", help="time the HIP side only (for a kernel-trace run)")
    a = ap.parse_args()
    import losses_ext_ref as R
    from p2igan_bench import _hip
    from p2igan_bench.modules import losses as L
    _hip.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    shape = (a.b, a.t, a.hw, a.hw)
    pred, true = torch.rand(shape, generator=gen).to(dev), torch.rand(shape, generator=gen).to(dev)
    pd, td = (pred[:, 1:] - pred[:, :-1]).contiguous(), (true[:, 1:] - true[:, :-1]).contiguous()
    pp, qq = R.softmax_temperature(pd, 0.1), R.softmax_temperature(td, 0.1)
    # name -> (keyword arguments of both sides, differentiated input, the other inputs)
    cases = {
        "transform": ({}, pred, []),
        "weighted_l1_distance": ({}, pred, [true]),
        "softmax_temperature": (dict(temperature=0.1), pd, []),
        "kl_divergence": ({}, pp, [qq]),
        "compute_forward_difference": ({}, pred, []),
        "spatial_pool": ({}, pd, []),
        "temporal_difference_matching_loss": ({}, pd, [td, true]),
        "shock_map": ({}, pred, []),
        "shock_map_loss": ({}, pred, [true]),
        "shock_map_loss_metric_defaults": (dict(beta=0.02, border_ignore=2, pool=1), pred, [true]),
        "k1_loss": ({}, pred, [true, 1.0, 0.05]),
    }
    res = {"workload": "loss_ext", "B": a.b, "T": a.t, "H": a.hw, "W": a.hw, "unit": "ms", "functions": {}}
    for name, (kw, x, rest) in cases.items():
        fname = "shock_map_loss" if name.startswith("shock_map_loss") else name
        fns = {}
        for side, mod in (("hip", L),) + (() if a.no_eager else (("eager", R),)):
            f = getattr(mod, fname)
            xg = x.clone().requires_grad_(True)
            g = torch.ones_like(f(x, *rest, **kw))

            def fwd(f=f):
                with torch.no_grad():
                    f(x, *rest, **kw)

            def fwd_bwd(f=f, xg=xg, g=g):
                torch.autograd.grad(f(xg, *rest, **kw), xg, g)
            fns[f"{side}_fwd"], fns[f"{side}_fwd_bwd"] = fwd, fwd_bwd
        row = timed_interleaved(fns, a.min_s)
        if not a.no_eager:
            row["speedup_fwd"] = round(row["eager_fwd"] / row["hip_fwd"], 2)
            row["speedup_fwd_bwd"] = round(row["eager_fwd_bwd"] / row["hip_fwd_bwd"], 2)
        res["functions"][name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
