#!/usr/bin/env python3
"""STDK baseline train step at the benchmark size (B=8, T=16, 128x128, sti block-10 mask) on the MI355X: step time from device
events over a >= 1 s window (median and spread of per-step times), FLOPs counted from shapes, and the fp32 torch-eager restatement
of the reference (tests/stdk_ref.py) timed in the same process for context.  Kernel times: run under
`rocprofv3 --kernel-trace --stats` separately (profiles/README.md).  Prints one JSON line.

usage: python tools/stdk_bench.py [--b 8] [--t 16] [--hw 128] [--no-eager]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

PEAK_F32 = 155e12        # measured f32-MFMA bound (MI355X_MICROARCH.md)


def timed(fn, min_s=1.0, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times, total = [], 0.0
    while total < min_s * 1e3 or len(times) < 5:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
        total += times[-1]
    return statistics.median(times), min(times), max(times), len(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=16)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    from p2igan_bench import _hip
    from p2igan_bench.engine import TrainEngine
    from p2igan_bench.models import build_generator
    from p2igan_bench.utils import seeded
    _hip.load()
    dev = torch.device("cuda:0")
    cfg = {"model": {"name": "stdk"}, "data": {"train": {"h": a.hw, "w": a.hw, "sample_length": a.t}},
           "loss": {"use_gan": 0, "k1_weight": 0.0005}, "train": {"optimizer": {"lr": 1e-4, "beta1": 0.0, "beta2": 0.99}}}
    G = build_generator(cfg).to(dev)
    G.load_state_dict(seeded.seeded_stdk_state(a.t), strict=True)
    frames, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(a.b, a.t, a.hw, a.hw, seeded.block_mask(a.hw, a.hw, 10))]
    eng = TrainEngine(G, None, cfg)
    med, lo, hi, n = timed(lambda: eng.train_step(frames, masked, masks))
    rows = a.b * a.t * a.hw * a.hw
    f = G.state_dict()["_mlp.net.0.weight"].shape[1]
    fwd = 2.0 * rows * (100 * 100 * 2 + 100)                       # fused layers 2..4
    bwd = 2.0 * fwd + 2.0 * rows * (100 * 100 * 2 + 100)           # recompute + data gradients + weight gradients
    res = {"workload": "stdk_train_step", "B": a.b, "T": a.t, "H": a.hw, "W": a.hw, "rows": rows, "step_ms_median": round(med, 3),
           "step_ms_min": round(lo, 3), "step_ms_max": round(hi, 3), "steps_timed": n, "mlp_fwd_gflop": round(fwd / 1e9, 1),
           "mlp_bwd_gflop": round(bwd / 1e9, 1), "f32_mfma_floor_ms": round((fwd + bwd) / PEAK_F32 * 1e3, 3),
           "step_share_of_f32_bound": round((fwd + bwd) / PEAK_F32 * 1e3 / med, 3)}
    if not a.no_eager:
        import stdk_ref
        params = [p.detach().clone().requires_grad_(True) for p in G.parameters()]
        phi_s, phi_t = G.bases(a.hw, a.hw, a.t, dev)
        opt = torch.optim.Adam(params, lr=1e-4, betas=(0.0, 0.99))

        def eager_step():
            y = stdk_ref.forward(params, phi_s, phi_t, masked, masks)
            loss = (y - frames).abs().mean()            # (an L1 stand-in for the loss: the eager side's time is the MLP's)
            opt.zero_grad()
            loss.backward()
            opt.step()
        emed, elo, ehi, en = timed(eager_step, warm=2)
        res.update(eager_ms_median=round(emed, 3), eager_ms_min=round(elo, 3), eager_ms_max=round(ehi, 3), eager_steps=en,
                   speedup_vs_eager=round(emed / med, 2), eager_layer1_gflop=round(6.0 * rows * f * 100 / 1e9, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
