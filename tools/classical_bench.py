#!/usr/bin/env python3
"""Classical baselines (ordinary kriging, all-gauge IDW) at the benchmark size (B=8, T=16, 128x128) on the MI355X, for a block-4 mask
(N = 1024 gauges per frame) and a block-10 mask (N = 169): ms per stage from device events (median over a >= 0.5 s window after
warm-up), the whole forward with one system per sample (the frames share their mask) and with one per frame, and a torch-on-device
restatement of the fixed-variogram kriging (cdist + torch.linalg.cholesky + cholesky_solve + matmul, fp32) where that runs.
No time target exists yet: the numbers are recorded (profiles/README.md).  Prints one JSON line.

usage: python tools/classical_bench.py [--b 8] [--t 16] [--hw 128] [--no-torch]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd")]

import torch  # noqa: E402

FIXED = {"model": "exponential", "fit": False, "nugget": 0.002, "psill": 0.05, "range": 6.0}


def timed(fn, min_s=0.5, warm=2):
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
    return round(statistics.median(times), 3)


def torch_kriging(masked, masks, nugget, psill, rng):
    """Fixed exponential variogram, frames sharing one mask per sample: the same dual form in batched torch ops, fp32."""
    b, t, _, h, w = masked.shape
    idx = masks[0, 0, 0].flatten().nonzero().squeeze(1)
    xy = torch.stack([idx // w, idx % w], 1).float()
    z = masked.reshape(b, t, h * w)[:, :, idx]                                        # (B, T, N)
    K = psill * torch.exp(-torch.cdist(xy, xy) / rng) + nugget * torch.eye(len(idx), device=xy.device)
    L = torch.linalg.cholesky(K.expand(b, -1, -1).contiguous())                      # one system per sample, as the kernels factor
    rhs = torch.cat([torch.ones(b, 1, len(idx), device=xy.device), z], 1).transpose(1, 2)
    sol = torch.cholesky_solve(rhs, L)                                               # (B, N, T + 1)
    u, v = sol[:, :, :1], sol[:, :, 1:]
    m = v.sum(1, keepdim=True) / u.sum(1, keepdim=True)
    alpha = v - m * u
    yy, xx = torch.meshgrid(torch.arange(h, device=xy.device), torch.arange(w, device=xy.device), indexing="ij")
    px = torch.stack([yy.flatten(), xx.flatten()], 1).float()
    d = torch.cdist(px, xy)
    c0 = psill * torch.exp(-d / rng) + nugget * (d == 0)
    return (m + c0 @ alpha).transpose(1, 2).reshape(b, t, 1, h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=16)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    from p2igan_bench import _hip, ops
    from p2igan_bench.models import build_generator
    from p2igan_bench.utils import seeded
    _hip.load()
    dev = torch.device("cuda:0")
    res = {"workload": "classical_baselines", "B": a.b, "T": a.t, "H": a.hw, "W": a.hw, "masks": {}}
    for block in (4, 10):
        _, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(a.b, a.t, a.hw, a.hw, seeded.block_mask(a.hw, a.hw, block))]
        b, t, h, w = a.b, a.t, a.hw, a.hw
        f = b * t
        x, m = masked.reshape(b, t, h, w), masks.reshape(b, t, h, w)
        pix, z, info = ops.krig_compact(x, m, 1024)
        n = int(info[:f].max())
        np_ = max(32, (n + 31) // 32 * 32)
        lag = (min(h, w) / 2.0) / 16
        _, _, cand, params = ops.krig_variogram(pix, z, info, b, t, 16, lag, 0)
        out = {"gauges_per_frame": n, "padded_system": np_}
        out["compact_ms"] = timed(lambda: ops.krig_compact(x, m, 1024))
        out["variogram_bins_and_fit_ms"] = timed(lambda: ops.krig_variogram(pix, z, info, b, t, 16, lag, 0))
        alpha = torch.empty(f, 1024, device=dev)
        mean = torch.empty(f, device=dev)
        for label, r in (("shared", t), ("per_frame", 1)):
            nsys = f // r
            work = torch.empty(nsys * np_ * np_, device=dev)
            status = torch.zeros(nsys, device=dev, dtype=torch.int32)
            ch = ops.KrigSystems(pix, z, info, params, cand, 0, r, t, np_, status).chunk(0, nsys)
            out[f"factor_{label}_ms"] = timed(lambda: ops.krig_factor(ch, work))
            out[f"solve_{label}_ms"] = timed(lambda: ops.krig_solve(ch, work, alpha, mean))
            out[f"predict_{label}_ms"] = timed(lambda: ops.krig_predict(ch, alpha, mean, h, w))
            assert int(status.sum()) == 0
            del work
        out["idw_all_ms"] = timed(lambda: ops.idw_all(pix, z, info, h, w, 2.0))
        for label, model in (("kriging_fit_shared", {"name": "kriging"}), ("kriging_fit_per_frame", {"name": "kriging", "share_sets": False}),
                             ("kriging_fixed_shared", {"name": "kriging", "variogram": FIXED}), ("idw", {"name": "idw"})):
            G = build_generator({"model": model}).to(dev)
            out[f"forward_{label}_ms"] = timed(lambda: G(masked, masks))
        res["masks"][f"block{block}"] = out
    if not a.no_torch:
        print(json.dumps(res), file=sys.stderr, flush=True)       # the kernels' figures, should the restatement take the process down
        for block in (4, 10):
            out = res["masks"][f"block{block}"]
            _, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(a.b, a.t, a.hw, a.hw, seeded.block_mask(a.hw, a.hw, block))]
            try:
                ref = torch_kriging(masked, masks, FIXED["nugget"], FIXED["psill"], FIXED["range"])
                got = build_generator({"model": {"name": "kriging", "variogram": FIXED}}).to(dev)(masked, masks)
                out["torch_restatement_max_abs_diff"] = float((ref - got).abs().max())
                out["torch_restatement_ms"] = timed(lambda: torch_kriging(masked, masks, FIXED["nugget"], FIXED["psill"], FIXED["range"]))
            except RuntimeError as e:            # torch.linalg.cholesky needs a device LAPACK backend
                out["torch_restatement_ms"] = None
                out["torch_restatement_error"] = str(e).splitlines()[0][:200]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
