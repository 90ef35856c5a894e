#!/usr/bin/env python3
"""Kriging variance and leave-one-out kernels (csrc/krig_uq.hip) at the classical bench's two regimes (B=8, T=16, 128x128; block-4 mask:
N = 1024 gauges per frame, block-10 mask: N = 169; one system per sample): us of p2i_krig_invert, p2i_krig_variance and p2i_krig_loo
from device events (median over a >= 0.5 s window after warm-up), the variance kernel's fraction of the f32 matrix peak (157.3 TF,
counting N^2 HW flop per system), and a torch-on-device restatement of the same map measured in the same process
(torch.linalg.solve_triangular of the factor against the materialised c0 matrix, then the column norms).  No time target exists: the
numbers are recorded (profiles/README.md).  Prints one JSON line.

usage: python tools/krig_uq_bench.py [--b 8] [--t 16] [--hw 128] [--no-torch]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from classical_bench import FIXED, timed  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def torch_variance(L, u, xy, h, w, nugget, psill, rng):
    """The same map in batched torch ops, fp32: L (S, N, N) lower factors, u (S, N) = K^-1 1, xy (N, 2) the shared gauge set."""
    yy, xx = torch.meshgrid(torch.arange(h, device=xy.device), torch.arange(w, device=xy.device), indexing="ij")
    d = torch.cdist(xy, torch.stack([yy.flatten(), xx.flatten()], 1).float())                   # (N, HW)
    c0 = psill * torch.exp(-d / rng) + nugget * (d == 0)
    y = torch.linalg.solve_triangular(L, c0.expand(L.shape[0], -1, -1), upper=False)          # (S, N, HW) = L^-1 k(p)
    var = (psill + nugget) - (y * y).sum(1) + (1.0 - u @ c0) ** 2 / u.sum(1, keepdim=True)
    return torch.where((d == 0).any(0), torch.zeros_like(var), var.clamp(min=0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=16)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    from p2igan_bench import _hip, ops
    from p2igan_bench.utils import seeded
    _hip.load()
    dev = torch.device("cuda:0")
    b, t, h, w = a.b, a.t, a.hw, a.hw
    f = b * t
    res = {"workload": "kriging_variance_and_loo", "B": b, "T": t, "H": h, "W": w, "masks": {}}
    params = torch.tensor(tuple(FIXED[k] for k in ("nugget", "psill", "range")) + (0.0,), dtype=torch.float32).repeat(b, 1).to(dev)
    for block in (4, 10):
        _, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(b, t, h, w, seeded.block_mask(h, w, block))]
        pix, z, info = ops.krig_compact(masked.reshape(b, t, h, w), masks.reshape(b, t, h, w), 1024)
        n = int(info[:f].max())
        np_ = max(32, (n + 31) // 32 * 32)
        work = torch.empty(b * np_ * np_, device=dev)
        winv = torch.empty_like(work)
        status = torch.zeros(b, device=dev, dtype=torch.int32)
        alpha, mean = torch.empty(f, 1024, device=dev), torch.empty(f, device=dev)
        var = torch.empty(f, h * w, device=dev)
        pred, lvar = torch.empty_like(z), torch.empty_like(z)
        ch = ops.KrigSystems(pix, z, info, params, None, 0, t, t, np_, status).chunk(0, b)
        ops.krig_factor(ch, work)
        sol = ops.krig_solve(ch, work, alpha, mean)
        assert int(status.sum()) == 0
        out = {"gauges_per_frame": n, "padded_system": np_, "systems": b}
        out["invert_us"] = round(1e3 * timed(lambda: ops.krig_invert(work, b, np_, winv)), 1)
        out["variance_us"] = round(1e3 * timed(lambda: ops.krig_variance(ch, winv, sol, h, w, var)), 1)
        out["loo_us"] = round(1e3 * timed(lambda: ops.krig_loo(ch, winv, sol, alpha, pred, lvar)), 1)
        out["variance_fraction_of_f32_mfma_peak"] = round(float(n) * n * h * w * b / (out["variance_us"] * 1e-6) / PEAK_F32_MFMA, 4)
        if not a.no_torch:
            print(json.dumps({f"block{block}": out}), file=sys.stderr, flush=True)   # the kernels' figures, should the restatement fail
            idx = masks[0, 0, 0].flatten().nonzero().squeeze(1)
            xy = torch.stack([idx // w, idx % w], 1).float()
            L = torch.tril(work.view(b, np_, np_))[:, :n, :n].contiguous()
            u = sol[:, 0, :n].float()
            try:
                ref = torch_variance(L, u, xy, h, w, FIXED["nugget"], FIXED["psill"], FIXED["range"])
                out["torch_restatement_max_abs_diff_of_c00"] = float((ref - var.view(b, t, h * w)[:, 0]).abs().max()) / (FIXED["nugget"] + FIXED["psill"])
                out["torch_restatement_us"] = round(1e3 * timed(lambda: torch_variance(L, u, xy, h, w, FIXED["nugget"], FIXED["psill"], FIXED["range"])), 1)
            except RuntimeError as e:
                out["torch_restatement_us"] = None
                out["torch_restatement_error"] = str(e).splitlines()[0][:200]
        res["masks"][f"block{block}"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
