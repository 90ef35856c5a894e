#!/usr/bin/env python3
"""Ensemble-verification kernels (csrc/eval_ens.hip) at 128 frames of 128 x 128, M = 32 f32 members read in place from one
(T, M, H, W) tensor, truth uint8, every pixel selected: ms of p2i_ens_points per box size (1, 4, 16) with its merge, of
p2i_ens_energy and of p2i_ens_variogram (16 offsets) from device events (median over a >= 0.5 s window after warm-up), the share of
the HBM peak (8 TB/s) that the box-1 per-point launch reaches counting every member and truth byte once plus the partial records it
writes, and the whole EnsembleEvaluator.update + compute.  The same scores as a torch-on-device restatement (torch.sort for the
per-point scores, torch.cdist for the energy score's distances, shifted differences for the variogram) are timed in the same
process, stage by stage.  No time target exists: the numbers are recorded (profiles/README.md).  Prints one JSON line.

usage: python tools/ens_bench.py [--frames 128] [--hw 128] [--members 32] [--no-torch]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "p2i-gan-benchmark_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from classical_bench import timed  # noqa: E402

PEAK_HBM = 8.0e12
BOXES = (1, 4, 16)


def torch_points(x, y, box, xq, edges):
    """The per-point sums in torch, fp64: x (T, M, H, W), y (T, H, W).  Returns the sums stacked, so that every stage stays alive."""
    T, M, H, W = x.shape
    if box > 1:
        x = torch.nn.functional.avg_pool2d(x.reshape(T * M, 1, H, W), box).reshape(T, M, H // box, W // box)
        y = torch.nn.functional.avg_pool2d(y.reshape(T, 1, H, W), box).reshape(T, H // box, W // box)
    xs = torch.sort(x, dim=1).values
    y1 = y[:, None]
    a = (xs - y1).abs().mean(1)
    wgt = (2.0 * torch.arange(M, device=x.device, dtype=x.dtype) - M + 1).view(1, M, 1, 1)
    S = 2.0 * (wgt * xs).sum(1)
    crps, fair = a - S / (2.0 * M * M), a - S / (2.0 * M * (M - 1))
    mean, var = xs.mean(1), xs.var(1, unbiased=True)
    e = mean - y
    b, k = (xs < y1).sum(1), (xs == y1).sum(1)
    q = torch.div(1 << 32, k + 1, rounding_mode="floor")
    diff = torch.zeros(M + 2, device=x.device, dtype=torch.int64)
    diff.index_add_(0, b.flatten(), q.flatten() + ((1 << 32) - q * (k + 1)).flatten())
    diff.index_add_(0, (b + k + 1).flatten(), -q.flatten())
    sb = torch.bucketize(var.sqrt(), edges, right=True)
    sb_n = torch.bincount(sb.flatten(), minlength=len(edges) + 1)
    sb_e2 = torch.zeros(len(edges) + 1, device=x.device, dtype=x.dtype).index_add_(0, sb.flatten(), (e * e).flatten())
    out = [crps.sum(), fair.sum(), e.sum(), e.abs().sum(), (e * e).sum(), var.sum(), diff.sum(), sb_n.sum(), sb_e2.sum()]
    for t in xq:
        c = (xs >= t).sum(1)
        o = y >= t
        p = c.to(x.dtype) / M
        out += [p.sum(), ((p - o.to(x.dtype)) ** 2).sum(), torch.bincount((c * 2 + o).flatten(), minlength=2 * (M + 1)).sum()]
    return torch.stack([v.to(torch.float64) for v in out])


def torch_energy(x, y):
    T, M, H, W = x.shape
    z = torch.cat([x.reshape(T, M, H * W), y.reshape(T, 1, H * W)], 1)
    d = torch.cdist(z, z, compute_mode="donot_use_mm_for_euclid_dist")
    return d[:, :M, M].mean(1) - d[:, :M, :M].sum((1, 2)) / (2.0 * M * M)


def torch_variogram(x, y, offsets):
    T, M, H, W = x.shape
    out = []
    for dy, dx in offsets:
        ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        gm = (x[:, :, ya:yb, xa:xb] - x[:, :, ya + dy:yb + dy, xa + dx:xb + dx]).abs().sqrt().mean(1)
        gy = (y[:, ya:yb, xa:xb] - y[:, ya + dy:yb + dy, xa + dx:xb + dx]).abs().sqrt()
        out.append(((gy - gm) ** 2).sum((1, 2)))
    return torch.stack(out, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    from p2igan_bench import _hip, ops
    from p2igan_bench.evaluation import DEFAULT_OFFSETS, DEFAULT_SIGMA_EDGES, DEFAULT_THRESHOLDS, EnsembleEvaluator, pixel_threshold
    _hip.load()
    dev = torch.device("cuda:0")
    T, S, M = a.frames, a.hw, a.members
    g = torch.Generator(device="cpu").manual_seed(7)
    torch.manual_seed(7)
    truth = (torch.rand(T, S, S, generator=g) < 0.6) * torch.clamp(torch.distributions.Gamma(0.6, 1.0 / 40.0).sample((T, S, S)), max=250.0)
    truth = truth.round()
    ens = torch.clamp(truth[:, None] + 3.0 + 12.0 * torch.randn(T, M, S, S, generator=g), min=0.0).to(dev)
    truth = truth.to(torch.uint8).to(dev)
    views, stride, origins = [ens[:, m] for m in range(M)], M * S * S, [(0, 0)] * M
    xq = tuple(pixel_threshold(q, True) for q in DEFAULT_THRESHOLDS)
    nf, ni = ops.ens_record(M, len(xq), len(DEFAULT_SIGMA_EDGES))
    res = {"workload": "ensemble_verification", "frames": T, "H": S, "W": S, "members": M, "member_dtype": "f32", "record_words": nf + ni}
    acc = torch.zeros(nf + ni, device=dev, dtype=torch.float64)
    for box in BOXES:
        nwg = -(-T * (S // box) ** 2 // ops.ENS_WG_PIXELS)
        part = torch.empty(nwg * (nf + ni), device=dev, dtype=torch.float64)
        res[f"points_box{box}_ms"] = timed(lambda: ops.ens_points(views, origins, stride, truth, (0, 0), S, S, box, None, xq,
                                                                  DEFAULT_SIGMA_EDGES, part))
        res[f"merge_box{box}_ms"] = timed(lambda: ops.prob_merge(part, nf, ni, acc))
        if box == 1:
            moved = ens.numel() * 4 + truth.numel() + part.numel() * 8
            res["points_box1_bytes"] = moved
            res["points_box1_share_of_hbm_peak"] = round(moved / (res["points_box1_ms"] * 1e-3) / PEAK_HBM, 4)
    en = torch.empty(T, 4, device=dev, dtype=torch.float64)
    va = torch.empty(T, len(DEFAULT_OFFSETS), 2, device=dev, dtype=torch.float64)
    res["energy_ms"] = timed(lambda: ops.ens_energy(views, origins, stride, truth, (0, 0), S, S, None, en))
    res["variogram_ms"] = timed(lambda: ops.ens_variogram(views, origins, stride, truth, (0, 0), S, S, None, DEFAULT_OFFSETS, va))

    def whole():
        ev = EnsembleEvaluator(S, device=dev)
        ev.update("e", ens, truth)
        return ev.compute()
    res["evaluator_update_compute_ms"] = timed(whole)
    if not a.no_torch:
        print(json.dumps(res), file=sys.stderr, flush=True)        # the kernels' figures, should the restatement fail
        x64, y64 = ens.double(), truth.double()
        edges = torch.tensor(DEFAULT_SIGMA_EDGES, device=dev, dtype=torch.float64)
        try:
            for box in BOXES:
                res[f"torch_points_box{box}_ms"] = timed(lambda: torch_points(x64, y64, box, xq, edges))
            res["torch_energy_ms"] = timed(lambda: torch_energy(x64, y64))
            res["torch_variogram_ms"] = timed(lambda: torch_variogram(x64, y64, DEFAULT_OFFSETS))
            es = torch_energy(x64, y64)
            res["torch_restatement_energy_rel_diff"] = float(((es - en[:, 1]).abs() / en[:, 1]).max())
            vs = torch_variogram(x64, y64, DEFAULT_OFFSETS)
            res["torch_restatement_variogram_rel_diff"] = float(((vs - va[..., 0]).abs() / va[..., 0]).max())
        except RuntimeError as e:
            res["torch_restatement_error"] = str(e).splitlines()[0][:200]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
