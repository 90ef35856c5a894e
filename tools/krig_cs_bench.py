#!/usr/bin/env python3
"""Conditional-simulation kernels (csrc/krig_cs.hip) at the classical bench's two regimes (B=8, T=16, 128x128, M=32 members; block-4
mask: N = 1024 gauges per frame, block-10 mask: N = 169), on the shared-set path (one system per sample, R = T) and on the per-frame
path (R = 1): us of p2i_krig_cs_spectrum, p2i_krig_cs_fields, p2i_krig_cs_weights and p2i_krig_cs_predict from device events (median
over a >= 0.5 s window after warm-up), and the two MFMA stages' fraction of the f32 matrix peak (157.3 TF), counting
8 Sy Sx W + 8 H Sy W flop per member pair for the fields and 2 N H W flop per member for the predictor.  The same work as a
torch-on-device restatement (torch.fft.fft2 of the full torus, cholesky_solve of the residuals, matmul against a materialised c0) is
timed in the same process.  No time target exists: the numbers are recorded (profiles/README.md).  Prints one JSON line.

usage: python tools/krig_cs_bench.py [--b 8] [--t 16] [--hw 128] [--members 32] [--no-torch]
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
EMBED = 2


def torch_members(amp, L, u, z, xy, h, w, members, nugget, psill, rng):
    """The same members in batched torch ops, fp32, for samples that share their gauge set: amp (B, Sy, Sx), L (B, N, N) lower
    factors, u (B, N), z (B, T, N), xy (N, 2).  Returns the three stages' outputs so that each can be timed on its own."""
    b, t, n = z.shape
    npairs = (members + 1) // 2

    def fields():
        xi = torch.randn(b, t, npairs, *amp.shape[1:], dtype=torch.complex64, device=amp.device) * (2.0 ** 0.5)
        y = torch.fft.fft2(amp[:, None, None] * xi)[..., :h, :w]
        return torch.stack([y.real, y.imag], 3).reshape(b, t, 2 * npairs, h * w)[:, :, :members]

    def weights(U):
        r = z[:, :, None, :] - U[..., xy[:, 0] * w + xy[:, 1]]                                     # (B, T, M, N)
        v = torch.cholesky_solve(r.reshape(b, t * members, n).transpose(1, 2), L)                   # (B, N, T M)
        mu = (u[:, None, :] @ r.reshape(b, t * members, n).transpose(1, 2)) / u.sum(1)[:, None, None]
        return v - mu * u[:, :, None], mu

    def predict(U, alpha, mu):
        yy, xx = torch.meshgrid(torch.arange(h, device=xy.device), torch.arange(w, device=xy.device), indexing="ij")
        d = torch.cdist(torch.stack([yy.flatten(), xx.flatten()], 1).float(), xy.float())           # (HW, N)
        c0 = psill * torch.exp(-d / rng) + nugget * (d == 0)
        return U + (mu + c0 @ alpha).transpose(1, 2).reshape(b, t, members, h * w)

    return fields, weights, predict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=16)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    from p2igan_bench import _hip, ops
    from p2igan_bench.utils import seeded
    _hip.load()
    dev = torch.device("cuda:0")
    b, t, h, w, M = a.b, a.t, a.hw, a.hw, a.members
    f, npairs = b * t, (a.members + 1) // 2
    Sy, Sx = ops.krig_cs_torus(h, w, EMBED)
    res = {"workload": "kriging_conditional_simulation", "B": b, "T": t, "H": h, "W": w, "members": M, "embed": EMBED, "masks": {}}
    params = torch.tensor(tuple(FIXED[k] for k in ("nugget", "psill", "range")) + (0.0,), dtype=torch.float32).repeat(b, 1).to(dev)
    streams = torch.arange(f, dtype=torch.int64, device=dev)
    ens = torch.empty(f, M, h * w, device=dev)
    amp, clip = ops.krig_cs_spectrum(params, None, 0, h, w, EMBED)
    res["clip_share"] = float(clip.max())
    res["spectrum_us"] = round(1e3 * timed(lambda: ops.krig_cs_spectrum(params, None, 0, h, w, EMBED)), 1)
    res["fields_us"] = round(1e3 * timed(lambda: ops.krig_cs_fields(amp, streams, 1, t, M, h, w, EMBED, ens)), 1)
    fields_flop = float(f) * npairs * (8.0 * Sy * Sx * w + 8.0 * h * Sy * w)
    res["fields_fraction_of_f32_mfma_peak"] = round(fields_flop / (res["fields_us"] * 1e-6) / PEAK_F32_MFMA, 4)
    for block in (4, 10):
        _, masked, masks = [x.to(dev) for x in seeded.synthetic_batch(b, t, h, w, seeded.block_mask(h, w, block))]
        pix, z, info = ops.krig_compact(masked.reshape(b, t, h, w), masks.reshape(b, t, h, w), 1024)
        n = int(info[:f].max())
        np_ = max(32, (n + 31) // 32 * 32)
        out = {"gauges_per_frame": n, "padded_system": np_}
        for path, r in (("shared", t), ("per_frame", 1)):
            nsys = f // r
            work = torch.empty(nsys * np_ * np_, device=dev)
            winv = torch.empty_like(work)
            status = torch.zeros(nsys, device=dev, dtype=torch.int32)
            alpha, mean = torch.empty(f, 1024, device=dev), torch.empty(f, device=dev)
            ch = ops.KrigSystems(pix, z, info, params, None, 0, r, t, np_, status).chunk(0, nsys)
            ops.krig_factor(ch, work)
            sol = ops.krig_solve(ch, work, alpha, mean)
            ops.krig_invert(work, nsys, np_, winv)
            assert int(status.sum()) == 0
            ops.krig_cs_fields(amp, streams, 1, t, M, h, w, EMBED, ens)
            ca, cm = ops.krig_cs_weights(ch, winv, sol, ens, M, h, w)
            o = {"systems": nsys}
            o["weights_us"] = round(1e3 * timed(lambda: ops.krig_cs_weights(ch, winv, sol, ens, M, h, w)), 1)
            # in place: every timed call adds the conditioning once more to the same buffer, which costs what the first call costs
            o["predict_us"] = round(1e3 * timed(lambda: ops.krig_cs_predict(ch, ca, cm, M, h, w, ens)), 1)
            o["predict_fraction_of_f32_mfma_peak"] = round(2.0 * n * h * w * M * f / (o["predict_us"] * 1e-6) / PEAK_F32_MFMA, 4)
            out[path] = o
            if path == "shared" and not a.no_torch:
                print(json.dumps({f"block{block}": out}), file=sys.stderr, flush=True)   # the kernels' figures, should the restatement fail
                idx = masks[0, 0, 0].flatten().nonzero().squeeze(1)
                xy = torch.stack([idx // w, idx % w], 1)
                L = torch.tril(work.view(nsys, np_, np_))[:, :n, :n].contiguous()
                u = sol[:, 0, :n].float()
                fields, weights, predict = torch_members(amp, L, u, z.view(b, t, -1)[:, :, :n].contiguous(), xy, h, w, M, FIXED["nugget"],
                                                         FIXED["psill"], FIXED["range"])
                try:
                    U = fields()
                    al, mu = weights(U)
                    full = predict(U, al, mu)
                    at = xy[:, 0] * w + xy[:, 1]
                    o["torch_restatement_gauge_residual"] = float((full[..., at] - z.view(b, t, 1, -1)[..., :n]).abs().max())
                    o["torch_fields_us"] = round(1e3 * timed(fields), 1)
                    o["torch_weights_us"] = round(1e3 * timed(lambda: weights(U)), 1)
                    o["torch_predict_us"] = round(1e3 * timed(lambda: predict(U, al, mu)), 1)
                except RuntimeError as e:
                    o["torch_restatement_error"] = str(e).splitlines()[0][:200]
            del work, winv
        res["masks"][f"block{block}"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
