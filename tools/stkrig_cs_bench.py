#!/usr/bin/env python3
"""Space-time conditional-simulation kernels (csrc/stkrig_cs.hip) at B=8 samples of T=16 frames, 128x128, M=32 members, embed =
embed_time = 2 (torus 32 x 256 x 256): us of p2i_stcs_spectrum, of p2i_stcs_fields as a whole and stage by stage, and of
p2i_stcs_weights and p2i_stcs_predict at n = 1024 and n = 4096 points per sample (64 and 256 sites seen in every frame), from device
events (median over a >= 0.5 s window after warm-up).  Shares of the machine's peaks: stages 1 and 2 and the predictor against the f32
matrix peak (157.3 TF), counting 8 St Sy Sx W and 8 St H Sy W flop per member pair and 2 n T H W flop per member; stage 3 against the
HBM peak (8 TB/s), counting the reads of P2 (once per group of 16 frames) and the writes of the members.  The same work as a
torch-on-device restatement (torch.fft.fftn of the full torus with torch.randn noise, cholesky_solve of the member residuals, matmul
against a materialised c0) is timed in the same process.  No time target exists: the numbers are recorded (profiles/README.md).  Prints
one JSON line.

usage: python tools/stkrig_cs_bench.py [--b 8] [--t 16] [--hw 128] [--members 32] [--points 1024 4096] [--no-torch]
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
PEAK_HBM = 8.0e12
EMBED = EMBED_TIME = 2
KAPPA = 2.0
STAGE3_FRAMES = 16          # frames per pass of stage 3 over P2 (TG of csrc/stkrig_cs.hip)


def torch_members(amp, L, u, z, xy, tt, t, h, w, members, nugget, psill, rng, kappa):
    """The same members in batched torch ops, fp32: amp (B, St, Sy, Sx), L (B, N, N) lower factors, u (B, N), z (B, N), the points'
    pixels xy (N, 2) and frames tt (N,), shared by the samples.  Returns the three stages so that each can be timed on its own."""
    b, n = z.shape
    npairs = (members + 1) // 2
    cell = (tt * h + xy[:, 0]) * w + xy[:, 1]

    def fields():
        xi = torch.randn(b, npairs, *amp.shape[1:], dtype=torch.complex64, device=amp.device) * (2.0 ** 0.5)
        y = torch.fft.fftn(amp[:, None] * xi, dim=(2, 3, 4))[..., :t, :h, :w]
        return torch.stack([y.real, y.imag], 2).reshape(b, 2 * npairs, t * h * w)[:, :members]          # (B, M, T HW)

    def weights(U):
        r = (z[:, None, :] - U[..., cell]).transpose(1, 2).contiguous()                                 # (B, N, M)
        v = torch.cholesky_solve(r, L)
        mu = (u[:, None, :] @ r) / u.sum(1)[:, None, None]                                             # (B, 1, M)
        return v - mu * u[:, :, None], mu

    def predict(U, alpha, mu):
        yy, xx = torch.meshgrid(torch.arange(h, device=xy.device), torch.arange(w, device=xy.device), indexing="ij")
        d2 = torch.cdist(torch.stack([yy.flatten(), xx.flatten()], 1).float(), xy.float()) ** 2         # (HW, N)
        dt = torch.arange(t, device=xy.device)[:, None] - tt[None, :]                                   # (T, N)
        d = torch.sqrt(d2[None] + (kappa * kappa) * (dt * dt).float()[:, None, :]).reshape(t * h * w, n)
        c0 = psill * torch.exp(-d / rng) + nugget * (d == 0)
        return U + (mu + c0 @ alpha).transpose(1, 2)

    return fields, weights, predict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=16)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--points", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    from p2igan_bench import _hip, ops
    _hip.load()
    dev = torch.device("cuda:0")
    b, t, h, w, M = a.b, a.t, a.hw, a.hw, a.members
    npairs = (M + 1) // 2
    St, Sy, Sx = ops.stcs_torus(t, h, w, EMBED, EMBED_TIME)
    res = {"workload": "stkriging_conditional_simulation", "B": b, "T": t, "H": h, "W": w, "members": M, "embed": EMBED,
           "embed_time": EMBED_TIME, "points": {}}
    nugget, psill, rng = (FIXED[k] for k in ("nugget", "psill", "range"))
    params = torch.tensor((nugget, psill, rng, KAPPA), dtype=torch.float32).repeat(b, 1).to(dev)
    streams = torch.arange(b, dtype=torch.int64, device=dev)
    ens = torch.empty(b, t, M, h * w, device=dev)
    amp, clip = ops.stcs_spectrum(params, None, 0, t, h, w, EMBED, EMBED_TIME)
    res["clip_share"] = float(clip.max())
    res["spectrum_us"] = round(1e3 * timed(lambda: ops.stcs_spectrum(params, None, 0, t, h, w, EMBED, EMBED_TIME)), 1)

    def fields(stages=ops.STCS_STAGES_ALL):
        ops.stcs_fields(amp, streams, 1, M, t, h, w, EMBED, EMBED_TIME, ens, stages)

    res["fields_us"] = round(1e3 * timed(fields), 1)
    units = float(b) * npairs
    for bit, flop, nbytes in ((1, 8.0 * St * Sy * Sx * w, None), (2, 8.0 * St * h * Sy * w, None),
                              (4, None, 4.0 * h * w * (2 * St * -(-t // STAGE3_FRAMES) + 2 * t))):
        k = {1: "stage1", 2: "stage2", 4: "stage3"}[bit]
        res[f"fields_{k}_us"] = round(1e3 * timed(lambda: fields(bit)), 1)     # a stage on what the full call left in the workspaces
        if flop is not None:
            res[f"fields_{k}_fraction_of_f32_mfma_peak"] = round(units * flop / (res[f"fields_{k}_us"] * 1e-6) / PEAK_F32_MFMA, 4)
        else:
            res[f"fields_{k}_fraction_of_hbm_peak"] = round(units * nbytes / (res[f"fields_{k}_us"] * 1e-6) / PEAK_HBM, 4)
    for n in a.points:
        sites = n // t
        gen = torch.Generator().manual_seed(n)
        idx = torch.randperm(h * w, generator=gen)[:sites].sort().values
        masks = torch.zeros(b, t, h * w)
        masks[:, :, idx] = 1.0
        masked = (torch.rand(b, t, h * w, generator=gen) * masks).to(dev).view(b, t, h, w)
        masks = masks.to(dev).view(b, t, h, w)
        pix, z, info = ops.krig_compact(masked, masks, max(32, (sites + 31) // 32 * 32))
        np_ = max(32, (sites * t + 31) // 32 * 32)
        stpix, stt, stz, stinfo = ops.stkrig_gather(pix, z, info, b, t, np_)
        work = torch.empty(b * np_ * np_, device=dev)
        winv = torch.empty_like(work)
        status = torch.zeros(b, device=dev, dtype=torch.int32)
        alpha, mean = torch.empty(b, np_, device=dev), torch.empty(b, device=dev)
        ch = ops.KrigSystems(stpix, stz, stinfo, params, None, 0, 1, 1, np_, status).chunk(0, b)
        ops.stkrig_factor(ch, stt, work)
        sol = ops.krig_solve(ch, work, alpha, mean)
        ops.krig_invert(work, b, np_, winv)
        assert int(status.sum()) == 0
        fields()
        ca, cm = ops.stcs_weights(ch, stt, winv, sol, ens, M, t, h, w)
        o = {"points_per_sample": sites * t, "padded_system": np_}
        o["weights_us"] = round(1e3 * timed(lambda: ops.stcs_weights(ch, stt, winv, sol, ens, M, t, h, w)), 1)
        # in place: every timed call adds the conditioning once more to the same buffer, which costs what the first call costs
        o["predict_us"] = round(1e3 * timed(lambda: ops.stcs_predict(ch, stt, ca, cm, M, t, h, w, ens)), 1)
        o["predict_fraction_of_f32_mfma_peak"] = round(2.0 * sites * t * t * h * w * M * b / (o["predict_us"] * 1e-6) / PEAK_F32_MFMA, 4)
        if not a.no_torch:
            print(json.dumps({f"n{n}": o}), file=sys.stderr, flush=True)      # the kernels' figures, should the restatement fail
            nn = sites * t
            xy = torch.stack([idx // w, idx % w], 1).repeat(t, 1).to(dev)
            tt = torch.arange(t, device=dev).repeat_interleave(sites)
            L = torch.tril(work.view(b, np_, np_))[:, :nn, :nn].contiguous()
            tf, tw, tp = torch_members(amp, L, sol[:, 0, :nn].float(), stz[:, :nn].contiguous(), xy, tt, t, h, w, M, nugget, psill, rng, KAPPA)
            try:
                U = tf()
                al, mu = tw(U)
                full = tp(U, al, mu)
                o["torch_restatement_point_residual"] = float((full[..., (tt * h + xy[:, 0]) * w + xy[:, 1]] - stz[:, None, :nn]).abs().max())
                o["torch_fields_us"] = round(1e3 * timed(tf), 1)
                o["torch_weights_us"] = round(1e3 * timed(lambda: tw(U)), 1)
                o["torch_predict_us"] = round(1e3 * timed(lambda: tp(U, al, mu)), 1)
                del U, al, mu, full
            except torch.cuda.OutOfMemoryError as e:      # the restatement materialises c0; anything else ends the run
                o["torch_restatement_error"] = str(e).splitlines()[0][:200]
        del work, winv
        res["points"][f"n{n}"] = o
    print(json.dumps(res))


if __name__ == "__main__":
    main()
