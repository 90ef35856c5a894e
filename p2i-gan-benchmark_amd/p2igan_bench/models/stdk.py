"""STDK (spatio-temporal DeepKriging) baseline of the reference (models/stdk.py) on the HIP path.

The reference concatenates, for every (sample, frame, pixel) row, a spatial Wendland basis phi_s[p], a temporal one phi_t[t] and
the sample's 79 visible values per frame z[b], and runs a 100-100-100-1 MLP over that [B*T*H*W, K_s + K_t + 79 T] tensor
(stdk.py:149-186).  Its first layer splits exactly into a pixel, a frame and a sample term, so this build never materialises the
features: P = phi_s W1s^T and Q[b, t] = phi_t[t] W1t^T + z[b] W1z^T + b1 are small GEMMs, and h1 = relu(P[p] + Q[b, t]) feeds the
fused layers 2..4 (csrc/stdk.hip).

Parameters are the reference's four nn.Linear modules under _mlp.net (keys, shapes, construction and init RNG draws match seed for
seed); the bases are cached per (H, W, T, device) outside the state dict.  The 79 visible pixels of a frame are its observed pixels
in raster order, then its unobserved ones in raster order (the build's definition of the reference's topk(sorted=False) order)."""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn as nn

from .. import ops

NUM_BASIS = (10, 19, 37, 73)
K_VISIBLE = ops.STDK_K


def _subsample(k_full: int, m: int) -> torch.Tensor:
    """Indices round(linspace(0, k_full - 1, m)) in float32 with round-half-even (stdk.py:58-65, 229-243); all of them if m >= k_full."""
    if m >= k_full:
        return torch.arange(k_full)
    return torch.round(torch.linspace(0, k_full - 1, steps=m, dtype=torch.float32)).long().clamp(0, k_full - 1)


def space_knots(h: int, w: int, num_basis=NUM_BASIS) -> Tuple[torch.Tensor, torch.Tensor]:
    """Knots [K_s, 2] (y, x) and theta [K_s] of the multi-resolution 2-D basis (stdk.py:245-266): grid spacing
    max(1, round(min(h, w) / 4) >> level), theta = 4 * spacing."""
    base = max(1, int(round(min(h, w) / 4)))
    knots, theta = [], []
    for lvl, m in enumerate(num_basis):
        sp = max(1, base // (2 ** lvl))
        ys, xs = torch.arange(0, h, sp), torch.arange(0, w, sp)
        full = torch.stack(torch.meshgrid(ys, xs, indexing="ij"), dim=-1).reshape(-1, 2)
        sub = full[_subsample(full.shape[0], m)]
        knots.append(sub)
        theta.append(torch.full((sub.shape[0],), 4.0 * float(sp)))
    return torch.cat(knots).float(), torch.cat(theta)


def time_knots(t: int, num_basis=NUM_BASIS) -> Tuple[torch.Tensor, torch.Tensor]:
    """Knots [K_t, 2] as (t, 0) and theta [K_t] of the 1-D temporal basis (stdk.py:67-93): theta = 2.5 * spacing."""
    base = max(1, int(round(t / 4)))
    knots, theta = [], []
    for lvl, m in enumerate(num_basis):
        sp = max(1, base // (2 ** lvl))
        full = torch.arange(0, t, sp)
        sub = full[_subsample(full.shape[0], m)]
        knots.append(sub)
        theta.append(torch.full((sub.shape[0],), 2.5 * float(sp)))
    k = torch.cat(knots).float()
    return torch.stack([k, torch.zeros_like(k)], dim=1), torch.cat(theta)


class DKMLP(nn.Module):
    """Parameter holder with the reference's module tree (stdk.py:9-23): net.{0,2,4,6} are nn.Linear."""

    def __init__(self, feature_dim: int, hidden_dim: int = 100, out_dim: int = 1):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(feature_dim, hidden_dim), nn.ReLU(inplace=True), nn.Linear(hidden_dim, hidden_dim),
                                 nn.ReLU(inplace=True), nn.Linear(hidden_dim, hidden_dim), nn.ReLU(inplace=True),
                                 nn.Linear(hidden_dim, out_dim))


class _STDKFn(torch.autograd.Function):
    """y = MLP([phi_s | phi_t | z]) over every row, forward and backward on the library's STDK kernels."""

    @staticmethod
    def forward(ctx, z, phi_s, phi_t, B, T, w1, b1, w2, b2, w3, b3, w4, b4):
        P, Q = ops.stdk_layer1_fwd(phi_s, phi_t, z, w1, b1, B, T)
        y = ops.stdk_mlp_fwd(P, Q, w2, b2, w3, b3, w4, b4)
        ctx.save_for_backward(z, phi_s, phi_t, P, Q, w2, b2, w3, b3, w4)
        ctx.bt = (B, T)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, phi_s, phi_t, P, Q, w2, b2, w3, b3, w4 = ctx.saved_tensors
        B, T = ctx.bt
        dP, dQ, (dw2, db2, dw3, db3, dw4, db4) = ops.stdk_mlp_bwd(P, Q, w2, b2, w3, b3, w4, dy.contiguous())
        dw1, db1 = ops.stdk_layer1_bwd(phi_s, phi_t, z, dP, dQ, B, T)
        # (no gradient to the visible values: they come from the data, stdk.py:173-175 runs under no_grad topk + gather)
        return None, None, None, None, None, dw1, db1, dw2, db2, dw3, db3, dw4, db4


class STDKGenerator(nn.Module):
    """STDKGenerator(config, length=16, inference=False, init_weights=True) of the reference (stdk.py:96-186)."""

    def __init__(self, config, length=16, inference=False, init_weights=True, num_basis_space=NUM_BASIS, num_basis_time=NUM_BASIS):
        super().__init__()
        self.config = config
        self.keep = config.get("data_loader", {}).get("keep")
        self.length = length
        self.num_basis_space, self.num_basis_time = tuple(num_basis_space), tuple(num_basis_time)
        k_s = sum(self.num_basis_space)
        k_t = time_knots(length, self.num_basis_time)[0].shape[0]
        self._mlp = DKMLP(feature_dim=k_s + k_t + length * K_VISIBLE)
        self._cache: Dict = {}
        if init_weights:
            self.init_weights()

    def init_weights(self):
        """BaseNetwork.init_weights('kaiming') (modules/layer.py:20-40): kaiming_normal_(fan_in) weights, zero biases, module order."""
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.kaiming_normal_(m.weight.data, a=0, mode="fan_in")
                nn.init.constant_(m.bias.data, 0.0)

    def bases(self, h: int, w: int, t: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(phi_s [h*w, K_s], phi_t [t, K_t]) on `device`, computed once by p2i_stdk_basis from the host knot tables."""
        key = (h, w, t, str(device))
        if key not in self._cache:
            ks, ths = space_knots(h, w, self.num_basis_space)
            kt, tht = time_knots(t, self.num_basis_time)
            phi_s = ops.stdk_basis(ks.to(device), ths.to(device), h, w)
            phi_t = ops.stdk_basis(kt.to(device), tht.to(device), t, 1)
            self._cache[key] = (phi_s, phi_t)
        return self._cache[key]

    def forward(self, masked_frames, masks):
        b, t, c, h, w = masked_frames.size()
        if t != self.length:
            raise RuntimeError(f"STDKGenerator built for {self.length} frames, got {t}")
        if c != 1:
            raise RuntimeError("STDKGenerator takes one channel")
        if h * w < K_VISIBLE:
            raise ValueError(f"STDK needs at least {K_VISIBLE} pixels per frame (got {h}x{w})")
        if not masked_frames.is_cuda:
            raise RuntimeError("STDKGenerator runs on the HIP path only (CUDA tensors)")
        phi_s, phi_t = self.bases(h, w, t, masked_frames.device)
        x = masked_frames.reshape(b, t, h * w).contiguous().float()
        m = masks.reshape(b, t, h * w).contiguous().float()
        _, z = ops.stdk_select(x, m)
        net = self._mlp.net
        y = _STDKFn.apply(z.reshape(b, t * K_VISIBLE), phi_s, phi_t, b, t, net[0].weight, net[0].bias, net[2].weight, net[2].bias,
                          net[4].weight, net[4].bias, net[6].weight, net[6].bias)
        return y.view(b, t, 1, h, w)


InpaintGenerator = STDKGenerator
