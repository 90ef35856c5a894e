"""An fp32 torch restatement of the STDK baseline's arithmetic (reference models/stdk.py:149-186), written from its description:
the [B*T*H*W, K_s + K_t + 79 T] feature rows [phi_s[p] | phi_t[t] | z[b]] are materialised and pushed through the four linear
layers with autograd.  Used by the GPU tests and tools/stdk_bench.py as the independent check of the fused kernels."""
import torch


def visible(masked, masks, k=79):
    """z [B, T * k]: per frame the observed pixels in raster order, then the unobserved ones, first k."""
    b, t = masked.shape[:2]
    x = masked.reshape(b, t, -1)
    m = masks.reshape(b, t, -1)
    order = torch.argsort((m == 0).to(torch.int64), dim=2, stable=True)[..., :k]
    return torch.gather(x, 2, order).reshape(b, t * k), order


def forward(params, phi_s, phi_t, masked, masks):
    """params: [w1, b1, w2, b2, w3, b3, w4, b4] (tensors, may require grad).  Returns (B, T, 1, H, W) in the parameters' dtype
    (fp32, or fp64 as an arbiter of rounding)."""
    b, t, _, h, w = masked.shape
    dt = params[0].dtype
    phi_s, phi_t = phi_s.to(dt), phi_t.to(dt)
    z, _ = visible(masked.to(dt), masks)
    hw, ks, kt = phi_s.shape[0], phi_s.shape[1], phi_t.shape[1]
    feats = torch.cat([phi_s.reshape(1, 1, hw, ks).expand(b, t, hw, ks), phi_t.reshape(1, t, 1, kt).expand(b, t, hw, kt),
                       z.reshape(b, 1, 1, -1).expand(b, t, hw, z.shape[1])], dim=3).reshape(b * t * hw, -1)
    w1, b1, w2, b2, w3, b3, w4, b4 = params
    y = torch.relu(feats @ w1.t() + b1)
    y = torch.relu(y @ w2.t() + b2)
    y = torch.relu(y @ w3.t() + b3)
    y = y @ w4.t() + b4
    return y.reshape(b, t, 1, h, w)
