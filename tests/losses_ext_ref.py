"""Torch restatement, in this build's own words, of the objectives of modules/losses.py that csrc/loss_ext.hip computes: for the GPU
box, where the reference is absent, and for timing an eager baseline (tools/loss_ext_bench.py).  Differentiable through torch's
autograd in any dtype; tests/test_losses_ext_cpu.py pins it to the genuine reference's float64 fixtures
(tests/golden/losses_ext.npz) to 1e-12.  Also the case tables of that fixture (tests/golden/make_golden_losses_ext.py)."""
import torch
import torch.nn.functional as F

# index -> ((B, T, H, W), beta, pool, border_ignore); the last map spans 3 x 3 of the kernel's 32 x 8 tiles, a multiple of neither
SHOCK_LOSS = [((1, 1, 3, 3), 30.0, 1, 0), ((1, 2, 7, 6), 30.0, 2, 0), ((2, 3, 9, 11), 30.0, 2, 0), ((2, 3, 9, 11), 0.02, 1, 2),
              ((2, 2, 13, 10), 1.0, 3, 1), ((1, 2, 6, 7), 0.02, 1, 2), ((1, 1, 17, 67), 30.0, 1, 0)]
SHOCK_MAP = [((2, 3, 9, 11), 30.0), ((1, 2, 6, 7), 30.0)]
TDM = [(1, 1, 1, 1), (1, 2, 5, 4), (2, 3, 9, 11), (2, 2, 13, 8)]
SOFTMAX = [(2, 3, 1, 4, 4), (1, 1, 33, 65), (2, 2, 1), (2, 3, 1, 4, 4)]       # the last one: inputs x 50
KL = [0, 1, 2]
TEMP = 0.1


def transform(x):
    return 0.036 * torch.pow(10.0, x * 255.0 / 3.0 * 0.0625)


def weighted_l1_distance(pred, true):
    w = 0.5 * torch.exp(5.14 * torch.clamp(true, max=0.7)) + 0.12
    return (w * (pred - true).abs()).mean()


def softmax_temperature(x, temperature):
    z = x.reshape(x.shape[0], x.shape[1], -1) / temperature
    z = z - z.max(dim=-1, keepdim=True).values.detach()
    e = z.exp()
    return (e / e.sum(dim=-1, keepdim=True)).reshape(x.shape)


def kl_divergence(p, q):
    return (torch.xlogy(q, q) - q * p.log()).sum() / p.shape[0]


def compute_forward_difference(x):
    return x[:, 1:] - x[:, :-1]


def spatial_pool(x):
    return F.max_pool2d(x, kernel_size=5, stride=4, padding=2)


def temporal_difference_matching_loss(pred_diff, true_diff, true, beta=1.0, eps=1e-6):
    d = spatial_pool(pred_diff) - spatial_pool(true_diff)
    return (d * d / (1.0 + beta * spatial_pool(true[:, :-1]) + eps)).mean()


def shock_map(x, beta=30.0, eps=1e-12):
    h, w = x.shape[-2:]
    p = F.pad(x.reshape(-1, 1, h, w), (1, 1, 1, 1), mode="reflect").reshape(x.shape[:-2] + (h + 2, w + 2))

    def s(dy, dx):           # the padded plane shifted by (dy, dx)
        return p[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    gx = ((s(-1, -1) - s(-1, 1)) + 2.0 * (s(0, -1) - s(0, 1)) + (s(1, -1) - s(1, 1))) / 8.0
    gy = ((s(-1, -1) - s(1, -1)) + 2.0 * (s(-1, 0) - s(1, 0)) + (s(-1, 1) - s(1, 1))) / 8.0
    lap = s(-1, 0) + s(0, -1) + s(0, 1) + s(1, 0) - 4.0 * s(0, 0)
    return torch.tanh(beta * lap) * torch.sqrt(gx * gx + gy * gy + eps)


def shock_map_loss(pred, true, beta=30.0, border_ignore=0, pool=2, eps=1e-12):
    if pool > 1:
        pred, true = F.max_pool2d(pred, pool, pool), F.max_pool2d(true, pool, pool)
    d = F.relu(shock_map(true, beta, eps).abs() - shock_map(pred, beta, eps).abs())
    m = border_ignore
    return d[..., m:d.shape[-2] - m, m:d.shape[-1] - m] if m > 0 else d


def k1_loss(pred, true, temp_alpha, k1_alpha):
    loss = weighted_l1_distance(pred, true)
    if k1_alpha > 0:
        loss = loss + k1_alpha * kl_divergence(softmax_temperature(compute_forward_difference(pred), TEMP),
                                               softmax_temperature(compute_forward_difference(true), TEMP))
    return loss


def reconstruction_loss(pred, true, k1_alpha):
    return weighted_l1_distance(pred, true) + k1_alpha * kl_divergence(
        softmax_temperature(compute_forward_difference(pred), TEMP), softmax_temperature(compute_forward_difference(true), TEMP))


def value_and_grad(fn, inputs, g, dtype, device="cpu"):
    """fn(*inputs) and d sum(fn * g) / d inputs[0], from numpy arrays, computed in `dtype` on `device`."""
    xs = [torch.as_tensor(a).to(device=device, dtype=dtype) for a in inputs]
    xs[0].requires_grad_(True)
    out = fn(*xs)
    (out * torch.as_tensor(g).to(device=device, dtype=dtype)).sum().backward()
    return out.detach(), xs[0].grad


def golden_cases(g):
    """Every case of tests/golden/losses_ext.npz as (tag, build function name, keyword arguments, input arrays)."""
    import numpy as np
    out = []
    for i, (_, beta, pool, border) in enumerate(SHOCK_LOSS):
        assert list(g[f"shock_loss/{i}/params"]) == [beta, pool, border]
        out.append((f"shock_loss/{i}", "shock_map_loss", dict(beta=beta, pool=pool, border_ignore=border),
                    [g[f"shock_loss/{i}/pred"], g[f"shock_loss/{i}/true"]]))
    for i, (_, beta) in enumerate(SHOCK_MAP):
        out.append((f"shock_map/{i}", "shock_map", dict(beta=beta), [g[f"shock_map/{i}/x"]]))
    for i in range(len(TDM)):
        out.append((f"tdm/{i}", "temporal_difference_matching_loss", {}, [g[f"tdm/{i}/{n}"] for n in ("pred_diff", "true_diff", "true")]))
        out.append((f"spool/{i}", "spatial_pool", {}, [g[f"spool/{i}/x"]]))
    for i in range(len(SOFTMAX)):
        out.append((f"softmax/{i}", "softmax_temperature", dict(temperature=TEMP), [g[f"softmax/{i}/x"]]))
    for i in KL:
        out.append((f"kl/{i}", "kl_divergence", {}, [g[f"softmax/{i}/out"].astype(np.float32), g[f"kl/{i}/q"]]))
    out.append(("fdiff/0", "compute_forward_difference", {}, [g["fdiff/0/x"]]))
    out.append(("transform/0", "transform", {}, [g["transform/0/x"]]))
    out.append(("wl1/0", "weighted_l1_distance", {}, [g["wl1/0/pred"], g["wl1/0/true"]]))
    return out

