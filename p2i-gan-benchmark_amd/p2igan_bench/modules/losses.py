"""The reference's loss module (modules/losses.py) on HIP kernels, with its names, signatures and defaults.

ReconstructionLoss / gan_loss (losses.py:32-48, 232-253) are fused loss+gradient kernels (p2i_recloss, p2i_gan_loss).  The other
objectives -- transform, weighted L1, temperature softmax, KL, forward difference, spatial pool, temporal-difference matching,
shock map / shock loss, k1_loss (losses.py:51-189) -- are torch.autograd.Functions over the kernels of csrc/loss_ext.hip, so they
compose under autograd as the reference's do.  Gradients flow to the prediction-side argument only; a target-side tensor that
requires grad raises RuntimeError.  AdversarialLoss and the three loss-tracking metric classes (losses.py:192-226, 256-310)
keep the reference's constructor arguments; the metric classes are plain classes with the update / compute / reset / to
surface of metrics/metric.py (torchmetrics is not a dependency of this build)."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import ops

__all__ = [
    "ReconstructionLoss",
    "gan_loss",
    "transform",
    "weighted_l1_distance",
    "softmax_temperature",
    "kl_divergence",
    "compute_forward_difference",
    "spatial_pool",
    "temporal_difference_matching_loss",
    "shock_map",
    "shock_map_loss",
    "k1_loss",
    "AdversarialLoss",
    "WeightedL1Metric",
    "K1LossMetric",
    "ShockDifferenceMetric",
]


class DeviceScalar:
    """A loss component that stays on the device until someone asks for a float (the reference
    returns python floats here, which costs a host sync per step: train.py:245)."""

    def __init__(self, t: torch.Tensor):
        self._t = t

    def __float__(self):
        return float(self._t)

    def tensor(self):
        return self._t

    def __repr__(self):
        return f"DeviceScalar({float(self._t):.6g})"

    def __format__(self, spec):
        return format(float(self._t), spec)


class _RecLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, k1_alpha):
        out3, dpred = ops.recloss(pred.contiguous().float(), target.contiguous().float(), k1_alpha)
        ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(out3)
        return out3[2].clone(), out3

    @staticmethod
    def backward(ctx, gloss, _g3):
        (dpred,) = ctx.saved_tensors
        return dpred * gloss, None, None


class ReconstructionLoss:
    """Weighted L1 + k1_alpha * KL of temporal-difference softmaxes (losses.py:32-48)."""

    def __init__(self, k1_alpha: float = 0.0):
        self.k1_alpha = k1_alpha

    def __call__(self, prediction: torch.Tensor, target: torch.Tensor, mask: torch.Tensor | None = None):
        loss, out3 = _RecLossFn.apply(prediction, target, float(self.k1_alpha))
        return loss, {"pool": DeviceScalar(out3[0]), "reg": DeviceScalar(out3[1])}


class _GanDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits_real, logits_fake, loss_type, real_label, fake_label):
        loss, da, db = ops.gan_loss_d(logits_real.contiguous(), logits_fake.contiguous(), loss_type, real_label, fake_label)
        ctx.save_for_backward(da, db)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        da, db = ctx.saved_tensors
        return da * g, db * g, None, None, None


class _GanGFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, weight, loss_type, real_label):
        loss, da = ops.gan_loss_g(logits.contiguous(), weight, loss_type, real_label)
        ctx.save_for_backward(da)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (da,) = ctx.saved_tensors
        return da * g, None, None, None


def discriminator_loss(logits_real, logits_fake, loss_type="hinge", target_real_label=1.0, target_fake_label=0.0):
    """0.5 * (L(real) + L(fake)) of train.py:266-283 in one fused kernel."""
    return _GanDFn.apply(logits_real, logits_fake, loss_type, target_real_label, target_fake_label)


def generator_adv_loss(logits, weight, loss_type="hinge", target_real_label=1.0):
    """gan_loss(logits, True, is_disc=False) * adversarial_weight of train.py:301-308."""
    return _GanGFn.apply(logits, float(weight), loss_type, target_real_label)


def gan_loss(logits: torch.Tensor, target_is_real: bool, *, loss_type: str = "nsgan", is_disc: bool = False,
             target_real_label: float = 1.0, target_fake_label: float = 0.0) -> torch.Tensor:
    """Reference-compatible single-term helper (losses.py:232-253): hinge / lsgan / nsgan.  'nsgan' is nn.BCELoss on the RAW
    logits (losses.py:201-202) and, like torch, raises for any logit outside [0, 1]."""
    if loss_type not in ("hinge", "lsgan", "nsgan"):
        raise ValueError(f"Unsupported GAN loss type: {loss_type}")
    if loss_type == "hinge" and is_disc is None:
        raise ValueError("`is_disc` must be set when using hinge loss.")
    if loss_type == "hinge" and not is_disc:
        return generator_adv_loss(logits, 1.0, "hinge", target_real_label)
    if loss_type in ("lsgan", "nsgan"):
        label = target_real_label if target_is_real else target_fake_label
        return generator_adv_loss(logits, 1.0, loss_type, label)       # mean((x-label)^2) / mean(BCE(x, label))
    # hinge discriminator single term: relu(1 -/+ x).mean() == 2 * D-loss with the other side saturated
    big = torch.full_like(logits, 1e30)
    if target_is_real:
        return 2.0 * discriminator_loss(logits, -big, "hinge")
    return 2.0 * discriminator_loss(big, logits, "hinge")


# --------------------------------------------------------------------------- the reference's other objectives (csrc/loss_ext.hip)
def _in(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


def _wants_grad(t: torch.Tensor) -> bool:
    """False: nothing will be differentiated, the op is called directly (an autograd.Function costs several microseconds of host
    time per call, as much as these kernels run for at the benchmark's size)."""
    return t.requires_grad and torch.is_grad_enabled()


def _target(t: torch.Tensor, name: str, fn: str) -> torch.Tensor:
    if t.requires_grad:
        raise RuntimeError(f"{fn}: `{name}` is the target side and gets no gradient here; detach it")
    return t


class _TransformFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _in(x)
        ctx.save_for_backward(x)
        return ops.loss_transform_fwd(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.loss_transform_bwd(x, _in(g))


class _WL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, true):
        pred, true = _in(pred), _in(true)
        ctx.save_for_backward(pred, true)
        return ops.wl1_fwd(pred, true)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pred, true = ctx.saved_tensors
        return ops.wl1_bwd(pred, true, _in(g)), None


class _SoftmaxTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, temperature):
        y = ops.softmax_t_fwd(_in(x), temperature)
        ctx.save_for_backward(y)
        ctx.temperature = temperature
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return ops.softmax_t_bwd(y, _in(g), ctx.temperature), None


class _KLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, q):
        p, q = _in(p), _in(q)
        ctx.save_for_backward(p, q)
        return ops.kl_fwd(p, q)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, q = ctx.saved_tensors
        return ops.kl_bwd(p, q, _in(g)), None


class _FDiffFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.frames = x.shape[1] if x.dim() >= 2 else 0
        return ops.fdiff_fwd(_in(x))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ops.fdiff_bwd(_in(g), ctx.frames)


class _SPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        out, idx = ops.spool_fwd(_in(x), want_idx=ctx.needs_input_grad[0])
        ctx.in_shape = tuple(x.shape)
        if idx is not None:
            ctx.save_for_backward(idx)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return ops.spool_bwd(idx, _in(g), ctx.in_shape)


class _TDMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_diff, true_diff, true, beta, eps):
        out, coef, idx = ops.tdm_fwd(_in(pred_diff), _in(true_diff), _in(true), beta, eps, save=ctx.needs_input_grad[0])
        ctx.in_shape = tuple(pred_diff.shape)
        if idx is not None:
            ctx.save_for_backward(coef, idx)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        coef, idx = ctx.saved_tensors
        return ops.spool_bwd(idx, coef, ctx.in_shape, scale=_in(g)), None, None, None, None


class _ShockMapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, beta, eps):
        x = _in(x)
        ctx.save_for_backward(x)
        ctx.args = (beta, eps)
        return ops.shock_map_fwd(x, beta, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.shock_map_bwd(x, _in(g), *ctx.args), None, None


class _ShockLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, true, beta, pool, border, eps):
        pred, true = _in(pred), _in(true)
        ctx.save_for_backward(pred, true)                 # the inputs only: the backward pass recomputes both maps
        ctx.args = (beta, pool, border, eps)
        return ops.shock_loss_fwd(pred, true, beta, pool, border, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pred, true = ctx.saved_tensors
        return ops.shock_loss_bwd(pred, true, _in(g), *ctx.args), None, None, None, None, None


def transform(x: torch.Tensor) -> torch.Tensor:
    """Normalised rainfall -> mm scale, the legacy helper 0.036 * 10^((x*255/3)*0.0625) (losses.py:51-53; not metrics.transform)."""
    return _TransformFn.apply(x) if _wants_grad(x) else ops.loss_transform_fwd(_in(x))


def weighted_l1_distance(x_pred: torch.Tensor, x_true: torch.Tensor) -> torch.Tensor:
    """Weighted L1 distance (losses.py:56-65)."""
    x_true = _target(x_true, "x_true", "weighted_l1_distance")
    return _WL1Fn.apply(x_pred, x_true) if _wants_grad(x_pred) else ops.wl1_fwd(_in(x_pred), _in(x_true))


def softmax_temperature(tensor: torch.Tensor, temperature: float) -> torch.Tensor:
    """Softmax of tensor / temperature over everything after dim 1 (losses.py:68-73)."""
    return _SoftmaxTFn.apply(tensor, float(temperature)) if _wants_grad(tensor) else ops.softmax_t_fwd(_in(tensor), float(temperature))


def kl_divergence(p: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """F.kl_div(p.log(), q, 'batchmean') (losses.py:76-80)."""
    q = _target(q, "q", "kl_divergence")
    return _KLFn.apply(p, q) if _wants_grad(p) else ops.kl_fwd(_in(p), _in(q))


def compute_forward_difference(series: torch.Tensor) -> torch.Tensor:
    """series[:, 1:] - series[:, :-1] (losses.py:83-85)."""
    return _FDiffFn.apply(series) if _wants_grad(series) else ops.fdiff_fwd(_in(series))


def spatial_pool(x: torch.Tensor) -> torch.Tensor:
    """MaxPool2d(kernel_size=5, stride=4, padding=2) on the last two dims of a 3-D or 4-D tensor (losses.py:88-91)."""
    return _SPoolFn.apply(x) if _wants_grad(x) else ops.spool_fwd(_in(x), want_idx=False)[0]


def temporal_difference_matching_loss(pred_diff: torch.Tensor, true_diff: torch.Tensor, true: torch.Tensor, beta: float = 1.0,
                                      eps: float = 1e-6) -> torch.Tensor:
    """Weighted matching of pooled temporal gradients (losses.py:94-109), one fused kernel over the three pools."""
    fn = "temporal_difference_matching_loss"
    true_diff, true = _target(true_diff, "true_diff", fn), _target(true, "true", fn)
    if _wants_grad(pred_diff):
        return _TDMFn.apply(pred_diff, true_diff, true, float(beta), float(eps))
    return ops.tdm_fwd(_in(pred_diff), _in(true_diff), _in(true), float(beta), float(eps), save=False)[0]


def shock_map(x: torch.Tensor, beta: float = 30.0, eps: float = 1e-12) -> torch.Tensor:
    """tanh(beta * laplacian) * sqrt(gx^2 + gy^2 + eps) of a [B, T, H, W] tensor under reflect padding (losses.py:128-137)."""
    return _ShockMapFn.apply(x, float(beta), float(eps)) if _wants_grad(x) else ops.shock_map_fwd(_in(x), float(beta), float(eps))


def shock_map_loss(pred: torch.Tensor, true: torch.Tensor, beta: float = 30.0, tau: float = 25.0, border_ignore: int = 0,
                   pool: int = 2, eps: float = 1e-12) -> torch.Tensor:
    """relu(|shock(true)| - |shock(pred)|) after an optional max_pool2d(pool, pool), cropped by border_ignore: a TENSOR
    [B, T, H', W'] (losses.py:140-162).  `tau` is the reference's unused legacy argument."""
    del tau
    pool = int(pool) if pool > 1 else 1
    border = int(border_ignore) if border_ignore > 0 else 0
    true = _target(true, "true", "shock_map_loss")
    if _wants_grad(pred):
        return _ShockLossFn.apply(pred, true, float(beta), pool, border, float(eps))
    return ops.shock_loss_fwd(_in(pred), _in(true), float(beta), pool, border, float(eps))


def k1_loss(pred: torch.Tensor, true: torch.Tensor, temp_alpha: float, k1_alpha: float) -> torch.Tensor:
    """pool + k1_alpha * reg (losses.py:165-189), with reg only when k1_alpha > 0.  The reference's result never includes its shock
    term: it computes that term only when temp_alpha == 0 and then multiplies it by temp_alpha, so no shock pass is run here and
    `temp_alpha` does not change the value.  k1_loss(p, t, a, k) equals ReconstructionLoss(k)'s loss for k > 0 and
    weighted_l1_distance for k <= 0."""
    del temp_alpha
    _target(true, "true", "k1_loss")
    if k1_alpha > 0:
        return _RecLossFn.apply(pred, true, float(k1_alpha))[0]
    return weighted_l1_distance(pred, true)


class AdversarialLoss(nn.Module):
    """Multi-mode adversarial loss (losses.py:192-226): a module around gan_loss with the reference's two label buffers."""

    def __init__(self, loss_type: str = "nsgan", target_real_label: float = 1.0, target_fake_label: float = 0.0):
        super().__init__()
        if loss_type not in ("nsgan", "lsgan", "hinge"):
            raise ValueError(f"Unsupported GAN loss type: {loss_type}")
        self.loss_type = loss_type
        self.register_buffer("real_label", torch.tensor(target_real_label))
        self.register_buffer("fake_label", torch.tensor(target_fake_label))
        self._labels = (float(target_real_label), float(target_fake_label))      # host copies: no sync per call

    def forward(self, outputs: torch.Tensor, is_real: bool, is_disc: bool | None = None) -> torch.Tensor:
        if self.loss_type == "hinge" and is_disc is None:
            raise ValueError("`is_disc` must be set when using hinge loss.")
        return gan_loss(outputs, is_real, loss_type=self.loss_type, is_disc=bool(is_disc), target_real_label=self._labels[0],
                        target_fake_label=self._labels[1])


class _BaseLossMetric:
    """Running mean of a loss (losses.py:256-269): two device scalars, read back by nobody before compute()."""

    def __init__(self):
        self.device = None
        self.loss_sum = None
        self.n_obs = None

    def to(self, device):
        self.device = torch.device(device)
        self.reset()
        return self

    def reset(self):
        if self.device is not None:
            self.loss_sum = torch.zeros(1, device=self.device)
            self.n_obs = torch.zeros(1, device=self.device)
            self._one = torch.ones(1, device=self.device)

    def _accumulate(self, loss: torch.Tensor) -> None:
        if self.loss_sum is None or self.loss_sum.device != loss.device:
            self.to(loss.device)
        ops.axpy_(self.loss_sum, loss.detach().float().reshape(1))
        ops.axpy_(self.n_obs, self._one)

    def compute(self) -> torch.Tensor:
        return (self.loss_sum / torch.clamp(self.n_obs, min=1.0)).reshape(())


class WeightedL1Metric(_BaseLossMetric):
    """Running mean of weighted_l1_distance (losses.py:272-277)."""

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self._accumulate(weighted_l1_distance(preds.detach(), target.detach()))


class K1LossMetric(_BaseLossMetric):
    """Running mean of k1_loss (losses.py:280-290)."""

    def __init__(self, temp_alpha: float = 1.0, k1_alpha: float = 0.0):
        super().__init__()
        self.temp_alpha = temp_alpha
        self.k1_alpha = k1_alpha

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self._accumulate(k1_loss(preds.detach(), target.detach(), self.temp_alpha, self.k1_alpha))


class ShockDifferenceMetric(_BaseLossMetric):
    """Running mean of the mean shock-map discrepancy (losses.py:293-310)."""

    def __init__(self, beta: float = 0.02, border_ignore: int = 2, pool: int = 1):
        super().__init__()
        self.beta = beta
        self.border_ignore = border_ignore
        self.pool = pool

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        diff = shock_map_loss(preds.detach(), target.detach(), beta=self.beta, border_ignore=self.border_ignore, pool=self.pool)
        self._accumulate(diff.mean())
