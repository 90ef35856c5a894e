#!/usr/bin/env python3
"""Generate tests/golden/losses_ext.npz by running the GENUINE reference's modules/losses.py on CPU.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_losses_ext.py
The reference is imported as-is; its one missing dependency (`torchmetrics`, the base class of the metric wrappers,
losses.py:10,256-310) is stubbed with an empty ``Metric`` class as in the other make_golden_*.py scripts.

For every case the fixture holds the seeded float32 inputs, the upstream gradient, and the reference's outputs and input
gradients computed in FLOAT64.  The reference is also run in float32 on the same inputs; a case is kept only when float32 and
float64 agree within 1e-5 of the float64 result's max-abs, values and gradients -- otherwise the case is re-seeded.  A relu /
abs / argmax kink that rounding could flip would show as such a disagreement, so no committed case sits on one.
The fixture holds data only (inputs, parameters, results)."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

tm = types.ModuleType("torchmetrics")


class _Metric(nn.Module):
    def __init__(self, *a, **k):
        super().__init__()

    def add_state(self, name, default, dist_reduce_fx=None):
        setattr(self, name, default)


tm.Metric = _Metric
sys.modules["torchmetrics"] = tm
sys.path.insert(0, "/root/reference")
import importlib.util  # noqa: E402

_spec = importlib.util.spec_from_file_location("ref_losses", "/root/reference/p2igan_bench/modules/losses.py")
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

OUT = os.path.dirname(os.path.abspath(__file__))
GATE = 1e-5

# (B, T, H, W), beta, pool, border_ignore  -- the last one spans 3 x 3 of the kernel's 32 x 8 tiles and is no multiple of either
SHOCK_LOSS = [((1, 1, 3, 3), 30.0, 1, 0), ((1, 2, 7, 6), 30.0, 2, 0), ((2, 3, 9, 11), 30.0, 2, 0), ((2, 3, 9, 11), 0.02, 1, 2),
              ((2, 2, 13, 10), 1.0, 3, 1), ((1, 2, 6, 7), 0.02, 1, 2), ((1, 1, 17, 67), 30.0, 1, 0)]
SHOCK_MAP = [((2, 3, 9, 11), 30.0), ((1, 2, 6, 7), 30.0)]
TDM = [(1, 1, 1, 1), (1, 2, 5, 4), (2, 3, 9, 11), (2, 2, 13, 8)]          # shapes of the differences; true has one more frame
SOFTMAX = [((2, 3, 1, 4, 4), 1.0), ((1, 1, 33, 65), 1.0), ((2, 2, 1), 1.0), ((2, 3, 1, 4, 4), 50.0)]    # shape, input scale
KL = [0, 1, 2]                                                            # the softmax cases KL runs on (not the x50 one)
TEMP = 0.1


def rng_for(tag, attempt):
    seed = int.from_bytes(tag.encode(), "little") % (2 ** 31) + 7919 * attempt
    return np.random.default_rng(seed)


def run(fn, inputs, g, dtype):
    """fn over `inputs` (the first one gets the gradient) in dtype; returns (value, gradient of sum(value * g))."""
    xs = [torch.from_numpy(a).to(dtype) for a in inputs]
    xs[0].requires_grad_(True)
    out = fn(*xs)
    (out * torch.from_numpy(g).to(dtype)).sum().backward()
    return out.detach().numpy(), xs[0].grad.numpy()


def close(a32, a64):
    return np.abs(a32.astype(np.float64) - a64).max() <= GATE * max(np.abs(a64).max(), 1e-30)


def case(res, tag, fn, make_inputs, names, out_shape):
    for attempt in range(50):
        rng = rng_for(tag, attempt)
        inputs = make_inputs(rng)
        g = rng.standard_normal(out_shape(inputs)).astype(np.float32)
        v64, d64 = run(fn, inputs, g, torch.float64)
        v32, d32 = run(fn, inputs, g, torch.float32)
        if close(v32, v64) and close(d32, d64):
            break
        print(f"{tag}: float32 and float64 disagree (attempt {attempt}), re-seeding")
    else:
        raise SystemExit(f"{tag}: no seed passed the float32 / float64 gate")
    for n, a in zip(names, inputs):
        res[f"{tag}/{n}"] = a
    res[f"{tag}/g"] = g
    res[f"{tag}/out"] = v64
    res[f"{tag}/grad"] = d64
    print(f"{tag}: attempt {attempt}, f32 vs f64 value {np.abs(v32 - v64).max() / max(np.abs(v64).max(), 1e-30):.2e} "
          f"grad {np.abs(d32 - d64).max() / max(np.abs(d64).max(), 1e-30):.2e}")


def uni(rng, shape):
    return rng.random(shape, dtype=np.float32)


def main():
    res = {}
    for i, (shape, beta, pool, border) in enumerate(SHOCK_LOSS):
        res[f"shock_loss/{i}/params"] = np.array([beta, pool, border], dtype=np.float64)
        hp, wp = (shape[2] // pool, shape[3] // pool) if pool > 1 else shape[2:]
        case(res, f"shock_loss/{i}", lambda p, t: ref.shock_map_loss(p, t, beta=beta, border_ignore=border, pool=pool),
             lambda rng: [uni(rng, shape), uni(rng, shape)], ["pred", "true"],
             lambda ins: (shape[0], shape[1], hp - 2 * border, wp - 2 * border))
    for i, (shape, beta) in enumerate(SHOCK_MAP):
        res[f"shock_map/{i}/params"] = np.array([beta], dtype=np.float64)
        case(res, f"shock_map/{i}", lambda x: ref.shock_map(x, beta), lambda rng: [uni(rng, shape)], ["x"], lambda ins: shape)
    for i, (b, t, h, w) in enumerate(TDM):
        # centred on zero (a zero-padded pool would give other maxima); true in (-0.5, 0.5) keeps the weight's denominator off 0
        def mk(rng):
            return [rng.standard_normal((b, t, h, w)).astype(np.float32), rng.standard_normal((b, t, h, w)).astype(np.float32),
                    (uni(rng, (b, t + 1, h, w)) - 0.5).astype(np.float32)]
        case(res, f"tdm/{i}", lambda pd, td, tr: ref.temporal_difference_matching_loss(pd, td, tr), mk,
             ["pred_diff", "true_diff", "true"], lambda ins: ())
        case(res, f"spool/{i}", ref.spatial_pool, lambda rng: [rng.standard_normal((b, t, h, w)).astype(np.float32)], ["x"],
             lambda ins: (b, t, (h - 1) // 4 + 1, (w - 1) // 4 + 1))
    for i, (shape, scale) in enumerate(SOFTMAX):
        case(res, f"softmax/{i}", lambda x: ref.softmax_temperature(x, TEMP),
             lambda rng: [(scale * 0.2 * rng.standard_normal(shape)).astype(np.float32)], ["x"], lambda ins: shape)
    for i in KL:
        shape = SOFTMAX[i][0]

        def mk(rng):
            q = ref.softmax_temperature(torch.from_numpy(0.2 * rng.standard_normal(shape)), TEMP).float().numpy()
            return [res[f"softmax/{i}/out"].astype(np.float32), q]
        case(res, f"kl/{i}", ref.kl_divergence, mk, ["p", "q"], lambda ins: ())
        del res[f"kl/{i}/p"]            # p is float32(softmax/<i>/out): derived by the tests, not stored twice
    shape = (2, 4, 3, 5)
    case(res, "fdiff/0", ref.compute_forward_difference, lambda rng: [rng.standard_normal(shape).astype(np.float32)], ["x"],
         lambda ins: (2, 3, 3, 5))
    case(res, "transform/0", ref.transform, lambda rng: [uni(rng, shape)], ["x"], lambda ins: shape)
    case(res, "wl1/0", ref.weighted_l1_distance, lambda rng: [uni(rng, shape), uni(rng, shape)], ["pred", "true"], lambda ins: ())
    path = os.path.join(OUT, "losses_ext.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, len(res), "arrays,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
