"""The restatement behind the kriging variance and leave-one-out kernels (tests/krig_uq_ref.py) against first principles, fp64 numpy:
the L^-1 variance formula against the per-pixel primal system, Dubrule's closed-form LOO against N refits, the IDW LOO against a
refit with the gauge deleted, and the calibration of the LOO variance on fields drawn from the model's own covariance.  The package's
surface for these (methods, entry points, scripts) is checked for presence; the numbers on the device are tests/test_krig_uq_gpu.py's."""
import os

import numpy as np
import pytest
import scipy.linalg

import classical_ref as cr
import krig_uq_ref as kr
from conftest import PKG

H = W = 16
PARAMS = {("exponential", True): (0.01, 0.05, 6.0), ("exponential", False): (0.0, 0.05, 6.0),
          ("spherical", True): (0.005, 0.05, 10.0), ("spherical", False): (0.0, 0.05, 10.0)}


def _gauges(n, seed=3, h=H, w=W):
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.permutation(h * w)[:n])
    return np.stack([idx // w, idx % w], axis=1), rng.random(n).astype(np.float32)


@pytest.mark.parametrize("nugget", [True, False])
@pytest.mark.parametrize("model", cr.MODELS)
def test_variance_formula_equals_the_primal_system(model, nugget):
    xy, _ = _gauges(40)
    params = PARAMS[(model, nugget)]
    raw, top = kr.variance_frame(xy, H, W, params, model, clamp=False)
    ref = kr.variance_primal(xy, H, W, params, model)
    assert np.abs(raw - ref).max() <= 1e-9
    at = (xy[:, 0], xy[:, 1])
    assert np.abs(raw[at]).max() <= 1e-12                       # zero at the gauges
    assert (raw <= top + 1e-15).all()                           # never above c00 + (1 - u^T k)^2 / s
    var, _ = kr.variance_frame(xy, H, W, params, model)
    assert (var >= 0).all() and not var[at].any()


def test_variance_of_a_single_gauge():
    xy, _ = _gauges(1)
    params = PARAMS[("exponential", True)]
    var, _ = kr.variance_frame(xy, H, W, params, "exponential")
    c00 = params[0] + params[1]
    k = cr.covariance(cr.grid(H, W), xy, *params, "exponential", np.float64)[:, 0]
    ref = c00 - k * k / c00 + (1 - k / c00) ** 2 * c00
    ref[xy[0, 0] * W + xy[0, 1]] = 0.0
    assert np.abs(var.ravel() - ref).max() <= 1e-15


@pytest.mark.parametrize("model", cr.MODELS)
def test_loo_closed_form_equals_refits(model):
    xy, z = _gauges(40)
    params = PARAMS[(model, True)]
    pred, var = kr.loo_frame(xy, z, params, model)
    rpred, rvar = kr.loo_refit(xy, z, params, model)
    assert np.abs(pred - rpred).max() <= 1e-12
    assert np.abs(var - rvar).max() <= 1e-12


def test_loo_of_two_gauges_is_the_other_gauge():
    xy, z = _gauges(2)
    pred, _ = kr.loo_frame(xy, z, PARAMS[("exponential", True)], "exponential")
    assert np.abs(pred - z[::-1]).max() <= 1e-12


@pytest.mark.parametrize("power", [2.0, 1.5])
def test_idw_loo_equals_a_refit_without_the_gauge(power):
    xy, z = _gauges(40)
    pred = kr.idw_loo_frame(xy, z, power)
    masks = np.zeros((1, 1, 1, H, W), np.float32)
    masks[0, 0, 0, xy[:, 0], xy[:, 1]] = 1.0
    masked = np.zeros_like(masks)
    masked[0, 0, 0, xy[:, 0], xy[:, 1]] = z
    for i in range(len(z)):
        m, v = masks.copy(), masked.copy()
        m[0, 0, 0, xy[i, 0], xy[i, 1]] = 0.0
        v[0, 0, 0, xy[i, 0], xy[i, 1]] = 0.0
        assert abs(cr.idw(v, m, power)[0, 0, 0, xy[i, 0], xy[i, 1]] - pred[i]) <= 1e-12
    assert np.isnan(kr.idw_loo_frame(xy[:1], z[:1], power)).all()


def test_msdr_of_fields_drawn_from_the_model_is_one():
    """z = L xi has covariance K, so e_i^2 / sigma^2_-i has mean 1: MSDR over 200 draws at N = 64 lies in [0.8, 1.2]."""
    xy, _ = _gauges(64, seed=7)
    params = PARAMS[("exponential", True)]
    L = scipy.linalg.cholesky(cr.covariance(xy, xy, *params, "exponential", np.float64), lower=True)
    rng = np.random.default_rng(2024)
    zs, preds, vars_ = [], [], []
    for _ in range(200):
        z = L @ rng.standard_normal(64)
        pred, var = kr.loo_frame(xy, z, params, "exponential")
        zs.append(z), preds.append(pred), vars_.append(var)
    s = kr.scores(np.concatenate(zs), np.concatenate(preds), np.concatenate(vars_))
    print(f"MSDR {s['MSDR']:.4f} over n = {s['n']}")
    assert s["n"] == 200 * 64 and 0.8 <= s["MSDR"] <= 1.2


def test_the_surface_exists():
    from p2igan_bench import _hip, evaluation
    from p2igan_bench.models.classical import IDWGenerator, KrigingGenerator, LOOResult
    for name in ("p2i_krig_invert", "p2i_krig_variance", "p2i_krig_loo", "p2i_idw_loo", "p2i_loo_scores"):
        assert name in _hip.SIGNATURES
    assert callable(KrigingGenerator.forward_uq) and callable(KrigingGenerator.cross_validate) and callable(IDWGenerator.cross_validate)
    assert callable(LOOResult.scores) and callable(evaluation.run_loo)
    assert os.path.exists(os.path.join(PKG, "scripts", "crossvalidate.py"))


def test_run_loo_refuses_learnt_models_before_anything_is_built():
    from p2igan_bench.evaluation import run_loo
    with pytest.raises(RuntimeError, match="classical baselines"):
        run_loo({"model": {"name": "p2igan"}}, "unused")
