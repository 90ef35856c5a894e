"""Classical baselines without a GPU: the registry and script surface, and the numpy restatement (tests/classical_ref.py) pinned
independently of itself -- its dual-form prediction against the primal ordinary-kriging system, its fit against an exact model."""
import json
import os
import sys

import numpy as np
import pytest

import classical_ref as cr
from conftest import PKG

CONFIG_DIR = os.path.join(PKG, "p2igan_bench", "config")


def test_registry_builds_the_two_parameter_free_generators():
    from p2igan_bench.models import build_discriminator, build_generator
    from p2igan_bench.models.classical import IDWGenerator, KrigingGenerator
    for name, cls in (("kriging", KrigingGenerator), ("idw", IDWGenerator)):
        G = build_generator({"model": {"name": name}})
        assert type(G) is cls
        assert len(G.state_dict()) == 0 and not list(G.parameters())
        with pytest.raises(NotImplementedError):
            build_discriminator({"model": {"name": name}})
    for name in ("dk", "simple"):
        with pytest.raises(NotImplementedError):
            build_generator({"model": {"name": name}, "data": {"train": {"h": 32, "w": 32}}})
    with pytest.raises(ValueError):
        build_generator({"model": {"name": "kriging", "variogram": {"model": "gaussian"}}})
    with pytest.raises(ValueError):
        build_generator({"model": {"name": "kriging", "variogram": {"model": "spherical", "fit": False, "psill": 1.0}}})
    with pytest.raises(ValueError):
        build_generator({"model": {"name": "idw", "power": 0}})


def test_configs_load_cpu_tensors_raise_and_train_refuses(tmp_path):
    import torch
    from p2igan_bench.models import build_generator
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train as train_script
    stdk = json.load(open(os.path.join(CONFIG_DIR, "stdk_baseline.json")))
    x = torch.zeros(1, 2, 1, 8, 8)
    for name in ("kriging", "idw"):
        path = os.path.join(CONFIG_DIR, f"{name}_baseline.json")
        cfg = json.load(open(path))
        assert cfg["model"]["name"] == name and cfg["data"] == stdk["data"]
        G = build_generator(cfg)
        assert G.max_points == 1024
        with pytest.raises(RuntimeError, match="HIP path"):
            G(x, x)
        with pytest.raises(RuntimeError, match="nothing to train"):
            train_script.main(["--config", path])
    G = build_generator(json.load(open(os.path.join(CONFIG_DIR, "kriging_baseline.json"))))
    assert G.fit and G.n_lags == 16 and G.variogram_model == 0


def _case16(seed=3, n=24):
    rng = np.random.default_rng(seed)
    h = w = 16
    idx = rng.permutation(h * w)[:n]
    mask = np.zeros((h, w), np.float32)
    mask.ravel()[idx] = 1.0
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    field = (0.5 + 0.3 * np.sin(yy / 3.0) * np.cos(xx / 4.0) + 0.05 * rng.standard_normal((h, w))).astype(np.float32)
    return field, mask


@pytest.mark.parametrize("model,params", [("exponential", (0.01, 0.8, 6.0)), ("spherical", (0.0, 1.3, 9.0)),
                                          ("spherical", (0.05, 0.5, 4.0))])
def test_dual_form_equals_the_primal_system(model, params):
    field, mask = _case16()
    xy, z = cr.gauges(field * mask, mask)
    dual = cr.krige_frame(xy, z, 16, 16, params, model, np.float64)
    primal, lam = cr.krige_frame_primal(xy, z, 16, 16, params, model)
    assert np.abs(dual - primal).max() <= 1e-9
    assert np.abs(lam.sum(1) - 1.0).max() <= 1e-9                      # the implied weights sum to 1
    assert np.abs(dual[xy[:, 0], xy[:, 1]] - z).max() <= 1e-9          # exact at gauges
    const = cr.krige_frame(xy, np.full(len(z), 0.37, np.float32), 16, 16, params, model, np.float64)
    assert np.abs(const - np.float32(0.37)).max() <= 1e-9              # a constant field gives a constant


def test_frame_rules_of_the_restatement():
    field, mask = _case16()
    xy, z = cr.gauges(field * mask, mask)
    assert not cr.krige_frame(xy[:0], z[:0], 16, 16, (0.0, 1.0, 5.0), "exponential").any()
    one = cr.krige_frame(xy[:1], z[:1], 16, 16, (0.0, 1.0, 5.0), "exponential")
    assert np.abs(one - z[0]).max() <= 1e-12
    deg = cr.krige_frame(xy, z, 16, 16, None, "exponential")
    assert np.abs(deg - z.astype(np.float64).mean()).max() <= 1e-7
    m5 = np.broadcast_to(mask, (1, 1, 1, 16, 16))
    f5 = (field * mask).reshape(1, 1, 1, 16, 16)
    out = cr.idw(f5, m5, 2.0)[0, 0, 0]
    assert np.abs(out[xy[:, 0], xy[:, 1]] - z).max() == 0.0 and z.min() <= out.min() and out.max() <= z.max()
    assert not cr.idw(f5, np.zeros_like(m5), 2.0).any()
    assert np.abs(cr.gauge_mean_predictor(f5, m5) - z.astype(np.float64).mean()).max() <= 1e-12


@pytest.mark.parametrize("model", cr.MODELS)
@pytest.mark.parametrize("nugget", [0.0, 0.02])
def test_fit_recovers_an_exact_model_variogram(model, nugget):
    n_lags, lw, c_true, psill = 16, 1.0, 11, 0.7
    a = lw * 2.0 ** ((c_true - 6) / 3.0)
    hb = (np.arange(n_lags) + 0.5) * lw
    n = np.linspace(40.0, 400.0, n_lags).round()
    gam = nugget + psill * cr.g_of(hb / a, model)
    c, nug, ps, rng, sse, _ = cr.fit_bins(n, gam * n, hb * n, lw, model)
    assert c == c_true and abs(rng - a) <= 1e-12 * a
    assert abs(nug - nugget) <= 1e-9 and abs(ps - psill) <= 1e-9 and sse <= 1e-18
    assert cr.fit_bins(np.zeros(n_lags), np.zeros(n_lags), np.zeros(n_lags), lw, model)[0] == -1      # no non-empty bin
    assert cr.fit_bins(n, np.zeros(n_lags), hb * n, lw, model)[0] == -1                                # zero variance


def test_bins_count_every_pair_once():
    field, mask = _case16(n=20)
    xy, z = cr.gauges(field * mask, mask)
    n, sg, sh = cr.variogram_bins([(xy, z), (xy[:7], z[:7])], 16, 16, 8)
    lw = cr.lag_width(16, 16, 8)
    want = 0
    for pts in (xy, xy[:7]):
        d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
        want += int((np.triu(d < 8 * lw, 1)).sum())
    assert int(n.sum()) == want and (sg >= 0).all() and (sh[n > 0] / n[n > 0] < 8 * lw).all()
