"""Space-time ordinary kriging without a GPU: the numpy restatement (tests/stkriging_ref.py) pinned independently of itself (the
per-target primal system, the spatial restatement at T = 1, an exact model variogram, a brute-force pair count, a field on which
neighbouring frames must help), and the surface (registry, config, scripts)."""
import json
import os
import sys

import numpy as np
import pytest

import classical_ref as cr
import stkriging_ref as sr
from conftest import PKG

CONFIG_DIR = os.path.join(PKG, "p2igan_bench", "config")


def _sample16(seed=3, T=3, n=8, flat=None):
    """(xy, t, z) of a 16 x 16, T-frame sample with n gauges per frame at sites drawn per frame."""
    rng = np.random.default_rng(seed)
    h = w = 16
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    masked, masks = np.zeros((T, 1, h, w), np.float32), np.zeros((T, 1, h, w), np.float32)
    for t in range(T):
        field = 0.5 + 0.3 * np.sin((yy + t) / 3.0) * np.cos((xx - 0.5 * t) / 4.0) + 0.05 * rng.standard_normal((h, w))
        masks[t, 0].ravel()[rng.permutation(h * w)[:n]] = 1.0
        masked[t, 0] = (field if flat is None else flat) * masks[t, 0]
    return sr.points(masked, masks), masked, masks


@pytest.mark.parametrize("kappa", [0.5, 2.0])
@pytest.mark.parametrize("model,params", [("exponential", (0.01, 0.8, 6.0)), ("spherical", (0.0, 1.3, 9.0))])
def test_dual_form_equals_the_primal_system(model, params, kappa):
    (xy, tt, z), masked, masks = _sample16()
    assert len(z) == 24 and list(np.bincount(tt)) == [8, 8, 8]
    p = params + (kappa,)
    dual = sr.krige_sample(xy, tt, z, 3, 16, 16, p, model)
    primal, lam = sr.krige_sample_primal(xy, tt, z, 3, 16, 16, p, model)
    assert np.abs(dual - primal).max() <= 1e-9
    assert np.abs(lam.sum(1) - 1.0).max() <= 1e-9                             # the implied weights sum to 1
    at = masks[:, 0] != 0
    assert np.abs(dual[at] - masked[:, 0][at]).max() <= 1e-9                  # exact at each gauge in its own frame
    (xy, tt, zc), _, _ = _sample16(flat=0.37)
    assert np.abs(sr.krige_sample(xy, tt, zc, 3, 16, 16, p, model) - np.float32(0.37)).max() <= 1e-9


@pytest.mark.parametrize("kappa", [0.25, 1.0, 7.0])
@pytest.mark.parametrize("model,params", [("exponential", (0.01, 0.8, 6.0)), ("spherical", (0.0, 1.3, 9.0))])
def test_one_frame_is_spatial_kriging(model, params, kappa):
    (xy, tt, z), _, _ = _sample16(seed=5, T=1, n=24)
    got = sr.krige_sample(xy, tt, z, 1, 16, 16, params + (kappa,), model)[0]
    assert np.abs(got - cr.krige_frame(xy, z, 16, 16, params, model)).max() <= 1e-12


def test_sample_rules_of_the_restatement():
    e = np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    assert not sr.krige_sample(*e, 3, 8, 8, (0.0, 1.0, 4.0, 1.0), "exponential").any()
    (xy, tt, z), _, _ = _sample16()
    out = sr.krige_sample(xy, tt, z, 3, 16, 16, None, "exponential")
    assert out.shape == (3, 16, 16) and np.abs(out - z.astype(np.float64).mean()).max() <= 1e-12


def _exact_bins(q, c, nugget, psill, model, lw, n_lags=16, nu=4):
    """Bins whose means lie exactly on the family's member (q, c)."""
    rng = np.random.default_rng(7)
    n = rng.integers(5, 60, size=(nu, n_lags)).astype(np.float64)
    hb = (np.arange(n_lags)[None, :] + rng.uniform(0.3, 0.7, size=(nu, n_lags))) * lw
    u = np.broadcast_to(np.arange(nu, dtype=np.float64)[:, None], hb.shape)
    gam = sr.model_gamma(hb, u, nugget, psill, sr.range_of(c, lw), sr.kappa_of(q), model)
    return n, gam * n, hb * n


@pytest.mark.parametrize("nugget", [0.0, 0.02])
@pytest.mark.parametrize("model,q,c", [("exponential", 8, 10), ("spherical", 3, 13), ("exponential", 12, 6), ("spherical", 10, 16)])
def test_fit_recovers_an_exact_model_variogram(model, q, c, nugget):
    lw = cr.lag_width(32, 32, 16)
    got = sr.fit_st(*_exact_bins(q, c, nugget, 0.7, model, lw), lw, model)
    assert got[:2] == (q, c)
    assert abs(got[2] - nugget) <= 1e-9 and abs(got[3] - 0.7) <= 1e-9
    assert got[4] == sr.range_of(c, lw) and got[5] == sr.kappa_of(q) and got[6] <= 1e-18


def test_fit_of_empty_or_flat_bins_is_degenerate():
    z = np.zeros((4, 16))
    assert sr.fit_st(z, z, z, 1.0, "exponential")[:2] == (-1, -1)
    n, _, sh = _exact_bins(6, 8, 0.0, 0.5, "spherical", 1.0)
    assert sr.fit_st(n, np.zeros_like(n), sh, 1.0, "spherical")[:2] == (-1, -1)           # zero variance


@pytest.mark.parametrize("model", cr.MODELS)
def test_no_temporal_lags_is_the_spatial_fit(model):
    (_, _, _), masked, masks = _sample16(seed=9, T=4, n=30)
    frames = [cr.gauges(masked[t, 0], masks[t, 0]) for t in range(4)]
    lw = cr.lag_width(16, 16, 16)
    want = cr.fit_bins(*cr.variogram_bins(frames, 16, 16, 16), lw, model)
    n, sg, sh = sr.st_bins(frames, 16, 16, 16, 0)
    assert n.shape == (1, 16)
    got = sr.fit_st(n, sg, sh, lw, model)
    assert got[0] == 0 and got[1] == want[0] and got[1] >= 0
    assert got[2:5] == want[1:4] and got[6] == want[4]
    n1, sg1, sh1 = sr.st_bins(frames[:1], 16, 16, 16, 3)                                   # T = 1 clips n_tlags to 0
    assert n1.shape == (1, 16) and sr.fit_st(n1, sg1, sh1, lw, model)[0] == 0


def test_bins_count_every_pair_once():
    (_, _, _), masked, masks = _sample16(seed=11, T=5, n=20)
    masks[2] = 0.0                                                                        # a frame without gauges
    masked[2] = 0.0
    frames = [cr.gauges(masked[t, 0], masks[t, 0]) for t in range(5)]
    n, sg, sh = sr.st_bins(frames, 16, 16, 16, 3)
    n0, sg0, sh0 = cr.variogram_bins(frames, 16, 16, 16)
    assert np.array_equal(n[0], n0) and np.array_equal(sg[0], sg0) and np.array_equal(sh[0], sh0)
    lw = cr.lag_width(16, 16, 16)
    for u in (1, 2, 3):
        cnt, tot = np.zeros(16), 0.0
        for t in range(5 - u):
            for (ya, xa), za in zip(*frames[t]):
                for (yb, xb), zb in zip(*frames[t + u]):
                    hh = np.sqrt(float((ya - yb) ** 2 + (xa - xb) ** 2))
                    if hh < 16 * lw:
                        cnt[min(int(np.floor(hh / lw)), 15)] += 1
                        tot += 0.5 * (float(za) - float(zb)) ** 2
        assert np.array_equal(n[u], cnt) and cnt.sum() > 0
        assert abs(sg[u].sum() - tot) <= 1e-12 * tot
    assert n[1, 0] > 0                                                                    # equal pixels of two frames are pairs


def advecting_case(seed=0, T=16, n=79, h=32, w=32):
    """The field of DESIGN.md section 17: 0.5 + 0.3 sin((y + t) / 3) cos((x - t / 2) / 4), n fixed sites."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    truth = np.stack([0.5 + 0.3 * np.sin((yy + t) / 3.0) * np.cos((xx - 0.5 * t) / 4.0) for t in range(T)]).astype(np.float32)
    m = np.zeros(h * w, np.float32)
    m[np.random.default_rng(seed).permutation(h * w)[:n]] = 1.0
    masks = np.broadcast_to(m.reshape(1, 1, 1, h, w), (1, T, 1, h, w)).copy()
    truth = truth.reshape(1, T, 1, h, w)
    return truth, truth * masks, masks


def _rmse(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b) ** 2).mean()))


def test_neighbouring_frames_help_on_an_advecting_field():
    """Fixed spherical (0, 0.8, 12): with kappa = 2 px / frame the fp64 space-time RMSE is at most 0.9 x the per-frame kriging RMSE
    (0.0305 against 0.0439 with this draw of sites).  The fitted case is run and printed, not asserted: on this field the metric
    family's least-squares kappa is too small (exponential: (q, c) = (3, 11), kappa 0.354, RMSE 0.0915 against the fitted per-frame
    kriging's 0.0736), so the fit as defined does not beat per-frame kriging here (DESIGN.md section 17 records both models)."""
    truth, masked, masks = advecting_case()
    fixed = {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 12.0}
    per_frame = _rmse(cr.kriging(masked, masks, fixed)[0], truth)
    st = _rmse(sr.stkriging(masked, masks, dict(fixed, time_scale=2.0))[0], truth)
    print(f"fixed spherical: space-time RMSE {st:.4f}, per-frame RMSE {per_frame:.4f}, ratio {st / per_frame:.3f}")
    assert st <= 0.9 * per_frame
    for model in cr.MODELS:
        out, fits = sr.stkriging(masked, masks, {"model": model, "fit": True, "n_lags": 16, "n_tlags": 3})
        pf = _rmse(cr.kriging(masked, masks, {"model": model, "fit": True, "n_lags": 16})[0], truth)
        print(f"fitted {model}: (q, c) = {fits[0][:2]}, kappa {fits[0][5]:.3f}, range {fits[0][4]:.2f}, space-time RMSE "
              f"{_rmse(out, truth):.4f}, per-frame RMSE {pf:.4f}")
        assert fits[0][0] >= 0 and np.isfinite(out).all()


def test_registry_builds_the_space_time_generator():
    from p2igan_bench.models import CLASSICAL, SpaceTimeKrigingGenerator, build_discriminator, build_generator
    G = build_generator({"model": {"name": "stkriging"}})
    assert type(G) is SpaceTimeKrigingGenerator and CLASSICAL["stkriging"] is SpaceTimeKrigingGenerator
    assert len(G.state_dict()) == 0 and not list(G.parameters())
    assert G.max_points == 4096 and G.fit and G.n_lags == 16 and G.n_tlags == 3
    assert not hasattr(G, "forward_uq")
    with pytest.raises(NotImplementedError):
        build_discriminator({"model": {"name": "stkriging"}})
    ok = {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 1.0, "range": 5.0, "time_scale": 2.0}
    assert build_generator({"model": {"name": "stkriging", "variogram": ok}}).fixed == (0.0, 1.0, 5.0, 2.0)
    bad = [{k: v for k, v in ok.items() if k != "time_scale"}, dict(ok, time_scale=0.0), dict(ok, time_scale=-1.0), dict(ok, psill=0.0),
           {"model": "gaussian"}, {"fit": True, "n_tlags": 8}, {"fit": True, "n_tlags": -1}, {"fit": True, "n_lags": 33}]
    for vg in bad:
        with pytest.raises(ValueError):
            build_generator({"model": {"name": "stkriging", "variogram": vg}})
    with pytest.raises(ValueError, match="max_points"):
        build_generator({"model": {"name": "stkriging", "max_points": 4097}})


def test_config_loads_cpu_tensors_raise_and_scripts_refuse(tmp_path):
    import torch
    from p2igan_bench.evaluation import run_loo
    from p2igan_bench.models import build_generator
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train as train_script
    path = os.path.join(CONFIG_DIR, "stkriging_baseline.json")
    cfg = json.load(open(path))
    assert cfg["model"]["name"] == "stkriging"
    assert cfg["data"] == json.load(open(os.path.join(CONFIG_DIR, "kriging_baseline.json")))["data"]
    G = build_generator(cfg)
    assert G.max_points == 4096 and G.fit and G.variogram_model == 0 and (G.n_lags, G.n_tlags) == (16, 3)
    x = torch.zeros(1, 2, 1, 8, 8)
    with pytest.raises(RuntimeError, match="HIP path"):
        G(x, x)
    with pytest.raises(RuntimeError, match="nothing to train"):
        train_script.main(["--config", path])
    with pytest.raises(RuntimeError, match="leave-one-site-out"):
        run_loo(cfg, str(tmp_path / "loo"))
    with pytest.raises(RuntimeError, match="leave-one-site-out"):
        G.cross_validate(x, x)
