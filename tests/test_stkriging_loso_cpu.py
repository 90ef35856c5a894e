"""Leave-one-site-out cross-validation of space-time kriging without a GPU: the numpy restatement (tests/stkriging_loso_ref.py) pinned
against brute-force refits and against the spatial leave-one-out at T = 1, what the score is for (the advecting field of DESIGN.md
section 17), and the surface (methods, run_loso, refusals)."""
import json
import os

import numpy as np
import pytest

import classical_ref as cr
import krig_uq_ref as kr
import stkriging_loso_ref as lr
import stkriging_ref as sr
from conftest import PKG
from test_stkriging_cpu import advecting_case

CONFIG_DIR = os.path.join(PKG, "p2igan_bench", "config")


def _sites16(seed=4):
    """(masked, masks) (3, 1, 16, 16): 30 pixels of which 8 are gauges in all three frames, 10 in two and 12 in one."""
    rng = np.random.default_rng(seed)
    h = w = 16
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    masks = np.zeros((3, 1, h * w), np.float32)
    pool = rng.permutation(h * w)[:30]
    for k, p in enumerate(pool):
        frames = (0, 1, 2) if k < 8 else ((k % 3, (k + 1) % 3) if k < 18 else (k % 3,))
        for t in frames:
            masks[t, 0, p] = 1.0
    masks = masks.reshape(3, 1, h, w)
    field = np.stack([0.5 + 0.3 * np.sin((yy + t) / 3.0) * np.cos((xx - 0.5 * t) / 4.0) + 0.05 * rng.standard_normal((h, w))
                      for t in range(3)]).astype(np.float32)[:, None]
    return field * masks, masks


@pytest.mark.parametrize("nugget,kappa", [(0.0, 2.0), (0.05, 0.5)])
@pytest.mark.parametrize("model,psill,rng", [("exponential", 0.8, 6.0), ("spherical", 1.3, 9.0)])
def test_closed_form_equals_refits(model, psill, rng, nugget, kappa):
    masked, masks = _sites16()
    xy, tt, z = sr.points(masked, masks)
    site = lr.site_index(xy)
    sizes = np.bincount(site)
    assert len(z) == 8 * 3 + 10 * 2 + 12 and len(sizes) == 30 and sorted(set(sizes)) == [1, 2, 3]
    params = (nugget, psill, rng, kappa)
    pred, var = lr.block_loo(xy, tt, z, params, model, site)
    rp, rv = lr.block_refit(xy, tt, z, params, model, site)
    print(f"{model} nugget {nugget} kappa {kappa}: |pred - refit| {np.abs(pred - rp).max():.3e}  |var - refit| {np.abs(var - rv).max():.3e}")
    assert np.isfinite(pred).all() and np.isfinite(var).all() and (var > 0).all()
    assert np.abs(pred - rp).max() <= 1e-9 and np.abs(var - rv).max() <= 1e-9
    # leaving a whole site out is not leaving a point out: the point-wise form differs wherever a site has more than one point
    pp, _ = lr.block_loo(xy, tt, z, params, model, np.arange(len(z)))
    many = sizes[site] > 1
    assert np.abs(pp - pred)[many].max() > 1e-3 and np.abs(pp - pred)[~many].max() <= 1e-12


def test_rules_of_the_restatement():
    masked, masks = _sites16()
    params = (0.0, 0.8, 6.0, 2.0)
    one = masks * (np.arange(256).reshape(16, 16) == np.flatnonzero(masks.sum(0).ravel() == 3)[0])            # one site, in all frames
    xy, tt, z = sr.points(masked * one, one)
    assert len(z) >= 1 and len(np.unique(lr.site_index(xy))) == 1
    pred, var = lr.block_loo(xy, tt, z, params, "exponential", lr.site_index(xy))
    assert np.isnan(pred).all() and np.isnan(var).all()
    xy, tt, z = sr.points(masked, masks)
    pred, var = lr.block_loo(xy, tt, z, None, "exponential", lr.site_index(xy))                             # a degenerate fit
    assert np.isnan(pred).all() and np.isnan(var).all()
    flat = 0.25 * masks
    rows = lr.loso(np.stack([masked, flat, np.zeros_like(masked)]), np.stack([masks, masks, np.zeros_like(masks)]),
                   {"model": "exponential", "fit": True, "n_lags": 16, "n_tlags": 2})
    assert len(rows) == 9 and [len(r[0]) for r in rows[6:]] == [0, 0, 0]                                    # no gauges: nothing
    assert all(np.isfinite(r[1]).all() and np.isfinite(r[2]).all() for r in rows[:3])
    assert all(np.isnan(r[1]).all() and np.isnan(r[2]).all() and len(r[0]) for r in rows[3:6])              # constant values: degenerate
    assert np.array_equal(np.concatenate([r[3] for r in rows[:3]]), lr.site_index(xy))


@pytest.mark.parametrize("kappa", [0.25, 7.0])
@pytest.mark.parametrize("model,params", [("exponential", (0.01, 0.8, 6.0)), ("spherical", (0.0, 1.3, 9.0))])
def test_one_frame_is_the_spatial_leave_one_out(model, params, kappa):
    masked, masks = _sites16(seed=6)
    xy, tt, z = sr.points(masked[:1], masks[:1])
    pred, var = lr.block_loo(xy, tt, z, params + (kappa,), model, lr.site_index(xy))
    rp, rv = kr.loo_frame(xy, z, params, model)
    assert np.abs(pred - rp).max() <= 1e-12 and np.abs(var / rv - 1.0).max() <= 1e-12


def _rmse(rows):
    z, p = (np.concatenate([np.asarray(r[k], np.float64) for r in rows]) for k in (0, 1))
    return float(np.sqrt(((z - p) ** 2).mean()))


def test_site_score_orders_kappa_as_the_truth_does():
    """The advecting field of DESIGN.md section 17 with fixed spherical (0, 0.8, 12): the LOSO RMSE falls from the fitted kappa = 0.354
    to kappa = 2 and is there below per-frame kriging's LOO, as the RMSE against the gridded truth does; the point-wise LOO of the same
    systems is less than half of it, which is why it is no score of this method."""
    truth, masked, masks = advecting_case()
    fixed = {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 12.0}
    per_frame = _rmse(kr.kriging_uq(masked, masks, fixed)[2])
    table = {}
    print(f"per-frame kriging LOO RMSE {per_frame:.4f}")
    print("   kappa   LOSO RMSE   point-LOO RMSE   RMSE against the truth")
    for kappa in (0.354, 0.5, 1.0, 2.0, 4.0, 8.0, 32.0):
        vg = dict(fixed, time_scale=kappa)
        out = sr.stkriging(masked, masks, vg)[0]
        table[kappa] = (_rmse(lr.loso(masked, masks, vg)), _rmse(lr.loso(masked, masks, vg, pointwise=True)),
                        float(np.sqrt(((out.astype(np.float64) - truth) ** 2).mean())))
        print(f"{kappa:8.3f}   {table[kappa][0]:.4f}      {table[kappa][1]:.4f}           {table[kappa][2]:.4f}")
    assert table[2.0][0] < table[0.354][0] and table[2.0][0] < per_frame
    assert table[2.0][1] < 0.5 * table[2.0][0]
    assert abs(table[32.0][0] - per_frame) <= 0.02 * per_frame                 # kappa -> infinity: the frames decouple


def test_surface(tmp_path):
    import torch
    from p2igan_bench import evaluation, ops
    from p2igan_bench.evaluation import loso_lines, run_loso
    from p2igan_bench.models import CLASSICAL, build_generator
    from p2igan_bench.models.classical import ST_NO_LOO, LOOResult
    assert "leave-one-site-out" in ST_NO_LOO and "cross_validate_sites" in ST_NO_LOO
    x = torch.zeros(1, 2, 1, 8, 8)
    for name in sorted(CLASSICAL):
        G = build_generator({"model": {"name": name}})
        assert hasattr(G, "cross_validate_sites")
        with pytest.raises(RuntimeError, match="HIP path"):
            G.cross_validate_sites(x, x)
    G = build_generator({"model": {"name": "stkriging"}})
    assert not hasattr(G, "forward_uq")
    with pytest.raises(RuntimeError, match="leave-one-site-out"):
        G.cross_validate(x, x)
    assert LOOResult(*[None] * 6).site is None
    for fn in ("stkrig_gather_sites", "stkrig_site_gram", "stkrig_loso"):
        assert callable(getattr(ops, fn))
    assert evaluation.run_loso is run_loso and callable(loso_lines)
    # learnt models are refused before anything is built (no GPU, no data here)
    cfg = json.load(open(os.path.join(CONFIG_DIR, "p2igan_baseline.json")))
    with pytest.raises(RuntimeError, match="classical baselines"):
        run_loso(cfg, str(tmp_path / "loso"))
    cfg = json.load(open(os.path.join(CONFIG_DIR, "stkriging_baseline.json")))
    with pytest.raises(ValueError, match="at most 32 frames"):
        run_loso(cfg, str(tmp_path / "loso"), stride=33)
    assert not (tmp_path / "loso").exists()


def test_script_has_the_by_site_flag():
    import sys
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import crossvalidate as cv_script
    assert cv_script.parse_args(["--config", "c.json", "--output", "o"]).by_site is False
    assert cv_script.parse_args(["--config", "c.json", "--output", "o", "--by-site"]).by_site is True
