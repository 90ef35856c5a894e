"""Moving-neighbourhood space-time kriging without a GPU: the numpy restatement (tests/lkriging_ref.py) pinned independently of
itself in fp64 (against the global space-time and the per-frame restatements where the neighbourhood is everything, against global
leave-one-site-out, by the textbook properties, and by a hand-written sort on a lattice full of exact ties), the surface (registry,
config, refusals), and what a neighbourhood costs in skill on the field of DESIGN.md section 17."""
import json
import os

import numpy as np
import pytest

import classical_ref as cr
import krig_uq_ref as ur
import lkriging_ref as lr
import stkriging_loso_ref as slr
import stkriging_ref as sr
from conftest import PKG
from test_stkriging_cpu import _sample16, advecting_case, _rmse

CONFIG_DIR = os.path.join(PKG, "p2igan_bench", "config")
CASES = [("exponential", (0.01, 0.8, 6.0)), ("spherical", (0.0, 1.3, 9.0))]


@pytest.mark.parametrize("kappa", [0.5, 2.0])
@pytest.mark.parametrize("model,params", CASES)
def test_whole_sample_neighbourhood_is_global_space_time_kriging(model, params, kappa):
    (xy, tt, z), masked, masks = _sample16()
    assert len(z) == 24
    p = params + (kappa,)
    want = sr.krige_sample(xy, tt, z, 3, 16, 16, p, model)
    for k, frames in ((24, 2), (64, 5)):
        got, var, _ = lr.krige_sample(xy, tt, z, 3, 16, 16, p, model, k, frames)
        assert np.abs(got.reshape(3, 16, 16) - want).max() <= 1e-9
        assert np.isfinite(var).all() and var.min() >= 0.0


@pytest.mark.parametrize("model,params", CASES)
def test_window_of_one_frame_is_per_frame_kriging_with_its_variance(model, params):
    (xy, tt, z), masked, masks = _sample16(seed=4, T=3, n=11)
    got, var, _ = lr.krige_sample(xy, tt, z, 3, 16, 16, params + (1.7,), model, 16, 0)
    for t in range(3):
        at = tt == t
        assert np.abs(got[t].reshape(16, 16) - cr.krige_frame(xy[at], z[at], 16, 16, params, model)).max() <= 1e-9
        assert np.abs(var[t].reshape(16, 16) - ur.variance_frame(xy[at], 16, 16, params, model)[0]).max() <= 1e-9


@pytest.mark.parametrize("model,params", CASES)
def test_loso_with_every_point_is_global_leave_one_site_out(model, params):
    rng = np.random.default_rng(8)
    T, h, w = 3, 16, 16
    m = np.zeros(h * w, np.float32)
    m[rng.permutation(h * w)[:9]] = 1.0
    masks = np.broadcast_to(m.reshape(1, 1, h, w), (T, 1, h, w)).copy()
    masks[1, 0].ravel()[np.flatnonzero(m)[0]] = 0.0                  # a site that misses a frame
    masked = (rng.random((T, 1, h, w)).astype(np.float32) + 0.2) * masks
    xy, tt, z = sr.points(masked, masks)
    p = params + (1.3,)
    site = slr.site_index(xy)
    want_p, want_v = slr.block_refit(xy, tt, z, p, model, site)
    got_p, got_v = lr.loso_sample(xy, tt, z, p, model, 64, T - 1)
    assert np.abs(got_p - want_p).max() <= 1e-9 and np.abs(got_v - want_v).max() <= 1e-9
    closed_p, closed_v = slr.block_loo(xy, tt, z, p, model, site)
    assert np.abs(got_p - closed_p).max() <= 1e-9 and np.abs(got_v - closed_v).max() <= 1e-9
    one_p, one_v = lr.loso_sample(xy[site == 0], tt[site == 0], z[site == 0], p, model, 8, T - 1)      # one site: nothing is left
    assert np.isnan(one_p).all() and np.isnan(one_v).all()


@pytest.mark.parametrize("model,params", CASES)
def test_textbook_properties(model, params):
    (xy, tt, z), masked, masks = _sample16(seed=6, T=4, n=12)
    p = params + (2.0,)
    px = cr.grid(16, 16)
    for t in (0, 3):
        sel = lr.select(px, t, xy, tt, 2.0, 7, 1)
        for q in range(0, 256, 5):
            s = sel[q]
            assert (s >= 0).all()
            pred, var, lam = lr.solve_target(px[q, 0], px[q, 1], t, xy[s], tt[s], z[s], p, model)
            assert abs(lam.sum() - 1.0) <= 1e-9
            flat, _, _ = lr.solve_target(px[q, 0], px[q, 1], t, xy[s], tt[s], np.full(len(s), 0.37, np.float32), p, model)
            assert abs(flat - np.float32(0.37)) <= 1e-9
    got, var, _ = lr.krige_sample(xy, tt, z, 4, 16, 16, p, model, 7, 1)
    at = (masks[:, 0] != 0).reshape(4, 256)
    assert np.abs(got[at] - masked[:, 0].reshape(4, 256)[at]).max() <= 1e-9          # a gauge is reproduced in its own frame
    assert var[at].max() <= 1e-12
    one, _, _ = lr.krige_sample(xy, tt, z, 4, 16, 16, p, model, 1, 1)                    # m = 1: lambda = 1, the nearest value
    sel1 = lr.select(px, 2, xy, tt, 2.0, 1, 1)[:, 0]
    assert np.abs(one[2] - z[sel1]).max() <= 1e-12
    _, _, lam = lr.solve_target(3, 3, 2, xy[sel1[:1]], tt[sel1[:1]], z[sel1[:1]], p, model)
    assert abs(lam[0] - 1.0) <= 1e-12


def lattice_case(T=5, h=16, w=16):
    """Gauges on the 4-spaced lattice of every frame; kappa = 2 makes every key an integer, with many exact ties."""
    masks = np.zeros((T, 1, h, w), np.float32)
    masks[:, 0, ::4, ::4] = 1.0
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    masked = np.stack([(0.3 + 0.02 * yy + 0.01 * xx + 0.05 * t)[None] for t in range(T)]).astype(np.float32) * masks
    return masked, masks


def hand_sorted(ty, tx, t, masks, k, frames, exclude_own=False):
    """The selection by a triple loop and Python's sort of integer tuples (kappa = 2): [(frame, y, x)] of the first k."""
    T, _, h, w = masks.shape
    found = []
    for tp in range(T):
        if abs(tp - t) > frames:
            continue
        for y in range(h):
            for x in range(w):
                if masks[tp, 0, y, x] != 0 and not (exclude_own and (y, x) == (ty, tx)):
                    found.append(((y - ty) ** 2 + (x - tx) ** 2 + 4 * (tp - t) ** 2, tp, y * w + x))
    return [(tp, r // w, r % w) for _, tp, r in sorted(found)[:k]]


def test_selection_on_a_lattice_of_ties_is_the_hand_written_sort():
    masked, masks = lattice_case()
    xy, tt, z = sr.points(masked, masks)
    T = masks.shape[0]
    for t, ty, tx, k, frames in ((0, 0, 0, 9, 2), (0, 6, 6, 12, 1), (2, 6, 6, 12, 2), (2, 8, 8, 7, 4), (4, 15, 15, 5, 1), (4, 2, 10, 20, 3),
                                 (3, 7, 9, 1, 0), (1, 10, 2, 16, 0), (4, 6, 6, 64, 4)):
        s = lr.select([[ty, tx]], t, xy, tt, 2.0, k, frames)[0]
        s = s[s >= 0]
        want = hand_sorted(ty, tx, t, masks, k, frames)
        assert [(int(tt[i]), int(xy[i, 0]), int(xy[i, 1])) for i in s] == want
        assert len(want) == min(k, 16 * (min(T - 1, t + frames) - max(0, t - frames) + 1))
    for t, ty, tx in ((0, 4, 4), (2, 8, 12), (4, 12, 0)):                 # leave-one-site-out: the pixel is out in every frame
        s = lr.select([[ty, tx]], t, xy, tt, 2.0, 10, 2, exclude_own=True)[0]
        assert [(int(tt[i]), int(xy[i, 0]), int(xy[i, 1])) for i in s] == hand_sorted(ty, tx, t, masks, 10, 2, True)
    assert (lr.select([[1, 1]], 0, xy[tt == 4], tt[tt == 4], 2.0, 4, 2) == -1).all()      # nothing in the window


def test_sample_rules_of_the_restatement():
    e = np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    pred, var, _ = lr.krige_sample(*e, 2, 8, 8, (0.0, 1.0, 4.0, 1.0), "exponential", 4, 1)
    assert not pred.any() and np.isnan(var).all()
    (xy, tt, z), _, _ = _sample16()
    pred, var, _ = lr.krige_sample(xy, tt, z, 3, 16, 16, None, "exponential", 4, 1)
    assert np.abs(pred - z.astype(np.float64).mean()).max() <= 1e-12 and np.isnan(var).all()
    last = tt == 2                                                        # all gauges in the last frame, window of one frame
    pred, var, _ = lr.krige_sample(xy[last], tt[last], z[last], 3, 16, 16, (0.0, 1.0, 4.0, 1.0), "exponential", 4, 0)
    assert np.abs(pred[:2] - z[last].astype(np.float64).mean()).max() <= 1e-12 and np.isnan(var[:2]).all()
    assert np.isfinite(var[2]).all()


def test_surface():
    import torch
    from p2igan_bench import ops
    from p2igan_bench.models import CLASSICAL, LocalKrigingGenerator, build_generator
    from p2igan_bench.models.classical import LOCAL_NO_LOO, SPACE_TIME
    G = build_generator({"model": {"name": "localkriging"}})
    assert type(G) is LocalKrigingGenerator and CLASSICAL["localkriging"] is LocalKrigingGenerator
    assert (G.k, G.frames, G.max_points, G.fit) == (32, 2, 1024, True) and not list(G.parameters())
    assert "localkriging" not in SPACE_TIME and "leave-one-site-out" in LOCAL_NO_LOO and "'localkriging'" in LOCAL_NO_LOO
    for bad in ({"k": 0}, {"k": 65}, {"k": 2.5}, {"k": "8"}, {"frames": -1}, {"frames": 1.5}, {"k": True}):
        with pytest.raises(ValueError, match="model.neighbourhood"):
            build_generator({"model": {"name": "localkriging", "neighbourhood": bad}})
    with pytest.raises(ValueError, match="time_scale"):
        build_generator({"model": {"name": "localkriging", "variogram": {"fit": False, "nugget": 0, "psill": 1, "range": 3}}})
    with pytest.raises(ValueError, match="max_points"):
        build_generator({"model": {"name": "localkriging", "max_points": 5000}})
    assert build_generator({"model": {"name": "localkriging", "neighbourhood": {"k": 64, "frames": 0}}}).k == 64
    x = torch.zeros(1, 2, 1, 8, 8)
    with pytest.raises(RuntimeError) as e:
        G.cross_validate(x, x)
    assert str(e.value) == LOCAL_NO_LOO
    for call in (G.forward, G.forward_uq, G.cross_validate_sites):
        with pytest.raises(RuntimeError, match="HIP path"):
            call(x, x)
    assert callable(ops.lkrig_predict) and callable(ops.lkrig_loso)
    with pytest.raises(NotImplementedError, match="'localkriging'"):
        build_generator({"model": {"name": "nosuchmodel"}})
    with open(os.path.join(CONFIG_DIR, "localkriging_baseline.json")) as f:
        cfg = json.load(f)
    G = build_generator(cfg)
    assert type(G) is LocalKrigingGenerator and (G.k, G.frames) == (32, 2)


def test_run_loo_refuses_the_model_and_names_leave_one_site_out():
    from p2igan_bench.evaluation import run_loo
    from p2igan_bench.models.classical import LOCAL_NO_LOO
    with pytest.raises(RuntimeError) as e:
        run_loo({"model": {"name": "localkriging"}}, "unused")
    assert str(e.value) == LOCAL_NO_LOO


def test_what_a_neighbourhood_costs_on_the_advecting_field():
    """Section 17's field (32 x 32, T = 16, 79 fixed sites, fixed spherical (0, 0.8, 12), kappa = 2), fp64 RMSE against the truth.
    Recorded, not asserted beyond being finite: local (k = 32, frames = 2) 0.0447, global stkriging 0.0305,
    per-frame kriging 0.0439.  With fixed sites and kappa = 2 the 32 nearest points are 6 to 7 sites in 5 frames each: the
    neighbourhood trades spatial support for temporal copies of the same sites and loses what the global system gains."""
    truth, masked, masks = advecting_case()
    fixed = {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 12.0}
    per_frame = _rmse(cr.kriging(masked, masks, fixed)[0], truth)
    st = _rmse(sr.stkriging(masked, masks, dict(fixed, time_scale=2.0))[0], truth)
    local = _rmse(lr.localkriging(masked, masks, dict(fixed, time_scale=2.0), 32, 2)[0], truth)
    print(f"RMSE local (k = 32, frames = 2) {local:.4f}, global space-time {st:.4f}, per-frame {per_frame:.4f}")
    assert np.isfinite([local, st, per_frame]).all()
