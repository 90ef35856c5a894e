"""Moving-neighbourhood kriging in the Lagrangian frame without a GPU: the numpy restatement (tests/llkriging_ref.py) pinned in fp64
against things other than itself -- lkriging_ref at v = 0, the global Lagrangian restatement and an independently written dense
ordinary-kriging variance where the neighbourhood is everything, global Lagrangian leave-one-site-out, a hand-written sort on a lattice
of exact ties after an integer shift -- its skill on lagkriging_ref's seeded translating fields, and the
surface (registry, config, refusals, entry points)."""
import functools
import json
import os
import re
import sys

import numpy as np
import pytest

import classical_ref as cr
import lagkriging_ref as lg
import lkriging_ref as lr
import llkriging_ref as ll
import stkriging_ref as sr
from conftest import PKG
from test_localkriging_cpu import lattice_case
from test_stkriging_cpu import _sample16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG_DIR = os.path.join(PKG, "p2igan_bench", "config")
MODELS = [("exponential", (0.01, 0.8, 6.0)), ("spherical", (0.0, 1.3, 9.0))]


@pytest.mark.parametrize("kappa", [0.5, 2.0])
@pytest.mark.parametrize("model,params", MODELS)
def test_zero_velocity_is_the_static_neighbourhood(model, params, kappa):
    (xy, tt, z), _, _ = _sample16(seed=6, T=4, n=12)
    p = params + (kappa,)
    px = cr.grid(16, 16)
    for t in range(4):
        for k, frames, own in ((7, 1, False), (20, 3, False), (5, 2, True)):
            targets = xy[tt == t] if own else px
            assert np.array_equal(ll.select(targets, t, xy, tt, kappa, (0.0, 0.0), k, frames, own), lr.select(targets, t, xy, tt, kappa, k, frames, own))
    got, var, nbr = ll.krige_sample(xy, tt, z, 4, 16, 16, p, (0.0, 0.0), model, 7, 1, fcap=64)
    want, wvar, wnbr = lr.krige_sample(xy, tt, z, 4, 16, 16, p, model, 7, 1, fcap=64)
    assert np.array_equal(nbr, wnbr)
    assert np.abs(got - want).max() <= 1e-12 and np.abs(var - wvar).max() <= 1e-12
    lp, lv = ll.loso_sample(xy, tt, z, p, (0.0, 0.0), model, 6, 2)
    wp, wv = lr.loso_sample(xy, tt, z, p, model, 6, 2)
    assert np.abs(lp - wp).max() <= 1e-12 and np.abs(lv - wv).max() <= 1e-12


def dense_ok_variance(ty, tx, t, xy, tt, params, v, model):
    """The ordinary-kriging variance from the bordered system [[K, 1], [1^T, 0]] (lambda, mu) = (c0, 1), written out with loops and one
    general solve: c00 - lambda^T c0 - mu."""
    nugget, psill, rng, kappa = params
    n = len(tt)

    def cov(ay, ax, at, by, bx, bt):
        dt = at - bt
        ey, ex = (ay - by) - v[0] * dt, (ax - bx) - v[1] * dt
        r = np.sqrt(ey * ey + ex * ex + kappa * kappa * dt * dt) / rng
        g = 1.0 - np.exp(-r) if model == "exponential" else (1.5 * r - 0.5 * r ** 3 if r < 1.0 else 1.0)
        return psill * (1.0 - g) + (nugget if (ay == by and ax == bx and at == bt) else 0.0)

    A, rhs = np.zeros((n + 1, n + 1)), np.ones(n + 1)
    for i in range(n):
        for j in range(n):
            A[i, j] = cov(float(xy[i, 0]), float(xy[i, 1]), float(tt[i]), float(xy[j, 0]), float(xy[j, 1]), float(tt[j]))
        A[i, n] = A[n, i] = 1.0
        rhs[i] = cov(float(ty), float(tx), float(t), float(xy[i, 0]), float(xy[i, 1]), float(tt[i]))
    sol = np.linalg.solve(A, rhs)
    return psill + nugget - sol[:n] @ rhs[:n] - sol[n]


@pytest.mark.parametrize("v", [(1.5, -0.5), (-2.0, 0.75)])
@pytest.mark.parametrize("model,params", MODELS)
def test_whole_sample_neighbourhood_is_global_lagrangian_kriging(model, params, v):
    (xy, tt, z), _, _ = _sample16()
    assert len(z) == 24
    p = params + (1.3,)
    want = lg.krige_sample(xy, tt, z, 3, 16, 16, p, v, model)
    for k, frames in ((24, 2), (64, 5)):
        got, var, _ = ll.krige_sample(xy, tt, z, 3, 16, 16, p, v, model, k, frames)
        assert np.abs(got.reshape(3, 16, 16) - want).max() <= 1e-9
        assert np.isfinite(var).all() and var.min() >= 0.0
    at_gauge = np.zeros((3, 256), bool)
    at_gauge[tt, xy[:, 0] * 16 + xy[:, 1]] = True
    assert not var[at_gauge].any()
    for t in range(3):
        for q in range(t, 256, 7):
            if not at_gauge[t, q]:
                assert abs(var[t, q] - dense_ok_variance(q // 16, q % 16, t, xy, tt, p, v, model)) <= 1e-9


@pytest.mark.parametrize("vkey", ["exponential", "spherical"])
def test_loso_with_every_point_is_global_lagrangian_leave_one_site_out(vkey):
    rng = np.random.default_rng(8)
    T, h, w = 3, 16, 16
    m = np.zeros(h * w, np.float32)
    m[rng.permutation(h * w)[:9]] = 1.0
    masks = np.broadcast_to(m.reshape(1, 1, 1, h, w), (1, T, 1, h, w)).copy()
    masks[0, 1, 0].ravel()[np.flatnonzero(m)[0]] = 0.0                  # a site that misses a frame
    masked = (rng.random((1, T, 1, h, w)).astype(np.float32) + 0.2) * masks
    params = dict(MODELS)[vkey]
    vg = {"model": vkey, "fit": False, "nugget": params[0], "psill": params[1], "range": params[2], "time_scale": 1.3}
    adv = {"fit": False, "vy": 1.5, "vx": -0.5}
    want = lg.loso(masked, masks, vg, adv)
    got = ll.loso(masked, masks, vg, adv, 64, T - 1)
    assert len(got) == len(want) == T
    for a, b in zip(got, want):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
        assert np.abs(a[1] - b[1]).max() <= 1e-9 and np.abs(a[2] - b[2]).max() <= 1e-9


def hand_sorted(ty, tx, t, masks, v, k, frames, exclude_own=False):
    """The selection by a triple loop and Python's sort of integer tuples (kappa = 2, integer v): [(frame, y, x)] of the first k."""
    T, _, h, w = masks.shape
    found = []
    for tp in range(T):
        if abs(tp - t) > frames:
            continue
        for y in range(h):
            for x in range(w):
                if masks[tp, 0, y, x] != 0 and not (exclude_own and (y, x) == (ty, tx)):
                    ey, ex = (ty - y) - v[0] * (t - tp), (tx - x) - v[1] * (t - tp)
                    found.append((ey * ey + ex * ex + 4 * (tp - t) ** 2, tp, y * w + x))
    return [(tp, r // w, r % w) for _, tp, r in sorted(found)[:k]]


@pytest.mark.parametrize("v", [(1, 0), (-2, 3)])
def test_selection_on_a_shifted_lattice_of_ties_is_the_hand_written_sort(v):
    masked, masks = lattice_case()
    xy, tt, z = sr.points(masked, masks)
    vf = (float(v[0]), float(v[1]))
    for t, ty, tx, k, frames in ((0, 0, 0, 9, 2), (0, 6, 6, 12, 1), (2, 6, 6, 12, 2), (2, 8, 8, 7, 4), (4, 15, 15, 5, 1), (4, 2, 10, 20, 3),
                                 (3, 7, 9, 1, 0), (1, 10, 2, 16, 0), (4, 6, 6, 64, 4)):
        s = ll.select([[ty, tx]], t, xy, tt, 2.0, vf, k, frames)[0]
        s = s[s >= 0]
        want = hand_sorted(ty, tx, t, masks, v, k, frames)
        assert [(int(tt[i]), int(xy[i, 0]), int(xy[i, 1])) for i in s] == want
    assert hand_sorted(2, 6, 2, masks, v, 12, 2) != hand_sorted(2, 6, 2, masks, (0, 0), 12, 2)      # the shift reorders the lattice
    for t, ty, tx in ((0, 4, 4), (2, 8, 12), (4, 12, 0)):                 # leave-one-site-out: the pixel is out in every frame
        s = ll.select([[ty, tx]], t, xy, tt, 2.0, vf, 10, 2, exclude_own=True)[0]
        assert [(int(tt[i]), int(xy[i, 0]), int(xy[i, 1])) for i in s] == hand_sorted(ty, tx, t, masks, v, 10, 2, True)


def test_sample_rules_of_the_restatement():
    e = np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    v = (1.5, -0.5)
    pred, var, _ = ll.krige_sample(*e, 2, 8, 8, (0.0, 1.0, 4.0, 1.0), v, "exponential", 4, 1)
    assert not pred.any() and np.isnan(var).all()
    (xy, tt, z), _, _ = _sample16()
    pred, var, _ = ll.krige_sample(xy, tt, z, 3, 16, 16, None, v, "exponential", 4, 1)
    assert np.abs(pred - z.astype(np.float64).mean()).max() <= 1e-12 and np.isnan(var).all()
    last = tt == 2                                                        # all gauges in the last frame, window of one frame
    pred, var, _ = ll.krige_sample(xy[last], tt[last], z[last], 3, 16, 16, (0.0, 1.0, 4.0, 1.0), v, "exponential", 4, 0)
    assert np.abs(pred[:2] - z[last].astype(np.float64).mean()).max() <= 1e-12 and np.isnan(var[:2]).all()
    assert np.isfinite(var[2]).all()


@functools.lru_cache(maxsize=None)
def skill(tag):
    """RMSE against the truth on one of lagkriging_ref's translating fields (32 x 32, T = 8, 40 fixed sites), velocity and variogram
    fitted with ADVECTION / FITTED: static global, Lagrangian global, local Lagrangian with k = 32 at frames = 2 and frames = T - 1."""
    v, seed = lg.CASES[tag]
    T = 8
    truth, masked, masks = lg.translating_field(seed, v, T)
    static = lg.rmse(sr.stkriging(masked, masks, lg.FITTED)[0], truth)
    glob, fits = lg.lagkriging(masked, masks, lg.FITTED, lg.ADVECTION)
    near, _, _, lfits = ll.locallagkriging(masked, masks, lg.FITTED, lg.ADVECTION, 32, 2)
    wide = ll.locallagkriging(masked, masks, lg.FITTED, lg.ADVECTION, 32, T - 1)[0]
    assert lfits[0][:2] == fits[0][:2]
    return {"static": static, "global": lg.rmse(glob, truth), "near": lg.rmse(near, truth), "wide": lg.rmse(wide, truth), "pred": near,
            "fit": fits[0], "masked": masked, "masks": masks}


@pytest.mark.parametrize("tag", lg.MOVING)
def test_skill_on_the_moving_fields(tag):
    r = skill(tag)
    print(f"{tag}: v {r['fit'][0]}  RMSE static global {r['static']:.4f}  Lagrangian global {r['global']:.4f}  local Lagrangian k=32 frames=2 "
          f"{r['near']:.4f} ({r['near'] / r['static']:.3f} of static)  frames=7 {r['wide']:.4f} ({r['wide'] / r['global']:.3f} of global)")
    assert r["near"] <= 0.70 * r["static"]
    assert r["wide"] <= 1.05 * r["global"]


def test_resting_field_is_the_static_neighbourhood():
    r = skill("rest")
    v, params = r["fit"][:2]
    print(f"rest: v {v}  RMSE static global {r['static']:.4f}  Lagrangian global {r['global']:.4f}  local k=32 frames=2 {r['near']:.4f}  "
          f"frames=7 {r['wide']:.4f}")
    assert v == (0.0, 0.0)
    xy, tt, z = sr.points(r["masked"][0], r["masks"][0])
    want = lr.krige_sample(xy, tt, z, 8, 32, 32, params, "exponential", 32, 2)[0]
    assert np.abs(r["pred"][0, :, 0].reshape(8, -1) - want).max() <= 1e-9


def test_surface(tmp_path):
    import torch
    from p2igan_bench import _hip, ops
    from p2igan_bench.evaluation import run_loo
    from p2igan_bench.models import CLASSICAL, LocalKrigingGenerator, LocalLagrangianKrigingGenerator, build_generator
    from p2igan_bench.models.classical import LOCAL, LOCAL_LAG_NO_LOO, SPACE_TIME
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import crossvalidate as cv_script
    import train as train_script
    G = build_generator({"model": {"name": "locallagkriging"}})
    assert type(G) is LocalLagrangianKrigingGenerator and CLASSICAL["locallagkriging"] is LocalLagrangianKrigingGenerator
    assert isinstance(G, LocalKrigingGenerator) and not list(G.parameters())
    assert (G.k, G.frames, G.max_points, G.fit) == (32, 2, 1024, True)
    assert G.fit_velocity and (G.vmax, G.vstep, G.adv_tlags, G.bandwidth, G.nhalf) == (4.0, 0.5, 3, 1.5, 8)
    assert LOCAL == ("localkriging", "locallagkriging") and "locallagkriging" not in SPACE_TIME
    assert "leave-one-site-out" in LOCAL_LAG_NO_LOO and "'locallagkriging'" in LOCAL_LAG_NO_LOO
    for bad in ({"k": 0}, {"k": 65}, {"k": 2.5}, {"k": "8"}, {"frames": -1}, {"frames": 1.5}, {"k": True}):
        with pytest.raises(ValueError, match="model.neighbourhood"):
            build_generator({"model": {"name": "locallagkriging", "neighbourhood": bad}})
    bad = [{"fit": False, "vy": 1.0}, {"fit": False, "vx": 1.0}, {"fit": False, "vy": float("nan"), "vx": 0.0}, {"vstep": 0.0}, {"vstep": -0.5},
           {"vmax": -1.0}, {"vmax": 8.5, "vstep": 0.5}, {"vmax": 4.0, "vstep": 0.1}, {"n_tlags": 8}, {"n_tlags": -1}, {"bandwidth": 0.0}]
    for adv in bad:
        with pytest.raises(ValueError, match="advection"):
            build_generator({"model": {"name": "locallagkriging", "advection": adv}})
    with pytest.raises(ValueError, match="time_scale"):
        build_generator({"model": {"name": "locallagkriging", "variogram": {"fit": False, "nugget": 0, "psill": 1, "range": 3}}})
    with pytest.raises(ValueError, match="max_points"):
        build_generator({"model": {"name": "locallagkriging", "max_points": 5000}})
    fixed = build_generator({"model": {"name": "locallagkriging", "neighbourhood": {"k": 64, "frames": 0},
                                       "advection": {"fit": False, "vy": 0.75, "vx": -1.25}}})
    assert fixed.k == 64 and not fixed.fit_velocity and fixed.fixed_v == (0.75, -1.25)
    with pytest.raises(NotImplementedError, match="'locallagkriging'"):
        build_generator({"model": {"name": "nosuchmodel"}})

    path = os.path.join(CONFIG_DIR, "locallagkriging_baseline.json")
    cfg = json.load(open(path))
    assert cfg["model"]["name"] == "locallagkriging" and cfg["model"]["advection"] == lg.ADVECTION
    assert cfg["model"]["neighbourhood"] == {"k": 32, "frames": 2}
    assert cfg["data"] == json.load(open(os.path.join(CONFIG_DIR, "localkriging_baseline.json")))["data"]
    G = build_generator(cfg)
    assert type(G) is LocalLagrangianKrigingGenerator and (G.k, G.frames, G.nhalf) == (32, 2, 8)
    x = torch.zeros(1, 2, 1, 8, 8)
    with pytest.raises(RuntimeError) as e:
        G.cross_validate(x, x)
    assert str(e.value) == LOCAL_LAG_NO_LOO
    for call in (G.forward, G.forward_uq, G.cross_validate_sites):
        with pytest.raises(RuntimeError, match="HIP path"):
            call(x, x)
    with pytest.raises(RuntimeError) as e:
        run_loo(cfg, str(tmp_path / "loo"))
    assert str(e.value) == LOCAL_LAG_NO_LOO
    with pytest.raises(RuntimeError) as e:
        cv_script.main(["--config", path, "--output", str(tmp_path / "loo")])
    assert str(e.value) == LOCAL_LAG_NO_LOO
    with pytest.raises(RuntimeError, match="nothing to train"):
        train_script.main(["--config", path])
    assert not (tmp_path / "loo").exists()

    assert callable(ops.lkrig_predict) and callable(ops.lkrig_loso)
    import inspect
    assert inspect.signature(ops.lkrig_predict).parameters["velf"].default is None
    assert inspect.signature(ops.lkrig_loso).parameters["velf"].default is None
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2i_hip.h")).read(), flags=re.S)
    lib = _hip.load()
    for name, nargs in (("p2i_lkrig_predict", 20), ("p2i_lkrig_loso", 17)):           # the lists without a velocity (19, 16) plus velf
        proto = re.search(rf"\bint {name}\s*\(([^;]*)\);", header)
        assert proto and re.search(r"\bconst float\s*\*\s*velf\b", proto.group(1)) and hasattr(lib, name)
        assert len(proto.group(1).split(",")) == nargs == len(_hip.SIGNATURES[name])
        gone = name + "_lag"                                                          # one entry point per stage, no Lagrangian twin
        assert not re.search(rf"\b{gone}\b", header) and not hasattr(lib, gone) and gone not in _hip.SIGNATURES
