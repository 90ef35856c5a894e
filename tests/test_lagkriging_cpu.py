"""Lagrangian space-time kriging without a GPU: the numpy restatement (tests/lagkriging_ref.py) on seeded translating fields -- the
velocity estimate, the gain over static space-time kriging against the truth and in leave-one-site-out -- its consistency with
stkriging_ref at v = 0 and under a shear of the coordinates, and the surface (registry, config, refusals).

The fields: 32 x 32, 40 gauges at fixed sites, 8 frames (lagkriging_ref.translating_field).  The seeds below were chosen once so that
the restatement holds the bounds with room (the figures are printed) and are kept."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import classical_ref as cr
import lagkriging_ref as lg
import stkriging_loso_ref as lr
import stkriging_ref as sr
from conftest import PKG

CONFIG_DIR = os.path.join(PKG, "p2igan_bench", "config")
CASES, MOVING, VG = lg.CASES, lg.MOVING, lg.FITTED
KAPPAS = (1.0, 2.0, 4.0, 8.0, 1000.0)


@functools.lru_cache(maxsize=None)
def run(tag):
    """Everything the tests below read of one case, computed once: the fields, the Lagrangian restatement, static space-time kriging
    at the fitted spatial variogram for every kappa of KAPPAS, and the leave-one-site-out RMSE of both."""
    v, seed = CASES[tag]
    truth, masked, masks = lg.translating_field(seed, v, 8)
    out, fits = lg.lagkriging(masked, masks, VG, lg.ADVECTION)
    sfit = sr.fit_st(*sr.st_bins(lg.frames_of(masked[0], masks[0]), 32, 32, 16, 3), cr.lag_width(32, 32, 16), "exponential")
    static = {}
    for kappa in KAPPAS:
        fixed = {"model": "exponential", "fit": False, "nugget": sfit[2], "psill": sfit[3], "range": sfit[4], "time_scale": kappa}
        static[kappa] = lg.rmse(sr.stkriging(masked, masks, fixed)[0], truth)
    best = min(static, key=static.get)
    fixed = {"model": "exponential", "fit": False, "nugget": sfit[2], "psill": sfit[3], "range": sfit[4], "time_scale": best}
    return {"truth": truth, "masked": masked, "masks": masks, "fit": fits[0], "rmse": lg.rmse(out, truth), "static": static, "best": best,
            "loso": lg.loso_rmse(lg.loso(masked, masks, VG, lg.ADVECTION)), "loso_static": lg.loso_rmse(lr.loso(masked, masks, fixed)),
            "loso_static_fit": lg.loso_rmse(lr.loso(masked, masks, VG))}


def test_the_field_moves_as_asked():
    truth = lg.translating_field(0, (-2.0, 2.0), 4, size=32)[0][0, :, 0]
    raw = lg.translating_field(0, (0.0, 0.0), 4, size=32)[0][0, :, 0]
    assert np.abs(raw[1:] - raw[0]).max() == 0.0                             # v = 0: every frame is the first
    # an integer velocity is a plain shift: frame t at x equals frame 0 at x - v t (where both are inside the crop); all frames of a
    # call are standardised by the same constants
    assert np.abs(truth[1][:-2, 2:] - truth[0][2:, :-2]).max() <= 1e-5
    assert (truth >= 0).all() and 0.2 < (truth == 0).mean() < 0.8            # rectified at 0


@pytest.mark.parametrize("tag", sorted(CASES))
def test_velocity_estimate(tag):
    r = run(tag)
    v, _, est, _ = r["fit"]
    print(f"{tag}: true v {CASES[tag][0]}  estimate {v}  gap to the runner-up {est[3]:.3g}")
    assert abs(v[0] - CASES[tag][0][0]) <= 1.0 and abs(v[1] - CASES[tag][0][1]) <= 1.0


@pytest.mark.parametrize("tag", MOVING)
def test_moving_fields_gain(tag):
    r = run(tag)
    ratio = r["rmse"] / r["static"][r["best"]]
    print(f"{tag}: Lagrangian RMSE {r['rmse']:.4f}  static {r['static']}  ratio to the best {ratio:.3f};  LOSO RMSE Lagrangian "
          f"{r['loso']:.4f}  static at its best kappa {r['loso_static']:.4f}  static fitted {r['loso_static_fit']:.4f}")
    assert ratio <= 0.8
    assert r["loso"] < r["loso_static"] and r["loso"] < r["loso_static_fit"]    # leave-one-site-out orders them as the truth does


def test_resting_field_equals_static():
    r = run("rest")
    ratio = r["rmse"] / r["static"][r["best"]]
    print(f"rest: Lagrangian RMSE {r['rmse']:.4f}  static {r['static']}  ratio to the best {ratio:.3f}")
    assert abs(ratio - 1.0) <= 0.05


def test_eligibility_rule_needs_the_distinct_pixels():
    """Why the support counts pairs of distinct pixels: with fixed sites the same-pixel pairs add one full-weight pair per site and
    frame pair to W(0) and next to nothing to a fast candidate, so 'W(v) >= W(0) / 2' would rule the true velocity out."""
    r = run("right")
    frames = lg.frames_of(r["masked"][0], r["masks"][0])
    W, S, N = lg.score_tables(frames, 3, 8, 0.5, 1.5)
    true = (8, 8 + 6)                                                         # v = (0, 3) on the 0.5 grid
    print(f"right: W(v) / W(0) at the truth {W[true] / W[8, 8]:.3f}  N(v) / N(0) {N[true] / N[8, 8]:.3f}")
    assert W[true] < 0.5 * W[8, 8] and N[true] >= 0.5 * N[8, 8]
    (i, j), _ = lg.pick(W, S, W)                                              # the rule on W: the estimate stays slow
    assert abs(0.5 * j - 3.0) > 1.0


def test_zero_velocity_is_stkriging_and_a_shear_is_a_shift():
    rng = np.random.default_rng(2)
    T, h, w, n = 4, 12, 14, 9
    masks = np.zeros((1, T, 1, h, w), np.float32)
    for t in range(T):
        masks[0, t, 0].ravel()[rng.permutation(h * w)[:n]] = 1.0
    masked = (rng.random((1, T, 1, h, w)).astype(np.float32) + 0.1) * masks
    fixed = {"model": "spherical", "fit": False, "nugget": 0.01, "psill": 0.8, "range": 9.0, "time_scale": 1.5}
    rest = {"fit": False, "vy": 0.0, "vx": 0.0}
    assert np.array_equal(lg.lagkriging(masked, masks, fixed, rest)[0], sr.stkriging(masked, masks, fixed)[0])
    frames = lg.frames_of(masked[0], masks[0])
    for a, b in zip(lg.lag_bins(frames, h, w, 16, 3, (0.0, 0.0)), sr.st_bins(frames, h, w, 16, 3)):
        assert np.array_equal(a, b)
    # integer v: the Lagrangian prediction at (t, p) is the static one at (t, p - v t + offset) on a canvas enlarged by |v| (T - 1) with
    # the gauges of frame t moved to x - v t + offset
    v = (1, -2)
    oy, ox = v[0] * (T - 1), 0                                              # offsets that keep y - v_y t and x - v_x t >= 0
    H2, W2 = h + abs(v[0]) * (T - 1), w + abs(v[1]) * (T - 1)
    m2, z2 = np.zeros((1, T, 1, H2, W2), np.float32), np.zeros((1, T, 1, H2, W2), np.float32)
    for t in range(T):
        ys, xs = np.nonzero(masks[0, t, 0])
        m2[0, t, 0, ys - v[0] * t + oy, xs - v[1] * t + ox] = 1.0
        z2[0, t, 0, ys - v[0] * t + oy, xs - v[1] * t + ox] = masked[0, t, 0, ys, xs]
    lag = lg.lagkriging(masked, masks, fixed, {"fit": False, "vy": float(v[0]), "vx": float(v[1])})[0]
    big = sr.stkriging(z2, m2, fixed)[0]
    for t in range(T):
        y0, x0 = oy - v[0] * t, ox - v[1] * t
        assert np.abs(lag[0, t, 0] - big[0, t, 0, y0:y0 + h, x0:x0 + w]).max() <= 1e-9


def test_pick_rules():
    W = np.ones((3, 3))
    assert lg.pick(W, np.zeros((3, 3)), W)[0] == (0, 0)                       # zero variance: every score ties, v = 0
    assert lg.pick(np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3)))[0] == (0, 0)      # no pair: every score is inf
    S = np.ones((3, 3))
    S[0, 1] = S[1, 0] = 0.5                                                   # a tie at equal |v|^2: the lower (i, j)
    assert lg.pick(W, S, W)[0] == (-1, 0)
    S[2, 2] = 0.5                                                             # ... and the smaller |v|^2 before that
    assert lg.pick(W, S, W)[0] == (-1, 0)
    N = W.copy()
    N[0, 1] = 0.49                                                            # below half the support of v = 0: not eligible
    assert lg.pick(W, S, N)[0] == (0, -1)
    assert lg.nhalf_of(4.0, 0.5) == 8 and lg.nhalf_of(1.25, 0.5) == 3 and lg.nhalf_of(0.0, 0.5) == 0


def test_registry_builds_the_lagrangian_generator():
    from p2igan_bench import ops
    from p2igan_bench.models import CLASSICAL, LagrangianKrigingGenerator, SpaceTimeKrigingGenerator, build_discriminator, build_generator
    G = build_generator({"model": {"name": "lagkriging"}})
    assert type(G) is LagrangianKrigingGenerator and CLASSICAL["lagkriging"] is LagrangianKrigingGenerator
    assert isinstance(G, SpaceTimeKrigingGenerator) and type(build_generator({"model": {"name": "stkriging"}})) is SpaceTimeKrigingGenerator
    assert len(G.state_dict()) == 0 and not list(G.parameters())
    assert G.max_points == 4096 and G.fit and G.n_lags == 16 and G.n_tlags == 3
    assert G.fit_velocity and (G.vmax, G.vstep, G.adv_tlags, G.bandwidth, G.nhalf) == (4.0, 0.5, 3, 1.5, 8)
    assert not hasattr(G, "forward_uq")
    assert ops.LAGKRIG_MAX_CANDIDATES == (2 * ops.LAGKRIG_MAX_VHALF + 1) ** 2 == 1089
    for fn in ("lagkrig_velocity", "lagkrig_variogram", "lagkrig_factor", "lagkrig_predict"):
        assert callable(getattr(ops, fn))
    with pytest.raises(NotImplementedError):
        build_discriminator({"model": {"name": "lagkriging"}})
    G = build_generator({"model": {"name": "lagkriging", "advection": {"fit": False, "vy": 0.75, "vx": -1.25}}})
    assert not G.fit_velocity and G.fixed_v == (0.75, -1.25)
    assert build_generator({"model": {"name": "lagkriging", "advection": {"vmax": 8.0, "vstep": 0.5}}}).nhalf == 16
    bad = [{"fit": False, "vy": 1.0}, {"fit": False, "vx": 1.0}, {"fit": False, "vy": float("nan"), "vx": 0.0}, {"vstep": 0.0}, {"vstep": -0.5},
           {"vmax": -1.0}, {"vmax": 8.5, "vstep": 0.5}, {"vmax": 4.0, "vstep": 0.1}, {"n_tlags": 8}, {"n_tlags": -1}, {"bandwidth": 0.0}]
    for adv in bad:
        with pytest.raises(ValueError, match="advection"):
            build_generator({"model": {"name": "lagkriging", "advection": adv}})
    with pytest.raises(ValueError, match="candidate"):
        build_generator({"model": {"name": "lagkriging", "advection": {"vmax": 8.5, "vstep": 0.5}}})
    with pytest.raises(ValueError, match="time_scale"):                       # the variogram is stkriging's
        build_generator({"model": {"name": "lagkriging", "variogram": {"fit": False, "nugget": 0.0, "psill": 1.0, "range": 5.0}}})
    with pytest.raises(ValueError, match="max_points"):
        build_generator({"model": {"name": "lagkriging", "max_points": 4097}})


def test_config_loads_cpu_tensors_raise_and_scripts_refuse(tmp_path):
    import torch
    from p2igan_bench.evaluation import run_loo, run_loso
    from p2igan_bench.models import build_generator
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import crossvalidate as cv_script
    import train as train_script
    path = os.path.join(CONFIG_DIR, "lagkriging_baseline.json")
    cfg = json.load(open(path))
    assert cfg["model"]["name"] == "lagkriging" and cfg["model"]["advection"] == lg.ADVECTION
    assert cfg["data"] == json.load(open(os.path.join(CONFIG_DIR, "stkriging_baseline.json")))["data"]
    G = build_generator(cfg)
    assert G.max_points == 4096 and G.fit and G.fit_velocity and G.variogram_model == 0 and (G.n_lags, G.n_tlags, G.nhalf) == (16, 3, 8)
    x = torch.zeros(1, 2, 1, 8, 8)
    with pytest.raises(RuntimeError, match="HIP path"):
        G(x, x)
    with pytest.raises(RuntimeError, match="HIP path"):
        G.cross_validate_sites(x, x)
    with pytest.raises(RuntimeError, match="lagkriging.*leave-one-site-out"):
        G.cross_validate(x, x)
    with pytest.raises(RuntimeError, match="nothing to train"):
        train_script.main(["--config", path])
    with pytest.raises(RuntimeError, match="lagkriging.*leave-one-site-out"):
        run_loo(cfg, str(tmp_path / "loo"))
    with pytest.raises(RuntimeError, match="leave-one-site-out"):
        cv_script.main(["--config", path, "--output", str(tmp_path / "loo")])
    with pytest.raises(ValueError, match="'lagkriging'.*at most 32 frames"):
        run_loso(cfg, str(tmp_path / "loso"), stride=33)
    with pytest.raises(ValueError, match="at most 32 frames"):
        cv_script.main(["--config", path, "--output", str(tmp_path / "loso"), "--by-site", "--stride", "33"])
    assert not (tmp_path / "loo").exists() and not (tmp_path / "loso").exists()
