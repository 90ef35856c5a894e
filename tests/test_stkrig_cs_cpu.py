"""The restatement behind the space-time conditional-simulation kernels (tests/stkrig_cs_ref.py) against first
principles, fp64 numpy: members that honour every point, ensemble statistics against the space-time kriging mean and variance, the
unconditional fields' covariance in space and time, the variance of a pixel's accumulation over the sample (the property the feature
exists for), exact and clipped embeddings, and the independence of a member from the ensemble size.  The package's surface is checked for
its refusals; the numbers on the device are tests/test_stkrig_cs_gpu.py's.

Statistical bounds, M = 2048 members, six standard errors of each estimator: a mean of M Gaussians with variance s2 has standard error
sqrt(s2 / M); a sample variance of M Gaussians has relative standard error sqrt(2 / (M - 1)); a sample covariance of two Gaussians with
variances <= c00 has standard error <= c00 sqrt(2 / M) <= c00 sqrt(2 / (M - 1)); a sample correlation of n independent pairs of
uncorrelated Gaussians has standard error 1 / sqrt(n).  Only cases whose fp64 clip share is exactly 0 are used: with a clipped
spectrum the simulated covariance is not the variogram's."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import stkrig_cs_ref as sc
import stkriging_ref as st
from conftest import PKG

M = 2048
T, H, W = 4, 8, 8
BOUND = 6.0 * np.sqrt(2.0 / (M - 1))
# (nugget, psill, range, kappa) of the two statistics cases at T = 4, 8 x 8, embed = embed_time = 2
CASES = {"exponential": (0.05, 0.6, 2.0, 3.0), "spherical": (0.02, 0.8, 6.0, 2.0)}
# model, (nugget, psill, range), kappa, T, frame: embeddings that clip nothing at embed = embed_time = 2
EXACT = [("exponential", (0.05, 0.6, 2.0), 3.0, 4, (8, 8)), ("exponential", (0.05, 0.6, 2.0), 4.0, 3, (17, 23)),
         ("spherical", (0.02, 0.8, 6.0), 2.0, 4, (8, 8)), ("spherical", (0.02, 0.8, 6.0), 2.0, 4, (16, 16)),
         ("spherical", (0.02, 0.8, 9.0), 3.0, 5, (17, 23))]


def _sites(n=12, seed=3, t=T, h=H, w=W):
    """n gauge pixels observed in every frame: (xy (n t, 2), tt (n t,), z (n t,) fp32), frame-major as the device gathers them."""
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.permutation(h * w)[:n])
    xy = np.tile(np.stack([idx // w, idx % w], axis=1), (t, 1))
    return xy, np.repeat(np.arange(t, dtype=np.int64), n), rng.random(n * t).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _members(model):
    """(xy, tt, z, Z (M, T, H, W) fp64) of the statistics case; built once, never modified."""
    xy, tt, z = _sites()
    return xy, tt, z, sc.members_sample(xy, tt, z, T, H, W, CASES[model], model, M, seed=11, stream=5)


@functools.lru_cache(maxsize=None)
def _fields(model):
    """(b (St, Sy, Sx), U (M, T, H, W) fp64): the base and the unconditional fields of the statistics case; never modified."""
    A, rho = sc.spectrum(CASES[model], model, T, H, W)
    assert rho == 0.0
    return sc.base(CASES[model], model, T, H, W), sc.unconditional(A, 11, 5, M, T, H, W)


@pytest.mark.parametrize("model", cr.MODELS)
def test_members_equal_z_at_the_points(model):
    xy, tt, z, Z = _members(model)
    assert np.abs(Z[:, tt, xy[:, 0], xy[:, 1]] - z[None, :].astype(np.float64)).max() <= 1e-12
    # and before the points are written: the conditioning itself reproduces z
    raw = sc.members_sample(xy, tt, z, T, H, W, CASES[model], model, 4, seed=11, stream=5, write_points=False)
    assert np.abs(raw[:, tt, xy[:, 0], xy[:, 1]] - z[None, :].astype(np.float64)).max() <= 1e-12
    full = sc.members_sample(xy, tt, z, T, H, W, CASES[model], model, 4, seed=11, stream=5)
    cells = (tt * H + xy[:, 0]) * W + xy[:, 1]
    assert np.array_equal(np.delete(raw.reshape(4, -1), cells, axis=1), np.delete(full.reshape(4, -1), cells, axis=1))
    less = sc.members_sample(xy[:-1], tt[:-1], z[:-1], T, H, W, CASES[model], model, 4, seed=11, stream=5)
    assert np.abs(less - full).max() > 1e-3           # the last point matters, so the check above is not vacuous


@pytest.mark.parametrize("model", cr.MODELS)
def test_ensemble_statistics(model):
    xy, tt, z, Z = _members(model)
    params = CASES[model]
    c00 = params[0] + params[1]
    mean = st.krige_sample(xy, tt, z, T, H, W, params, model)
    var = sc.kriging_variance(xy, tt, T, H, W, params, model)
    assert np.abs(var[tt, xy[:, 0], xy[:, 1]]).max() <= 1e-12          # the analytic variance vanishes at the points
    ok = var > 1e-3 * c00
    assert ok.sum() >= T * H * W // 2
    zs = float((np.abs(Z.mean(0) - mean)[ok] / np.sqrt(var[ok] / M)).max())
    vr = float(np.abs(Z.var(0, ddof=1)[ok] / var[ok] - 1.0).max())
    print(f"{model}: mean {zs:.2f} sigma  variance {vr:.4f} (bound {BOUND:.4f}) over {int(ok.sum())} targets")
    assert zs <= 6.0
    assert vr <= BOUND


@pytest.mark.parametrize("model", cr.MODELS)
def test_unconditional_covariance_in_space_and_time(model):
    """cov(U(t, p), U(t + u, p + h)) against b[u, h] for u = 0, 1, 2 and a few h, at every (t, p) where both ends are in the sample."""
    b, U = _fields(model)
    c00 = CASES[model][0] + CASES[model][1]
    assert abs(b[0, 0, 0] - (float(np.float32(CASES[model][0])) + float(np.float32(CASES[model][1])))) <= 1e-15
    worst = 0.0
    for u in (0, 1, 2):
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 3), (0, 4), (3, 0)):
            a, c = U[:, :T - u, :H - dy, :W - dx], U[:, u:, dy:, dx:]
            emp = (a * c).sum(0) / (M - 1) - a.sum(0) * c.sum(0) / (M * (M - 1))
            err = float(np.abs(emp - b[u, dy, dx]).max()) / c00
            worst = max(worst, err)
            assert err <= BOUND, (u, dy, dx, err)
    print(f"{model}: covariance {worst:.4f} c00 (bound {BOUND:.4f} c00)")


@pytest.mark.parametrize("model", cr.MODELS)
def test_the_accumulation_variance_is_the_space_time_model_s(model):
    """The variance of a pixel's T-frame sum is sum_t,t' b[t - t'], and is NOT T b[0], the figure of frame-wise independent noise."""
    b, U = _fields(model)
    want = sum(b[abs(t - s), 0, 0] for t in range(T) for s in range(T))
    indep = T * b[0, 0, 0]
    emp = U.sum(1).var(0, ddof=1)                                       # (H, W): one estimate per pixel
    rel = float(np.abs(emp / want - 1.0).max())
    off = float(np.abs(emp / indep - 1.0).min())
    print(f"{model}: accumulation variance {emp.mean():.4f}, model {want:.4f} (worst pixel off by {rel:.4f}, bound {BOUND:.4f}); "
          f"independent frames would give {indep:.4f} (nearest pixel off by {off:.4f})")
    assert rel <= BOUND
    assert off > BOUND


@pytest.mark.parametrize("model", cr.MODELS)
def test_the_two_members_of_a_pair_are_uncorrelated(model):
    """Per cell of the sample, the correlation of Re and Im over the M / 2 pairs: standard error 1 / sqrt(M / 2)."""
    _, U = _fields(model)
    re, im = U[0::2].reshape(M // 2, -1), U[1::2].reshape(M // 2, -1)
    re, im = re - re.mean(0), im - im.mean(0)
    corr = (re * im).sum(0) / np.sqrt((re * re).sum(0) * (im * im).sum(0))
    print(f"{model}: pair correlation, worst cell {np.abs(corr).max():.4f} (bound {6.0 / np.sqrt(M // 2):.4f}), mean {corr.mean():+.5f}")
    assert np.abs(corr).max() <= 6.0 / np.sqrt(M // 2)
    assert abs(corr.mean()) <= 6.0 / np.sqrt(M // 2)


@pytest.mark.parametrize("model,vg,kappa,t,frame", EXACT)
def test_exact_embeddings_clip_nothing(model, vg, kappa, t, frame):
    A, rho = sc.spectrum(vg + (kappa,), model, t, frame[0], frame[1])
    assert rho == 0.0 and A.shape == (2 * t, 2 * frame[0], 2 * frame[1])
    c00 = float(np.float32(vg[0])) + float(np.float32(vg[1]))           # the spectrum starts from the fp32 parameters
    assert abs((A * A).sum() - c00) <= 1e-12                           # sum lambda / (St Sy Sx) = b[0, 0, 0] = c00


def test_a_slow_decorrelation_clips_and_a_longer_torus_clips_less():
    A, rho = sc.spectrum((0.05, 0.6, 3.0, 1.5), "exponential", 4, 8, 8)
    print("clip share of exponential (0.05, 0.6, 3), kappa 1.5, T = 4, 8 x 8:", rho)
    assert abs(rho - 5.147e-3) <= 5e-7
    assert abs((A * A).sum() - (float(np.float32(0.05)) + float(np.float32(0.6)))) <= 1e-12       # the variance is restored after clipping
    longer = [sc.spectrum((0.05, 0.6, 3.0, 1.5), "exponential", 4, 8, 8, 2, et)[1] for et in (3, 4)]
    print("  with embed_time 3, 4:", longer)
    assert longer[0] < rho and longer[1] < rho


def test_the_noise_is_krig_cs_noise_over_the_flat_cell_index():
    import krig_cs_ref as cs
    xi = sc.noise(7, (3 << 32) | 9, [0, 2], 6, 10, 14)
    flat = cs.noise(7, (3 << 32) | 9, [0, 2], 60, 14)
    assert xi.shape == (2, 6, 10, 14) and np.array_equal(xi.reshape(2, 60, 14), flat)
    assert xi[1, 2, 3, 4] == flat[1, 2 * 10 + 3, 4]                    # cell = (l Sy + j) Sx + k


def test_a_member_does_not_depend_on_the_ensemble_size():
    xy, tt, z = _sites()
    run = functools.partial(sc.members_sample, xy, tt, z, T, H, W, CASES["exponential"], "exponential", seed=7, stream=(9 << 32) | 4)
    five = run(members=5)
    assert np.array_equal(run(members=3), five[:3]) and np.array_equal(run(members=2), five[:2])


def test_a_member_changes_with_the_stream_and_the_seed():
    xy, tt, z = _sites()
    base = sc.members_sample(xy, tt, z, T, H, W, CASES["spherical"], "spherical", 2, seed=7, stream=4)
    for seed, stream in ((7, 5), (7, (1 << 32) | 4), (8, 4), ((1 << 32) | 7, 4)):
        other = sc.members_sample(xy, tt, z, T, H, W, CASES["spherical"], "spherical", 2, seed=seed, stream=stream)
        assert np.abs(other - base).max() > 0.1, (seed, stream)


def test_the_batch_restatement_applies_the_sample_rules():
    masks = np.zeros((3, T, 1, H, W), np.float32)
    xy, tt, z = _sites()
    at = (tt[tt > 0], 0, xy[tt > 0, 0], xy[tt > 0, 1])
    masks[0][at] = 1.0                                                # sample 0: a frame without gauges, then healthy ones
    masked = np.zeros_like(masks)
    masked[0][at] = z[tt > 0]
    masks[2][(tt, 0, xy[:, 0], xy[:, 1])] = 1.0                        # sample 2: constant values, a degenerate fit; sample 1: no points
    masked[2] = 0.4 * masks[2]
    ens, rho = sc.simulation(masked, masks, {"model": "exponential", "fit": True, "n_lags": 4, "n_tlags": 2}, 3, seed=1)
    assert np.isfinite(ens[0]).all() and np.isnan(ens[1]).all() and np.isnan(ens[2]).all()
    assert np.isfinite(rho[0]) and np.isnan(rho[1]) and np.isnan(rho[2])
    assert np.abs(ens[0, 0]).max() > 0                                # the gauge-less frame is simulated like any other
    got = ens[0].transpose(1, 0, 2, 3)[:, tt[tt > 0], xy[tt > 0, 0], xy[tt > 0, 1]]
    assert np.array_equal(got, np.broadcast_to(z[tt > 0].astype(np.float64), got.shape))


# ---- the package's surface: refusals that need no device
def _model(name="stkriging", **model):
    from p2igan_bench.models import build_generator
    return build_generator({"model": dict({"name": name}, **model)})


def test_forward_simulation_refuses_cpu_tensors():
    x = torch.zeros(1, 2, 1, H, W)
    with pytest.raises(RuntimeError, match="HIP path only"):
        _model().forward_simulation(x, x, 3)


@pytest.mark.parametrize("key", ["embed", "embed_time"])
@pytest.mark.parametrize("value", [1, 5, 2.0, "2", True, None])
def test_a_bad_embed_is_refused(key, value):
    with pytest.raises(ValueError, match=f"model.ensemble.{key} "):
        _model(ensemble={key: value})


def test_the_embeds_are_read_from_the_config():
    G = _model()
    assert (G.embed, G.embed_time) == (2, 2) and G.last_ensemble is None
    G = _model(ensemble={"embed": 3, "embed_time": 4})
    assert (G.embed, G.embed_time) == (3, 4)
    assert _model(ensemble={}).embed_time == 2
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "stkriging_ensemble.json")))
    assert cfg["model"]["name"] == "stkriging"
    G = _model(**{k: v for k, v in cfg["model"].items() if k != "name"})
    assert (G.embed, G.embed_time) == (cfg["model"]["ensemble"]["embed"], cfg["model"]["ensemble"]["embed_time"])
    base = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "stkriging_baseline.json")))
    assert {k: v for k, v in cfg["model"].items() if k != "ensemble"} == base["model"] and cfg["data"] == base["data"]
    with pytest.raises(ValueError, match="ensemble"):
        _model(ensemble=[2, 2])


def test_a_torus_past_its_limits_is_refused_before_any_launch():
    x = torch.zeros(1, 65, 1, 8, 8)                                  # CPU tensors: the size is looked at first; 2 x 65 = 130 cells
    with pytest.raises(ValueError, match="128"):
        _model().forward_simulation(x, x, 2)
    x = torch.zeros(1, 33, 1, 8, 8)
    with pytest.raises(ValueError, match="128"):
        _model(ensemble={"embed_time": 4}).forward_simulation(x, x, 2)
    with pytest.raises(RuntimeError, match="HIP path only"):        # 4 x 32 = 128 fits
        _model(ensemble={"embed_time": 4}).forward_simulation(torch.zeros(1, 32, 1, 8, 8), torch.zeros(1, 32, 1, 8, 8), 2)
    x = torch.zeros(1, 2, 1, 257, 16)
    with pytest.raises(ValueError, match="512"):
        _model().forward_simulation(x, x, 2)
    x = torch.zeros(1, 2, 1, 16, 129)
    with pytest.raises(ValueError, match="512"):
        _model(ensemble={"embed": 4}).forward_simulation(x, x, 2)


@pytest.mark.parametrize("members", [0, 65, -1, 2.0, True])
def test_members_outside_1_to_64_are_refused(members):
    x = torch.zeros(1, 2, 1, H, W)
    with pytest.raises(ValueError, match="members must be an integer in \\[1, 64\\]"):
        _model().forward_simulation(x, x, members)


def test_the_other_models_refuse():
    from p2igan_bench import inference
    from p2igan_bench.models import CLASSICAL
    assert [n for n, c in CLASSICAL.items() if hasattr(c, "forward_simulation")] == ["stkriging", "lagkriging"]
    x = torch.zeros(1, 2, 1, H, W)
    with pytest.raises(RuntimeError, match="'lagkriging'.* has no conditional simulation: .*sheared torus"):
        _model("lagkriging").forward_simulation(x, x, 3)
    with pytest.raises(RuntimeError, match="sheared torus"):
        inference.infer_event_ensemble(_model("lagkriging"), x, x, 3)
    for name in ("localkriging", "locallagkriging", "idw"):
        with pytest.raises(RuntimeError, match="has no conditional simulation"):
            inference.infer_event_ensemble(_model(name), x, x, 3)


@pytest.mark.parametrize("name", ["lagkriging", "localkriging", "locallagkriging", "idw"])
def test_infer_refuses_an_ensemble_of_the_other_models(tmp_path, name):
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import infer as infer_script
    cfg = os.path.join(PKG, "p2igan_bench", "config", f"{name}_baseline.json")
    with pytest.raises(RuntimeError, match="--ensemble-output needs model.name 'kriging' or 'stkriging'"):
        infer_script.main(["--config", cfg, "--output", str(tmp_path / "o.zarr"), "--ensemble-output", str(tmp_path / "ens"), "--members", "3"])
    assert not (tmp_path / "o.zarr").exists() and not (tmp_path / "ens").exists()


def test_infer_checks_the_members_of_stkriging(tmp_path):
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import infer as infer_script
    cfg = os.path.join(PKG, "p2igan_bench", "config", "stkriging_ensemble.json")
    for extra in ([], ["--members", "0"], ["--members", "65"]):
        with pytest.raises(ValueError, match="--members"):
            infer_script.main(["--config", cfg, "--output", str(tmp_path / "k.zarr"), "--ensemble-output", str(tmp_path / "ens")] + extra)
    assert not (tmp_path / "k.zarr").exists() and not (tmp_path / "ens").exists()


def test_the_surface_exists():
    from p2igan_bench import _hip, inference, ops
    for name in ("p2i_stcs_spectrum", "p2i_stcs_noise", "p2i_stcs_fields", "p2i_stcs_weights", "p2i_stcs_predict"):
        assert name in _hip.STCS_SIGNATURES and name not in _hip.SIGNATURES
        assert callable(getattr(ops, name[4:]))
    assert ops.stcs_torus(16, 128, 128, 2, 2) == (32, 256, 256) and ops.stcs_torus(32, 128, 128, 4, 4) == (128, 512, 512)
    assert callable(inference.infer_event_ensemble)
    assert os.path.exists(os.path.join(os.path.dirname(PKG), "tools", "stkrig_cs_bench.py"))
