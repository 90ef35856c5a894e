"""The restatement behind the conditional-simulation kernels (tests/krig_cs_ref.py) against first principles,
fp64 numpy: Philox4x32-10 against the published known-answer vectors, members that honour the gauges, ensemble statistics against
the kriging mean, the kriging variance and the analytic posterior covariance, exact and clipped embeddings, and the independence of a
member from the ensemble size.  The package's surface is checked for its refusals; the numbers on the device are
tests/test_krig_cs_gpu.py's."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import krig_cs_ref as cs
import krig_uq_ref as ur
from conftest import PKG

H = W = 16
M = 2048
CASES = {"exponential": (0.05, 0.6, 3.0), "spherical": (0.02, 0.8, 9.0)}


def _gauges(n=12, seed=3, h=H, w=W):
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.permutation(h * w)[:n])
    return np.stack([idx // w, idx % w], axis=1), rng.random(n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _members(model):
    """(xy, z, Z (M, H, W) fp64) of the statistics case; built once, never modified."""
    xy, z = _gauges()
    return xy, z, cs.members_frame(xy, z, H, W, CASES[model], model, M, seed=11, stream=5)


def test_philox_known_answers():
    """Random123's kat_vectors, philox4x32 with 10 rounds: counter = key = 0, counter = key = all ones, and the digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert tuple(int(w) for w in cs.philox4x32_10(counter, key)) == want
    # the vectorised form: the three counters in one call under one key equal the calls one by one
    ctr = np.array([k[0] for k in kat], dtype=np.uint64).T
    both = cs.philox4x32_10(tuple(ctr), kat[2][1])
    for i in range(3):
        assert tuple(int(w[i]) for w in both) == tuple(int(w) for w in cs.philox4x32_10(kat[i][0], kat[2][1]))


@pytest.mark.parametrize("model", cr.MODELS)
def test_members_equal_z_at_the_gauges(model):
    xy, z, Z = _members(model)
    assert np.abs(Z[:, xy[:, 0], xy[:, 1]] - z[None, :].astype(np.float64)).max() <= 1e-12
    # and before the gauge pixels are written: the conditioning itself reproduces z
    raw = cs.members_frame(xy[:-1], z[:-1], H, W, CASES[model], model, 4, seed=11, stream=5)
    full = cs.members_frame(xy, z, H, W, CASES[model], model, 4, seed=11, stream=5)
    assert np.abs(raw - full).max() > 1e-3          # the last gauge matters, so the check below is not vacuous
    nugget, psill, rng = CASES[model]
    U = cs.unconditional(cs.spectrum(CASES[model], model, H, W)[0], 11, 5, 4, H, W)
    K = cr.covariance(xy, xy, nugget, psill, rng, model, np.float64)
    u = np.linalg.solve(K, np.ones(len(z)))
    v = np.linalg.solve(K, z[:, None] - U[:, xy[:, 0], xy[:, 1]].T)
    mu = v.sum(0) / u.sum()
    at = U[:, xy[:, 0], xy[:, 1]].T + mu[None, :] + K @ (v - mu[None, :] * u[:, None])
    assert np.abs(at - z[:, None]).max() <= 1e-12


@pytest.mark.parametrize("model", cr.MODELS)
def test_ensemble_statistics(model):
    """Six standard errors of each estimator at M = 2048 (a float64 prototype used 3.0 of them for the mean, 0.097 of 0.1875 for the
    variance and 0.087 c00 of 0.1875 c00 for the covariance)."""
    xy, z, Z = _members(model)
    params = CASES[model]
    c00 = params[0] + params[1]
    mean = cr.krige_frame(xy, z, H, W, params, model)
    var = ur.variance_frame(xy, H, W, params, model)[0]
    ok = var > 1e-3 * c00
    assert ok.sum() >= H * W // 2
    zs = float((np.abs(Z.mean(0) - mean)[ok] / np.sqrt(var[ok] / M)).max())
    vr = float(np.abs(Z.var(0, ddof=1)[ok] / var[ok] - 1.0).max())
    emp = np.cov(Z.reshape(M, H * W).T)
    cv = float(np.abs(emp - cs.posterior_covariance(xy, H, W, params, model)).max() / c00)
    d = (Z - mean[None]).reshape(M // 2, 2, -1)
    corr = float(np.corrcoef(d[:, 0].ravel(), d[:, 1].ravel())[0, 1])
    print(f"{model}: mean {zs:.2f} sigma  variance {vr:.4f} (bound {6 * np.sqrt(2 / (M - 1)):.4f})  covariance {cv:.4f} c00 "
          f"(bound {6 * np.sqrt(2 / M):.4f} c00)  pair correlation {corr:+.4f}")
    assert zs <= 6.0
    assert vr <= 6.0 * np.sqrt(2.0 / (M - 1))
    assert cv <= 6.0 * np.sqrt(2.0 / M)
    # the two members of a pair are independent: 1024 pairs of fields with a few tens of independent pixels each give the sample
    # correlation a standard error near 0.007; three of them
    assert abs(corr) <= 0.02


@pytest.mark.parametrize("model,rng,h,w", [("exponential", 3.0, 16, 16), ("spherical", 9.0, 16, 16), ("exponential", 5.0, 32, 32),
                                           ("spherical", 12.0, 24, 40), ("exponential", 4.0, 17, 23)])
def test_exact_embeddings_clip_nothing(model, rng, h, w):
    for nugget in (0.05, 0.0):
        A, rho = cs.spectrum((nugget, 0.6, rng), model, h, w, 2)
        assert rho == 0.0 and A.shape == (2 * h, 2 * w)
        c00 = float(np.float32(nugget)) + float(np.float32(0.6))     # the spectrum starts from the fp32 parameters
        assert abs((A * A).sum() - c00) <= 1e-12                     # sum lambda / (Sy Sx) = b[0, 0] = c00


def test_a_long_range_clips_and_a_wider_torus_clips_less():
    rho = [cs.spectrum((0.05, 0.6, 20.0), "exponential", 32, 32, e)[1] for e in (2, 3, 4)]
    print("clip share of exponential a = 20 at 32 x 32, e = 2, 3, 4:", rho)
    assert rho[0] > 0.0 and rho[2] < rho[0] and rho[1] < rho[0]
    A, _ = cs.spectrum((0.05, 0.6, 20.0), "exponential", 32, 32, 2)
    assert abs((A * A).sum() - (float(np.float32(0.05)) + float(np.float32(0.6)))) <= 1e-12       # the variance is restored after clipping


def test_a_member_does_not_depend_on_the_ensemble_size():
    xy, z = _gauges()
    a = cs.members_frame(xy, z, H, W, CASES["exponential"], "exponential", 3, seed=7, stream=(9 << 32) | 4)
    b = cs.members_frame(xy, z, H, W, CASES["exponential"], "exponential", 5, seed=7, stream=(9 << 32) | 4)
    assert np.array_equal(a, b[:3])
    assert np.array_equal(a[:2], cs.members_frame(xy, z, H, W, CASES["exponential"], "exponential", 2, seed=7, stream=(9 << 32) | 4))


def test_a_member_changes_with_the_stream_and_the_seed():
    xy, z = _gauges()
    base = cs.members_frame(xy, z, H, W, CASES["spherical"], "spherical", 2, seed=7, stream=4)
    for seed, stream in ((7, 5), (7, (1 << 32) | 4), (8, 4), ((1 << 32) | 7, 4)):
        other = cs.members_frame(xy, z, H, W, CASES["spherical"], "spherical", 2, seed=seed, stream=stream)
        assert np.abs(other - base).max() > 0.1, (seed, stream)


def test_the_batch_restatement_applies_the_frame_rules():
    masks = np.zeros((2, 2, 1, H, W), np.float32)
    xy, z = _gauges()
    masks[0, 1, 0, xy[:, 0], xy[:, 1]] = 1.0                         # sample 0: a frame without gauges, then a healthy one
    masks[1, :, 0, xy[:, 0], xy[:, 1]] = 1.0                         # sample 1: constant values, a degenerate fit
    masked = np.zeros_like(masks)
    masked[0, 1, 0, xy[:, 0], xy[:, 1]] = z
    masked[1] = 0.4 * masks[1]
    ens, rho = cs.ensemble(masked, masks, {"model": "exponential", "fit": True, "n_lags": 8}, 3, seed=1)
    assert np.isnan(ens[0, 0]).all() and np.isfinite(ens[0, 1]).all() and np.isnan(ens[1]).all()
    assert np.isfinite(rho[0]) and np.isnan(rho[1])
    assert np.array_equal(ens[0, 1][:, xy[:, 0], xy[:, 1]], np.broadcast_to(z.astype(np.float64), (3, len(z))))


def _kriging(**model):
    from p2igan_bench.models import build_generator
    return build_generator({"model": dict({"name": "kriging"}, **model)})


def test_forward_ensemble_refuses_cpu_tensors():
    G = _kriging()
    x = torch.zeros(1, 2, 1, H, W)
    with pytest.raises(RuntimeError, match="HIP path only"):
        G.forward_ensemble(x, x, 3)


@pytest.mark.parametrize("embed", [1, 5, 2.0, "2", True, None])
def test_a_bad_embed_is_refused(embed):
    with pytest.raises(ValueError, match="embed"):
        _kriging(ensemble={"embed": embed})


def test_embed_is_read_from_the_config():
    assert _kriging().embed == 2 and _kriging(ensemble={}).embed == 2 and _kriging(ensemble={"embed": 3}).embed == 3
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "kriging_ensemble.json")))
    assert cfg["model"]["name"] == "kriging" and _kriging(**cfg["model"]).embed == cfg["model"]["ensemble"]["embed"]
    with pytest.raises(ValueError, match="ensemble"):
        _kriging(ensemble=[2])


def test_a_torus_past_512_is_refused_before_any_launch():
    x = torch.zeros(1, 1, 1, 257, 16)                                # CPU tensors: the size is looked at first
    with pytest.raises(ValueError, match="512"):
        _kriging().forward_ensemble(x, x, 2)
    x = torch.zeros(1, 1, 1, 16, 129)
    with pytest.raises(ValueError, match="512"):
        _kriging(ensemble={"embed": 4}).forward_ensemble(x, x, 2)
    with pytest.raises(RuntimeError, match="HIP path only"):        # 128 x 4 = 512 fits
        _kriging(ensemble={"embed": 4}).forward_ensemble(torch.zeros(1, 1, 1, 16, 128), torch.zeros(1, 1, 1, 16, 128), 2)


@pytest.mark.parametrize("members", [0, 65, -1, 2.0, True])
def test_members_outside_1_to_64_are_refused(members):
    x = torch.zeros(1, 2, 1, H, W)
    with pytest.raises(ValueError, match="members"):
        _kriging().forward_ensemble(x, x, members)


def test_only_kriging_has_forward_ensemble():
    from p2igan_bench.models import CLASSICAL
    from p2igan_bench.models.classical import KrigingGenerator
    assert [n for n, c in CLASSICAL.items() if hasattr(c, "forward_ensemble")] == ["kriging"]
    assert CLASSICAL["kriging"] is KrigingGenerator


def test_infer_refuses_an_ensemble_of_another_model(tmp_path):
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import infer as infer_script
    idw = os.path.join(PKG, "p2igan_bench", "config", "idw_baseline.json")
    with pytest.raises(RuntimeError, match="--ensemble-output needs model.name 'kriging'"):
        infer_script.main(["--config", idw, "--output", str(tmp_path / "i.zarr"), "--ensemble-output", str(tmp_path / "ens"), "--members", "3"])
    assert not (tmp_path / "i.zarr").exists() and not (tmp_path / "ens").exists()
    krig = os.path.join(PKG, "p2igan_bench", "config", "kriging_ensemble.json")
    for extra in ([], ["--members", "0"], ["--members", "65"]):
        with pytest.raises(ValueError, match="--members"):
            infer_script.main(["--config", krig, "--output", str(tmp_path / "k.zarr"), "--ensemble-output", str(tmp_path / "ens")] + extra)
    assert not (tmp_path / "k.zarr").exists() and not (tmp_path / "ens").exists()


def test_the_surface_exists():
    from p2igan_bench import _hip, inference, ops
    for name in ("p2i_krig_cs_spectrum", "p2i_krig_cs_noise", "p2i_krig_cs_fields", "p2i_krig_cs_weights", "p2i_krig_cs_predict"):
        assert name in _hip.SIGNATURES
        assert callable(getattr(ops, name[4:]))
    assert callable(inference.infer_event_ensemble)
    assert os.path.exists(os.path.join(os.path.dirname(PKG), "tools", "krig_cs_bench.py"))
