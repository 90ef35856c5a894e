"""Space-time ordinary kriging on the GPU (SpaceTimeKrigingGenerator on csrc/stkrig.hip and csrc/classical.hip's shared Cholesky)
against the fp64 numpy restatement (tests/stkriging_ref.py).

Error bound of every prediction, as in test_classical_gpu.py: max(32 e32, 1e-6) max|ref|, with e32 the fp32 restatement's own error
against fp64 relative to max|ref|, computed in the same test; both are printed beside the device error."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import stkriging_ref as sr
from conftest import PKG

pytestmark = pytest.mark.gpu

FIXED = {"exponential": {"model": "exponential", "fit": False, "nugget": 0.01, "psill": 0.8, "range": 6.0, "time_scale": 2.0},
         "spherical": {"model": "spherical", "fit": False, "nugget": 0.01, "psill": 0.8, "range": 10.0, "time_scale": 0.5},
         "spherical-k8": {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 12.0, "time_scale": 8.0}}
FITTED = {m: {"model": m, "fit": True, "n_lags": 16, "n_tlags": 3} for m in cr.MODELS}
VARIOGRAMS = {**{f"{k}-fixed": v for k, v in FIXED.items()}, **{f"{k}-fit": v for k, v in FITTED.items()}}
TILE_COUNTS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 97)
TILE_SPLITS = {31: (20, 0, 11), 32: (0, 0, 32)}          # a middle frame without gauges; every gauge in the last frame
GROUP_T = (1, 8, 9, 17)                                  # around the predictor's group of 8 target frames


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _tile_split(n):
    if n in TILE_SPLITS:
        return TILE_SPLITS[n]
    a, b = n * 5 // 10, n * 2 // 10
    return a, b, n - a - b


def _random_masks(rng, b, t, h, w, counts):
    m = np.zeros((b, t, h * w), np.float32)
    for i in range(b):
        for j in range(t):
            m[i, j, rng.permutation(h * w)[:counts[i][j]]] = 1.0
    return torch.from_numpy(m.reshape(b, t, 1, h, w))


@functools.lru_cache(maxsize=None)
def case(tag):
    """(frames, masked, masks) as (B, T, 1, H, W) fp32 numpy arrays; built once, never modified."""
    from p2igan_bench.utils import seeded
    if tag == "tiles":
        b, t, h, w = len(TILE_COUNTS), 3, 16, 16
        frames = (seeded.synthetic_event(b * t, h, w).float() / 255.0).reshape(b, t, 1, h, w)
        masks = _random_masks(np.random.default_rng(5), b, t, h, w, [_tile_split(n) for n in TILE_COUNTS])
    elif tag == "mixed":          # sample 0: one mask shared by its frames; sample 1: a mask per frame
        b, t, h, w = 2, 4, 24, 40
        frames = (seeded.synthetic_event(b * t, h, w).float() / 255.0).reshape(b, t, 1, h, w)
        masks = torch.from_numpy((np.random.default_rng(11).random((b, t, 1, h, w)) < 0.04).astype(np.float32))
        masks[0] = masks[0, 0]
    elif tag.startswith("group"):
        t, h, w = int(tag[5:]), 16, 16
        frames = (seeded.synthetic_event(t, h, w).float() / 255.0).reshape(1, t, 1, h, w)
        masks = _random_masks(np.random.default_rng(17), 1, t, h, w, [[12] * t])
    elif tag in ("limit", "half-limit"):          # 1024 gauges per frame: N_st = 4096 with 4 frames, 2048 with 2
        t = 4 if tag == "limit" else 2
        return tuple(x.contiguous().numpy() for x in seeded.synthetic_batch(1, t, 64, 64, seeded.block_mask(64, 64, 2)))
    elif tag == "advect":         # a field that moves across the frames; sample 0 shares its mask, sample 1 has one per frame
        b, t, h, w = 2, 5, 24, 40
        rng = np.random.default_rng(28)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        f = [[0.5 + 0.3 * np.sin((yy + k + 2.0 * i) / 3.0) * np.cos((xx - 0.5 * k + i) / 4.0) for k in range(t)] for i in range(b)]
        frames = torch.from_numpy(np.asarray(f, np.float32).reshape(b, t, 1, h, w))
        masks = torch.from_numpy((rng.random((b, t, 1, h, w)) < 0.05).astype(np.float32))
        masks[0] = masks[0, 0]
    else:
        raise KeyError(tag)
    return tuple(x.contiguous().numpy() for x in (frames, frames * masks, masks))


@functools.lru_cache(maxsize=None)
def st_ref(tag, vkey):
    """(fp64 prediction, fits, e32, bound) of a case."""
    _, masked, masks = case(tag)
    r64, fits = sr.stkriging(masked, masks, VARIOGRAMS[vkey], np.float64)
    r32, _ = sr.stkriging(masked, masks, VARIOGRAMS[vkey], np.float32)
    return (r64, fits) + _bound(r64, r32)


def _bound(r64, r32):
    top = float(np.abs(r64).max())
    e32 = float(np.abs(r32.astype(np.float64) - r64).max()) / max(top, 1e-30)
    return e32, max(32.0 * e32, 1e-6) * top


def _model(dev, **model):
    from p2igan_bench.models import build_generator
    return build_generator({"model": model}).to(dev)


def _run(G, tag, dev):
    _, masked, masks = case(tag)
    out = G(torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev))
    assert out.shape == masked.shape and out.dtype == torch.float32
    return out


def _check(tag, what, got, ref, e32, bound):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{tag} {what}: device err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}")
    assert np.isfinite(got).all() and err <= bound, (tag, what, err, bound)


@pytest.mark.parametrize("model", cr.MODELS)
def test_tile_edges(dev, model):
    _, masked, masks = case("tiles")
    assert [int(masks[i].sum()) for i in range(len(TILE_COUNTS))] == list(TILE_COUNTS)
    assert not masks[3, 1].any() and masks[3, 0].any() and masks[3, 2].any()               # N = 31: the middle frame is empty
    assert not masks[4, :2].any()                                                          # N = 32: all in the last frame
    vkey = f"{model}-fixed"
    ref, _, e32, bound = st_ref("tiles", vkey)
    G = _model(dev, name="stkriging", variogram=VARIOGRAMS[vkey])
    got = _run(G, "tiles", dev).cpu().numpy()
    for i, n in enumerate(TILE_COUNTS):
        print(f"N_st = {n}: device err {float(np.abs(got[i] - ref[i]).max()):.3e}")
    _check("tiles", vkey, got, ref, e32, bound)
    assert int(G.last_status.sum()) == 0 and G.last_status.numel() == len(TILE_COUNTS)     # one system per sample
    assert not got[0].any()                                                                # no point: zeros
    assert np.abs(got[1] - masked[1][masks[1] != 0][0]).max() <= bound                     # one point: its value in every frame
    assert np.abs(got[3, 1] - ref[3, 1]).max() <= bound and np.ptp(ref[3, 1]) > 100 * bound  # the empty frame is predicted from the others


@pytest.mark.parametrize("vkey", sorted(VARIOGRAMS))
def test_shared_and_per_frame_masks(dev, vkey):
    _, masked, masks = case("mixed")
    assert np.array_equal(masks[0, 0], masks[0, 3]) and not np.array_equal(masks[1, 0], masks[1, 3])
    ref, _, e32, bound = st_ref("mixed", vkey)
    G = _model(dev, name="stkriging", variogram=VARIOGRAMS[vkey])
    got = _run(G, "mixed", dev).cpu().numpy()
    _check("mixed", vkey, got, ref, e32, bound)
    assert int(G.last_status.sum()) == 0 and G.last_status.numel() == 2


@pytest.mark.parametrize("t", GROUP_T)
def test_frame_group_boundary(dev, t):
    tag = f"group{t}"
    for vkey in ("exponential-fixed", "spherical-k8-fixed"):
        ref, _, e32, bound = st_ref(tag, vkey)
        got = _run(_model(dev, name="stkriging", variogram=VARIOGRAMS[vkey]), tag, dev).cpu().numpy()
        _check(tag, vkey, got, ref, e32, bound)
        if t == 1:                # one frame: the spatial model with the same variogram, whatever kappa is
            _, masked, masks = case(tag)
            spatial = {k: v for k, v in VARIOGRAMS[vkey].items() if k != "time_scale"}
            s64, _ = cr.kriging(masked, masks, spatial, np.float64)
            e32s, bounds = _bound(s64, cr.kriging(masked, masks, spatial, np.float32)[0])
            other = _run(_model(dev, name="kriging", variogram=spatial), tag, dev).cpu().numpy()
            diff = float(np.abs(got.astype(np.float64) - other).max())
            print(f"{tag} {vkey}: |stkriging - kriging| {diff:.3e}  bounds {bound:.3e} + {bounds:.3e}")
            assert diff <= bound + bounds


@pytest.mark.parametrize("model", cr.MODELS)
def test_exact_at_a_gauge_in_its_own_frame_only(dev, model):
    vkey = f"{model}-fixed"
    assert VARIOGRAMS[vkey]["nugget"] > 0
    _, masked, masks = case("mixed")
    ref, _, e32, bound = st_ref("mixed", vkey)
    got = _run(_model(dev, name="stkriging", variogram=VARIOGRAMS[vkey]), "mixed", dev).cpu().numpy()
    at = masks != 0
    err = float(np.abs(got[at].astype(np.float64) - masked[at]).max())
    print(f"mixed {vkey}: err at the gauges {err:.3e}  bound {bound:.3e}")
    assert err <= bound
    # sample 1 has a mask per frame: the gauge pixels of frame 0 that are no gauges in frame 1 are not pinned to frame 0's values there
    # (a nugget term applied on the pixel alone would pin them); shown on the restatement first, then on the device
    only0 = (masks[1, 0] != 0) & (masks[1, 1] == 0)
    assert only0.sum() >= 10
    gap_ref = float(np.abs(ref[1, 1][only0] - masked[1, 0][only0]).max())
    gap = float(np.abs(got[1, 1][only0].astype(np.float64) - masked[1, 0][only0]).max())
    print(f"mixed {vkey}: next-frame gap at frame 0's gauge pixels, restatement {gap_ref:.3e}  device {gap:.3e}")
    assert gap_ref > 100 * bound and abs(gap - gap_ref) <= bound


def test_point_limit(dev):
    """64 x 64 with a block-2 mask has 1024 gauges per frame.  The fp64 and fp32 restatements at N_st = 4096 take about 18 s on the
    host together, so the comparison against them runs at N_st = 2048 (T = 2, fitted exponential); the full limit, N_st = 4096
    exactly (T = 4), is run twice and checked for finite, identical output and a factorisation without a failed pivot; T = 5 is
    refused on the host."""
    assert int(case("half-limit")[2].sum()) == 2048
    ref, fits, e32, bound = st_ref("half-limit", "exponential-fit")
    G = _model(dev, name="stkriging", variogram=VARIOGRAMS["exponential-fit"])
    got = _run(G, "half-limit", dev).cpu().numpy()
    print(f"half-limit: restatement (q, c) = {fits[0][:2]}, device cand {int(G.last_fit['cand'][0])}")
    _check("half-limit", "exponential-fit", got, ref, e32, bound)
    _, masked, masks = case("limit")
    assert int(masks.sum()) == 4096
    a = _run(G, "limit", dev)
    assert int(G.last_status.sum()) == 0 and int(G.last_fit["cand"][0]) >= 0
    b = _run(G, "limit", dev)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    at = masks != 0
    print(f"limit: max |out - z| at the gauges {float(np.abs(a.cpu().numpy()[at] - masked[at]).max()):.3e}")
    five = tuple(torch.from_numpy(np.concatenate([x, x[:, :1]], axis=1)).to(dev) for x in (masked, masks))
    with pytest.raises(ValueError, match=r"max_points.*--stride"):
        G(*five)
    with pytest.raises(ValueError, match="max_points"):                                   # a lower limit of the model's own
        _run(_model(dev, name="stkriging", max_points=4095, variogram=VARIOGRAMS["exponential-fit"]), "limit", dev)


@pytest.mark.parametrize("tag,model", [("mixed", "exponential"), ("advect", "exponential"), ("advect", "spherical")])
def test_variogram_bins_and_fit(dev, tag, model):
    _, masked, masks = case(tag)
    G = _model(dev, name="stkriging", variogram=FITTED[model])
    _run(G, tag, dev)
    bins, fit, cand, qd, cd = (G.last_fit[k].cpu().numpy() for k in ("bins", "fit", "cand", "q", "c"))
    h, w = masked.shape[-2:]
    lw = cr.lag_width(h, w, 16)
    for b in range(masked.shape[0]):
        frames = [cr.gauges(masked[b, t, 0], masks[b, t, 0]) for t in range(masked.shape[1])]
        n, sg, sh = sr.st_bins(frames, h, w, 16, 3)
        q, c, nug, ps, rng, kap, sse, sses = sr.fit_st(n, sg, sh, lw, model)
        runner_up = np.sort(sses.ravel())[1]
        print(f"{tag} {model} sample {b}: (q, c) ({q}, {c}) nugget {nug:.6e} psill {ps:.6e} range {rng:.4f} kappa {kap:.4f} sse {sse:.4e} "
              f"runner-up {runner_up:.4e}")
        assert runner_up - sse > 1e-3 * sse                                  # the indices are stable on these inputs
        assert bins.shape[1:] == (4, 16, 3) and np.array_equal(bins[b, :, :, 0], n)          # counts exactly
        assert np.abs(bins[b, :, :, 1] - sg).max() <= 1e-10 * np.abs(sg).max()
        assert np.abs(bins[b, :, :, 2] - sh).max() <= 1e-10 * np.abs(sh).max()
        assert (int(qd[b]), int(cd[b])) == (q, c) and int(cand[b]) == q * 25 + c
        assert abs(fit[b, 0] - nug) <= 1e-8 * abs(nug) and abs(fit[b, 1] - ps) <= 1e-8 * abs(ps)
        assert abs(fit[b, 2] - rng) <= 1e-12 * rng and abs(fit[b, 3] - kap) <= 1e-12 * kap


def test_one_frame_fits_as_the_spatial_model(dev):
    _, masked, masks = case("group1")
    G = _model(dev, name="stkriging", variogram=FITTED["exponential"])
    _run(G, "group1", dev)
    K = _model(dev, name="kriging", variogram={"model": "exponential", "fit": True, "n_lags": 16})
    _run(K, "group1", dev)
    assert int(G.last_fit["q"][0]) == 0 and int(G.last_fit["c"][0]) == int(K.last_fit["cand"][0]) >= 0
    assert G.last_fit["bins"].shape == (1, 1, 16, 3)                          # n_tlags is clipped to T - 1 = 0
    assert torch.equal(G.last_fit["bins"][:, 0, :, 0], K.last_fit["bins"][:, :, 0])


def test_zero_variance_sample_is_degenerate(dev):
    _, masked, masks = case("mixed")
    flat = masked.copy()
    flat[1] = 0.25 * masks[1]
    G = _model(dev, name="stkriging", variogram=FITTED["exponential"])
    got = G(torch.from_numpy(flat).to(dev), torch.from_numpy(masks).to(dev)).cpu().numpy()
    cand = G.last_fit["cand"].cpu().numpy()
    assert cand[0] >= 0 and cand[1] == -1
    assert np.abs(got[1] - np.float32(0.25)).max() <= 1e-6 * 0.25            # a degenerate sample predicts its gauge mean
    ref, _, _, bound = st_ref("mixed", "exponential-fit")
    assert np.abs(got[0].astype(np.float64) - ref[0]).max() <= bound         # the other sample is untouched by it


def test_two_runs_are_identical(dev):
    for tag in ("mixed", "group17"):
        for vg in (FITTED["exponential"], FIXED["spherical"]):
            a = _run(_model(dev, name="stkriging", variogram=vg), tag, dev)
            b = _run(_model(dev, name="stkriging", variogram=vg), tag, dev)
            assert torch.equal(a, b), (tag, vg)


def test_infer_script_writes_scorable_events(dev, tmp_path):
    from p2igan_bench.data import zarr_lite
    from p2igan_bench.data.dataloader import P2IDataModule
    from p2igan_bench.evaluation import run_exp1
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import infer as infer_script
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "stkriging_baseline.json")))
    for k in ("train", "test"):
        cfg["data"][k].update(w=32, h=32)
        cfg["data"][k]["mask"]["block_sizes"] = [4]
    cp = tmp_path / "stkriging.json"
    json.dump(cfg, open(cp, "w"))
    infer_script.main(["--config", str(cp), "--output", str(tmp_path / "stkriging.zarr"), "--stride", "8"])
    out = zarr_lite.Group(str(tmp_path / "stkriging.zarr"))
    assert out.attrs["checkpoint"] is None and out.attrs["model_name"] == "stkriging"
    preds = {k: out[k][:] for k in ("event_01", "event_02")}
    for arr in preds.values():
        assert arr.shape == (40, 1, 32, 32) and arr.dtype == np.float32 and np.isfinite(arr).all() and float(arr.min()) >= 0.0
    truth, mask = {}, None
    for i, batch in enumerate(P2IDataModule(cfg).test_dataloader()):
        truth[f"event_{i + 1:02d}"] = (batch[0][0, :, :, :, 0] * 255.0).round().numpy().astype(np.uint8)[:, None]
        mask = batch[2][0, 0, :, :, 0].numpy() != 0
    scores = run_exp1({"stkriging": preds}, truth, mask, "radar", 32)
    for key in ("MAE", "RMSE"):
        assert np.isfinite(float(scores["stkriging"][key])), (key, scores["stkriging"][key])
    with pytest.raises(RuntimeError, match="variance-output"):
        infer_script.main(["--config", str(cp), "--output", str(tmp_path / "x.zarr"), "--variance-output", str(tmp_path / "v.zarr")])
