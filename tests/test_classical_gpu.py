"""Classical baselines on the GPU (models/classical.py on csrc/classical.hip) against the fp64 numpy restatement
(tests/classical_ref.py).

Error bound of every comparison: max(32 e32, 1e-6) max|ref|, with e32 the fp32 restatement's own error against fp64 relative to
max|ref|, computed in the same test (the factor 32: the kernels' summation order and exp differ from LAPACK's and libm's)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
from conftest import PKG

pytestmark = pytest.mark.gpu

FIXED = {"exponential": {"model": "exponential", "fit": False, "nugget": 0.002, "psill": 0.05, "range": 6.0},
         "spherical": {"model": "spherical", "fit": False, "nugget": 0.001, "psill": 0.05, "range": 10.0}}
FITTED = {m: {"model": m, "fit": True, "n_lags": 16} for m in cr.MODELS}
VARIOGRAMS = {f"{m}-{k}": v[m] for m in cr.MODELS for k, v in (("fixed", FIXED), ("fit", FITTED))}
TILE_COUNTS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 130, 257)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(tag):
    """(frames, masked, masks) as (B, T, 1, H, W) fp32 numpy arrays; built once, never modified."""
    from p2igan_bench.utils import seeded
    if tag in ("block4", "gauge12"):
        mask = seeded.block_mask(32, 32, 4) if tag == "block4" else seeded.gauge_mask(32, 32, 12)
        out = seeded.synthetic_batch(2, 4, 32, 32, mask)
    elif tag in ("perframe", "edges"):
        t, h, w = 3, 24, 40
        frames = (seeded.synthetic_event(t, h, w).float() / 255.0).reshape(1, t, 1, h, w)
        masks = torch.from_numpy((np.random.default_rng(11).random((1, t, 1, h, w)) < 0.05).astype(np.float32))
        masked = frames * masks
        if tag == "edges":          # no gauge / one gauge / gauges that all hold the same value
            masks[0, 0] = 0.0
            masks[0, 1] = 0.0
            masks[0, 1, 0, 7, 19] = 1.0
            masked = frames * masks
            masked[0, 2] = 0.4 * masks[0, 2]
        out = (frames, masked, masks)
    elif tag == "tiles":
        t, h, w = len(TILE_COUNTS), 32, 32
        frames = (seeded.synthetic_event(t, h, w).float() / 255.0).reshape(1, t, 1, h, w)
        perm = np.random.default_rng(5).permutation(h * w)
        m = np.zeros((t, h * w), np.float32)
        for i, n in enumerate(TILE_COUNTS):
            m[i, perm[:n]] = 1.0
        masks = torch.from_numpy(m.reshape(1, t, 1, h, w))
        out = (frames, frames * masks, masks)
    elif tag == "largest":
        out = seeded.synthetic_batch(1, 1, 64, 64, seeded.block_mask(64, 64, 2))
    else:
        raise KeyError(tag)
    return tuple(x.contiguous().numpy() for x in out)


@functools.lru_cache(maxsize=None)
def krig_ref(tag, vkey):
    """(fp64 prediction, fits, e32, bound) of a case."""
    _, masked, masks = case(tag)
    r64, fits = cr.kriging(masked, masks, VARIOGRAMS[vkey], np.float64)
    r32, _ = cr.kriging(masked, masks, VARIOGRAMS[vkey], np.float32)
    return (r64, fits) + _bound(r64, r32)


@functools.lru_cache(maxsize=None)
def idw_ref(tag, power):
    _, masked, masks = case(tag)
    r64 = cr.idw(masked, masks, power, np.float64)
    return (r64,) + _bound(r64, cr.idw(masked, masks, power, np.float32))


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


@pytest.mark.parametrize("vkey", sorted(VARIOGRAMS))
@pytest.mark.parametrize("tag", ["block4", "gauge12"])
def test_shared_gauge_set(dev, tag, vkey):
    frames, masked, masks = case(tag)
    ref, _, e32, bound = krig_ref(tag, vkey)
    G = _model(dev, name="kriging", variogram=VARIOGRAMS[vkey])
    got = _run(G, tag, dev).cpu().numpy()
    _check(tag, vkey, got, ref, e32, bound)
    at = masks != 0
    assert float(np.abs(got[at].astype(np.float64) - masked[at]).max()) <= bound          # exact at gauges
    assert int(G.last_status.sum()) == 0 and G.last_status.numel() == 2                     # one system per sample
    rmse = float(np.sqrt(((got - frames).astype(np.float64) ** 2).mean()))
    base = float(np.sqrt(((cr.gauge_mean_predictor(masked, masks) - frames) ** 2).mean()))
    print(f"{tag} {vkey}: RMSE {rmse:.4f} against the gauge-mean predictor's {base:.4f}")
    assert rmse < base


@pytest.mark.parametrize("vkey", ["exponential-fit", "spherical-fixed", "spherical-fit", "exponential-fixed"])
@pytest.mark.parametrize("tag", ["perframe", "edges"])
def test_per_frame_sets_and_edges(dev, tag, vkey):
    _, masked, masks = case(tag)
    ref, fits, e32, bound = krig_ref(tag, vkey)
    G = _model(dev, name="kriging", variogram=VARIOGRAMS[vkey])
    got = _run(G, tag, dev).cpu().numpy()
    _check(tag, vkey, got, ref, e32, bound)
    assert G.last_status.numel() == 3 and int(G.last_status.sum()) == 0                     # one system per frame
    if tag == "edges":
        assert not got[0, 0].any()                                                         # no gauges: zeros
        assert np.abs(got[0, 1] - masked[0, 1, 0, 7, 19]).max() <= bound                   # one gauge: its value
        assert np.abs(got[0, 2] - np.float32(0.4)).max() <= bound                          # equal values: that value
        if VARIOGRAMS[vkey]["fit"]:
            assert fits[0][0] == -1 and int(G.last_fit["cand"][0]) == -1                   # no variance anywhere: degenerate


def test_tile_edges(dev):
    ref, _, e32, bound = krig_ref("tiles", "exponential-fixed")
    G = _model(dev, name="kriging", variogram=VARIOGRAMS["exponential-fixed"])
    got = _run(G, "tiles", dev).cpu().numpy()
    for i, n in enumerate(TILE_COUNTS):
        print(f"N = {n}: device err {float(np.abs(got[0, i] - ref[0, i]).max()):.3e}")
    _check("tiles", "exponential-fixed", got, ref, e32, bound)
    ref, _, e32, bound = krig_ref("tiles", "spherical-fixed")
    got = _run(_model(dev, name="kriging", variogram=VARIOGRAMS["spherical-fixed"]), "tiles", dev).cpu().numpy()
    _check("tiles", "spherical-fixed", got, ref, e32, bound)


def test_largest_system_and_the_point_limit(dev):
    _, masked, masks = case("largest")
    assert int(masks.sum()) == 1024
    ref, _, e32, bound = krig_ref("largest", "exponential-fit")
    G = _model(dev, name="kriging", variogram=VARIOGRAMS["exponential-fit"])
    _check("largest", "exponential-fit", _run(G, "largest", dev).cpu().numpy(), ref, e32, bound)
    more = masks.copy()
    more.reshape(-1)[int(np.flatnonzero(masks.reshape(-1) == 0)[0])] = 1.0
    assert int(more.sum()) == 1025
    for G in (G, _model(dev, name="idw", max_points=1024)):
        with pytest.raises(ValueError, match="max_points"):
            G(torch.from_numpy(masked).to(dev), torch.from_numpy(more).to(dev))


@pytest.mark.parametrize("model", cr.MODELS)
@pytest.mark.parametrize("tag", ["block4", "perframe"])
def test_variogram_bins_and_fit(dev, tag, model):
    _, masked, masks = case(tag)
    G = _model(dev, name="kriging", variogram=FITTED[model])
    _run(G, tag, dev)
    bins, fit, cand = (G.last_fit[k].cpu().numpy() for k in ("bins", "fit", "cand"))
    h, w = masked.shape[-2:]
    for b in range(masked.shape[0]):
        frames = [cr.gauges(masked[b, t, 0], masks[b, t, 0]) for t in range(masked.shape[1])]
        n, sg, sh = cr.variogram_bins(frames, h, w, 16)
        c, nug, ps, rng, sse, sses = cr.fit_bins(n, sg, sh, cr.lag_width(h, w, 16), model)
        runner_up = np.sort(sses)[1]
        print(f"{tag} {model} sample {b}: cand {c} nugget {nug:.6e} psill {ps:.6e} range {rng:.4f} sse {sse:.4e} runner-up {runner_up:.4e}")
        assert runner_up - sse > 1e-3 * sse                                  # the index is stable on these inputs
        assert np.array_equal(bins[b, :, 0], n)                              # counts exactly
        assert np.abs(bins[b, :, 1] - sg).max() <= 1e-10 * np.abs(sg).max()
        assert np.abs(bins[b, :, 2] - sh).max() <= 1e-10 * np.abs(sh).max()
        assert int(cand[b]) == c
        assert abs(fit[b, 0] - nug) <= 1e-8 * abs(nug) and abs(fit[b, 1] - ps) <= 1e-8 * abs(ps)
        assert abs(fit[b, 2] - rng) <= 1e-12 * rng


def test_zero_variance_sample_is_degenerate(dev):
    _, masked, masks = case("block4")
    flat = masked.copy()
    flat[1] = 0.25 * masks[1]
    G = _model(dev, name="kriging", variogram=FITTED["exponential"])
    got = G(torch.from_numpy(flat).to(dev), torch.from_numpy(masks).to(dev)).cpu().numpy()
    cand = G.last_fit["cand"].cpu().numpy()
    assert cand[0] >= 0 and cand[1] == -1
    assert np.abs(got[1] - np.float32(0.25)).max() <= 1e-6 * 0.25            # a degenerate sample predicts each frame's gauge mean
    ref, _, _, bound = krig_ref("block4", "exponential-fit")
    assert np.abs(got[0].astype(np.float64) - ref[0]).max() <= bound         # the other sample is untouched by it


@pytest.mark.parametrize("vkey", ["exponential-fit", "spherical-fixed"])
def test_shared_set_path_equals_per_frame_path(dev, vkey):
    ref, _, e32, bound = krig_ref("block4", vkey)
    a = _run(_model(dev, name="kriging", variogram=VARIOGRAMS[vkey]), "block4", dev)
    G = _model(dev, name="kriging", variogram=VARIOGRAMS[vkey], share_sets=False)
    b = _run(G, "block4", dev)
    assert G.last_status.numel() == 8
    _check("block4", vkey + " per frame", b.cpu().numpy(), ref, e32, bound)
    assert float((a - b).abs().max()) <= bound


@pytest.mark.parametrize("power", [2.0, 3.0])
@pytest.mark.parametrize("tag", ["block4", "gauge12", "perframe", "edges"])
def test_idw(dev, tag, power):
    _, masked, masks = case(tag)
    ref, e32, bound = idw_ref(tag, power)
    got = _run(_model(dev, name="idw", power=power), tag, dev).cpu().numpy()
    _check(tag, f"idw power {power}", got, ref, e32, bound)
    at = masks != 0
    assert np.array_equal(got[at], masked[at])                               # a gauge pixel takes its gauge's value
    if tag == "edges":
        assert not got[0, 0].any()


def test_two_runs_are_identical(dev):
    for tag in ("block4", "perframe"):
        for model in ({"name": "kriging", "variogram": FITTED["exponential"]}, {"name": "kriging", "variogram": FIXED["spherical"]},
                      {"name": "idw", "power": 3.0}):
            a = _run(_model(dev, **model), tag, dev)
            b = _run(_model(dev, **model), tag, dev)
            assert torch.equal(a, b), (tag, model)


def test_infer_script_writes_scorable_events_and_train_refuses(dev, tmp_path):
    from p2igan_bench.data import zarr_lite
    from p2igan_bench.data.dataloader import P2IDataModule
    from p2igan_bench.evaluation import run_exp1
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import infer as infer_script
    import train as train_script
    preds, truth, mask = {}, {}, None
    for name in ("kriging", "idw"):
        cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", f"{name}_baseline.json")))
        for k in ("train", "test"):
            cfg["data"][k].update(w=32, h=32)
            cfg["data"][k]["mask"]["block_sizes"] = [4]
        cp = tmp_path / f"{name}.json"
        json.dump(cfg, open(cp, "w"))
        infer_script.main(["--config", str(cp), "--output", str(tmp_path / f"{name}.zarr")])
        out = zarr_lite.Group(str(tmp_path / f"{name}.zarr"))
        assert out.attrs["checkpoint"] is None and out.attrs["model_name"] == name
        preds[name] = {k: out[k][:] for k in ("event_01", "event_02")}
        for arr in preds[name].values():
            assert arr.shape == (40, 1, 32, 32) and arr.dtype == np.float32 and np.isfinite(arr).all() and float(arr.min()) >= 0.0
        if not truth:
            for i, batch in enumerate(P2IDataModule(cfg).test_dataloader()):
                truth[f"event_{i + 1:02d}"] = (batch[0][0, :, :, :, 0] * 255.0).round().numpy().astype(np.uint8)[:, None]
                mask = batch[2][0, 0, :, :, 0].numpy() != 0
        if name == "kriging":
            with pytest.raises(RuntimeError, match="nothing to train"):
                train_script.main(["--config", str(cp)])
    scores = run_exp1(preds, truth, mask, "radar", 32)
    for name in ("kriging", "idw"):
        for key in ("MAE", "RMSE"):
            assert np.isfinite(float(scores[name][key])), (name, key, scores[name][key])
