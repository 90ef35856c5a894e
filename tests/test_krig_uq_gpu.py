"""Kriging variance maps and leave-one-out (LOO) cross-validation on the GPU (models/classical.py on csrc/krig_uq.hip) against the fp64
numpy restatement (tests/krig_uq_ref.py), on the cases of tests/test_classical_gpu.py.

Error bound of every comparison, the rule of the classical baselines: device error <= max(32 e32, 1e-6) scale, with e32 the fp32
restatement's own error against fp64 relative to the same scale, computed in the same test.  scale = c00 = psill + nugget of the
frame's sample for variances, max|z| of the case for LOO predictions; LOO variances are compared relatively."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import krig_uq_ref as kr
import test_classical_gpu as tc
from conftest import PKG

pytestmark = pytest.mark.gpu

VARIOGRAMS = tc.VARIOGRAMS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def uq_ref(tag, vkey):
    """((var, c00, loo) in fp64, (var, loo) in fp32) of a case; built once, never modified."""
    _, masked, masks = tc.case(tag)
    v64, c00, l64 = kr.kriging_uq(masked, masks, VARIOGRAMS[vkey], np.float64)
    v32, _, l32 = kr.kriging_uq(masked, masks, VARIOGRAMS[vkey], np.float32)
    return (v64, c00, l64), (v32, l32)


def _tensors(tag, dev):
    _, masked, masks = tc.case(tag)
    return torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)


def _rel(e32):
    return max(32.0 * e32, 1e-6)


def check_variance(tag, what, got, ref64, ref32, c00, masks):
    """got, ref: (B, T, 1, H, W); the NaN frames agree, gauge pixels are exactly 0, nothing is negative, the rest is within the bound."""
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), (tag, what, "NaN frames differ")
    scale = c00[:, :, None, None, None]
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.abs(got.astype(np.float64) - ref64) / scale, initial=0.0))
        e32 = float(np.nanmax(np.abs(ref32.astype(np.float64) - ref64) / scale, initial=0.0))
    print(f"{tag} {what} variance: device err {err:.3e}  e32 {e32:.3e}  bound {_rel(e32):.3e}  (of c00)")
    assert err <= _rel(e32), (tag, what, err, _rel(e32))
    assert not got[(masks != 0) & ~nan].any()
    assert (got[~nan] >= 0).all()
    return err, e32


def check_loo(tag, what, res, loo64, loo32):
    """res: the device's LOOResult; loo: per frame (z, pred, var) in raster order."""
    z, pred, var = (x.cpu().numpy() for x in (res.z, res.pred, res.var))
    counts = res.counts.cpu().numpy()
    assert len(loo64) == len(counts) == pred.shape[0]
    scale = max(float(np.abs(f[0]).max()) for f in loo64 if len(f[0]))
    err = e32 = verr = v32 = 0.0
    for f, ((zr, p64, s64), (_, p32, s32)) in enumerate(zip(loo64, loo32)):
        n = len(zr)
        assert counts[f] == n and np.array_equal(z[f, :n], zr)
        assert not pred[f, n:].any() and not var[f, n:].any()                    # zero past the count
        nan = np.isnan(p64)
        assert np.array_equal(np.isnan(pred[f, :n]), nan) and np.array_equal(np.isnan(var[f, :n]), nan), (tag, what, f)
        if n == 0 or nan.all():
            continue
        err = max(err, float(np.abs(pred[f, :n] - p64).max()))
        e32 = max(e32, float(np.abs(p32.astype(np.float64) - p64).max()))
        verr = max(verr, float(np.abs(var[f, :n] / s64 - 1.0).max()))
        v32 = max(v32, float(np.abs(s32.astype(np.float64) / s64 - 1.0).max()))
    e32 /= scale
    print(f"{tag} {what} LOO: prediction err {err:.3e}  e32 {e32 * scale:.3e}  bound {_rel(e32) * scale:.3e};  "
          f"variance rel err {verr:.3e}  e32 {v32:.3e}  bound {_rel(v32):.3e}")
    assert err <= _rel(e32) * scale, (tag, what, err)
    assert verr <= _rel(v32), (tag, what, verr)
    return _rel(e32) * scale


def _flat(loo, k):
    return np.concatenate([np.asarray(f[k], np.float64) for f in loo])


def check_scores(res, loo64, bound):
    """The score kernel against numpy on the device's own arrays (1e-12), and against the restatement's scores within the bound of the
    predictions they are means of (|e| is within it gauge by gauge, and the RMSE is 1-Lipschitz in the residuals' RMS norm)."""
    got = res.scores()
    counts = res.counts.cpu().numpy()
    own = [np.concatenate([a[f, :n] for f, n in enumerate(counts)]) for a in (x.cpu().numpy() for x in (res.z, res.pred, res.var))]
    mine, ref = kr.scores(*own), kr.scores(_flat(loo64, 0), _flat(loo64, 1), _flat(loo64, 2))
    assert got["n"] == mine["n"] == ref["n"]
    for k in ("ME", "MAE", "RMSE", "MSDR"):
        assert abs(got[k] - mine[k]) <= 1e-12 * max(abs(mine[k]), mine["MAE"]), (k, got[k], mine[k])
    for k in ("ME", "MAE", "RMSE"):
        assert abs(got[k] - ref[k]) <= bound, (k, got[k], ref[k], bound)


@pytest.mark.parametrize("vkey", sorted(VARIOGRAMS))
@pytest.mark.parametrize("tag", ["block4", "gauge12", "perframe"])
def test_variance_and_loo(dev, tag, vkey):
    _, _, masks = tc.case(tag)
    (v64, c00, l64), (v32, l32) = uq_ref(tag, vkey)
    G = tc._model(dev, name="kriging", variogram=VARIOGRAMS[vkey])
    x, m = _tensors(tag, dev)
    pred, var = G.forward_uq(x, m)
    assert int(G.last_status.sum()) == 0 and G.last_status.numel() == (3 if tag == "perframe" else 2)
    assert pred.shape == var.shape == x.shape and var.dtype == torch.float32
    assert torch.equal(pred, G(x, m))
    check_variance(tag, vkey, var.cpu().numpy(), v64, v32, c00, masks)
    res = G.cross_validate(x, m)
    check_scores(res, l64, check_loo(tag, vkey, res, l64, l32))


@pytest.mark.parametrize("vkey", ["exponential-fit", "spherical-fixed"])
def test_per_frame_systems_equal_the_shared_path(dev, vkey):
    _, _, masks = tc.case("block4")
    (v64, c00, l64), (v32, l32) = uq_ref("block4", vkey)
    x, m = _tensors("block4", dev)
    a = tc._model(dev, name="kriging", variogram=VARIOGRAMS[vkey]).forward_uq(x, m)[1]
    G = tc._model(dev, name="kriging", variogram=VARIOGRAMS[vkey], share_sets=False)
    b = G.forward_uq(x, m)[1]
    assert G.last_status.numel() == 8
    _, e32 = check_variance("block4", vkey + " per frame", b.cpu().numpy(), v64, v32, c00, masks)
    assert float(((a - b).abs().cpu().numpy() / c00[:, :, None, None, None]).max()) <= _rel(e32)
    check_loo("block4", vkey + " per frame", G.cross_validate(x, m), l64, l32)


@pytest.mark.parametrize("vkey", ["exponential-fixed", "spherical-fixed"])
def test_tile_edges(dev, vkey):
    _, masked, masks = tc.case("tiles")
    (v64, c00, l64), (v32, l32) = uq_ref("tiles", vkey)
    G = tc._model(dev, name="kriging", variogram=VARIOGRAMS[vkey])
    x, m = _tensors("tiles", dev)
    var = G.forward_uq(x, m)[1].cpu().numpy()
    for i, n in enumerate(tc.TILE_COUNTS):
        print(f"N = {n}: variance err {float(np.abs(var[0, i] - v64[0, i]).max() / c00[0, i]):.3e} of c00")
    check_variance("tiles", vkey, var, v64, v32, c00, masks)
    res = G.cross_validate(x, m)
    bound = check_loo("tiles", vkey, res, l64, l32)
    pred = res.pred.cpu().numpy()
    assert tc.TILE_COUNTS[:2] == (1, 2)
    assert np.isfinite(var[0, 0]).all() and np.isnan(pred[0, 0])                 # one gauge: a variance, no LOO
    z2 = res.z.cpu().numpy()[1, :2]
    assert np.abs(pred[1, :2] - z2[::-1]).max() <= bound                         # two gauges: the other gauge's value


def test_largest_system(dev):
    _, _, masks = tc.case("largest")
    (v64, c00, l64), (v32, l32) = uq_ref("largest", "exponential-fit")
    G = tc._model(dev, name="kriging", variogram=VARIOGRAMS["exponential-fit"])
    x, m = _tensors("largest", dev)
    check_variance("largest", "exponential-fit", G.forward_uq(x, m)[1].cpu().numpy(), v64, v32, c00, masks)
    check_loo("largest", "exponential-fit", G.cross_validate(x, m), l64, l32)


@pytest.mark.parametrize("vkey", ["exponential-fit", "exponential-fixed"])
def test_edges(dev, vkey):
    _, masked, masks = tc.case("edges")
    (v64, c00, l64), (v32, l32) = uq_ref("edges", vkey)
    G = tc._model(dev, name="kriging", variogram=VARIOGRAMS[vkey])
    x, m = _tensors("edges", dev)
    pred, var = G.forward_uq(x, m)
    assert torch.equal(pred, G(x, m))                                            # the prediction keeps its fallbacks
    var = var.cpu().numpy()
    check_variance("edges", vkey, var, v64, v32, c00, masks)
    res = G.cross_validate(x, m)
    check_loo("edges", vkey, res, l64, l32)
    loo = res.pred.cpu().numpy()
    counts = res.counts.cpu().numpy()
    assert np.isnan(var[0, 0]).all() and counts[0] == 0                          # no gauges: no model
    assert counts[1] == 1 and np.isnan(loo[1, 0])                                # one gauge: nothing to leave out
    if VARIOGRAMS[vkey]["fit"]:                                                  # equal values: a degenerate sample
        assert int(G.last_fit["cand"][0]) == -1
        assert np.isnan(var[0, 2]).all() and np.isnan(loo[2, :counts[2]]).all()
    else:
        assert np.isfinite(var[0, 1]).all() and np.isfinite(var[0, 2]).all()


def test_two_calls_are_identical(dev):
    for tag in ("block4", "perframe"):
        x, m = _tensors(tag, dev)
        for vg in (tc.FITTED["exponential"], tc.FIXED["spherical"]):
            a = tc._model(dev, name="kriging", variogram=vg)
            b = tc._model(dev, name="kriging", variogram=vg)
            (pa, va), (pb, vb) = a.forward_uq(x, m), b.forward_uq(x, m)
            assert torch.equal(pa, pb) and torch.equal(va, vb), (tag, vg)
            ra, rb = a.cross_validate(x, m), b.cross_validate(x, m)
            assert torch.equal(ra.pred, rb.pred) and torch.equal(ra.var, rb.var) and ra.scores() == rb.scores(), (tag, vg)
        ra, rb = (tc._model(dev, name="idw", power=1.5).cross_validate(x, m) for _ in range(2))
        assert torch.equal(ra.pred, rb.pred)


@pytest.mark.parametrize("power", [2.0, 1.5])
@pytest.mark.parametrize("tag", ["block4", "perframe", "edges"])
def test_idw_cross_validate(dev, tag, power):
    _, masked, masks = tc.case(tag)
    l64, l32 = kr.idw_loo(masked, masks, power, np.float64), kr.idw_loo(masked, masks, power, np.float32)
    x, m = _tensors(tag, dev)
    res = tc._model(dev, name="idw", power=power).cross_validate(x, m)
    assert res.var is None and res.status is None
    pred, counts = res.pred.cpu().numpy(), res.counts.cpu().numpy()
    scale = max(float(np.abs(f[0]).max()) for f in l64 if len(f[0]))
    err = e32 = 0.0
    for f, ((zr, p64), (_, p32)) in enumerate(zip(l64, l32)):
        n = len(zr)
        assert counts[f] == n and not pred[f, n:].any()
        assert np.array_equal(np.isnan(pred[f, :n]), np.isnan(p64))
        if n >= 2:
            err = max(err, float(np.abs(pred[f, :n] - p64).max()))
            e32 = max(e32, float(np.abs(p32.astype(np.float64) - p64).max()))
    print(f"{tag} idw power {power} LOO: device err {err:.3e}  e32 {e32:.3e}  bound {_rel(e32 / scale) * scale:.3e}")
    assert err <= _rel(e32 / scale) * scale
    got, ref = res.scores(), kr.scores(_flat(l64, 0), _flat(l64, 1))
    assert got["n"] == ref["n"] and "MSDR" not in got
    assert abs(got["RMSE"] - ref["RMSE"]) <= _rel(e32 / scale) * scale


def test_loo_scores_kernel(dev):
    """[5][64] with ragged counts, NaN entries and one empty frame: n exactly, the sums to 1e-12 relative."""
    from p2igan_bench import ops
    rng = np.random.default_rng(17)
    z, pred = rng.random((5, 64), dtype=np.float32), rng.random((5, 64), dtype=np.float32)
    var = (0.01 + rng.random((5, 64), dtype=np.float32)).astype(np.float32)
    counts = np.array([64, 0, 17, 33, 1], np.int32)
    pred[0, 5] = pred[2, 16] = pred[3, 40] = np.nan          # (3, 40) lies past its count: not counted anyway
    var[0, 9] = var[4, 0] = np.nan
    t = [torch.from_numpy(a).to(dev) for a in (z, pred, var, counts)]
    for with_var in (True, False):
        got = ops.loo_scores(t[0], t[1], t[2] if with_var else None, t[3]).cpu().numpy()
        keep = np.arange(64)[None, :] < counts[:, None]
        keep &= ~np.isnan(pred) & (~np.isnan(var) if with_var else True)
        e = z.astype(np.float64)[keep] - pred.astype(np.float64)[keep]
        ref = np.array([keep.sum(), e.sum(), np.abs(e).sum(), (e * e).sum(), (e * e / var.astype(np.float64)[keep]).sum() if with_var else 0.0])
        assert got[0] == ref[0] == (64 + 17 + 33 + 1 - (4 if with_var else 2))
        assert np.abs(got[1:] - ref[1:]).max() <= 1e-12 * np.abs(ref[1:]).max(), (got, ref)


def test_scripts_end_to_end(dev, tmp_path):
    """crossvalidate.py and infer.py --variance-output on a synthetic two-event store at 32 x 32."""
    from p2igan_bench.data import synth_store, zarr_lite
    from p2igan_bench.data.dataloader import P2IDataModule
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import crossvalidate as cv_script
    import infer as infer_script
    store = tmp_path / "test.zarr"
    synth_store.write_test_zarr(str(store), n_events=2, frames_per_event=20, h=32, w=32)
    paths = {}
    for name in ("kriging", "idw"):
        cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", f"{name}_baseline.json")))
        cfg["data"]["test"].update(w=32, h=32, data_root=str(store))
        cfg["data"]["test"]["mask"]["block_sizes"] = [4]
        paths[name] = tmp_path / f"{name}.json"
        json.dump(cfg, open(paths[name], "w"))
    cfg = json.load(open(paths["kriging"]))
    # the restatement on the same masks: the scripts seed the global generators before the loader draws them
    np.random.seed(cfg["seed"])
    chunks = []
    for batch in P2IDataModule(cfg).test_dataloader():
        _, masked, masks = [t.permute(0, 1, 4, 2, 3).contiguous() for t in batch]
        chunks.append([(masked[:, s:s + 16].contiguous(), masks[:, s:s + 16].contiguous()) for s in range(0, masked.shape[1], 16)])
    assert len(chunks) == 2 and [len(c) for c in chunks] == [2, 2]
    z, p64, p32, v64 = [], [], [], []
    for ev in chunks:
        for masked, masks in ev:
            for dt, out in ((np.float64, p64), (np.float32, p32)):
                _, _, loo = kr.kriging_uq(masked.numpy(), masks.numpy(), cfg["model"]["variogram"], dt)
                out.append(_flat(loo, 1))
                if dt is np.float64:
                    z.append(_flat(loo, 0)), v64.append(_flat(loo, 2))
    z, p64, p32, v64 = (np.concatenate(a) for a in (z, p64, p32, v64))
    ref = kr.scores(z, p64, v64)
    e32 = float(np.abs(p32 - p64).max()) / float(np.abs(z).max())

    out = tmp_path / "loo"
    cv_script.main(["--config", str(paths["kriging"]), "--output", str(out), "--stride", "16"])
    for name in ("loo.json", "loo.txt", "loo_data.npz"):
        assert (out / name).exists()
    res = json.load(open(out / "loo.json"))
    assert sorted(res["events"]) == ["event_01", "event_02"] and 0 < res["overall"]["n"] == ref["n"] <= 2 * 20 * 64
    bound = _rel(e32) * float(np.abs(z).max()) * 255.0
    print(f"loo.json overall RMSE {res['overall']['RMSE']:.6f}  restatement {ref['RMSE'] * 255.0:.6f}  bound {bound:.3e}")
    assert abs(res["overall"]["RMSE"] - ref["RMSE"] * 255.0) <= bound
    assert np.isfinite([res["overall"][k] for k in ("ME", "MAE", "MSDR", "ME_mmhr", "MAE_mmhr", "RMSE_mmhr")]).all()
    data = np.load(out / "loo_data.npz")
    assert np.array_equal(data["z"], z.astype(np.float32)) and data["frame"].max() == 19 and set(data["event"]) == {1, 2}
    assert np.abs(data["pred"] - p64).max() <= _rel(e32) * float(np.abs(z).max())

    infer_script.main(["--config", str(paths["kriging"]), "--output", str(tmp_path / "k.zarr"), "--variance-output", str(tmp_path / "kv.zarr")])
    main, var = zarr_lite.Group(str(tmp_path / "k.zarr")), zarr_lite.Group(str(tmp_path / "kv.zarr"))
    G = tc._model(dev, **cfg["model"])
    for i, ev in enumerate(chunks):
        key = f"event_{i + 1:02d}"
        got = var[key][:]
        assert got.shape == main[key][:].shape == (20, 1, 32, 32) and got.dtype == np.float32
        want = torch.cat([G.forward_uq(a.to(dev), b.to(dev))[1][0] for a, b in ev], dim=0) * 255.0 ** 2
        assert np.array_equal(got, want.cpu().numpy())
    with pytest.raises(FileExistsError):
        infer_script.main(["--config", str(paths["kriging"]), "--output", str(tmp_path / "k2.zarr"), "--variance-output", str(tmp_path / "kv.zarr")])
    with pytest.raises(RuntimeError, match="--variance-output needs model.name 'kriging'"):
        infer_script.main(["--config", str(paths["idw"]), "--output", str(tmp_path / "i.zarr"), "--variance-output", str(tmp_path / "iv.zarr")])
    assert not (tmp_path / "i.zarr").exists() and not (tmp_path / "iv.zarr").exists()
