"""Moving-neighbourhood space-time kriging (model.name: localkriging, csrc/lkrig.hip) on the GPU against the
numpy restatement tests/lkriging_ref.py.  Every prediction and variance is held to the project's rule: error <= max(32 e32, 1e-6) x
scale against the fp64 restatement, e32 the float32 restatement's error on the same case, scale max|ref| for predictions and c00 for
variances (leave-one-site-out variances relatively, as DESIGN.md section 16 does).  The kernel's own selection (last_neighbours) is
compared exactly in every case."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import lkriging_ref as lr
import stkriging_loso_ref as slr
import stkriging_ref as sr
import test_krig_uq_gpu as tu
from conftest import PKG
from test_localkriging_cpu import lattice_case

pytestmark = pytest.mark.gpu

FIXED = {"exponential": {"model": "exponential", "fit": False, "nugget": 0.01, "psill": 0.8, "range": 6.0, "time_scale": 1.5},
         "spherical": {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 1.3, "range": 9.0, "time_scale": 0.5}}
FITTED = {m: {"model": m, "fit": True, "n_lags": 16, "n_tlags": 3} for m in FIXED}
VARIOGRAMS = {f"{m}-{k}": v[m] for m in FIXED for k, v in (("fixed", FIXED), ("fit", FITTED))}
FCAP = 1024              # the device's slots per frame at the default model.max_points


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def field(B, T, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f = np.stack([[0.5 + 0.3 * np.sin((yy + t + 2 * b) / 3.0) * np.cos((xx - 0.5 * t) / 4.0) for t in range(T)] for b in range(B)])
    return (f + 0.05 * rng.standard_normal(f.shape)).astype(np.float32).reshape(B, T, 1, h, w)


def counts_masks(counts, h, w, seed):
    """(1, T, 1, h, w) masks with counts[t] gauges in frame t at sites drawn per frame."""
    rng = np.random.default_rng(seed)
    m = np.zeros((1, len(counts), 1, h, w), np.float32)
    for t, n in enumerate(counts):
        m[0, t, 0].ravel()[rng.permutation(h * w)[:n]] = 1.0
    return m


def model(dev, variogram, k, frames, name="localkriging", **more):
    from p2igan_bench.models import build_generator
    return build_generator({"model": dict(name=name, variogram=variogram, neighbourhood={"k": k, "frames": frames}, **more)}).to(dev)


def c00_of(masked, masks, variogram):
    """psill + nugget per sample (NaN where the fit is degenerate)."""
    out = []
    for b in range(masked.shape[0]):
        _, p = slr.sample_params(masked, masks, b, variogram)
        out.append(np.nan if p is None else p[0] + p[1])
    return np.array(out)


def check(tag, dev, masked, masks, variogram, k, frames, every=1):
    """forward_uq, forward (with the selection) and a second run against the restatement; returns the device's (pred, var)."""
    B, T, _, h, w = masked.shape
    G = model(dev, variogram, k, frames)
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    pred, var = G.forward_uq(x, m)
    assert int(G.last_status.sum()) == 0 and G.last_status.shape == (B,) and G.last_neighbours is None
    again = G.forward(x, m, neighbours=True)
    nbr = G.last_neighbours.cpu().numpy()
    assert torch.equal(pred, again) and torch.equal(G(x, m), again) and G.last_neighbours is None
    v2 = G.forward_uq(x, m)[1]
    assert torch.equal(torch.nan_to_num(var, nan=-1.0), torch.nan_to_num(v2, nan=-1.0))
    pred, var = pred.cpu().numpy(), var.cpu().numpy()
    assert pred.shape == var.shape == (B, T, 1, h, w) and np.isfinite(pred).all()
    r64, v64, n64 = lr.localkriging(masked, masks, variogram, k, frames, np.float64, every, FCAP)
    r32, v32, _ = lr.localkriging(masked, masks, variogram, k, frames, np.float32, every)
    done = np.isfinite(r64)                       # every > 1: the restatement solved these targets only
    assert done.all() if every == 1 else done.sum() >= done.size // every
    assert np.array_equal(nbr.reshape(B, T, h * w, k)[done.reshape(B, T, h * w)], n64[done.reshape(B, T, h * w)]), (tag, "selection differs")
    top = float(np.abs(r64[done]).max()) or 1.0
    err = float(np.abs(pred[done] - r64[done]).max()) / top
    e32 = float(np.abs(r32[done].astype(np.float64) - r64[done]).max()) / top
    nan = np.isnan(v64)
    assert np.array_equal(np.isnan(var)[done], nan[done]), (tag, "NaN variances differ")
    scale = c00_of(masked, masks, variogram)[:, None, None, None, None]
    ok = done & ~nan
    with np.errstate(invalid="ignore"):
        verr = float((np.abs(var - v64) / scale)[ok].max(initial=0.0))
        ve32 = float((np.abs(v32.astype(np.float64) - v64) / scale)[ok].max(initial=0.0))
    print(f"{tag}: prediction err {err:.3e} e32 {e32:.3e} bound {tu._rel(e32):.3e} (of max|ref|); variance err {verr:.3e} e32 {ve32:.3e} "
          f"bound {tu._rel(ve32):.3e} (of c00)")
    assert err <= tu._rel(e32), (tag, err, tu._rel(e32))
    assert verr <= tu._rel(ve32), (tag, verr, tu._rel(ve32))
    assert not var[(masks != 0) & ok].any() and (var[ok] >= 0).all()               # exactly 0 on a gauge pixel in its own frame
    return pred, var


@pytest.mark.parametrize("k,frames", [(12, 2), (64, 4), (5, 0)])
def test_selection_on_the_lattice_of_ties(dev, k, frames):
    masked, masks = lattice_case()
    variogram = dict(FIXED["exponential"], time_scale=2.0)
    check(f"lattice k={k} frames={frames}", dev, masked[None], masks[None], variogram, k, frames)


@pytest.mark.parametrize("vkey", ["exponential-fixed", "spherical-fit"])
def test_random_masks_shared_and_per_frame(dev, vkey):
    """24 x 40, T = 4: sample 0 shares one mask over its frames, sample 1 draws one per frame; with the fit, kappa comes from it."""
    rng = np.random.default_rng(21)
    masks = np.zeros((2, 4, 1, 24, 40), np.float32)
    masks[0, :, 0].reshape(4, -1)[:, rng.permutation(960)[:45]] = 1.0
    masks[1] = counts_masks([40, 52, 33, 47], 24, 40, 22)[0]
    masked = field(2, 4, 24, 40, 23) * masks
    check(f"random {vkey}", dev, masked, masks, VARIOGRAMS[vkey], 20, 1)


SWEEP_COUNTS = {"small": (0, 1, 2), "mid": (31, 33, 65), "gap": (97, 0, 31)}      # "gap": a middle frame without gauges


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    masks = counts_masks(SWEEP_COUNTS[name], 16, 16, 31)
    return field(1, 3, 16, 16, 32) * masks, masks


@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("name", sorted(SWEEP_COUNTS))
def test_edge_sweep_of_k_against_frame_sizes(dev, name, k):
    masked, masks = sweep_case(name)
    check(f"sweep {name} k={k}", dev, masked, masks, FIXED["exponential"], k, 1)


@pytest.mark.parametrize("frames", [0, 1, 2, 6])
@pytest.mark.parametrize("name", ["mid", "gap"])
def test_edge_sweep_of_the_window(dev, name, frames):
    masked, masks = sweep_case(name)
    check(f"window {name} frames={frames}", dev, masked, masks, FIXED["spherical"], 32, frames)


def test_rules(dev):
    """All gauges in the last frame with frames = 0 (the other frames take the sample's gauge mean, NaN variance), and a sample without
    any gauge (zeros, NaN)."""
    masks = np.concatenate([counts_masks((0, 0, 19), 16, 16, 41), counts_masks((0, 0, 0), 16, 16, 42)])
    masked = field(2, 3, 16, 16, 43) * masks
    pred, var = check("rules", dev, masked, masks, FIXED["exponential"], 8, 0)
    mean = masked[0][masks[0] != 0].astype(np.float64).mean()
    assert np.abs(pred[0, :2] - mean).max() <= 1e-6 and np.isnan(var[0, :2]).all() and np.isfinite(var[0, 2]).all()
    assert not pred[1].any() and np.isnan(var[1]).all()
    flat = masks[:1] * np.float32(0.4)                                  # zero variance: a degenerate fitted sample
    pred, var = check("degenerate fit", dev, flat, masks[:1], FITTED["exponential"], 8, 2)
    assert np.abs(pred - np.float32(0.4)).max() <= 1e-6 and np.isnan(var).all()


@pytest.mark.parametrize("T", [1, 8, 17])
@pytest.mark.parametrize("vkey", sorted(VARIOGRAMS))
def test_models_nuggets_fits_and_lengths(dev, vkey, T):
    rng = np.random.default_rng(50 + T)
    masks = counts_masks(rng.integers(14, 27, T), 16, 16, 51 + T)
    masked = field(1, T, 16, 16, 52) * masks
    check(f"{vkey} T={T}", dev, masked, masks, VARIOGRAMS[vkey], 16, 2)


def test_the_point_cap_is_gone(dev):
    """32 x 32, T = 40, a gauge on every second pixel of every second row: 256 per frame, 10 240 points in the sample."""
    masks = np.zeros((1, 40, 1, 32, 32), np.float32)
    masks[..., ::2, ::2] = 1.0
    masked = field(1, 40, 32, 32, 61) * masks
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    with pytest.raises(ValueError, match="space-time points"):
        model(dev, FIXED["exponential"], 32, 2, name="stkriging")(x, m)
    pred, _ = check("no cap", dev, masked, masks, FIXED["exponential"], 32, 2, every=7)
    assert np.isfinite(pred).all()


def test_leave_one_site_out_beyond_32_frames(dev):
    """T = 40: sample 0 has 24 sites (one of them misses every third frame), sample 1 a single site (nothing is left: NaN)."""
    rng = np.random.default_rng(71)
    T, h, w = 40, 32, 32
    masks = np.zeros((2, T, 1, h, w), np.float32)
    sites = rng.permutation(h * w)[:24]
    masks[0, :, 0].reshape(T, -1)[:, sites] = 1.0
    masks[0, ::3, 0].reshape(-1, h * w)[:, sites[0]] = 0.0
    masks[1, :, 0, 9, 17] = 1.0
    masked = field(2, T, h, w, 72) * masks
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    with pytest.raises(ValueError, match="at most 32 frames"):
        model(dev, FIXED["exponential"], 16, 2, name="stkriging").cross_validate_sites(x, m)
    for vkey, k, frames in (("exponential-fixed", 16, 2), ("spherical-fixed", 64, 1)):
        G = model(dev, VARIOGRAMS[vkey], k, frames)
        res = G.cross_validate_sites(x, m)
        assert int(G.last_status.sum()) == 0
        l64 = lr.loso(masked, masks, VARIOGRAMS[vkey], k, frames, np.float64)
        l32 = lr.loso(masked, masks, VARIOGRAMS[vkey], k, frames, np.float32)
        tu.check_loo("T=40", f"{vkey} k={k}", res, [f[:3] for f in l64], [f[:3] for f in l32])
        site, counts = res.site.cpu().numpy(), res.counts.cpu().numpy()
        for f, n in enumerate(counts):
            assert np.array_equal(site[f, :n], l64[f][3]) and (site[f, n:] == -1).all()
        pred = res.pred.cpu().numpy()
        assert np.isnan(pred[T:, 0]).all() and np.isfinite(pred[:T][site[:T] >= 0]).all()
        got = res.scores()
        assert got["n"] == int(counts[:T].sum()) and np.isfinite([got["RMSE"], got["MSDR"]]).all()
        again = G.cross_validate_sites(x, m)
        assert torch.equal(torch.nan_to_num(res.pred, nan=-1.0), torch.nan_to_num(again.pred, nan=-1.0))
        assert torch.equal(torch.nan_to_num(res.var, nan=-1.0), torch.nan_to_num(again.var, nan=-1.0))


@pytest.mark.parametrize("vkey", ["exponential-fixed", "spherical-fixed"])
def test_whole_sample_neighbourhood_and_the_global_model_on_the_device(dev, vkey):
    """16 x 16, T = 3, 24 points, k = 64, frames = 2: the local and the global model each meet their bound against one fp64 reference."""
    masks = counts_masks((8, 8, 8), 16, 16, 81)
    masked = field(1, 3, 16, 16, 82) * masks
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    ref = sr.stkriging(masked, masks, VARIOGRAMS[vkey])[0]
    top = float(np.abs(ref).max())
    e_local = float(np.abs(lr.localkriging(masked, masks, VARIOGRAMS[vkey], 64, 2, np.float32)[0] - ref).max()) / top
    e_global = float(np.abs(sr.stkriging(masked, masks, VARIOGRAMS[vkey], np.float32)[0] - ref).max()) / top
    local = model(dev, VARIOGRAMS[vkey], 64, 2)(x, m).cpu().numpy()
    glob = model(dev, VARIOGRAMS[vkey], 64, 2, name="stkriging")(x, m).cpu().numpy()
    d_local, d_global = float(np.abs(local - ref).max()) / top, float(np.abs(glob - ref).max()) / top
    print(f"{vkey}: local err {d_local:.3e} (e32 {e_local:.3e}), global err {d_global:.3e} (e32 {e_global:.3e})")
    assert d_local <= tu._rel(e_local) and d_global <= tu._rel(e_global)


def test_scripts_end_to_end(dev, tmp_path):
    """infer.py --variance-output and crossvalidate.py --by-site --stride 40 on a synthetic two-event store at 32 x 32."""
    from p2igan_bench.data import synth_store, zarr_lite
    from p2igan_bench.data.dataloader import P2IDataModule
    from p2igan_bench.models import build_generator
    from p2igan_bench.models.classical import LOCAL_NO_LOO
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import crossvalidate as cv_script
    import infer as infer_script
    store = tmp_path / "test.zarr"
    synth_store.write_test_zarr(str(store), n_events=2, frames_per_event=40, h=32, w=32)
    paths = {}
    for name in ("localkriging", "idw"):
        cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", f"{name}_baseline.json")))
        cfg["data"]["test"].update(w=32, h=32, data_root=str(store))
        cfg["data"]["test"]["mask"]["block_sizes"] = [4]
        paths[name] = tmp_path / f"{name}.json"
        json.dump(cfg, open(paths[name], "w"))
    cfg = json.load(open(paths["localkriging"]))
    np.random.seed(cfg["seed"])                   # the scripts seed the global generators before the loader draws the masks
    events = []
    for batch in P2IDataModule(cfg).test_dataloader():
        _, masked, masks = [t.permute(0, 1, 4, 2, 3).contiguous() for t in batch]
        events.append((masked, masks))
    assert len(events) == 2 and events[0][0].shape[1] == 40

    infer_script.main(["--config", str(paths["localkriging"]), "--output", str(tmp_path / "l.zarr"), "--variance-output", str(tmp_path / "lv.zarr")])
    main, var = zarr_lite.Group(str(tmp_path / "l.zarr")), zarr_lite.Group(str(tmp_path / "lv.zarr"))
    G = build_generator(cfg).to(dev)
    for i, (masked, masks) in enumerate(events):
        key = f"event_{i + 1:02d}"
        got = var[key][:]
        assert got.shape == main[key][:].shape == (40, 1, 32, 32) and got.dtype == np.float32
        want = torch.cat([G.forward_uq(masked[:, s:s + 16].contiguous().to(dev), masks[:, s:s + 16].contiguous().to(dev))[1][0]
                          for s in range(0, 40, 16)], dim=0) * 255.0 ** 2
        assert np.array_equal(got, want.cpu().numpy(), equal_nan=True) and np.isfinite(got).any()

    out = tmp_path / "loso"
    cv_script.main(["--config", str(paths["localkriging"]), "--output", str(out), "--by-site", "--stride", "40"])
    for name in ("loso.json", "loso.txt", "loso_data.npz"):
        assert (out / name).exists()
    res = json.load(open(out / "loso.json"))
    assert sorted(res["events"]) == ["event_01", "event_02"] and res["overall"]["n"] > 0
    assert np.isfinite([res["overall"][k] for k in ("ME", "MAE", "RMSE", "MSDR")]).all()
    with pytest.raises(RuntimeError) as e:
        cv_script.main(["--config", str(paths["localkriging"]), "--output", str(tmp_path / "loo"), "--stride", "16"])
    assert str(e.value) == LOCAL_NO_LOO
    with pytest.raises(RuntimeError, match="--variance-output needs model.name 'kriging'"):
        infer_script.main(["--config", str(paths["idw"]), "--output", str(tmp_path / "i.zarr"), "--variance-output", str(tmp_path / "iv.zarr")])
    assert not (tmp_path / "i.zarr").exists() and not (tmp_path / "iv.zarr").exists()
