"""Leave-one-site-out cross-validation of space-time kriging on the GPU (SpaceTimeKrigingGenerator.cross_validate_sites on
csrc/stkrig_loso.hip) against the fp64 numpy restatement (tests/stkriging_loso_ref.py).

Error bound, the rule of the classical baselines (test_krig_uq_gpu.py): device error <= max(32 e32, 1e-6) scale, with e32 the all-fp32
restatement's own error against fp64 on the same case, scale = max|z| for the predictions; the variances are held relatively.  No
point that the restatement predicts may come back NaN, and the reverse.  Every figure is printed beside its bound."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import krig_uq_ref as kr
import stkriging_loso_ref as lr
import stkriging_ref as sr
from conftest import PKG

pytestmark = pytest.mark.gpu

FIXED = {"exponential-k2": {"model": "exponential", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 6.0, "time_scale": 2.0},
         "exponential-k.5n": {"model": "exponential", "fit": False, "nugget": 0.01, "psill": 0.8, "range": 6.0, "time_scale": 0.5},
         "exponential-k8": {"model": "exponential", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 6.0, "time_scale": 8.0},
         "spherical-k2": {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 10.0, "time_scale": 2.0},
         "spherical-k.5n": {"model": "spherical", "fit": False, "nugget": 0.01, "psill": 0.8, "range": 10.0, "time_scale": 0.5},
         "spherical-k8": {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 12.0, "time_scale": 8.0}}
FITTED = {f"{m}-fit": {"model": m, "fit": True, "n_lags": 16, "n_tlags": 3} for m in cr.MODELS}
VARIOGRAMS = {**FIXED, **FITTED}
TILE_COUNTS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 97)       # points of a sample around the 32-wide tiles


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _site_masks(rng, t, h, w, mult):
    """(t, 1, h, w) masks of len(mult) sites at random pixels other than (0, 0); the site with the k-th smallest pixel is a gauge in
    mult[k] frames (all of them, or frames k, k + 1, ... modulo t)."""
    m = np.zeros((t, h * w), np.float32)
    for k, p in enumerate(np.sort(1 + rng.permutation(h * w - 1)[:len(mult)])):
        for j in range(mult[k]):
            m[(k + j) % t if mult[k] < t else j, p] = 1.0
    return m.reshape(t, 1, h, w)


def _values(b, t, h, w):
    from p2igan_bench.utils import seeded
    return (seeded.synthetic_event(b * t, h, w).float() / 255.0).numpy().reshape(b, t, 1, h, w)


@functools.lru_cache(maxsize=None)
def case(tag):
    """(masked, masks) as (B, T, 1, H, W) fp32 numpy arrays; built once, never modified."""
    if tag == "straddle":         # N = 33 twice: 11 shared sites (the last block is columns 30 .. 32); 16 sites in 1, 2 and 3 frames
        rng = np.random.default_rng(5)
        masks = np.stack([_site_masks(rng, 3, 16, 16, [3] * 11), _site_masks(rng, 3, 16, 16, [3] + [1, 2, 3] * 5)])
    elif tag == "tiles":          # n % 3 sites in one frame (they sort first and shift the blocks), then n // 3 sites in all three
        rng = np.random.default_rng(7)
        masks = np.stack([_site_masks(rng, 3, 16, 16, [1] * (n % 3) + [3] * (n // 3)) for n in TILE_COUNTS])
    elif tag in ("full", "full-shifted"):       # 5 sites in all 32 frames: five aligned 32-blocks; a gauge at pixel (0, 0) shifts them
        rng = np.random.default_rng(9)
        masks = _site_masks(rng, 32, 8, 8, [32] * 5)[None]
        assert not masks[0, :, 0, 0, 0].any()
        if tag == "full-shifted":
            masks[0, 0, 0, 0, 0] = 1.0
    elif tag == "mixed":          # sample 0: one mask shared by its frames; sample 1: a mask per frame
        masks = (np.random.default_rng(11).random((2, 4, 1, 24, 40)) < 0.04).astype(np.float32)
        masks[0] = masks[0, 0]
    elif tag == "rules":          # healthy, one site only, no gauges, constant values (degenerate when fitted)
        rng = np.random.default_rng(13)
        ok = _site_masks(rng, 3, 16, 16, [3, 1, 2] * 6)
        masks = np.stack([ok, _site_masks(rng, 3, 16, 16, [3]), np.zeros_like(ok), ok])
    elif tag == "one-frame":
        masks = _site_masks(np.random.default_rng(17), 1, 16, 16, [1] * 40)[None]
    else:
        raise KeyError(tag)
    masks = np.ascontiguousarray(masks, np.float32)
    values = _values(*masks.shape[:2], *masks.shape[3:])
    if tag == "rules":
        values[3] = 0.25
    return values * masks, masks


@functools.lru_cache(maxsize=None)
def loso_ref(tag, vkey):
    masked, masks = case(tag)
    return lr.loso(masked, masks, VARIOGRAMS[vkey], np.float64), lr.loso(masked, masks, VARIOGRAMS[vkey], np.float32)


def _rel(e32):
    return max(32.0 * e32, 1e-6)


def _model(dev, **model):
    from p2igan_bench.models import build_generator
    return build_generator({"model": model}).to(dev)


def _tensors(tag, dev):
    return tuple(torch.from_numpy(x).to(dev) for x in case(tag))


def check_loso(tag, what, res, rows64, rows32):
    """res: the device's LOOResult; rows: per frame (z, pred, var, site) in raster order.  Returns the prediction bound."""
    z, pred, var, site = (x.cpu().numpy() for x in (res.z, res.pred, res.var, res.site))
    counts = res.counts.cpu().numpy()
    assert len(rows64) == len(counts) == pred.shape[0]
    scale = max(float(np.abs(f[0]).max()) for f in rows64 if len(f[0]))
    err = e32 = verr = v32 = 0.0
    for f, ((zr, p64, s64, g64), (_, p32, s32, _)) in enumerate(zip(rows64, rows32)):
        n = len(zr)
        assert counts[f] == n and np.array_equal(z[f, :n], zr)
        assert not pred[f, n:].any() and not var[f, n:].any()                    # zero past the count
        assert np.array_equal(site[f, :n], g64) and (site[f, n:] == -1).all(), (tag, what, f)
        nan = np.isnan(p64)
        assert np.array_equal(np.isnan(pred[f, :n]), nan) and np.array_equal(np.isnan(var[f, :n]), nan), (tag, what, f)
        assert np.array_equal(np.isnan(p32), nan), "the fp32 yardstick lost a point"
        if n == 0 or nan.all():
            continue
        err = max(err, float(np.abs(pred[f, :n] - p64).max()))
        e32 = max(e32, float(np.abs(p32.astype(np.float64) - p64).max()))
        verr = max(verr, float(np.abs(var[f, :n] / s64 - 1.0).max()))
        v32 = max(v32, float(np.abs(s32.astype(np.float64) / s64 - 1.0).max()))
    e32 /= scale
    print(f"{tag} {what} LOSO: prediction err {err:.3e}  e32 {e32 * scale:.3e}  bound {_rel(e32) * scale:.3e};  "
          f"variance rel err {verr:.3e}  e32 {v32:.3e}  bound {_rel(v32):.3e}")
    assert err <= _rel(e32) * scale, (tag, what, err)
    assert verr <= _rel(v32), (tag, what, verr)
    return _rel(e32) * scale


def _flat(rows, k):
    return np.concatenate([np.asarray(f[k], np.float64) for f in rows])


def _run(dev, tag, vkey, **kw):
    G = _model(dev, name="stkriging", variogram=VARIOGRAMS[vkey], **kw)
    res = G.cross_validate_sites(*_tensors(tag, dev))
    return G, res


@pytest.mark.parametrize("vkey", ["exponential-k2", "spherical-k.5n"])
def test_blocks_straddle_the_tile_edge(dev, vkey):
    masked, masks = case("straddle")
    assert [int(m.sum()) for m in masks] == [33, 33]
    xy = sr.points(masked[0], masks[0])[0]
    assert len(np.unique(lr.site_index(xy))) == 11                                # 11 blocks of 3: the last is columns 30 .. 32
    sizes = np.bincount(lr.site_index(sr.points(masked[1], masks[1])[0]))
    assert sorted(set(sizes)) == [1, 2, 3] and sizes[-1] == 3
    G, res = _run(dev, "straddle", vkey)
    check_loso("straddle", vkey, res, *loso_ref("straddle", vkey))
    assert int(G.last_status.sum()) == 0 and G.last_status.numel() == 2


@pytest.mark.parametrize("vkey", ["exponential-k.5n", "spherical-k2"])
def test_tile_edges(dev, vkey):
    masked, masks = case("tiles")
    assert [int(m.sum()) for m in masks] == list(TILE_COUNTS)
    G, res = _run(dev, "tiles", vkey)
    r64, r32 = loso_ref("tiles", vkey)
    check_loso("tiles", vkey, res, r64, r32)
    pred = res.pred.cpu().numpy()
    assert not pred[:3].any()                                                     # no point: nothing to report
    assert np.isnan(pred[3, 0]) and np.isnan(res.var.cpu().numpy()[3, 0])         # one point: its only site holds it
    assert all(len(r64[f][1]) == 1 and np.isfinite(r64[f][1]).all() for f in (6, 7))      # two one-point sites predict each other
    assert int(G.last_status.sum()) == 0


@pytest.mark.parametrize("tag", ["full", "full-shifted"])
@pytest.mark.parametrize("vkey", ["exponential-k2", "spherical-k.5n"])
def test_full_width_blocks(dev, tag, vkey):
    masked, masks = case(tag)
    assert int(masks.sum()) == 160 + (tag == "full-shifted")
    sizes = np.bincount(lr.site_index(sr.points(masked[0], masks[0])[0]))
    assert list(sizes) == ([1] if tag == "full-shifted" else []) + [32] * 5
    G, res = _run(dev, tag, vkey)
    check_loso(tag, vkey, res, *loso_ref(tag, vkey))
    assert int(G.last_status.sum()) == 0


def test_more_than_32_frames_are_refused(dev):
    masked, masks = (torch.from_numpy(np.concatenate([x, x[:, :1]], axis=1)).to(dev) for x in case("full"))
    assert masked.shape[1] == 33
    G = _model(dev, name="stkriging", variogram=VARIOGRAMS["exponential-k2"])
    with pytest.raises(ValueError, match=r"at most 32 frames.*--stride"):
        G.cross_validate_sites(masked, masks)
    with pytest.raises(ValueError, match="max_points"):                           # the point limit is forward()'s
        _model(dev, name="stkriging", max_points=159, variogram=VARIOGRAMS["exponential-k2"]).cross_validate_sites(*_tensors("full", dev))


@pytest.mark.parametrize("vkey", sorted(VARIOGRAMS))
def test_models_and_parameters(dev, vkey):
    masked, masks = case("mixed")
    assert np.array_equal(masks[0, 0], masks[0, 3]) and not np.array_equal(masks[1, 0], masks[1, 3])
    G, res = _run(dev, "mixed", vkey)
    r64, r32 = loso_ref("mixed", vkey)
    bound = check_loso("mixed", vkey, res, r64, r32)
    assert int(G.last_status.sum()) == 0 and G.last_status.numel() == 2
    assert (G.last_fit is not None) == VARIOGRAMS[vkey]["fit"]
    # the score kernel on the device's own arrays (1e-9 relative), and against the restatement's scores within the bound of the
    # predictions they are means of (fp32 outputs cannot meet an fp64 figure more closely than that)
    counts = res.counts.cpu().numpy()
    own = [np.concatenate([a[f, :n] for f, n in enumerate(counts)]) for a in (x.cpu().numpy() for x in (res.z, res.pred, res.var))]
    got, mine, ref = res.scores(), kr.scores(*own), kr.scores(_flat(r64, 0), _flat(r64, 1), _flat(r64, 2))
    sums = res.sums().cpu().numpy()
    assert got["n"] == mine["n"] == ref["n"] == int(sums[0]) == int(masks.sum())
    assert abs(sums[3] / sums[0] - mine["RMSE"] ** 2) <= 1e-9 * mine["RMSE"] ** 2
    for k in ("ME", "MAE", "RMSE", "MSDR"):
        assert abs(got[k] - mine[k]) <= 1e-9 * max(abs(mine[k]), mine["MAE"]), (k, got[k], mine[k])
    for k in ("ME", "MAE", "RMSE"):
        assert abs(got[k] - ref[k]) <= bound, (k, got[k], ref[k], bound)
    print(f"mixed {vkey}: LOSO RMSE {got['RMSE']:.6f} (restatement {ref['RMSE']:.6f})  MSDR {got['MSDR']:.4f} (restatement {ref['MSDR']:.4f})")


def test_rules(dev):
    masked, masks = case("rules")
    assert [int(m.sum()) for m in masks] == [36, 3, 0, 36]
    G, res = _run(dev, "rules", "exponential-fit")
    r64, r32 = loso_ref("rules", "exponential-fit")
    check_loso("rules", "exponential-fit", res, r64, r32)
    pred, var, counts = res.pred.cpu().numpy(), res.var.cpu().numpy(), res.counts.cpu().numpy()
    cand = G.last_fit["cand"].cpu().numpy()
    assert cand[0] >= 0 and cand[3] == -1 and int(G.last_status.sum()) == 0
    assert all(np.isfinite(pred[f, :counts[f]]).all() and np.isfinite(var[f, :counts[f]]).all() and counts[f] for f in range(3))
    assert all(np.isnan(pred[f, :counts[f]]).all() and np.isnan(var[f, :counts[f]]).all() and counts[f] == 1 for f in range(3, 6))
    assert not counts[6:9].any() and not pred[6:9].any() and not var[6:9].any()
    assert all(np.isnan(pred[f, :counts[f]]).all() and np.isnan(var[f, :counts[f]]).all() and counts[f] for f in range(9, 12))
    # the healthy sample alone gives the same figures within the bound: its neighbours in the batch do not touch it
    alone = _model(dev, name="stkriging", variogram=VARIOGRAMS["exponential-fit"]).cross_validate_sites(
        *(torch.from_numpy(x[:1]).to(dev) for x in (masked, masks)))
    check_loso("rules", "sample 0 alone", alone, r64[:3], r32[:3])
    assert res.scores()["n"] == 36


def test_one_frame_is_kriging_cross_validation(dev):
    masked, masks = case("one-frame")
    for vkey in ("exponential-k.5n", "spherical-k8"):
        _, res = _run(dev, "one-frame", vkey)
        bound = check_loso("one-frame", vkey, res, *loso_ref("one-frame", vkey))
        spatial = {k: v for k, v in VARIOGRAMS[vkey].items() if k != "time_scale"}
        other = _model(dev, name="kriging", variogram=spatial).cross_validate(*_tensors("one-frame", dev))
        _, _, l64 = kr.kriging_uq(masked, masks, spatial, np.float64)
        _, _, l32 = kr.kriging_uq(masked, masks, spatial, np.float32)
        scale = float(np.abs(l64[0][0]).max())
        bk = _rel(float(np.abs(l32[0][1].astype(np.float64) - l64[0][1]).max()) / scale) * scale
        vk = _rel(float(np.abs(l32[0][2].astype(np.float64) / l64[0][2] - 1.0).max()))
        vs = _rel(float(np.abs(loso_ref("one-frame", vkey)[1][0][2].astype(np.float64) / loso_ref("one-frame", vkey)[0][0][2] - 1.0).max()))
        assert int(res.counts[0]) == int(other.counts[0]) == 40
        diff = float((res.pred[:, :40] - other.pred[:, :40]).abs().max())
        vdiff = float((res.var[:, :40] / other.var[:, :40] - 1.0).abs().max())
        print(f"one-frame {vkey}: |LOSO - kriging LOO| {diff:.3e}  bounds {bound:.3e} + {bk:.3e};  variance rel {vdiff:.3e}  bounds {vs:.3e} + {vk:.3e}")
        assert np.abs(l64[0][1] - loso_ref("one-frame", vkey)[0][0][1]).max() <= 1e-12         # the two restatements agree
        assert diff <= bound + bk and vdiff <= vs + vk + vs * vk


@pytest.mark.parametrize("name", ["kriging", "idw"])
def test_per_frame_models_fill_the_site_field(dev, name):
    masked, masks = case("mixed")
    model = {"name": name, "variogram": {"model": "exponential", "fit": False, "nugget": 0.01, "psill": 0.8, "range": 6.0}} if name == "kriging" \
        else {"name": name}
    G = _model(dev, **model)
    a, b = G.cross_validate(*_tensors("mixed", dev)), G.cross_validate_sites(*_tensors("mixed", dev))
    assert a.site is None and b.site.dtype == torch.int32 and b.site.shape == b.pred.shape
    assert torch.equal(a.pred.view(torch.int32), b.pred.view(torch.int32))        # bit for bit, NaN included
    if name == "kriging":
        assert torch.equal(a.var.view(torch.int32), b.var.view(torch.int32))
    else:
        assert a.var is None and b.var is None
    site, counts = b.site.cpu().numpy(), b.counts.cpu().numpy()
    rows = lr.loso(masked, masks, FIXED["exponential-k2"])
    for f, n in enumerate(counts):
        assert np.array_equal(site[f, :n], rows[f][3]) and (site[f, n:] == -1).all()


def test_two_runs_are_identical_and_forward_is_untouched(dev):
    for tag, vkey in (("mixed", "exponential-fit"), ("straddle", "spherical-k.5n"), ("full-shifted", "exponential-k2")):
        G = _model(dev, name="stkriging", variogram=VARIOGRAMS[vkey])
        x = _tensors(tag, dev)
        before = G(*x)
        a = G.cross_validate_sites(*x)
        b = _model(dev, name="stkriging", variogram=VARIOGRAMS[vkey]).cross_validate_sites(*x)
        for k in ("pix", "z", "pred", "var", "counts", "site"):
            u, v = getattr(a, k), getattr(b, k)
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (tag, k)            # bit for bit, NaN included
        assert torch.equal(a.sums(), b.sums())
        assert torch.equal(G(*x), before), tag


def test_script_by_site(dev, tmp_path):
    """crossvalidate.py --by-site on a synthetic two-event store at 32 x 32 (block-4 mask: 64 gauges per frame)."""
    from p2igan_bench.data import synth_store
    from p2igan_bench.data.dataloader import P2IDataModule
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import crossvalidate as cv_script
    store = tmp_path / "test.zarr"
    synth_store.write_test_zarr(str(store), n_events=2, frames_per_event=20, h=32, w=32)
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "stkriging_baseline.json")))
    cfg["data"]["test"].update(w=32, h=32, data_root=str(store))
    cfg["data"]["test"]["mask"]["block_sizes"] = [4]
    path = tmp_path / "stkriging.json"
    json.dump(cfg, open(path, "w"))
    np.random.seed(cfg["seed"])                    # the script seeds the global generators before the loader draws the masks
    gauges = sum(int((batch[2] != 0).sum()) for batch in P2IDataModule(cfg).test_dataloader())
    assert gauges == 2 * 20 * 64
    out = tmp_path / "loso"
    cv_script.main(["--config", str(path), "--output", str(out), "--by-site", "--stride", "8"])
    for name in ("loso.json", "loso.txt", "loso_data.npz"):
        assert (out / name).exists()
    assert not (out / "loo.json").exists()
    res = json.load(open(out / "loso.json"))
    assert res["model_name"] == "stkriging" and res["stride"] == 8
    assert sorted(res["events"]) == ["event_01", "event_02"] and res["overall"]["n"] == gauges
    assert np.isfinite([res["overall"][k] for k in ("ME", "MAE", "RMSE", "MSDR", "ME_mmhr", "MAE_mmhr", "RMSE_mmhr")]).all()
    assert open(out / "loso.txt").readline().startswith("leave-one-site-out cross-validation: stkriging")
    data = np.load(out / "loso_data.npz")
    assert sorted(data.files) == sorted(["event", "frame", "y", "x", "z", "pred", "var", "site"])
    assert len(data["z"]) == gauges and data["frame"].max() == 19 and set(data["event"]) == {1, 2}
    assert data["site"].min() == 0 and data["site"].max() >= 63 and np.isfinite(data["pred"]).all() and (data["var"] > 0).all()
    print(f"loso.json overall: RMSE {res['overall']['RMSE']:.4f}  MSDR {res['overall']['MSDR']:.4f}  n {res['overall']['n']}")
    with pytest.raises(ValueError, match="at most 32 frames"):
        cv_script.main(["--config", str(path), "--output", str(tmp_path / "x"), "--by-site", "--stride", "40"])
    assert not (tmp_path / "x").exists()
    with pytest.raises(RuntimeError, match="leave-one-site-out"):                 # without the flag the script behaves as before
        cv_script.main(["--config", str(path), "--output", str(tmp_path / "x"), "--stride", "8"])
