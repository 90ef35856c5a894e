"""Lagrangian space-time kriging on the GPU (LagrangianKrigingGenerator on csrc/lagkrig.hip and the shared kernels of stkrig.hip,
stkrig_loso.hip and classical.hip) against the fp64 numpy restatement (tests/lagkriging_ref.py).

Velocity tables and bins are fp64 on the device and held to 1e-10 relative, the bins' tolerance of test_stkriging_gpu.py.  Error bound
of every prediction, as there: max(32 e32, 1e-6) max|ref|, with e32 the fp32 restatement's own error against fp64 relative to
max|ref|, computed in the same test; leave-one-site-out is held by test_stkriging_loso_gpu.py's check_loso.  Every figure is printed
beside its bound."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import lagkriging_ref as lg
import stkriging_loso_ref as lr
import stkriging_ref as sr
from conftest import PKG
from test_stkriging_loso_gpu import check_loso

pytestmark = pytest.mark.gpu

V = {"fit": False, "vy": 0.75, "vx": -1.25}
REST = {"fit": False, "vy": 0.0, "vx": 0.0}
FIXED = {"exponential": {"model": "exponential", "fit": False, "nugget": 0.01, "psill": 0.8, "range": 6.0, "time_scale": 2.0},
         "spherical": {"model": "spherical", "fit": False, "nugget": 0.01, "psill": 0.8, "range": 5.0, "time_scale": 0.5},
         "exponential-n0": {"model": "exponential", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 6.0, "time_scale": 2.0},
         "spherical-n0": {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 10.0, "time_scale": 2.0}}
TILE_COUNTS = (31, 32, 33, 65)
GROUP_T = (1, 7, 8, 9)                                   # around the predictor's group of 8 target frames


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _masks(rng, counts, h, w):
    """(B, T, 1, h, w) masks with counts[b][t] gauges at random pixels."""
    m = np.zeros((len(counts), len(counts[0]), h * w), np.float32)
    for b, row in enumerate(counts):
        for t, n in enumerate(row):
            m[b, t, rng.permutation(h * w)[:n]] = 1.0
    return m.reshape(len(counts), len(counts[0]), 1, h, w)


def _values(rng, masks):
    return ((0.1 + rng.random(masks.shape)).astype(np.float32) * masks).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(tag):
    """(masked, masks) as (B, T, 1, H, W) fp32 numpy arrays; built once, never modified."""
    if tag == "per-sample":       # 127 / 128 / 129 points per sample over three frames, differing counts
        rng = np.random.default_rng(3)
        masks = _masks(rng, [(42, 43, 42), (43, 42, 43), (43, 43, 43)], 16, 16)
    elif tag == "per-frame":      # 127 / 128 / 129 gauges in the later frame: around the velocity kernel's staging chunk of 128
        rng = np.random.default_rng(4)
        masks = _masks(rng, [(9, 127), (140, 128), (5, 129)], 16, 16)
    elif tag == "rules":          # healthy; a middle frame without gauges; constant values; one frame only has gauges (no pair)
        rng = np.random.default_rng(6)
        masks = _masks(rng, [(12, 11, 13), (14, 0, 12), (12, 12, 12), (0, 20, 0)], 12, 10)
    elif tag == "one-frame":
        rng = np.random.default_rng(8)
        masks = _masks(rng, [(30,)], 12, 10)
    elif tag == "tiles":          # N per sample 31, 32, 33, 65 over three 9 x 13 frames
        rng = np.random.default_rng(10)
        masks = _masks(rng, [(n // 2, n // 5, n - n // 2 - n // 5) for n in TILE_COUNTS], 9, 13)
    elif tag.startswith("group"):  # T frames of 17 x 16 with 12 gauges each, a mask per frame
        rng = np.random.default_rng(12)
        masks = _masks(rng, [(12,) * int(tag[5:])], 17, 16)
    else:
        raise KeyError(tag)
    masked = _values(rng, masks)
    if tag == "rules":
        masked[2] = np.float32(0.25) * masks[2]
    return masked, masks


@functools.lru_cache(maxsize=None)
def field(tag):
    v, seed = lg.CASES[tag]
    return lg.translating_field(seed, v, 8)


@functools.lru_cache(maxsize=None)
def lag_ref(tag, vkey, vy, vx):
    """(fp64 prediction, e32, bound) of a case with fixed parameters."""
    masked, masks = case(tag)
    adv = {"fit": False, "vy": vy, "vx": vx}
    r64 = lg.lagkriging(masked, masks, FIXED[vkey], adv, np.float64)[0]
    r32 = lg.lagkriging(masked, masks, FIXED[vkey], adv, np.float32)[0]
    return (r64,) + _bound(r64, r32)


def _bound(r64, r32):
    top = float(np.abs(r64).max())
    e32 = float(np.abs(r32.astype(np.float64) - r64).max()) / max(top, 1e-30)
    return e32, max(32.0 * e32, 1e-6) * top


def _model(dev, **model):
    from p2igan_bench.models import build_generator
    return build_generator({"model": model}).to(dev)


def _dev(arrays, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in arrays)


def _check(tag, what, got, ref, e32, bound):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{tag} {what}: device err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}")
    assert np.isfinite(got).all() and err <= bound, (tag, what, err, bound)


def _close(got, ref, what):
    """1e-10 relative to the table's largest finite entry; infinities in the same places."""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), what
    assert np.array_equal(got[~fin], ref[~fin]), what
    if fin.any():
        err, top = float(np.abs(got[fin] - ref[fin]).max()), float(np.abs(ref[fin]).max())
        print(f"{what}: err {err:.3e}  bound {1e-10 * top:.3e}")
        assert err <= 1e-10 * top, (what, err, top)


def _tables(dev, tag, n_tlags, nhalf, vstep=0.5, r0=1.5):
    """The device's tables and choice for a case against the restatement's, sample by sample; returns the chosen velocities."""
    from p2igan_bench import ops
    masked, masks = case(tag)
    b, t, _, h, w = masked.shape
    x, m = _dev((masked.reshape(b, t, h, w), masks.reshape(b, t, h, w)), dev)
    pix, z, info = ops.krig_compact(x, m, 160)
    score, weight, support, vel, velf, vcand = (a.cpu().numpy() for a in ops.lagkrig_velocity(pix, z, info, b, t, min(n_tlags, t - 1), nhalf,
                                                                                             vstep, r0))
    n = 2 * nhalf + 1
    assert score.shape == weight.shape == support.shape == (b, n, n) and vel.shape == (b, 2)
    for i in range(b):
        W, S, N = lg.score_tables(lg.frames_of(masked[i], masks[i]), n_tlags, nhalf, vstep, r0)
        what = f"{tag} sample {i} n_tlags {n_tlags} grid {n} x {n}"
        _close(weight[i], W, what + " weight")
        _close(support[i], N, what + " support")
        _close(score[i], lg.score_of(W, S), what + " score")
        (ci, cj), gap = lg.pick(W, S, N)
        print(f"{what}: restatement v ({ci * vstep}, {cj * vstep}) gap {gap:.3g}  device v {tuple(vel[i])}")
        if gap > 1e-6 or not W.any() or not S.any():         # a clear winner, or the all-tie cases that the rule sends to v = 0
            assert tuple(vel[i]) == (ci * vstep, cj * vstep) and int(vcand[i]) == (ci + nhalf) * n + cj + nhalf
        assert np.array_equal(velf[i], vel[i].astype(np.float32))
    return vel


@pytest.mark.parametrize("tag", ["per-sample", "per-frame"])
@pytest.mark.parametrize("nhalf", [0, 1, 8])
def test_velocity_tables(dev, tag, nhalf):
    masked, masks = case(tag)
    sums = [int(m.sum()) for m in masks]
    assert sums == [127, 128, 129] if tag == "per-sample" else [int(m[1].sum()) for m in masks] == [127, 128, 129]
    vel = _tables(dev, tag, 3, nhalf)
    if nhalf == 0:
        assert not vel.any()                                                   # one candidate: v = 0


def test_velocity_rules(dev):
    masked, masks = case("rules")
    assert not masks[1, 1].any() and np.ptp(masked[2][masks[2] != 0]) == 0 and int(masks[3].sum()) == 20
    vel = _tables(dev, "rules", 3, 8)
    assert not vel[2].any() and not vel[3].any()                               # zero variance; no pair: v = 0
    vel = _tables(dev, "rules", 2, 2, vstep=1.25, r0=2.0)                      # two lags, 5 x 5, another step and bandwidth
    assert not vel[2].any() and not vel[3].any()
    vel = _tables(dev, "rules", 2, 16, vstep=0.25, r0=2.0)                     # 33 x 33 = 1089: the largest grid, two candidates per thread
    assert not vel[2].any() and not vel[3].any()
    assert not _tables(dev, "rules", 0, 8).any()                               # n_tlags 0: no pair anywhere
    assert not _tables(dev, "one-frame", 3, 8).any()                           # T = 1: n_tlags is capped at 0


def test_bins(dev):
    masked, masks = case("rules")
    x = _dev((masked, masks), dev)
    vg = dict(lg.FITTED)
    S = _model(dev, name="stkriging", variogram=vg)
    S(*x)
    G = _model(dev, name="lagkriging", variogram=vg, advection=REST)
    G(*x)
    assert torch.equal(G.last_fit["bins"], S.last_fit["bins"]) and torch.equal(G.last_fit["cand"], S.last_fit["cand"])
    assert torch.equal(G.last_fit["fit"], S.last_fit["fit"]) and not G.last_fit["velocity"].any()
    G = _model(dev, name="lagkriging", variogram=vg, advection=V)
    G(*x)
    bins = G.last_fit["bins"].cpu().numpy()
    assert not torch.equal(G.last_fit["bins"], S.last_fit["bins"])
    for b in range(masked.shape[0]):
        n, sg, sh = lg.lag_bins(lg.frames_of(masked[b], masks[b]), 12, 10, 16, 3, (0.75, -1.25))
        assert bins.shape[1:] == (3, 16, 3) and np.array_equal(bins[b, :, :, 0], n)          # counts exactly (T = 3: two temporal lags)
        assert np.abs(bins[b, :, :, 1] - sg).max() <= 1e-10 * max(np.abs(sg).max(), 1e-300)
        assert np.abs(bins[b, :, :, 2] - sh).max() <= 1e-10 * max(np.abs(sh).max(), 1e-300)


@pytest.mark.parametrize("vkey", ["exponential", "spherical"])
def test_tile_edges(dev, vkey):
    masked, masks = case("tiles")
    assert [int(m.sum()) for m in masks] == list(TILE_COUNTS) and masked.shape[-2:] == (9, 13)
    ref, e32, bound = lag_ref("tiles", vkey, V["vy"], V["vx"])
    G = _model(dev, name="lagkriging", variogram=FIXED[vkey], advection=V)
    got = G(*_dev((masked, masks), dev)).cpu().numpy()
    for i, n in enumerate(TILE_COUNTS):
        print(f"N_st = {n}: device err {float(np.abs(got[i] - ref[i]).max()):.3e}")
    _check("tiles", vkey, got, ref, e32, bound)
    assert int(G.last_status.sum()) == 0 and G.last_status.numel() == len(TILE_COUNTS)
    if vkey == "spherical":       # the early-out fires: most (pixel, point, frame) triples lie beyond the range of 5 px
        xy, tt, _ = sr.points(masked[3], masks[3])
        c0 = lg.lag_covariance(cr.grid(9, 13), np.zeros(117, np.int64), xy, tt, 0.0, 0.8, 5.0, 0.5, (0.75, -1.25), "spherical", np.float64)
        assert (c0 == 0).mean() > 0.5 and (c0 > 0).any()


@pytest.mark.parametrize("t", GROUP_T)
def test_frame_group_boundary(dev, t):
    tag = f"group{t}"
    masked, masks = case(tag)
    assert masked.shape == (1, t, 1, 17, 16)
    for vkey in ("exponential", "spherical"):
        ref, e32, bound = lag_ref(tag, vkey, V["vy"], V["vx"])
        got = _model(dev, name="lagkriging", variogram=FIXED[vkey], advection=V)(*_dev((masked, masks), dev)).cpu().numpy()
        _check(tag, vkey, got, ref, e32, bound)


def test_shear_identity_against_stkriging(dev):
    """Integer v = (1, -2): the lagkriging prediction at (t, p) is the stkriging prediction at (t, p - v t + offset) on a canvas
    enlarged by |v| (T - 1) whose gauges of frame t are moved to x - v t + offset: the new distance pinned to trusted kernels."""
    masked, masks = case("group7")
    T, h, w = 7, 17, 16
    vy, vx = 1, -2
    oy, ox = vy * (T - 1), 0
    H2, W2 = h + abs(vy) * (T - 1), w + abs(vx) * (T - 1)
    m2, z2 = np.zeros((1, T, 1, H2, W2), np.float32), np.zeros((1, T, 1, H2, W2), np.float32)
    for t in range(T):
        ys, xs = np.nonzero(masks[0, t, 0])
        m2[0, t, 0, ys - vy * t + oy, xs - vx * t + ox] = 1.0
        z2[0, t, 0, ys - vy * t + oy, xs - vx * t + ox] = masked[0, t, 0, ys, xs]
    assert int(m2.sum()) == int(masks.sum())
    for vkey in ("exponential", "spherical-n0"):
        ref, e32, bound = lag_ref("group7", vkey, float(vy), float(vx))
        lag = _model(dev, name="lagkriging", variogram=FIXED[vkey], advection={"fit": False, "vy": vy, "vx": vx})(
            *_dev((masked, masks), dev)).cpu().numpy()
        big = _model(dev, name="stkriging", variogram=FIXED[vkey])(*_dev((z2, m2), dev)).cpu().numpy()
        _check("group7 sheared", vkey, lag, ref, e32, bound)
        diff = 0.0
        for t in range(T):
            y0, x0 = oy - vy * t, ox - vx * t
            diff = max(diff, float(np.abs(lag[0, t, 0].astype(np.float64) - big[0, t, 0, y0:y0 + h, x0:x0 + w]).max()))
        print(f"group7 {vkey}: |lagkriging - sheared stkriging| {diff:.3e}  bound {bound:.3e}")
        assert diff <= bound


def test_resting_case_is_stkriging(dev):
    for tag, vkey in (("tiles", "spherical"), ("group9", "exponential")):
        masked, masks = case(tag)
        ref, e32, bound = lag_ref(tag, vkey, 0.0, 0.0)
        x = _dev((masked, masks), dev)
        lag = _model(dev, name="lagkriging", variogram=FIXED[vkey], advection=REST)(*x)
        st = _model(dev, name="stkriging", variogram=FIXED[vkey])(*x)
        _check(tag + " at rest", vkey, lag.cpu().numpy(), ref, e32, bound)
        diff = float((lag.double() - st.double()).abs().max())
        print(f"{tag} {vkey}: |lagkriging(v = 0) - stkriging| {diff:.3e}  bound {bound:.3e}")
        assert diff <= bound
        assert np.array_equal(ref, sr.stkriging(masked, masks, FIXED[vkey])[0])            # the restatements agree exactly


@pytest.mark.parametrize("vkey", ["exponential-n0", "spherical-n0"])
def test_exact_at_a_gauge_in_its_own_frame_only(dev, vkey):
    assert FIXED[vkey]["nugget"] == 0.0
    masked, masks = case("group8")
    ref, e32, bound = lag_ref("group8", vkey, V["vy"], V["vx"])
    got = _model(dev, name="lagkriging", variogram=FIXED[vkey], advection=V)(*_dev((masked, masks), dev)).cpu().numpy()
    _check("group8", vkey, got, ref, e32, bound)
    at = masks != 0
    err = float(np.abs(got[at].astype(np.float64) - masked[at]).max())
    print(f"group8 {vkey}: err at the gauges {err:.3e}  bound {bound:.3e}")
    assert err <= bound
    only0 = (masks[0, 0] != 0) & (masks[0, 1] == 0)                            # gauges of frame 0 that frame 1 does not have
    assert only0.sum() >= 8
    gap_ref = float(np.abs(ref[0, 1][only0] - masked[0, 0][only0]).max())
    gap = float(np.abs(got[0, 1][only0].astype(np.float64) - masked[0, 0][only0]).max())
    print(f"group8 {vkey}: next-frame gap at frame 0's gauge pixels, restatement {gap_ref:.3e}  device {gap:.3e}")
    assert gap_ref > 100 * bound and abs(gap - gap_ref) <= bound


@functools.lru_cache(maxsize=None)
def fitted_ref(tag):
    truth, masked, masks = field(tag)
    r64, fits = lg.lagkriging(masked, masks, lg.FITTED, lg.ADVECTION, np.float64)
    r32, _ = lg.lagkriging(masked, masks, lg.FITTED, lg.ADVECTION, np.float32)
    return (r64, fits[0]) + _bound(r64, r32)


@pytest.mark.parametrize("tag", sorted(lg.CASES))
def test_end_to_end_with_fitted_velocity(dev, tag):
    truth, masked, masks = field(tag)
    ref, (v, params, est, fit), e32, bound = fitted_ref(tag)
    x = _dev((masked, masks), dev)
    G = _model(dev, name="lagkriging", variogram=lg.FITTED, advection=lg.ADVECTION)
    got = G(*x).cpu().numpy()
    vel = G.last_fit["velocity"].cpu().numpy()[0]
    print(f"{tag}: true v {lg.CASES[tag][0]}  restatement {v} (gap {est[3]:.3g})  device {tuple(vel)};  fit (q, c) restatement {fit[:2]} device "
          f"({int(G.last_fit['q'][0])}, {int(G.last_fit['c'][0])})")
    assert est[3] > 1e-6 and tuple(vel) == v
    _close(G.last_fit["weight"].cpu().numpy()[0], est[1], f"{tag} weight")
    _close(G.last_fit["score"].cpu().numpy()[0], est[2], f"{tag} score")
    _close(G.last_fit["support"].cpu().numpy()[0], est[4], f"{tag} support")
    sses = np.sort(fit[7].ravel())
    if sses[1] - sses[0] > 1e-3 * sses[0]:                                     # the fit's indices are stable on this input
        assert (int(G.last_fit["q"][0]), int(G.last_fit["c"][0])) == tuple(fit[:2])
    _check(tag, "fitted", got, ref, e32, bound)
    st = _model(dev, name="stkriging", variogram=lg.FITTED)(*x).cpu().numpy()
    ratio = lg.rmse(got, truth) / lg.rmse(st, truth)
    print(f"{tag}: RMSE lagkriging {lg.rmse(got, truth):.4f}  stkriging {lg.rmse(st, truth):.4f}  ratio {ratio:.3f}")
    if tag in lg.MOVING:
        assert ratio <= 0.8
    else:
        assert abs(ratio - 1.0) <= 0.05


def test_leave_one_site_out(dev):
    truth, masked, masks = field("right")
    x = _dev((masked, masks), dev)
    G = _model(dev, name="lagkriging", variogram=lg.FITTED, advection=lg.ADVECTION)
    res = G.cross_validate_sites(*x)
    r64 = lg.loso(masked, masks, lg.FITTED, lg.ADVECTION, np.float64)
    r32 = lg.loso(masked, masks, lg.FITTED, lg.ADVECTION, np.float32)
    check_loso("right", "lagkriging fitted", res, r64, r32)
    assert int(G.last_status.sum()) == 0 and tuple(G.last_fit["velocity"].cpu().numpy()[0]) == (0.0, 3.0)
    st = _model(dev, name="stkriging", variogram=lg.FITTED).cross_validate_sites(*x)
    ref_lag, ref_st = lg.loso_rmse(r64), lg.loso_rmse(lr.loso(masked, masks, lg.FITTED))
    dev_lag, dev_st = res.scores()["RMSE"], st.scores()["RMSE"]
    print(f"right: LOSO RMSE lagkriging {dev_lag:.4f} (restatement {ref_lag:.4f})  stkriging {dev_st:.4f} (restatement {ref_st:.4f})")
    assert (dev_lag < dev_st) == (ref_lag < ref_st) and ref_lag < ref_st
    # a given velocity with per-frame masks and blocks that straddle the 32-wide tile: the sites of "tiles" sample 3 (65 points)
    masked, masks = case("tiles")
    G = _model(dev, name="lagkriging", variogram=FIXED["exponential-n0"], advection=V)
    res = G.cross_validate_sites(*_dev((masked, masks), dev))
    check_loso("tiles", "lagkriging v given", res, lg.loso(masked, masks, FIXED["exponential-n0"], V, np.float64),
               lg.loso(masked, masks, FIXED["exponential-n0"], V, np.float32))
    with pytest.raises(RuntimeError, match="leave-one-site-out"):
        G.cross_validate(*_dev((masked, masks), dev))


def test_two_runs_are_identical(dev):
    _, masked, masks = field("down-left")
    x = _dev((masked, masks), dev)
    G = _model(dev, name="lagkriging", variogram=lg.FITTED, advection=lg.ADVECTION)
    a, fa = G(*x), {k: v.clone() for k, v in G.last_fit.items()}
    ra = G.cross_validate_sites(*x)
    H = _model(dev, name="lagkriging", variogram=lg.FITTED, advection=lg.ADVECTION)
    b = H(*x)
    rb = H.cross_validate_sites(*x)
    assert torch.equal(a, b) and all(torch.equal(fa[k], H.last_fit[k]) for k in fa)
    for k in ("pred", "var", "site"):
        assert torch.equal(getattr(ra, k).view(torch.int32), getattr(rb, k).view(torch.int32)), k
    y = _dev(case("tiles"), dev)
    F = _model(dev, name="lagkriging", variogram=FIXED["spherical"], advection=V)
    assert torch.equal(F(*y), F(*y))


def test_limits(dev):
    masked, masks = case("tiles")                                               # 65 points in the largest sample
    with pytest.raises(ValueError, match=r"max_points.*--stride"):
        _model(dev, name="lagkriging", max_points=64, variogram=FIXED["exponential"], advection=V)(*_dev((masked, masks), dev))
    long = _dev(case("group9"), dev)
    long = tuple(torch.cat([a, a, a, a[:, :6]], dim=1).contiguous() for a in long)
    assert long[0].shape[1] == 33
    G = _model(dev, name="lagkriging", variogram=FIXED["exponential"], advection=V)
    with pytest.raises(ValueError, match=r"at most 32 frames.*--stride"):
        G.cross_validate_sites(*long)
    assert G(*long).shape == long[0].shape                                       # forward takes them: 396 points


def test_scripts(dev, tmp_path):
    """infer.py and crossvalidate.py --by-site on synthetic 32 x 32 data (block-4 mask: 64 gauges per frame), and their refusals."""
    from p2igan_bench.data import synth_store, zarr_lite
    from p2igan_bench.data.dataloader import P2IDataModule
    from p2igan_bench.evaluation import run_exp1
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import crossvalidate as cv_script
    import infer as infer_script
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "lagkriging_baseline.json")))
    for k in ("train", "test"):
        cfg["data"][k].update(w=32, h=32)
        cfg["data"][k]["mask"]["block_sizes"] = [4]
    cp = tmp_path / "lagkriging.json"
    json.dump(cfg, open(cp, "w"))
    infer_script.main(["--config", str(cp), "--output", str(tmp_path / "lagkriging.zarr"), "--stride", "8"])
    out = zarr_lite.Group(str(tmp_path / "lagkriging.zarr"))
    assert out.attrs["checkpoint"] is None and out.attrs["model_name"] == "lagkriging"
    preds = {k: out[k][:] for k in ("event_01", "event_02")}
    for arr in preds.values():
        assert arr.shape == (40, 1, 32, 32) and arr.dtype == np.float32 and np.isfinite(arr).all() and float(arr.min()) >= 0.0
    truth, mask = {}, None
    for i, batch in enumerate(P2IDataModule(cfg).test_dataloader()):
        truth[f"event_{i + 1:02d}"] = (batch[0][0, :, :, :, 0] * 255.0).round().numpy().astype(np.uint8)[:, None]
        mask = batch[2][0, 0, :, :, 0].numpy() != 0
    scores = run_exp1({"lagkriging": preds}, truth, mask, "radar", 32)
    for key in ("MAE", "RMSE"):
        assert np.isfinite(float(scores["lagkriging"][key])), (key, scores["lagkriging"][key])
    with pytest.raises(RuntimeError, match="variance-output"):
        infer_script.main(["--config", str(cp), "--output", str(tmp_path / "x.zarr"), "--variance-output", str(tmp_path / "v.zarr")])
    store = tmp_path / "test.zarr"
    synth_store.write_test_zarr(str(store), n_events=2, frames_per_event=20, h=32, w=32)
    cfg["data"]["test"]["data_root"] = str(store)
    json.dump(cfg, open(cp, "w"))
    loso = tmp_path / "loso"
    cv_script.main(["--config", str(cp), "--output", str(loso), "--by-site", "--stride", "8"])
    res = json.load(open(loso / "loso.json"))
    assert res["model_name"] == "lagkriging" and res["stride"] == 8 and res["overall"]["n"] == 2 * 20 * 64
    assert np.isfinite([res["overall"][k] for k in ("ME", "MAE", "RMSE", "MSDR", "ME_mmhr", "MAE_mmhr", "RMSE_mmhr")]).all()
    assert open(loso / "loso.txt").readline().startswith("leave-one-site-out cross-validation: lagkriging")
    data = np.load(loso / "loso_data.npz")
    assert sorted(data.files) == sorted(["event", "frame", "y", "x", "z", "pred", "var", "site"])
    assert len(data["z"]) == 2 * 20 * 64 and np.isfinite(data["pred"]).all() and (data["var"] > 0).all()
    with pytest.raises(ValueError, match="at most 32 frames"):
        cv_script.main(["--config", str(cp), "--output", str(tmp_path / "x"), "--by-site", "--stride", "40"])
    with pytest.raises(RuntimeError, match="leave-one-site-out"):
        cv_script.main(["--config", str(cp), "--output", str(tmp_path / "x"), "--stride", "8"])
    assert not (tmp_path / "x").exists()
