"""Moving-neighbourhood kriging in the Lagrangian frame (model.name: locallagkriging, csrc/lkrig.hip's LAG kernels)
on the GPU against the numpy restatement tests/llkriging_ref.py.  Every prediction and variance is held to the project's rule: error
<= max(32 e32, 1e-6) x scale against the fp64 restatement, e32 the float32 restatement's error on the same case, scale max|ref| for
predictions and c00 for variances (leave-one-site-out variances relatively, as DESIGN.md section 16 does).  The kernel's own selection
(last_neighbours) is compared exactly in every case."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import lagkriging_ref as lg
import llkriging_ref as ll
import lkriging_ref as lr
import test_krig_uq_gpu as tu
from conftest import PKG
from test_localkriging_gpu import FCAP, FITTED, FIXED, counts_masks, field

pytestmark = pytest.mark.gpu

V_FRAC = {"fit": False, "vy": 1.5, "vx": -0.5}            # a fractional velocity
V_EDGE = {"fit": False, "vy": 4.0, "vx": -0.5}            # a component at the default vmax
REST = {"fit": False, "vy": 0.0, "vx": 0.0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def model(dev, variogram, advection, k, frames, name="locallagkriging"):
    from p2igan_bench.models import build_generator
    mc = dict(name=name, variogram=variogram)
    if name != "lagkriging":
        mc["neighbourhood"] = {"k": k, "frames": frames}
    if name != "localkriging":
        mc["advection"] = advection
    return build_generator({"model": mc}).to(dev)


def within_bounds(tag, pred, var, ref, done, scale):
    """pred, var (B, T, 1, h, w) of the device against ref = (r64, v64, r32, v32) on the targets `done`; scale: c00 per sample."""
    r64, v64, r32, v32 = ref
    top = float(np.abs(r64[done]).max()) or 1.0
    err = float(np.abs(pred[done] - r64[done]).max()) / top
    e32 = float(np.abs(r32[done].astype(np.float64) - r64[done]).max()) / top
    nan = np.isnan(v64)
    assert np.array_equal(np.isnan(var)[done], nan[done]), (tag, "NaN variances differ")
    ok = done & ~nan
    with np.errstate(invalid="ignore"):
        verr = float((np.abs(var - v64) / scale)[ok].max(initial=0.0))
        ve32 = float((np.abs(v32.astype(np.float64) - v64) / scale)[ok].max(initial=0.0))
    print(f"{tag}: prediction err {err:.3e} e32 {e32:.3e} bound {tu._rel(e32):.3e} (of max|ref|); variance err {verr:.3e} e32 {ve32:.3e} "
          f"bound {tu._rel(ve32):.3e} (of c00)")
    assert err <= tu._rel(e32), (tag, err, tu._rel(e32))
    assert verr <= tu._rel(ve32), (tag, verr, tu._rel(ve32))
    return ok


def check(tag, dev, masked, masks, variogram, advection, k, frames, every=1):
    """forward_uq, forward (with the selection) and a second run against the restatement; returns the device's (pred, var) and the
    model."""
    B, T, _, h, w = masked.shape
    G = model(dev, variogram, advection, k, frames)
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
    r64, v64, n64, fits = ll.locallagkriging(masked, masks, variogram, advection, k, frames, np.float64, every, FCAP)
    r32, v32, _, _ = ll.locallagkriging(masked, masks, variogram, advection, k, frames, np.float32, every)
    vel = G.last_fit["velocity"].cpu().numpy()
    assert vel.shape == (B, 2) and all(tuple(vel[b]) == fits[b][0] for b in range(B)), (tag, vel, [f[0] for f in fits])
    done = np.isfinite(r64)                       # every > 1: the restatement solved these targets only
    assert done.all() if every == 1 else done.sum() >= done.size // every
    assert np.array_equal(nbr.reshape(B, T, h * w, k)[done.reshape(B, T, h * w)], n64[done.reshape(B, T, h * w)]), (tag, "selection differs")
    scale = np.array([np.nan if f[1] is None else f[1][0] + f[1][1] for f in fits])[:, None, None, None, None]
    ok = within_bounds(tag, pred, var, (r64, v64, r32, v32), done, scale)
    assert not var[(masks != 0) & ok].any() and (var[ok] >= 0).all()               # exactly 0 on a gauge pixel in its own frame
    return pred, var, G


SWEEP_COUNTS = {"small": (0, 1, 2), "mid": (31, 33, 65), "gap": (97, 0, 31)}      # "gap": a middle frame without gauges


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    masks = counts_masks(SWEEP_COUNTS[name], 16, 16, 31)
    return field(1, 3, 16, 16, 32) * masks, masks


@pytest.mark.parametrize("k", [1, 31, 32, 33, 64])
@pytest.mark.parametrize("name", sorted(SWEEP_COUNTS))
def test_edge_sweep_of_k_against_frame_sizes(dev, name, k):
    """16 x 16, T = 3: both KC instantiations and the list edge, exponential with a nugget, a fractional velocity."""
    masked, masks = sweep_case(name)
    check(f"sweep {name} k={k}", dev, masked, masks, FIXED["exponential"], V_FRAC, k, 1)


@pytest.mark.parametrize("frames", [0, 1, 2, 6])
@pytest.mark.parametrize("name", ["mid", "gap"])
def test_edge_sweep_of_the_window(dev, name, frames):
    """Spherical without a nugget, a velocity with a component at vmax; frames = 6 = T + 3 is clipped to T - 1."""
    masked, masks = sweep_case(name)
    check(f"window {name} frames={frames}", dev, masked, masks, FIXED["spherical"], V_EDGE, 32, frames)


@pytest.mark.parametrize("k", [1, 33, 64])
def test_edge_sweep_of_k_at_vmax(dev, k):
    masked, masks = sweep_case("mid")
    check(f"vmax k={k}", dev, masked, masks, FIXED["spherical"], V_EDGE, k, 2)


@pytest.mark.parametrize("vkey", ["exponential", "spherical"])
def test_zero_velocity_against_localkriging_on_the_device(dev, vkey):
    """At v = 0 the key is localkriging's bit for bit, so the two kernels select the same neighbours; their predictions each meet the
    bound against the one fp64 reference.  They are not required to be bit-equal: lag_dist (fmaf of the squares) and st_dist (an exact
    integer d2, one fmaf) round the same distance differently."""
    masked, masks = sweep_case("mid")
    B, T, _, h, w = masked.shape
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    pred, var, G = check(f"rest {vkey}", dev, masked, masks, FIXED[vkey], REST, 20, 2)
    G.forward(x, m, neighbours=True)
    S = model(dev, FIXED[vkey], None, 20, 2, name="localkriging")
    sp, sv = S.forward_uq(x, m)
    S.forward(x, m, neighbours=True)
    assert torch.equal(G.last_neighbours, S.last_neighbours)
    r64, v64, _ = lr.localkriging(masked, masks, FIXED[vkey], 20, 2, np.float64)
    r32, v32, _ = lr.localkriging(masked, masks, FIXED[vkey], 20, 2, np.float32)
    scale = np.full((B, 1, 1, 1, 1), FIXED[vkey]["nugget"] + FIXED[vkey]["psill"])
    done = np.ones(r64.shape, bool)
    within_bounds(f"rest {vkey} static kernel", sp.cpu().numpy(), sv.cpu().numpy(), (r64, v64, r32, v32), done, scale)
    within_bounds(f"rest {vkey} Lagrangian kernel, static reference", pred, var, (r64, v64, r32, v32), done, scale)


def test_fitted_velocity_and_variogram_on_a_moving_field(dev):
    """lagkriging_ref's 'down-left' field (32 x 32, T = 8, 40 fixed sites): velocity and variogram fitted on the device; every 5th target
    in the restatement.  check() holds last_fit['velocity'] to the restatement's."""
    v, seed = lg.CASES["down-left"]
    truth, masked, masks = lg.translating_field(seed, v, 8)
    pred, _, G = check("down-left fitted", dev, masked, masks, lg.FITTED, lg.ADVECTION, 32, 2, every=5)
    assert set(G.last_fit) >= {"velocity", "score", "weight", "support", "vcand", "bins", "fit", "cand", "q", "c"}
    vel = tuple(G.last_fit["velocity"].cpu().numpy()[0])
    assert abs(vel[0] - v[0]) <= 1.0 and abs(vel[1] - v[1]) <= 1.0
    static = model(dev, lg.FITTED, None, 32, 2, name="localkriging")(torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev))
    print(f"down-left on the device: RMSE local Lagrangian {lg.rmse(pred, truth):.4f}, local static {lg.rmse(static.cpu().numpy(), truth):.4f}")


@pytest.mark.parametrize("vkey", ["exponential", "spherical"])
def test_whole_sample_neighbourhood_and_the_global_model_on_the_device(dev, vkey):
    """16 x 16, T = 3, 24 points, k = 64, frames = T - 1: the local and the global Lagrangian model each meet their bound against one
    fp64 reference."""
    masks = counts_masks((8, 8, 8), 16, 16, 81)
    masked = field(1, 3, 16, 16, 82) * masks
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    ref = lg.lagkriging(masked, masks, FIXED[vkey], V_FRAC)[0]
    top = float(np.abs(ref).max())
    e_local = float(np.abs(ll.locallagkriging(masked, masks, FIXED[vkey], V_FRAC, 64, 2, np.float32)[0] - ref).max()) / top
    e_global = float(np.abs(lg.lagkriging(masked, masks, FIXED[vkey], V_FRAC, np.float32)[0] - ref).max()) / top
    local = model(dev, FIXED[vkey], V_FRAC, 64, 2)(x, m).cpu().numpy()
    glob = model(dev, FIXED[vkey], V_FRAC, 64, 2, name="lagkriging")(x, m).cpu().numpy()
    d_local, d_global = float(np.abs(local - ref).max()) / top, float(np.abs(glob - ref).max()) / top
    print(f"{vkey}: local err {d_local:.3e} (e32 {e_local:.3e}), global err {d_global:.3e} (e32 {e_global:.3e})")
    assert d_local <= tu._rel(e_local) and d_global <= tu._rel(e_global)


def test_leave_one_site_out_beyond_32_frames(dev):
    """16 x 16, T = 40: sample 0 has 20 sites (one of them misses every third frame), sample 1 a single site (alone in its window once its
    own pixel is out: NaN).  lagkriging refuses the length."""
    rng = np.random.default_rng(71)
    T, h, w = 40, 16, 16
    masks = np.zeros((2, T, 1, h, w), np.float32)
    sites = rng.permutation(h * w)[:20]
    masks[0, :, 0].reshape(T, -1)[:, sites] = 1.0
    masks[0, ::3, 0].reshape(-1, h * w)[:, sites[0]] = 0.0
    masks[1, :, 0, 9, 7] = 1.0
    masked = field(2, T, h, w, 72) * masks
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    with pytest.raises(ValueError, match="at most 32 frames"):
        model(dev, FIXED["exponential"], V_FRAC, 16, 2, name="lagkriging").cross_validate_sites(x, m)
    for vkey, adv, k, frames in (("exponential", V_FRAC, 16, 2), ("spherical", V_EDGE, 64, 1)):
        G = model(dev, FIXED[vkey], adv, k, frames)
        res = G.cross_validate_sites(x, m)
        assert int(G.last_status.sum()) == 0
        l64 = ll.loso(masked, masks, FIXED[vkey], adv, k, frames, np.float64)
        l32 = ll.loso(masked, masks, FIXED[vkey], adv, k, frames, np.float32)
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


def test_rules(dev):
    """All gauges in the last frame with frames = 0 (the other frames take the sample's gauge mean, NaN variance), a sample without any
    gauge (zeros, NaN), and a degenerate fitted sample (its gauge mean, NaN)."""
    masks = np.concatenate([counts_masks((0, 0, 19), 16, 16, 41), counts_masks((0, 0, 0), 16, 16, 42)])
    masked = field(2, 3, 16, 16, 43) * masks
    pred, var, _ = check("rules", dev, masked, masks, FIXED["exponential"], V_FRAC, 8, 0)
    mean = masked[0][masks[0] != 0].astype(np.float64).mean()
    assert np.abs(pred[0, :2] - mean).max() <= 1e-6 and np.isnan(var[0, :2]).all() and np.isfinite(var[0, 2]).all()
    assert not pred[1].any() and np.isnan(var[1]).all()
    flat = masks[:1] * np.float32(0.4)                                  # zero variance: a degenerate fitted sample, and v = 0 by the tie rule
    pred, var, G = check("degenerate fit", dev, flat, masks[:1], FITTED["exponential"], lg.ADVECTION, 8, 2)
    assert np.abs(pred - np.float32(0.4)).max() <= 1e-6 and np.isnan(var).all()
    assert not G.last_fit["velocity"].any()


def test_scripts_end_to_end(dev, tmp_path):
    """infer.py --variance-output and crossvalidate.py --by-site --stride 40 on a synthetic two-event store at 32 x 32."""
    from p2igan_bench.data import synth_store, zarr_lite
    from p2igan_bench.data.dataloader import P2IDataModule
    from p2igan_bench.models import build_generator
    from p2igan_bench.models.classical import LOCAL_LAG_NO_LOO
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import crossvalidate as cv_script
    import infer as infer_script
    store = tmp_path / "test.zarr"
    synth_store.write_test_zarr(str(store), n_events=2, frames_per_event=40, h=32, w=32)
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "locallagkriging_baseline.json")))
    cfg["data"]["test"].update(w=32, h=32, data_root=str(store))
    cfg["data"]["test"]["mask"]["block_sizes"] = [4]
    path = tmp_path / "locallagkriging.json"
    json.dump(cfg, open(path, "w"))
    np.random.seed(cfg["seed"])                   # the scripts seed the global generators before the loader draws the masks
    events = []
    for batch in P2IDataModule(cfg).test_dataloader():
        _, masked, masks = [t.permute(0, 1, 4, 2, 3).contiguous() for t in batch]
        events.append((masked, masks))
    assert len(events) == 2 and events[0][0].shape[1] == 40

    infer_script.main(["--config", str(path), "--output", str(tmp_path / "l.zarr"), "--variance-output", str(tmp_path / "lv.zarr")])
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
    cv_script.main(["--config", str(path), "--output", str(out), "--by-site", "--stride", "40"])
    for name in ("loso.json", "loso.txt", "loso_data.npz"):
        assert (out / name).exists()
    res = json.load(open(out / "loso.json"))
    assert sorted(res["events"]) == ["event_01", "event_02"] and res["overall"]["n"] > 0
    assert np.isfinite([res["overall"][k] for k in ("ME", "MAE", "RMSE", "MSDR")]).all()
    with pytest.raises(RuntimeError) as e:
        cv_script.main(["--config", str(path), "--output", str(tmp_path / "loo"), "--stride", "16"])
    assert str(e.value) == LOCAL_LAG_NO_LOO
