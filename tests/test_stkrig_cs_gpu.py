"""Space-time conditional simulation on the GPU (SpaceTimeKrigingGenerator.forward_simulation on csrc/stkrig_cs.hip) against the fp64
numpy restatement (tests/stkrig_cs_ref.py).

Error bound of every comparison, the rule of the classical baselines: device error <= max(32 e32, 1e-6) scale
against the fp64 restatement, with e32 the fp32 restatement's own error against fp64 relative to the same scale, computed in the same
test.  scale = max|xi| for the noise, max A for the amplitude, max|ref| of the case for the members."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import stkrig_cs_ref as sc
from conftest import PKG

pytestmark = pytest.mark.gpu

VG = {"exp-nug": {"model": "exponential", "fit": False, "nugget": 0.05, "psill": 0.6, "range": 2.0, "time_scale": 3.0},
      "exp-0": {"model": "exponential", "fit": False, "nugget": 0.0, "psill": 0.6, "range": 4.0, "time_scale": 1.5},
      "exp-clip": {"model": "exponential", "fit": False, "nugget": 0.05, "psill": 0.6, "range": 3.0, "time_scale": 1.5},
      "sph-nug": {"model": "spherical", "fit": False, "nugget": 0.02, "psill": 0.8, "range": 9.0, "time_scale": 3.0},
      "sph-0": {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 6.0, "time_scale": 2.0},
      "exp-fit": {"model": "exponential", "fit": True, "n_lags": 8, "n_tlags": 2},
      "sph-fit": {"model": "spherical", "fit": True, "n_lags": 8, "n_tlags": 2}}

# name: (H, W, T, gauge counts per frame (one: the same sites in every frame; T of them: every frame its own), variogram, members,
# embed, embed_time).  St = 2, 6, 9, 10 and 15 are no powers of two and ragged against the 32-wide tiles, as 17 x 23 and its tori are;
# 1, 2, 33 and 65 points are the edges of the 32-point slabs and of the padded system; members 1, 3 and 33 are an odd ensemble, the
# dropped imaginary part and a second 32-member tile with an odd last pair.
CASES = {
    "17x23-t3-exp-nug-n33-m3": (17, 23, 3, (11,), "exp-nug", 3, 2, 2),
    "16-t1-sph-0-n1-m1": (16, 16, 1, (1,), "sph-0", 1, 2, 2),
    "16-t5-exp-fit-n65-m33": (16, 16, 5, (13,), "exp-fit", 33, 2, 2),
    "17x23-t3-sph-nug-n2-m3-e3": (17, 23, 3, (1, 0, 1), "sph-nug", 3, 3, 3),
    "17x23-t3-sph-fit-n60-m3": (17, 23, 3, (20,), "sph-fit", 3, 2, 2),
    "16-t5-exp-0-n33-m33-et3": (16, 16, 5, (5, 9, 6, 7, 6), "exp-0", 33, 2, 3),
    "17x23-t5-sph-0-n65-m1-e3": (17, 23, 5, (13,), "sph-0", 1, 3, 2),
    "8-t4-exp-clip-n48-m3": (8, 8, 4, (12,), "exp-clip", 3, 2, 2),
}
SEED = (3 << 32) | 11


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(e32):
    return max(32.0 * e32, 1e-6)


def _field(t, h, w, seed=0):
    """(t, h, w) fp32 in [0, 1]: a smooth field that moves from frame to frame plus texture."""
    rng = np.random.default_rng(100 + seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.empty((t, h, w), np.float32)
    for i in range(t):
        out[i] = 0.5 + 0.3 * np.sin(0.37 * yy + 0.2 * i) * np.cos(0.29 * xx - 0.3 * i) + 0.15 * rng.random((h, w))
    return out


def _frames(h, w, t, counts, seed=0):
    """(masked, masks) (1, t, 1, h, w) fp32 with `counts` gauges per frame (one count: the same sites in every frame)."""
    rng = np.random.default_rng(seed)
    masks = np.zeros((1, t, 1, h, w), np.float32)
    perm = rng.permutation(h * w)
    for i in range(t):
        n = counts[i % len(counts)]
        idx = perm[:n] if len(counts) == 1 else rng.permutation(h * w)[:n]
        masks[0, i, 0].reshape(-1)[idx] = 1.0
    frames = _field(t, h, w, seed).reshape(1, t, 1, h, w)
    return (frames * masks).astype(np.float32), masks


@functools.lru_cache(maxsize=None)
def case(name):
    """(masked, masks, streams, fp64 members, fp32 members, rho) of a case; built once, never modified."""
    h, w, t, counts, vkey, members, embed, et = CASES[name]
    masked, masks = _frames(h, w, t, counts, seed=len(name))
    streams = np.array([(len(name) << 32) | 5], dtype=np.int64)
    r64, rho = sc.simulation(masked, masks, VG[vkey], members, SEED, streams, embed, et, np.float64)
    r32, _ = sc.simulation(masked, masks, VG[vkey], members, SEED, streams, embed, et, np.float32)
    return masked, masks, streams, r64, r32, rho


def _model(dev, vkey, embed=2, embed_time=2):
    from p2igan_bench.models import build_generator
    return build_generator({"model": {"name": "stkriging", "variogram": VG[vkey],
                                      "ensemble": {"embed": embed, "embed_time": embed_time}}}).to(dev)


def _check(what, got, r64, r32):
    """NaN samples agree; the rest is within the bound.  Returns (err, e32), both relative to max|ref|."""
    nan = np.isnan(r64)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN samples differ")
    scale = float(np.nanmax(np.abs(r64)))
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.abs(got.astype(np.float64) - r64))) / scale
        e32 = float(np.nanmax(np.abs(r32.astype(np.float64) - r64))) / scale
    print(f"{what}: device err {err:.3e}  e32 {e32:.3e}  bound {_rel(e32):.3e}  (of max|ref| = {scale:.3f})")
    assert err <= _rel(e32), (what, err, _rel(e32))
    return err, e32


def test_noise(dev):
    """xi on the torus 6 x 34 x 46 for the pairs 0 and 3 and two streams with a non-zero high word."""
    from p2igan_bench import ops
    St, Sy, Sx = 6, 34, 46
    for stream in ((7 << 32) | 3, (0x9abcdef1 << 32) | 0xfffffffe):
        signed = stream - (1 << 64) if stream >= (1 << 63) else stream
        got = ops.stcs_noise(SEED, signed, 0, 4, St, Sy, Sx, dev).cpu().numpy()
        assert got.shape == (4, St, Sy, Sx, 2) and got.dtype == np.float32
        r64 = sc.noise(SEED, stream, [0, 3], St, Sy, Sx, np.float64)
        r32 = sc.noise(SEED, stream, [0, 3], St, Sy, Sx, np.float32)
        scale = float(np.abs(r64).max())
        for k, q in enumerate((0, 3)):
            g = got[q, ..., 0].astype(np.float64) + 1j * got[q, ..., 1].astype(np.float64)
            err, e32 = float(np.abs(g - r64[k]).max()) / scale, float(np.abs(r32[k].astype(np.complex128) - r64[k]).max()) / scale
            print(f"noise stream {stream:#x} pair {q}: device err {err:.3e}  e32 {e32:.3e}  bound {_rel(e32):.3e}  (of max|xi| = {scale:.3f})")
            assert err <= _rel(e32)
        alone = ops.stcs_noise(SEED, signed, 3, 1, St, Sy, Sx, dev).cpu().numpy()      # a pair is a function of its own index
        assert np.array_equal(alone[0], got[3])


@pytest.mark.parametrize("t,h,w,embed,et", [(3, 17, 23, 2, 2), (5, 16, 16, 2, 3), (1, 16, 16, 3, 2), (4, 8, 8, 2, 2)])
def test_spectrum(dev, t, h, w, embed, et):
    """The amplitude and the clip share of both models, with and without a nugget, and one slow decorrelation that clips."""
    from p2igan_bench import ops
    rows = [(0.05, 0.6, 2.0, 3.0), (0.0, 0.6, 4.0, 4.0), (0.05, 0.6, 3.0, 1.5), (0.02, 0.8, 9.0, 0.5)]
    params = torch.tensor(rows, dtype=torch.float32, device=dev)
    clipped = 0
    for model in ("exponential", "spherical"):
        amp, clip = ops.stcs_spectrum(params, None, ops.KRIG_MODELS[model], t, h, w, embed, et)
        assert amp.shape == (4, et * t, embed * h, embed * w) and amp.dtype == torch.float32 and clip.dtype == torch.float64
        amp, clip = amp.cpu().numpy(), clip.cpu().numpy()
        for i, r in enumerate(rows):
            A, rho = sc.spectrum(r, model, t, h, w, embed, et)
            scale = float(A.max())
            err = float(np.abs(amp[i] - A).max()) / scale
            e32 = float(np.abs(A.astype(np.float32).astype(np.float64) - A).max()) / scale
            print(f"spectrum {model} {r} T {t} {h} x {w} e = {embed} e_t = {et}: A err {err:.3e}  e32 {e32:.3e}  bound {_rel(e32):.3e};  "
                  f"rho {clip[i]:.6e}  restatement {rho:.6e}")
            assert err <= _rel(e32) and abs(clip[i] - rho) <= 1e-9
            clipped += rho > 0
            if model == "exponential" and i == 2 and (t, h, w, embed, et) == (4, 8, 8, 2, 2):
                assert abs(clip[i] - 5.147e-3) <= 5e-7
    assert clipped >= 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_members(dev, name):
    h, w, t, counts, vkey, members, embed, et = CASES[name]
    masked, masks, streams, r64, r32, rho = case(name)
    G = _model(dev, vkey, embed, et)
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    pred, ens = G.forward_simulation(x, m, members, seed=SEED, streams=torch.from_numpy(streams))
    assert ens.shape == (1, t, members, h, w) and ens.dtype == torch.float32 and pred.shape == x.shape
    assert int(G.last_status.sum()) == 0 and G.last_status.numel() == 1
    assert np.isfinite(r64).all()
    _check(name, ens.cpu().numpy(), r64, r32)
    assert torch.equal(pred, G(x, m))                                            # the kriging mean is forward()'s
    at = (m != 0).expand(1, t, members, h, w)
    assert torch.equal(ens[at], x.expand(1, t, members, h, w)[at])               # z at the points, bit for bit
    clip = G.last_ensemble["clip"].cpu().numpy()
    assert G.last_ensemble["embed"] == embed and G.last_ensemble["embed_time"] == et
    assert clip.shape == (1,) and abs(clip[0] - rho[0]) <= 1e-9
    if vkey == "exp-clip":
        assert abs(clip[0] - 5.147e-3) <= 5e-7


def _batch():
    """B = 3 at 16 x 16, T = 3: a sample with a gauge-less frame, a sample without points and a constant sample (a degenerate fit)."""
    h, w, t = 16, 16, 3
    a_masked, a_masks = _frames(h, w, t, (14,), seed=1)
    a_masks[0, 1] = 0.0                                                          # sample 0: 14 gauges, none, 14
    a_masked[0, 1] = 0.0
    b_masks = np.zeros_like(a_masks)                                             # sample 1: no points
    c_masked, c_masks = _frames(h, w, t, (20,), seed=2)
    c_masked = 0.4 * c_masks                                                     # sample 2: a constant field
    return np.concatenate([a_masked, b_masks, c_masked]), np.concatenate([a_masks, b_masks, c_masks])


def test_sample_rules_in_a_batch(dev):
    masked, masks = _batch()
    r64, rho = sc.simulation(masked, masks, VG["exp-fit"], 5, SEED, None, 2, 2, np.float64)
    r32, _ = sc.simulation(masked, masks, VG["exp-fit"], 5, SEED, None, 2, 2, np.float32)
    assert np.isfinite(r64[0]).all() and np.isnan(r64[1]).all() and np.isnan(r64[2]).all()
    assert np.abs(r64[0, 1]).max() > 0                                           # the gauge-less frame is simulated
    G = _model(dev, "exp-fit")
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    pred, ens = G.forward_simulation(x, m, 5, seed=SEED)
    cand = G.last_fit["cand"].cpu().numpy()
    assert cand[0] >= 0 and cand[1] == -1 and cand[2] == -1 and G.last_status.numel() == 3
    _check("sample rules", ens.cpu().numpy(), r64, r32)
    assert torch.equal(pred, G(x, m)) and torch.isfinite(pred).all()             # forward()'s fallbacks are untouched
    clip = G.last_ensemble["clip"].cpu().numpy()
    assert np.isnan(clip[1]) and np.isnan(clip[2]) and abs(clip[0] - rho[0]) <= 1e-9
    # with fixed parameters the sample without points is still NaN, and the constant one has a model
    G = _model(dev, "exp-nug")
    ens = G.forward_simulation(x, m, 2, seed=SEED)[1]
    assert torch.isfinite(ens[0]).all() and torch.isnan(ens[1]).all() and torch.isfinite(ens[2]).all()
    assert torch.isfinite(G.last_ensemble["clip"]).all()


def test_exact_properties(dev):
    name = "17x23-t3-exp-nug-n33-m3"
    h, w, t, counts, vkey, members, embed, et = CASES[name]
    masked, masks, streams, _, _, _ = case(name)
    x, m, st = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev), torch.from_numpy(streams)
    p5, e5 = _model(dev, vkey).forward_simulation(x, m, 5, seed=SEED, streams=st)
    q5, f5 = _model(dev, vkey).forward_simulation(x, m, 5, seed=SEED, streams=st)
    assert torch.equal(p5, q5) and torch.equal(e5, f5)                           # two runs
    p3, e3 = _model(dev, vkey).forward_simulation(x, m, 3, seed=SEED, streams=st)
    assert torch.equal(p3, p5) and torch.equal(e3, e5[:, :, :3])                 # a member does not depend on the ensemble size
    e2 = _model(dev, vkey).forward_simulation(x, m, 2, seed=SEED, streams=st)[1]
    assert torch.equal(e2, e5[:, :, :2])
    for seed, stream in ((SEED, st + 1), (SEED, st + (1 << 32)), (SEED + 1, st), (SEED + (1 << 32), st)):
        other = _model(dev, vkey).forward_simulation(x, m, 3, seed=seed, streams=stream)[1]
        assert float((other - e3).abs().max()) > 0.1                             # and changes with its stream and either seed word
    for bad in (torch.zeros(1, t, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="streams must be an int64 \\(1,\\) tensor"):
            _model(dev, vkey).forward_simulation(x, m, 3, streams=bad)


def test_a_sample_alone_equals_the_sample_in_a_batch_and_in_chunked_systems(dev, monkeypatch):
    """Three samples of 36, 60 and 48 points (one padded size, 64): the second alone, in the batch, and in the batch with the factor
    workspace bounded to one system per chunk."""
    from p2igan_bench.models import classical
    h, w, t = 17, 23, 3
    parts = [_frames(h, w, t, c, seed=20 + i) for i, c in enumerate(((12,), (20,), (10, 30, 8)))]
    masked, masks = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    streams = torch.tensor([5, (1 << 40) + 1000, 7], dtype=torch.int64)
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    G = _model(dev, "sph-fit")
    pred, ens = G.forward_simulation(x, m, 4, seed=SEED, streams=streams)
    fit, status = {k: v.clone() for k, v in G.last_fit.items()}, G.last_status.clone()
    assert int(status.sum()) == 0 and status.numel() == 3 and torch.isfinite(ens).all()
    r64, _ = sc.simulation(masked[1:2], masks[1:2], VG["sph-fit"], 4, SEED, streams[1:2].numpy(), 2, 2, np.float64)
    r32, _ = sc.simulation(masked[1:2], masks[1:2], VG["sph-fit"], 4, SEED, streams[1:2].numpy(), 2, 2, np.float32)
    alone = G.forward_simulation(x[1:2].contiguous(), m[1:2].contiguous(), 4, seed=SEED, streams=streams[1:2])[1]
    _check("alone", alone.cpu().numpy(), r64, r32)
    assert torch.equal(alone, ens[1:2])
    np_ = 64
    monkeypatch.setattr(classical, "_FACTOR_BYTES", 2 * np_ * np_ * 4)           # factor and inverse of one system
    H2 = _model(dev, "sph-fit")
    pred2, ens2 = H2.forward_simulation(x, m, 4, seed=SEED, streams=streams)
    assert torch.equal(pred2, pred) and torch.equal(ens2, ens)
    assert all(torch.equal(fit[k], H2.last_fit[k]) for k in fit) and torch.equal(H2.last_status, status)
    assert torch.equal(H2(x, m), pred)


def test_infer_writes_the_members(dev, tmp_path):
    """scripts/infer.py --ensemble-output with stkriging on a synthetic two-event store at 32 x 32, 3 members, chunks of 4 frames; then
    scripts/evaluate.py --ens takes the directory."""
    from p2igan_bench.data import synth_store, zarr_lite
    from p2igan_bench.data.dataloader import P2IDataModule
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    try:
        import evaluate
        import infer as infer_script
    finally:
        sys.path.pop(0)
    store = tmp_path / "test.zarr"
    synth_store.write_test_zarr(str(store), n_events=2, frames_per_event=20, h=32, w=32)
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "stkriging_ensemble.json")))
    cfg["data"]["test"].update(w=32, h=32, data_root=str(store))
    cfg["data"]["test"]["mask"]["block_sizes"] = [4]
    path = tmp_path / "stkriging_ensemble.json"
    json.dump(cfg, open(path, "w"))
    np.random.seed(cfg["seed"])                                  # the script seeds the global generators before the loader draws the masks
    events = [[t.permute(0, 1, 4, 2, 3).contiguous().numpy() for t in batch][1:] for batch in P2IDataModule(cfg).test_dataloader()]

    def run(tag):
        infer_script.main(["--config", str(path), "--output", str(tmp_path / f"{tag}.zarr"), "--ensemble-output", str(tmp_path / tag),
                           "--members", "3", "--ensemble-seed", "5", "--stride", "4"])
        return [zarr_lite.Group(str(tmp_path / tag / f"member_{k:03d}.zarr")) for k in range(3)]

    first, main = run("a"), zarr_lite.Group(str(tmp_path / "a.zarr"))
    assert sorted(os.listdir(tmp_path / "a")) == [f"member_{k:03d}.zarr" for k in range(3)]
    arrays = []
    for k, g in enumerate(first):
        assert g.attrs["member"] == k and g.attrs["members"] == 3 and g.attrs["seed"] == 5
        assert g.attrs["embed"] == 2 and g.attrs["embed_time"] == 2
        assert g.attrs["model_name"] == "stkriging" and g.attrs["output_scale"] == 255.0 and 0.0 <= g.attrs["clip_share_max"] < 1.0
        assert sorted(g.array_keys()) == sorted(main.array_keys()) == ["event_01", "event_02"]
        for i, (masked, masks) in enumerate(events):
            got = g[f"event_{i + 1:02d}"][:]
            assert got.shape == main[f"event_{i + 1:02d}"][:].shape == (20, 1, 32, 32) and got.dtype == np.float32
            assert np.isfinite(got).all() and (got >= 0).all()
            at = masks[0] != 0
            assert np.array_equal(got[at], (torch.from_numpy(masked[0][at]) * 255.0).numpy())      # the observation x scale
            arrays.append(got)
    assert np.abs(arrays[0] - arrays[2]).max() > 1.0                                               # the members differ
    second = run("b")                                                                              # the same seed: the same arrays
    for g, h in zip(first, second):
        for key in ("event_01", "event_02"):
            assert np.array_equal(g[key][:], h[key][:])
    np.savetxt(tmp_path / "mask.txt", (np.arange(32 * 32).reshape(32, 32) % 11 == 0).astype(np.float64))
    evaluate.main(["--truth", str(store), "--method", f"st={tmp_path / 'a.zarr'}", "--mask", str(tmp_path / "mask.txt"), "--crop-size", "24",
                   "--thresholds", "0.5", "2",
                   "--output", str(tmp_path / "plain"), "--ens", str(tmp_path / "ens"), "--ensemble", f"stcs={tmp_path / 'a'}",
                   "--box-sizes", "1", "4"])
    got = json.loads((tmp_path / "ens" / "metrics.json").read_text())["stcs"]
    assert got["box_1"]["M"] == 3 and got["energy"]["n_frames"] == 40
