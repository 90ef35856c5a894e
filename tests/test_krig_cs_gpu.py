"""Conditional simulation on the GPU (KrigingGenerator.forward_ensemble on csrc/krig_cs.hip) against the fp64 numpy restatement
(tests/krig_cs_ref.py).

Error bound of every comparison, the rule of the classical baselines: device error <= max(32 e32, 1e-6) scale against the fp64
restatement, with e32 the fp32 restatement's own error against fp64 relative to the same scale, computed in the same test.  scale =
max|xi| for the noise, max A for the amplitude, max|ref| of the case for the members."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import krig_cs_ref as cs
from conftest import PKG

pytestmark = pytest.mark.gpu

VG = {"exp-nug": {"model": "exponential", "fit": False, "nugget": 0.05, "psill": 0.6, "range": 3.0},
      "exp-0": {"model": "exponential", "fit": False, "nugget": 0.0, "psill": 0.6, "range": 4.0},
      "sph-nug": {"model": "spherical", "fit": False, "nugget": 0.02, "psill": 0.8, "range": 9.0},
      "sph-0": {"model": "spherical", "fit": False, "nugget": 0.0, "psill": 0.8, "range": 6.0},
      "exp-fit": {"model": "exponential", "fit": True, "n_lags": 8},
      "sph-fit": {"model": "spherical", "fit": True, "n_lags": 8}}

# name: (H, W, T, gauge counts (one: the sample's frames share the set; T of them: every frame its own), variogram, share_sets,
# members, embed).  The counts 1, 2, 31, 32, 33 and 65 are the edges of the 32-wide gauge slabs and of the padded system size;
# members 1, 2, 5, 32 and 33 are an odd ensemble, the dropped imaginary part and a second 32-column tile; 17 x 23 is ragged in every
# tile dimension of both DFT products.
CASES = {
    "16-exp-nug-n12-m5": (16, 16, 2, (12,), "exp-nug", True, 5, 2),
    "16-sph-0-n31-m2": (16, 16, 3, (31,), "sph-0", True, 2, 2),
    "24x40-exp-fit-n1-2-33-m2": (24, 40, 3, (1, 2, 33), "exp-fit", True, 2, 2),
    "17x23-sph-fit-n32-m33": (17, 23, 2, (32,), "sph-fit", True, 33, 2),
    "17x23-exp-0-n65-perframe-m32": (17, 23, 2, (65,), "exp-0", False, 32, 2),
    "24x40-sph-nug-n65-m1": (24, 40, 2, (65,), "sph-nug", True, 1, 2),
    "16-sph-nug-n33-e3-m5": (16, 16, 2, (33,), "sph-nug", True, 5, 3),
    "17x23-exp-nug-n2-31-perframe-m5": (17, 23, 2, (2, 31), "exp-nug", True, 5, 2),
    # T M = 165 columns of one shared system: the predictor's second column group (one full 32-column tile and one of 5)
    "16-exp-nug-n33-m33-t5": (16, 16, 5, (33,), "exp-nug", True, 33, 2),
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
    """(masked, masks) (1, t, 1, h, w) fp32 with `counts` gauges per frame (one count: the same set in every frame)."""
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
    h, w, t, counts, vkey, _, members, embed = CASES[name]
    masked, masks = _frames(h, w, t, counts, seed=len(name))
    streams = (np.arange(t, dtype=np.int64)[None, :] + 5) | (np.int64(len(name)) << 32)
    r64, rho = cs.ensemble(masked, masks, VG[vkey], members, SEED, streams, embed, np.float64)
    r32, _ = cs.ensemble(masked, masks, VG[vkey], members, SEED, streams, embed, np.float32)
    return masked, masks, streams, r64, r32, rho


def _model(dev, vkey, share=True, embed=2):
    from p2igan_bench.models import build_generator
    return build_generator({"model": {"name": "kriging", "variogram": VG[vkey], "share_sets": share, "ensemble": {"embed": embed}}}).to(dev)


def _check(what, got, r64, r32):
    """NaN frames agree; the rest is within the bound.  Returns (err, e32), both relative to max|ref|."""
    nan = np.isnan(r64)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN frames differ")
    scale = float(np.nanmax(np.abs(r64)))
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.abs(got.astype(np.float64) - r64))) / scale
        e32 = float(np.nanmax(np.abs(r32.astype(np.float64) - r64))) / scale
    print(f"{what}: device err {err:.3e}  e32 {e32:.3e}  bound {_rel(e32):.3e}  (of max|ref| = {scale:.3f})")
    assert err <= _rel(e32), (what, err, _rel(e32))
    return err, e32


def test_noise(dev):
    """xi at S = 34 x 46 for the pairs 0 and 3 and two streams with a non-zero high word."""
    from p2igan_bench import ops
    Sy, Sx = 34, 46
    for stream in ((7 << 32) | 3, (0x9abcdef1 << 32) | 0xfffffffe):
        signed = stream - (1 << 64) if stream >= (1 << 63) else stream
        got = ops.krig_cs_noise(SEED, signed, 0, 4, Sy, Sx, dev).cpu().numpy()
        assert got.shape == (4, Sy, Sx, 2) and got.dtype == np.float32
        r64 = cs.noise(SEED, stream, [0, 3], Sy, Sx, np.float64)
        r32 = cs.noise(SEED, stream, [0, 3], Sy, Sx, np.float32)
        scale = float(np.abs(r64).max())
        for k, q in enumerate((0, 3)):
            g = got[q, ..., 0].astype(np.float64) + 1j * got[q, ..., 1].astype(np.float64)
            err, e32 = float(np.abs(g - r64[k]).max()) / scale, float(np.abs(r32[k].astype(np.complex128) - r64[k]).max()) / scale
            print(f"noise stream {stream:#x} pair {q}: device err {err:.3e}  e32 {e32:.3e}  bound {_rel(e32):.3e}  (of max|xi| = {scale:.3f})")
            assert err <= _rel(e32)
        alone = ops.krig_cs_noise(SEED, signed, 3, 1, Sy, Sx, dev).cpu().numpy()      # a pair is a function of its own index
        assert np.array_equal(alone[0], got[3])


@pytest.mark.parametrize("embed", [2, 3])
@pytest.mark.parametrize("h,w", [(16, 16), (24, 40), (17, 23)])
def test_spectrum(dev, h, w, embed):
    """The amplitude and the clip share of both models, with and without a nugget, and one range long enough to clip."""
    from p2igan_bench import ops
    rows = [(0.05, 0.6, 3.0), (0.0, 0.6, 5.0), (0.05, 0.6, 30.0)]
    params = torch.tensor([r + (0.0,) for r in rows], dtype=torch.float32, device=dev)
    clipped = 0
    for model in ("exponential", "spherical"):
        amp, clip = ops.krig_cs_spectrum(params, None, ops.KRIG_MODELS[model], h, w, embed)
        assert amp.shape == (3, embed * h, embed * w) and amp.dtype == torch.float32 and clip.dtype == torch.float64
        amp, clip = amp.cpu().numpy(), clip.cpu().numpy()
        for i, r in enumerate(rows):
            A, rho = cs.spectrum(r, model, h, w, embed)
            scale = float(A.max())
            err = float(np.abs(amp[i] - A).max()) / scale
            e32 = float(np.abs(A.astype(np.float32).astype(np.float64) - A).max()) / scale
            print(f"spectrum {model} {r} {h} x {w} e = {embed}: A err {err:.3e}  e32 {e32:.3e}  bound {_rel(e32):.3e};  "
                  f"rho {clip[i]:.6e}  restatement {rho:.6e}")
            assert err <= _rel(e32) and abs(clip[i] - rho) <= 1e-9
            clipped += rho > 0
    assert clipped >= 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_members(dev, name):
    h, w, t, counts, vkey, share, members, embed = CASES[name]
    masked, masks, streams, r64, r32, rho = case(name)
    G = _model(dev, vkey, share, embed)
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    pred, ens = G.forward_ensemble(x, m, members, seed=SEED, streams=torch.from_numpy(streams))
    assert ens.shape == (1, t, members, h, w) and ens.dtype == torch.float32 and pred.shape == x.shape
    shared = len(counts) == 1 and share
    assert int(G.last_status.sum()) == 0 and G.last_status.numel() == (1 if shared else t)
    assert np.isfinite(r64).all()
    _check(name, ens.cpu().numpy(), r64, r32)
    assert torch.equal(pred, G(x, m))                                            # the kriging mean is forward()'s
    at = (m != 0).expand(1, t, members, h, w)
    assert torch.equal(ens[at], x.expand(1, t, members, h, w)[at])               # z at the gauge pixels, bit for bit
    clip = G.last_ensemble["clip"].cpu().numpy()
    assert G.last_ensemble["embed"] == embed and clip.shape == (1,) and abs(clip[0] - rho[0]) <= 1e-9


def test_frame_rules_in_a_batch(dev):
    """A frame without gauges, a sample whose gauges all hold one value (a degenerate fit) and a healthy sample in one batch."""
    h = w = 16
    a_masked, a_masks = _frames(h, w, 2, (12,), seed=1)
    a_masks[0, 0] = 0.0                                                          # sample 0: no gauges, then 12
    a_masked[0, 0] = 0.0
    b_masked, b_masks = _frames(h, w, 2, (20,), seed=2)
    b_masked = 0.4 * b_masks                                                     # sample 1: a constant field
    c_masked, c_masks = _frames(h, w, 2, (33,), seed=3)                          # sample 2: healthy
    masked, masks = np.concatenate([a_masked, b_masked, c_masked]), np.concatenate([a_masks, b_masks, c_masks])
    r64, rho = cs.ensemble(masked, masks, VG["exp-fit"], 5, SEED, None, 2, np.float64)
    r32, _ = cs.ensemble(masked, masks, VG["exp-fit"], 5, SEED, None, 2, np.float32)
    assert np.isnan(r64[0, 0]).all() and np.isfinite(r64[0, 1]).all() and np.isnan(r64[1]).all() and np.isfinite(r64[2]).all()
    G = _model(dev, "exp-fit")
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    pred, ens = G.forward_ensemble(x, m, 5, seed=SEED)
    assert int(G.last_fit["cand"][1]) == -1 and G.last_status.numel() == 6       # sample 0's frames differ: one system per frame
    _check("frame rules", ens.cpu().numpy(), r64, r32)
    assert torch.equal(pred, G(x, m)) and torch.isfinite(pred).all()             # forward()'s fallbacks are untouched
    clip = G.last_ensemble["clip"].cpu().numpy()
    assert np.isnan(clip[1]) and np.abs(clip[[0, 2]] - rho[[0, 2]]).max() <= 1e-9


@pytest.mark.parametrize("name", ["16-exp-nug-n12-m5", "17x23-exp-nug-n2-31-perframe-m5"])
def test_exact_properties(dev, name):
    h, w, t, counts, vkey, share, members, embed = CASES[name]
    masked, masks, streams, r64, r32, _ = case(name)
    x, m, st = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev), torch.from_numpy(streams)
    assert members == 5
    p5, e5 = _model(dev, vkey, share, embed).forward_ensemble(x, m, 5, seed=SEED, streams=st)
    q5, f5 = _model(dev, vkey, share, embed).forward_ensemble(x, m, 5, seed=SEED, streams=st)
    assert torch.equal(p5, q5) and torch.equal(e5, f5)                           # two runs
    p3, e3 = _model(dev, vkey, share, embed).forward_ensemble(x, m, 3, seed=SEED, streams=st)
    assert torch.equal(p3, p5) and torch.equal(e3, e5[:, :, :3])                 # a member does not depend on the ensemble size
    other = _model(dev, vkey, share, embed).forward_ensemble(x, m, 3, seed=SEED, streams=st + 1)[1]
    assert float((other - e3).abs().max()) > 0.1                                 # and changes with its stream
    if share and len(counts) == 1:                                               # per-frame systems give the shared path's members
        per = _model(dev, vkey, False, embed).forward_ensemble(x, m, 5, seed=SEED, streams=st)[1]
        scale = float(np.abs(r64).max())
        e32 = float(np.abs(r32.astype(np.float64) - r64).max()) / scale
        assert float((per - e5).abs().max()) / scale <= 2 * _rel(e32)


def test_a_sample_alone_equals_the_sample_in_a_batch(dev):
    h, w, t = 17, 23, 2
    parts = [_frames(h, w, t, c, seed=20 + i) for i, c in enumerate(((12,), (33,), (5, 40)))]
    masked, masks = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    streams = torch.arange(3 * t, dtype=torch.int64).view(3, t) * 1000 + (1 << 40)
    G = _model(dev, "sph-fit")
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    ens = G.forward_ensemble(x, m, 4, seed=SEED, streams=streams)[1]
    r64, _ = cs.ensemble(masked[1:2], masks[1:2], VG["sph-fit"], 4, SEED, streams[1:2].numpy(), 2, np.float64)
    r32, _ = cs.ensemble(masked[1:2], masks[1:2], VG["sph-fit"], 4, SEED, streams[1:2].numpy(), 2, np.float32)
    alone = G.forward_ensemble(x[1:2].contiguous(), m[1:2].contiguous(), 4, seed=SEED, streams=streams[1:2])[1]
    _, e32 = _check("alone", alone.cpu().numpy(), r64, r32)
    _check("in a batch of three", ens[1:2].cpu().numpy(), r64, r32)
    assert float((alone - ens[1:2]).abs().max()) / float(np.abs(r64).max()) <= 2 * _rel(e32)


def test_infer_writes_the_members(dev, tmp_path):
    """scripts/infer.py --ensemble-output on a synthetic two-event store at 32 x 32 with 3 members."""
    from p2igan_bench.data import synth_store, zarr_lite
    from p2igan_bench.data.dataloader import P2IDataModule
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import infer as infer_script
    store = tmp_path / "test.zarr"
    synth_store.write_test_zarr(str(store), n_events=2, frames_per_event=20, h=32, w=32)
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "kriging_ensemble.json")))
    cfg["data"]["test"].update(w=32, h=32, data_root=str(store))
    cfg["data"]["test"]["mask"]["block_sizes"] = [4]
    path = tmp_path / "kriging_ensemble.json"
    json.dump(cfg, open(path, "w"))
    np.random.seed(cfg["seed"])                                  # the script seeds the global generators before the loader draws the masks
    events = [[t.permute(0, 1, 4, 2, 3).contiguous().numpy() for t in batch][1:] for batch in P2IDataModule(cfg).test_dataloader()]

    def run(tag, *extra):
        infer_script.main(["--config", str(path), "--output", str(tmp_path / f"{tag}.zarr"), "--ensemble-output", str(tmp_path / tag),
                           "--members", "3", "--ensemble-seed", "5", "--passes", "2"] + list(extra))
        return [zarr_lite.Group(str(tmp_path / tag / f"member_{k:03d}.zarr")) for k in range(3)]

    first, main = run("a"), zarr_lite.Group(str(tmp_path / "a.zarr"))
    assert sorted(os.listdir(tmp_path / "a")) == [f"member_{k:03d}.zarr" for k in range(3)]
    arrays = []
    for k, g in enumerate(first):
        assert g.attrs["member"] == k and g.attrs["members"] == 3 and g.attrs["seed"] == 5 and g.attrs["embed"] == 2
        assert g.attrs["model_name"] == "kriging" and g.attrs["output_scale"] == 255.0 and 0.0 <= g.attrs["clip_share_max"] < 1.0
        assert sorted(g.array_keys()) == sorted(main.array_keys()) == ["event_01", "event_02"]
        for i, (masked, masks) in enumerate(events):
            got = g[f"event_{i + 1:02d}"][:]
            assert got.shape == main[f"event_{i + 1:02d}"][:].shape == (20, 1, 32, 32) and got.dtype == np.float32
            assert np.isfinite(got).all() and (got >= 0).all()
            at = masks[0] != 0
            assert np.array_equal(got[at], (torch.from_numpy(masked[0][at]) * 255.0).numpy())      # the observation x scale
            arrays.append(got)
    assert np.abs(arrays[0] - arrays[2]).max() > 1.0                                               # the members differ
    run("b")                                                                                       # the same seed: the same bytes
    files = sorted(os.path.relpath(os.path.join(d, f), tmp_path / "a") for d, _, fs in os.walk(tmp_path / "a") for f in fs)
    assert len(files) >= 3 * (2 + 2 * 2) and files == sorted(os.path.relpath(os.path.join(d, f), tmp_path / "b")
                                                            for d, _, fs in os.walk(tmp_path / "b") for f in fs)
    for rel in files:
        assert open(tmp_path / "a" / rel, "rb").read() == open(tmp_path / "b" / rel, "rb").read(), rel
    with pytest.raises(FileExistsError):
        run("a2", "--ensemble-output", str(tmp_path / "a"))
    assert not (tmp_path / "a2.zarr").exists()
    # the chunk length changes the fit, not the noise: the streams are (event << 32) | frame
    from p2igan_bench.inference import infer_event_ensemble
    from p2igan_bench.models import build_generator
    G = build_generator({"model": dict(cfg["model"], variogram=VG["exp-nug"])}).to(dev)
    masked, masks = (torch.from_numpy(a).to(dev) for a in events[1])
    e16 = infer_event_ensemble(G, masked, masks, 3, 5, 1, 16, 255.0)
    e8 = infer_event_ensemble(G, masked, masks, 3, 5, 1, 8, 255.0)
    assert e16.shape == (20, 3, 32, 32) and float((e16 - e8).abs().max()) <= 1e-4 * float(e16.abs().max())
