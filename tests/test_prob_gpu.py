"""csrc/eval_prob.hip against tests/prob_ref.py (numpy / scipy, fp64).

Bounds.  The seeds are fixed so that no scored element of a case lies within 1e-9 of a decision edge (``edge_count == 0``, asserted),
so every element falls in the same bin on both sides and
  * integer counts are exact;
  * plain fp64 sums (e, |e|, e^2, sigma^2, interval widths, the per-sigma-bin sums) agree within 1e-12 relative;
  * sums through erfc / exp / pow / a division by sigma (CRPS, p, Brier, z, z^2) agree within 1e-9 relative
-- the two bounds tests/test_exp1_gpu.py uses for the same two classes.  The fixed-point sums (p per reliability bin, the PIT
weights) get n * 2^-33 absolute on top: each of the at most n contributions to a bin is stored as rint(v * 2^32) / 2^32, an error of
at most half a unit, 2^-33, and integer addition adds none.  (A PIT bin takes at most one term per pixel: the pixel's own bin
weight, or its prefix weight at a higher index, never both.)"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import prob_ref as pr

pytestmark = pytest.mark.gpu

THR4 = (0.5, 2.0, 4.0, 8.0)
THR8 = (0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0)
LEV8 = (0.1, 0.25, 0.5, 0.68, 0.8, 0.9, 0.95, 0.99)
EDGES16 = tuple(float(v) for v in np.geomspace(0.25, 96.0, 16))
INT_KEYS = ("n", "n_skipped", "n_zero_var", "inside", "o", "sb_n", "rel_n", "rel_o")
PLAIN_KEYS = ("e", "ae", "e2", "s2", "width", "sb_s2", "sb_e2")
SPECIAL_KEYS = ("crps", "p", "brier", "z", "z2")
FIXED_KEYS = ("pit", "rel_p")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _center(shape, rows, cols):
    return (shape[0] - rows) // 2, (shape[1] - cols) // 2


def _embed(rng, base, shape, dtype):
    """base [T, rows, cols] as the centre crop of a [T, *shape] array whose other pixels hold unrelated values."""
    T, rows, cols = base.shape
    if dtype == np.uint8:
        full = rng.integers(0, 256, (T,) + shape).astype(np.uint8)
    else:
        full = rng.uniform(0.0, 300.0, (T,) + shape).astype(dtype)
    top, left = _center(shape, rows, cols)
    full[:, top:top + rows, left:left + cols] = base.astype(dtype)
    return full


def _fields(rng, T, rows, cols):
    """Rain-like truth (40 % exact zeros), a biased noisy prediction (some of it negative) and variances whose sigma spans the
    default edges' underflow and overflow bins."""
    size = (T, rows, cols)
    truth = np.minimum(rng.gamma(0.6, 14.0, size), 250.0) * (rng.random(size) < 0.6)
    pred = truth - 2.0 + rng.normal(0.0, 6.0, size)
    var = np.exp(rng.normal(np.log(16.0), 1.6, size))
    return pred, var, truth


# name -> seed, T, crop (rows, cols), the inputs' (pred, var, truth) shapes (None: the crop) and dtypes, the variance mode, the
# selection, the evaluator's parameters and the special data to plant
CASES = {
    "1x1_T1": dict(seed=1, T=1, crop=(1, 1)),
    "5x5_origins": dict(seed=2, T=3, crop=(5, 5), shapes=((7, 9), (9, 7), (8, 8))),
    "u8_f32_f32_radar_3wg": dict(seed=3, T=3, crop=(36, 36), shapes=((40, 40), (38, 38), (36, 40)), dtypes=("f32", "f32", "u8"),
                                 sel="radar"),
    "u8_f32_f64_gauge": dict(seed=4, T=3, crop=(20, 20), shapes=((24, 24), (20, 20), (22, 26)), dtypes=("f32", "f64", "u8"), sel="gauge"),
    "dressed_scalar": dict(seed=5, T=3, crop=(20, 20), dtypes=("f32", None, "u8"), scalar=37.5, sel="radar"),
    "select_0": dict(seed=6, T=2, crop=(6, 6), sel="none"),
    "select_1": dict(seed=7, T=3, crop=(6, 6), sel="one"),
    "thr8_lev8_edges16_plain": dict(seed=8, T=2, crop=(24, 24), thresholds=THR8, levels=LEV8, edges=EDGES16, censor=False),
    "thr1_lev1_edge1": dict(seed=9, T=2, crop=(12, 12), thresholds=(2.0,), levels=(0.9,), edges=(4.0,)),
    "no_div3_bins": dict(seed=10, T=2, crop=(12, 12), divide_by_3=False, pit_bins=7, rel_bins=32),
    "special_data": dict(seed=11, T=4, crop=(12, 12), dtypes=("f64", "f64", "f64"), special=True),
    "special_data_plain": dict(seed=12, T=4, crop=(12, 12), dtypes=("f32", "f32", "f32"), special=True, censor=False),
    "all_skipped": dict(seed=13, T=2, crop=(5, 5), all_nan=True),
}
for _n in (1, 63, 64, 65, 257, 4099):
    CASES[f"points_{_n}"] = dict(seed=20 + _n, T=1, crop=(1, _n))

_DT = {"f32": np.float32, "f64": np.float64, "u8": np.uint8}


def _plant(rng, pred, var, truth):
    """NaN in each input, a whole NaN-variance frame, negative variances, sigma^2 == 0 pixels (among them y == mu, y == mu' == 0
    with mu < 0, y above and below mu), y == 0 with mu >> sigma (P0 underflows) and a negative truth."""
    T, rows, cols = pred.shape
    flat = rng.permutation(rows * cols)
    at = lambda i: np.unravel_index(flat[i], (rows, cols))      # noqa: E731
    pred[0][at(0)] = np.nan
    var[0][at(1)] = np.nan
    truth[0][at(2)] = np.nan
    var[0][at(3)] = -1.0
    var[0][at(4)] = -1e-30
    for i, (m, y) in enumerate(((7.25, 7.25), (-3.0, 0.0), (5.0, 9.0), (5.0, 2.0), (0.0, 0.0))):
        var[0][at(5 + i)], pred[0][at(5 + i)], truth[0][at(5 + i)] = 0.0, m, y
    for i, (m, s2) in enumerate(((200.0, 4.0), (90.0, 1.0), (40.0, 0.16), (30.0, 1.0))):       # the last: P0 = 5e-198, not yet 0
        var[0][at(10 + i)], pred[0][at(10 + i)], truth[0][at(10 + i)] = s2, m, 0.0
    truth[0][at(14)] = -0.5
    var[2] = np.nan


@functools.lru_cache(maxsize=None)
def build(name):
    """(inputs, evaluator keywords, the cropped arrays, the selection, the reference's sums); built once, never modified."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    T, (rows, cols) = c["T"], c["crop"]
    pred, var, truth = _fields(rng, T, rows, cols)
    dts = c.get("dtypes", ("f64", "f64", "f64"))
    if dts[2] == "u8":
        truth = np.rint(truth)
    if c.get("special"):
        _plant(rng, pred, var, truth)
    if c.get("all_nan"):
        var[0], pred[1] = np.nan, np.nan
    shapes = c.get("shapes", ((rows, cols),) * 3)
    full_p = _embed(rng, pred, shapes[0], _DT[dts[0]])
    full_g = _embed(rng, truth, shapes[2], _DT[dts[2]])
    full_v = c["scalar"] if "scalar" in c else _embed(rng, var, shapes[1], _DT[dts[1]])
    sel_kind, mask, mode, sel = c.get("sel"), None, "radar", None
    if sel_kind in ("radar", "gauge"):
        mask, mode = rng.random((rows, cols)) < 0.15, sel_kind
        sel = ~mask if mode == "radar" else mask
    elif sel_kind == "none":
        mask, sel = np.ones((rows, cols), bool), np.zeros((rows, cols), bool)
    elif sel_kind == "one":
        mask = np.ones((rows, cols), bool)
        mask[3, 2] = False
        sel = ~mask
    kw = dict(thresholds=c.get("thresholds", THR4), levels=c.get("levels", pr.DEFAULT_LEVELS), sigma_edges=c.get("edges", pr.DEFAULT_EDGES),
              pit_bins=c.get("pit_bins", 20), rel_bins=c.get("rel_bins", 10), censor=c.get("censor", True),
              divide_by_3=c.get("divide_by_3", True))

    def crop(a):
        top, left = _center(a.shape[1:], rows, cols)
        return a[:, top:top + rows, left:left + cols]
    cp, cg = crop(full_p), crop(full_g)
    cv = full_v if "scalar" in c else crop(full_v)
    ref = pr.prob_sums(cp, cv, cg, sel, **kw)
    return (full_p, full_v, full_g), dict(crop_size=(rows, cols), mask=mask, mode=mode, **kw), (cp, cv, cg), sel, ref


def assert_sums(tag, got, ref):
    """The bounds of the module's docstring; every figure is printed before it is asserted."""
    n = ref["n"]
    classes = ((PLAIN_KEYS, 1e-12, 0.0), (SPECIAL_KEYS, 1e-9, 0.0), (FIXED_KEYS, 1e-9, n * 2.0 ** -33))
    figures = []
    for keys, rel, extra in classes:
        for k in keys:
            g, w = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
            assert g.shape == w.shape, (tag, k, g.shape, w.shape)
            if g.size:
                figures.append(f"{k} abs {np.abs(g - w).max():.2e} of {np.abs(w).max():.2e}")
    print(f"{tag}: n {n} skipped {ref['n_skipped']} zero-var {ref['n_zero_var']}  " + "  ".join(figures))
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(ref[k], np.int64)), (tag, k, got[k], ref[k])
    for keys, rel, extra in classes:
        for k in keys:
            g, w = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
            assert np.all(np.abs(g - w) <= rel * np.abs(w) + extra), (tag, k, g, w)


def _evaluator(dev, kw):
    from p2igan_bench.evaluation import ProbEvaluator
    return ProbEvaluator(device=dev, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_reference(dev, name):
    (p, v, g), kw, _, _, ref = build(name)
    assert ref["edge_count"] == 0, f"{name}: {ref['edge_count']} elements within 1e-9 of a decision edge: re-seed the case"
    ev = _evaluator(dev, kw)
    ev.update("m", p, g, v)
    assert_sums(name, ev.sums("m"), ref)
    if name == "u8_f32_f32_radar_3wg":
        from p2igan_bench import ops
        assert -(-p.shape[0] * 36 * 36 // ops.PROB_WG_PIXELS) >= 3       # the merge folds several records
    if name == "special_data":
        assert ref["n_zero_var"] == 5 and ref["n_skipped"] >= 6 + 144
    if name in ("all_skipped", "select_0"):
        res = ev.compute()["m"]
        assert res["n"] == 0 and res["n_skipped"] == (50 if name == "all_skipped" else 0) and res["n_zero_var"] == 0
        assert all(np.isnan(res[k]) for k in ("CRPS", "ME", "MAE", "RMSE", "MSDR")) and all(np.isnan(x) for x in res["pit"])
        assert all(np.isnan(x) for x in res["coverage"].values())


def test_scores_match_reference(dev):
    (p, v, g), kw, _, _, ref = build("u8_f32_f32_radar_3wg")
    ev = _evaluator(dev, kw)
    ev.update("m", p, g, v)
    assert_scores(ev.compute()["m"], pr.prob_scores(ref, kw["thresholds"], kw["levels"], kw["sigma_edges"]))


def assert_scores(got, want, path=""):
    """Derived scores: the same keys, integers exact, floats within 1e-9 relative plus the fixed-point allowance (the scores are
    ratios of the sums that assert_sums bounds), NaN exactly where the reference has NaN."""
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), (path, sorted(got), sorted(want))
        for k in want:
            assert_scores(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), path
        for i, (a, b) in enumerate(zip(got, want)):
            assert_scores(a, b, f"{path}[{i}]")
    elif isinstance(want, (int, np.integer)) and not isinstance(want, bool):
        assert got == want, (path, got, want)
    elif isinstance(want, float) and np.isnan(want):
        assert np.isnan(got), (path, got)
    else:
        assert abs(got - want) <= 1e-9 * abs(want) + 2.0 ** -30, (path, got, want)


def test_runs_are_bit_identical(dev):
    (p, v, g), kw, _, _, _ = build("u8_f32_f32_radar_3wg")
    raws = []
    for _ in range(2):
        ev = _evaluator(dev, kw)
        ev.update("m", p, g, v)
        ev.update("m", p[:2], g[:2], 12.5)
        raws.append(ev.raw("m").clone())
    assert torch.equal(raws[0].view(torch.int64), raws[1].view(torch.int64))


def test_two_pieces_equal_one(dev):
    (p, v, g), kw, _, _, ref = build("u8_f32_f32_radar_3wg")
    one, two = _evaluator(dev, kw), _evaluator(dev, kw)
    one.update("m", p, g, v)
    two.update("m", p[:1], g[:1], v[:1])
    two.update("m", p[1:], g[1:], v[1:])
    assert_sums("two pieces", two.sums("m"), one.sums("m"))
    assert_sums("two pieces vs reference", two.sums("m"), ref)


@pytest.mark.parametrize("scalar", [False, True])
def test_launch_cuts_inside_one_update(dev, monkeypatch, scalar):
    """``max_frames`` cuts the three frames of one update into launches of 1 and of 2 frames (2 + 1), with the variance map (cut
    along with the prediction) and with one variance for every pixel.  The workgroups' boundaries move with the cuts, so the fp64
    sums hold at the bounds of two pieces against one, not bit for bit; a cut run repeats itself bit for bit."""
    from p2igan_bench import ops
    (p, v, g), kw, (cp, _, cg), sel, ref = build("u8_f32_f32_radar_3wg")
    if scalar:
        v = 37.5
        ref = pr.prob_sums(cp, v, cg, sel, **{k: x for k, x in kw.items() if k not in ("crop_size", "mask", "mode")})
        assert ref["edge_count"] == 0
    launches, real = [], ops.prob_accumulate
    monkeypatch.setattr(ops, "prob_accumulate", lambda *a, **k: (launches.append(a[0].shape[0]), real(*a, **k))[1])

    def run(max_frames):
        ev = _evaluator(dev, kw)
        ev.max_frames = max_frames
        del launches[:]
        ev.update("m", p, g, v)
        return ev.sums("m"), ev.raw("m").clone(), list(launches)
    whole = run(None)
    assert whole[2] == [3]
    assert_sums(f"one launch (scalar {scalar}) vs reference", whole[0], ref)
    for max_frames, want in ((1, [1, 1, 1]), (2, [2, 1])):
        sums, raw, n = run(max_frames)
        assert n == want
        assert_sums(f"launches of {max_frames} (scalar {scalar})", sums, whole[0])
        assert_sums(f"launches of {max_frames} (scalar {scalar}) vs reference", sums, ref)
        assert torch.equal(raw.view(torch.int64), run(max_frames)[1].view(torch.int64))


def test_krig_uq_end_to_end(dev, tmp_path):
    """KrigingGenerator.forward_uq and cross_validate on a 16 x 16, 4-frame synthetic event with 24 gauges, through run_prob /
    write_prob_outputs and run_prob_points: the files exist, the JSON equals prob_ref on the same arrays, `map` is there for kriging
    and absent for IDW."""
    from p2igan_bench.evaluation import run_prob, run_prob_points, write_prob_outputs
    from p2igan_bench.models import build_generator
    from p2igan_bench.utils import seeded
    mask = seeded.gauge_mask(16, 16, 24)
    frames, masked, masks = seeded.synthetic_batch(1, 4, 16, 16, mask)
    x, m = masked.to(dev), masks.to(dev)
    vg = {"model": "exponential", "fit": False, "nugget": 0.002, "psill": 0.03, "range": 6.0}
    K = build_generator({"model": {"name": "kriging", "variogram": vg}}).to(dev)
    idw = build_generator({"model": {"name": "idw"}}).to(dev)
    pred, var = K.forward_uq(x, m)
    truth = (frames[0, :, 0] * 255.0).numpy().astype(np.float32)
    preds = {"kriging": (pred[0, :, 0] * 255.0).clamp(min=0.0).cpu().numpy(), "idw": (idw(x, m)[0, :, 0] * 255.0).clamp(min=0.0).cpu().numpy()}
    variances = {"kriging": (var[0, :, 0] * 255.0 ** 2).cpu().numpy()}
    gmask = masks[0, 0, 0].numpy() != 0
    assert gmask.shape == (16, 16) and int(gmask.sum()) == 24
    res = run_prob(preds, variances, truth, gmask, "radar", 16, thresholds=THR4, device=dev)
    out = tmp_path / "prob"
    write_prob_outputs(str(out), res)
    for f in ("metrics.json", "metrics.txt", "prob_data.npz", "prob_panels.pdf"):
        assert (out / f).is_file() and (out / f).stat().st_size > 0, f
    got = json.loads((out / "metrics.json").read_text())
    assert sorted(got) == ["idw", "kriging"] and "map" in got["kriging"] and "map" not in got["idw"]
    assert "CRPSS_map_vs_dressed" in got["kriging"] and "CRPSS_map_vs_dressed" not in got["idw"]
    kw = dict(thresholds=THR4, levels=pr.DEFAULT_LEVELS, sigma_edges=pr.DEFAULT_EDGES)
    dressed = {}
    for name in preds:
        point = pr.prob_sums(preds[name], 0.0, truth, ~gmask, **kw)
        mse = point["e2"] / point["n"]
        want = dressed[name] = pr.prob_scores(pr.prob_sums(preds[name], mse, truth, ~gmask, **kw), **kw)
        d = dict(got[name]["dressed"])
        assert d.pop("sigma0_sq_in_sample") is True and abs(d.pop("sigma0_sq") - mse) <= 1e-12 * mse
        assert_scores(d, want)
    want = pr.prob_scores(pr.prob_sums(preds["kriging"], variances["kriging"], truth, ~gmask, **kw), **kw)
    assert_scores(got["kriging"]["map"], want)
    assert want["n_zero_var"] == 0 and want["n"] == 4 * (256 - 24)
    crpss = 1.0 - want["CRPS"] / dressed["kriging"]["CRPS"]
    assert abs(got["kriging"]["CRPSS_map_vs_dressed"] - crpss) <= 1e-8
    assert any(line.startswith("CRPS_kriging_map: ") for line in (out / "metrics.txt").read_text().splitlines())
    assert any(line.startswith("COV90_idw_dressed: ") for line in (out / "metrics.txt").read_text().splitlines())
    assert any(line.startswith("BRIER_kriging_map_thr2: ") for line in (out / "metrics.txt").read_text().splitlines())

    # the cross-validation columns as scripts/crossvalidate.py collects them
    loo = K.cross_validate(x, m)
    counts = loo.counts.cpu().numpy()
    col = lambda a: np.concatenate([a.cpu().numpy()[f, :int(c)] for f, c in enumerate(counts)])       # noqa: E731
    z, zp, zv = col(loo.z), col(loo.pred), col(loo.var)
    assert len(z) == 4 * 24
    cv = run_prob_points(z, zp, zv, 255.0, name="kriging", thresholds=THR4, device=dev)
    write_prob_outputs(str(tmp_path / "cv"), cv, stem="prob", figure=False)
    for f in ("prob.json", "prob.txt", "prob_data.npz"):
        assert (tmp_path / "cv" / f).is_file(), f
    got = json.loads((tmp_path / "cv" / "prob.json").read_text())
    z64, p64, v64 = (a.astype(np.float64).reshape(1, 1, -1) for a in (z, zp, zv))
    want = pr.prob_scores(pr.prob_sums(p64 * 255.0, v64 * 255.0 ** 2, z64 * 255.0, None, **kw), **kw)
    assert_scores(got["kriging"]["map"], want)
    assert want["n"] + want["n_skipped"] == len(z) and want["n"] > 0


def _script(name):
    from conftest import PKG
    import sys
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_evaluate_cli_end_to_end(dev, tmp_path):
    """scripts/evaluate.py --prob on zarrs of [T, 1, H, W] events: the files, the JSON equal to run_prob on the same arrays, the
    other outputs untouched by --prob, and the refusals that need the zarrs (a missing variance event, disagreeing output scales)."""
    from p2igan_bench.data import zarr_lite
    from p2igan_bench.evaluation import run_prob
    evaluate = _script("evaluate")
    S, H, W = 12, 16, 18
    rng = np.random.default_rng(41)
    truth, preds, var = {}, {"krig": {}, "gan": {}}, {}
    for i in range(2):
        p, v, g = _fields(rng, 3 + i, H, W)
        k = f"event_{i + 1:02d}"
        truth[k] = np.rint(g).astype(np.uint8)[:, None]
        preds["krig"][k], preds["gan"][k] = np.maximum(p, 0.0).astype(np.float32)[:, None], np.maximum(p + 3.0, 0.0).astype(np.float32)[:, None]
        var[k] = v.astype(np.float32)[:, None]
        var[k][0] = np.nan                                     # a frame without a model
    for name, events, attrs in (("truth", truth, {}), ("krig", preds["krig"], {"output_scale": 255.0}), ("gan", preds["gan"], {}),
                                ("kvar", var, {"output_scale": 255.0}), ("kvar1", var, {"output_scale": 1.0}),
                                ("kvar_short", {"event_01": var["event_01"]}, {})):
        grp = zarr_lite.Group(str(tmp_path / f"{name}.zarr"), "w")
        for k, v in events.items():
            grp.create_dataset(k, v)
        if attrs:
            grp.attrs.update(attrs)
    mask = np.arange(H * W).reshape(H, W) % 7 == 0
    np.savetxt(tmp_path / "mask.txt", mask.astype(np.float64))
    base = ["--truth", str(tmp_path / "truth.zarr"), "--method", f"krig={tmp_path / 'krig.zarr'}", "--method", f"gan={tmp_path / 'gan.zarr'}",
            "--mask", str(tmp_path / "mask.txt"), "--crop-size", str(S), "--thresholds", "0.5", "2"]
    evaluate.main(base + ["--output", str(tmp_path / "plain")])
    pdir = tmp_path / "prob"
    evaluate.main(base + ["--output", str(tmp_path / "with"), "--prob", str(pdir), "--variance", f"krig={tmp_path / 'kvar.zarr'}",
                          "--levels", "0.5", "0.9"])
    for f in ("metrics.json", "metrics.txt"):
        assert (tmp_path / "with" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    for f in ("metrics.json", "metrics.txt", "prob_data.npz", "prob_panels.pdf"):
        assert (pdir / f).stat().st_size > 0, f
    top, left = (H - S) // 2, (W - S) // 2
    want = run_prob(preds, {"krig": var}, truth, mask[top:top + S, left:left + S], "radar", S, thresholds=(0.5, 2.0), levels=(0.5, 0.9))
    assert (pdir / "metrics.json").read_text() == json.dumps(want, indent=2, sort_keys=True)
    assert list(want) == ["krig", "gan"] and "map" in want["krig"] and "map" not in want["gan"]
    sel = int((~mask[top:top + S, left:left + S]).sum())
    assert want["krig"]["map"]["n_skipped"] == 2 * sel and want["krig"]["map"]["n"] == 5 * sel and want["krig"]["dressed"]["n"] == 7 * sel
    ref = pr.prob_sums(np.concatenate([preds["krig"][k][:, 0, top:top + S, left:left + S] for k in truth]),
                       np.concatenate([var[k][:, 0, top:top + S, left:left + S] for k in truth]),
                       np.concatenate([truth[k][:, 0, top:top + S, left:left + S] for k in truth]), ~mask[top:top + S, left:left + S],
                       thresholds=(0.5, 2.0), levels=(0.5, 0.9))
    assert ref["edge_count"] == 0
    assert_scores(want["krig"]["map"], pr.prob_scores(ref, (0.5, 2.0), (0.5, 0.9)))
    with pytest.raises(SystemExit, match="lacks truth event"):
        evaluate.main(base + ["--output", str(tmp_path / "o2"), "--prob", str(tmp_path / "p2"), "--variance", f"krig={tmp_path / 'kvar_short.zarr'}"])
    with pytest.raises(SystemExit, match="output_scale"):
        evaluate.main(base + ["--output", str(tmp_path / "o3"), "--prob", str(tmp_path / "p3"), "--variance", f"krig={tmp_path / 'kvar1.zarr'}"])
    assert not (tmp_path / "p2").exists() and not (tmp_path / "p3").exists()


def test_crossvalidate_cli_end_to_end(dev, tmp_path):
    """scripts/crossvalidate.py --prob on a synthetic two-event store at 32 x 32: prob.json / prob.txt / prob_data.npz from the
    collected columns equal prob_ref on loo_data.npz, and the run's other files are byte for byte those of a run without --prob."""
    from conftest import PKG
    from p2igan_bench.data import synth_store
    cv = _script("crossvalidate")
    store = tmp_path / "test.zarr"
    synth_store.write_test_zarr(str(store), n_events=2, frames_per_event=8, h=32, w=32)
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "kriging_baseline.json")))
    cfg["data"]["test"].update(w=32, h=32, data_root=str(store))
    cfg["data"]["test"]["mask"]["block_sizes"] = [4]
    path = tmp_path / "kriging.json"
    json.dump(cfg, open(path, "w"))
    a, b = tmp_path / "plain", tmp_path / "prob"
    cv.main(["--config", str(path), "--output", str(a), "--stride", "8"])
    cv.main(["--config", str(path), "--output", str(b), "--stride", "8", "--prob"])
    assert sorted(os.listdir(a)) == ["loo.json", "loo.txt", "loo_data.npz"]
    assert sorted(os.listdir(b)) == ["loo.json", "loo.txt", "loo_data.npz", "prob.json", "prob.txt", "prob_data.npz"]
    for f in ("loo.json", "loo.txt"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    da, db = np.load(a / "loo_data.npz"), np.load(b / "loo_data.npz")
    assert sorted(da.files) == sorted(db.files) and all(np.array_equal(da[k], db[k], equal_nan=True) for k in da.files)
    got = json.loads((b / "prob.json").read_text())
    assert list(got) == ["kriging"] and sorted(got["kriging"]) == ["CRPSS_map_vs_dressed", "dressed", "map"]
    col = lambda k, s: db[k].astype(np.float64).reshape(1, 1, -1) * s      # noqa: E731
    kw = dict(thresholds=(0.5, 2.0, 4.0, 8.0))
    ref = pr.prob_sums(col("pred", 255.0), col("var", 255.0 ** 2), col("z", 255.0), None, **kw)
    assert ref["edge_count"] == 0 and ref["n"] > 0 and ref["n"] + ref["n_skipped"] == len(db["z"])
    assert_scores(got["kriging"]["map"], pr.prob_scores(ref, **kw))
    assert (b / "prob.txt").read_text().startswith("CRPS_kriging_dressed: ")


def _far_crop_values(T=5, n=65):
    """(pred, var, truth) of the far-offset test's crop: uint8 prediction and truth, f32 variance, [T, 1, n]."""
    rng = np.random.default_rng(77)
    p, v, g = _fields(rng, T, 1, n)
    p8, g8 = np.clip(np.rint(p), 0, 255).astype(np.uint8), np.rint(g).astype(np.uint8)
    p8[(p8 == g8) & (g8 > 0)] += 1          # y == mu > 0 is u = Phi(0) = 0.5, exactly on a PIT bin edge: kept out of this case
    return p8, v.astype(np.float32), g8


def test_element_offsets_past_2_to_the_32(dev):
    """uint8 inputs of 5 frames of 1 x (2^30 + 128): the centre crop of frame 2 starts past element 2^31 and that of frame 4 past
    2^32, where a 32-bit offset would wrap and read the zeros around the crop.  The variance is a crop-sized input of its own
    extent (origin 0).  Only the 65 crop columns hold data, so the reference is 325 pixels."""
    W, n, T = 2 ** 30 + 128, 65, 5
    cp, cv, cg = _far_crop_values(T, n)
    kw = dict(thresholds=THR4, levels=pr.DEFAULT_LEVELS, sigma_edges=pr.DEFAULT_EDGES)
    ref = pr.prob_sums(cp, cv, cg, None, **kw)
    assert ref["edge_count"] == 0 and ref["n"] == T * n
    left = (W - n) // 2
    assert 2 * W + left > 2 ** 31 and 4 * W + left > 2 ** 32
    pred = torch.zeros((T, 1, W), dtype=torch.uint8, device=dev)
    truth = torch.zeros((T, 1, W), dtype=torch.uint8, device=dev)
    pred[:, :, left:left + n] = torch.from_numpy(cp).to(dev)
    truth[:, :, left:left + n] = torch.from_numpy(cg).to(dev)
    ev = _evaluator(dev, dict(crop_size=(1, n), **kw))
    ev.update("m", pred, truth, torch.from_numpy(cv).to(dev))
    assert_sums("far offsets", ev.sums("m"), ref)
