"""csrc/eval_ens.hip against tests/ens_ref.py (numpy, fp64).

Bounds, the two classes of tests/test_prob_gpu.py.  The box values are formed by the same additions in the same order on both
sides, so every decision (rank, ties, member counts, the skip) is made on equal numbers; the sigma-bin and the thresholds are
guarded by ``edge_count == 0`` (no scored value within 1e-9 of an edge, asserted).  Then
  * every int64 section (counts, the rank histogram in units of 2^-32, the reliability tables) is exactly equal;
  * plain fp64 sums (CRPS, fair CRPS, e, |e|, e^2, s^2, p, Brier, the per-sigma-bin sums) agree within 1e-12 relative;
  * sums through a square root (the energy score, the variogram score) agree within 1e-9 relative.
Every figure is printed before it is asserted."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import ens_ref as er

pytestmark = pytest.mark.gpu

T, ROWS, COLS, H, W = 3, 17, 23, 20, 29
THR = (0.5, 2.0, 8.0)
BOXES = (1, 4, 5)
INT_KEYS = ("n", "n_skipped", "o", "rank", "sb_n", "rel_n", "rel_o")
PLAIN_KEYS = ("crps", "crps_fair", "e", "ae", "e2", "s2", "p", "brier", "sb_s2", "sb_e2")
MS = (1, 2, 3, 33, 64)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _xq():
    from p2igan_bench.evaluation import pixel_threshold
    return tuple(pixel_threshold(q, True) for q in THR)


def _dtypes(M, kind):
    return [np.float32 if kind == "f32" or (kind == "mix" and m % 2 == 0) else np.float64 for m in range(M)]


def _rain(rng, M, t, rows, cols, kinds):
    """Truth (uint8 values, 40 % exact zeros) and M members = max(truth + 3 + noise, 0) rounded to their dtypes, as fp64 arrays.
    Frame 0: an all-zero truth under members clipped at 0, the ties of rain."""
    size = (t, rows, cols)
    truth = np.rint(np.minimum(rng.gamma(0.6, 40.0, size), 250.0) * (rng.random(size) < 0.6))
    truth[0] = 0.0
    members = np.empty((M,) + size)
    for m in range(M):
        x = np.maximum(truth + 3.0 + rng.normal(0.0, 12.0, size), 0.0)
        x[0] = np.maximum(rng.normal(-5.0, 8.0, size[1:]), 0.0)
        members[m] = x.astype(kinds[m]).astype(np.float64)
    return members, truth


@functools.lru_cache(maxsize=None)
def build(M, kind, sel_kind, nan_frame=False):
    """(member arrays [T, H, W], their crop origins, the truth and its origin, the mask, the selection, the cropped fp64 members and
    truth); built once, never modified.  Every input has its own crop origin inside its 20 x 29 (they cycle through the 4 x 7
    that exist).  Frame 1 holds a few NaN and one inf; with ``nan_frame`` the last member's frame 2 is NaN: a frame without a valid pixel."""
    rng = np.random.default_rng(1000 + 7 * M + len(kind) + (3 if sel_kind else 0))
    kinds = _dtypes(M, kind)
    members, truth = _rain(rng, M, T, ROWS, COLS, kinds)
    for i in range(5):
        members[rng.integers(M), 1, rng.integers(ROWS), rng.integers(COLS)] = np.nan
    members[M - 1, 1, 3, 4] = np.inf
    if nan_frame:
        members[M - 1, 2] = np.nan
    mask = sel = None
    if sel_kind:
        mask = rng.random((ROWS, COLS)) < 0.15
        mask[4:8, 8:12] = True                           # box (1, 2) of size 4 has no selected pixel
        mask[10:15, 15:20] = True                        # nor box (2, 3) of size 5
        sel = ~mask
    origins = [((3 * i + 1) % 4, (5 * i + 2) % 7) for i in range(M + 1)]

    def embed(a, dtype, org):
        full = (rng.uniform(0.0, 255.0, (T, H, W))).astype(dtype)
        full[:, org[0]:org[0] + ROWS, org[1]:org[1] + COLS] = a.astype(dtype)
        return full
    arrays = [embed(members[m], kinds[m], origins[m]) for m in range(M)]
    g = embed(truth, np.uint8, origins[M])
    return arrays, origins[:M], g, origins[M], mask, sel, members, truth


def _close(tag, key, got, want, rel):
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert g.shape == w.shape, (tag, key, g.shape, w.shape)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, key, g, w)
    with np.errstate(invalid="ignore"):
        ok = np.isnan(w) | (np.abs(g - w) <= rel * np.abs(w))
    assert np.all(ok), (tag, key, g, w)


def assert_sums(tag, got, ref):
    figures = []
    for k in PLAIN_KEYS:
        g, w = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        if g.size and g.shape == w.shape:
            figures.append(f"{k} {np.abs(g - w).max():.1e}/{np.abs(w).max():.1e}")
    print(f"{tag}: n {ref['n']} skipped {ref['n_skipped']}  " + " ".join(figures))
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(ref[k], np.int64)), (tag, k, got[k], ref[k])
    for k in PLAIN_KEYS:
        _close(tag, k, got[k], ref[k], 1e-12)


def assert_frames(tag, en, va, ref_en, ref_va):
    with np.errstate(invalid="ignore"):
        print(f"{tag}: d {ref_en[:, 0].tolist()}  ES abs err {np.nanmax(np.abs(en[:, 1:] - ref_en[:, 1:])):.1e} of {np.nanmax(np.abs(ref_en[:, 1:])):.1e}"
              f"  VS abs err {np.abs(va[..., 0] - ref_va[..., 0]).max():.1e} of {np.abs(ref_va[..., 0]).max():.1e}")
    assert np.array_equal(en[:, 0], ref_en[:, 0]) and np.array_equal(va[..., 1], ref_va[..., 1])
    _close(tag, "energy", en[:, 1:], ref_en[:, 1:], 1e-9)
    _close(tag, "variogram", va[..., 0], ref_va[..., 0], 1e-9)


def _ops_sums(dev, arrays, origins, stride, g, gtl, rows, cols, sel, box, xq, edges):
    """The per-point sums of one ops.ens_points launch, merged by ops.prob_merge, and the number of records."""
    from p2igan_bench import ops
    from p2igan_bench.evaluation._common import device_tables
    from p2igan_bench.evaluation.ensemble import _Layout, unpack_record
    M = len(arrays)
    lay = _Layout(M, len(xq), len(edges))
    _, rank = device_tables(dev, True, sel)
    nrec = -(-g.shape[0] * (rows // box) * (cols // box) // ops.ENS_WG_PIXELS)
    part = torch.full((nrec * (lay.nf + lay.ni),), float("nan"), device=dev, dtype=torch.float64)
    ops.ens_points(arrays, origins, stride, g, gtl, rows, cols, box, rank, xq, edges, part)
    acc = torch.zeros(lay.nf + lay.ni, device=dev, dtype=torch.float64)
    ops.prob_merge(part, lay.nf, lay.ni, acc)
    row = acc.cpu().numpy()
    return unpack_record(row[:lay.nf], np.ascontiguousarray(row[lay.nf:]).view(np.int64), lay), nrec


@pytest.mark.parametrize("sel_kind", [None, "radar"])
@pytest.mark.parametrize("kind", ["f32", "f64", "mix"])
@pytest.mark.parametrize("M", MS)
def test_kernels_match_reference(dev, M, kind, sel_kind):
    """A 17 x 23 crop of 20 x 29 inputs, every input at its own origin, truth uint8, at box sizes 1, 4 and 5 (17 = 3 * 5 + 2: the
    remainder is dropped), with and without a radar-mode mask that empties one box of each size; the mixed-dtype cases carry a
    frame without a valid pixel."""
    from p2igan_bench import ops
    from p2igan_bench.evaluation._common import device_tables
    nan_frame = kind == "mix"
    arrays, origins, g, gtl, mask, sel, members, truth = build(M, kind, sel_kind, nan_frame)
    da, dg = [torch.from_numpy(a).to(dev) for a in arrays], torch.from_numpy(g).to(dev)
    xq, edges = _xq(), er.DEFAULT_EDGES
    tag = f"M{M}-{kind}-{sel_kind}"
    for box in BOXES:
        ref = er.ens_sums(members, truth, sel, box, xq, edges)
        assert ref["edge_count"] == 0, f"{tag}: {ref['edge_count']} values within 1e-9 of a decision edge: re-seed the case"
        got, _ = _ops_sums(dev, da, origins, 0, dg, gtl, ROWS, COLS, sel, box, xq, edges)
        assert_sums(f"{tag}-box{box}", got, ref)
        boxes = (ROWS // box) * (COLS // box) - (1 if sel_kind else 0) if box > 1 else (int(sel.sum()) if sel_kind else ROWS * COLS)
        scored_frames = T - 1 if nan_frame else T
        assert ref["n"] + ref["n_skipped"] == T * boxes
        assert ref["n_skipped"] >= (boxes if nan_frame else 0) + 1 and ref["n"] > (scored_frames - 1) * boxes - 8
        if M > 1 and box == 1:
            assert ref["rank"][1:M].sum() > 0          # ties spread weight over inner bins
    _, rank = device_tables(dev, True, sel)
    en = torch.full((T, 4), float("nan"), device=dev, dtype=torch.float64)
    va = torch.full((T, len(er.DEFAULT_OFFSETS), 2), float("nan"), device=dev, dtype=torch.float64)
    ops.ens_energy(da, origins, 0, dg, gtl, ROWS, COLS, rank, en)
    ops.ens_variogram(da, origins, 0, dg, gtl, ROWS, COLS, rank, er.DEFAULT_OFFSETS, va)
    ref_en, ref_va = er.energy_frames(members, truth, sel), er.variogram_frames(members, truth, sel)
    assert_frames(tag, en.cpu().numpy(), va.cpu().numpy(), ref_en, ref_va)
    assert (ref_en[2, 0] == 0) == nan_frame and ref_en[1, 0] < ref_en[0, 0]
    if nan_frame:
        assert np.all(ref_va[2] == 0.0)


@pytest.mark.parametrize("extra", [0, 1])
def test_workgroup_boundaries(dev, extra):
    """A piece of exactly P2I_ENS_WG_PIXELS points (one record) and one of a point more (two, the second with one point)."""
    from p2igan_bench import ops
    n = ops.ENS_WG_PIXELS + extra
    rng = np.random.default_rng(50 + extra)
    members, truth = (a[..., 1:, :, :] for a in _rain(rng, 5, 2, 1, n, [np.float32] * 5))       # the second frame: rain, not the all-zero one
    da = [torch.from_numpy(m.astype(np.float32)).to(dev) for m in members]
    dg = torch.from_numpy(truth.astype(np.uint8)).to(dev)
    ref = er.ens_sums(members, truth, None, 1, _xq(), er.DEFAULT_EDGES)
    assert ref["edge_count"] == 0
    got, nrec = _ops_sums(dev, da, [(0, 0)] * 5, 0, dg, (0, 0), 1, n, None, 1, _xq(), er.DEFAULT_EDGES)
    assert nrec == 1 + extra and ref["n"] == n
    assert_sums(f"{n} points", got, ref)


def _evaluator(dev, mask=None, **kw):
    from p2igan_bench.evaluation import EnsembleEvaluator
    kw.setdefault("box_sizes", BOXES)
    return EnsembleEvaluator((ROWS, COLS), mask=mask, thresholds=THR, device=dev, **kw)


def _bits(ev, name="e"):
    st = ev._methods[name]
    return torch.cat([st["acc"][s] for s in ev.box_sizes] + [t.reshape(-1) for t in st["energy"] + st["variogram"]]).view(torch.int64)


@functools.lru_cache(maxsize=None)
def centred(M, kind, sel_kind):
    """The same fields, every input H x W with the centre crop (the evaluator's rule)."""
    arrays, _, g, _, mask, sel, members, truth = build(M, kind, sel_kind)
    top, left = (H - ROWS) // 2, (W - COLS) // 2
    def centre(a, c):
        out = a.copy()
        out[:, top:top + ROWS, left:left + COLS] = c.astype(a.dtype)
        return out
    return [centre(a, members[m]) for m, a in enumerate(arrays)], centre(g, truth), mask, sel, members, truth


def _reference(members, truth, sel, boxes=BOXES):
    ref = {f"box_{s}": er.ens_sums(members, truth, sel, s, _xq(), er.DEFAULT_EDGES) for s in boxes}
    ref["energy"], ref["variogram"] = er.energy_frames(members, truth, sel), er.variogram_frames(members, truth, sel)
    return ref


def assert_all(tag, got, ref):
    for key in ref:
        if key.startswith("box_"):
            assert_sums(f"{tag}-{key}", got[key], ref[key])
    assert_frames(tag, got["energy"], got["variogram"], ref["energy"], ref["variogram"])


@pytest.mark.parametrize("M,kind", [(3, "mix"), (33, "f32"), (64, "f64")])
def test_evaluator_matches_reference(dev, M, kind):
    arrays, g, mask, sel, members, truth = centred(M, kind, "radar")
    ev = _evaluator(dev, mask)
    ev.update("e", arrays, g)
    assert_all(f"evaluator M{M}", ev.sums("e"), _reference(members, truth, sel))


def test_permuted_members(dev):
    """The per-point record is a function of the member set: bit-identical under a permutation.  The energy and variogram scores
    add the members in another order and hold at their bound."""
    arrays, g, mask, sel, members, truth = centred(33, "mix", "radar")
    perm = np.random.default_rng(5).permutation(33)
    a, b = _evaluator(dev, mask), _evaluator(dev, mask)
    a.update("e", arrays, g)
    b.update("e", [arrays[i] for i in perm], g)
    for s in BOXES:
        assert torch.equal(a.raw("e", s).view(torch.int64), b.raw("e", s).view(torch.int64)), s
    sa, sb = a.sums("e"), b.sums("e")
    assert_frames("permuted", sb["energy"], sb["variogram"], sa["energy"], sa["variogram"])
    assert_all("permuted vs reference", sb, _reference(members, truth, sel))


@pytest.mark.parametrize("M", [1, 5, 64])
def test_strided_form_is_bit_identical(dev, M):
    """One (T, M, H, W) tensor, its members read in place at stride M h w, against M contiguous copies."""
    arrays, g, mask, sel, members, truth = centred(M, "f32", None)
    stack = torch.from_numpy(np.stack(arrays, axis=1)).to(dev)
    assert stack.shape == (T, M, H, W)
    a, b = _evaluator(dev), _evaluator(dev)
    a.update("e", arrays, g)
    b.update("e", stack, g)
    assert torch.equal(_bits(a), _bits(b))
    c = _evaluator(dev)
    c.update("e", np.stack(arrays, axis=1), g)           # the same from the host
    assert torch.equal(_bits(a), _bits(c))
    assert_all(f"strided M{M}", b.sums("e"), _reference(members, truth, sel))


def test_runs_are_bit_identical(dev):
    arrays, g, mask, sel, _, _ = centred(33, "mix", "radar")
    runs = []
    for _ in range(2):
        ev = _evaluator(dev, mask)
        ev.update("e", arrays, g)
        ev.update("e", [a[:2] for a in arrays], g[:2])
        runs.append(_bits(ev))
    assert torch.equal(runs[0], runs[1])


def test_launch_cuts_inside_one_update(dev, monkeypatch):
    """``max_frames`` cuts the three frames into launches of 1 and of 2 (+ 1): the integers are equal, the fp64 sums hold at the
    bounds (the workgroups' boundaries move with the cuts), the per-frame outputs are the same bits, a cut run repeats bit for bit."""
    from p2igan_bench import ops
    arrays, g, mask, sel, members, truth = centred(33, "mix", "radar")
    ref = _reference(members, truth, sel)
    launches, real = [], ops.ens_energy
    monkeypatch.setattr(ops, "ens_energy", lambda *a, **k: (launches.append(a[3].shape[0]), real(*a, **k))[1])

    def run(max_frames):
        ev = _evaluator(dev, mask)
        ev.max_frames = max_frames
        del launches[:]
        ev.update("e", arrays, g)
        return ev, list(launches)
    whole, l0 = run(None)
    assert l0 == [3]
    for max_frames, want in ((1, [1, 1, 1]), (2, [2, 1])):
        cut, l1 = run(max_frames)
        assert l1 == want
        got = cut.sums("e")
        assert_all(f"max_frames {max_frames}", got, ref)
        full = whole.sums("e")
        assert np.array_equal(got["energy"], full["energy"], equal_nan=True) and np.array_equal(got["variogram"], full["variogram"])
        again, _ = run(max_frames)
        assert torch.equal(_bits(cut), _bits(again))


def test_identical_members_crps_is_mae(dev):
    """M copies of one field: CRPS = MAE of that field, the spread is 0, and the MAE is ProbEvaluator's at variance 0."""
    from p2igan_bench.evaluation import ProbEvaluator
    arrays, g, mask, sel, members, truth = centred(1, "f32", "radar")
    field = arrays[0].copy()
    field[~np.isfinite(field)] = np.nan                  # both evaluators skip NaN; an infinite mean is ProbEvaluator's to score
    arrays = [field]
    ev = _evaluator(dev, mask, box_sizes=(1,))
    ev.update("e", [arrays[0]] * 8, g)
    res = ev.compute()["e"]
    b = res["box_1"]
    pe = ProbEvaluator((ROWS, COLS), mask=mask, thresholds=THR, censor=False, device=dev)
    pe.update("p", arrays[0], g, 0.0)
    p = pe.compute()["p"]
    print(f"CRPS {b['CRPS']!r} MAE {b['MAE']!r} fair {b['CRPS_fair']!r}  ProbEvaluator MAE {p['MAE']!r} n {p['n']}")
    assert b["CRPS"] == b["MAE"] == b["CRPS_fair"] and b["mean_var"] == 0.0 and b["n"] == p["n"] and b["n_skipped"] == p["n_skipped"]
    assert abs(b["MAE"] - p["MAE"]) <= 1e-12 * p["MAE"] and abs(b["RMSE"] - p["RMSE"]) <= 1e-12 * p["RMSE"]
    en = np.asarray(res["energy"]["frames"]["ES"])
    dist = np.asarray(res["energy"]["frames"]["dist_truth"])
    assert np.array_equal(en, dist) and np.array_equal(np.asarray(res["energy"]["frames"]["ES_fair"]), dist)    # pair distances are exactly 0


def assert_scores(got, want, path=""):
    """Derived scores: the same keys, integers exact, floats within 1e-9 relative (ratios of the bounded sums), NaN where the
    reference has NaN."""
    if isinstance(want, dict):
        assert set(want) <= set(got), (path, sorted(got), sorted(want))
        for k in want:
            assert_scores(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), path
        for i, (a, b) in enumerate(zip(got, want)):
            assert_scores(a, b, f"{path}[{i}]")
    elif isinstance(want, (int, np.integer)) and not isinstance(want, bool):
        assert got == want, (path, got, want)
    elif np.isnan(want):
        assert np.isnan(got), (path, got)
    else:
        assert abs(got - want) <= 1e-9 * abs(want) + 1e-300, (path, got, want)


def _ref_scores(members, truth, sel, boxes, thresholds=THR, offsets=er.DEFAULT_OFFSETS):
    from p2igan_bench.evaluation import pixel_threshold
    xq = tuple(pixel_threshold(q, True) for q in thresholds)
    want = {f"box_{s}": er.ens_scores(er.ens_sums(members, truth, sel, s, xq, er.DEFAULT_EDGES), members.shape[0], thresholds) for s in boxes}
    want["energy"] = er.energy_scores(er.energy_frames(members, truth, sel))
    want["variogram"] = er.variogram_scores(er.variogram_frames(members, truth, sel, offsets), offsets)
    return want


@pytest.mark.parametrize("M", [1, 33])
def test_scores_match_reference(dev, M):
    from p2igan_bench.evaluation import run_ensemble
    arrays, g, mask, sel, members, truth = centred(M, "f64", "radar")
    got = run_ensemble({"e": arrays}, g, mask, "radar", (ROWS, COLS), box_sizes=BOXES, thresholds=THR, device=dev)["e"]
    assert_scores(got, _ref_scores(members, truth, sel, BOXES))
    if M == 1:
        assert all(np.isnan(got["box_1"][k]) for k in ("CRPS_fair", "mean_var", "spread_skill_ratio")) and np.isnan(got["energy"]["ES_fair_norm"])
        assert got["box_1"]["CRPS"] == got["box_1"]["MAE"]


def test_event_dicts_and_refusals(dev):
    from p2igan_bench.evaluation import EnsembleEvaluator, run_ensemble
    arrays, g, mask, sel, members, truth = centred(3, "f32", None)
    kw = dict(crop_size=(ROWS, COLS), box_sizes=(1, 4), thresholds=THR, device=dev)
    one = run_ensemble({"e": arrays}, g, **kw)["e"]
    two = run_ensemble({"e": {"a": [a[:1] for a in arrays], "b": [a[1:] for a in arrays], "c": None}}, {"a": g[:1], "b": g[1:], "c": g, "d": None}, **kw)["e"]
    assert two["box_1"]["n"] == one["box_1"]["n"] and two["box_4"]["rank_histogram"] == one["box_4"]["rank_histogram"]
    assert_scores(two, {k: {kk: vv for kk, vv in v.items() if kk != "frames"} for k, v in one.items()})
    with pytest.raises(TypeError):
        run_ensemble({"e": arrays}, {"a": g}, **kw)
    with pytest.raises(TypeError):
        run_ensemble({"e": {"a": arrays}}, g, **kw)
    with pytest.raises(ValueError, match="box_sizes"):
        EnsembleEvaluator((ROWS, COLS), box_sizes=(1, 18), device=dev)
    with pytest.raises(ValueError, match="offsets"):
        EnsembleEvaluator((ROWS, COLS), offsets=[(0, 1)] * 17, device=dev)
    ev = EnsembleEvaluator((ROWS, COLS), device=dev, box_sizes=(1,))
    ev.update("e", arrays, g)
    with pytest.raises(ValueError, match="had 3 members"):
        ev.update("e", arrays[:2], g)
    with pytest.raises(ValueError, match="1 to 64 members"):
        ev.update("f", [arrays[0]] * 65, g)
    with pytest.raises(ValueError, match="exceeds input"):
        ev.update("f", [a[:, :16] for a in arrays], g)


def test_kriging_ensemble_end_to_end(dev, tmp_path):
    """KrigingGenerator.forward_ensemble on a 16 x 16, 4-frame synthetic event with 24 gauges, M = 8, through run_ensemble and
    write_ens_outputs; the kriging mean rides along as a one-member ensemble."""
    from p2igan_bench.evaluation import run_ensemble, write_ens_outputs
    from p2igan_bench.models import build_generator
    h = w = 16
    rng = np.random.default_rng(77)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    field = np.stack([0.5 + 0.3 * np.sin(0.37 * yy + 0.2 * i) * np.cos(0.29 * xx - 0.3 * i) + 0.15 * rng.random((h, w)) for i in range(4)])
    field = field.astype(np.float32)
    masks = np.zeros((1, 4, 1, h, w), np.float32)
    masks.reshape(4, -1)[:, rng.permutation(h * w)[:24]] = 1.0
    frames = torch.from_numpy(field.reshape(1, 4, 1, h, w))
    G = build_generator({"model": {"name": "kriging", "variogram": {"model": "exponential", "fit": False, "nugget": 0.002, "psill": 0.03,
                                                                     "range": 4.0}, "share_sets": True, "ensemble": {"embed": 2}}}).to(dev)
    m = torch.from_numpy(masks).to(dev)
    pred, ens = G.forward_ensemble((frames * torch.from_numpy(masks)).to(dev), m, 8, seed=11)
    assert ens.shape == (1, 4, 8, h, w)
    members, mean, truth = ens[0] * 255.0, pred[0] * 255.0, (frames[0, :, 0] * 255.0).to(dev)
    gauges = masks[0, 0, 0] != 0
    kw = dict(crop_size=16, thresholds=(0.5, 2.0), device=dev)
    res = run_ensemble({"ens": members, "mean": mean}, truth, gauges, "radar", **kw)
    write_ens_outputs(str(tmp_path / "out"), res)
    for f in ("metrics.json", "metrics.txt", "ens_data.npz"):
        assert (tmp_path / "out" / f).is_file(), f
    try:
        import matplotlib  # noqa: F401
        assert (tmp_path / "out" / "ens_panels.pdf").is_file()
    except ImportError:
        pass
    got = json.loads((tmp_path / "out" / "metrics.json").read_text())
    hm, hx, hy = members.cpu().numpy().astype(np.float64).transpose(1, 0, 2, 3), mean.cpu().numpy().astype(np.float64).transpose(1, 0, 2, 3), \
        truth.cpu().numpy().astype(np.float64)
    assert_scores(got["ens"], _ref_scores(hm, hy, ~gauges, (1, 4, 16), (0.5, 2.0)))
    assert_scores(got["mean"], _ref_scores(hx, hy, ~gauges, (1, 4, 16), (0.5, 2.0)))
    data = np.load(tmp_path / "out" / "ens_data.npz")
    assert data["ens/box_1/rank_histogram"].shape == (9,) and data["mean/box_16/rank_histogram"].shape == (2,)
    for name in ("ens", "mean"):
        print(f"{name}: CRPS {got[name]['box_1']['CRPS']:.4f} fair {got[name]['box_1']['CRPS_fair']:.4f} box4 {got[name]['box_4']['CRPS']:.4f} "
              f"box16 {got[name]['box_16']['CRPS']:.4f} ES {got[name]['energy']['ES_norm']:.4f} VS {got[name]['variogram']['VS']:.4f} "
              f"SSR {got[name]['box_1']['spread_skill_ratio']:.3f} outliers {got[name]['box_1']['outlier_share']:.3f}")
    # at the gauges every member equals the truth: CRPS exactly 0 and the tie rule's shares in every bin
    at = run_ensemble({"ens": members}, truth, gauges, "gauge", box_sizes=(1,), **kw)["ens"]["box_1"]
    assert at["n"] == 4 * 24 and at["CRPS"] == 0.0 and at["CRPS_fair"] == 0.0 and at["MAE"] == 0.0
    q, r = divmod(1 << 32, 9)
    assert at["rank_histogram"] == [(q + r) / (1 << 32)] + [q / (1 << 32)] * 8
    en = run_ensemble({"ens": members}, truth, gauges, "gauge", box_sizes=(1,), **kw)["ens"]["energy"]
    assert en["frames"]["ES"] == [0.0] * 4 and en["frames"]["d"] == [24] * 4


def test_evaluate_cli(dev, tmp_path):
    """scripts/infer.py --ensemble-output on a synthetic store, then scripts/evaluate.py --ens: the files exist, a second run gives
    the same arrays, the other outputs do not change, and --ensemble without --ens is an argument error."""
    from conftest import PKG
    from p2igan_bench.data import synth_store
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    try:
        import evaluate
        import infer
    finally:
        sys.path.pop(0)
    store = tmp_path / "test.zarr"
    synth_store.write_test_zarr(str(store), n_events=2, frames_per_event=20, h=32, w=32)
    cfg = json.load(open(os.path.join(PKG, "p2igan_bench", "config", "kriging_ensemble.json")))
    cfg["data"]["test"].update(w=32, h=32, data_root=str(store))
    cfg["data"]["test"]["mask"]["block_sizes"] = [4]
    json.dump(cfg, open(tmp_path / "cfg.json", "w"))
    infer.main(["--config", str(tmp_path / "cfg.json"), "--output", str(tmp_path / "krig.zarr"), "--ensemble-output", str(tmp_path / "members"),
                "--members", "3", "--ensemble-seed", "5"])
    np.savetxt(tmp_path / "mask.txt", (np.arange(32 * 32).reshape(32, 32) % 11 == 0).astype(np.float64))
    base = ["--truth", str(store), "--method", f"krig={tmp_path / 'krig.zarr'}", "--mask", str(tmp_path / "mask.txt"), "--crop-size", "24",
            "--thresholds", "0.5", "2"]
    evaluate.main(base + ["--output", str(tmp_path / "plain")])
    runs = []
    for tag in ("a", "b"):
        evaluate.main(base + ["--output", str(tmp_path / f"with_{tag}"), "--ens", str(tmp_path / f"ens_{tag}"), "--ensemble",
                              f"cs={tmp_path / 'members'}", "--box-sizes", "1", "4"])
        for f in ("metrics.json", "metrics.txt", "ens_data.npz"):
            assert (tmp_path / f"ens_{tag}" / f).is_file(), f
        runs.append(dict(np.load(tmp_path / f"ens_{tag}" / "ens_data.npz")))
    assert sorted(runs[0]) == sorted(runs[1]) and all(np.array_equal(runs[0][k], runs[1][k], equal_nan=True) for k in runs[0] if k != "ensembles")
    assert (tmp_path / "ens_a" / "metrics.json").read_bytes() == (tmp_path / "ens_b" / "metrics.json").read_bytes()
    for f in ("metrics.json", "metrics.txt"):
        assert (tmp_path / "with_a" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    got = json.loads((tmp_path / "ens_a" / "metrics.json").read_text())["cs"]
    assert sorted(got) == ["box_1", "box_4", "energy", "variogram"] and got["box_1"]["M"] == 3
    assert got["box_1"]["n"] == 40 * int((np.arange(32 * 32).reshape(32, 32) % 11 != 0)[4:28, 4:28].sum()) and got["energy"]["n_frames"] == 40
    assert len(got["box_1"]["rank_histogram"]) == 4 and abs(sum(got["box_1"]["rank_histogram"]) - 1.0) < 1e-12
    with pytest.raises(SystemExit):
        evaluate.main(base + ["--output", str(tmp_path / "o2"), "--ensemble", f"cs={tmp_path / 'members'}"])
    assert not (tmp_path / "o2").exists()
