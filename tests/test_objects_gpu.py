"""Object-based verification on the MI355X against the restatement (tests/objects_ref.py): every integer the device returns (frame
records, level records, offsets, object tables) bit for bit over crop sizes, connectivities, frame counts, dtype pairs, off-centre
crops and both labelling paths; the mask patterns that stress a labelling; NaN and dry frames; streaming and path independence;
scripts/evaluate.py --objects end to end.  The derived scores are float64 numpy on both sides from equal integers: they may differ
by the rounding of sums of at most a few thousand terms of order 1, 4096 * 2^-53 ~ 5e-13, and are held to 1e-10."""
import itertools
import json
import math
import os
import sys

import numpy as np
import pytest

import objects_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTS = ("rec", "lev", "offsets", "table")


def evaluator(S, connectivity=8, thresholds=ref.CASE_THRESHOLDS, workspace=None, **kw):
    from p2igan_bench.evaluation import ObjectEvaluator
    ev = ObjectEvaluator(S, thresholds, connectivity, **kw)
    if workspace is not None:
        assert workspace or not ev.use_workspace
        ev.use_workspace = workspace
    return ev


def paths(S):
    return (False, True) if S <= 128 else (True,)


def assert_ints_equal(got, want, what):
    for k in INTS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)


def assert_close(a, b, path=()):
    if isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            assert_close(a[k], b[k], path + (k,))
    elif isinstance(a, float) and math.isnan(a):
        assert isinstance(b, float) and math.isnan(b), path
    elif isinstance(a, float):
        assert abs(a - b) <= 1e-10, (path, a, b)
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("T", ref.CASE_FRAMES)
@pytest.mark.parametrize("S", ref.CASE_SIZES)
def test_integers_bit_for_bit(S, T):
    pred, truth = ref.exact_inputs(S, T)
    p_in = {dt: ref.as_dtype(pred, dt) for dt in ref.DTYPES}
    g_in = {dt: ref.as_dtype(truth, dt) for dt in ref.DTYPES}
    assert p_in[np.uint8].shape[1:] == (S + 17, S + 13) and g_in[np.uint8].shape[1:] == (S + 7, S + 27)      # odd, different crop origins
    # all nine pairs on the small crops; three that hold every dtype on either side on the large ones
    pairs = list(itertools.product(ref.DTYPES, ref.DTYPES)) if S <= 33 else [(np.float32, np.uint8), (np.uint8, np.float64),
                                                                              (np.float64, np.float32)]
    for conn in (4, 8):
        evs = [evaluator(S, conn, workspace=w) for w in paths(S)]
        for pd, gd in pairs:
            name = f"{np.dtype(pd).name}/{np.dtype(gd).name}"
            want = ref.records(p_in[pd], g_in[gd], S, ref.CASE_THRESHOLDS, conn)
            for ev in evs:
                ev.update(name, p_in[pd], g_in[gd])
                assert_ints_equal(ev.records(name), want, (name, conn, ev.use_workspace))
        # the whole restatement on one pair, through the public result
        frames, ref_frames = {}, {}
        got = evs[0].compute(frames)["float32/uint8"]
        want = ref.run_objects({"m": p_in[np.float32]}, g_in[np.uint8], S, ref.CASE_THRESHOLDS, conn, frames_out=ref_frames)["m"]
        assert_close(want, got)
        for k in ("S", "A", "L", "L1", "L2"):
            assert np.allclose(frames["float32/uint8"][k], ref_frames["m"][k], rtol=0, atol=1e-10, equal_nan=True), k
        assert frames["float32/uint8"]["frame"].tolist() == list(range(T))


@pytest.mark.parametrize("conn", [4, 8])
def test_patterns_on_both_paths(conn):
    """S = 128 is the LDS path's largest crop and 2 x 2 tiles of the workspace path; the canvases are larger than the crop, so the
    full frame, the checkerboard, the serpentines, the spiral and the combs continue outside and are cut at the crop edge."""
    S = 128
    pred, truth, names = ref.pattern_events(S)
    assert pred.shape[1:] == (S + 6, S + 10)
    want = ref.records(pred, truth, S, ref.PATTERN_THRESHOLDS, conn)
    got = None
    for w in paths(S):
        ev = evaluator(S, conn, ref.PATTERN_THRESHOLDS, workspace=w)
        ev.update("m", pred, truth)
        got = ev.records("m")
        assert_ints_equal(got, want, (conn, w))
    at = {n: i for i, n in enumerate(names)}
    lev = got["lev"][:, 1, 0]                 # the truth at 0.5 mm/h: the whole pattern
    assert lev[at["empty"], :2].tolist() == [0, 0]
    assert lev[at["full"], :2].tolist() == [1, S * S]
    assert lev[at["checkerboard"], :2].tolist() == ([1, S * S // 2] if conn == 8 else [S * S // 2, S * S // 2])
    for n in ("serpentine", "serpentine_t", "spiral"):
        assert lev[at[n], 0] == 1 and lev[at[n], 1] > S * S // 3, n
    assert got["lev"][at["diagonals"], 1, 0, 0] == want["lev"][at["diagonals"], 1, 0, 0] > 1
    # the prediction is the truth's next frame: the same objects one frame earlier
    assert np.array_equal(got["lev"][:-1, 0], got["lev"][1:, 1])


def test_paths_pieces_and_reruns_agree():
    S, T = 128, 5
    pred, truth = ref.exact_inputs(S, T)
    p, g = pred.astype(np.float32), ref.as_dtype(truth, np.uint8)

    def run(cuts, workspace):
        ev = evaluator(S, 8, workspace=workspace)
        for a, b in zip(cuts, cuts[1:]):
            ev.update("m", p[a:b], g[a:b], origin=(0, a))
        return ev.records("m"), json.dumps(ev.compute(), sort_keys=True)
    one, again, big, pieces = run((0, T), False), run((0, T), False), run((0, T), True), run((0, 1, 3, T), True)
    for other in (again, big, pieces):
        assert_ints_equal(other[0], one[0], "paths / pieces / reruns")
        assert other[0]["frame"].tolist() == list(range(T)) and other[1] == one[1]
    ev = evaluator(S)
    ev.update("m", p, g)
    ev.reset()
    assert ev.compute() == {}


@pytest.mark.parametrize("workspace", [False, True])
def test_launch_cuts_inside_one_update_agree(monkeypatch, workspace):
    """``max_frames`` cuts the five frames of one update into launches of 1 and of 2 frames (2 + 2 + 1), on both labelling paths.
    Frames are labelled and scored on their own, so the integers, the frames' positions and the result do not depend on the cuts;
    a launch's frames follow on the piece's ``origin``."""
    from p2igan_bench import ops
    S, T = 33, 5
    pred, truth = ref.exact_inputs(S, T)
    p, g = pred.astype(np.float32), ref.as_dtype(truth, np.uint8)
    launches, real = [], ops.objects_label
    monkeypatch.setattr(ops, "objects_label", lambda *a, **k: (launches.append(a[1]), real(*a, **k))[1])

    def run(max_frames, **kw):
        ev = evaluator(S, 8, workspace=workspace)
        ev.max_frames = max_frames
        del launches[:]
        ev.update("m", p, g, **kw)
        return ev.records("m"), json.dumps(ev.compute(), sort_keys=True), list(launches)
    whole = run(None)
    assert whole[2] == [T] and whole[0]["frame"].tolist() == list(range(T)) and whole[0]["event"].tolist() == [0] * T
    for max_frames, want in ((1, [1] * 5), (2, [2, 2, 1])):
        rec, res, n = run(max_frames)
        assert n == want
        assert_ints_equal(rec, whole[0], ("cuts", max_frames, workspace))
        assert rec["frame"].tolist() == list(range(T)) and rec["event"].tolist() == [0] * T
        assert res == whole[1], max_frames
    rec, _, n = run(2, origin=(2, 7))
    assert n == [2, 2, 1] and rec["frame"].tolist() == list(range(7, 7 + T)) and rec["event"].tolist() == [2] * T
    assert_ints_equal(rec, whole[0], ("cuts at an origin", workspace))


@pytest.mark.parametrize("conn", [4, 8])
def test_large_crop_through_the_workspace_path(conn):
    """S = 160: 3 x 3 tiles with a ragged last row and column; patterns that straddle every border and corner, and a float field."""
    S = 160
    pred, truth, names = ref.pattern_events(S)
    ev = evaluator(S, conn, ref.PATTERN_THRESHOLDS)
    assert ev.use_workspace
    keep = [names.index(n) for n in ("straddlers", "spiral", "serpentine_t", "nested_u", "comb_up", "checkerboard", "random_0.59")]
    ev.update("patterns", pred[keep], truth[keep])
    assert_ints_equal(ev.records("patterns"), ref.records(pred[keep], truth[keep], S, ref.PATTERN_THRESHOLDS, conn), "patterns")
    fp, fg = ref.exact_inputs(S, 1)
    ev2 = evaluator(S, conn)
    ev2.update("field", fp, ref.as_dtype(fg, np.uint8))
    assert_ints_equal(ev2.records("field"), ref.records(fp, ref.as_dtype(fg, np.uint8), S, ref.CASE_THRESHOLDS, conn), "field")


def test_nan_frame_is_skipped_and_counted():
    S, T = 33, 5
    pred, truth = ref.exact_inputs(S, T)
    p, g = pred.astype(np.float32), truth.copy()
    top, left = (p.shape[1] - S) // 2, (p.shape[2] - S) // 2
    p[2, top + 3, left + 5] = np.nan            # inside the crop: frame 2 is left out
    p[4, 0, 0] = np.nan                         # outside the crop: frame 4 stays
    g[0, (g.shape[1] - S) // 2, (g.shape[2] - S) // 2] = np.nan     # a NaN of the truth counts as well
    from p2igan_bench.evaluation import run_objects
    for w in paths(S):
        ev = evaluator(S, workspace=w)
        ev.update("m", p, g)
        assert_ints_equal(ev.records("m"), ref.records(p, g, S, ref.CASE_THRESHOLDS), w)
    got = run_objects({"m": p}, g, S, ref.CASE_THRESHOLDS)["m"]
    want = ref.run_objects({"m": p}, g, S, ref.CASE_THRESHOLDS)["m"]
    assert got["frames"] == 5 and got["frames_skipped"] == want["frames_skipped"] == 2
    assert_close(want, got)
    assert sum(got["levels"]["rel"][k] for k in ("frames_scored", "frames_pred_only", "frames_truth_only", "frames_no_object")) == 3


def test_dry_truth_against_wet_prediction():
    from p2igan_bench.evaluation import run_objects
    S = 16
    dry = np.zeros((3, S + 3, S + 1), np.uint8)
    wet = np.zeros((3, S, S), np.float32)
    wet[:, 3:6, 3:9] = 180.0
    wet[2] = 0.0
    got = run_objects({"m": wet}, dry, S, (0.5,))["m"]
    assert_close(ref.run_objects({"m": wet}, dry, S, (0.5,))["m"], got)
    for key in ("thr_0.5", "rel"):
        m = got["levels"][key]
        assert (m["frames_scored"], m["frames_pred_only"], m["frames_truth_only"], m["frames_no_object"]) == (0, 2, 0, 1)
        assert m["pred"]["objects_max"] == 1 and m["truth"]["objects_max"] == 0 and math.isnan(m["S_mean"])
    # without the floor the dry truth is one object of the whole crop and every frame is scored
    got = run_objects({"m": wet}, dry, S, (0.5,), sal_floor=0.0)["m"]["levels"]["rel"]
    assert got["frames_scored"] == 3 and got["truth"]["area_mean"] == S * S


def test_what_the_scores_say():
    """The truth against itself scores zero; a smoothed field has larger objects, fewer of them at a fixed
    threshold, and a positive structure error."""
    from p2igan_bench.evaluation import run_objects
    S, T = 64, 5
    _, truth = ref.exact_inputs(S, T)
    g = ref.as_dtype(truth, np.uint8)
    smooth = ref.smoother(ref.smoother(ref.smoother(truth)))
    res = run_objects({"same": g, "smooth": smooth}, g, S, ref.CASE_THRESHOLDS)
    for m in res["same"]["levels"].values():
        assert m["frames_scored"] == T and all(m[f"{k}_{s}"] == 0.0 for k in ("S", "A", "L", "L1", "L2") for s in ("mean", "median"))
    rel = res["smooth"]["levels"]["rel"]
    assert rel["S_median"] > 0.0 and rel["pred"]["area_mean"] > rel["truth"]["area_mean"]
    low = res["smooth"]["levels"]["thr_0.5"]
    assert low["pred"]["objects_mean"] < low["truth"]["objects_mean"]
    assert rel["pred"]["single_pixel_share"] < rel["truth"]["single_pixel_share"]


def test_guards_on_the_device():
    from p2igan_bench.evaluation import run_objects
    with pytest.raises(ValueError, match="exceeds"):
        run_objects({"m": np.zeros((1, 8, 8), np.uint8)}, np.zeros((1, 8, 8), np.uint8), 16)
    with pytest.raises(TypeError, match="per-event"):
        run_objects({"m": {"e": np.zeros((1, 8, 8), np.uint8)}}, np.zeros((1, 8, 8), np.uint8), 8)


def test_cli_end_to_end(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts"))
    try:
        import evaluate
    finally:
        sys.path.pop(0)
    from p2igan_bench.data import zarr_lite
    from p2igan_bench.evaluation import run_objects
    S, H, W = 32, 37, 40
    truth = {f"event_{i + 1:02d}": ref.as_dtype(ref.smoother(ref.field(300 + i, 3 + i, H, W)), np.uint8)[:, None] for i in range(2)}
    preds = {"same": {k: v.copy() for k, v in truth.items()},
             "smooth": {k: ref.smoother(ref.smoother(v[:, 0].astype(np.float64))).astype(np.float32)[:, None] for k, v in truth.items()}}
    for path, events in [("truth", truth)] + [(m, e) for m, e in preds.items()]:
        grp = zarr_lite.Group(str(tmp_path / f"{path}.zarr"), "w")
        for k, v in events.items():
            grp.create_dataset(k, v)
    np.savetxt(tmp_path / "mask.txt", (np.arange(H * W).reshape(H, W) % 7 == 0).astype(np.float64))
    base = ["--truth", str(tmp_path / "truth.zarr"), "--method", f"same={tmp_path / 'same.zarr'}", "--method",
            f"smooth={tmp_path / 'smooth.zarr'}", "--mask", str(tmp_path / "mask.txt"), "--crop-size", str(S), "--thresholds", "0.5", "2"]
    plain, with_objects, odir = tmp_path / "plain", tmp_path / "exp1", tmp_path / "objects"
    evaluate.main(base + ["--output", str(plain)])
    evaluate.main(base + ["--output", str(with_objects), "--objects", str(odir), "--connectivity", "4", "--sal-factor", "0.1"])
    for f in ("metrics.json", "metrics.txt"):
        assert (plain / f).read_bytes() == (with_objects / f).read_bytes(), f           # exp1's outputs do not depend on --objects
    files = ["metrics.json", "metrics.txt", "objects_data.npz"]
    try:
        import matplotlib  # noqa: F401
        files.append("objects_panels.pdf")
    except ImportError:
        pass
    for f in files:
        assert (odir / f).stat().st_size > 0, f
    want = run_objects(preds, truth, S, thresholds=(0.5, 2.0), connectivity=4, sal_factor=0.1)
    assert list(want) == ["same", "smooth"] and want["same"]["frames"] == 7 and want["same"]["connectivity"] == 4
    assert (odir / "metrics.json").read_text() == json.dumps(want, indent=2, sort_keys=True)
    lines = (odir / "metrics.txt").read_text().splitlines()
    assert lines[0] == "SAL_same_thr0.5: S=0.000000 A=0.000000 L=0.000000" and any(ln.startswith("OBJ_smooth_rel: pred=") for ln in lines)
    data = np.load(odir / "objects_data.npz")
    assert data["smooth/S"].shape == (7, 3) and data["smooth/event"].tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert data["smooth/frame"].tolist() == [0, 1, 2, 0, 1, 2, 3]
