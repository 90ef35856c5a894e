"""Scale-aware verification on the MI355X against the float64 numpy restatement (tests/scale_ref.py): the FSS sums bit for bit over
crop sizes, window sizes, frame counts, dtype pairs and off-centre crops; the radial spectra within the rounding of a direct S^2-term
sum; what the scores mean; streaming and path independence; scripts/evaluate.py --scale end to end."""
import functools
import itertools
import json
import math
import os
import sys

import numpy as np
import pytest

import scale_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0.5, 2.0, 4.0, 8.0)
DTYPES = (np.uint8, np.float32, np.float64)


def window_sizes(S):
    return tuple(sorted({n for n in (1, 2, 3, S - 1, S, S + 1, 2 * S + 1) if n >= 1}))


@functools.lru_cache(maxsize=None)
def inputs(S, T):
    """(pred, truth) on the 0-255 scale as float64, larger than the crop and of different sizes, so the two crop origins differ
    (40 x 36 and 31 x 50 at S = 24); the prediction is the smoother method of another draw mixed with the truth."""
    truth = scale_ref.field(1000 + 10 * S + T, T, S + 7, S + 26)
    own = scale_ref.field(2000 + 10 * S + T, T, S + 16, S + 12)
    tc = scale_ref.crop(truth, S)
    pred = own.copy()
    top, left = (own.shape[1] - S) // 2, (own.shape[2] - S) // 2
    pred[:, top:top + S, left:left + S] = 0.5 * tc + 0.5 * scale_ref.smoother(scale_ref.crop(own, S))
    return pred, truth


def evaluator(S, scales, thresholds=THRESHOLDS):
    from p2igan_bench.evaluation import ScaleEvaluator
    return ScaleEvaluator(S, thresholds, scales)


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("S", [1, 7, 8, 24, 27, 33, 64, 128])
def test_fss_sums_bit_for_bit(S, T):
    pred, truth = inputs(S, T)
    scales = window_sizes(S)
    ev = evaluator(S, scales)
    p_in = {dt: scale_ref.as_dtype(pred, dt) for dt in DTYPES}
    g_in = {dt: scale_ref.as_dtype(truth, dt) for dt in DTYPES}
    for x in list(p_in.values())[1:] + list(g_in.values())[1:]:
        # float inputs stay clear of the thresholds (the device's pow against numpy's); uint8 goes through the host's table
        assert scale_ref.threshold_margin(x, THRESHOLDS) > 1e-9
    # the window counts of each input once, the nine pairs from them
    def counts(x):
        mm = scale_ref.transform(scale_ref.crop(x, S))
        return {(q, n): scale_ref.window_counts(mm >= q, n) for q in THRESHOLDS for n in scales}, [int((mm >= q).sum()) for q in THRESHOLDS]
    cp = {dt: counts(x)[0] for dt, x in p_in.items()}
    cg = {dt: counts(x) for dt, x in g_in.items()}
    for pd, gd in itertools.product(DTYPES, DTYPES):
        name = f"{np.dtype(pd).name}/{np.dtype(gd).name}"
        ev.update(name, p_in[pd], g_in[gd])
        want = [[v for n in scales for v in (int((cp[pd][q, n] ** 2).sum()), int((cg[gd][0][q, n] ** 2).sum()),
                                             int((cp[pd][q, n] * cg[gd][0][q, n]).sum()))] + [cg[gd][1][j]]
                for j, q in enumerate(THRESHOLDS)]
        assert ev.sums(name).tolist() == want, name
    # and the whole restatement on one pair, through the public result
    got = ev.compute()["float32/uint8"]
    ref = scale_ref.run_scale({"m": p_in[np.float32]}, g_in[np.uint8], S, THRESHOLDS, scales)["m"]
    for k in ("FSS", "useful_scale", "frames", "frames_skipped", "wavelength_px"):
        assert json.dumps(got[k], sort_keys=True) == json.dumps(ref[k], sort_keys=True), k        # NaN compares as text


def check_spectra(got, ref, S):
    for k in ("spectrum", "truth_spectrum"):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape == (S // 2 + 1,)
        err = np.abs(g - r) / r[0]
        print(f"S={S} {k}: max |P - P_ref| / P_ref(0) = {err.max():.3e}")
        assert np.all(err <= 1e-10), (k, err.max())
        assert r.min() >= 1e-6 * r[0]           # with the per-bin tolerance: each log10 P within 1e-4 * 10 / ln 10 dB < 1e-3 dB
    if S == 1:
        assert math.isnan(got["LSD"]) and math.isnan(ref["LSD"]) and math.isnan(got["HF_ratio"])
    else:
        print(f"S={S} LSD {got['LSD']:.6f} dB (ref {ref['LSD']:.6f}), HF_ratio {got['HF_ratio']:.6f} (ref {ref['HF_ratio']:.6f})")
        assert abs(got["LSD"] - ref["LSD"]) <= 1e-3
        if not math.isnan(ref["HF_ratio"]):
            assert abs(got["HF_ratio"] - ref["HF_ratio"]) <= 1e-6 * abs(ref["HF_ratio"])


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("S", [1, 7, 8, 12, 27, 64, 128])
def test_spectra_match_fft2(S, T):
    pred, truth = inputs(S, T)
    p, g = scale_ref.as_dtype(pred, np.float32), scale_ref.as_dtype(truth, np.uint8)
    from p2igan_bench.evaluation import run_scale
    got = run_scale({"a": p, "b": pred}, g, S, scales=(1, 3))
    ref = scale_ref.run_scale({"a": p, "b": pred}, g, S, scales=(1, 3))
    for m in ("a", "b"):
        assert got[m]["frames"] == T and got[m]["frames_skipped"] == 0
        check_spectra(got[m], ref[m], S)


def test_nan_frame_is_skipped_and_counted():
    S, T = 27, 5
    pred, truth = inputs(S, T)
    p = pred.astype(np.float32)
    top, left = (p.shape[1] - S) // 2, (p.shape[2] - S) // 2
    p[2, top + 3, left + 5] = np.nan            # inside the crop: frame 2 leaves both spectra
    p[4, 0, 0] = np.nan                         # outside the crop: frame 4 stays
    g = truth.copy()
    g[0, (g.shape[1] - S) // 2, (g.shape[2] - S) // 2] = np.nan     # a NaN of the truth counts as well
    from p2igan_bench.evaluation import run_scale
    got = run_scale({"m": p}, g, S, scales=(1, 3, 5))["m"]
    ref = scale_ref.run_scale({"m": p}, g, S, scales=(1, 3, 5))["m"]
    assert got["frames"] == 5 and got["frames_skipped"] == ref["frames_skipped"] == 2
    check_spectra(got, ref, S)
    assert json.dumps(got["FSS"], sort_keys=True) == json.dumps(ref["FSS"], sort_keys=True)        # NaN compares false there
    allnan = run_scale({"m": np.full((2, S, S), np.nan, np.float32)}, g[:2], S, scales=(1,))["m"]
    assert allnan["frames_skipped"] == 2 and all(math.isnan(v) for v in allnan["spectrum"]) and math.isnan(allnan["LSD"])


def test_scores_mean_what_they_say():
    from p2igan_bench.evaluation import run_scale
    S, T = 64, 3
    g = scale_ref.field(77, T, S, S)
    scales = (1, 3, 5, 9, 17, 33)
    res = run_scale({"smooth": scale_ref.smoother(g), "shift": np.roll(g, 2, axis=2), "same": g}, g, S, scales=scales)
    assert res["smooth"]["HF_ratio"] < 1.0 and abs(res["same"]["HF_ratio"] - 1.0) < 1e-12 and res["same"]["LSD"] < 1e-9
    assert res["smooth"]["LSD"] > res["same"]["LSD"]
    by_n = [res["shift"]["FSS"]["thr_2"][f"n_{n}"] for n in scales]
    assert all(a < b for a, b in zip(by_n, by_n[1:])), by_n
    assert all(v == 1.0 for v in res["same"]["FSS"]["thr_2"].values()) and res["same"]["useful_scale"]["thr_2"] == 1
    us = res["shift"]["useful_scale"]["thr_2"]
    assert us is not None and us > 1 and res["shift"]["FSS"]["thr_2"][f"n_{us}"] >= 0.5


def test_streaming_and_reruns_are_bit_identical():
    S, T = 27, 6
    pred, truth = inputs(S, T)
    p, g = pred.astype(np.float32), scale_ref.as_dtype(truth, np.uint8)
    scales = (1, 2, 5, 27, 55)

    def run(cuts):
        ev = evaluator(S, scales, (0.5, 2.0))
        for a, b in zip(cuts, cuts[1:]):
            ev.update("m", p[a:b], g[a:b])
        return ev.compute(), ev.sums("m").tolist()
    one, again, pieces = run((0, T)), run((0, T)), run((0, 1, 3, T))
    assert json.dumps(one) == json.dumps(again) and one[1] == again[1]
    assert json.dumps(one) == json.dumps(pieces) and one[0]["m"]["frames"] == T
    ev = evaluator(S, scales, (0.5, 2.0))
    ev.update("m", p, g)
    ev.reset()
    assert ev.compute() == {}


@pytest.mark.parametrize("workspace", [False, True])
def test_launch_cuts_inside_one_update_are_bit_identical(monkeypatch, workspace):
    """``max_frames`` cuts the six frames of one update into launches of 1, 2 and 4 frames (4 + 2); with ``use_workspace`` the
    large-crop path's table workspace is cut as well.  The sums are integers and the spectra are folded per frame in frame order, so
    where the launches are cut does not matter."""
    from p2igan_bench import ops
    S, T = 27, 6
    pred, truth = inputs(S, T)
    p, g = pred.astype(np.float32), scale_ref.as_dtype(truth, np.uint8)
    launches, real = [], ops.scale_fss
    monkeypatch.setattr(ops, "scale_fss", lambda *a, **k: (launches.append(a[0].shape[0]), real(*a, **k))[1])

    def run(max_frames):
        ev = evaluator(S, (1, 2, 5, 27, 55), (0.5, 2.0))
        ev.use_workspace, ev.max_frames = workspace, max_frames
        del launches[:]
        ev.update("m", p, g)
        return json.dumps(ev.compute()), ev.sums("m").tolist(), list(launches)
    whole = run(None)
    assert whole[2] == [T] and json.loads(whole[0])["m"]["frames"] == T
    for max_frames, want in ((1, [1] * 6), (2, [2, 2, 2]), (4, [4, 2])):
        res, sums, n = run(max_frames)
        assert n == want
        assert sums == whole[1], max_frames
        assert res == whole[0], max_frames


def test_large_crop_path_equals_lds_path_and_restatement():
    S, T = 128, 2
    pred, truth = inputs(S, T)
    p, g = pred.astype(np.float32), scale_ref.as_dtype(truth, np.uint8)
    scales = window_sizes(S)
    lds, big = evaluator(S, scales), evaluator(S, scales)
    assert not lds.use_workspace
    big.use_workspace = True
    lds.update("m", p, g)
    big.update("m", p, g)
    assert lds.sums("m").tolist() == big.sums("m").tolist()
    assert json.dumps(lds.compute()) == json.dumps(big.compute())
    S = 160
    pred, truth = inputs(S, 1)
    p, g = pred.astype(np.float64), scale_ref.as_dtype(truth, np.uint8)
    scales = (1, 2, 9, 159, 160, 161, 321)
    ev = evaluator(S, scales)
    assert ev.use_workspace
    ev.update("m", p, g)
    assert scale_ref.threshold_margin(p, THRESHOLDS) > 1e-9
    want = scale_ref.fss_sums(scale_ref.transform(scale_ref.crop(p, S)), scale_ref.transform(scale_ref.crop(g, S)), THRESHOLDS, scales)
    assert ev.sums("m").tolist() == want.tolist()
    check_spectra(ev.compute()["m"], scale_ref.run_scale({"m": p}, g, S, THRESHOLDS, scales)["m"], S)


def test_guards_on_the_device():
    from p2igan_bench.evaluation import ScaleEvaluator, run_scale
    ev = ScaleEvaluator(1024, (2.0,), (1025,))
    with pytest.raises(OverflowError):
        ev.update("m", np.zeros((8, 1024, 1024), np.uint8), np.zeros((8, 1024, 1024), np.uint8))
    with pytest.raises(ValueError, match="exceeds"):
        run_scale({"m": np.zeros((1, 8, 8), np.uint8)}, np.zeros((1, 8, 8), np.uint8), 16)


def test_cli_end_to_end(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts"))
    try:
        import evaluate
    finally:
        sys.path.pop(0)
    from p2igan_bench.data import zarr_lite
    from p2igan_bench.evaluation import run_scale
    S, H, W = 16, 20, 24
    truth = {f"event_{i + 1:02d}": scale_ref.as_dtype(scale_ref.field(300 + i, 3 + i, H, W), np.uint8)[:, None] for i in range(2)}
    preds = {"gan": {k: scale_ref.smoother(v[:, 0].astype(np.float64)).astype(np.float32)[:, None] for k, v in truth.items()},
             "idw": {k: scale_ref.smoother(scale_ref.smoother(v[:, 0].astype(np.float64))).astype(np.float32)[:, None]
                     for k, v in truth.items()}}
    for path, events in [("truth", truth)] + [(m, e) for m, e in preds.items()]:
        grp = zarr_lite.Group(str(tmp_path / f"{path}.zarr"), "w")
        for k, v in events.items():
            grp.create_dataset(k, v)
    np.savetxt(tmp_path / "mask.txt", (np.arange(H * W).reshape(H, W) % 7 == 0).astype(np.float64))
    out, sdir = tmp_path / "exp1", tmp_path / "scale"
    evaluate.main(["--truth", str(tmp_path / "truth.zarr"), "--method", f"gan={tmp_path / 'gan.zarr'}", "--method",
                   f"idw={tmp_path / 'idw.zarr'}", "--mask", str(tmp_path / "mask.txt"), "--crop-size", str(S), "--output", str(out),
                   "--thresholds", "0.5", "2", "--scale", str(sdir), "--scales", "1", "3", "8"])
    assert (out / "metrics.json").exists()
    for f in ("metrics.json", "metrics.txt", "scale_data.npz", "scale_panels.pdf"):
        assert (sdir / f).stat().st_size > 0, f
    want = run_scale(preds, truth, S, thresholds=(0.5, 2.0), scales=(1, 3, 8))
    assert list(want) == ["gan", "idw"] and want["gan"]["frames"] == 7
    assert (sdir / "metrics.json").read_text() == json.dumps(want, indent=2, sort_keys=True)
    lines = (sdir / "metrics.txt").read_text().splitlines()
    assert lines[0] == f"FSS_gan_thr0.5_n1: {want['gan']['FSS']['thr_0.5']['n_1']:.6f}" and f"LSD_idw: {want['idw']['LSD']:.6f}" in lines
