"""exp1 scoring on the MI355X (csrc/eval_exp1.hip through p2igan_bench.evaluation): the reference's numbers from
tests/golden/exp1_cases.npz, a bigger case against the numpy restatement tests/exp1_ref.py, input forms, determinism, the device
transform's agreement with numpy, and scripts/evaluate.py end to end."""
import json
import math
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import exp1_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT32_KEYS = ("SSIM", "DTSSIM_L1", "DTSSIM_L2")
CAT_SUBS = ("POD", "FAR", "CSI", "HSS")


def assert_device_matches(got: dict, want: dict):
    """MAE / RMSE / NSE within 1e-9 relative, PSS and the categorical scores within 1e-12 (exact counts), SSIM terms within 5e-6
    absolute; NaN exactly where the reference has NaN."""
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        v = got[k]
        key = k.split("/")[1]
        if math.isnan(w):
            assert math.isnan(v), (k, v, w)
            continue
        assert not math.isnan(v), (k, v, w)
        if key in FLOAT32_KEYS:
            assert abs(v - w) <= 5e-6, (k, v, w)
        elif key in ("MAE", "RMSE", "NSE"):
            assert abs(v - w) <= 1e-9 * abs(w) + 1e-300, (k, v, w)
        else:
            assert abs(v - w) <= 1e-12 * abs(w) + 1e-300, (k, v, w)


def _ref(preds, truth, mask, kw):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return exp1_ref.flatten(exp1_ref.run_exp1(preds, truth, mask, **kw))


@pytest.mark.parametrize("case", [c["name"] for c in exp1_ref.CASES])
def test_golden_case_on_device(golden, case):
    from p2igan_bench.evaluation import run_exp1
    g = golden("exp1_cases.npz")
    c = next(c for c in exp1_ref.CASES if c["name"] == case)
    want = {k[len(case) + 1:]: g[k] for k in g.files if k.startswith(case + "/")}
    preds, truth, mask, kw = exp1_ref.build_case(c)
    if "error" in want:
        msg = str(want["error"]).split(": ", 1)[1]
        with pytest.raises(ValueError, match=re.escape(msg)):
            run_exp1(preds, truth, mask, **kw)
        return
    got = exp1_ref.flatten(run_exp1(preds, truth, mask, **kw))
    assert_device_matches(got, {k: float(v) for k, v in want.items() if k not in ("recipe", "thr_margin")})


def _big(mode):
    rng_seeds = {"p2igan": (301, 10.0, 0.02, 0.01), "stdk": (302, 25.0, 0.05, 0.0), "idw": (303, 40.0, 0.0, 0.03)}
    from p2igan_bench.utils import seeded
    truths = [seeded.exp1_truth(500 + i, t, 160, 144) for i, t in enumerate((40, 60, 52))]
    keys = [f"event_{i + 1:02d}" for i in range(3)]
    preds = {name: {k: seeded.exp1_pred(s * 10 + i, g, n, z, o) for i, (k, g) in enumerate(zip(keys, truths))}
             for name, (s, n, z, o) in rng_seeds.items()}
    mask = seeded.exp1_mask(77, 128, 128, 0.3 if mode == "radar" else 0.02)
    return preds, dict(zip(keys, truths)), mask


@pytest.mark.parametrize("mode", ["radar", "gauge"])
def test_bigger_case_matches_restatement(mode):
    from p2igan_bench.evaluation import run_exp1
    preds, truth, mask = _big(mode)
    kw = {"mode": mode, "crop_size": 128, "thresholds": (0.5, 2.0, 4.0, 8.0), "use_pool8": True}
    got = exp1_ref.flatten(run_exp1(preds, truth, mask, **kw))
    assert_device_matches(got, _ref(preds, truth, mask, kw))


def test_input_forms_and_streaming_agree_bit_for_bit():
    from p2igan_bench.evaluation import Exp1Evaluator, run_exp1
    preds, truth, mask = _big("radar")
    keys = list(truth)
    a = run_exp1(preds, truth, mask, "radar", 128)
    cat_truth = np.concatenate([truth[k] for k in keys])
    cat_preds = {n: np.concatenate([p[k] for k in keys]) for n, p in preds.items()}
    b = run_exp1(cat_preds, cat_truth, mask, "radar", 128)
    dev = torch.device("cuda")
    c = run_exp1({n: torch.from_numpy(p).to(dev) for n, p in cat_preds.items()}, torch.from_numpy(cat_truth).to(dev), mask, "radar", 128)
    ev = Exp1Evaluator(mask, "radar", 128)
    for n, p in preds.items():
        for k in keys:
            ev.update(n, p[k], truth[k])
    d = ev.compute()
    fa = exp1_ref.flatten(a)
    for other in (b, c, d):
        fo = exp1_ref.flatten(other)
        assert fa.keys() == fo.keys()
        for k in fa:
            assert np.float64(fa[k]).tobytes() == np.float64(fo[k]).tobytes(), k


def _cut_case():
    """crop 16 with 8x8 pooling, T = 5: a float32 prediction [5, 1, 20, 24] (crop origin (2, 4)) that follows a uint8 truth
    [5, 1, 23, 19] (crop origin (3, 1)) inside the crop and holds unrelated values around it, and a mask with both classes."""
    from p2igan_bench.utils import seeded
    S, T = 16, 5
    truth = seeded.exp1_truth(610, T, 23, 19)
    pred = seeded.exp1_pred(611, seeded.exp1_truth(612, T, 20, 24), 30.0)
    pred[:, :, 2:2 + S, 4:4 + S] = seeded.exp1_pred(613, truth[:, :, 3:3 + S, 1:1 + S], 10.0, 0.02, 0.01)
    mask = seeded.exp1_mask(614, S, S, 0.3)
    assert pred.dtype == np.float32 and truth.dtype == np.uint8 and mask.any() and not mask.all()
    return pred, truth, mask


@pytest.mark.parametrize("mode", ["radar", "gauge"])
def test_launch_cuts_inside_one_update_agree_bit_for_bit(monkeypatch, mode):
    """``max_frames`` cuts the five frames of one update into launches of 1 and of 2 frames (2 + 2 + 1).  Where the launches are cut
    does not matter: every value is bit-identical to the single launch's, dTSSIM (which pairs frames across the cuts) included."""
    from p2igan_bench import ops
    from p2igan_bench.evaluation import Exp1Evaluator
    pred, truth, mask = _cut_case()
    kw = {"mode": mode, "crop_size": 16, "thresholds": (0.5, 2.0, 4.0, 8.0), "use_pool8": True}
    launches, real = [], ops.exp1_accumulate
    monkeypatch.setattr(ops, "exp1_accumulate", lambda *a, **k: (launches.append(a[0].shape[0]), real(*a, **k))[1])

    def run(max_frames):
        ev = Exp1Evaluator(mask, **kw)
        ev.max_frames = max_frames
        del launches[:]
        ev.update("m", pred, truth)
        return exp1_ref.flatten(ev.compute()), list(launches)
    whole, n_whole = run(None)
    assert n_whole == [5]
    assert_device_matches(whole, _ref({"m": pred}, truth, mask, kw))        # the input says something: it scores as restated
    assert not any(math.isnan(v) for k, v in whole.items() if k.split("/")[1] in FLOAT32_KEYS + ("PSS",))
    for max_frames, want in ((1, [1] * 5), (2, [2, 2, 1])):
        cut, n_cut = run(max_frames)
        assert n_cut == want
        assert cut.keys() == whole.keys()
        for k in whole:
            assert np.float64(cut[k]).tobytes() == np.float64(whole[k]).tobytes(), (max_frames, k)


def test_two_runs_are_bit_identical():
    from p2igan_bench.evaluation import run_exp1
    preds, truth, mask = _big("gauge")
    r1 = exp1_ref.flatten(run_exp1(preds, truth, mask, "gauge", 128))
    r2 = exp1_ref.flatten(run_exp1(preds, truth, mask, "gauge", 128))
    assert all(np.float64(r1[k]).tobytes() == np.float64(r2[k]).tobytes() for k in r1)


def test_device_transform_agrees_with_numpy():
    """Device pow (fp64) vs numpy's transform: measured ulp distance, reported; the uint8 path uses numpy's own table."""
    from p2igan_bench import ops
    from p2igan_bench.evaluation import transform_mmhr
    rng = np.random.default_rng(3)
    x = np.concatenate([np.arange(256, dtype=np.float32), rng.uniform(-10, 400, 200000).astype(np.float32),
                        np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32)])
    for div3 in (True, False):
        want = transform_mmhr(x, div3)
        got = ops.exp1_transform(torch.from_numpy(x).cuda(), div3).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        ulp = np.abs(got[ok].view(np.int64) - want[ok].view(np.int64))
        print(f"device transform vs numpy (divide_by_3={div3}): max {int(ulp.max())} ulp, {float((ulp == 0).mean()) * 100:.2f} % equal")
        assert ulp.max() <= 4


def test_cli_end_to_end(tmp_path):
    from p2igan_bench.data import zarr_lite
    from p2igan_bench.evaluation import crop_mask, run_exp1
    from p2igan_bench.utils import seeded
    truths = {f"event_{i + 1:02d}": seeded.exp1_truth(900 + i, t, 48, 40) for i, t in enumerate((9, 14))}
    g = zarr_lite.Group(str(tmp_path / "truth.zarr"), "w")
    for k, v in truths.items():
        g.create_dataset(k, v, chunks=v.shape)
    preds = {}
    for j, name in enumerate(("p2igan", "idw")):
        pg = zarr_lite.Group(str(tmp_path / f"{name}.zarr"), "w")
        preds[name] = {}
        for i, (k, v) in enumerate(truths.items()):
            p = seeded.exp1_pred(950 + 10 * j + i, v, 12.0 + 10 * j)
            pg.create_dataset(k, p, chunks=p.shape)
            preds[name][k] = p
    full = seeded.exp1_mask(5, 48, 40, 0.2)
    np.savetxt(tmp_path / "mask.txt", full.astype(np.float64), fmt="%d")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts", "evaluate.py"), "--truth", str(tmp_path / "truth.zarr"),
           "--method", f"p2igan={tmp_path / 'p2igan.zarr'}", "--method", f"idw={tmp_path / 'idw.zarr'}", "--mask", str(tmp_path / "mask.txt"),
           "--mode", "radar", "--crop-size", "32", "--output", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads((out / "metrics.json").read_text())
    want = json.loads(json.dumps(run_exp1(preds, truths, crop_mask(full, 32), "radar", 32)))
    assert exp1_ref.flatten(got).keys() == exp1_ref.flatten(want).keys()
    for k, v in exp1_ref.flatten(want).items():
        w = exp1_ref.flatten(got)[k]
        assert (math.isnan(v) and math.isnan(w)) or v == w, k
    assert (out / "metrics.txt").read_text().startswith("[p2igan]\nMAE: ")
    # a method zarr that lacks a truth event is refused, naming the event
    bad = zarr_lite.Group(str(tmp_path / "bad.zarr"), "w")
    bad.create_dataset("event_01", preds["idw"]["event_01"])
    r = subprocess.run(cmd[:2] + ["--truth", str(tmp_path / "truth.zarr"), "--method", f"bad={tmp_path / 'bad.zarr'}", "--mask",
                                  str(tmp_path / "mask.txt"), "--crop-size", "32", "--output", str(tmp_path / "o2")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "event_02" in r.stderr
