"""exp1 scoring on CPU: the numpy restatement (tests/exp1_ref.py) against tests/golden/exp1_cases.npz (captured from the reference
by tests/golden/make_golden_exp1.py), the host tables the device path relies on (uint8 transform table, PSS edges and bin rule),
scripts/evaluate.py's argument handling and output layout, and the new ABI symbols."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

import exp1_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT32_KEYS = ("SSIM", "DTSSIM_L1", "DTSSIM_L2")


def golden_case(g, name):
    pre = f"{name}/"
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def assert_matches(got: dict, want: dict, rel=1e-12, ssim_abs=1e-6):
    """got / want: flattened {'method/KEY[/SUB]': float}.  NaN where the other is NaN; SSIM terms within ssim_abs."""
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        v = got[k]
        if math.isnan(w):
            assert math.isnan(v), (k, v, w)
            continue
        assert not math.isnan(v), (k, v, w)
        if k.split("/")[1] in FLOAT32_KEYS:
            assert abs(v - w) <= ssim_abs, (k, v, w)
        else:
            assert abs(v - w) <= rel * max(abs(w), 1e-300) or v == w, (k, v, w, abs(v - w) / max(abs(w), 1e-300))


def test_fixture_holds_every_case(golden):
    g = golden("exp1_cases.npz")
    for c in exp1_ref.CASES:
        assert str(g[f"{c['name']}/recipe"]) == exp1_ref.recipe_json(c), c["name"]
        # no transformed value sits within 1e-12 relative of a threshold: the contingency counts are exact
        assert float(g[f"{c['name']}/thr_margin"]) > 1e-9, c["name"]


@pytest.mark.parametrize("case", [c["name"] for c in exp1_ref.CASES])
def test_restatement_reproduces_reference(golden, case):
    g = golden("exp1_cases.npz")
    c = next(c for c in exp1_ref.CASES if c["name"] == case)
    want = golden_case(g, case)
    preds, truth, mask, kw = exp1_ref.build_case(c)
    if "error" in want:
        typ, msg = str(want["error"]).split(": ", 1)
        assert typ == "ValueError"
        with pytest.raises(ValueError, match=re.escape(msg)):
            exp1_ref.run_exp1(preds, truth, mask, **kw)
        return
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = exp1_ref.flatten(exp1_ref.run_exp1(preds, truth, mask, **kw))
    want = {k: float(v) for k, v in want.items() if k not in ("recipe", "thr_margin")}
    assert_matches(got, want)


def test_golden_cases_cover_the_issue_list(golden):
    g = golden("exp1_cases.npz")
    f = {k: float(g[k]) for k in g.files if not k.endswith("/recipe") and not k.endswith("/error")}
    assert math.isnan(f["t2/gan/DTSSIM_L2"]) and not math.isnan(f["t2/gan/DTSSIM_L1"])
    assert math.isnan(f["t1/gan/DTSSIM_L1"]) and math.isnan(f["t1/gan/DTSSIM_L2"])
    assert math.isnan(f["below_half/gan/PSS"])
    assert "Too many bins" in str(g["constant/error"])
    assert math.isnan(f["nan_pred/gan/MAE"]) and math.isnan(f["nan_pred/gan/SSIM"]) and not math.isnan(f["nan_pred/gan/PSS"])
    assert not math.isnan(f["nan_pred/clean/MAE"])
    e = {k.split("/", 2)[2]: v for k, v in f.items() if k.startswith("empty_sel/gan/")}
    assert math.isnan(e["MAE"]) and math.isnan(e["RMSE"]) and math.isnan(e["PSS"]) and e["NSE"] == 1.0
    assert e["CAT_0.5/POD"] == 0.0 and e["CAT_0.5/FAR"] == 0.0 and e["CAT_0.5/CSI"] == 0.0 and math.isnan(e["CAT_0.5/HSS"])
    assert "gauge_nopool/gan/CAT_1/POD" in f


def test_truth_table_is_transform_bit_for_bit():
    from p2igan_bench.evaluation import transform_mmhr, truth_lut
    for div3 in (True, False):
        lut = truth_lut(div3)
        ref = transform_mmhr(np.arange(256, dtype=np.float64), div3)
        assert lut.dtype == np.float64 and lut.shape == (256,)
        assert np.array_equal(lut.view(np.int64), ref.view(np.int64))
        assert np.array_equal(lut.view(np.int64), exp1_ref.transform(np.arange(256), div3).view(np.int64))
    assert truth_lut()[255] == 200.0         # saturates


def test_transform_keeps_nan_and_clips():
    from p2igan_bench.evaluation import transform_mmhr
    x = np.array([np.nan, -np.inf, -5.0, 0.0, 300.0, np.inf, 1e30], dtype=np.float32)
    y = transform_mmhr(x)
    assert math.isnan(y[0])
    assert y[1] == y[2] == y[3] == transform_mmhr(0.001)
    assert y[4] == y[5] == y[6] == 200.0


def test_pss_edges_and_bin_rule_equal_np_histogram():
    from p2igan_bench.evaluation import pss_bin, pss_edges
    rng = np.random.default_rng(7)
    for i in range(300):
        lo = float(np.float32(rng.uniform(0.5, 150.0)))
        hi = float(np.float32(lo + rng.choice([1e-3, 0.1, 5.0, 60.0]) * rng.random() + 1e-4))
        if i == 0:
            hi = 200.0
        try:
            np.histogram(np.array([lo], np.float32), bins=50, range=(lo, hi))
        except ValueError:                  # too narrow for 50 float32 bins: refused by both
            with pytest.raises(ValueError, match="Too many bins"):
                pss_edges(lo, hi)
            continue
        edges = pss_edges(lo, hi)
        assert np.array_equal(edges, np.histogram_bin_edges(np.array([lo], np.float32), bins=50, range=(lo, hi)))
        probe = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)),
                                rng.uniform(lo, hi, 200).astype(np.float32)]).astype(np.float32)
        probe = probe[(probe >= edges[0]) & (probe <= edges[-1])]
        want = np.histogram(probe, bins=50, range=(lo, hi))[0]
        got = np.bincount(pss_bin(probe, edges), minlength=50)
        assert np.array_equal(got, want), i


def test_constant_range_refused_like_np_histogram():
    from p2igan_bench.evaluation import pss_edges
    v = float(np.float32(48.0))
    with pytest.raises(ValueError, match="Too many bins"):
        np.histogram(np.array([v], np.float32), bins=50, range=(v, v + 1e-6))
    with pytest.raises(ValueError, match="Too many bins"):
        pss_edges(v, v)


def test_evaluator_refuses_to_run_without_gpu(monkeypatch):
    import torch
    from p2igan_bench import evaluation
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluation.Exp1Evaluator(np.zeros((16, 16), bool), "radar", 16)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluation.run_exp1({"a": np.zeros((2, 16, 16), np.float32)}, np.zeros((2, 16, 16), np.uint8), np.zeros((16, 16), bool),
                            "radar", 16)


def test_selection_rules():
    from p2igan_bench.evaluation import crop_origin, selection
    m = np.zeros((4, 4), bool)
    m[1, 2] = True
    assert selection(m, "gauge", 4).sum() == 1 and selection(m, "radar", 4).sum() == 15
    with pytest.raises(ValueError, match="Mask shape"):
        selection(m, "radar", 5)
    with pytest.raises(ValueError, match="Unknown mode"):
        selection(m, "satellite", 4)
    assert crop_origin(40, 48, 32) == (4, 8) and crop_origin(45, 45, 36) == (4, 4)
    with pytest.raises(ValueError, match="exceeds"):
        crop_origin(30, 40, 32)


def test_event_lists_rules():
    """run_exp1's reading of (preds, truth), which run_scale and run_objects share."""
    from p2igan_bench.evaluation._common import event_lists
    a, b, c = (np.full((2, 4, 4), v, np.uint8) for v in (1, 2, 3))
    truth = {"z": a, "m": None, "k": b, "a": c}                      # not sorted: the truth's own key order counts
    preds = {"full": {"a": c + 10, "k": b + 10, "z": a + 10}, "lacks_k": {"z": a + 20, "k": None, "a": c + 20, "extra": a},
             "array": a + 30, "none": {}}
    events, methods = event_lists(preds, truth)
    assert [int(e[0, 0, 0]) for e in events] == [1, 2, 3]           # the None-valued event is dropped
    assert list(methods) == ["full", "lacks_k", "none"]              # a method that is not a dict is left out
    assert [int(e[0, 0, 0]) for e in methods["full"]] == [11, 12, 13]
    assert [int(e[0, 0, 0]) for e in methods["lacks_k"]] == [21, 23]         # skipped for this method only
    assert methods["none"] == []
    events, methods = event_lists({"m": a + 1, "n": b}, a)
    assert len(events) == 1 and events[0] is a and list(methods) == ["m", "n"] and methods["n"][0] is b
    with pytest.raises(TypeError, match="method 'd': per-event predictions need a per-event truth"):
        event_lists({"m": a, "d": {"z": a}}, a)
    assert event_lists(preds, {}) == ([], {})
    with pytest.raises(ValueError, match=r"Expected \[T,H,W\], got shape \(0,\)"):
        event_lists(preds, {"z": None})


def _evaluate_module():
    sys.path.insert(0, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts"))
    try:
        import evaluate
    finally:
        sys.path.pop(0)
    return evaluate


def test_cli_parses_and_pairs(tmp_path):
    ev = _evaluate_module()
    a = ev.parse_args(["--truth", "t.zarr", "--method", "gan=g.zarr", "--method", "stdk=s.zarr", "--mask", "m.txt", "--mode", "gauge",
                       "--crop-size", "64", "--no-pool8", "--thresholds", "1", "2", "--output", str(tmp_path)])
    assert a.method == [("gan", "g.zarr"), ("stdk", "s.zarr")] and a.mode == "gauge" and a.crop_size == 64 and a.no_pool8
    assert a.thresholds == [1.0, 2.0] and a.device is None
    d = ev.parse_args(["--truth", "t", "--method", "x=y", "--mask", "m", "--output", "o"])
    assert d.crop_size == 128 and d.mode == "radar" and not d.no_pool8 and tuple(d.thresholds) == (0.5, 2.0, 4.0, 8.0)
    with pytest.raises(SystemExit):
        ev.parse_args(["--truth", "t", "--method", "noequals", "--mask", "m", "--output", "o"])
    with pytest.raises(SystemExit):
        ev.parse_args(["--truth", "t", "--method", "x=a", "--method", "x=b", "--mask", "m", "--output", "o"])
    ev.check_events(["event_01", "event_02"], "gan", {"event_01", "event_02", "event_03"})
    with pytest.raises(ValueError, match="'gan' lacks truth event 'event_02'"):
        ev.check_events(["event_01", "event_02"], "gan", {"event_01"})


def test_cli_mask_crop_and_event_order(tmp_path):
    ev = _evaluate_module()
    from p2igan_bench.data import zarr_lite
    full = (np.arange(10 * 12).reshape(10, 12) % 3 == 0).astype(np.float64)
    np.savetxt(tmp_path / "mask.txt", full)
    m = ev.load_mask(str(tmp_path / "mask.txt"), 6)
    assert m.dtype == bool and np.array_equal(m, full.astype(bool)[2:8, 3:9])
    g = zarr_lite.Group(str(tmp_path / "t.zarr"), "w")
    for k in ("event_10", "event_02", "event_01"):
        g.create_dataset(k, np.full((2, 1, 4, 4), int(k[-2:]), np.uint8))
    evs = ev.load_events(str(tmp_path / "t.zarr"))
    assert list(evs) == ["event_01", "event_02", "event_10"] and evs["event_10"].dtype == np.uint8


def test_cli_output_layout_matches_main(tmp_path):
    ev = _evaluate_module()
    metrics = {"gan": {"MAE": 1.5, "PSS": float("nan"), "CAT_0.5": {"POD": 0.25, "FAR": 0.0, "CSI": 1 / 3, "HSS": 0.5}},
               "idw": {"MAE": 2.0, "CAT_0.5": {"POD": 1.0, "FAR": 0.0, "CSI": 1.0, "HSS": 1.0}}}
    ev.write_outputs(str(tmp_path), metrics)
    txt = (tmp_path / "metrics.txt").read_text().splitlines()
    assert txt[:9] == ["[gan]", "MAE: 1.500000", "PSS: nan", "CAT_0.5:", "  POD: 0.250000", "  FAR: 0.000000", "  CSI: 0.333333",
                       "  HSS: 0.500000", ""]
    assert txt[9] == "[idw]" and txt[-1] == ""
    raw = (tmp_path / "metrics.json").read_text()
    assert raw == json.dumps(metrics, indent=2, sort_keys=True)


def test_exp1_abi_is_declared_bound_and_documented():
    from p2igan_bench import _hip
    hdr = open(os.path.join(ROOT, "include", "p2i_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = ("p2i_exp1_transform", "p2i_exp1_workspace", "p2i_exp1_accumulate", "p2i_exp1_merge", "p2i_exp1_hist", "p2i_exp1_ssim", "p2i_exp1_finalize")
    for n in names:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _hip.SIGNATURES, n
        assert n in doc, n
    import ctypes
    lib = ctypes.CDLL(_hip.lib_path())
    for n in names:
        assert hasattr(lib, n), n
    assert "eval_exp1.hip" in open(os.path.join(ROOT, "p2i-gan-benchmark_amd", "csrc", "Makefile")).read()
