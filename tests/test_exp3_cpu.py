"""exp3 analysis on CPU: the numpy restatement (tests/exp3_ref.py) against tests/golden/exp3_cases.npz (captured from the reference
by tests/golden/make_golden_exp3.py), the numpy linregress against scipy's, the figure writer on a stored result, the exp3_data.npz
round trip, scripts/evaluate.py's --exp3 handling and the new ABI symbols."""
import json
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest

import exp3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [c["name"] for c in exp3_ref.CASES]


def golden_case(g, name):
    pre = f"{name}/"
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def sub(want, key):
    """{'<key>/<name>': v} -> {name: v}"""
    return {k.split("/", 1)[1]: v for k, v in want.items() if k.startswith(key + "/")}


def close(v, w, rel):
    if math.isnan(w):
        return math.isnan(v)
    return abs(v - w) <= rel * abs(w) or v == w


def check_against_golden(got, want, rel=1e-10, fit_tol=1e-12, exact_samples=True, exact_freq=True, exact_x=True):
    """got: {'metrics': {NSE_<n>: v}, 'nse', 'x', 'y', 'fit_scatter', 'fit_residual', 'freq_truth', 'freq'} (exp3_ref's layout)."""
    metrics = sub(want, "metrics")
    assert sorted(got["metrics"]) == sorted(f"NSE_{n}" for n in metrics)
    for n, w in metrics.items():
        assert close(got["metrics"][f"NSE_{n}"], float(w), rel), (n, got["metrics"][f"NSE_{n}"], float(w))
    nse = sub(want, "nse")
    assert sorted(got["nse"]) == sorted(nse)
    for n, w in nse.items():
        v = np.asarray(got["nse"][n], np.float64)
        assert v.shape == w.shape, n
        assert all(close(a, b, rel) for a, b in zip(v, w)), (n, v, w)
    xs, ys = sub(want, "x"), sub(want, "y")
    assert sorted(got["x"]) == sorted(xs)
    for n in xs:
        x, y = np.asarray(got["x"][n]), np.asarray(got["y"][n])
        assert x.shape == xs[n].shape and y.shape == ys[n].shape, n
        if exact_samples:
            assert np.array_equal(x, xs[n]) and np.array_equal(y, ys[n]), n
        else:
            if exact_x:
                assert np.array_equal(x, xs[n]), n      # uint8 truth: numpy's own table on both sides
            else:                                       # a float truth goes through the device pow, as the predictions do
                assert np.allclose(x, xs[n], rtol=fit_tol, atol=0), (n, float(np.max(np.abs(x - xs[n]))))
            assert np.allclose(y, ys[n], rtol=fit_tol, atol=0), (n, float(np.max(np.abs(y - ys[n]))))
    for key in ("fit_scatter", "fit_residual"):
        fw = sub(want, key)
        assert sorted(got[key]) == sorted(fw), key
        for n, w in fw.items():
            v = np.asarray(got[key][n], np.float64)
            assert np.all(np.abs(v - w) <= fit_tol * np.maximum(np.abs(w), 1.0)), (key, n, v, w)
    if "freq_truth" in want:
        cmp = np.array_equal if exact_freq else (lambda a, b: np.allclose(a, b, rtol=0, atol=1e-12))
        assert cmp(np.asarray(got["freq_truth"]), want["freq_truth"])
        fq = sub(want, "freq")
        assert sorted(got["freq"]) == sorted(fq)
        for n, w in fq.items():
            assert cmp(np.asarray(got["freq"][n]), w), n
    else:
        assert got.get("freq_truth") is None and not got["freq"]


def test_fixture_holds_every_case(golden):
    g = golden("exp3_cases.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "exp3_cases.npz")) < 160 * 1024
    for c in exp3_ref.CASES:
        assert str(g[f"{c['name']}/recipe"]) == exp3_ref.recipe_json(c), c["name"]
        # no float-transformed value within 1e-9 of a bin edge, no value within 1e-9 relative of 0.1: pools and bins are exact
        assert float(g[f"{c['name']}/edge_margin"]) > 1e-9, c["name"]
        assert float(g[f"{c['name']}/min_margin"]) > 1e-9, c["name"]


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference(golden, case):
    g = golden("exp3_cases.npz")
    c = next(c for c in exp3_ref.CASES if c["name"] == case)
    want = golden_case(g, case)
    preds, truth, mask, kw = exp3_ref.build_case(c)
    if "error" in want:
        typ, msg = str(want["error"]).split(": ", 1)
        with pytest.raises({"ValueError": ValueError, "TypeError": TypeError}[typ], match=re.escape(msg)):
            exp3_ref.exp3(preds, truth, mask, **kw)
        return
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = exp3_ref.exp3(preds, truth, mask, **kw)
    check_against_golden(got, want)


def test_golden_cases_cover_the_issue_list(golden):
    g = golden("exp3_cases.npz")
    # sampling: 2000 points where the pool is larger; the mostly-NaN method in between is not sampled
    assert g["radar_sampled/x/gan"].size == 2000 and g["radar_sampled/x/stdk"].size == 2000
    assert 2 <= g["radar_sampled/x/sparse"].size < 2000
    assert g["gauge_small/x/gan"].size <= 2000
    assert g["missing_event/nse/gan"].size == 2 and g["missing_event/nse/stdk"].size == 3
    # the carry-over: "full" inherits the cuts of "short" (its stack is as short), so its panel pool is no larger
    assert g["carry_over/nse/short"].size == g["carry_over/nse/full"].size == 3
    assert g["carry_over/x/full"].size == g["carry_over/x/short"].size
    assert math.isnan(float(g["nan_pred/metrics/allnan"])) and np.isnan(g["nan_pred/nse/allnan"]).all()
    assert "nan_pred/freq/allnan" not in g.files and "nan_pred/freq/gan" in g.files
    assert "array_input/nse/gan" not in g.files and "array_input/freq_truth" not in g.files and "array_input/x/gan" in g.files
    assert g["tiny_pool/x/gan"].size == 1 and g["tiny_pool/x/holed"].size == 0 and "tiny_pool/fit_scatter/gan" not in g.files
    assert str(g["err_not_dict/error"]).startswith("ValueError") and str(g["err_crop/error"]).startswith("ValueError")
    assert str(g["err_dict_array/error"]).startswith("TypeError")


def test_constant_frame_nse_is_clipped():
    c = next(c for c in exp3_ref.CASES if c["name"] == "constant_frame")
    preds, truth, mask, kw = exp3_ref.build_case(c)
    g = np.asarray(truth["event_01"])[2, 0]
    assert g.min() == g.max()
    # the per-event NSE of the case is the mean over 5 frames, one of them clipped to 0: recomputed without the clip it differs
    from exp1_ref import crop, transform
    sel = mask.ravel()
    p = crop(transform(preds["gan"]["event_01"]), 8)[2].ravel()[sel]
    gg = crop(transform(truth["event_01"]), 8)[2].ravel()[sel]
    assert 1.0 - np.sum((p - gg) ** 2) / (np.sum((gg - gg.mean()) ** 2) + 1e-10) < -1e6


def test_linregress_matches_scipy():
    stats = pytest.importorskip("scipy.stats")
    from p2igan_bench.evaluation import linregress
    rng = np.random.default_rng(5)
    for i in range(50):
        n = int(rng.integers(2, 3000))
        x = rng.uniform(0.1, 32, n)
        y = x * rng.uniform(-2, 2) + rng.normal(0, rng.uniform(0, 5), n)
        if i == 0:
            y = 3.0 * x + 1.0                       # exact line: r clamps to 1
        if i == 1:
            y = np.full(n, 2.5)                     # constant y: r = 0
        want = stats.linregress(x, y)
        got = linregress(x, y)
        for v, w in zip(got, (want.slope, want.intercept, want.rvalue)):
            assert v == w or abs(v - w) <= 1e-13 * max(abs(w), 1.0), (i, got, want)
    for bad in ((np.array([1.0, 1.0]), np.array([1.0, 2.0])), (np.array([]), np.array([]))):
        with pytest.raises(ValueError) as a:
            linregress(*bad)
        with pytest.raises(ValueError) as b:
            stats.linregress(*bad)
        assert str(a.value) == str(b.value)


def _stored_result(golden, case):
    """An Exp3Result assembled from a fixture case (the reference's numbers), as exp3_data.npz holds one."""
    from p2igan_bench.evaluation import LOGFREQ_EDGES, Exp3Result
    want = golden_case(golden("exp3_cases.npz"), case)
    names = list(sub(want, "metrics"))
    xs, ys = sub(want, "x"), sub(want, "y")
    r = Exp3Result(methods=names, metrics={f"NSE_{n}": float(v) for n, v in sub(want, "metrics").items()},
                   nse_by_method={n: [float(a) for a in v] for n, v in sub(want, "nse").items()},
                   per_event="freq_truth" in want, has_scatter=bool(xs), pool={n: int(xs[n].size) for n in xs},
                   x=xs, y_scatter=ys, y_residual={n: ys[n] - xs[n] for n in xs},
                   fit_scatter={n: tuple(float(a) for a in v) for n, v in sub(want, "fit_scatter").items()},
                   fit_residual={n: tuple(float(a) for a in v) for n, v in sub(want, "fit_residual").items()})
    if r.per_event:
        r.logfreq_edges, r.freq_truth, r.freq = LOGFREQ_EDGES.copy(), want["freq_truth"], sub(want, "freq")
    return r


def test_exp3_data_round_trip(golden, tmp_path):
    from p2igan_bench.evaluation import Exp3Result
    for case in ("radar_sampled", "array_input", "tiny_pool"):
        r = _stored_result(golden, case)
        r.save(str(tmp_path / f"{case}.npz"))
        b = Exp3Result.load(str(tmp_path / f"{case}.npz"))
        assert b.methods == r.methods and b.per_event == r.per_event and b.has_scatter == r.has_scatter and b.pool == r.pool
        assert json.dumps(b.metrics) == json.dumps(r.metrics) and json.dumps(b.nse_by_method) == json.dumps(r.nse_by_method)
        assert b.fit_scatter == r.fit_scatter and b.fit_residual == r.fit_residual
        for key in ("x", "y_scatter", "y_residual", "freq"):
            assert sorted(getattr(b, key)) == sorted(getattr(r, key))
            for n, v in getattr(r, key).items():
                assert np.array_equal(getattr(b, key)[n], v), (case, key, n)
        assert (b.freq_truth is None) == (r.freq_truth is None)


def test_figures_from_stored_result(golden, tmp_path):
    pytest.importorskip("matplotlib")
    from p2igan_bench.evaluation import Exp3Result, write_exp3_figures
    r = _stored_result(golden, "radar_sampled")
    r.save(str(tmp_path / "exp3_data.npz"))
    out = tmp_path / "figs"
    written = write_exp3_figures(Exp3Result.load(str(tmp_path / "exp3_data.npz")), str(out))
    names = ("scatter_panels.pdf", "residual_panels.pdf", "nse_boxplot.pdf", "logfreq.pdf")
    assert sorted(os.path.basename(p) for p in written) == sorted(names)
    for n in names:
        assert (out / n).read_bytes()[:5] == b"%PDF-", n
    # the array path has no per-event NSE and no log-frequency figure; a single-point pool gets a panel without a fit
    a = write_exp3_figures(_stored_result(golden, "array_input"), str(tmp_path / "arr"))
    assert sorted(os.path.basename(p) for p in a) == ["residual_panels.pdf", "scatter_panels.pdf"]
    t = write_exp3_figures(_stored_result(golden, "tiny_pool"), str(tmp_path / "tiny"))
    assert len(t) == 4


def test_figures_skip_without_matplotlib(golden, tmp_path, monkeypatch):
    import builtins
    from p2igan_bench.evaluation import write_exp3_figures
    real = builtins.__import__

    def no_mpl(name, *a, **k):
        if name.split(".")[0] == "matplotlib":
            raise ImportError("no matplotlib")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_mpl)
    with pytest.warns(UserWarning, match="matplotlib"):
        assert write_exp3_figures(_stored_result(golden, "radar_sampled"), str(tmp_path)) == []
    assert not list(tmp_path.iterdir())


def test_evaluator_refuses_to_run_without_gpu(monkeypatch):
    import torch
    from p2igan_bench import evaluation
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluation.Exp3Evaluator(np.zeros((16, 16), bool), "radar", 16, ["a"])
    with pytest.raises(RuntimeError, match="GPU"):
        evaluation.compute_exp3({"a": {"e": np.zeros((2, 16, 16), np.float32)}}, {"e": np.zeros((2, 16, 16), np.uint8)},
                                np.zeros((16, 16), bool), "radar", 16)


def _evaluate_module():
    sys.path.insert(0, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts"))
    try:
        import evaluate
    finally:
        sys.path.pop(0)
    return evaluate


def test_cli_exp3_flag_parses_and_writes_main_layout(tmp_path):
    ev = _evaluate_module()
    a = ev.parse_args(["--truth", "t", "--method", "x=y", "--mask", "m", "--output", "o", "--exp3", str(tmp_path / "e3")])
    assert a.exp3 == str(tmp_path / "e3")
    assert ev.parse_args(["--truth", "t", "--method", "x=y", "--mask", "m", "--output", "o"]).exp3 is None
    ev.write_exp3_outputs(str(tmp_path / "e3"), {"NSE_gan": 0.5, "NSE_idw": float("nan"), "NSE_b": -1 / 3})
    assert (tmp_path / "e3" / "metrics.txt").read_text() == "NSE_gan: 0.500000\nNSE_idw: nan\nNSE_b: -0.333333\n"
    assert json.loads((tmp_path / "e3" / "metrics.json").read_text(), parse_constant=float)["NSE_gan"] == 0.5


def test_exp3_abi_is_declared_bound_and_documented():
    from p2igan_bench import _hip
    hdr = open(os.path.join(ROOT, "include", "p2i_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = ("p2i_exp3_accumulate", "p2i_exp3_truth_hist", "p2i_exp3_scan", "p2i_exp3_gather", "p2i_exp3_nse")
    for n in names:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _hip.SIGNATURES, n
        assert n in doc, n
    import ctypes
    lib = ctypes.CDLL(_hip.lib_path())
    for n in names:
        assert hasattr(lib, n), n
    mk = open(os.path.join(ROOT, "p2i-gan-benchmark_amd", "csrc", "Makefile")).read()
    assert "eval_exp3.hip" in mk and "eval_common.h" in mk
