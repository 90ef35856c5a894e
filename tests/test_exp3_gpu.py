"""exp3 analysis on the MI355X (csrc/eval_exp3.hip through p2igan_bench.evaluation): the reference's numbers from
tests/golden/exp3_cases.npz, bigger cases against the numpy restatement tests/exp3_ref.py, determinism, input forms, and
scripts/evaluate.py --exp3 end to end."""
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import exp3_ref
from test_exp3_cpu import check_against_golden, golden_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def as_ref_layout(r):
    """Exp3Result -> exp3_ref's dict layout."""
    return {"metrics": r.metrics, "nse": r.nse_by_method, "x": r.x, "y": r.y_scatter,
            "fit_scatter": {n: v for n, v in r.fit_scatter.items() if r.x[n].size >= 2},
            "fit_residual": {n: v for n, v in r.fit_residual.items() if r.x[n].size >= 2},
            "freq_truth": r.freq_truth, "freq": r.freq}


def as_golden_layout(ref):
    """exp3_ref's output -> the fixture's flat layout (the arbiter for the bigger cases)."""
    w = {f"metrics/{k[4:]}": np.float64(v) for k, v in ref["metrics"].items()}
    w.update({f"nse/{n}": np.array(v, np.float64) for n, v in ref["nse"].items()})
    for key in ("x", "y", "fit_scatter", "fit_residual", "freq"):
        w.update({f"{key}/{n}": np.asarray(v, np.float64) for n, v in ref[key].items()})
    if "freq_truth" in ref:
        w["freq_truth"] = ref["freq_truth"]
    return w


@pytest.mark.parametrize("case", [c["name"] for c in exp3_ref.CASES])
def test_golden_case_on_device(golden, case, tmp_path):
    from p2igan_bench.evaluation import Exp3Result, run_exp3
    c = next(c for c in exp3_ref.CASES if c["name"] == case)
    want = golden_case(golden("exp3_cases.npz"), case)
    preds, truth, mask, kw = exp3_ref.build_case(c)
    if "error" in want:
        typ, msg = str(want["error"]).split(": ", 1)
        with pytest.raises({"ValueError": ValueError, "TypeError": TypeError}[typ], match=re.escape(msg)):
            run_exp3(preds, truth, mask, out_dir=str(tmp_path), **kw)
        return
    metrics = run_exp3(preds, truth, mask, out_dir=str(tmp_path), **kw)
    res = Exp3Result.load(str(tmp_path / "exp3_data.npz"))
    assert json.dumps(metrics) == json.dumps(res.metrics)
    # samples: the observed values exactly (uint8 truth: numpy's table), the predicted within 1e-12; frequencies exact
    check_against_golden(as_ref_layout(res), want, rel=1e-10, fit_tol=1e-12, exact_samples=False, exact_freq=True)
    for n in res.methods:
        if n in res.x:
            assert np.array_equal(res.y_residual[n], res.y_scatter[n] - res.x[n])


def _big(mode):
    from p2igan_bench.utils import seeded
    truths = [seeded.exp1_truth(600 + i, t, 160, 144) for i, t in enumerate((40, 60, 52))]
    keys = [f"event_{i + 1:02d}" for i in range(3)]
    spec = {"p2igan": (401, 10.0, 0.02, 0.01), "stdk": (402, 25.0, 0.05, 0.0), "idw": (403, 40.0, 0.0, 0.03)}
    preds = {name: {k: seeded.exp1_pred(s * 10 + i, g, n, z, 0.0, nan) for i, (k, g) in enumerate(zip(keys, truths))}
             for name, (s, n, z, nan) in spec.items()}
    mask = seeded.exp1_mask(78, 128, 128, 0.3 if mode == "radar" else 0.02)
    return preds, dict(zip(keys, truths)), mask


@pytest.mark.parametrize("mode", ["radar", "gauge"])
def test_bigger_case_matches_restatement(mode):
    from p2igan_bench.evaluation import compute_exp3
    preds, truth, mask = _big(mode)
    res = compute_exp3(preds, truth, mask, mode, 128)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = exp3_ref.exp3(preds, truth, mask, mode, 128)
    assert all(res.pool[n] > 2000 for n in res.methods) and res.pool == ref["pool"]      # sampling is active
    check_against_golden(as_ref_layout(res), as_golden_layout(ref), rel=1e-10, fit_tol=1e-12, exact_samples=False, exact_freq=True)


def test_carry_over_and_missing_events_match_restatement():
    """Shortened events before a full method and a missing event: the per-event and stack pairs differ (the second pass)."""
    from p2igan_bench.evaluation import compute_exp3
    preds, truth, mask = _big("radar")
    keys = list(truth)
    preds = {"short": {k: v[: [30, 60, 20][i]] for i, (k, v) in enumerate(preds["stdk"].items())},
             "full": preds["p2igan"], "gappy": {k: v for k, v in preds["idw"].items() if k != keys[1]}}
    res = compute_exp3(preds, truth, mask, "radar", 128)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = exp3_ref.exp3(preds, truth, mask, "radar", 128)
    assert res.pool == ref["pool"]
    check_against_golden(as_ref_layout(res), as_golden_layout(ref), rel=1e-10, fit_tol=1e-12, exact_samples=False, exact_freq=True)


def _bits(r):
    parts = [np.float64(v).tobytes() for v in r.metrics.values()]
    parts += [np.asarray(v, np.float64).tobytes() for v in r.nse_by_method.values()]
    for d in (r.x, r.y_scatter, r.freq):
        parts += [np.asarray(v).tobytes() for v in d.values()]
    parts += [np.float64(a).tobytes() for v in list(r.fit_scatter.values()) + list(r.fit_residual.values()) for a in v]
    return b"".join(parts)


def test_two_runs_are_bit_identical():
    from p2igan_bench.evaluation import compute_exp3
    preds, truth, mask = _big("gauge")
    assert _bits(compute_exp3(preds, truth, mask, "gauge", 128)) == _bits(compute_exp3(preds, truth, mask, "gauge", 128))


def test_dict_and_device_tensor_inputs_agree_bit_for_bit():
    from p2igan_bench.evaluation import Exp3Evaluator, compute_exp3
    preds, truth, mask = _big("radar")
    a = compute_exp3(preds, truth, mask, "radar", 128)
    dev = torch.device("cuda")
    b = compute_exp3({n: {k: torch.from_numpy(v).to(dev) for k, v in p.items()} for n, p in preds.items()},
                     {k: torch.from_numpy(v).to(dev) for k, v in truth.items()}, mask, "radar", 128)
    ev = Exp3Evaluator(mask, "radar", 128, list(preds))
    for k in truth:
        ev.add_event(truth[k], {n: p[k] for n, p in preds.items()})
    c = ev.compute()
    assert _bits(a) == _bits(b) == _bits(c)


def test_cli_exp3_end_to_end(tmp_path):
    from p2igan_bench.data import zarr_lite
    from p2igan_bench.evaluation import compute_exp3, crop_mask
    from p2igan_bench.utils import seeded
    truths = {f"event_{i + 1:02d}": seeded.exp1_truth(910 + i, t, 48, 40) for i, t in enumerate((9, 14))}
    g = zarr_lite.Group(str(tmp_path / "truth.zarr"), "w")
    for k, v in truths.items():
        g.create_dataset(k, v, chunks=v.shape)
    preds = {}
    for j, name in enumerate(("p2igan", "idw")):
        pg = zarr_lite.Group(str(tmp_path / f"{name}.zarr"), "w")
        preds[name] = {}
        for i, (k, v) in enumerate(truths.items()):
            p = seeded.exp1_pred(960 + 10 * j + i, v, 12.0 + 10 * j)
            pg.create_dataset(k, p, chunks=p.shape)
            preds[name][k] = p
    full = seeded.exp1_mask(6, 48, 40, 0.2)
    np.savetxt(tmp_path / "mask.txt", full.astype(np.float64), fmt="%d")
    cmd = [sys.executable, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts", "evaluate.py"), "--truth", str(tmp_path / "truth.zarr"),
           "--method", f"p2igan={tmp_path / 'p2igan.zarr'}", "--method", f"idw={tmp_path / 'idw.zarr'}", "--mask", str(tmp_path / "mask.txt"),
           "--mode", "radar", "--crop-size", "32"]
    r = subprocess.run(cmd + ["--output", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(cmd + ["--output", str(tmp_path / "with"), "--exp3", str(tmp_path / "e3")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    # exp1's outputs do not depend on the flag
    for f in ("metrics.json", "metrics.txt"):
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "with" / f).read_bytes(), f
    assert sorted(os.listdir(tmp_path / "plain")) == ["metrics.json", "metrics.txt"]
    e3 = tmp_path / "e3"
    assert sorted(os.listdir(e3)) == sorted(["metrics.json", "metrics.txt", "exp3_data.npz", "scatter_panels.pdf", "residual_panels.pdf",
                                             "nse_boxplot.pdf", "logfreq.pdf"])
    want = compute_exp3(preds, truths, crop_mask(full, 32), "radar", 32).metrics
    assert json.loads((e3 / "metrics.json").read_text()) == json.loads(json.dumps(want))
    assert (e3 / "metrics.txt").read_text() == "".join(f"{k}: {v:.6f}\n" for k, v in want.items())
