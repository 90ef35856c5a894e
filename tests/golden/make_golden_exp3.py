#!/usr/bin/env python3
"""Generate tests/golden/exp3_cases.npz by running the GENUINE reference's experiments.exp3.run_exp3 on CPU.

Run where a checkout of the reference is at hand:  python tests/golden/make_golden_exp3.py REFERENCE_ROOT
(needs matplotlib and scipy, which the reference's exp3 imports).  The inputs are rebuilt from the recipes in tests/exp3_ref.py
(numpy-only generators of p2igan_bench.utils.seeded), so the fixture holds recipe parameters and the reference's outputs only.
Besides the returned metrics, the reference's figure functions are observed while they run: the ``nse_by_method`` handed to
``_nse_boxplot``, the ``(x, y)`` of every ``Axes.scatter`` panel and the ``stats.linregress`` results of both panel figures, and
the frequencies handed to ``Axes.semilogy``.  Per case:
    <case>/recipe (JSON), <case>/metrics/<name>, <case>/nse/<name>, <case>/x/<name>, <case>/y/<name> (the scatter panel's
    points), <case>/fit_scatter/<name> and <case>/fit_residual/<name> (slope, intercept, r), <case>/freq_truth,
    <case>/freq/<name>; or <case>/error (``Type: message``).  The residual panel's x equals the scatter panel's and its y equals y - x bit for bit (checked here).
<case>/edge_margin is the smallest distance of a float-transformed value to a 0.5-multiple bin edge, <case>/min_margin the smallest
relative distance of any transformed value to 0.1: the device pow is within a few ulp of numpy's, so pools and bins are exact when
these are well above 1e-12.
"""
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) != 2:
    sys.exit("usage: make_golden_exp3.py REFERENCE_ROOT")
REF = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, "p2i-gan-benchmark_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exp3_ref  # noqa: E402

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import matplotlib.axes  # noqa: E402

sys.path.insert(0, REF)
import experiments.exp3 as ref_exp3  # noqa: E402
from experiments.exp1 import transform_mmhr  # noqa: E402

LOG = {}


def _observe():
    """Wrap the reference's figure functions and the matplotlib / scipy calls inside them; records into LOG."""
    orig_scatter, orig_semilogy = matplotlib.axes.Axes.scatter, matplotlib.axes.Axes.semilogy
    stats = ref_exp3.stats

    def scatter(self, x, y, *a, **k):
        LOG.setdefault(LOG["fig"] + "_xy", []).append((np.array(x, np.float64), np.array(y, np.float64)))
        return orig_scatter(self, x, y, *a, **k)

    def semilogy(self, x, y, *a, **k):
        LOG.setdefault("freq", []).append((k.get("label"), np.array(y, np.float64)))
        return orig_semilogy(self, x, y, *a, **k)

    class Stats:
        @staticmethod
        def linregress(x, y):
            r = stats.linregress(x, y)
            LOG.setdefault(LOG["fig"] + "_fit", []).append((r.slope, r.intercept, r.rvalue))
            return r

    def tagged(fn, tag):
        def run(*a, **k):
            LOG["fig"] = tag
            return fn(*a, **k)
        return run

    box = ref_exp3._nse_boxplot

    def boxplot(nse_by_method, out_path):
        LOG["nse"] = {k: list(v) for k, v in nse_by_method.items()}
        return box(nse_by_method, out_path)

    matplotlib.axes.Axes.scatter = scatter
    matplotlib.axes.Axes.semilogy = semilogy
    ref_exp3.stats = Stats
    ref_exp3._scatter_multi_row = tagged(ref_exp3._scatter_multi_row, "scatter")
    ref_exp3._residual_multi_row = tagged(ref_exp3._residual_multi_row, "residual")
    ref_exp3._nse_boxplot = boxplot


def margins(preds, truth):
    edge, rel = [np.inf], [np.inf]
    for src in list(preds.values()) + [truth]:
        for a in (src.values() if isinstance(src, dict) else [src]):
            v = transform_mmhr(a).ravel()
            v = v[np.isfinite(v)]
            if not v.size:
                continue
            rel.append(float(np.min(np.abs(v - 0.1) / 0.1)))
            if np.asarray(a).dtype != np.uint8:          # uint8 goes through numpy's own table on the device
                inside = v[v <= 32.0]
                if inside.size:
                    edge.append(float(np.min(np.abs(inside * 2.0 - np.rint(inside * 2.0)) / 2.0)))
    return min(edge), min(rel)


def main():
    _observe()
    out = {}
    for c in exp3_ref.CASES:
        name = c["name"]
        preds, truth, mask, kw = exp3_ref.build_case(c)
        out[f"{name}/recipe"] = np.array(exp3_ref.recipe_json(c))
        em, rm = margins(preds, truth)
        out[f"{name}/edge_margin"], out[f"{name}/min_margin"] = np.float64(em), np.float64(rm)
        LOG.clear()
        LOG["fig"] = "none"
        try:
            with tempfile.TemporaryDirectory() as td, np.errstate(all="ignore"):
                res = ref_exp3.run_exp3(preds, truth, mask, out_dir=td, **kw)
        except Exception as e:          # recorded: the device path must raise the same
            out[f"{name}/error"] = np.array(f"{type(e).__name__}: {e}")
            print(name, "raises", type(e).__name__, e)
            continue
        names = list(preds)
        for n in names:
            out[f"{name}/metrics/{n}"] = np.float64(res[f"NSE_{n}"])
        if "nse" in LOG:
            for n in names:
                out[f"{name}/nse/{n}"] = np.array(LOG["nse"][n], np.float64)
        sc, rs = LOG.get("scatter_xy", []), LOG.get("residual_xy", [])
        assert len(sc) == len(rs) == (len(names) if sc else 0), name
        fits_s, fits_r = iter(LOG.get("scatter_fit", [])), iter(LOG.get("residual_fit", []))
        for n, (x, y), (xr, yr) in zip(names, sc, rs):
            assert np.array_equal(x, xr) and np.array_equal(yr, y - x), (name, n)
            out[f"{name}/x/{n}"], out[f"{name}/y/{n}"] = x, y
            if x.size >= 2:
                out[f"{name}/fit_scatter/{n}"] = np.array(next(fits_s), np.float64)
                out[f"{name}/fit_residual/{n}"] = np.array(next(fits_r), np.float64)
        for label, y in LOG.get("freq", []):
            out[f"{name}/freq_truth" if label == "Obs" else f"{name}/freq/{label}"] = y
        print(name, {k: round(v, 6) for k, v in res.items()}, "samples", [x.size for x, _ in sc])
    path = os.path.join(ROOT, "tests", "golden", "exp3_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
