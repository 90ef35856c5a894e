#!/usr/bin/env python3
"""Generate tests/golden/exp1_cases.npz by running the GENUINE reference's experiments.exp1.run_exp1 on CPU.

Run where a checkout of the reference is at hand:  python tests/golden/make_golden_exp1.py REFERENCE_ROOT
experiments/exp1.py and experiments/io.py import numpy and torch only (checked below: neither xarray nor zarr is loaded).  The
inputs are rebuilt from the recipes in tests/exp1_ref.py (numpy-only generators of p2igan_bench.utils.seeded), so the fixture
holds recipe parameters and the reference's outputs only: per case ``<case>/recipe`` (JSON), ``<case>/<method>/<KEY>`` and
``<case>/<method>/CAT_<thr>/<SUB>`` (float64), or ``<case>/error`` (the reference's exception, ``Type: message``).  It also records
``<case>/thr_margin``: the smallest relative distance of a transformed value of the selection to a threshold (the contingency
counts are exact when it is well above 1e-12).
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) != 2:
    sys.exit("usage: make_golden_exp1.py REFERENCE_ROOT")
REF = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, "p2i-gan-benchmark_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exp1_ref  # noqa: E402

sys.path.insert(0, REF)
from experiments.exp1 import run_exp1, transform_mmhr  # noqa: E402

assert not any(m.split(".")[0] in ("xarray", "zarr") for m in sys.modules), "the reference's exp1 pulled in xarray / zarr"


def margin(preds, truth, mask, kw):
    vals = []
    for src in list(preds.values()) + [truth]:
        for a in (src.values() if isinstance(src, dict) else [src]):
            v = transform_mmhr(a).ravel()
            vals.append(v[np.isfinite(v)])
    v = np.concatenate(vals)
    return min(float(np.min(np.abs(v - t) / t)) for t in kw["thresholds"])


def main():
    out = {}
    for c in exp1_ref.CASES:
        preds, truth, mask, kw = exp1_ref.build_case(c)
        out[f"{c['name']}/recipe"] = np.array(exp1_ref.recipe_json(c))
        out[f"{c['name']}/thr_margin"] = np.float64(margin(preds, truth, mask, kw))
        try:
            res = run_exp1(preds, truth, mask, **kw, divide_by_3=True)
        except Exception as e:          # recorded: the device path must raise the same
            out[f"{c['name']}/error"] = np.array(f"{type(e).__name__}: {e}")
            print(c["name"], "raises", type(e).__name__, e)
            continue
        for k, v in exp1_ref.flatten(res).items():
            out[f"{c['name']}/{k}"] = np.float64(v)
        print(c["name"], {k: round(v, 6) for k, v in list(exp1_ref.flatten(res).items())[:7]})
    path = os.path.join(ROOT, "tests", "golden", "exp1_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
