"""The evaluation kernels' input view and dtype dispatch on the MI355X (csrc/eval_common.h Crop<T>, dispatch1 / dispatch2): every
(prediction dtype, truth dtype) pair of uint8 / f32 / f64 through run_exp1 and compute_exp3, every dtype through ops.exp2_index, with
a prediction and a truth of different H and W, so that the two crop origins differ and neither is (0, 0).  The shapes are the
smallest at which an address or a dispatch slip shows: crop 8 and 9 of [3, 11, 13] against [3, 9, 12] (9 leaves partial pooling
cells), crop 67 of [2, 70, 69] against [2, 67, 71] (a crop row spans two 64-lane rounds of exp3's row counter), crop 7 of [3, 11, 13].
The arbiters are the numpy restatements (tests/exp1_ref.py, exp3_ref.py, exp2_ref.py) under the existing GPU tests' comparison rules.

The device pow is a few ulp from numpy's on f32 / f64 inputs, so equal counts, pools and indices are only fair where no transformed
value sits on a cut: every test first asserts, on the host, that its float inputs keep the margins the fixtures record."""
import functools
import warnings

import numpy as np
import pytest
import torch

import exp1_ref
import exp2_ref
import exp3_ref
from p2igan_bench.utils import seeded
from test_exp1_gpu import assert_device_matches
from test_exp3_cpu import check_against_golden
from test_exp3_gpu import as_golden_layout, as_ref_layout

pytestmark = pytest.mark.gpu
KINDS = ("u8", "f32", "f64")
THRESHOLDS = (0.5, 2.0, 4.0, 8.0)


# name -> (seed, the common field's [T, H, W], the prediction's and the truth's window (row0, rows, column0, columns) of it): the
# windows are placed so that the two center crops cover the same pixels of the field (at crop 9: one column apart)
FIELDS = {"small": (8100, (3, 11, 13), (0, 11, 0, 13), (1, 9, 0, 12)),          # crop 8: origins (1, 2) and (0, 2); 9: (1, 2), (0, 1)
          "large": (8500, (2, 70, 71), (0, 70, 1, 69), (1, 67, 0, 71))}         # crop 67: origins (1, 1) and (0, 2)


@functools.lru_cache(maxsize=None)
def field(name, side, kind, nan=0.0):
    """[T, 1, h, w] from the seeded generators: the side's window of the common uint8 field (the truth as it is, the prediction
    through noise), or a float field near it with exact zeros and values past the scale (and NaN when asked); the f64 one is
    shifted by 1e-7 so that its values are no float32 values."""
    seed, (t, H, W), pwin, gwin = FIELDS[name]
    r0, h, c0, w = pwin if side == "pred" else gwin
    base = np.ascontiguousarray(seeded.exp1_truth(seed, t, H, W)[:, :, r0:r0 + h, c0:c0 + w])
    if kind == "u8" and side == "truth":
        return base
    noise, salt = (8.0, 1) if side == "pred" else (2.0, 2)
    if kind == "u8":
        return np.clip(np.rint(seeded.exp1_pred(seed + salt, base, noise)), 0, 255).astype(np.uint8)
    p = seeded.exp1_pred(seed + salt, base, noise, 0.03, 0.03, nan)
    return p if kind == "f32" else p.astype(np.float64) + 1e-7


def assert_clear_of_cuts(golden, *arrays):
    """No transformed float value closer to a categorical threshold or to the 0.5 / 0.1 cuts (relative) than the smallest
    thr_margin of exp1_cases.npz, to a colour-table bound (relative) than the same, or to a log-frequency bin edge (absolute) than
    the smallest edge_margin of exp3_cases.npz (the 6.7e-6 of DESIGN.md section 11).  uint8 inputs go through numpy's own table."""
    g1, g3 = golden("exp1_cases.npz"), golden("exp3_cases.npz")
    rel = min(float(g1[k]) for k in g1.files if k.endswith("/thr_margin"))
    edge = min(float(g3[k]) for k in g3.files if k.endswith("/edge_margin"))
    assert 2e-6 < rel < 1e-5 and 6e-6 < edge < 1e-5
    cuts = np.array(sorted({0.1, 0.5, *THRESHOLDS}))
    bounds = exp2_ref.cmap_tables()[0]
    for a in arrays:
        if a.dtype == np.uint8:
            continue
        v = exp1_ref.transform(a).ravel()
        v = v[np.isfinite(v)]
        assert (np.abs(v[:, None] - cuts) / cuts).min() >= rel
        inside = v[v <= 32.0]
        assert (np.abs(inside * 2.0 - np.rint(inside * 2.0)) / 2.0).min() >= edge
        v = v[(v > 0.0) & (v < 200.0)]                         # the clip's own constants are exact on both sides
        assert (np.abs(v[:, None] - bounds) / np.maximum(bounds, 1e-300)).min() >= rel


@pytest.mark.parametrize("gk", KINDS)
@pytest.mark.parametrize("pk", KINDS)
def test_run_exp1_over_every_dtype_pair(golden, pk, gk):
    from p2igan_bench.evaluation import run_exp1
    pred, truth = field("small", "pred", pk), field("small", "truth", gk)
    assert_clear_of_cuts(golden, pred, truth)
    for crop, mode in ((8, "radar"), (9, "gauge")):
        mask = seeded.exp1_mask(8300 + crop, crop, crop, 0.3)
        for pool8 in (True, False):
            kw = {"mode": mode, "crop_size": crop, "thresholds": THRESHOLDS, "use_pool8": pool8}
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = exp1_ref.flatten(exp1_ref.run_exp1({"m": pred}, truth, mask, **kw))
            assert_device_matches(exp1_ref.flatten(run_exp1({"m": pred}, truth, mask, **kw)), want)


def check_exp3(res, ref, truth_kind):
    """check_against_golden under test_exp3_gpu's settings.  It holds the observed samples to equality where the truth is uint8
    (numpy's own table on both sides); a float truth goes through the device pow as the predictions do, so its samples are held
    to the predictions' rule (rtol 1e-12)."""
    assert res.pool == ref["pool"]
    check_against_golden(as_ref_layout(res), as_golden_layout(ref), rel=1e-10, fit_tol=1e-12, exact_samples=False, exact_freq=True,
                         exact_x=truth_kind == "u8")


def run_exp3(golden, preds, truth, crop, truth_kind):
    from p2igan_bench.evaluation import compute_exp3
    assert_clear_of_cuts(golden, truth["event_01"], *(p["event_01"] for p in preds.values()))
    mask = seeded.exp1_mask(8400 + crop, crop, crop, 0.3)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = exp3_ref.exp3(preds, truth, mask, "radar", crop)
    check_exp3(compute_exp3(preds, truth, mask, "radar", crop), ref, truth_kind)
    return ref


@pytest.mark.parametrize("gk", KINDS)
def test_compute_exp3_over_every_dtype_pair(golden, gk):
    """One method per prediction dtype against a truth of dtype gk: accumulate, truth_hist and gather of every pair."""
    preds = {pk: {"event_01": field("small", "pred", pk, 0.0 if pk == "u8" else 0.02)} for pk in KINDS}
    ref = run_exp3(golden, preds, {"event_01": field("small", "truth", gk)}, 8, gk)
    assert all(0 < n <= 3 * 64 for n in ref["pool"].values())


def test_compute_exp3_crop_row_of_two_lane_rounds(golden):
    """Crop 67: columns 64 .. 66 of every crop row fall in the row counter's second round; the pool is sampled."""
    preds = {"m": {"event_01": field("large", "pred", "f64", 0.02)}}
    ref = run_exp3(golden, preds, {"event_01": field("large", "truth", "f32")}, 67, "f32")
    assert ref["pool"]["m"] > 2000 and ref["x"]["m"].size == 2000


@pytest.mark.parametrize("kind", KINDS)
def test_exp2_index_over_every_dtype(golden, kind):
    from p2igan_bench import ops
    from p2igan_bench.evaluation import crop_origin, paper_cmap, truth_lut
    base = seeded.exp1_truth(8700, 3, 11, 13)
    x = np.ascontiguousarray((base if kind == "u8" else exp2_ref._floaty(8701, base, kind))[:, 0])
    assert_clear_of_cuts(golden, x)
    tl = crop_origin(11, 13, 7)
    assert tl == (2, 3)
    dev = torch.device("cuda")
    out = torch.empty(3, 7, 7, device=dev, dtype=torch.uint8)
    ops.exp2_index(torch.from_numpy(x).to(dev), tl, 7, 3, torch.from_numpy(paper_cmap()[0]).to(dev),
                   torch.from_numpy(truth_lut(True)).to(dev), True, out)
    want = exp2_ref.index(x[:, tl[0]:tl[0] + 7, tl[1]:tl[1] + 7])
    assert np.array_equal(out.cpu().numpy(), want)
    assert kind == "u8" or (want == exp2_ref.BAD).any()
