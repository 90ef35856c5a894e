"""The inputs of tests/metric_cases.py have the properties that test_metric_kernels_gpu.py relies on: every value keeps its margin
from every threshold (so the float64 contingency table is the only correct answer), every contingency cell is populated, the
integer regression sums and the power-of-two FSS sums are exact in float32 in any order, and every listed reason (block boundary,
second trip, scale larger than the field) is true of its case."""
import random

import numpy as np
import pytest
import torch

import metric_cases as mc


# ------------------------------------------------------------------------------------------------ pointwise
@pytest.mark.parametrize("thresholds", mc.THRESHOLD_SETS, ids=["nt4", "nt1"])
@pytest.mark.parametrize("n", mc.POINT_SIZES)
def test_pointwise_inputs_keep_the_margin_and_fill_every_cell(n, thresholds):
    p, t = mc.point_inputs(n, thresholds)
    assert p.shape == (n,) and p.dtype == torch.float32
    for x in (p, t):
        assert mc.margin_of(x) >= mc.MARGIN_HELD                 # against all four default thresholds, whichever set is asked
        assert float(x.min()) >= mc.X_LO and float(x.max()) <= mc.X_HI
    # 0.01 in x is a relative step of 10^(0.01/16) - 1 = 1.4e-3 in the rain rate: four orders above any powf rounding
    assert 1.4e-3 < 10 ** (mc.MARGIN / 16) - 1 < 1.5e-3
    table, bits = mc.point_expected(n, thresholds)
    assert table.sum(dim=1).tolist() == [n] * len(thresholds)
    if n >= 4 * len(thresholds):
        assert bool((table > 0).all())                           # all 4 * nt cells
        # ... and the planted pairs, which sit in the tail, alone already fill them
        k = 4 * len(thresholds)
        tail = torch.zeros_like(table)
        for j in range(len(thresholds)):
            pp, tt = (bits[n - k:] >> j) & 1, (bits[n - k:] >> (4 + j)) & 1
            tail[j] = torch.stack([(pp & tt).sum(), ((1 - pp) & tt).sum(), (pp & (1 - tt)).sum(), ((1 - pp) & (1 - tt)).sum()])
        assert bool((tail > 0).all())
        for (a, b), pv, tv in zip(mc.plants(thresholds), p[n - k:], t[n - k:]):
            assert float(pv) == np.float32(a) and float(tv) == np.float32(b)
    assert int(bits.max()) < (1 << 8) and (len(thresholds) == 4 or not bool((bits & 0xEE).any()))
    # the oracle's own float32 table agrees wherever it is evaluated on these inputs (nothing sits near a threshold)
    if n <= 4096:
        from oracle import metrics_oracle as mo
        assert torch.equal(mo.contingency(p, t, thresholds), table)


def test_pointwise_sizes_hit_the_planner_edges():
    assert [mc.point_blocks(n) for n in (1, 2047, 2048, 2049)] == [1, 1, 1, 2]          # the 2048-element block boundary
    assert [mc.point_trips(n) for n in (1, 255, 256, 257)] == [1, 1, 1, 2]              # second trip of a lone workgroup
    assert mc.point_blocks(mc.BIG_N) == mc.MAX_BLOCKS and mc.BIG_N > mc.MAX_BLOCKS * mc.BLOCK_ELEMS
    assert mc.point_trips(mc.BIG_N) == 9                         # past the 8 trips of a full grid: every workgroup goes round again
    assert mc.BIG_N % 256 != 0 and mc.BIG_N % mc.BLOCK_ELEMS != 0
    assert 2 * 4 * mc.BIG_N < 80e6                               # about 67 MB of inputs


@pytest.mark.parametrize("n", mc.POINT_SIZES)
def test_integer_regression_sums_are_exact(n):
    p, t = mc.integer_inputs(n)
    assert torch.equal(p, p.round()) and torch.equal(t, t.round())
    sa, sq = mc.integer_sums(n)
    assert 0 < sa < mc.EXACT / 2 and 0 < sq < mc.EXACT / 2       # two calls accumulate: twice the sums stay exact
    d = p - t
    if n > 4096:
        assert set(d.unique().tolist()) <= {0.0, 1.0, -1.0, 2.0, -2.0} and float(d[-1]) != 0
        assert float((d != 0).float().mean()) < 0.01
    # a sum of integers below 2^24 in float32, in a shuffled order, is the float64 sum
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    assert float(d.abs()[perm].sum(dtype=torch.float32)) == sa and float((d * d)[perm].sum(dtype=torch.float32)) == sq


def test_regression_reference_is_the_oracle_in_float64():
    from oracle import metrics_oracle as mo
    for n in (257, 2049):
        p, t = mc.point_inputs(n)
        _, _, mae, rmse = mc.regression_expected(n)
        o = mo.regression(p, t, True)                            # the oracle's float32 evaluation of the same lines
        assert abs(o["mae"] - mae) <= 1e-5 * mae and abs(o["rmse"] - rmse) <= 1e-5 * rmse


# ------------------------------------------------------------------------------------------------ FSS
@pytest.mark.parametrize("case", mc.FSS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fss_sums_are_exact_in_any_order(case):
    N, H, W = case
    assert mc.fss_small_exact_bound(case)                        # 2 N (H+1) (W+1) <= 4096: exact for every scale <= 8
    for nt in mc.FSS_NT:
        b = mc.fss_bits(case, nt)
        assert b.shape == case and b.dtype == torch.uint8
        used = sum(1 << k for k in range(nt)) * 0x11
        assert not bool((b & ~used & 0xFF).any())
        for scales in mc.FSS_SCALE_LISTS:
            num, den = mc.fss_expected(case, nt, scales)
            assert bool((num <= den).all())
            if max(scales) <= 8:
                assert mc.fss_exact(case, nt, scales)
                assert bool((den * 4096 == (den * 4096).round()).all()) and float(den.max()) <= 2 * mc.fss_positions(case)
    # random order, float32, on the case itself (all default scales, the widest threshold set)
    b = mc.fss_bits(case, 4)
    num, den = mc.fss_expected(case, 4, mc.SCALES)
    rnd = random.Random(3)
    for si, s in enumerate(mc.SCALES):
        pm = (b & 1).double().reshape(N, 1, H, W)
        tm = ((b >> 4) & 1).double().reshape(N, 1, H, W)
        fp = torch.nn.functional.avg_pool2d(pm, s, 1, s // 2).float().reshape(-1)
        ft = torch.nn.functional.avg_pool2d(tm, s, 1, s // 2).float().reshape(-1)
        add_n, add_d = ((fp - ft) * (fp - ft)).tolist(), (fp * fp + ft * ft).tolist()
        order = list(range(len(add_n)))
        rnd.shuffle(order)
        sn = sd = np.float32(0)
        for j in order:
            sn, sd = np.float32(sn + np.float32(add_n[j])), np.float32(sd + np.float32(add_d[j]))
        assert float(sn) == float(num[0, si]) and float(sd) == float(den[0, si])


def test_fss_reasons_hold():
    N, H, W = (1, 3, 5)
    assert all(s > H or s > W for s in mc.SCALES if s >= 4) and 64 > max(max(c[1:]) for c in mc.FSS_CASES)
    assert [mc.out_extent(20, s) for s in (1, 2, 3, 4, 8, 64)] == [20, 21, 20, 21, 21, 21]      # H + 1 for even scales, H for odd
    assert mc.fss_positions(mc.FSS_STRIDE_CASE) == 2162688 > mc.FSS_GRID
    assert all(mc.fss_positions(c) <= 8 * 256 for c in mc.FSS_CASES)              # at most 8 workgroups: the odd-scale bound's premise
    assert max(len(s) for s in mc.FSS_SCALE_LISTS) == mc.MAX_SCALE and max(mc.FSS_NT) == mc.MAX_THR
    # scale 64: exact where the sums stay below 2^24 * 2^-24, else the rounding bound applies; both kinds occur
    kinds = {mc.fss_exact(c, nt, (64,)) for c in mc.FSS_CASES for nt in mc.FSS_NT}
    assert kinds == {True, False}
    assert mc.fss_exact((1, 1, 1), 1, (64,)) and mc.fss_exact((1, 3, 5), 4, (64,))


def test_fss_stride_case_is_sparse_and_exact():
    N, H, W = mc.FSS_STRIDE_CASE
    b = mc.fss_bits(mc.FSS_STRIDE_CASE, 4)
    for plane in range(8):
        per_frame = ((b >> plane) & 1).reshape(N, -1).sum(dim=1)
        assert int(per_frame.max()) <= mc.FSS_STRIDE_PIXELS and int(per_frame.min()) > 0
    last = b[N - 1]
    assert int(last[H - 1, W - 1]) == 0xFF and bool(last[H - 1].any()) and bool(last[:, W - 1].any())
    assert mc.fss_exact(mc.FSS_STRIDE_CASE, 4, mc.SCALES)
    num, den = mc.fss_expected(mc.FSS_STRIDE_CASE, 4, mc.SCALES)
    assert bool((den > 0).all()) and bool((num > 0).all())


def test_fss_even_scale_extent_matters():
    """the sums over H x W instead of (H+1) x (W+1) differ on the cases: an off-by-one in the even-scale extent cannot pass"""
    case = (2, 20, 28)
    N, H, W = case
    b = mc.fss_bits(case, 1)
    _, den = mc.fss_expected(case, 1, (2,))
    pm = (b & 1).double().reshape(N, 1, H, W)
    tm = ((b >> 4) & 1).double().reshape(N, 1, H, W)
    fp = torch.nn.functional.avg_pool2d(pm, 2, 1, 1)[..., :H, :W]
    ft = torch.nn.functional.avg_pool2d(tm, 2, 1, 1)[..., :H, :W]
    assert float((fp ** 2 + ft ** 2).sum()) != float(den[0, 0])


def test_class_inputs():
    p, t = mc.class_inputs()
    assert p.shape == mc.CLASS_SHAPE and mc.margin_of(p) >= mc.MARGIN_HELD and mc.margin_of(t) >= mc.MARGIN_HELD
    table, _ = mc.point_expected(p.numel())
    assert bool((table > 0).all())
