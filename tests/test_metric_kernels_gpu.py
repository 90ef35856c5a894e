"""Shape sweep of the evaluation-metric kernels (csrc/metrics.hip), called directly the way metrics/metric.py calls them, and through
the metric classes.  Contingency counts, the threshold bit plane, the integer regression sums and the power-of-two FSS sums are
compared EXACTLY: the inputs of tests/metric_cases.py keep a margin of 0.01 in x (1.4e-3 in the rain rate, four orders above any powf
rounding) from every threshold, resp. are chosen so that every float32 sum is exact in any order -- under both endings of the
cross-workgroup sums.  test_metric_cases_cpu.py checks those properties on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import metric_cases as mc

pytestmark = pytest.mark.gpu

POISON = 12345.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from p2igan_bench import ops as o
    o._hip.load()
    return o


@pytest.fixture(params=["det", "atomic"])
def reduce(request, ops):
    """How the cross-workgroup sums end: "det" = partials in the registered scratch, added in a fixed order (the default);
    "atomic" = the scratch unregistered for the test, the kernels fall back to float atomics."""
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.det_ready(dev)
    orig = ops._DET[dev.index]
    if request.param == "det":
        if orig is None:
            raise RuntimeError("the deterministic scratch is not registered (P2I_DETERMINISTIC=0?)")
        yield "det"
        return
    lib = ops._hip.load()
    torch.cuda.synchronize()
    ops._hip.check(lib.p2i_det_workspace(None, 0, None, 0), "p2i_det_workspace")
    ops._DET[dev.index] = None
    try:
        yield "atomic"
    finally:
        torch.cuda.synchronize()
        if orig is not None:
            ops._hip.check(lib.p2i_det_workspace(orig[0].data_ptr(), orig[0].numel(), orig[1].data_ptr(), orig[1].numel()), "p2i_det_workspace")
        ops._DET[dev.index] = orig


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pointwise(ops, p, t, thresholds, apply_transform, sums, counts, bits):
    thr = (ctypes.c_float * len(thresholds))(*thresholds) if thresholds else None
    rc = ops._hip.load().p2i_metrics_pointwise(p.data_ptr(), t.data_ptr(), p.numel(), thr, len(thresholds), int(apply_transform),
                                               sums.data_ptr(), None if counts is None else counts.data_ptr(),
                                               None if bits is None else bits.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc


def _fss(ops, bits, case, nt, scales, num, den):
    N, H, W = case
    sc = (ctypes.c_int * len(scales))(*scales)
    rc = ops._hip.load().p2i_metrics_fss(bits.data_ptr(), N, H, W, nt, sc, len(scales), num.data_ptr(), den.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def big(ops):
    """the large pointwise inputs on the device, uploaded once"""
    p, t = mc.point_inputs(mc.BIG_N)
    ip, it = mc.integer_inputs(mc.BIG_N)
    return {"x": (p.cuda(), t.cuda()), "int": (ip.cuda(), it.cuda())}


def _dev(big, kind, n, thresholds=mc.THRESHOLDS):
    if n == mc.BIG_N and thresholds == mc.THRESHOLDS:
        return big[kind]
    a, b = mc.point_inputs(n, thresholds) if kind == "x" else mc.integer_inputs(n)
    return a.cuda(), b.cuda()


# ------------------------------------------------------------------------------------------------ pointwise: counts and bit plane
@pytest.mark.parametrize("thresholds", mc.THRESHOLD_SETS, ids=["nt4", "nt1"])
@pytest.mark.parametrize("n", mc.POINT_SIZES)
def test_contingency_counts_and_bit_plane_exact(ops, big, reduce, n, thresholds):
    nt = len(thresholds)
    table, ebits = mc.point_expected(n, thresholds)
    p, t = _dev(big, "x", n, thresholds)
    ops.det_ready(p.device)
    sums = torch.zeros(2, device="cuda")
    counts = torch.zeros(4 * nt + 4, device="cuda", dtype=torch.int64)            # one guard row behind the table
    bits = torch.full((n + 64,), 0xA5, device="cuda", dtype=torch.uint8)          # 64 guard bytes behind the plane
    assert _pointwise(ops, p, t, thresholds, 1, sums, counts, bits) == 0
    assert counts[:4 * nt].cpu().view(nt, 4).tolist() == table.tolist()
    assert torch.equal(bits[:n].cpu(), ebits)                                    # every byte
    assert bool((bits[n:] == 0xA5).all()) and not bool(counts[4 * nt:].any())
    # counts are ADDED to by a second call; without a bit plane the counts are the same
    assert _pointwise(ops, p, t, thresholds, 1, sums, counts, None) == 0
    assert counts[:4 * nt].cpu().view(nt, 4).tolist() == (2 * table).tolist()
    if thresholds != mc.THRESHOLDS:
        return
    # regression sums of the same pass against float64
    sa, sq, _, _ = mc.regression_expected(n)
    got = sums.double().cpu() / 2
    print("pointwise", n, reduce, "sum|d|", float(got[0]), sa, "sum d^2", float(got[1]), sq)
    mae, rmse = float(got[0]) / n, float(np.sqrt(float(got[1]) / n))
    assert abs(mae - sa / n) <= 2e-4 * max(1.0, sa / n)
    assert abs(rmse - np.sqrt(sq / n)) <= 2e-4 * max(1.0, np.sqrt(sq / n))


# ------------------------------------------------------------------------------------------------ pointwise: regression sums
@pytest.mark.parametrize("n", mc.POINT_SIZES)
def test_untransformed_regression_sums_exact(ops, big, reduce, n):
    """apply_transform = 0 on integer-valued inputs: every partial sum is an integer below 2^24, the result is exact whatever
    the order; nt = 0 with counts = NULL and thresholds = NULL is RegressionMetrics' call"""
    p, t = _dev(big, "int", n)
    ops.det_ready(p.device)
    sa, sq = mc.integer_sums(n)
    sums = torch.zeros(4, device="cuda")
    sums[2:] = POISON
    assert _pointwise(ops, p, t, (), 0, sums, None, None) == 0
    assert sums.cpu().tolist() == [sa, sq, POISON, POISON]
    assert _pointwise(ops, p, t, (), 0, sums, None, None) == 0                    # sums2 is added to
    assert sums.cpu().tolist() == [2 * sa, 2 * sq, POISON, POISON]


@pytest.mark.parametrize("n", mc.POINT_SIZES)
def test_transformed_regression_matches_float64(ops, big, reduce, n):
    from p2igan_bench.metrics import RegressionMetrics
    p, t = _dev(big, "x", n)
    _, _, mae, rmse = mc.regression_expected(n)
    m = RegressionMetrics(apply_transform=True).to("cuda")
    m.update(p.view(1, -1), t.view(1, -1))               # the classes take (..., H, W)
    out = m.compute()
    print("regression", n, reduce, out, mae, rmse)
    assert abs(out["mae"] - mae) <= 2e-4 * max(1.0, abs(mae)) and abs(out["rmse"] - rmse) <= 2e-4 * max(1.0, abs(rmse))
    if n <= 4096:
        ip, it = _dev(big, "int", n)
        m = RegressionMetrics(apply_transform=False).to("cuda")
        m.update(ip.view(1, -1), it.view(1, -1))
        sa, sq = mc.integer_sums(n)
        assert m.sums.cpu().tolist() == [sa, sq]


def test_pointwise_refusals_leave_the_outputs_untouched(ops):
    p, t = (x.cuda() for x in mc.point_inputs(257))
    sums = torch.full((2,), POISON, device="cuda")
    counts = torch.full((20,), 77, device="cuda", dtype=torch.int64)
    bits = torch.full((257,), 0xA5, device="cuda", dtype=torch.uint8)
    lib = ops._hip.load()
    assert _pointwise(ops, p, t, (0.5, 1.0, 2.0, 4.0, 8.0), 1, sums, counts, bits) != 0            # nt = 5
    thr = (ctypes.c_float * 4)(*mc.THRESHOLDS)
    assert lib.p2i_metrics_pointwise(p.data_ptr(), t.data_ptr(), 0, thr, 4, 1, sums.data_ptr(), counts.data_ptr(), bits.data_ptr(), _stream()) != 0
    assert lib.p2i_metrics_pointwise(p.data_ptr(), t.data_ptr(), 257, thr, 4, 1, sums.data_ptr(), None, bits.data_ptr(), _stream()) != 0
    torch.cuda.synchronize()
    assert bool((sums == POISON).all()) and bool((counts == 77).all()) and bool((bits == 0xA5).all())


# ------------------------------------------------------------------------------------------------ FSS
def _fss_check(got_n, got_d, num, den, exact, what):
    gn, gd = got_n.double().cpu(), got_d.double().cpu()
    if exact:
        assert torch.equal(gn, num) and torch.equal(gd, den), (what, (gn - num).abs().max(), (gd - den).abs().max())
    else:
        en, ed = (gn - num).abs(), (gd - den).abs()
        print("fss", what, "err/den", float((en / den.clamp_min(1e-300)).max()), float((ed / den.clamp_min(1e-300)).max()))
        assert bool((en <= mc.FSS_ODD_BOUND * den).all()) and bool((ed <= mc.FSS_ODD_BOUND * den).all()), what


@pytest.mark.parametrize("scales", mc.FSS_SCALE_LISTS, ids=lambda s: "s" + "_".join(map(str, s)))
@pytest.mark.parametrize("nt", mc.FSS_NT)
@pytest.mark.parametrize("case", mc.FSS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fss_sums_exact(ops, reduce, case, nt, scales):
    """Power-of-two scales: exact in any order (metric_cases.fss_exact).  The one combination family where the sums outgrow 2^24
    units -- scale 64 on the fields of several hundred pixels, addends multiples of 2^-24 -- is held to the rounding bound of the odd
    scales instead (derived at test_fss_odd_scales)."""
    ns = len(scales)
    num, den = mc.fss_expected(case, nt, scales)
    exact = mc.fss_exact(case, nt, scales)
    assert exact or scales == (64,)
    bits = torch.cat([mc.fss_bits(case, nt).reshape(-1), torch.full((64,), 0xFF, dtype=torch.uint8)]).cuda()    # set guard bytes behind the planes
    ops.det_ready(bits.device)
    nd = torch.zeros(2, nt * ns + 4, device="cuda")
    assert _fss(ops, bits, case, nt, scales, nd[0], nd[1]) == 0
    _fss_check(nd[0, :nt * ns].view(nt, ns), nd[1, :nt * ns].view(nt, ns), num, den, exact, (case, nt, scales, reduce))
    assert not bool(nd[:, nt * ns:].any())
    if exact and float(den.max()) * max(scales) ** 4 * 2 < mc.EXACT:             # num / den are ADDED to by a second call
        assert _fss(ops, bits, case, nt, scales, nd[0], nd[1]) == 0
        _fss_check(nd[0, :nt * ns].view(nt, ns), nd[1, :nt * ns].view(nt, ns), 2 * num, 2 * den, True, (case, nt, scales, reduce, "twice"))


@pytest.mark.parametrize("case", mc.FSS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fss_odd_scales(ops, reduce, case):
    """Odd scales: 1.0f / (s * s) rounds, the sums are not exact.  Bound |err| <= 32 * 2^-24 * den for num and den alike: an addend
    carries at most 5 roundings relative to fp^2 + ft^2 (the reciprocal, two products count * inv, the squares and their sum; the
    error of (fp - ft)^2 is bounded by the same multiple of fp^2 + ft^2).  The sum: one addend per thread (at most 8 workgroups hold
    every position, no second trip), block_sum of common.h adds 6 butterfly levels and then the 4 wave sums serially (10 additions in
    a chain, not the 8 of a pure tree), and at most 8 workgroup partials are added by det_reduce or by atomics: 18 roundings, each at
    most 2^-24 of a partial sum <= den.  5 + 18 = 23 < 32."""
    nt, scales = 4, mc.FSS_ODD_SCALES
    num, den = mc.fss_expected(case, nt, scales)
    bits = mc.fss_bits(case, nt).cuda()
    ops.det_ready(bits.device)
    nd = torch.zeros(2, nt, len(scales), device="cuda")
    assert _fss(ops, bits, case, nt, scales, nd[0], nd[1]) == 0
    _fss_check(nd[0], nd[1], num, den, False, (case, reduce))


def test_fss_second_grid_stride_trip_exact(ops, reduce):
    case, nt, scales = mc.FSS_STRIDE_CASE, 4, mc.SCALES
    num, den = mc.fss_expected(case, nt, scales)
    bits = mc.fss_bits(case, nt).cuda()
    ops.det_ready(bits.device)
    nd = torch.zeros(2, nt, len(scales), device="cuda")
    assert _fss(ops, bits, case, nt, scales, nd[0], nd[1]) == 0
    _fss_check(nd[0], nd[1], num, den, True, (case, reduce))


@pytest.mark.parametrize("what,nt,scales,N", [("nt5", 5, (1, 2), 2), ("ns5", 4, (1, 2, 4, 8, 16), 2), ("scale0", 4, (1, 0), 2),
                                              ("scale65", 4, (65,), 2), ("N0", 4, (1, 2), 0)], ids=["nt5", "ns5", "scale0", "scale65", "N0"])
def test_fss_refusals_leave_the_outputs_untouched(ops, what, nt, scales, N):
    bits = mc.fss_bits((2, 20, 28), 4).cuda()
    nd = torch.full((2, 32), POISON, device="cuda")
    assert _fss(ops, bits, (N, 20, 28), nt, scales, nd[0], nd[1]) != 0
    assert len(ops._hip.load().p2i_last_error()) > 0
    assert bool((nd == POISON).all())


# ------------------------------------------------------------------------------------------------ class level
def test_metric_classes_match_the_oracle(ops):
    from oracle import metrics_oracle as mo
    from p2igan_bench.metrics import MetricConfig, RainfallMetricSuite
    from p2igan_bench.metrics.metric import CategoricalMetrics, FractionalSkillScoreMetric
    p, t = mc.class_inputs()
    pg, tg = p.cuda(), t.cuda()
    table, ebits = mc.point_expected(p.numel())
    want_cat = mo.categorical_scores(table, mc.THRESHOLDS)
    want_fss = mo.fss(p, t, mc.THRESHOLDS, mc.SCALES)
    assert torch.equal(mo.contingency(p, t, mc.THRESHOLDS), table)

    cat = CategoricalMetrics(mc.THRESHOLDS).to("cuda")
    cat.update(pg, tg)
    assert cat.counts.cpu().view(4, 4).tolist() == table.tolist()
    got = cat.compute()
    assert sorted(got) == sorted(want_cat)
    for k, v in want_cat.items():
        assert abs(got[k] - v) <= 1e-9, (k, got[k], v)             # the counts are exact

    f = FractionalSkillScoreMetric(mc.THRESHOLDS, mc.SCALES).to("cuda")
    f.update(pg, tg)
    assert np.allclose(f.score_sum.cpu().numpy(), want_fss.numpy(), rtol=2e-4, atol=2e-5)
    # the bit plane of one pointwise call, handed in: the same score bits as letting update() compute it
    bits = torch.empty(p.numel(), device="cuda", dtype=torch.uint8)
    assert _pointwise(ops, pg, tg, mc.THRESHOLDS, 1, torch.zeros(2, device="cuda"), torch.zeros(16, device="cuda", dtype=torch.int64), bits) == 0
    assert torch.equal(bits.cpu(), ebits)
    f2 = FractionalSkillScoreMetric(mc.THRESHOLDS, mc.SCALES).to("cuda")
    f2.update(pg, tg, bits=bits)
    assert torch.equal(f2.score_sum, f.score_sum)

    suite = RainfallMetricSuite(MetricConfig()).to("cuda")
    suite.update(pg, tg)
    out = suite.compute()
    assert suite.categorical.counts.cpu().view(4, 4).tolist() == table.tolist()
    for k, v in want_cat.items():
        assert abs(out[k] - v) <= 1e-9, (k, out[k], v)
    for ti, thr in enumerate(mc.THRESHOLDS):
        for si, s in enumerate(mc.SCALES):
            assert np.isclose(out[f"fss_thr{thr:.2f}_s{s}"], float(want_fss[ti, si]), rtol=2e-4, atol=2e-5)
    _, _, mae, rmse = mc.regression_expected(p.numel())
    assert abs(out["mae"] - mae) <= 2e-4 * max(1.0, mae) and abs(out["rmse"] - rmse) <= 2e-4 * max(1.0, rmse)
