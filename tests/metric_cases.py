"""Case tables, seeded input builders and float64 restatements for the shape sweep of the evaluation-metric kernels
(csrc/metrics.hip): test_metric_kernels_gpu.py runs them on the GPU, test_metric_cases_cpu.py checks on the CPU that the inputs have
the properties the exact comparisons rely on (the margin around every threshold, non-empty contingency cells, integer sums below
2^24, FSS sums that are exact in any order).  Everything here is torch / numpy on the CPU and a function of the case alone."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
EXACT = 1 << 24

THRESHOLDS = (0.5, 2.0, 4.0, 8.0)          # MetricConfig's defaults
THRESHOLD_SETS = [THRESHOLDS, (4.0,)]
SCALES = (1, 2, 4, 8)
MAX_THR = MAX_SCALE = 4

X_LO, X_HI = 0.0, 45.0
MARGIN = 0.01               # distance in x that every value is given from every threshold's pre-image
MARGIN_HELD = 0.0099        # what survives the float32 rounding of x near 40 (half an ulp: 2e-6)


def x_of(thr):
    """pre-image of a rain rate under 10^(x/16) * 0.036"""
    return 16.0 * math.log10(thr / 0.036)


def rate64(x):
    return torch.pow(torch.tensor(10.0, dtype=F64), x.to(F64) * 0.0625) * 0.036


# ------------------------------------------------------------------------------------------------ pointwise pass
BLOCK_ELEMS = 2048          # p2i_metrics_pointwise: ceil(n / 2048) workgroups of 256 threads, at most 4096
MAX_BLOCKS = 4096
POINT_SIZES = [1, 255, 256, 257, 2047, 2048, 2049, 4096 * 2048 + 2053]
BIG_N = POINT_SIZES[-1]


def point_blocks(n):
    return min(-(-n // BLOCK_ELEMS), MAX_BLOCKS)


def point_trips(n):
    """grid-stride trips of the first thread"""
    return -(-n // (point_blocks(n) * 256))


def _push(x, thresholds):
    """every value closer than MARGIN to a pre-image is moved to that distance on its own side (nothing is filtered)"""
    for thr in thresholds:
        c = x_of(thr)
        d = x - c
        near = d.abs() < MARGIN
        x = torch.where(near, torch.where(d >= 0, torch.full_like(x, c + MARGIN), torch.full_like(x, c - MARGIN)), x)
    return x


def plants(thresholds):
    """(pred, target) pairs at x_thr -+ MARGIN: for every threshold the four combinations hit / miss / false alarm / correct negative"""
    out = []
    for thr in thresholds:
        c = x_of(thr)
        for sp, st in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            out.append((c + sp * MARGIN, c + st * MARGIN))
    return out


@functools.lru_cache(maxsize=None)
def point_inputs(n, thresholds=THRESHOLDS):
    """float32 pred, target of n elements in x-space.  The planted pairs sit in the TAIL (as many as fit)."""
    g = torch.Generator().manual_seed(17 + n % 1000 + len(thresholds))
    p = _push((torch.rand(n, generator=g, dtype=F64) * (X_HI - X_LO) + X_LO), THRESHOLDS)
    t = _push((torch.rand(n, generator=g, dtype=F64) * (X_HI - X_LO) + X_LO), THRESHOLDS)
    pl = plants(thresholds)[:n]
    for j, (a, b) in enumerate(pl):
        p[n - len(pl) + j], t[n - len(pl) + j] = a, b
    return p.float(), t.float()


def margin_of(x, thresholds=THRESHOLDS):
    """smallest distance in x of any value from any pre-image, in float64 on the float32 values"""
    return min(float((x.to(F64) - x_of(thr)).abs().min()) for thr in thresholds)


@functools.lru_cache(maxsize=None)
def point_expected(n, thresholds=THRESHOLDS):
    """float64 contingency table (nt, 4) int64 [hits, misses, false alarms, correct negatives] and the bit plane (uint8)"""
    p, t = point_inputs(n, thresholds)
    rp, rt = rate64(p), rate64(t)
    bits = torch.zeros(n, dtype=torch.uint8)
    table = torch.zeros(len(thresholds), 4, dtype=torch.int64)
    for k, thr in enumerate(thresholds):
        pp, tt = rp >= thr, rt >= thr
        table[k] = torch.stack([(pp & tt).sum(), (~pp & tt).sum(), (pp & ~tt).sum(), (~pp & ~tt).sum()])
        bits |= (pp.to(torch.uint8) << k) | (tt.to(torch.uint8) << (4 + k))
    return table, bits


@functools.lru_cache(maxsize=None)
def regression_expected(n):
    """float64 (sum |d|, sum d^2, mae, rmse) of the transformed point_inputs(n): oracle.metrics_oracle.regression's lines in float64"""
    from oracle import metrics_oracle as mo
    p, t = point_inputs(n)
    d = mo.transform(p.to(F64)) - mo.transform(t.to(F64))
    return float(d.abs().sum()), float((d ** 2).sum()), float(d.abs().sum() / n), float(torch.sqrt((d ** 2).sum() / n))


@functools.lru_cache(maxsize=None)
def integer_inputs(n):
    """integer-valued pred, target for apply_transform = 0 with sum |d| and sum d^2 below 2^24.  Small n: values in [-8, 8].  The
    large n: target in [0, 40], pred = target + d with d in {+-1, +-2} on a seeded sparse set (1 in 128) and 0 elsewhere."""
    g = torch.Generator().manual_seed(23 + n % 1000)
    if n <= 4096:
        return (torch.randint(-8, 9, (n,), generator=g).float(), torch.randint(-8, 9, (n,), generator=g).float())
    t = torch.randint(0, 41, (n,), generator=g).float()
    d = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (n,), generator=g)]
    d = torch.where(torch.randint(0, 128, (n,), generator=g) == 0, d, torch.zeros(()))
    d[-1] = 2.0                                    # the tail belongs to the sum
    return t + d, t


def integer_sums(n):
    p, t = integer_inputs(n)
    d = (p - t).to(F64)
    return float(d.abs().sum()), float((d * d).sum())


# ------------------------------------------------------------------------------------------------ FSS
FSS_CASES = [(1, 1, 1), (3, 1, 7), (2, 7, 1), (1, 3, 5), (2, 20, 28), (4, 8, 8), (1, 31, 33)]        # (N, H, W)
FSS_NT = [1, 4]
FSS_SCALE_LISTS = [(1,), (2,), (8,), (1, 2, 4, 8), (64,)]
FSS_ODD_SCALES = (3, 5, 7)
FSS_STRIDE_CASE = (33, 255, 255)       # 33 * 256 * 256 = 2 162 688 positions > 8192 * 256: a second grid-stride trip
FSS_STRIDE_PIXELS = 16                 # set pixels per frame and plane in that case
FSS_GRID = 8192 * 256
FSS_DENSITY = 0.3
FSS_ODD_BOUND = 32 * 2.0 ** -24        # |err| <= this * den for the scales whose 1 / s^2 rounds (see test_metric_kernels_gpu.py)


def fss_positions(case):
    N, H, W = case
    return N * (H + 1) * (W + 1)


def out_extent(n, s):
    """the reference's avg_pool2d(kernel s, stride 1, padding s // 2) output extent: n + 1 for even s, n for odd"""
    return n + 2 * (s // 2) - s + 1


@functools.lru_cache(maxsize=None)
def fss_bits(case, nt):
    """byte plane (N, H, W): bit k = pred plane of threshold k, bit 4 + k = target plane; bits at density 0.3, built directly"""
    N, H, W = case
    g = torch.Generator().manual_seed(31 + 7 * N + 3 * H + W + nt)
    if case == FSS_STRIDE_CASE:
        b = torch.zeros(N, H * W, dtype=torch.uint8)
        for plane in list(range(nt)) + [4 + k for k in range(nt)]:
            for n in range(N):
                idx = torch.randint(0, H * W, (FSS_STRIDE_PIXELS,), generator=g)
                if n == N - 1:
                    idx[0], idx[1], idx[2] = H * W - 1, (H - 1) * W + 5, 7 * W + W - 1     # last row and last column of the last frame
                b[n, idx] |= 1 << plane                                     # (repeated indices: fewer than 16 pixels, still at most 16)
        return b.reshape(N, H, W)
    b = torch.zeros(N, H, W, dtype=torch.uint8)
    for plane in list(range(nt)) + [4 + k for k in range(nt)]:
        b |= (torch.rand(N, H, W, generator=g) < FSS_DENSITY).to(torch.uint8) << plane
    return b


@functools.lru_cache(maxsize=None)
def fss_expected(case, nt, scales):
    """float64 (num, den), each (nt, ns): sums of (fp - ft)^2 and fp^2 + ft^2 over the reference's own output extent"""
    N, H, W = case
    b = fss_bits(case, nt)
    num = torch.zeros(nt, len(scales), dtype=F64)
    den = torch.zeros(nt, len(scales), dtype=F64)
    for k in range(nt):
        pm = ((b >> k) & 1).to(F64).reshape(N, 1, H, W)
        tm = ((b >> (4 + k)) & 1).to(F64).reshape(N, 1, H, W)
        for si, s in enumerate(scales):
            fp = F.avg_pool2d(pm, kernel_size=s, stride=1, padding=s // 2, count_include_pad=True)
            ft = F.avg_pool2d(tm, kernel_size=s, stride=1, padding=s // 2, count_include_pad=True)
            assert fp.shape[-2:] == (out_extent(H, s), out_extent(W, s))
            num[k, si] = ((fp - ft) ** 2).sum()
            den[k, si] = (fp ** 2 + ft ** 2).sum()
    return num, den


def fss_exact(case, nt, scales):
    """True when float32 sums of the addends are exact in ANY order.  For a power-of-two scale s every fraction is a multiple of
    s^-2, so every addend is a non-negative multiple of q = s^-4 (and a float32 value: a window holds at most min(s^2, H W) <= 4096
    pixels, the squared count has at most 24 bits).  A sum of non-negative multiples of q is exact in any order while the TOTAL stays
    below 2^24 q, and num <= den term by term: den / q < 2^24 decides."""
    if any(s & (s - 1) for s in scales):
        return False
    _, den = fss_expected(case, nt, scales)
    return all(float(den[:, si].max()) * s ** 4 < EXACT for si, s in enumerate(scales))


def fss_small_exact_bound(case):
    """the bound for scales <= 8: addends are multiples of 2^-12 and at most 2, so 2 * positions <= 4096 suffices"""
    return 2 * fss_positions(case) <= 4096


# ------------------------------------------------------------------------------------------------ class level
CLASS_SHAPE = (2, 3, 20, 28)


@functools.lru_cache(maxsize=None)
def class_inputs():
    n = int(np.prod(CLASS_SHAPE))
    p, t = point_inputs(n)
    return p.reshape(CLASS_SHAPE), t.reshape(CLASS_SHAPE)
