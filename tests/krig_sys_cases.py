"""Cases of tests/test_krig_sys_gpu.py and tests/test_krig_sys_cases_cpu.py: the dense kriging family
(csrc/classical.hip, krig_uq.hip, krig_cs.hip, stkrig.hip, stkrig_loso.hip) where the other kriging tests never take it -- more than
one chunk of systems per call (models/classical.py _Systems: f0 > 0, a chunk-local status / sol / work / winv next to call-wide cand,
alpha, mean, var, pred, ens), a factorisation that fails, and a shared gauge set of more than 8 frames.  numpy only: inputs come from
seeded generators, the references are the fp64 / fp32 restatements of classical_ref, krig_uq_ref, krig_cs_ref, stkriging_ref and
stkriging_loso_ref.  Everything returned is built once and never modified.

  inputs        B x T, frame    gauges per frame (systems)                                      what it is for
  perframe      3 x 3, 24 x 40  5 31 33 | 40 64 12 (equal values) | 33 0 64                     one system per frame, np = 64
  shared        5 x 3, 24 x 40  31 | 33 | 0 | 40 (equal values) | 64, one set per sample        one system per sample, np = 64
  st            5 x 3, 24 x 40  3 2 0 | 11 10 10 | 11 11 11 | 14 13 13 (equal values) | 22 21 21  space-time, one system per sample
  pivot-frames  1 x 8, 40 x 40  8 / 43, 40, 43, 64, 67, 5, 33, 67 (the +3: the adjacent triple)   failed systems among healthy ones
  pivot-shared  2 x 3, 40 x 40  43 | 40                                                         a failed sample next to a healthy one
  pivot-st      3 x 2, 40 x 40  40 5 | 40 5+3 | 33 5                                            a failed space-time sample, tile 1
  wide          1 x {9, 17}, 24 x 40, 20 gauges                                                 krig_predict_kernel's blockIdx.z > 0"""
import functools

import numpy as np

import classical_ref as cr
import krig_cs_ref as cs
import krig_uq_ref as ur
import stkriging_loso_ref as sl
import stkriging_ref as sr

TILE = 32
RC = 8                            # frames of one shared set per workgroup of krig_predict_kernel (csrc/classical.hip)
SEED = (5 << 32) | 23             # ensemble seed of every case
EMBED = 2
SENTINEL = 0x4B1D5EED             # the bit pattern (a finite float, 1.03e7) that call-wide outputs hold before a stage-level call


def round_up(v, m):
    return (v + m - 1) // m * m


# ---- models/classical.py _Systems, restated
def per_of(nsys, np_, inverse, factor_bytes, limit=None):
    per = max(1, min(nsys, factor_bytes // (np_ * np_ * 4 * (2 if inverse else 1))))
    if limit is not None:
        per = max(1, min(per, limit))
    return per


def chunk_list(nsys, per):
    """[(first system, systems)] of _Systems.chunks()."""
    return [(s0, min(per, nsys - s0)) for s0 in range(0, nsys, per)]


def factor_bytes_for(per, np_, inverse):
    """The _FACTOR_BYTES at which the factor bound gives `per` systems a chunk."""
    return per * np_ * np_ * 4 * (2 if inverse else 1)


def ensemble_bounds(factor_bytes, nsys, np_, r, members, cap):
    """(systems the factor bound allows, systems forward_ensemble's limit allows) at this _FACTOR_BYTES."""
    return factor_bytes // (np_ * np_ * 8), factor_bytes // (r * members * cap * 4)


def ensemble_bytes_for(per, r, members, cap):
    """The _FACTOR_BYTES at which forward_ensemble's limit is `per`."""
    return per * r * members * cap * 4


# ---- seeded inputs
def field(t, h, w, seed):
    """(t, h, w) fp32 in (0.2, 1): a smooth field that moves from frame to frame plus texture."""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.empty((t, h, w), np.float32)
    for i in range(t):
        out[i] = 0.55 + 0.3 * np.sin(0.37 * yy + 0.2 * i + seed) * np.cos(0.29 * xx - 0.3 * i) + 0.1 * rng.random((h, w))
    return out


H, W = 24, 40                     # H W = 960 is no multiple of the 256 pixels of a predictor workgroup
PERFRAME_COUNTS = ((5, 31, 33), (40, 64, 12), (33, 0, 64))
SHARED_COUNTS = (31, 33, 0, 40, 64)
ST_COUNTS = ((3, 2, 0), (11, 10, 10), (11, 11, 11), (14, 13, 13), (22, 21, 21))
FLAT = {"perframe": 1, "shared": 3, "st": 3}          # the sample whose gauges all hold one value (a degenerate fit); never sample 0


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(masked, masks) (B, T, 1, H, W) fp32 of an input set."""
    if name.startswith("pivot"):
        return _pivot_inputs(name)
    if name.startswith("wide"):
        t = int(name[4:])
        masks = np.zeros((1, t, 1, H, W), np.float32)
        masks.reshape(t, -1)[:, np.random.default_rng(41).permutation(H * W)[:20]] = 1.0
        return (field(t, H, W, 9).reshape(masks.shape) * masks).astype(np.float32), masks
    counts = {"perframe": PERFRAME_COUNTS, "shared": tuple((n,) * 3 for n in SHARED_COUNTS), "st": ST_COUNTS}[name]
    b, t = len(counts), len(counts[0])
    rng = np.random.default_rng({"perframe": 7, "shared": 8, "st": 9}[name])
    masks = np.zeros((b, t, 1, H, W), np.float32)
    for i in range(b):
        perm = rng.permutation(H * W)
        for j in range(t):
            if name == "perframe":
                idx = rng.permutation(H * W)[:counts[i][j]]
            elif name == "shared":
                idx = perm[:counts[i][j]]
            else:                                      # overlapping windows: most sites hold more than one frame
                idx = perm[2 * j:2 * j + counts[i][j]]
            masks[i, j, 0].reshape(-1)[idx] = 1.0
    frames = np.stack([field(t, H, W, 10 * i + len(name)) for i in range(b)]).reshape(b, t, 1, H, W)
    masked = frames * masks
    masked[FLAT[name]] = 0.4 * masks[FLAT[name]]
    return masked.astype(np.float32), masks


def counts_of(masks):
    return (masks != 0).reshape(masks.shape[0], masks.shape[1], -1).sum(-1)


def streams_of(b, t, tag=3):
    """(B, T) int64 stream ids with a non-zero high word."""
    return (np.arange(b * t, dtype=np.int64).reshape(b, t) + 5) | (np.int64(tag) << 32)


# ---- section A: chunk invariance at the model level.  id: (model config, input, entry points); r = T where the sample's frames share
# their set, else 1; the kriging models take max_points = 4096 (cap = 4096) so that forward_ensemble's limit can decide the chunk
FIT = {"model": "exponential", "fit": True, "n_lags": 8}
FIT_SPH = {"model": "spherical", "fit": True, "n_lags": 8}
ST_FIT = {"model": "exponential", "fit": True, "n_lags": 8, "n_tlags": 2}
KRIG_ENTRIES = ("forward", "forward_uq", "cross_validate", "ensemble1", "ensemble3")
ST_ENTRIES = ("forward", "cross_validate_sites")
CAP_A = 4096
CHUNK_CASES = {
    "krig-perframe": ({"name": "kriging", "variogram": FIT, "max_points": CAP_A}, "perframe", KRIG_ENTRIES),
    "krig-shared": ({"name": "kriging", "variogram": FIT_SPH, "max_points": CAP_A}, "shared", KRIG_ENTRIES),
    "krig-unshared": ({"name": "kriging", "variogram": FIT_SPH, "max_points": CAP_A, "share_sets": False}, "shared", KRIG_ENTRIES),
    "stkrig": ({"name": "stkriging", "variogram": ST_FIT}, "st", ST_ENTRIES),
    "lagkrig": ({"name": "lagkriging", "variogram": ST_FIT, "advection": {"fit": False, "vy": 0.5, "vx": -0.25}}, "st", ST_ENTRIES),
}


def chunk_case_ids():
    return [f"{c}-{e}" for c, (_, _, entries) in CHUNK_CASES.items() for e in entries]


def systems_of(cid):
    """(nsys, r, np_, T) of a chunk case, from the inputs alone."""
    model, name, _ = CHUNK_CASES[cid]
    cnt = counts_of(inputs(name)[1])
    b, t = cnt.shape
    if model["name"] != "kriging":
        return b, 1, max(TILE, round_up(int(cnt.sum(1).max()), TILE)), t
    r = t if (name == "shared" and model.get("share_sets", True)) else 1
    return b * t // r, r, max(TILE, round_up(int(cnt.max()), TILE)), t


def chunk_plan(cid, entry):
    """[(per, the _FACTOR_BYTES that gives it, 'factor' or 'limit': the bound that decides)] for per in {1, 2, nsys - 1}."""
    nsys, r, np_, _ = systems_of(cid)
    out = []
    for per in sorted({1, 2, nsys - 1}):
        if entry.startswith("ensemble"):
            members = int(entry[8:])
            fb = ensemble_bytes_for(per, r, members, CAP_A)
            by_factor, by_limit = ensemble_bounds(fb, nsys, np_, r, members, CAP_A)
            if by_limit < by_factor:
                out.append((per, fb, "limit"))
                continue                               # else (one member, one frame, np = 64: 16 KiB against 32 KiB) the factor bound decides
        fb = factor_bytes_for(per, np_, entry != "forward")
        by = "factor"
        if entry.startswith("ensemble"):               # r M = 3 at per = 1: the limit is 0 there and the clamp to 1 decides
            by_factor, by_limit = ensemble_bounds(fb, nsys, np_, r, int(entry[8:]), CAP_A)
            by = "limit" if by_limit < by_factor else "factor"
        out.append((per, fb, by))
    return out


def planned_per(cid, entry, fb):
    nsys, r, np_, _ = systems_of(cid)
    limit = fb // (r * int(entry[8:]) * CAP_A * 4) if entry.startswith("ensemble") else None
    return per_of(nsys, np_, entry != "forward", fb, limit)


# ---- section B: stage-level calls of a sub-range.  Fixed parameters that differ from sample to sample (params[b] is read with the
# call-wide sample index)
STAGE_CASES = {
    # id: (input, model, R = T?, first system, systems, (nugget, psill, range) per sample)
    "perframe-r1": ("perframe", "exponential", False, 2, 5, ((0.002, 0.05, 6.0), (0.001, 0.04, 9.0), (0.004, 0.06, 5.0))),
    "shared-rT": ("shared", "spherical", True, 1, 3, ((0.001, 0.05, 10.0), (0.002, 0.04, 8.0), (0.001, 0.05, 7.0), (0.003, 0.06, 12.0),
                                                      (0.001, 0.05, 9.0))),
}
ST_STAGE = ("st", "exponential", 1, 3, ((0.002, 0.05, 6.0, 2.0), (0.001, 0.04, 9.0, 1.0), (0.004, 0.06, 5.0, 4.0), (0.002, 0.05, 7.0, 2.0),
                                        (0.001, 0.05, 8.0, 1.4)))
STAGE_MEMBERS = 3
STAGE_CAP, STAGE_NP = 96, 64      # cap > np: a row of alpha / pix / z is longer than a system


def f32(params):
    return tuple(float(np.float32(p)) for p in params)


def _solutions(xy, z, params, model, dtype):
    """(u = K^-1 1, v = K^-1 z) of a gauge set in dtype."""
    import scipy.linalg
    K = cr.covariance(xy, xy, *params, model, dtype)
    cf = scipy.linalg.cho_factor(K, lower=True)
    return scipy.linalg.cho_solve(cf, np.ones(len(z), dtype)), scipy.linalg.cho_solve(cf, z.astype(dtype))


def krig_stage_reference(masked, masks, model, params, members, streams, cap, np_, dtype):
    """Everything the per-frame stages leave behind, per frame, in dtype: pred, var (F, HW), ens (F, members, HW), loo_pred, loo_var,
    alpha (F, cap; zero past the count), mean (F,), u, v (F, np_; zero past the count).  Frame rules as on the device: no gauges give
    pred 0, alpha 0, mean 0 and NaN var / ens; fewer than 2 gauges give NaN LOO."""
    dt = np.dtype(dtype).type
    B, T, _, h, w = masked.shape
    F, HW = B * T, h * w
    out = {"pred": np.zeros((F, HW), dt), "var": np.full((F, HW), np.nan, dt), "ens": np.full((F, members, HW), np.nan, dt),
           "loo_pred": np.zeros((F, cap), dt), "loo_var": np.zeros((F, cap), dt), "alpha": np.zeros((F, cap), dt), "mean": np.zeros(F, dt),
           "u": np.zeros((F, np_), dt), "v": np.zeros((F, np_), dt)}
    for b in range(B):
        p = f32(params[b])
        A = cs.spectrum(p, model, h, w, EMBED)[0]
        for t in range(T):
            f = b * T + t
            xy, z = cr.gauges(masked[b, t, 0], masks[b, t, 0])
            n = len(z)
            if n == 0:
                continue
            out["pred"][f] = cr.krige_frame(xy, z, h, w, p, model, dt).ravel()
            out["var"][f] = ur.variance_frame(xy, h, w, p, model, dt)[0].ravel()
            out["ens"][f] = cs.members_frame(xy, z, h, w, p, model, members, SEED, int(streams[b, t]), EMBED, dt, A).reshape(members, HW)
            lp, lv = ur.loo_frame(xy, z, p, model, dt) if n >= 2 else (np.full(n, np.nan, dt),) * 2
            out["loo_pred"][f, :n], out["loo_var"][f, :n] = lp, lv
            u, v = _solutions(xy, z, p, model, dt)
            m = v.sum() / u.sum()
            out["u"][f, :n], out["v"][f, :n], out["mean"][f], out["alpha"][f, :n] = u, v, m, v - m * u
    return out


@functools.lru_cache(maxsize=None)
def stage_reference(cid, dtype_name):
    name, model, _, _, _, params = STAGE_CASES[cid]
    masked, masks = inputs(name)
    b, t = masked.shape[:2]
    return krig_stage_reference(masked, masks, model, params, STAGE_MEMBERS, streams_of(b, t), STAGE_CAP, STAGE_NP, dtype_name)


def st_stage_reference(masked, masks, model, params, dtype, fcap):
    """Leave-one-site-out of every sample with its own fixed (nugget, psill, range, kappa): (pred, var) (F, fcap), zero past the count."""
    dt = np.dtype(dtype).type
    B, T = masked.shape[:2]
    pred, var = np.zeros((B * T, fcap), dt), np.zeros((B * T, fcap), dt)
    for b in range(B):
        xy, tt, z = sr.points(masked[b], masks[b])
        p, v = sl.block_loo(xy, tt, z, f32(params[b]), model, sl.site_index(xy), dt)
        for t in range(T):
            at = tt == t
            pred[b * T + t, :at.sum()], var[b * T + t, :at.sum()] = p[at], v[at]
    return pred, var


@functools.lru_cache(maxsize=None)
def st_reference(dtype_name):
    name, model, _, _, params = ST_STAGE
    masked, masks = inputs(name)
    return st_stage_reference(masked, masks, model, params, dtype_name, STAGE_CAP)


def st_sample_counts(masks):
    return counts_of(masks).sum(1)


# ---- section C: a factorisation that fails by a wide margin in fp32 and fp64 alike.  Spherical, range 4, psill 0.05 and a nugget of
# -0.5 psill (ops takes it in a params tensor; a model's config refuses it).  `npre` gauges on a 5-pixel grid over rows 0 .. 35 are
# mutually uncorrelated (distance >= 5 > range) with diagonal psill + nugget = 0.5 psill; three adjacent gauges in row 39, four rows
# (exactly one range) below the grid, have C(1) = 0.633 psill between neighbours: the second of them meets the pivot 0.5 psill -
# (0.633 psill)^2 / (0.5 psill) = -0.30 psill, at index npre + 1.
PH = PW = 40
PSILL = 0.05
BAD = (-0.5 * PSILL, PSILL, 4.0)                      # (nugget, psill, range)
BENIGN = (0.1 * PSILL, PSILL, 4.0)
PIVOT_MODEL = "spherical"
TRIPLE = ((39, 10), (39, 11), (39, 12))
PIVOT_NPRE = (5, 40, 64)                              # first bad pivot at 6, 41, 65: tiles 0, 1, 2
# pivot-frames: (grid gauges, with the triple) of each frame; np = 96.  Failed systems first, in the middle and last of the call, and
# first and in the middle of the sub-range 2 .. 5
PIVOT_FRAMES = ((5, True), (40, False), (40, True), (64, False), (64, True), (5, False), (33, False), (64, True))
PIVOT_SUB = (2, 4)
PIVOT_NP, PIVOT_CAP = 96, 128
PIVOT_KAPPA = 8.0                                     # time_scale > range: the frames of a space-time sample decouple
PIVOT_ST = (((40, False), (5, False)), ((40, False), (5, True)), ((33, False), (5, False)))      # bad pivot at 40 + 6 = 46: tile 1


def pivot_mask(npre, triple):
    m = np.zeros((PH, PW), np.float32)
    grid = [(y, x) for y in range(0, 36, 5) for x in range(0, 36, 5)]
    for y, x in grid[:npre] + (list(TRIPLE) if triple else []):
        m[y, x] = 1.0
    return m


def _pivot_inputs(name):
    if name == "pivot-frames":
        masks = np.stack([pivot_mask(*f) for f in PIVOT_FRAMES])[None, :, None]
    elif name == "pivot-frames-healthy":              # the healthy frames of pivot-frames alone, in order
        masked, masks = inputs("pivot-frames")
        keep = pivot_healthy()
        return np.ascontiguousarray(masked[:, keep]), np.ascontiguousarray(masks[:, keep])
    elif name == "pivot-shared":
        masks = np.stack([np.stack([pivot_mask(40, True)] * 3), np.stack([pivot_mask(40, False)] * 3)])[:, :, None]
    elif name == "pivot-shared-healthy":
        masked, masks = inputs("pivot-shared")
        return np.ascontiguousarray(masked[1:]), np.ascontiguousarray(masks[1:])
    elif name == "pivot-table":                       # three samples on the grid-and-triple set; sample 1 holds one value
        masks = np.stack([np.stack([pivot_mask(40, True)] * 2)] * 3)[:, :, None]
    elif name == "pivot-st":
        masks = np.stack([np.stack([pivot_mask(*f) for f in s]) for s in PIVOT_ST])[:, :, None]
    else:
        raise KeyError(name)
    b, t = masks.shape[:2]
    frames = np.stack([field(t, PH, PW, 50 + i) for i in range(b)]).reshape(b, t, 1, PH, PW)
    masked = frames * masks
    if name == "pivot-table":
        masked[1] = 0.4 * masks[1]
    return masked.astype(np.float32), masks.astype(np.float32)


def pivot_healthy():
    return [i for i, (_, tr) in enumerate(PIVOT_FRAMES) if not tr]


def pivot_status():
    return [int(tr) for _, tr in PIVOT_FRAMES]


def elimination(K, dtype):
    """Plain right-looking elimination of K in dtype up to its first pivot that is not > 0: (index of that pivot or -1, the pivots met,
    that one included)."""
    A = np.array(K, dtype=dtype)
    piv = []
    for j in range(len(A)):
        p = A[j, j]
        piv.append(float(p))
        if not p > 0:
            return j, piv
        col = (A[j + 1:, j] / np.sqrt(p)).astype(dtype)
        A[j + 1:, j + 1:] = (A[j + 1:, j + 1:] - np.outer(col, col).astype(dtype)).astype(dtype)
    return -1, piv


def gauge_means(masked, masks):
    """(B, T) fp64 gauge mean of every frame (0 without gauges)."""
    m = (masks != 0).astype(np.float64)
    return ((masked.astype(np.float64) * m).sum((-1, -2, -3)) / np.maximum(m.sum((-1, -2, -3)), 1.0))
