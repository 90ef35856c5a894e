"""numpy / scipy restatement of Lagrangian space-time kriging (p2igan_bench/models/classical.py LagrangianKrigingGenerator, DESIGN.md
section 19) on top of stkriging_ref.py: the velocity score and weight tables and the choice among them, the variogram bins on the
advected spatial distance, the fit (stkriging_ref.fit_st, unchanged), the dual-form predictor with the distance
    d = sqrt((dy - v_y dt)^2 + (dx - v_x dt)^2 + kappa^2 dt^2)
and leave-one-site-out through stkriging_loso_ref.  `dtype` selects the arithmetic of the kriging part (float64: the reference of the
GPU tests; float32: the yardstick of their error bound); the velocity estimate and the variogram are float64 always, as on the device.
Also the seeded generator of translating fields that the tests of the method's skill run on."""
import math

import numpy as np
import scipy.linalg

import classical_ref as cr
import stkriging_loso_ref as lr
import stkriging_ref as sr

ADVECTION = {"fit": True, "vmax": 4.0, "vstep": 0.5, "n_tlags": 3, "bandwidth": 1.5}
# the translating fields of the tests (32 x 32, 40 gauges, 8 frames): tag -> (true velocity, seed); the seeds were chosen once so that
# the restatement holds test_lagkriging_cpu.py's bounds with room, and are kept
CASES = {"down-left": ((2.5, -1.5), 3), "up-right": ((-2.0, 2.0), 0), "right": ((0.0, 3.0), 0), "rest": ((0.0, 0.0), 3)}
MOVING = ("down-left", "up-right", "right")
FITTED = {"model": "exponential", "fit": True, "n_lags": 16, "n_tlags": 3}


def nhalf_of(vmax, vstep):
    return int(math.floor(vmax / vstep + 0.5))


# ---- velocity estimate
def score_tables(frames, n_tlags, nhalf, vstep, r0):
    """frames: list of (xy, z) per frame.  (W, S, N) [n, n], n = 2 nhalf + 1, entry [i + nhalf, j + nhalf] for v = (i, j) vstep: over the
    pairs (a in frame t, b in frame t + u), 1 <= u <= min(n_tlags, T - 1), w = exp(-|x_b - x_a - v u|^2 / (2 r0^2)), W = sum w,
    S = sum w (z_a - z_b)^2 / 2 (not yet divided by W), N = sum w over the pairs of distinct pixels."""
    n = 2 * nhalf + 1
    grid = np.arange(-nhalf, nhalf + 1, dtype=np.float64) * vstep
    W, S, N = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for u in range(1, min(n_tlags, len(frames) - 1) + 1):
        for t in range(len(frames) - u):
            (xa, za), (xb, zb) = frames[t], frames[t + u]
            if len(za) == 0 or len(zb) == 0:
                continue
            d = xb[None, :, :].astype(np.float64) - xa[:, None, :].astype(np.float64)
            g = 0.5 * (za.astype(np.float64)[:, None] - zb.astype(np.float64)[None, :]) ** 2
            ey = d[:, :, 0, None] - grid * u
            ex = d[:, :, 1, None] - grid * u
            w = np.exp(-(ey[:, :, :, None] ** 2 + ex[:, :, None, :] ** 2) / (2.0 * r0 * r0))
            W += w.sum((0, 1))
            S += (w * g[:, :, None, None]).sum((0, 1))
            N += (w * ((d * d).sum(-1) > 0)[:, :, None, None]).sum((0, 1))
    return W, S, N


def score_of(W, S):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(W > 0, S / np.where(W > 0, W, 1.0), np.inf)


def pick(W, S, N):
    """((i, j), gap): the eligible candidate (N >= N(0) / 2) of the smallest score, ties to the smaller i^2 + j^2, then to the lower
    (i, j); gap = (runner-up's score - the best) / |best| among the eligible ones (inf with one candidate, nan when both are inf)."""
    n = W.shape[0]
    nhalf = n // 2
    score = score_of(W, S)
    ii, jj = np.meshgrid(np.arange(-nhalf, nhalf + 1), np.arange(-nhalf, nhalf + 1), indexing="ij")
    ok = (N >= 0.5 * N[nhalf, nhalf]).ravel()
    idx = np.flatnonzero(ok)
    order = idx[np.lexsort((idx, (ii * ii + jj * jj).ravel()[idx], score.ravel()[idx]))]
    best = order[0]
    if len(order) == 1:
        gap = np.inf
    else:
        s0, s1 = np.sort(score.ravel()[idx])[:2]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = (s1 - s0) / abs(s0) if np.isfinite(s0) else np.nan
    return (int(ii.ravel()[best]), int(jj.ravel()[best])), float(gap)


def frames_of(masked_t1hw, masks_t1hw):
    return [cr.gauges(masked_t1hw[t, 0], masks_t1hw[t, 0]) for t in range(masked_t1hw.shape[0])]


def estimate(frames, h, w, n_lags, adv):
    """(v (v_y, v_x), W, score, gap, N) of one sample with the advection settings adv (ADVECTION's keys)."""
    adv = {**ADVECTION, **adv}
    nhalf = nhalf_of(adv["vmax"], adv["vstep"])
    W, S, N = score_tables(frames, adv["n_tlags"], nhalf, adv["vstep"], adv["bandwidth"] * cr.lag_width(h, w, n_lags))
    (i, j), gap = pick(W, S, N)
    return (i * adv["vstep"], j * adv["vstep"]), W, score_of(W, S), gap, N


# ---- variogram bins on the advected distance
def lag_bins(frames, h, w, n_lags, n_tlags, v):
    """stkriging_ref.st_bins with h = |x_j - x_i - v u| for a pair (i in frame t, j in frame t + u)."""
    lw = cr.lag_width(h, w, n_lags)
    nu = min(n_tlags, len(frames) - 1) + 1
    n, sg, sh = (np.zeros((nu, n_lags)) for _ in range(3))
    n[0], sg[0], sh[0] = cr.variogram_bins(frames, h, w, n_lags)
    for u in range(1, nu):
        for t in range(len(frames) - u):
            (xa, za), (xb, zb) = frames[t], frames[t + u]
            if len(za) == 0 or len(zb) == 0:
                continue
            d = xb[None, :, :].astype(np.float64) - xa[:, None, :].astype(np.float64)
            ey, ex = d[:, :, 0] - v[0] * u, d[:, :, 1] - v[1] * u
            hh = np.sqrt(ey * ey + ex * ex).ravel()
            zd = (za.astype(np.float64)[:, None] - zb.astype(np.float64)[None, :]).ravel()
            keep = hh < n_lags * lw
            k = np.minimum(np.floor(hh[keep] / lw).astype(np.int64), n_lags - 1)
            n[u] += np.bincount(k, minlength=n_lags)
            sg[u] += np.bincount(k, weights=0.5 * zd[keep] * zd[keep], minlength=n_lags)
            sh[u] += np.bincount(k, weights=hh[keep], minlength=n_lags)
    return n, sg, sh


# ---- kriging
def lag_covariance(axy, at, bxy, bt, nugget, psill, rng, kappa, v, model, dtype):
    """c0 [len(a), len(b)] = psill (1 - g(d / range)) + nugget [same pixel and same frame], d the Lagrangian distance, in dtype."""
    d = (axy[:, None, :] - bxy[None, :, :]).astype(np.int64)
    dt = (at[:, None] - bt[None, :]).astype(np.int64)
    ft = dt.astype(dtype)
    ey = d[:, :, 0].astype(dtype) - dtype(v[0]) * ft
    ex = d[:, :, 1].astype(dtype) - dtype(v[1]) * ft
    h = np.sqrt(ey * ey + ex * ex + dtype(kappa) * dtype(kappa) * (ft * ft)).astype(dtype)
    c = (dtype(psill) * (dtype(1.0) - cr.g_of(h / dtype(rng), model))).astype(dtype)
    return c + dtype(nugget) * (((d * d).sum(-1) == 0) & (dt == 0))


def krige_sample(xy, tt, z, T, h, w, params, v, model, dtype=np.float64):
    """stkriging_ref.krige_sample with the Lagrangian distance."""
    dtype = np.dtype(dtype).type
    if len(z) == 0:
        return np.zeros((T, h, w), dtype)
    z = z.astype(dtype)
    if params is None:
        return np.full((T, h, w), z.mean(dtype=np.float64), dtype)
    nugget, psill, rng, kappa = params
    K = lag_covariance(xy, tt, xy, tt, nugget, psill, rng, kappa, v, model, dtype)
    try:
        cf = scipy.linalg.cho_factor(K, lower=True)
    except np.linalg.LinAlgError:
        return np.full((T, h, w), z.mean(dtype=np.float64), dtype)
    u = scipy.linalg.cho_solve(cf, np.ones(len(z), dtype))
    s = scipy.linalg.cho_solve(cf, z)
    m = s.sum() / u.sum()
    alpha = s - m * u
    px = cr.grid(h, w)
    out = np.empty((T, h, w), dtype)
    for t in range(T):
        c0 = lag_covariance(px, np.full(len(px), t, np.int64), xy, tt, nugget, psill, rng, kappa, v, model, dtype)
        out[t] = (m + c0 @ alpha).astype(dtype).reshape(h, w)
    return out


def sample_fit(masked, masks, b, variogram, advection):
    """(v as the device's fp32 copy holds it, params with their fp32 rounding or None for a degenerate fitted sample, the estimate
    tuple or None, the fit_st tuple or None) of sample b."""
    _, T, _, H, W = masked.shape
    model = variogram.get("model", "exponential")
    n_lags = variogram.get("n_lags", 16)
    frames = frames_of(masked[b], masks[b])
    est = None
    if advection.get("fit", True):
        est = estimate(frames, H, W, n_lags, advection)
        v = est[0]
    else:
        v = (float(advection["vy"]), float(advection["vx"]))
    fit = None
    if variogram.get("fit", True):
        fit = sr.fit_st(*lag_bins(frames, H, W, n_lags, variogram.get("n_tlags", 3), v), cr.lag_width(H, W, n_lags), model)
        params = None if fit[0] < 0 else fit[2:6]
    else:
        params = (variogram["nugget"], variogram["psill"], variogram["range"], variogram["time_scale"])
    if params is not None:
        params = tuple(float(np.float32(p)) for p in params)
    return tuple(float(np.float32(c)) for c in v), params, est, fit


def lagkriging(masked, masks, variogram, advection, dtype=np.float64):
    """masked, masks: (B, T, 1, H, W) arrays.  Returns (out (B, T, 1, H, W) of dtype, per sample (v, params, estimate, fit))."""
    B, T, _, H, W = masked.shape
    model = variogram.get("model", "exponential")
    out = np.zeros((B, T, 1, H, W), np.dtype(dtype))
    fits = []
    for b in range(B):
        v, params, est, fit = sample_fit(masked, masks, b, variogram, advection)
        fits.append((v, params, est, fit))
        xy, tt, z = sr.points(masked[b], masks[b])
        out[b, :, 0] = krige_sample(xy, tt, z, T, H, W, params, v, model, dtype)
    return out, fits


def loso(masked, masks, variogram, advection, dtype=np.float64):
    """stkriging_loso_ref.loso for the Lagrangian model: the closed form runs on the points' positions in the moving frame, x - v t (a
    linear change of coordinates turns the Lagrangian distance into the static one; the nugget stays on the same pixel and frame)."""
    B, T = masked.shape[:2]
    model = variogram.get("model", "exponential")
    out = []
    for b in range(B):
        v, params, _, _ = sample_fit(masked, masks, b, variogram, advection)
        xy, tt, z = sr.points(masked[b], masks[b])
        site = lr.site_index(xy)
        moved = xy.astype(np.float64) - np.asarray(v, np.float64)[None, :] * tt[:, None].astype(np.float64)
        pred, var = lr.block_loo(moved, tt, z, params, model, site, dtype)
        for t in range(T):
            at = tt == t
            out.append((z[at], pred[at], var[at], site[at]))
    return out


# ---- translating fields
def translating_field(seed, v, T, size=32, n_gauges=40, torus=256, sigma=3.0):
    """(truth, masked, masks), each (1, T, 1, size, size) fp32: white noise on a torus^2 grid smoothed by a Gaussian of width sigma
    (correlation exp(-r^2 / (4 sigma^2)): a correlation length of about 2 sigma = 6 px), frame t the field shifted by v t through a
    Fourier phase ramp (exact for fractional shifts), cropped to size^2, standardised over the crop and rectified at 0; n_gauges
    gauges at seeded pixels, the same sites in every frame."""
    rng = np.random.default_rng(seed)
    k = np.fft.fftfreq(torus)
    ky, kx = np.meshgrid(k, k, indexing="ij")
    spec = np.fft.fft2(rng.standard_normal((torus, torus))) * np.exp(-2.0 * (np.pi * sigma) ** 2 * (ky * ky + kx * kx))
    o = (torus - size) // 2
    frames = np.stack([np.fft.ifft2(spec * np.exp(-2j * np.pi * (ky * v[0] + kx * v[1]) * t)).real[o:o + size, o:o + size]
                       for t in range(T)])
    frames = np.maximum((frames - frames.mean()) / frames.std(), 0.0).astype(np.float32)
    mask = np.zeros(size * size, np.float32)
    mask[rng.permutation(size * size)[:n_gauges]] = 1.0
    masks = np.broadcast_to(mask.reshape(1, 1, 1, size, size), (1, T, 1, size, size)).copy()
    truth = frames.reshape(1, T, 1, size, size)
    return truth, truth * masks, masks


def rmse(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean()))


def loso_rmse(rows):
    z = np.concatenate([np.asarray(r[0], np.float64) for r in rows])
    p = np.concatenate([np.asarray(r[1], np.float64) for r in rows])
    ok = ~np.isnan(p)
    return float(np.sqrt(((z[ok] - p[ok]) ** 2).mean()))
