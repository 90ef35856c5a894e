"""numpy / scipy restatement of moving-neighbourhood space-time kriging in the Lagrangian frame (p2igan_bench/models/classical.py
LocalLagrangianKrigingGenerator, csrc/lkrig.hip's LAG kernels), on top of lkriging_ref.py (candidates, window,
rules, tie order) and lagkriging_ref.py (velocity, variogram, lag_covariance): the brute-force selection of a target's k nearest points
by np.lexsort on (raster, frame, key) with the key measured in the frame that moves with the rain, the target's own system through
lagkriging_ref.lag_covariance in a chosen precision (float64: the reference of the GPU tests; float32: the yardstick of their error
bound; the key is float64 always, as on the device), and leave-one-site-out by the same routine with the target's pixel excluded.

key of a point (g, t') for a target (x, t), v and kappa the fp32 values: fdt = t - t', e = (x - g) - v fdt (one product, one difference
per axis), key = ((e_y e_y + e_x e_x) + (kappa kappa) dt^2), every operation rounded once.  With v = 0 it is lkriging_ref's key bit for
bit."""
import numpy as np
import scipy.linalg

import classical_ref as cr
import lagkriging_ref as lg
import lkriging_ref as lr
import stkriging_loso_ref as slr
import stkriging_ref as sr


def select(txy, t, xy, tt, kappa, v, k, frames, exclude_own=False):
    """lkriging_ref.select with the Lagrangian key; v = (v_y, v_x)."""
    txy = np.asarray(txy, np.int64).reshape(-1, 2)
    cols = np.flatnonzero(np.abs(tt - t) <= frames)
    sel = np.full((len(txy), k), -1, np.int64)
    if len(cols) == 0 or len(txy) == 0:
        return sel
    kk = float(np.float32(kappa)) * float(np.float32(kappa))
    vy, vx = float(np.float32(v[0])), float(np.float32(v[1]))
    d = txy[:, None, :] - xy[cols][None, :, :]
    dt = (t - tt[cols]).astype(np.int64)
    fdt = dt.astype(np.float64)
    ey = d[:, :, 0].astype(np.float64) - (vy * fdt)[None, :]
    ex = d[:, :, 1].astype(np.float64) - (vx * fdt)[None, :]
    key = (ey * ey + ex * ex) + (kk * (dt * dt).astype(np.float64))[None, :]
    if exclude_own:
        key = np.where((d * d).sum(-1) == 0, np.inf, key)
    raster = np.broadcast_to((xy[cols, 0] << 16) | xy[cols, 1], key.shape)
    frame = np.broadcast_to(tt[cols], key.shape)
    order = np.lexsort((raster, frame, key), axis=-1)[:, :k]
    ok = np.isfinite(np.take_along_axis(key, order, axis=1))
    sel[:, :order.shape[1]] = np.where(ok, cols[order], -1)
    return sel


def solve_target(ty, tx, t, xy, tt, z, params, v, model, dtype=np.float64):
    """lkriging_ref.solve_target with K and c0 from lagkriging_ref.lag_covariance."""
    dtype = np.dtype(dtype).type
    nugget, psill, rng, kappa = params
    txy, t1 = np.array([[ty, tx]], np.int64), np.array([t], np.int64)
    K = lg.lag_covariance(xy, tt, xy, tt, nugget, psill, rng, kappa, v, model, dtype).astype(dtype)
    c0 = lg.lag_covariance(txy, t1, xy, tt, nugget, psill, rng, kappa, v, model, dtype)[0].astype(dtype)
    try:
        cf = scipy.linalg.cho_factor(K, lower=True)
    except np.linalg.LinAlgError:
        return dtype(z.astype(np.float64).mean()), dtype(np.nan), None
    a = scipy.linalg.cho_solve(cf, c0).astype(dtype)
    u = scipy.linalg.cho_solve(cf, np.ones(len(z), dtype)).astype(dtype)
    mu = (a.sum(dtype=dtype) - dtype(1.0)) / u.sum(dtype=dtype)
    lam = (a - mu * u).astype(dtype)
    pred = (lam * z.astype(dtype)).sum(dtype=dtype)
    var = max(dtype(psill) + dtype(nugget) - (lam * c0).sum(dtype=dtype) - mu, dtype(0.0))
    if ((xy[:, 0] == ty) & (xy[:, 1] == tx) & (tt == t)).any():
        var = dtype(0.0)
    return dtype(pred), dtype(var), lam


def krige_sample(xy, tt, z, T, h, w, params, v, model, k, frames, dtype=np.float64, every=1, fcap=None):
    """lkriging_ref.krige_sample (its `every` and `fcap`, its rules) in the Lagrangian frame."""
    dtype = np.dtype(dtype).type
    hw = h * w
    pred, var = np.full((T, hw), np.nan, dtype), np.full((T, hw), np.nan, dtype)
    nbr = np.full((T, hw, k), -1, np.int64) if fcap is not None else None
    if len(z) == 0:
        return np.zeros((T, hw), dtype), var, nbr
    mean = z.astype(np.float64).mean()
    if params is None:
        return np.full((T, hw), mean, dtype), var, nbr
    px = cr.grid(h, w)
    code = tt * (fcap or 0) + lr.slots(tt)
    for t in range(T):
        todo = np.flatnonzero((t * hw + np.arange(hw)) % every == 0)
        sel = select(px[todo], t, xy, tt, params[3], v, k, frames)
        for p, s in zip(todo, sel):
            s = s[s >= 0]
            if nbr is not None:
                nbr[t, p, :len(s)] = code[s]
            if len(s) == 0:
                pred[t, p] = mean
                continue
            pred[t, p], var[t, p], _ = solve_target(px[p, 0], px[p, 1], t, xy[s], tt[s], z[s], params, v, model, dtype)
    return pred, var, nbr


def loso_sample(xy, tt, z, params, v, model, k, frames, dtype=np.float64):
    """(zhat, sigma^2) of every point from its k nearest points at OTHER pixels; NaN where none is left or params is None."""
    dtype = np.dtype(dtype).type
    n = len(z)
    pred, var = np.full(n, np.nan, dtype), np.full(n, np.nan, dtype)
    if params is None:
        return pred, var
    for t in np.unique(tt):
        rows = np.flatnonzero(tt == t)
        sel = select(xy[rows], t, xy, tt, params[3], v, k, frames, exclude_own=True)
        for i, s in zip(rows, sel):
            s = s[s >= 0]
            if len(s):
                pred[i], var[i], _ = solve_target(xy[i, 0], xy[i, 1], t, xy[s], tt[s], z[s], params, v, model, dtype)
    return pred, var


def locallagkriging(masked, masks, variogram, advection, k, frames, dtype=np.float64, every=1, fcap=None):
    """masked, masks: (B, T, 1, H, W).  Returns (out, var (B, T, 1, H, W) of dtype, nbr (B, T, H W, k) or None, per sample
    lagkriging_ref.sample_fit's (v, params, estimate, fit)): the velocity, the variogram and their fp32 rounding are lagkriging_ref's."""
    B, T, _, H, W = masked.shape
    model = variogram.get("model", "exponential")
    out, var = np.zeros((B, T, 1, H, W), np.dtype(dtype)), np.zeros((B, T, 1, H, W), np.dtype(dtype))
    nbr = np.full((B, T, H * W, k), -1, np.int64) if fcap is not None else None
    fits = []
    for b in range(B):
        fits.append(lg.sample_fit(masked, masks, b, variogram, advection))
        v, params = fits[-1][:2]
        xy, tt, z = sr.points(masked[b], masks[b])
        p, s2, nb = krige_sample(xy, tt, z, T, H, W, params, v, model, k, min(frames, T - 1), dtype, every, fcap)
        out[b, :, 0], var[b, :, 0] = p.reshape(T, H, W), s2.reshape(T, H, W)
        if nbr is not None:
            nbr[b] = nb
    return out, var, nbr, fits


def loso(masked, masks, variogram, advection, k, frames, dtype=np.float64):
    """Per frame (z, zhat, sigma^2, site) in raster order, frames in (b, t) order, as lkriging_ref.loso; the velocity and the variogram
    are fitted once from all sites."""
    B, T = masked.shape[:2]
    model = variogram.get("model", "exponential")
    out = []
    for b in range(B):
        v, params, _, _ = lg.sample_fit(masked, masks, b, variogram, advection)
        xy, tt, z = sr.points(masked[b], masks[b])
        site = slr.site_index(xy)
        pred, var = loso_sample(xy, tt, z, params, v, model, k, min(frames, T - 1), dtype)
        for t in range(T):
            at = tt == t
            out.append((z[at], pred[at], var[at], site[at]))
    return out
