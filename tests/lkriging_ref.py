"""numpy / scipy restatement of space-time ordinary kriging in a moving neighbourhood (p2igan_bench/models/classical.py
LocalKrigingGenerator, csrc/lkrig.hip), on top of stkriging_ref.py: the brute-force selection of a target's k
nearest points by np.lexsort on (raster, frame, key), the target's own system in a chosen precision (float64: the reference of the GPU
tests; float32: everything in fp32, the yardstick of their error bound; the selection key is float64 always, as on the device), and
leave-one-site-out by the same routine with the target's pixel excluded.

Points of a sample: stkriging_ref.points (frame-major, raster order inside a frame).  Candidates of a target in frame t: the points
with |t' - t| <= frames.  key = (dy^2 + dx^2) + (kappa kappa) dt^2 with kappa the fp32 parameter, one rounded product and one rounded
sum.  Neighbours: the first min(k, candidates) in ascending (key, frame, raster index)."""
import numpy as np
import scipy.linalg

import classical_ref as cr
import stkriging_ref as sr
import stkriging_loso_ref as slr


def select(txy, t, xy, tt, kappa, k, frames, exclude_own=False):
    """sel [n, k] int64: for the targets txy [n, 2] of frame t, the indices (into xy / tt) of the selected points in selection order, -1
    past m.  exclude_own: the points at the target's own pixel (in any frame) are no candidates."""
    txy = np.asarray(txy, np.int64).reshape(-1, 2)
    cols = np.flatnonzero(np.abs(tt - t) <= frames)
    sel = np.full((len(txy), k), -1, np.int64)
    if len(cols) == 0 or len(txy) == 0:
        return sel
    kk = float(np.float32(kappa)) * float(np.float32(kappa))
    d = txy[:, None, :] - xy[cols][None, :, :]
    d2 = (d * d).sum(-1)
    dt = (t - tt[cols]).astype(np.int64)
    key = d2.astype(np.float64) + (kk * (dt * dt).astype(np.float64))[None, :]
    if exclude_own:
        key = np.where(d2 == 0, np.inf, key)
    raster = np.broadcast_to((xy[cols, 0] << 16) | xy[cols, 1], key.shape)
    frame = np.broadcast_to(tt[cols], key.shape)
    order = np.lexsort((raster, frame, key), axis=-1)[:, :k]
    ok = np.isfinite(np.take_along_axis(key, order, axis=1))
    sel[:, :order.shape[1]] = np.where(ok, cols[order], -1)
    return sel


def solve_target(ty, tx, t, xy, tt, z, params, model, dtype=np.float64):
    """(prediction, variance, weights or None) of one target from the selected points (xy, tt, z) in selection order.  A factorisation
    that fails: the fp64 mean of the selected z and NaN variance."""
    dtype = np.dtype(dtype).type
    nugget, psill, rng, kappa = params
    txy, t1 = np.array([[ty, tx]], np.int64), np.array([t], np.int64)
    K = sr.st_covariance(xy, tt, xy, tt, nugget, psill, rng, kappa, model, dtype).astype(dtype)
    c0 = sr.st_covariance(txy, t1, xy, tt, nugget, psill, rng, kappa, model, dtype)[0].astype(dtype)
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


def slots(tt):
    """The rank of every point inside its frame (the points are frame-major)."""
    if len(tt) == 0:
        return np.zeros(0, np.int64)
    first = np.searchsorted(tt, tt, side="left")
    return np.arange(len(tt)) - first


def krige_sample(xy, tt, z, T, h, w, params, model, k, frames, dtype=np.float64, every=1, fcap=None):
    """(pred (T, H W), var (T, H W), nbr (T, H W, k) or None) of one sample.  every > 1: only the targets whose flat index t H W + p is
    a multiple of it are solved (the others are NaN).  nbr (with fcap given): frame * fcap + slot of the selection, -1 past m.
    Rules: no point: zeros, NaN variance; params None: the gauge mean, NaN; no candidate in the window: the gauge mean, NaN."""
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
    code = tt * (fcap or 0) + slots(tt)
    for t in range(T):
        todo = np.flatnonzero((t * hw + np.arange(hw)) % every == 0)
        sel = select(px[todo], t, xy, tt, params[3], k, frames)
        for p, s in zip(todo, sel):
            s = s[s >= 0]
            if nbr is not None:
                nbr[t, p, :len(s)] = code[s]
            if len(s) == 0:
                pred[t, p] = mean
                continue
            pred[t, p], var[t, p], _ = solve_target(px[p, 0], px[p, 1], t, xy[s], tt[s], z[s], params, model, dtype)
    return pred, var, nbr


def loso_sample(xy, tt, z, params, model, k, frames, dtype=np.float64):
    """(zhat, sigma^2) of every point from its k nearest points at OTHER pixels; NaN where none is left or params is None."""
    dtype = np.dtype(dtype).type
    n = len(z)
    pred, var = np.full(n, np.nan, dtype), np.full(n, np.nan, dtype)
    if params is None:
        return pred, var
    for t in np.unique(tt):
        rows = np.flatnonzero(tt == t)
        sel = select(xy[rows], t, xy, tt, params[3], k, frames, exclude_own=True)
        for i, s in zip(rows, sel):
            s = s[s >= 0]
            if len(s):
                pred[i], var[i], _ = solve_target(xy[i, 0], xy[i, 1], t, xy[s], tt[s], z[s], params, model, dtype)
    return pred, var


def localkriging(masked, masks, variogram, k, frames, dtype=np.float64, every=1, fcap=None):
    """masked, masks: (B, T, 1, H, W).  Returns (out, var (B, T, 1, H, W) of dtype, nbr (B, T, H W, k) or None); the variogram and the
    fp32 rounding of its parameters are stkriging_loso_ref.sample_params'."""
    B, T, _, H, W = masked.shape
    out, var = np.zeros((B, T, 1, H, W), np.dtype(dtype)), np.zeros((B, T, 1, H, W), np.dtype(dtype))
    nbr = np.full((B, T, H * W, k), -1, np.int64) if fcap is not None else None
    for b in range(B):
        model, params = slr.sample_params(masked, masks, b, variogram)
        xy, tt, z = sr.points(masked[b], masks[b])
        p, v, nb = krige_sample(xy, tt, z, T, H, W, params, model, k, min(frames, T - 1), dtype, every, fcap)
        out[b, :, 0], var[b, :, 0] = p.reshape(T, H, W), v.reshape(T, H, W)
        if nbr is not None:
            nbr[b] = nb
    return out, var, nbr


def loso(masked, masks, variogram, k, frames, dtype=np.float64):
    """Per frame (z, zhat, sigma^2, site) in raster order, frames in (b, t) order, as stkriging_loso_ref.loso."""
    B, T = masked.shape[:2]
    out = []
    for b in range(B):
        model, params = slr.sample_params(masked, masks, b, variogram)
        xy, tt, z = sr.points(masked[b], masks[b])
        site = slr.site_index(xy)
        pred, var = loso_sample(xy, tt, z, params, model, k, min(frames, T - 1), dtype)
        for t in range(T):
            at = tt == t
            out.append((z[at], pred[at], var[at], site[at]))
    return out
