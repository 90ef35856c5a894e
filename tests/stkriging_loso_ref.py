"""numpy / scipy restatement of the leave-one-site-out (LOSO) cross-validation of space-time ordinary kriging (csrc/stkrig_loso.hip,
DESIGN.md section 18), on top of stkriging_ref.py.  A site is the set of a sample's points that share a pixel.  With K = L L^T,
W = L^-1, u = K^-1 1, s = 1^T u and alpha the dual coefficients, for a site S (the block form of Dubrule's identity):
    B_SS = (W^T W)_SS - u_S u_S^T / s,   z_S - zhat_-S = B_SS^-1 alpha_S,   sigma^2_-S = diag(B_SS^-1)
`dtype` selects the arithmetic (float64: the reference of the GPU tests; float32: everything in fp32, the yardstick of their bound)."""
import numpy as np
import scipy.linalg

import classical_ref as cr
import stkriging_ref as sr


def site_index(xy):
    """Per point the rank of its pixel among the sample's distinct pixels in raster order."""
    if len(xy) == 0:
        return np.zeros(0, np.int64)
    return np.unique((xy[:, 0].astype(np.int64) << 16) | xy[:, 1].astype(np.int64), return_inverse=True)[1].astype(np.int64)


def block_loo(xy, tt, z, params, model, groups, dtype=np.float64):
    """(zhat, sigma^2) of every point with its whole group left out, by the closed form in `dtype`; groups: an index per point.  All
    NaN with fewer than 2 groups, params None or a factorisation that fails."""
    dtype = np.dtype(dtype).type
    n = len(z)
    pred, var = np.full(n, np.nan, dtype), np.full(n, np.nan, dtype)
    if n == 0 or params is None or len(np.unique(groups)) < 2:
        return pred, var
    nugget, psill, rng, kappa = params
    K = sr.st_covariance(xy, tt, xy, tt, nugget, psill, rng, kappa, model, dtype).astype(dtype)
    try:
        L = scipy.linalg.cholesky(K, lower=True)
    except np.linalg.LinAlgError:
        return pred, var
    W = scipy.linalg.solve_triangular(L, np.eye(n, dtype=dtype), lower=True).astype(dtype)
    zt = z.astype(dtype)
    u = scipy.linalg.cho_solve((L, True), np.ones(n, dtype)).astype(dtype)
    v = scipy.linalg.cho_solve((L, True), zt).astype(dtype)
    s = u.sum(dtype=dtype)
    alpha = (v - (v.sum(dtype=dtype) / s) * u).astype(dtype)
    G = (W.T @ W).astype(dtype)
    for g in np.unique(groups):
        idx = np.flatnonzero(groups == g)
        Bss = (G[np.ix_(idx, idx)] - np.outer(u[idx], u[idx]) / s).astype(dtype)
        try:
            cf = scipy.linalg.cho_factor(Bss, lower=True)
        except np.linalg.LinAlgError:
            continue
        inv = scipy.linalg.cho_solve(cf, np.eye(len(idx), dtype=dtype)).astype(dtype)
        pred[idx] = zt[idx] - inv @ alpha[idx]
        var[idx] = np.diag(inv)
    return pred, var


def block_refit(xy, tt, z, params, model, groups):
    """The same by one refit per group, fp64: ordinary kriging of the group's points from the other groups' points through the primal
    system [[K, 1], [1^T, 0]] [lambda; mu] = [k; 1], sigma^2 = c00 - lambda^T k - mu."""
    nugget, psill, rng, kappa = params
    n = len(z)
    pred, var = np.full(n, np.nan), np.full(n, np.nan)
    if len(np.unique(groups)) < 2:
        return pred, var
    for g in np.unique(groups):
        out, keep = np.flatnonzero(groups == g), np.flatnonzero(groups != g)
        m = len(keep)
        A = np.zeros((m + 1, m + 1))
        A[:m, :m] = sr.st_covariance(xy[keep], tt[keep], xy[keep], tt[keep], nugget, psill, rng, kappa, model, np.float64)
        A[:m, m] = A[m, :m] = 1.0
        k = sr.st_covariance(xy[out], tt[out], xy[keep], tt[keep], nugget, psill, rng, kappa, model, np.float64)
        sol = np.linalg.solve(A, np.concatenate([k, np.ones((len(out), 1))], axis=1).T)
        pred[out] = sol[:m].T @ z[keep].astype(np.float64)
        var[out] = psill + nugget - (sol[:m].T * k).sum(1) - sol[m]
    return pred, var


def sample_params(masked, masks, b, variogram):
    """(model, params or None for a degenerate fitted sample) of sample b, with the fp32 rounding of the device's parameter copy."""
    _, T, _, H, W = masked.shape
    model = variogram.get("model", "exponential")
    if variogram.get("fit", True):
        n_lags = variogram.get("n_lags", 16)
        frames = [cr.gauges(masked[b, t, 0], masks[b, t, 0]) for t in range(T)]
        fit = sr.fit_st(*sr.st_bins(frames, H, W, n_lags, variogram.get("n_tlags", 3)), cr.lag_width(H, W, n_lags), model)
        params = None if fit[0] < 0 else fit[2:6]
    else:
        params = (variogram["nugget"], variogram["psill"], variogram["range"], variogram["time_scale"])
    if params is not None:
        params = tuple(float(np.float32(p)) for p in params)
    return model, params


def loso(masked, masks, variogram, dtype=np.float64, pointwise=False):
    """masked, masks: (B, T, 1, H, W).  Per frame (z, zhat_-S, sigma^2_-S, site) in raster order, frames in (b, t) order; the
    prediction and variance are NaN over a sample with one site only or a degenerate fit.  pointwise: every point is its own group
    (the point-wise leave-one-out that flatters the method), the site column is unchanged."""
    B, T = masked.shape[:2]
    out = []
    for b in range(B):
        model, params = sample_params(masked, masks, b, variogram)
        xy, tt, z = sr.points(masked[b], masks[b])
        site = site_index(xy)
        pred, var = block_loo(xy, tt, z, params, model, np.arange(len(z)) if pointwise else site, dtype)
        for t in range(T):
            at = tt == t
            out.append((z[at], pred[at], var[at], site[at]))
    return out
