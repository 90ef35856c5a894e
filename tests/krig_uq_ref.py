"""numpy / scipy restatement of the kriging variance and of the leave-one-out (LOO) cross-validation of the classical baselines
(csrc/krig_uq.hip), on top of classical_ref.py.  `dtype` selects the arithmetic (float64: the reference of the
GPU tests; float32: Cholesky, triangular inverse and products in fp32, the yardstick of their error bound).  With K = L L^T, W = L^-1,
u = K^-1 1, s = 1^T u, k(p) = [c0(p, i)]_i and c00 = psill + nugget:
    sigma^2(p) = c00 - |W k(p)|^2 + (1 - u^T k(p))^2 / s   (clamped at 0; exactly 0 on a gauge pixel)
    B_ii = sum_k W_ki^2 - u_i^2 / s,   z_i - zhat_-i = alpha_i / B_ii,   sigma^2_-i = 1 / B_ii          (Dubrule 1983)"""
import numpy as np
import scipy.linalg

import classical_ref as cr


def _system(xy, params, model, dtype):
    """(W = L^-1, u, s) of a gauge set in `dtype`."""
    nugget, psill, rng = params
    K = cr.covariance(xy, xy, nugget, psill, rng, model, dtype)
    L = scipy.linalg.cholesky(K, lower=True)
    W = scipy.linalg.solve_triangular(L, np.eye(len(xy), dtype=dtype), lower=True)
    u = scipy.linalg.cho_solve((L, True), np.ones(len(xy), dtype))
    return W.astype(dtype), u.astype(dtype), u.sum(dtype=dtype)


def variance_frame(xy, h, w, params, model, dtype=np.float64, clamp=True):
    """Kriging variance (H, W) by the L^-1 formula; also returns the unclamped upper bound c00 + (1 - u^T k)^2 / s."""
    dtype = np.dtype(dtype).type
    nugget, psill, rng = params
    W, u, s = _system(xy, params, model, dtype)
    k = cr.covariance(cr.grid(h, w), xy, nugget, psill, rng, model, dtype).astype(dtype)       # [HW, N]
    q = ((k @ W.T) ** 2).sum(1, dtype=dtype)
    lag = (dtype(1.0) - k @ u) ** 2 / s
    c00 = dtype(psill) + dtype(nugget)
    var = c00 - q + lag
    if clamp:
        var = np.maximum(var, dtype(0.0))
        var[(xy[:, 0] * w + xy[:, 1])] = dtype(0.0)
    return var.reshape(h, w), (c00 + lag).reshape(h, w)


def variance_primal(xy, h, w, params, model):
    """The textbook system per pixel, fp64: [[K, 1], [1^T, 0]] [lambda; mu] = [k(p); 1], sigma^2 = c00 - lambda^T k - mu."""
    nugget, psill, rng = params
    n = len(xy)
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = cr.covariance(xy, xy, nugget, psill, rng, model, np.float64)
    A[:n, n] = A[n, :n] = 1.0
    k = cr.covariance(cr.grid(h, w), xy, nugget, psill, rng, model, np.float64)
    sol = np.linalg.solve(A, np.concatenate([k, np.ones((h * w, 1))], axis=1).T)
    return (psill + nugget - (sol[:n].T * k).sum(1) - sol[n]).reshape(h, w)


def loo_frame(xy, z, params, model, dtype=np.float64):
    """(zhat_-i, sigma^2_-i) of every gauge by the closed form, in `dtype`."""
    dtype = np.dtype(dtype).type
    nugget, psill, rng = params
    W, u, s = _system(xy, params, model, dtype)
    K = cr.covariance(xy, xy, nugget, psill, rng, model, dtype)
    v = scipy.linalg.cho_solve(scipy.linalg.cho_factor(K, lower=True), z.astype(dtype)).astype(dtype)
    alpha = v - (v.sum(dtype=dtype) / s) * u
    bii = (W * W).sum(0, dtype=dtype) - u * u / s
    return (z.astype(dtype) - alpha / bii).astype(dtype), (dtype(1.0) / bii).astype(dtype)


def loo_refit(xy, z, params, model):
    """The same by N refits, fp64: ordinary kriging of gauge i from the others through the primal system."""
    nugget, psill, rng = params
    n = len(z)
    pred, var = np.zeros(n), np.zeros(n)
    for i in range(n):
        keep = np.arange(n) != i
        m = n - 1
        A = np.zeros((m + 1, m + 1))
        A[:m, :m] = cr.covariance(xy[keep], xy[keep], nugget, psill, rng, model, np.float64)
        A[:m, m] = A[m, :m] = 1.0
        k = cr.covariance(xy[i:i + 1], xy[keep], nugget, psill, rng, model, np.float64)[0]
        sol = np.linalg.solve(A, np.concatenate([k, [1.0]]))
        pred[i] = sol[:m] @ z[keep].astype(np.float64)
        var[i] = psill + nugget - sol[:m] @ k - sol[m]
    return pred, var


def idw_loo_frame(xy, z, power=2.0, dtype=np.float64):
    """zhat_-i = sum_{j != i} w_j z_j / sum_{j != i} w_j, w_j = |x_i - x_j|^-power; NaN with fewer than 2 gauges."""
    dtype = np.dtype(dtype).type
    n = len(z)
    if n < 2:
        return np.full(n, np.nan, dtype)
    h, _ = cr._dist(xy, xy, dtype)
    with np.errstate(divide="ignore"):
        wgt = np.where(np.eye(n, dtype=bool), dtype(0), h ** dtype(-power)).astype(dtype)
    return ((wgt @ z.astype(dtype)) / wgt.sum(1)).astype(dtype)


def sample_params(masked, masks, b, variogram):
    """(model, params or None for a degenerate fitted sample) of sample b, with the fp32 rounding of the device's parameter copy."""
    _, T, _, H, W = masked.shape
    model = variogram.get("model", "exponential")
    if variogram.get("fit", True):
        n_lags = variogram.get("n_lags", 16)
        fit = cr.fit_bins(*cr.variogram_bins(cr._frames_of(masked, masks, b), H, W, n_lags), cr.lag_width(H, W, n_lags), model)
        params = None if fit[0] < 0 else fit[1:4]
    else:
        params = (variogram["nugget"], variogram["psill"], variogram["range"])
    if params is not None:
        params = tuple(float(np.float32(p)) for p in params)
    return model, params


def kriging_uq(masked, masks, variogram, dtype=np.float64):
    """masked, masks: (B, T, 1, H, W).  Returns (var (B, T, 1, H, W), c00 (B, T), loo: per frame (z, zhat_-i, sigma^2_-i) in raster
    order) with the frame rules: var is NaN over a frame without gauges or of a degenerate sample (c00 NaN too); the LOO arrays are NaN
    there and where a frame has fewer than 2 gauges."""
    B, T, _, H, W = masked.shape
    dt = np.dtype(dtype).type
    var = np.full((B, T, 1, H, W), np.nan, dt)
    c00 = np.full((B, T), np.nan)
    loo = []
    for b in range(B):
        model, params = sample_params(masked, masks, b, variogram)
        for t in range(T):
            xy, z = cr.gauges(masked[b, t, 0], masks[b, t, 0])
            nan = np.full(len(z), np.nan, dt)
            if params is None or len(z) == 0:
                loo.append((z, nan, nan))
                continue
            var[b, t, 0] = variance_frame(xy, H, W, params, model, dt)[0]
            c00[b, t] = params[0] + params[1]
            loo.append((z,) + (loo_frame(xy, z, params, model, dt) if len(z) >= 2 else (nan, nan)))
    return var, c00, loo


def idw_loo(masked, masks, power=2.0, dtype=np.float64):
    """Per frame (z, zhat_-i) in raster order."""
    B, T = masked.shape[:2]
    out = []
    for b in range(B):
        for t in range(T):
            xy, z = cr.gauges(masked[b, t, 0], masks[b, t, 0])
            out.append((z, idw_loo_frame(xy, z, power, dtype)))
    return out


def scores(z, pred, var=None):
    """n, ME, MAE, RMSE (and MSDR) over the gauges whose prediction (and variance) is not NaN; fp64."""
    z, pred = np.asarray(z, np.float64), np.asarray(pred, np.float64)
    ok = ~np.isnan(pred) & (True if var is None else ~np.isnan(np.asarray(var, np.float64)))
    e = z[ok] - pred[ok]
    out = {"n": int(ok.sum()), "ME": e.mean(), "MAE": np.abs(e).mean(), "RMSE": np.sqrt((e * e).mean())}
    if var is not None:
        out["MSDR"] = (e * e / np.asarray(var, np.float64)[ok]).mean()
    return out
