"""numpy / scipy restatement of space-time ordinary kriging (p2igan_bench/models/classical.py SpaceTimeKrigingGenerator, DESIGN.md
section 17): the space-time point set of a sample, the (u, k) variogram bins, the 17 x 25 (kappa, range) candidate fit and the
dual-form predictor.  `dtype` selects the arithmetic of the kriging part (float64: the reference of the GPU tests; float32: the
yardstick of their error bound); the variogram is float64 always, as on the device.  The spatial pieces are classical_ref's."""
import numpy as np
import scipy.linalg

import classical_ref as cr

N_RANGE = cr.N_CAND
N_KAPPA = 17
MAX_TLAGS = 7


def kappa_of(q):
    return 2.0 ** ((q - 6) / 2.0)


def range_of(c, lw):
    return lw * 2.0 ** ((c - 6) / 3.0)


def points(masked_t1hw, masks_t1hw):
    """(xy [N, 2] int64 (y, x), t [N] int64, z [N] float32) of one sample (T, 1, H, W): the frames' gauges, frame-major."""
    fr = [cr.gauges(masked_t1hw[t, 0], masks_t1hw[t, 0]) for t in range(masked_t1hw.shape[0])]
    xy = np.concatenate([f[0].reshape(-1, 2) for f in fr]).astype(np.int64)
    tt = np.concatenate([np.full(len(f[1]), t, np.int64) for t, f in enumerate(fr)])
    return xy, tt, np.concatenate([f[1] for f in fr]).astype(np.float32)


def st_covariance(axy, at, bxy, bt, nugget, psill, rng, kappa, model, dtype):
    """c0 [len(a), len(b)] = psill (1 - g(sqrt(dy^2 + dx^2 + kappa^2 dt^2) / range)) + nugget [same pixel and same frame]."""
    d = axy[:, None, :] - bxy[None, :, :]
    d2 = (d * d).sum(-1)
    dt = at[:, None] - bt[None, :]
    h = np.sqrt(d2.astype(dtype) + dtype(kappa) * dtype(kappa) * (dt * dt).astype(dtype)).astype(dtype)
    c = (dtype(psill) * (dtype(1.0) - cr.g_of(h / dtype(rng), model))).astype(dtype)
    return c + dtype(nugget) * ((d2 == 0) & (dt == 0))


def krige_sample(xy, tt, z, T, h, w, params, model, dtype=np.float64):
    """Dual-form space-time ordinary kriging of one sample -> (T, H, W).  No points: zeros.  params None (degenerate sample) or a
    failed factorisation: the mean of all the sample's gauges."""
    dtype = np.dtype(dtype).type
    if len(z) == 0:
        return np.zeros((T, h, w), dtype)
    z = z.astype(dtype)
    if params is None:
        return np.full((T, h, w), z.mean(dtype=np.float64), dtype)
    nugget, psill, rng, kappa = params
    K = st_covariance(xy, tt, xy, tt, nugget, psill, rng, kappa, model, dtype)
    try:
        cf = scipy.linalg.cho_factor(K, lower=True)
    except np.linalg.LinAlgError:
        return np.full((T, h, w), z.mean(dtype=np.float64), dtype)
    u = scipy.linalg.cho_solve(cf, np.ones(len(z), dtype))
    v = scipy.linalg.cho_solve(cf, z)
    m = v.sum() / u.sum()
    alpha = v - m * u
    px = cr.grid(h, w)
    out = np.empty((T, h, w), dtype)
    for t in range(T):                  # frame by frame: c0 of a whole sample would not fit at the point limit
        c0 = st_covariance(px, np.full(len(px), t, np.int64), xy, tt, nugget, psill, rng, kappa, model, dtype)
        out[t] = (m + c0 @ alpha).astype(dtype).reshape(h, w)
    return out


def krige_sample_primal(xy, tt, z, T, h, w, params, model):
    """The textbook system per target, fp64: [[K, 1], [1^T, 0]] [lambda; mu] = [c0; 1], prediction lambda^T z.  Returns the prediction
    (T, H, W) and the weights [T H W, N]."""
    nugget, psill, rng, kappa = params
    n = len(z)
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = st_covariance(xy, tt, xy, tt, nugget, psill, rng, kappa, model, np.float64)
    A[:n, n] = A[n, :n] = 1.0
    px = np.tile(cr.grid(h, w), (T, 1))
    pt = np.repeat(np.arange(T, dtype=np.int64), h * w)
    c0 = st_covariance(px, pt, xy, tt, nugget, psill, rng, kappa, model, np.float64)
    lam = np.linalg.solve(A, np.concatenate([c0, np.ones((len(px), 1))], axis=1).T)[:n].T
    return (lam @ z.astype(np.float64)).reshape(T, h, w), lam


def st_bins(frames, h, w, n_lags, n_tlags):
    """frames: list of (xy, z) per frame.  Returns (n, sum of (z_i - z_j)^2 / 2, sum of the spatial h), each [n_tlags + 1, n_lags]
    (n_tlags clipped to T - 1): lag u = 0 holds the pairs i < j of one frame, u >= 1 all pairs (i in frame t, j in frame t + u)."""
    lw = cr.lag_width(h, w, n_lags)
    nu = min(n_tlags, len(frames) - 1) + 1
    n, sg, sh = (np.zeros((nu, n_lags)) for _ in range(3))
    n[0], sg[0], sh[0] = cr.variogram_bins(frames, h, w, n_lags)
    for u in range(1, nu):
        for t in range(len(frames) - u):
            (xa, za), (xb, zb) = frames[t], frames[t + u]
            if len(za) == 0 or len(zb) == 0:
                continue
            d = xa[:, None, :].astype(np.int64) - xb[None, :, :].astype(np.int64)
            hh = np.sqrt((d * d).sum(-1).astype(np.float64)).ravel()
            zd = (za.astype(np.float64)[:, None] - zb.astype(np.float64)[None, :]).ravel()
            keep = hh < n_lags * lw
            k = np.minimum(np.floor(hh[keep] / lw).astype(np.int64), n_lags - 1)
            n[u] += np.bincount(k, minlength=n_lags)
            sg[u] += np.bincount(k, weights=0.5 * zd[keep] * zd[keep], minlength=n_lags)
            sh[u] += np.bincount(k, weights=hh[keep], minlength=n_lags)
    return n, sg, sh


def model_gamma(hbar, u, nugget, psill, a, kappa, model):
    """gamma of the fitted family at mean spatial distance hbar and temporal lag u (u = 0: the spatial distance as it is)."""
    d = np.where(u == 0, hbar, np.sqrt(hbar * hbar + (kappa * u) * (kappa * u)))
    return nugget + psill * cr.g_of(d / a, model)


def fit_st(n, sg, sh, lw, model):
    """The (kappa_q, a_c) candidate fit over the non-empty bins.  Returns (q, c, nugget, psill, range, kappa, sse, all_sse [17, 25] (inf
    where invalid)); q = c = -1 (others None) for a degenerate sample.  The lowest q 25 + c wins a tie."""
    ok = n > 0
    sses = np.full((N_KAPPA, N_RANGE), np.inf)
    sol = {}
    if ok.any():
        uu = np.broadcast_to(np.arange(n.shape[0], dtype=np.float64)[:, None], n.shape)[ok]
        nn, gam, hb = n[ok], sg[ok] / n[ok], sh[ok] / n[ok]
        for q in range(N_KAPPA):
            for c in range(N_RANGE):
                g = model_gamma(hb, uu, 0.0, 1.0, range_of(c, lw), kappa_of(q), model)
                S0, S1, S2, T0, T1 = nn.sum(), (nn * g).sum(), (nn * g * g).sum(), (nn * gam).sum(), (nn * g * gam).sum()
                det = S0 * S2 - S1 * S1
                nug, ps = -1.0, 0.0
                if det > 1e-12 * S0 * S2:
                    ps = (S0 * T1 - S1 * T0) / det
                    nug = (T0 - ps * S1) / S0
                if nug < 0.0:
                    nug, ps = 0.0, (T1 / S2 if S2 > 0 else 0.0)
                if not ps > 0:
                    continue
                sses[q, c] = (nn * (gam - nug - ps * g) ** 2).sum()
                sol[q, c] = (nug, ps)
    if not np.isfinite(sses).any():
        return -1, -1, None, None, None, None, None, sses
    q, c = divmod(int(np.argmin(sses.ravel())), N_RANGE)          # first minimum: the lowest q 25 + c on a tie
    return (q, c) + sol[q, c] + (range_of(c, lw), kappa_of(q), float(sses[q, c]), sses)


def stkriging(masked, masks, variogram, dtype=np.float64):
    """masked, masks: (B, T, 1, H, W) arrays.  Returns (out (B, T, 1, H, W) of dtype, fits: per sample the fit_st tuple or None)."""
    B, T, _, H, W = masked.shape
    model = variogram.get("model", "exponential")
    out = np.zeros((B, T, 1, H, W), np.dtype(dtype))
    fits = []
    for b in range(B):
        if variogram.get("fit", True):
            n_lags = variogram.get("n_lags", 16)
            frames = [cr.gauges(masked[b, t, 0], masks[b, t, 0]) for t in range(T)]
            fit = fit_st(*st_bins(frames, H, W, n_lags, variogram.get("n_tlags", 3)), cr.lag_width(H, W, n_lags), model)
            fits.append(fit)
            params = None if fit[0] < 0 else fit[2:6]
        else:
            fits.append(None)
            params = (variogram["nugget"], variogram["psill"], variogram["range"], variogram["time_scale"])
        if params is not None:        # the device hands the kernels an fp32 copy of the parameters
            params = tuple(float(np.float32(p)) for p in params)
        xy, tt, z = points(masked[b], masks[b])
        out[b, :, 0] = krige_sample(xy, tt, z, T, H, W, params, model, dtype)
    return out, fits
