"""numpy / scipy restatement of the classical baselines (p2igan_bench/models/classical.py): ordinary kriging in
its dual form, the empirical variogram with its candidate-range fit, and all-gauge IDW.  `dtype` selects the arithmetic of the
kriging and IDW parts (float64: the reference of the GPU tests; float32: the yardstick of their error bound); the variogram is
float64 always, as on the device.  Gauges of a frame: pixels with mask != 0 in raster order, coordinates (y, x) in pixels."""
import numpy as np
import scipy.linalg

MODELS = ("exponential", "spherical")
N_CAND = 25


def gauges(masked_hw, mask_hw):
    """(xy [N, 2] int64 (y, x), z [N] float32) of one frame."""
    idx = np.flatnonzero(np.asarray(mask_hw).ravel() != 0)
    w = mask_hw.shape[1]
    return np.stack([idx // w, idx % w], axis=1), np.asarray(masked_hw, dtype=np.float32).ravel()[idx]


def g_of(r, model):
    if model == "exponential":
        return 1.0 - np.exp(-r)
    return np.where(r < 1.0, 1.5 * r - 0.5 * r ** 3, 1.0).astype(r.dtype)


def _dist(a, b, dtype):
    d = a[:, None, :] - b[None, :, :]
    d2 = (d * d).sum(-1)
    return np.sqrt(d2.astype(dtype)), d2


def covariance(a, b, nugget, psill, rng, model, dtype):
    """c0 [len(a), len(b)] = psill (1 - g(h / range)) + nugget [a_i = b_j]."""
    h, d2 = _dist(a, b, dtype)
    c = (dtype(psill) * (dtype(1.0) - g_of(h / dtype(rng), model))).astype(dtype)
    return c + dtype(nugget) * (d2 == 0)


def grid(h, w):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([yy.ravel(), xx.ravel()], axis=1)


def krige_frame(xy, z, h, w, params, model, dtype=np.float64):
    """Dual-form ordinary kriging of one frame -> (H, W).  No gauges: zeros.  params None (degenerate sample) or a failed
    factorisation: the gauge mean."""
    dtype = np.dtype(dtype).type
    if len(z) == 0:
        return np.zeros((h, w), dtype)
    z = z.astype(dtype)
    if params is None:
        return np.full((h, w), z.mean(dtype=np.float64), dtype)
    nugget, psill, rng = params
    K = covariance(xy, xy, nugget, psill, rng, model, dtype)
    try:
        cf = scipy.linalg.cho_factor(K, lower=True)
    except np.linalg.LinAlgError:
        return np.full((h, w), z.mean(dtype=np.float64), dtype)
    u = scipy.linalg.cho_solve(cf, np.ones(len(z), dtype))
    v = scipy.linalg.cho_solve(cf, z)
    m = v.sum() / u.sum()
    alpha = v - m * u
    c0 = covariance(grid(h, w), xy, nugget, psill, rng, model, dtype)
    return (m + c0 @ alpha).astype(dtype).reshape(h, w)


def krige_frame_primal(xy, z, h, w, params, model):
    """The textbook system per pixel, fp64: [[K, 1], [1^T, 0]] [lambda; mu] = [c0(p); 1], prediction lambda^T z.  Returns the
    prediction (H, W) and the weights [H W, N]."""
    nugget, psill, rng = params
    n = len(z)
    K = covariance(xy, xy, nugget, psill, rng, model, np.float64)
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = K
    A[:n, n] = A[n, :n] = 1.0
    c0 = covariance(grid(h, w), xy, nugget, psill, rng, model, np.float64)
    rhs = np.concatenate([c0, np.ones((h * w, 1))], axis=1).T
    lam = np.linalg.solve(A, rhs)[:n].T
    return (lam @ z.astype(np.float64)).reshape(h, w), lam


def lag_width(h, w, n_lags):
    return (min(h, w) / 2.0) / n_lags


def variogram_bins(frames, h, w, n_lags):
    """frames: list of (xy, z).  Returns (n [n_lags], sum of (z_i - z_j)^2 / 2, sum of h), pooled over the frames' pairs i < j."""
    lw = lag_width(h, w, n_lags)
    n, sg, sh = np.zeros(n_lags), np.zeros(n_lags), np.zeros(n_lags)
    for xy, z in frames:
        if len(z) < 2:
            continue
        i, j = np.triu_indices(len(z), 1)
        d = (xy[i] - xy[j]).astype(np.int64)
        hh = np.sqrt((d * d).sum(-1).astype(np.float64))
        keep = hh < n_lags * lw
        k = np.minimum(np.floor(hh[keep] / lw).astype(np.int64), n_lags - 1)
        zd = z[i][keep].astype(np.float64) - z[j][keep].astype(np.float64)
        n += np.bincount(k, minlength=n_lags)
        sg += np.bincount(k, weights=0.5 * zd * zd, minlength=n_lags)
        sh += np.bincount(k, weights=hh[keep], minlength=n_lags)
    return n, sg, sh


def fit_bins(n, sg, sh, lw, model):
    """Candidate-range fit over the non-empty bins.  Returns (cand, nugget, psill, range, sse, all_sse [25] (inf where invalid)); cand
    -1 (others None) for a degenerate sample."""
    ok = n > 0
    sses = np.full(N_CAND, np.inf)
    sol = [None] * N_CAND
    if ok.any():
        nn, gam, hb = n[ok], sg[ok] / n[ok], sh[ok] / n[ok]
        for c in range(N_CAND):
            a = lw * 2.0 ** ((c - 6) / 3.0)
            g = g_of(hb / a, model)
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
            sses[c] = (nn * (gam - nug - ps * g) ** 2).sum()
            sol[c] = (nug, ps, a)
    if not np.isfinite(sses).any():
        return -1, None, None, None, None, sses
    c = int(np.argmin(sses))          # first minimum: the lowest c on a tie
    return (c,) + sol[c] + (float(sses[c]), sses)


def _frames_of(masked, masks, b):
    return [gauges(masked[b, t, 0], masks[b, t, 0]) for t in range(masked.shape[1])]


def kriging(masked, masks, variogram, dtype=np.float64):
    """masked, masks: (B, T, 1, H, W) arrays.  Returns (out (B, T, 1, H, W) of dtype, fits: per sample the fit_bins tuple or None)."""
    B, T, _, H, W = masked.shape
    model = variogram.get("model", "exponential")
    out = np.zeros((B, T, 1, H, W), np.dtype(dtype))
    fits = []
    for b in range(B):
        frames = _frames_of(masked, masks, b)
        if variogram.get("fit", True):
            n_lags = variogram.get("n_lags", 16)
            fit = fit_bins(*variogram_bins(frames, H, W, n_lags), lag_width(H, W, n_lags), model)
            fits.append(fit)
            params = None if fit[0] < 0 else fit[1:4]
        else:
            fits.append(None)
            params = (variogram["nugget"], variogram["psill"], variogram["range"])
        if params is not None:        # the device hands the kernels an fp32 copy of the parameters
            params = tuple(float(np.float32(p)) for p in params)
        for t, (xy, z) in enumerate(frames):
            out[b, t, 0] = krige_frame(xy, z, H, W, params, model, dtype)
    return out, fits


def idw(masked, masks, power=2.0, dtype=np.float64):
    dtype = np.dtype(dtype).type
    B, T, _, H, W = masked.shape
    out = np.zeros((B, T, 1, H, W), dtype)
    px = grid(H, W)
    for b in range(B):
        for t in range(T):
            xy, z = gauges(masked[b, t, 0], masks[b, t, 0])
            if len(z) == 0:
                continue
            h, d2 = _dist(px, xy, dtype)
            with np.errstate(divide="ignore"):
                wgt = np.where(d2 == 0, dtype(0), h ** dtype(-power)).astype(dtype)
            pred = (wgt @ z.astype(dtype)) / np.maximum(wgt.sum(1), np.finfo(dtype).tiny)
            hit = (d2 == 0)
            at = hit.any(1)
            pred[at] = z.astype(dtype)[hit[at].argmax(1)]
            out[b, t, 0] = pred.reshape(H, W)
    return out


def gauge_mean_predictor(masked, masks):
    """Per-frame gauge mean everywhere (0 without gauges), fp64: the trivial yardstick of the RMSE check."""
    m = (masks != 0).astype(np.float64)
    cnt = m.sum(axis=(-1, -2), keepdims=True)
    mean = (masked.astype(np.float64) * m).sum(axis=(-1, -2), keepdims=True) / np.maximum(cnt, 1.0)
    return np.broadcast_to(mean, masked.shape).copy()
