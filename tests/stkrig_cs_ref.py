"""numpy / scipy restatement of the conditional simulation of space-time ordinary kriging (csrc/stkrig_cs.hip),
on top of krig_cs_ref.py (Philox, Box-Muller) and stkriging_ref.py (points, covariance, fit).  `dtype` selects the arithmetic
(float64: the reference of the GPU tests; float32: Box-Muller, amplitude, scipy.fft.fftn on complex64, Cholesky and products in fp32,
the yardstick of their error bound).  The spectrum is float64 always, as on the device, and the amplitude is stored as fp32.

    b[l, j, k] = C(sqrt(dj^2 + dk^2 + kappa^2 dl^2)) + nugget [dl = dj = dk = 0] on the torus St x Sy x Sx = (e_t T) x (e H) x (e W)
    lambda = Re DFT3(b); A = sqrt(lambda+ / (St Sy Sx)), lambda+ = max(lambda, 0) sum lambda / sum max(lambda, 0)
    rho = sum max(-lambda, 0) / sum |lambda|
    xi = Box-Muller of Philox4x32-10(counter ((l Sy + j) Sx + k, q, stream lo, hi), key (seed lo, hi)); Y = DFT3(A xi)[:T, :H, :W]
    U_2q = Re Y, U_2q+1 = Im Y; r = z - U(t_i, p_i), v = K^-1 r, mu = 1^T v / s, alpha = v - mu u
    Z_m(t, p) = U_m(t, p) + mu + sum_i alpha_i c0((t, p), i), written as z_i at a point's own frame and pixel"""
import numpy as np
import scipy.fft
import scipy.linalg

import classical_ref as cr
import krig_cs_ref as cs
import stkriging_ref as st

MAX_ST = 128


def torus(t, h, w, embed=2, embed_time=2):
    if embed_time not in (2, 3, 4):
        raise ValueError(f"embed_time must be 2, 3 or 4 (got {embed_time})")
    Sy, Sx = cs.torus(h, w, embed)
    if embed_time * t > MAX_ST:
        raise ValueError(f"the torus has {embed_time * t} temporal cells, more than {MAX_ST}")
    return embed_time * t, Sy, Sx


def base(params, model, t, h, w, embed=2, embed_time=2):
    """b (St, Sy, Sx) float64 of one sample, from the fp32-rounded params (nugget, psill, range, kappa)."""
    nugget, psill, rng, kappa = (float(np.float32(p)) for p in params)
    St, Sy, Sx = torus(t, h, w, embed, embed_time)
    dl = np.minimum(np.arange(St), St - np.arange(St))[:, None, None]
    dj = np.minimum(np.arange(Sy), Sy - np.arange(Sy))[None, :, None]
    dk = np.minimum(np.arange(Sx), Sx - np.arange(Sx))[None, None, :]
    d2 = dj * dj + dk * dk
    d = np.sqrt(d2.astype(np.float64) + kappa * kappa * (dl * dl).astype(np.float64))
    return psill * (1.0 - cr.g_of(d / rng, model)) + nugget * ((d2 == 0) & (dl == 0))


def spectrum(params, model, t, h, w, embed=2, embed_time=2):
    """(A (St, Sy, Sx) float64, rho) of one sample."""
    b = base(params, model, t, h, w, embed, embed_time)
    lam = np.fft.fftn(b).real
    pos, neg = np.maximum(lam, 0.0), np.maximum(-lam, 0.0)
    lam_plus = pos * (lam.sum() / pos.sum())
    return np.sqrt(lam_plus / b.size), neg.sum() / (pos.sum() + neg.sum())


def noise(seed, stream, q, St, Sy, Sx, dtype=np.float64):
    """xi (len(q), St, Sy, Sx) complex of the member pairs q of sample id `stream`: krig_cs_ref's noise over the flat cell index."""
    xi = cs.noise(seed, stream, q, St * Sy, Sx, dtype)
    return xi.reshape(xi.shape[0], St, Sy, Sx)


def unconditional(A, seed, stream, members, t, h, w, dtype=np.float64):
    """U (members, t, h, w): the pairs' real and imaginary parts, the last imaginary part dropped for odd `members`."""
    ft = np.dtype(dtype).type
    St, Sy, Sx = A.shape
    npairs = (members + 1) // 2
    xi = noise(seed, stream, np.arange(npairs), St, Sy, Sx, ft)
    a = A.astype(np.float32).astype(ft)                       # the amplitude is stored as fp32
    Y = scipy.fft.fftn((a[None] * xi).astype(xi.dtype), axes=(1, 2, 3))[:, :t, :h, :w]
    U = np.empty((2 * npairs, t, h, w), ft)
    U[0::2], U[1::2] = Y.real, Y.imag
    return U[:members]


def members_sample(xy, tt, z, t, h, w, params, model, members, seed, stream, embed=2, embed_time=2, dtype=np.float64, A=None,
                   write_points=True):
    """The conditional members (members, t, h, w) of one sample with points (xy (N, 2), frames tt, values z) and params (nugget, psill,
    range, kappa).  write_points=False leaves the points as the conditioning computes them."""
    ft = np.dtype(dtype).type
    nugget, psill, rng, kappa = params
    if A is None:
        A = spectrum(params, model, t, h, w, embed, embed_time)[0]
    U = unconditional(A, seed, stream, members, t, h, w, ft)
    K = st.st_covariance(xy, tt, xy, tt, nugget, psill, rng, kappa, model, ft)
    cf = scipy.linalg.cho_factor(K, lower=True)
    u = scipy.linalg.cho_solve(cf, np.ones(len(z), ft)).astype(ft)
    px = cr.grid(h, w)
    c0 = [st.st_covariance(px, np.full(len(px), f, np.int64), xy, tt, nugget, psill, rng, kappa, model, ft).astype(ft) for f in range(t)]
    Z = np.empty((members, t, h, w), ft)
    for m in range(members):             # member by member: no library blocks over the members, so a member does not depend on their number
        r = (z.astype(ft) - U[m, tt, xy[:, 0], xy[:, 1]]).astype(ft)
        v = scipy.linalg.cho_solve(cf, r).astype(ft)
        mu = v.sum(dtype=ft) / u.sum(dtype=ft)
        alpha = (v - mu * u).astype(ft)
        for f in range(t):
            Z[m, f] = (U[m, f].reshape(h * w) + mu + c0[f] @ alpha).astype(ft).reshape(h, w)
    if write_points:
        Z[:, tt, xy[:, 0], xy[:, 1]] = z.astype(ft)[None, :]
    return Z


def sample_params(masked, masks, b, variogram):
    """(model, params or None) of sample b: the fixed parameters, or stkriging_ref's fit (None where it is degenerate), rounded to
    fp32 as the device hands them to the kernels."""
    model = variogram.get("model", "exponential")
    T, H, W = masked.shape[1], masked.shape[3], masked.shape[4]
    if variogram.get("fit", True):
        n_lags = variogram.get("n_lags", 16)
        frames = [cr.gauges(masked[b, t, 0], masks[b, t, 0]) for t in range(T)]
        fit = st.fit_st(*st.st_bins(frames, H, W, n_lags, variogram.get("n_tlags", 3)), cr.lag_width(H, W, n_lags), model)
        params = None if fit[0] < 0 else fit[2:6]
    else:
        params = (variogram["nugget"], variogram["psill"], variogram["range"], variogram["time_scale"])
    if params is not None:
        params = tuple(float(np.float32(p)) for p in params)
    return model, params


def simulation(masked, masks, variogram, members, seed=0, streams=None, embed=2, embed_time=2, dtype=np.float64):
    """masked, masks: (B, T, 1, H, W).  Returns (ens (B, T, members, H, W), rho (B,)) with the sample rules: NaN in every member of
    every frame of a sample without points or with a degenerate fit (rho NaN for the latter); a frame without gauges inside a sample
    that has points is simulated like any other.  streams (B,) defaults to b."""
    B, T, _, H, W = masked.shape
    ft = np.dtype(dtype).type
    ens = np.full((B, T, members, H, W), np.nan, ft)
    rho = np.full(B, np.nan)
    if streams is None:
        streams = np.arange(B, dtype=np.int64)
    for b in range(B):
        model, params = sample_params(masked, masks, b, variogram)
        if params is None:
            continue
        A, rho[b] = spectrum(params, model, T, H, W, embed, embed_time)
        xy, tt, z = st.points(masked[b], masks[b])
        if len(z):
            Z = members_sample(xy, tt, z, T, H, W, params, model, members, seed, int(streams[b]), embed, embed_time, ft, A)
            ens[b] = Z.transpose(1, 0, 2, 3)
    return ens, rho


def kriging_variance(xy, tt, t, h, w, params, model):
    """The analytic space-time ordinary-kriging variance (t, h, w), fp64: c00 - c0^T K^-1 c0 + (1 - u^T c0)^2 / s."""
    nugget, psill, rng, kappa = params
    K = st.st_covariance(xy, tt, xy, tt, nugget, psill, rng, kappa, model, np.float64)
    px = np.tile(cr.grid(h, w), (t, 1))
    pt = np.repeat(np.arange(t, dtype=np.int64), h * w)
    c0 = st.st_covariance(px, pt, xy, tt, nugget, psill, rng, kappa, model, np.float64)          # [t h w, N]
    Kc = np.linalg.solve(K, c0.T)
    u = np.linalg.solve(K, np.ones(len(xy)))
    var = (nugget + psill) - (c0 * Kc.T).sum(1) + (1.0 - c0 @ u) ** 2 / u.sum()
    return var.reshape(t, h, w)
