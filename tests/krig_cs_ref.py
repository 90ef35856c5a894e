"""numpy / scipy restatement of the conditional simulation of ordinary kriging (csrc/krig_cs.hip), on top of
classical_ref.py and krig_uq_ref.py.  `dtype` selects the arithmetic (float64: the reference of the GPU tests; float32: Box-Muller,
amplitude, scipy.fft.fft2 on complex64, Cholesky and products in fp32, the yardstick of their error bound).  The spectrum is float64
always, as on the device, and the amplitude is stored as fp32.

    b[j, k] = C(sqrt(dj^2 + dk^2)) + nugget [dj = dk = 0] on the torus Sy x Sx = (e H) x (e W); lambda = Re DFT2(b)
    A = sqrt(lambda+ / (Sy Sx)), lambda+ = max(lambda, 0) sum lambda / sum max(lambda, 0); rho = sum max(-lambda, 0) / sum |lambda|
    xi = Box-Muller of Philox4x32-10(counter (j Sx + k, q, stream lo, hi), key (seed lo, hi)); Y = DFT2(A xi)
    U_2q = Re Y[:H, :W], U_2q+1 = Im Y[:H, :W]; r = z - U(gauges), v = K^-1 r, mu = 1^T v / s, alpha = v - mu u
    Z_m(p) = U_m(p) + mu + sum_i alpha_i c0(p, i), written as z_i on a gauge pixel"""
import numpy as np
import scipy.fft
import scipy.linalg

import classical_ref as cr
import krig_uq_ref as ur

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011) in uint64 arithmetic.  counter: 4 arrays (or ints) of 32-bit words that
    broadcast together, key: 2.  Returns the 4 output words as uint64 arrays below 2^32."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = (np.uint64(int(v) & 0xFFFFFFFF) for v in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def noise(seed, stream, q, Sy, Sx, dtype=np.float64):
    """xi (len(q), Sy, Sx) complex of the member pairs q (an int or a sequence) of frame id `stream` (a 64-bit integer)."""
    ft = np.dtype(dtype).type
    q = np.atleast_1d(np.asarray(q, dtype=np.uint64))
    stream, seed = int(stream) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    idx = np.arange(Sy * Sx, dtype=np.uint64)[None, :]
    r = philox4x32_10((idx, q[:, None], stream & 0xFFFFFFFF, stream >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    r0, r1 = r[0], r[1]
    sc = ft(2.0 ** -32)
    low = r0 < np.uint64(2 ** 31)
    with np.errstate(divide="ignore"):
        lg = np.where(low, np.log((r0 + np.uint64(1)).astype(ft) * sc), np.log1p(-((np.uint64(2 ** 32 - 1) - r0).astype(ft) * sc)))
    rad = np.sqrt(ft(-2.0) * lg.astype(ft))
    ang = ft(2.0 * np.pi) * (r1.astype(ft) * sc)
    xi = rad * np.cos(ang) + 1j * (rad * np.sin(ang))
    return xi.reshape(len(q), Sy, Sx).astype(np.complex64 if ft is np.float32 else np.complex128)


def torus(h, w, embed):
    if embed not in (2, 3, 4):
        raise ValueError(f"embed must be 2, 3 or 4 (got {embed})")
    if max(embed * h, embed * w) > 512:
        raise ValueError(f"the torus {embed * h} x {embed * w} exceeds 512 on a side")
    return embed * h, embed * w


def spectrum(params, model, h, w, embed=2):
    """(A (Sy, Sx) float64, rho) of one sample, float64 from the fp32-rounded params (nugget, psill, range)."""
    nugget, psill, rng = (float(np.float32(p)) for p in params)
    Sy, Sx = torus(h, w, embed)
    dj = np.minimum(np.arange(Sy), Sy - np.arange(Sy))[:, None]
    dk = np.minimum(np.arange(Sx), Sx - np.arange(Sx))[None, :]
    d2 = dj * dj + dk * dk
    base = psill * (1.0 - cr.g_of(np.sqrt(d2.astype(np.float64)) / rng, model)) + nugget * (d2 == 0)
    lam = np.fft.fft2(base).real
    pos, neg = np.maximum(lam, 0.0), np.maximum(-lam, 0.0)
    lam_plus = pos * (lam.sum() / pos.sum())
    return np.sqrt(lam_plus / (Sy * Sx)), neg.sum() / (pos.sum() + neg.sum())


def unconditional(A, seed, stream, members, h, w, dtype=np.float64):
    """U (members, h, w): the pairs' real and imaginary parts, the last imaginary part dropped for odd `members`."""
    ft = np.dtype(dtype).type
    Sy, Sx = A.shape
    npairs = (members + 1) // 2
    xi = noise(seed, stream, np.arange(npairs), Sy, Sx, ft)
    a = A.astype(np.float32).astype(ft)                       # the amplitude is stored as fp32
    Y = scipy.fft.fft2((a[None] * xi).astype(xi.dtype), axes=(1, 2))[:, :h, :w]
    U = np.empty((2 * npairs, h, w), ft)
    U[0::2], U[1::2] = Y.real, Y.imag
    return U[:members]


def members_frame(xy, z, h, w, params, model, members, seed, stream, embed=2, dtype=np.float64, A=None):
    """The conditional members (members, h, w) of one frame with gauges xy (N, 2), values z and params (nugget, psill, range)."""
    ft = np.dtype(dtype).type
    nugget, psill, rng = params
    if A is None:
        A = spectrum(params, model, h, w, embed)[0]
    U = unconditional(A, seed, stream, members, h, w, ft)
    K = cr.covariance(xy, xy, nugget, psill, rng, model, ft)
    cf = scipy.linalg.cho_factor(K, lower=True)
    u = scipy.linalg.cho_solve(cf, np.ones(len(z), ft)).astype(ft)
    r = (z.astype(ft)[:, None] - U[:, xy[:, 0], xy[:, 1]].T).astype(ft)          # [N, members]
    v = scipy.linalg.cho_solve(cf, r).astype(ft)
    mu = v.sum(0, dtype=ft) / u.sum(dtype=ft)
    alpha = (v - mu[None, :] * u[:, None]).astype(ft)
    c0 = cr.covariance(cr.grid(h, w), xy, nugget, psill, rng, model, ft).astype(ft)
    Z = (U.reshape(members, h * w) + mu[:, None] + (c0 @ alpha).T).astype(ft).reshape(members, h, w)
    Z[:, xy[:, 0], xy[:, 1]] = z.astype(ft)[None, :]
    return Z


def ensemble(masked, masks, variogram, members, seed=0, streams=None, embed=2, dtype=np.float64):
    """masked, masks: (B, T, 1, H, W).  Returns (ens (B, T, members, H, W), rho (B,)) with the frame rules: NaN in every member over a
    frame without gauges or of a degenerate fitted sample (rho NaN there too).  streams (B, T) defaults to b T + t."""
    B, T, _, H, W = masked.shape
    ft = np.dtype(dtype).type
    ens = np.full((B, T, members, H, W), np.nan, ft)
    rho = np.full(B, np.nan)
    if streams is None:
        streams = np.arange(B * T, dtype=np.int64).reshape(B, T)
    for b in range(B):
        model, params = ur.sample_params(masked, masks, b, variogram)
        if params is None:
            continue
        A, rho[b] = spectrum(params, model, H, W, embed)
        for t in range(T):
            xy, z = cr.gauges(masked[b, t, 0], masks[b, t, 0])
            if len(z):
                ens[b, t] = members_frame(xy, z, H, W, params, model, members, seed, int(streams[b, t]), embed, ft, A)
    return ens, rho


def posterior_covariance(xy, h, w, params, model):
    """The analytic ordinary-kriging posterior covariance (h w, h w), fp64: Cgg - L C0^T - C0 L^T + L K L^T with L the kriging
    weights of every pixel."""
    nugget, psill, rng = params
    g = cr.grid(h, w)
    K = cr.covariance(xy, xy, nugget, psill, rng, model, np.float64)
    C0 = cr.covariance(g, xy, nugget, psill, rng, model, np.float64)
    Cgg = cr.covariance(g, g, nugget, psill, rng, model, np.float64)
    lam = cr.krige_frame_primal(xy, np.zeros(len(xy), np.float32), h, w, params, model)[1]
    return Cgg - lam @ C0.T - C0 @ lam.T + lam @ K @ lam.T
