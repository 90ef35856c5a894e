"""A float64 numpy / scipy restatement of the probabilistic verification: every sum the kernel of
csrc/eval_prob.hip accumulates, the scores derived from them, and the number of scored elements that lie within 1e-9 of a decision
edge (where a last-bit difference between scipy's and the device's erfc could move an element to another bin).  It imports nothing
from p2igan_bench.evaluation: the CPU tests check it against numerical integration and sampling, the GPU tests use it as the
arbiter."""
import numpy as np
from scipy.special import ndtr, ndtri

EDGE_EPS = 1e-9
DEFAULT_LEVELS = (0.5, 0.8, 0.9, 0.95)
DEFAULT_EDGES = tuple(float(v) for v in np.geomspace(0.5, 64.0, 12))


def transform(x, divide_by_3=True):
    x = np.maximum(np.asarray(x, dtype=np.float64), 0.001)
    if divide_by_3:
        x = x / 3.0
    return np.clip(10 ** np.minimum(x * 0.0625, 38.0) * 0.036, 0.0, 200.0)


def pixel_threshold(q, divide_by_3=True):
    """x_q with transform(x) >= q <=> x >= x_q (for transform(0.001) < q <= 200)."""
    return (48.0 if divide_by_3 else 16.0) * np.log10(q / 0.036)


def npdf(x):
    return np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def crps_plain(mu, sigma, y):
    z = (y - mu) / sigma
    return sigma * (z * (2.0 * ndtr(z) - 1.0) + 2.0 * npdf(z) - 1.0 / np.sqrt(np.pi))


def crps_censored(mu, sigma, y):
    """CRPS of max(0, N(mu, sigma^2)) for y >= 0 (Jordan, Krueger & Lerch 2019, the normal distribution left-censored at l)."""
    z, l = (y - mu) / sigma, -mu / sigma
    Fl = ndtr(l)
    return sigma * (-l * Fl * Fl + z * (2.0 * ndtr(z) - 1.0) + 2.0 * npdf(z) - 2.0 * npdf(l) * Fl
                    - (1.0 - ndtr(l * np.sqrt(2.0))) / np.sqrt(np.pi))


def crps_numeric(mu, sigma, y, censor, step, span=12.0):
    """The definition: the trapezoid rule on int (F(x) - 1[x >= y])^2 dx over a grid of the given step that holds y, 0 and the
    ends mu -+ span sigma as nodes' neighbours; the jump of the integrand at y (and of F at 0 under censoring) is met by splitting
    the integral there."""
    lo, hi = min(mu - span * sigma, y, 0.0) - 1.0, max(mu + span * sigma, y, 0.0) + 1.0
    cuts = sorted({lo, hi, y} | ({0.0} if censor else set()))
    total = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        n = max(2, int(np.ceil((b - a) / step)) + 1)
        x = np.linspace(a, b, n)
        mid = 0.5 * (a + b)
        F = ndtr((x - mu) / sigma)
        if censor and mid < 0.0:
            F = np.zeros_like(x)
        f = (F - (1.0 if mid >= y else 0.0)) ** 2
        total += float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(x)))
    return total


def pit_weights(P0, nb):
    """The non-randomised PIT of an atom of mass P0 at the censoring point: bin j gets |[j/nb, (j+1)/nb] n [0, P0]| / P0."""
    j = np.arange(nb, dtype=np.float64)
    if P0 <= 0.0:
        w = np.zeros(nb)
        w[0] = 1.0
        return w
    return np.clip(np.minimum((j + 1.0) / nb, P0) - j / nb, 0.0, None) / P0


def _interior_edge(v, nb):
    """|v - k| < EDGE_EPS for an integer 0 < k < nb: the ends 0 and nb decide nothing (the bin index is clamped)."""
    k = np.rint(v)
    return (np.abs(v - k) < EDGE_EPS) & (k > 0) & (k < nb)


def prob_sums(mu, var, y, sel=None, thresholds=(), levels=DEFAULT_LEVELS, sigma_edges=DEFAULT_EDGES, pit_bins=20, rel_bins=10,
              censor=True, divide_by_3=True):
    """mu, y [T, R, C] (already cropped; any real dtype), var the same shape or a float, sel [R, C] bool or None.  Returns the sums
    by name and ``edge_count``."""
    mu64 = np.asarray(mu, dtype=np.float64)
    y64 = np.asarray(y, dtype=np.float64)
    v64 = np.broadcast_to(np.asarray(var, dtype=np.float64), mu64.shape)
    ty = transform(np.asarray(y), divide_by_3)
    pick = np.ones(mu64.shape, bool) if sel is None else np.broadcast_to(np.asarray(sel, bool), mu64.shape)
    with np.errstate(invalid="ignore"):
        bad = np.isnan(mu64) | np.isnan(v64) | np.isnan(y64) | (v64 < 0.0)
        if censor:
            bad |= y64 < 0.0
    keep = pick & ~bad
    mu_, v_, y_, ty_ = mu64[keep], v64[keep], y64[keep], ty[keep]
    K, L, nb, rb = len(thresholds), len(levels), int(pit_bins), int(rel_bins)
    edges = np.asarray(sigma_edges, dtype=np.float64)
    NS = len(edges) + 1
    out = {"n": int(keep.sum()), "n_skipped": int((pick & bad).sum())}
    sg = np.sqrt(v_)
    pos = sg > 0.0
    out["n_zero_var"] = int((~pos).sum())
    mc = np.maximum(mu_, 0.0) if censor else mu_
    e = y_ - mc
    out["e"], out["ae"], out["e2"], out["s2"] = e.sum(), np.abs(e).sum(), (e * e).sum(), v_.sum()
    edge_count = 0
    with np.errstate(all="ignore"):
        z = np.where(pos, (y_ - mu_) / sg, 0.0)
        l = np.where(pos, -mu_ / sg, 0.0)
        safe = np.where(pos, sg, 1.0)
        c = crps_censored(mu_, safe, y_) if censor else crps_plain(mu_, safe, y_)
    out["crps"] = np.where(pos, c, np.abs(e)).sum()
    out["z"], out["z2"] = z[pos].sum(), (z[pos] * z[pos]).sum()
    # PIT
    pit = np.zeros(nb)
    u = np.where(pos, ndtr(z), np.where(y_ < mc, 0.0, np.where(y_ > mc, 1.0, 0.5)))
    atom = pos & (y_ == 0.0) if censor else np.zeros_like(pos)
    b = np.minimum(np.floor(u * nb).astype(np.int64), nb - 1)
    np.add.at(pit, b[~atom], 1.0)
    edge_count += int(_interior_edge(u[pos & ~atom] * nb, nb).sum())
    P0 = ndtr(l[atom])
    for p0 in P0:
        pit += pit_weights(float(p0), nb)
    # (the atom's weights are continuous in P0 -- bin m's share tends to 0 where P0 nb reaches m -- so P0 decides nothing sharply)
    out["pit"] = pit
    # central intervals
    out["inside"], out["width"] = np.zeros(L, np.int64), np.zeros(L)
    for k, lev in enumerate(levels):
        h = float(ndtri((1.0 + lev) / 2.0))
        lo, hi = mu_ - h * sg, mu_ + h * sg
        near = pos & (((np.abs(y_ - lo) < EDGE_EPS) & ((not censor) | (lo > 0.0))) | ((np.abs(y_ - hi) < EDGE_EPS) & ((not censor) | (hi > 0.0))))
        if censor:
            lo, hi = np.maximum(lo, 0.0), np.maximum(hi, 0.0)
        out["inside"][k] = int(((y_ >= lo) & (y_ <= hi)).sum())
        out["width"][k] = (hi - lo).sum()
        edge_count += int(near.sum())
    # spread-skill
    sb = (edges[None, :] <= sg[:, None]).sum(axis=1) if len(edges) else np.zeros(len(sg), np.int64)
    out["sb_n"] = np.bincount(sb, minlength=NS).astype(np.int64)
    out["sb_s2"] = np.bincount(sb, weights=v_, minlength=NS)
    out["sb_e2"] = np.bincount(sb, weights=e * e, minlength=NS)
    if len(edges):
        edge_count += int((np.abs(sg[:, None] - edges[None, :]) < EDGE_EPS).any(axis=1).sum())
    # exceedance
    out["o"], out["p"], out["brier"] = np.zeros(K, np.int64), np.zeros(K), np.zeros(K)
    out["rel_n"], out["rel_o"], out["rel_p"] = np.zeros((K, rb), np.int64), np.zeros((K, rb), np.int64), np.zeros((K, rb))
    tmc = transform(mc, divide_by_3)
    for k, q in enumerate(thresholds):
        xq = pixel_threshold(q, divide_by_3)
        with np.errstate(all="ignore"):
            p = np.where(pos, ndtr((mu_ - xq) / safe), (tmc >= q).astype(np.float64))
        o = ty_ >= q
        out["o"][k], out["p"][k], out["brier"][k] = int(o.sum()), p.sum(), ((p - o) ** 2).sum()
        rbin = np.minimum(np.floor(p * rb).astype(np.int64), rb - 1)
        out["rel_n"][k] = np.bincount(rbin, minlength=rb)
        out["rel_o"][k] = np.bincount(rbin, weights=o, minlength=rb).astype(np.int64)
        out["rel_p"][k] = np.bincount(rbin, weights=p, minlength=rb)
        edge_count += int(_interior_edge(p[pos] * rb, rb).sum()) + int((np.abs(ty_ - q) < EDGE_EPS).sum())
    out["edge_count"] = edge_count
    return out


def roc_area(rel_n, rel_o):
    """Trapezoid ROC area from a reliability table: warn when p falls in bin >= c, for c = rb .. 0."""
    n, o = np.asarray(rel_n, np.float64), np.asarray(rel_o, np.float64)
    ev, ne = o.sum(), (n - o).sum()
    if ev == 0 or ne == 0:
        return float("nan")
    pod = np.concatenate([[0.0], np.cumsum(o[::-1]) / ev])
    pofd = np.concatenate([[0.0], np.cumsum((n - o)[::-1]) / ne])
    return float(np.sum(0.5 * (pod[1:] + pod[:-1]) * np.diff(pofd)))


def prob_scores(s, thresholds=(), levels=DEFAULT_LEVELS, sigma_edges=DEFAULT_EDGES):
    """The reported scores from ``prob_sums``'s output, keyed as p2igan_bench.evaluation.prob reports them."""
    n, nz = s["n"], s["n"] - s["n_zero_var"]
    with np.errstate(all="ignore"):
        div = lambda a, b: float(a / b) if b else float("nan")      # noqa: E731
        res = {"n": n, "n_skipped": s["n_skipped"], "n_zero_var": s["n_zero_var"], "CRPS": div(s["crps"], n), "ME": div(s["e"], n),
               "MAE": div(s["ae"], n), "MSE": div(s["e2"], n), "RMSE": float(np.sqrt(div(s["e2"], n))), "mean_var": div(s["s2"], n), "z_mean": div(s["z"], nz),
               "MSDR": div(s["z2"], nz)}
        res["z_var"] = res["MSDR"] - res["z_mean"] ** 2
        res["coverage"] = {f"{lev:g}": div(s["inside"][k], n) for k, lev in enumerate(levels)}
        res["sharpness"] = {f"{lev:g}": div(s["width"][k], n) for k, lev in enumerate(levels)}
        tot = s["pit"].sum()
        res["pit"] = [div(v, tot) for v in s["pit"]]
        res["spread_skill"] = {"edges": [float(v) for v in sigma_edges], "count": [int(v) for v in s["sb_n"]],
                               "spread": [float(np.sqrt(div(a, c))) for a, c in zip(s["sb_s2"], s["sb_n"])],
                               "rmse": [float(np.sqrt(div(a, c))) for a, c in zip(s["sb_e2"], s["sb_n"])]}
        res["exceedance"] = {}
        for k, q in enumerate(thresholds):
            base = div(s["o"][k], n)
            bs = div(s["brier"][k], n)
            res["exceedance"][f"thr_{q:g}"] = {
                "base_rate": base, "mean_p": div(s["p"][k], n), "brier": bs,
                "bss": float(1.0 - bs / (base * (1.0 - base))) if n and 0.0 < base < 1.0 else float("nan"),
                "roc_area": roc_area(s["rel_n"][k], s["rel_o"][k]),
                "reliability": {"count": [int(v) for v in s["rel_n"][k]],
                                "mean_p": [div(a, c) for a, c in zip(s["rel_p"][k], s["rel_n"][k])],
                                "obs_freq": [div(a, c) for a, c in zip(s["rel_o"][k], s["rel_n"][k])]}}
    return res


def sample_censored(rng, mu, sigma):
    """One draw per element from max(0, N(mu, sigma^2))."""
    return np.maximum(0.0, mu + sigma * rng.standard_normal(np.shape(mu)))
