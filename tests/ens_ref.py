"""An fp64 numpy restatement of the ensemble scores, written from the definitions: double loops over member
pairs and over pixel pairs (no sorted shortcuts), the tie rule in Python integers.  tests/test_ens_cpu.py pins it against closed
forms; tests/test_ens_gpu.py uses it as the reference of csrc/eval_ens.hip.  Inputs are the CROPPED arrays: members [M, T, rows,
cols], truth [T, rows, cols], sel [rows, cols] bool or None."""
import math

import numpy as np

import prob_ref as pr

DEFAULT_EDGES = pr.DEFAULT_EDGES
DEFAULT_OFFSETS = tuple(o for h in (1, 2, 4, 8) for o in ((0, h), (h, 0), (h, h), (h, -h)))
UNIT = 1 << 32


def box_values(a, sel, s):
    """(values [..., rows // s, cols // s], has [rows // s, cols // s]): the mean over each box's selected pixels, summed in raster
    order; ``has`` is False for a box without a selected pixel (its value is meaningless)."""
    a = np.asarray(a, np.float64)
    rows, cols = a.shape[-2:]
    sel = np.ones((rows, cols), bool) if sel is None else np.asarray(sel, bool)
    br, bc = rows // s, cols // s
    total = np.zeros(a.shape[:-2] + (br, bc))
    count = np.zeros((br, bc))
    for dy in range(s):
        for dx in range(s):
            sub = a[..., dy:br * s:s, dx:bc * s:s]
            pick = sel[dy:br * s:s, dx:bc * s:s]
            total = total + np.where(pick, sub, 0.0)
            count = count + pick
    with np.errstate(all="ignore"):
        return total / np.where(count > 0, count, 1.0), count > 0


def point_scores(x, y):
    """One point, M member values x and the truth y, by the definitions: (CRPS, CRPS_fair, mean, s2, b, k).  CRPS_fair and s2 are NaN
    for one member."""
    x = [float(v) for v in x]
    M = len(x)
    a = sum(abs(v - y) for v in x) / M
    S = 0.0
    for i in range(M):
        for j in range(M):
            S += abs(x[i] - x[j])
    mean = sum(sorted(x)) / M
    s2 = sum((v - mean) ** 2 for v in sorted(x)) / (M - 1) if M > 1 else float("nan")
    fair = a - S / (2.0 * M * (M - 1)) if M > 1 else float("nan")
    return a - S / (2.0 * M * M), fair, mean, s2, sum(v < y for v in x), sum(v == y for v in x)


def tie_shares(b, k, M):
    """The point's weight 2^32 over the M + 1 bins, in integers: bins b .. b + k get floor(2^32 / (k + 1)) each, bin b the remainder."""
    q, r = divmod(UNIT, k + 1)
    h = [0] * (M + 1)
    for i in range(b, b + k + 1):
        h[i] += q
    h[b] += r
    return h


def crps_integral(x, y):
    """integral of (F_ens(t) - 1[y <= t])^2 dt, piecewise between the sorted breakpoints."""
    pts = sorted([float(v) for v in x] + [float(y)])
    M, tot = len(x), 0.0
    for lo, hi in zip(pts[:-1], pts[1:]):
        mid = 0.5 * (lo + hi)
        F = sum(v <= mid for v in x) / M
        tot += (F - (1.0 if y <= mid else 0.0)) ** 2 * (hi - lo)
    return tot


def ens_sums(members, truth, sel=None, box=1, xq=(), sigma_edges=DEFAULT_EDGES):
    """The per-point record's sums by name (the keys of ensemble.unpack_record), over all frames."""
    members, truth = np.asarray(members, np.float64), np.asarray(truth, np.float64)
    M = members.shape[0]
    xv, has = box_values(members, sel, box)             # [M, T, br, bc]
    yv, _ = box_values(truth, sel, box)
    T = truth.shape[0]
    has = np.broadcast_to(has, (T,) + has.shape)
    good = has & np.isfinite(yv) & np.isfinite(xv).all(axis=0)
    x = xv[:, good]                                     # [M, n]
    y = yv[good]
    n = int(good.sum())
    K, NS = len(xq), len(sigma_edges) + 1
    absd = np.zeros(n)
    for i in range(M):
        absd += np.abs(x[i] - y)
    absd /= M
    S = np.zeros(n)
    for i in range(M):
        for j in range(M):
            S += np.abs(x[i] - x[j])
    xs = np.sort(x, axis=0)
    sx = np.zeros(n)
    for i in range(M):
        sx += xs[i]
    mean = sx / M
    ss = np.zeros(n)
    for i in range(M):
        ss += (xs[i] - mean) ** 2
    s2 = ss / (M - 1) if M > 1 else np.zeros(n)
    e = mean - y
    crps = absd - S / (2.0 * M * M)
    fair = absd - S / (2.0 * M * (M - 1)) if M > 1 else np.zeros(n)
    b = (x < y).sum(axis=0)
    k = (x == y).sum(axis=0)
    hist = [0] * (M + 1)
    for bi, ki in zip(b.tolist(), k.tolist()):
        for i, v in enumerate(tie_shares(bi, ki, M)):
            hist[i] += v
    sg = np.sqrt(s2)
    edges = np.asarray(sigma_edges, np.float64)
    sb = (edges[None, :] <= sg[:, None]).sum(axis=1) if len(edges) else np.zeros(n, int)
    edge_count = int(sum(np.sum(np.abs(sg - ed) <= 1e-9 * ed) for ed in edges))
    res = {"crps": crps.sum(), "crps_fair": fair.sum(), "e": e.sum(), "ae": np.abs(e).sum(), "e2": (e * e).sum(), "s2": s2.sum(),
           "n": n, "n_skipped": int((has & ~good).sum()), "rank": np.array(hist, dtype=np.int64),
           "sb_n": np.array([(sb == j).sum() for j in range(NS)], dtype=np.int64),
           "sb_s2": np.array([s2[sb == j].sum() for j in range(NS)]), "sb_e2": np.array([(e * e)[sb == j].sum() for j in range(NS)]),
           "p": np.zeros(K), "brier": np.zeros(K), "o": np.zeros(K, np.int64), "rel_n": np.zeros((K, M + 1), np.int64),
           "rel_o": np.zeros((K, M + 1), np.int64)}
    for q, t in enumerate(xq):
        c = (x >= t).sum(axis=0)
        o = y >= t
        p = c / M
        res["p"][q], res["brier"][q], res["o"][q] = p.sum(), ((p - o) ** 2).sum(), o.sum()
        for ci in range(M + 1):
            res["rel_n"][q, ci] = (c == ci).sum()
            res["rel_o"][q, ci] = ((c == ci) & o).sum()
        edge_count += int(np.sum(np.abs(x - t) <= 1e-9 * t) + np.sum(np.abs(y - t) <= 1e-9 * t))
    res["edge_count"] = edge_count
    return res


def _div(a, b):
    return float(a) / float(b) if b else float("nan")


def ens_scores(s, M, thresholds=(), sigma_edges=DEFAULT_EDGES):
    """The reported figures of one box size from the sums."""
    n, nan = s["n"], float("nan")
    with np.errstate(all="ignore"):
        mse = _div(s["e2"], n)
        var = _div(s["s2"], n) if M > 1 else nan
        hist = [int(v) for v in s["rank"]]
        tot = float(sum(hist))
        f = [_div(v, tot) for v in hist]
        res = {"M": M, "n": n, "n_skipped": s["n_skipped"], "CRPS": _div(s["crps"], n), "CRPS_fair": _div(s["crps_fair"], n) if M > 1 else nan,
               "ME": _div(s["e"], n), "MAE": _div(s["ae"], n), "MSE": mse, "RMSE": math.sqrt(mse) if n else nan, "mean_var": var,
               "spread_skill_ratio": math.sqrt((M + 1) / M * var / mse) if n and M > 1 and mse > 0 else nan,
               "rank_histogram": f, "outlier_share": f[0] + f[-1], "reliability_index": float(sum(abs(v - 1.0 / (M + 1)) for v in f)),
               "spread_skill": {"edges": [float(v) for v in sigma_edges], "count": [int(v) for v in s["sb_n"]],
                                "spread": [float(np.sqrt(_div(a, c))) for a, c in zip(s["sb_s2"], s["sb_n"])],
                                "rmse": [float(np.sqrt(_div(a, c))) for a, c in zip(s["sb_e2"], s["sb_n"])]},
               "exceedance": {}}
        for k, q in enumerate(thresholds):
            base, bs = _div(s["o"][k], n), _div(s["brier"][k], n)
            res["exceedance"][f"thr_{q:g}"] = {
                "base_rate": base, "mean_p": _div(s["p"][k], n), "brier": bs,
                "bss": 1.0 - bs / (base * (1.0 - base)) if n and 0.0 < base < 1.0 else nan,
                "roc_area": pr.roc_area(s["rel_n"][k], s["rel_o"][k]),
                "reliability": {"count": [int(v) for v in s["rel_n"][k]],
                                "obs_freq": [_div(a, c) for a, c in zip(s["rel_o"][k], s["rel_n"][k])]}}
    return res


def valid_pixels(members, truth, sel=None):
    """[T, rows, cols] bool: selected and finite in the truth and in every member."""
    members, truth = np.asarray(members, np.float64), np.asarray(truth, np.float64)
    ok = np.isfinite(truth) & np.isfinite(members).all(axis=0)
    return ok if sel is None else ok & np.asarray(sel, bool)[None]


def energy_frames(members, truth, sel=None):
    """[T, 4]: per frame (d, ES, ES_fair, (1/M) sum |X_i - y|) over the valid pixels; a double loop over the member pairs."""
    members, truth = np.asarray(members, np.float64), np.asarray(truth, np.float64)
    M, T = members.shape[:2]
    ok = valid_pixels(members, truth, sel)
    out = np.zeros((T, 4))
    for t in range(T):
        X, y = members[:, t][:, ok[t]], truth[t][ok[t]]
        t1 = sum(math.sqrt(float(np.sum((X[i] - y) ** 2))) for i in range(M)) / M
        pairs = 0.0
        for i in range(M):
            for j in range(M):
                pairs += math.sqrt(float(np.sum((X[i] - X[j]) ** 2)))
        out[t] = (ok[t].sum(), t1 - pairs / (2.0 * M * M), t1 - pairs / (2.0 * M * (M - 1)) if M > 1 else np.nan, t1)
    return out


def variogram_frames(members, truth, sel=None, offsets=DEFAULT_OFFSETS):
    """[T, nof, 2]: per frame and offset (V_o, n_o) over the pixel pairs (a, a + o) inside the crop whose two pixels are valid."""
    members, truth = np.asarray(members, np.float64), np.asarray(truth, np.float64)
    M, T, rows, cols = members.shape
    ok = valid_pixels(members, truth, sel)
    out = np.zeros((T, len(offsets), 2))
    for oi, (dy, dx) in enumerate(offsets):
        ya, yb = max(0, -dy), min(rows, rows - dy)
        xa, xb = max(0, -dx), min(cols, cols - dx)
        if ya >= yb or xa >= xb:
            continue
        A = (slice(None), slice(ya, yb), slice(xa, xb))
        B = (slice(None), slice(ya + dy, yb + dy), slice(xa + dx, xb + dx))
        both = ok[A] & ok[B]
        with np.errstate(all="ignore"):
            gm = np.zeros(both.shape)
            for m in range(M):
                gm = gm + np.sqrt(np.abs(members[m][A] - members[m][B]))
            term = (np.sqrt(np.abs(truth[A] - truth[B])) - gm / M) ** 2
        for t in range(T):
            out[t, oi] = (term[t][both[t]].sum(), both[t].sum())
    return out


def energy_scores(frames):
    frames = np.asarray(frames, np.float64).reshape(-1, 4)
    f = frames[frames[:, 0] > 0]
    return {"n_frames": len(f), "n_frames_skipped": len(frames) - len(f),
            "ES_norm": float(np.mean(f[:, 1] / np.sqrt(f[:, 0]))) if len(f) else float("nan"),
            "ES_fair_norm": float(np.mean(f[:, 2] / np.sqrt(f[:, 0]))) if len(f) else float("nan")}


def variogram_scores(frames, offsets=DEFAULT_OFFSETS):
    frames = np.asarray(frames, np.float64).reshape(-1, len(offsets), 2)
    V, n = frames[:, :, 0].sum(axis=0), frames[:, :, 1].sum(axis=0)
    mean = [_div(a, c) for a, c in zip(V, n)]
    w = [1.0 / math.hypot(dy, dx) for dy, dx in offsets]
    have = [(wi, m) for wi, m in zip(w, mean) if not math.isnan(m)]
    return {"mean": mean, "pairs": [int(v) for v in n], "VS": float(sum(wi * m for wi, m in have)) if have else float("nan")}
