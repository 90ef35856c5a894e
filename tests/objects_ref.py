"""A numpy / plain-Python restatement of the object-based verification: the quantised rain Q = rint(R 2^24),
the level masks, connected components by flood fill in raster order (so an object's label is its smallest raster index by
construction), the integer moments as Python ints, and SAL per frame in scalar float64.  It imports nothing from
p2igan_bench.evaluation: the CPU tests check it against scipy and analytic cases, the GPU tests use it as the arbiter.  It also
holds the mask patterns and seeded inputs the tests share."""
import functools
import math

import numpy as np

SCALE = float(2 ** 24)
SAL_FACTOR = 1.0 / 15.0
SAL_FLOOR = 0.1


def transform(x, divide_by_3=True):
    x = np.maximum(np.asarray(x, dtype=np.float64), 0.001)
    if divide_by_3:
        x = x / 3.0
    return np.clip(10 ** np.minimum(x * 0.0625, 38.0) * 0.036, 0.0, 200.0)


def crop(a, size):
    h, w = a.shape[1:]
    if size > min(h, w):
        raise ValueError(f"crop size {size} exceeds input {h}x{w}")
    top, left = (h - size) // 2, (w - size) // 2
    return a[:, top:top + size, left:left + size]


def quantise(R):
    """int64 Q = rint(R 2^24) (np.rint rounds half to even), 0 for a NaN."""
    return np.where(np.isnan(R), 0.0, np.rint(R * SCALE)).astype(np.int64)


def masks(R, thresholds, factor=SAL_FACTOR, floor=SAL_FLOOR):
    """One [S, S] frame of rain rates -> the level masks [K + 1, S, S]: R >= q per threshold, then R >= max(factor Rmax, floor)."""
    with np.errstate(invalid="ignore"):
        rmax = np.max(R[~np.isnan(R)]) if (~np.isnan(R)).any() else 0.0
        rstar = max(factor * rmax, floor)
        return np.stack([R >= q for q in thresholds] + [R >= rstar])


def label(mask, connectivity=8):
    """[H, W] bool -> int64 labels: the smallest raster index y W + x of the pixel's component, -1 off the mask.  Flood fill from
    every unlabelled set pixel met in raster order."""
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8")
    H, W = mask.shape
    P = W + 2
    m = np.zeros((H + 2, P), np.uint8)
    m[1:-1, 1:-1] = mask
    todo = bytearray(m.tobytes())
    lab = [-1] * len(todo)
    steps = (-1, 1, -P, P) + ((-P - 1, -P + 1, P - 1, P + 1) if connectivity == 8 else ())
    for start in np.flatnonzero(m.ravel()).tolist():
        if not todo[start]:
            continue
        name = (start // P - 1) * W + (start % P - 1)
        todo[start] = 0
        stack = [start]
        while stack:
            p = stack.pop()
            lab[p] = name
            for s in steps:
                if todo[p + s]:
                    todo[p + s] = 0
                    stack.append(p + s)
    return np.array(lab, np.int64).reshape(H + 2, P)[1:-1, 1:-1]


@functools.lru_cache(maxsize=4096)
def _label_cached(key, shape, connectivity):
    return label(np.frombuffer(key, np.bool_).reshape(shape), connectivity)


def label_cached(mask, connectivity):
    mask = np.ascontiguousarray(mask, dtype=np.bool_)
    return _label_cached(mask.tobytes(), mask.shape, connectivity)


def objects_of(lab, Q):
    """The object table of one labelled frame: rows (label, area, sum Q, max Q, sum Q y, sum Q x) as Python ints, ascending label."""
    ys, xs = np.nonzero(lab >= 0)
    if not len(ys):
        return []
    order = np.argsort(lab[ys, xs], kind="stable")
    ys, xs = ys[order], xs[order]
    names, q = lab[ys, xs], Q[ys, xs]
    first = np.flatnonzero(np.concatenate([[True], names[1:] != names[:-1]]))
    cols = [names[first], np.add.reduceat(np.ones_like(q), first), np.add.reduceat(q, first), np.maximum.reduceat(q, first),
            np.add.reduceat(q * ys, first), np.add.reduceat(q * xs, first)]      # int64 throughout: exact
    return np.stack(cols, axis=1).tolist()


def records(pred, truth, S, thresholds, connectivity=8, factor=SAL_FACTOR, floor=SAL_FLOOR, divide_by_3=True):
    """pred, truth [T, H, W] on the 0-255 scale -> what the device returns, as int64 arrays: rec [T, 2, 5], lev [T, 2, L, 5],
    offsets [T 2 L + 1], table [N, 6]."""
    n = min(len(pred), len(truth))
    fields = [transform(crop(pred[:n], S), divide_by_3), transform(crop(truth[:n], S), divide_by_3)]
    L = len(thresholds) + 1
    ys, xs = np.mgrid[0:S, 0:S]
    rec, lev, counts, table = [], [], [], []
    for t in range(n):
        for R in (fields[0][t], fields[1][t]):
            Q = quantise(R)
            rec.append([int(Q.sum()), int((Q * ys).sum()), int((Q * xs).sum()), int(Q.max()), int(np.isnan(R).any())])
            for M in masks(R, thresholds, factor, floor):
                rows = objects_of(label_cached(M, connectivity), Q)
                lev.append([len(rows), int(M.sum()), int(Q[M].sum()), int((Q * ys)[M].sum()), int((Q * xs)[M].sum())])
                counts.append(len(rows))
                table += rows
    return {"rec": np.array(rec, np.int64).reshape(n, 2, 5), "lev": np.array(lev, np.int64).reshape(n, 2, L, 5),
            "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            "table": np.array(table, np.int64).reshape(-1, 6)}


def sal_of_frame(S, rec_p, rec_g, objs_p, objs_g):
    """SAL of one frame and level in scalar float64 from the integers: rec_* = (sum Q, sum Q y, sum Q x, ...) of the whole crop,
    objs_* = the object rows.  Returns (S, A, L, L1, L2)."""
    d = math.sqrt(2.0) * S
    Dp, Dg = rec_p[0] / (S * S), rec_g[0] / (S * S)
    A = (Dp - Dg) / (0.5 * (Dp + Dg))
    side = []
    for rec, objs in ((rec_p, objs_p), (rec_g, objs_g)):
        cy, cx = rec[1] / rec[0], rec[2] / rec[0]
        tot = sum(float(o[2]) for o in objs)
        V = sum(float(o[2]) * (float(o[2]) / float(o[3])) for o in objs) / tot
        r = sum(float(o[2]) * math.sqrt((o[4] / o[2] - cy) ** 2 + (o[5] / o[2] - cx) ** 2) for o in objs) / tot
        side.append((cy, cx, V, r))
    (py, px, Vp, rp), (gy, gx, Vg, rg) = side
    Sv = (Vp - Vg) / (0.5 * (Vp + Vg))
    L1 = math.sqrt((py - gy) ** 2 + (px - gx) ** 2) / d
    L2 = 2.0 * abs(rp - rg) / d
    return Sv, A, L1 + L2, L1, L2


def level_keys(thresholds):
    return [f"thr_{q:g}" for q in thresholds] + ["rel"]


def _mean(v):
    return float(np.mean(v)) if len(v) else float("nan")


def run_objects(preds, truth, crop_size, thresholds=(0.5, 2.0, 4.0, 8.0), connectivity=8, factor=SAL_FACTOR, floor=SAL_FLOOR,
                divide_by_3=True, frames_out=None):
    """preds {name: [T, H, W]}, truth [T, H, W] (arrays, one event) -> the product's dict."""
    S, keys, res = crop_size, level_keys(thresholds), {}
    for name, p in preds.items():
        r = records(p, truth, S, thresholds, connectivity, factor, floor, divide_by_3)
        rec, lev, off, table = r["rec"].tolist(), r["lev"].tolist(), r["offsets"].tolist(), r["table"].tolist()
        T, L = len(rec), len(keys)
        valid = [not (rec[t][0][4] or rec[t][1][4]) for t in range(T)]
        levels, per_frame = {}, {k: np.full((T, L), np.nan) for k in ("S", "A", "L", "L1", "L2")}
        for j, key in enumerate(keys):
            scores, kinds = [], {"scored": 0, "pred_only": 0, "truth_only": 0, "no_object": 0}
            pop = [{"n": [], "areas": [], "share": []}, {"n": [], "areas": [], "share": []}]
            for t in range(T):
                if not valid[t]:
                    continue
                objs = [table[off[(t * 2 + f) * L + j]:off[(t * 2 + f) * L + j + 1]] for f in (0, 1)]
                for f in (0, 1):
                    pop[f]["n"].append(len(objs[f]))
                    pop[f]["areas"] += [o[1] for o in objs[f]]
                    if objs[f]:
                        pop[f]["share"].append(max(o[1] for o in objs[f]) / sum(o[1] for o in objs[f]))
                kind = "scored" if objs[0] and objs[1] else "pred_only" if objs[0] else "truth_only" if objs[1] else "no_object"
                kinds[kind] += 1
                if kind == "scored":
                    s = sal_of_frame(S, rec[t][0], rec[t][1], objs[0], objs[1])
                    scores.append(s)
                    for k, v in zip(("S", "A", "L", "L1", "L2"), s):
                        per_frame[k][t, j] = v
            sc = np.array(scores, np.float64).reshape(-1, 5)
            m = {f"frames_{k}": v for k, v in kinds.items()}
            for i, k in enumerate(("S", "A", "L", "L1", "L2")):
                m[f"{k}_mean"] = _mean(sc[:, i])
                m[f"{k}_median"] = float(np.median(sc[:, i])) if len(sc) else float("nan")
            m["S_abs_mean"], m["A_abs_mean"] = _mean(np.abs(sc[:, 0])), _mean(np.abs(sc[:, 1]))
            for f, side in enumerate(("pred", "truth")):
                a = pop[f]["areas"]
                m[side] = {"objects_mean": _mean(pop[f]["n"]), "objects_max": max(pop[f]["n"], default=0),
                           "area_mean": sum(a) / len(a) if a else float("nan"),
                           "single_pixel_share": sum(1 for v in a if v == 1) / len(a) if a else float("nan"),
                           "largest_share_mean": _mean(pop[f]["share"])}
            levels[key] = m
        res[name] = {"levels": levels, "frames": T, "frames_skipped": T - sum(valid), "connectivity": connectivity,
                     "sal_factor": factor, "sal_floor": floor}
        if frames_out is not None:
            frames_out[name] = per_frame
    return res


def float_precondition(x, S, thresholds, factor=SAL_FACTOR, floor=SAL_FLOOR, divide_by_3=True):
    """Whether a float input's integers survive a transform that is off by up to 2 ulp (the device's pow against numpy's): no Q and
    no level decision of any crop pixel changes when every transformed value moves by -2 .. +2 ulp, the frame maximum included."""
    R = transform(crop(np.asarray(x), S), divide_by_3)
    lo = np.nextafter(np.nextafter(R, -np.inf), -np.inf)
    hi = np.nextafter(np.nextafter(R, np.inf), np.inf)
    ok = True
    for t in range(len(R)):
        if np.isnan(R[t]).any():
            continue
        ok &= bool((quantise(lo[t]) == quantise(hi[t])).all())
        for q in thresholds:
            ok &= bool(((lo[t] >= q) == (hi[t] >= q)).all())
        # the relative level: the lowest value against the highest bound and the other way round
        b_lo, b_hi = max(factor * lo[t].max(), floor), max(factor * hi[t].max(), floor)
        ok &= bool(((lo[t] >= b_hi) == (hi[t] >= b_lo)).all())
    return ok


# ---- mask patterns: every function returns [H, W] bool ----
def serpentine(H, W):
    """A one-pixel-wide path: every other row full, joined alternately at the right and the left end."""
    m = np.zeros((H, W), bool)
    m[::2] = True
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = True
    return m


def spiral(H, W):
    """A one-pixel-wide inward spiral with one-pixel gaps, walked from the top left corner: straight on while the cell ahead is free
    and the one after it is not part of the path, else a right turn; it ends where neither is possible."""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def free(y, x, dy, dx):
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= ny < H and 0 <= nx < W) or m[ny, nx]:
            return False
        return not (0 <= fy < H and 0 <= fx < W and m[fy, fx])
    while True:
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy
            if not free(y, x, dy, dx):
                return m
        y, x = y + dy, x + dx
        m[y, x] = True


def nested_u(H, W):
    """U shapes inside one another, joined only at the bottom row of each second one: labels merge late."""
    m = np.zeros((H, W), bool)
    k = 0
    while 2 * k < min(H, W) // 2:
        a = 2 * k
        m[a:H - a, a] = True
        m[a:H - a, W - 1 - a] = True
        m[H - 1 - a, a:W - a] = True
        k += 1
    return m


def comb(H, W):
    """Vertical teeth on every other column joined by the bottom row."""
    m = np.zeros((H, W), bool)
    m[:, ::2] = True
    m[:-1, 1::2] = False
    m[H - 1, :] = True
    return m


def checkerboard(H, W):
    return (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0


def diagonals(H, W, gap=3):
    d = np.subtract.outer(np.arange(H), np.arange(W))
    return (d % gap == 0) | ((np.add.outer(np.arange(H), np.arange(W)) % (2 * gap + 1)) == 0)


def straddlers(H, W, tile, top, left):
    """Small objects across every tile border and at every tile corner of a crop whose origin in the canvas is (top, left): 2 x 2
    blocks on the corners, bars across the borders between them, and diagonal pairs that only 8-connectivity joins."""
    m = np.zeros((H, W), bool)
    for by in range(tile, H - top, tile):
        for bx in range(tile, W - left, tile):
            y, x = top + by, left + bx
            if y + 1 < H and x + 1 < W:
                m[y - 1:y + 1, x - 1:x + 1] = True
    for by in range(tile, H - top, tile):
        y = top + by
        for x in range(left + 5, W - 3, 9):
            m[y - 1, x] = True
            m[y, x + ((x // 9) % 3 - 1)] = True      # below left, below, below right in turn
    for bx in range(tile, W - left, tile):
        x = left + bx
        for y in range(top + 5, H - 3, 9):
            m[y, x - 1] = True
            m[y + ((y // 9) % 3 - 1), x] = True
    return m


def random_mask(seed, H, W, density):
    return np.random.default_rng(seed).random((H, W)) < density


def pattern_masks(H, W, tile, top, left):
    """The named masks of the pattern tests on an H x W canvas whose crop, of H - 2 top x W - 2 left, starts at (top, left).  The
    winding shapes are drawn on the crop and continued outside it by repeating their edge pixels, the others cover the canvas: every
    one that touches the crop's edge goes on outside it."""
    h, w = H - 2 * top, W - 2 * left

    def inner(m):
        return np.pad(m, ((top, top), (left, left)), mode="edge")
    out = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool), "checkerboard": checkerboard(H, W),
           "diagonals": diagonals(H, W), "serpentine": inner(serpentine(h, w)), "serpentine_t": inner(serpentine(w, h).T),
           "spiral": inner(spiral(h, w)), "nested_u": inner(nested_u(h, w)), "comb": inner(comb(h, w)), "comb_up": inner(comb(h, w)[::-1]),
           "straddlers": straddlers(H, W, tile, top, left)}
    for i, dens in enumerate((0.3, 0.41, 0.5, 0.59, 0.7)):
        out[f"random_{dens}"] = random_mask(900 + i, H, W, dens)
    return out


# ---- seeded inputs: clip(gamma(0.3, 60), 0, 255) fields on the 0-255 scale; the smoother method is 0.5 g + 0.5 box3(g) ----
def field(seed, T, H, W):
    return np.clip(np.random.default_rng(seed).gamma(0.3, 60.0, size=(T, H, W)), 0.0, 255.0)


def box3(g):
    p = np.pad(g, ((0, 0), (1, 1), (1, 1)), mode="edge")
    return sum(p[:, dy:dy + g.shape[1], dx:dx + g.shape[2]] for dy in range(3) for dx in range(3)) / 9.0


def smoother(g):
    return 0.5 * g + 0.5 * box3(g)


def as_dtype(x, dtype):
    return np.rint(x).astype(np.uint8) if np.dtype(dtype) == np.uint8 else x.astype(dtype)


# ---- the cases the CPU and GPU tests share ----
CASE_THRESHOLDS = (0.5, 4.0)
CASE_SIZES = (1, 2, 7, 8, 33, 64, 128)
CASE_FRAMES = (1, 5)
DTYPES = (np.uint8, np.float32, np.float64)
SEED_BUMP = {}      # (S, T) -> an offset added to the seeds where float_precondition failed for the first draw (chosen on the CPU)


@functools.lru_cache(maxsize=None)
def exact_inputs(S, T):
    """(pred, truth) on the 0-255 scale as float64, larger than the crop and of different sizes with odd crop offsets (pred S + 17 x
    S + 13, truth S + 7 x S + 27); the prediction is another draw, smoothed, mixed with the truth inside the crop."""
    bump = SEED_BUMP.get((S, T), 0)
    truth = smoother(field(1000 + 10 * S + T + bump, T, S + 7, S + 27))
    own = field(2000 + 10 * S + T + bump, T, S + 17, S + 13)
    pred = own.copy()
    top, left = (own.shape[1] - S) // 2, (own.shape[2] - S) // 2
    pred[:, top:top + S, left:left + S] = 0.5 * crop(truth, S) + 0.5 * smoother(crop(own, S))
    return pred, truth


def pattern_events(S, tile=64):
    """(pred, truth, names): uint8 events on an S + 6 x S + 10 canvas (crop origin (3, 5)) whose frames are the pattern masks coded
    with rain rates that vary over the mask, so the levels cut different objects out of them; the prediction is the truth's next
    frame."""
    H, W = S + 6, S + 10
    pm = pattern_masks(H, W, tile, 3, 5)
    yy, xx = np.mgrid[0:H, 0:W]
    wet = (100 + (yy * 5 + xx * 3) % 120).astype(np.uint8)
    frames = np.stack([np.where(m, wet, 0).astype(np.uint8) for m in pm.values()])
    return np.roll(frames, -1, axis=0), frames, list(pm)


PATTERN_THRESHOLDS = (0.5, 30.0)
