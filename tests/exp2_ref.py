"""A numpy restatement of the benchmark's exp2 renders (reference experiments/exp2.py run_exp2 / _save_combo_gif with
experiments/io.py), written from the rules listed in DESIGN.md section 12, and the input recipes of tests/golden/exp2_cases.npz.
The CPU tests check the restatement against the fixture; the GPU tests use it as the arbiter for shapes the fixture does not hold.

``exp2(...)`` returns {"per_event": bool, "events": [{"key", "title", "labels", "gauge", "panels" [P, n, S, S] uint8, "points"
[K, 2] int (row, column), "point_idx" [n, K] uint8, "frames", "total", "range_line"}]}; ``compose(...)`` restates the device's
canvas kernel, the disc rule included."""
import json
import os

import numpy as np

from exp1_ref import thw, transform
from p2igan_bench.utils import seeded

NB, BAD = 142, 141
MAX_EVENTS, MAX_FRAMES = 20, 30


def cmap_tables():
    """(bounds [142], rgba [141, 4]) by the reference's recipe (experiments/exp2.py _build_paper_cmap)."""
    coarse = [0, 0.5, 1, 2, 4, 8, 16, 200]
    hexes = ["#000000", "#46327e", "#277f8e", "#4ac16d", "#a0da39", "#fde725", "#ffffff"]
    fine = []
    for i in range(7):
        seg = np.linspace(coarse[i], coarse[i + 1], 21, endpoint=False)
        fine += seg.tolist() if i == 0 else seg[1:].tolist()
    fine.append(coarse[-1])
    base = [[int(h[j:j + 2], 16) / 255.0 for j in (1, 3, 5)] for h in hexes]
    cols = []
    for c0, c1 in zip(base[:-1], base[1:]):
        for k in range(20):
            t = k / 19.0
            cols.append([(1 - t) * a + t * b for a, b in zip(c0, c1)])
    cols += [base[-1]] * (len(fine) - 1 - len(cols))
    return np.asarray(fine, float), np.concatenate([np.asarray(cols, float), np.ones((len(cols), 1))], axis=1)


def rgba_table():
    """index -> the bytes matplotlib paints: (rgba * 255) truncated; BAD is transparent black."""
    tab = np.zeros((256, 4), np.uint8)
    tab[:BAD] = (cmap_tables()[1] * 255).astype(np.uint8)
    return tab


def index(raw, divide_by_3=True):
    """np.digitize as BoundaryNorm(clip=True) uses it: clip(searchsorted_right(bounds, v) - 1, 0, 140); NaN -> BAD."""
    v = transform(raw, divide_by_3)
    idx = np.clip(np.searchsorted(cmap_tables()[0], v, side="right") - 1, 0, NB - 2)
    return np.where(np.isnan(v), BAD, idx).astype(np.uint8)


def crop_origin(h, w, size):
    if size > min(h, w):
        raise ValueError(f"crop size {size} exceeds input {h}x{w}")
    return (h - size) // 2, (w - size) // 2


def _crop(a, size):
    top, left = crop_origin(a.shape[1], a.shape[2], size)
    return a[:, top:top + size, left:left + size]


def _event(key, title_of, truth, obs, preds, mask, size, cap, mode):
    truth, obs = _crop(thw(truth), size)[:cap], _crop(thw(obs), size)[:cap]
    mask = np.asarray(mask).astype(bool)
    if mask.shape != (size, size):
        raise ValueError("mask shape")
    cur = truth.shape[0]
    srcs = {"Gauge" if mode == "gauge" else "Input": obs, "Radar" if mode == "gauge" else "Truth": truth}
    lengths = []
    for name, p in preds:
        p = thw(p)
        cur = min(p.shape[0], cur)              # align_length: the truth stays shortened for the methods after this one
        srcs[name] = _crop(p[:cur], size)[:cap]
        lengths.append(cur)
    total = min([cur] + lengths)
    frames = max(min(total, obs.shape[0]), 0)
    labels = list(srcs)
    panels = np.stack([index(srcs[lb][:frames]) for lb in labels]) if frames else np.zeros((len(labels), 0, size, size), np.uint8)
    points = np.argwhere(mask)
    return {"key": key, "title": title_of(total), "labels": labels, "gauge": [lb.lower() in ("input", "gauge") for lb in labels],
            "panels": panels, "points": points, "point_idx": panels[0][:, points[:, 0], points[:, 1]], "frames": frames, "total": total,
            "range_line": f"{key}: frames 1-{total} (count={total})"}


def exp2(preds, truth, observation, mask, crop_size, mode="radar"):
    if isinstance(truth, dict) and isinstance(observation, dict):
        keys = sorted(truth)                    # lexicographic: the reference's numeric pattern never matches
        if not keys:
            raise FileNotFoundError("No event groups found")
        events = []
        for key in keys[:MAX_EVENTS]:
            for src in (truth, observation):
                if key not in src:
                    raise FileNotFoundError(f"Missing event {key}")
            for a in (truth[key], observation[key]):
                crop_origin(*thw(a).shape[1:], crop_size)
            evp = []
            for name, src in preds.items():
                if isinstance(src, dict) and key not in src:
                    raise FileNotFoundError(f"Missing event {key}")
                evp.append((name, src[key] if isinstance(src, dict) else src))
            events.append(_event(key, lambda n, k=key: f"{k} | total frames {n}", truth[key], observation[key], evp, mask, crop_size,
                                 MAX_FRAMES, mode))
        return {"per_event": True, "events": events}
    ev = _event("event_01", lambda n: f"Event 01 | total frames {n}", truth, observation, list(preds.items()), mask, crop_size, None, mode)
    return {"per_event": False, "events": [ev]}


def compose(panels, zoom, gauge_bits, points, chrome, oy, ox, step, bg, edge):
    """The canvases [n, Hc, pitch] of p2i_exp2_compose.  The disc rule, in doubled coordinates: point (r, c) has its center at
    ((2 r + 1) zoom, (2 c + 1) zoom), panel pixel (y, x) lies at (2 y + 1, 2 x + 1), d2 is the squared distance; with R = 3 zoom,
    d2 <= (R - 2)^2 is the face (the panel's own index at the point; BAD shows the background index), (R - 2)^2 < d2 <= R^2 the edge
    ring; points are painted in order, the later one over the earlier."""
    P, n, S, _ = panels.shape
    side = S * zoom
    out = np.repeat(chrome[None], n, axis=0).copy()
    yy, xx = np.mgrid[0:side, 0:side]
    R = 3 * zoom
    for p in range(P):
        x0 = ox + p * step
        if (gauge_bits >> p) & 1:
            tile = np.full((n, side, side), bg, np.uint8)
            for r, c in np.asarray(points).reshape(-1, 2):
                d2 = (2 * yy + 1 - (2 * r + 1) * zoom) ** 2 + (2 * xx + 1 - (2 * c + 1) * zoom) ** 2
                face, ring = d2 <= (R - 2) ** 2, (d2 > (R - 2) ** 2) & (d2 <= R * R)
                for t in range(n):
                    col = panels[p, t, r, c]
                    tile[t][face] = col if col != BAD else bg
                    tile[t][ring] = edge
        else:
            tile = np.repeat(np.repeat(panels[p], zoom, axis=1), zoom, axis=2)
        out[:, oy:oy + side, x0:x0 + side] = tile
    return out


# ---- the fixture's cases: recipe -> (preds, truth, observation, mask, kwargs) --------------------------------------------------

CASES = [
    # keys whose lexicographic and numeric order differ; crop 8 from 11 x 9 (odd offsets); a longer f64 method; corner points and
    # two adjacent points; predictions with negatives, values above 200 mm/h and NaN
    {"name": "path_order", "form": "path", "mode": "radar", "crop": 8, "keys": ["event_2", "event_10"], "events": [[5, 11, 9], [4, 11, 9]],
     "truth": "u8", "points": [[0, 0], [0, 7], [3, 3], [3, 4], [7, 0], [7, 7]],
     "methods": {"gan": {"seed": 11, "noise": 10.0, "over": 0.03, "nan": 0.03, "neg_every": 7},
                 "stdk": {"seed": 12, "noise": 25.0, "dtype": "f64", "extra": 2}}},
    # 33 frames: the 30-frame cap; one mask point
    {"name": "path_cap", "form": "path", "mode": "radar", "crop": 8, "keys": ["event_01"], "events": [[33, 10, 10]], "truth": "u8",
     "points": [[4, 5]], "methods": {"gan": {"seed": 21, "noise": 12.0}}},
    # two methods shorten the truth in turn, the third is longer; gauge labels; a mask without a point; the observation is the
    # shortest of all (the GIF holds fewer frames than the range line counts)
    {"name": "path_shorten", "form": "path", "mode": "gauge", "crop": 8, "keys": ["event_01"], "events": [[6, 9, 11]], "truth": "u8",
     "obs_t": [2], "points": [],
     "methods": {"a": {"seed": 31, "noise": 8.0, "t": [4]}, "b": {"seed": 32, "noise": 8.0, "t": [3]}, "c": {"seed": 33, "noise": 8.0, "t": [8]}}},
    {"name": "path_missing", "form": "path", "mode": "radar", "crop": 8, "keys": ["event_01", "event_02"], "events": [[2, 9, 9], [2, 9, 9]],
     "truth": "u8", "points": [[1, 1]], "methods": {"gan": {"seed": 41, "noise": 8.0, "skip": [1]}}},
    # T = 1, 5-D inputs, f32 truth with NaN and negatives
    {"name": "array_t1", "form": "array", "mode": "radar", "crop": 8, "keys": ["event_01"], "events": [[1, 11, 9]], "truth": "f32",
     "five_d": True, "mask_frac": 0.15, "methods": {"gan": {"seed": 51, "noise": 10.0, "dtype": "f64", "nan": 0.05, "neg_every": 5}}},
    # f64 truth; no 30-frame cap in the array form (T = 32); a method shorter and one longer
    {"name": "array_long", "form": "array", "mode": "gauge", "crop": 8, "keys": ["event_01"], "events": [[32, 8, 8]], "truth": "f64",
     "mask_frac": 0.1, "methods": {"short": {"seed": 61, "noise": 10.0, "t": [31]}, "long": {"seed": 62, "noise": 10.0, "over": 0.05, "t": [34]}}},
]


def _floaty(seed, base, kind):
    """A float32 / float64 field near a uint8 one, with a NaN, negatives and a value far above the scale."""
    x = seeded.exp1_pred(seed, base, 6.0).astype(np.float32 if kind == "f32" else np.float64)
    x.reshape(-1)[3::11] = -4.5
    x.reshape(-1)[5::13] = np.nan
    x.reshape(-1)[7::17] = 900.0
    return x


def build_case(c):
    """(preds, truth, observation, mask, kwargs) of a recipe.  The path form's sources are dicts {key: [T, 1, H, W]}: write them
    with ``write_zarrs`` to get the zarr paths."""
    truths, obss = {}, {}
    for i, (key, (t, h, w)) in enumerate(zip(c["keys"], c["events"])):
        g = seeded.exp1_truth(5000 + i, t, h, w)
        o = seeded.exp1_truth(6000 + i, c["obs_t"][i] if "obs_t" in c else t, h, w)
        if c["truth"] != "u8":
            g, o = _floaty(5100 + i, g, c["truth"]), _floaty(6100 + i, o, c["truth"])
        truths[key], obss[key] = g, o
    preds = {}
    for name, m in c["methods"].items():
        evs = {}
        for i, key in enumerate(c["keys"]):
            if i in m.get("skip", []):
                continue
            g = truths[key] if c["truth"] == "u8" else seeded.exp1_truth(5000 + i, *c["events"][i])
            t = m["t"][i] if "t" in m else g.shape[0] + m.get("extra", 0)
            p = seeded.exp1_pred(m["seed"] * 100 + i, g, m.get("noise", 10.0), 0.0, m.get("over", 0.0), m.get("nan", 0.0), t=t)
            if m.get("dtype") == "f64":
                p = p.astype(np.float64) + 1e-7
            if "neg_every" in m:
                p.reshape(-1)[2::m["neg_every"]] = -3.25
            evs[key] = p
        preds[name] = evs
    s = c["crop"]
    if "points" in c:
        mask = np.zeros((s, s), bool)
        for y, x in c["points"]:
            mask[y, x] = True
    else:
        mask = seeded.exp1_mask(7000 + s, s, s, c["mask_frac"])
    kw = {"crop_size": s, "mode": c["mode"]}
    if c["form"] == "path":
        return preds, truths, obss, mask, kw
    k = c["keys"][0]
    five = (lambda a: a[None]) if c.get("five_d") else (lambda a: a)
    return {n: five(e[k]) for n, e in preds.items()}, five(truths[k]), five(obss[k]), mask, kw


def write_zarrs(root, preds, truth, observation):
    """The path form's dicts as zarr groups under root: (preds paths, truth path, observation path)."""
    from p2igan_bench.data import zarr_lite

    def put(name, events):
        path = os.path.join(str(root), name + ".zarr")
        g = zarr_lite.Group(path, "w")
        for k, v in events.items():
            g.create_dataset(k, v, chunks=v.shape)
        return path
    return {n: put("m_" + n, e) for n, e in preds.items()}, put("truth", truth), put("obs", observation)


def recipe_json(c):
    return json.dumps(c, sort_keys=True)
