"""A numpy restatement of the benchmark's exp3 numbers (reference experiments/exp3.py run_exp3 with experiments/io.py), written from
the rules listed in DESIGN.md section 11, and the input recipes of tests/golden/exp3_cases.npz.  The CPU tests check the restatement
against the fixture; the GPU tests use it as the arbiter at sizes the fixture does not hold.

``exp3(...)`` returns {"metrics": {NSE_<name>: float}, "nse": {name: [per-event NSE]} (dict input only), "pool": {name: int},
"x" / "y": {name: sampled observed / predicted}, "fit_scatter" / "fit_residual": {name: (slope, intercept, r)} (>= 2 points),
"freq_truth": [64] and "freq": {name: [64]} (dict input only; a method without a finite value has none)}; "x" and "y" are empty
when the truth stack has no finite value."""
import json

import numpy as np

from exp1_ref import crop, thw, transform
from p2igan_bench.utils import seeded

SHAPE_ERROR = "Expected [T,H,W], got shape (0,)"


def _nse(p, g):
    ok = np.isfinite(p) & np.isfinite(g)
    if not ok.any():
        return float("nan")
    p, g = p[ok], g[ok]
    return float(1.0 - np.sum((p - g) ** 2) / (np.sum((g - g.mean()) ** 2) + 1e-10))


def _fit(x, y):
    xm, ym = x.mean(), y.mean()
    sxx, syy, sxy = ((x - xm) ** 2).mean(), ((y - ym) ** 2).mean(), ((x - xm) * (y - ym)).mean()
    r = 0.0 if sxx == 0.0 or syy == 0.0 else float(np.clip(sxy / np.sqrt(sxx * syy), -1.0, 1.0))
    slope = sxy / sxx
    return float(slope), float(ym - slope * xm), r


def _freq(v):
    v = v[np.isfinite(v)]
    v = v[(v >= 0.0) & (v <= 32.0)]
    h = np.bincount(np.minimum(np.floor(v * 2.0).astype(np.int64), 63), minlength=64)
    return h / max(int(h.sum()), 1)


def exp3(preds, truth, mask, mode, crop_size, max_points=2000, seed=42):
    mask = np.asarray(mask).astype(bool)
    if mode not in ("radar", "gauge"):
        raise ValueError(f"Unknown mode: {mode}")
    if mask.shape != (crop_size, crop_size):
        raise ValueError(f"Mask shape {mask.shape} != data shape {(crop_size, crop_size)}")
    sel = (~mask if mode == "radar" else mask).ravel()
    names = list(preds)
    out = {"metrics": {}, "nse": {}, "pool": {}, "x": {}, "y": {}, "fit_scatter": {}, "fit_residual": {}, "freq": {}}
    per_event = isinstance(truth, dict)
    if per_event:
        if any(not isinstance(s, dict) for s in preds.values()):
            raise ValueError(SHAPE_ERROR)
        truth_stack, pieces = [], {n: [] for n in names}
        out["nse"] = {n: [] for n in names}
        for k in truth:
            if truth[k] is None:
                continue
            g = crop(transform(truth[k]), crop_size)
            truth_stack.append(g)
            cur = g
            for n in names:
                if preds[n].get(k) is None:
                    continue
                p = thw(transform(preds[n][k]))
                m = min(p.shape[0], cur.shape[0])
                p, cur = crop(p[:m], crop_size), cur[:m]           # the truncation carries over to the next methods
                fr = np.array([_nse(p[i].ravel()[sel], cur[i].ravel()[sel]) for i in range(m)], dtype=np.float64)
                fr = np.where(np.isfinite(fr), np.maximum(fr, 0.0), np.nan)
                ok = np.isfinite(fr)
                out["nse"][n].append(float(fr[ok].sum() / ok.sum()) if ok.any() else float("nan"))
                pieces[n].append(p)
        if not truth_stack:
            raise ValueError(SHAPE_ERROR)
        gt_all = np.concatenate(truth_stack)
        stacks = {n: np.concatenate(v) if v else None for n, v in pieces.items()}
    else:
        if any(isinstance(s, dict) for s in preds.values()):
            raise TypeError("float() argument must be a string or a real number, not 'dict'")
        gt_all = crop(transform(truth), crop_size)
        stacks = {n: thw(transform(p)) for n, p in preds.items()}
    if not names:
        raise ValueError("Number of columns must be a positive integer, not 0")
    pools = {}
    for n in names:
        if stacks[n] is None:
            raise ValueError(SHAPE_ERROR)
        m = min(stacks[n].shape[0], gt_all.shape[0])
        p, g = crop(stacks[n][:m], crop_size), gt_all[:m]
        stacks[n] = p
        out["metrics"][f"NSE_{n}"] = _nse(p.reshape(m, -1)[:, sel].ravel(), g.reshape(m, -1)[:, sel].ravel())
        pf, gf = p.ravel(), g.ravel()
        keep = np.isfinite(pf) & np.isfinite(gf) & (gf >= 0.1)
        pools[n] = (gf[keep], pf[keep])
        out["pool"][n] = int(keep.sum())
    if np.isfinite(gt_all).any():
        rng = np.random.default_rng(seed)
        for n in names:
            x, y = pools[n]
            if x.size > max_points:
                idx = rng.choice(x.size, size=max_points, replace=False)
                x, y = x[idx], y[idx]
            out["x"][n], out["y"][n] = x, y
            if x.size >= 2:
                out["fit_scatter"][n] = _fit(x, y)
                out["fit_residual"][n] = _fit(x, y - x)
        if per_event:
            out["freq_truth"] = _freq(gt_all.ravel())
            for n in names:
                if np.isfinite(stacks[n]).any():
                    out["freq"][n] = _freq(stacks[n].ravel())
    return out


# ---- the fixture's cases: recipe -> (preds, truth, mask, kwargs) --------------------------------------------------------------

CASES = [
    # three methods, the middle one mostly NaN: the rng draws for the first and the last only
    {"name": "radar_sampled", "mode": "radar", "crop": 32, "events": [[10, 40, 48], [7, 40, 48], [9, 40, 48]], "input": "dict",
     "mask_frac": 0.3, "methods": {"gan": {"seed": 11, "noise": 10.0, "zero": 0.05, "over": 0.02},
                                   "sparse": {"seed": 12, "noise": 20.0, "nan": 0.985},
                                   "stdk": {"seed": 13, "noise": 25.0}}},
    {"name": "gauge_small", "mode": "gauge", "crop": 8, "events": [[6, 12, 14], [4, 12, 14]], "input": "dict", "mask_frac": 0.1,
     "methods": {"gan": {"seed": 21, "noise": 8.0}, "idw": {"seed": 22, "noise": 30.0, "zero": 0.1}}},
    {"name": "missing_event", "mode": "radar", "crop": 8, "events": [[5, 12, 12], [4, 12, 12], [6, 12, 12]], "input": "dict",
     "mask_frac": 0.3, "methods": {"gan": {"seed": 31, "noise": 10.0, "skip": [1]}, "stdk": {"seed": 32, "noise": 20.0}}},
    # "short" cuts events 1 and 2; "full" comes after it and inherits the cuts (the reference's truth_ev = truth_aligned)
    {"name": "carry_over", "mode": "radar", "crop": 8, "events": [[6, 12, 12], [5, 12, 12], [4, 10, 12]], "input": "dict",
     "mask_frac": 0.25, "methods": {"short": {"seed": 41, "noise": 12.0, "t": [6, 3, 2]}, "full": {"seed": 42, "noise": 6.0}}},
    {"name": "nan_pred", "mode": "radar", "crop": 8, "events": [[6, 12, 12], [3, 12, 12]], "input": "dict", "mask_frac": 0.3,
     "methods": {"gan": {"seed": 51, "noise": 10.0, "nan": 0.05}, "allnan": {"seed": 52, "nan": 1.0},
                 "clean": {"seed": 53, "noise": 10.0}}},
    # frame 2 of the truth is constant: its NSE is clipped to 0
    {"name": "constant_frame", "mode": "gauge", "crop": 8, "events": [[5, 12, 12]], "input": "dict", "mask_frac": 0.5,
     "const_frame": [0, 2, 120], "methods": {"gan": {"seed": 61, "noise": 10.0}}},
    {"name": "array_input", "mode": "radar", "crop": 8, "events": [[10, 12, 14]], "input": "array", "mask_frac": 0.25,
     "methods": {"gan": {"seed": 71, "noise": 12.0, "t": [12]}, "idw": {"seed": 72, "noise": 30.0}}},
    # a truth of 10 (below 0.1 mm/h) but for one pixel: pools of one point and of none
    {"name": "tiny_pool", "mode": "radar", "crop": 8, "events": [[3, 10, 10]], "input": "dict", "mask_frac": 0.2, "truth_const": 10,
     "spike": [0, 1, 5, 5, 100], "methods": {"gan": {"seed": 81, "noise": 3.0}, "holed": {"seed": 82, "noise": 3.0, "nan_spike": True}}},
    {"name": "err_not_dict", "mode": "radar", "crop": 8, "events": [[3, 12, 12]], "input": "dict", "mask_frac": 0.3,
     "methods": {"gan": {"seed": 91, "noise": 10.0, "as_array": True}}},
    {"name": "err_crop", "mode": "radar", "crop": 16, "events": [[3, 12, 12]], "input": "dict", "mask_frac": 0.3,
     "methods": {"gan": {"seed": 92, "noise": 10.0}}},
    {"name": "err_dict_array", "mode": "radar", "crop": 8, "events": [[3, 12, 12]], "input": "array", "mask_frac": 0.3,
     "methods": {"gan": {"seed": 93, "noise": 10.0, "as_dict": True}}},
]


def build_case(c):
    """(preds, truth, mask, kwargs) of a recipe; dict inputs are {event_01: [T, 1, H, W], ...} as scripts/infer.py writes them."""
    truths = []
    for i, (t, h, w) in enumerate(c["events"]):
        if "truth_const" in c:
            g = np.full((t, 1, h, w), c["truth_const"], dtype=np.uint8)
        else:
            g = seeded.exp1_truth(3000 + i, t, h, w)
        if "const_frame" in c and c["const_frame"][0] == i:
            g[c["const_frame"][1]] = c["const_frame"][2]
        if "spike" in c and c["spike"][0] == i:
            _, f, y, x, v = c["spike"]
            g[f, 0, y, x] = v
        truths.append(g)
    keys = [f"event_{i + 1:02d}" for i in range(len(truths))]
    preds = {}
    for name, m in c["methods"].items():
        evs = {}
        for i, (k, g) in enumerate(zip(keys, truths)):
            if i in m.get("skip", []):
                continue
            t = m["t"][i] if "t" in m else None
            p = seeded.exp1_pred(m["seed"] * 100 + i, g, m.get("noise", 10.0), m.get("zero", 0.0), m.get("over", 0.0), m.get("nan", 0.0),
                                 t=t)
            if m.get("nan_spike"):
                _, f, y, x, _ = c["spike"]
                p[f, 0, y, x] = np.nan
            evs[k] = p
        if c["input"] == "dict":
            preds[name] = evs[keys[0]] if m.get("as_array") else evs
        else:
            preds[name] = evs if m.get("as_dict") else evs[keys[0]]
    truth = dict(zip(keys, truths)) if c["input"] == "dict" else truths[0]
    s = c["crop"]
    mask = seeded.exp1_mask(4000 + s, s, s, c["mask_frac"])
    return preds, truth, mask, {"mode": c["mode"], "crop_size": s}


def recipe_json(c):
    return json.dumps(c, sort_keys=True)
