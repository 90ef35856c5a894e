"""A numpy restatement of the benchmark's exp1 scores (reference experiments/exp1.py run_exp1 with experiments/io.py), written from
the rules listed in DESIGN.md section 10, and the input recipes of tests/golden/exp1_cases.npz.  The CPU tests check the
restatement against the fixture; the GPU tests use it as the arbiter at sizes the fixture does not hold.  SSIM and dTSSIM run in
float32, as the reference runs them through torch."""
import json

import numpy as np

from p2igan_bench.utils import seeded


def transform(x, divide_by_3=True):
    x = np.maximum(np.asarray(x, dtype=np.float64), 0.001)
    if divide_by_3:
        x = x / 3.0
    return np.clip(10 ** np.minimum(x * 0.0625, 38.0) * 0.036, 0.0, 200.0)


def thw(a):
    a = np.asarray(a)
    if a.ndim == 5 and a.shape[0] == 1:
        a = a[0]
    if a.ndim == 4 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim == 4 and a.shape[-1] == 1:
        a = a[..., 0]
    if a.ndim != 3:
        raise ValueError(f"Expected [T,H,W], got shape {a.shape}")
    return a


def crop(a, size):
    a = thw(a)
    h, w = a.shape[1:]
    if size > min(h, w):
        raise ValueError(f"crop size {size} exceeds input {h}x{w}")
    top, left = (h - size) // 2, (w - size) // 2
    return a[:, top:top + size, left:left + size]


def _ssim(a, b):
    """Global SSIM of two float32 frames in float32 (biased moments, c1 = 1e-4, c2 = 9e-4, + 1e-10)."""
    ma, mb = a.mean(dtype=np.float32), b.mean(dtype=np.float32)
    va = ((a - ma) ** 2).mean(dtype=np.float32)
    vb = ((b - mb) ** 2).mean(dtype=np.float32)
    vab = ((a - ma) * (b - mb)).mean(dtype=np.float32)
    num = (np.float32(2) * ma * mb + np.float32(1e-4)) * (np.float32(2) * vab + np.float32(9e-4))
    den = (ma * ma + mb * mb + np.float32(1e-4)) * (va + vb + np.float32(9e-4))
    return num / (den + np.float32(1e-10))


def _pool(x, use_pool8):
    x = x.astype(np.float32)
    if not use_pool8:
        return x
    t, h, w = x.shape
    ph, pw = h // 8, w // 8
    if ph == 0 or pw == 0:
        raise ValueError("crop smaller than the 8x8 pooling window")
    return x[:, :ph * 8, :pw * 8].reshape(t, ph, 8, pw, 8).mean(axis=(2, 4), dtype=np.float32)


def ssim_spatial(pred, gt, use_pool8=True):
    p, g = _pool(pred, use_pool8), _pool(gt, use_pool8)
    return float(np.mean(np.array([_ssim(p[i], g[i]) for i in range(p.shape[0])], dtype=np.float32), dtype=np.float32))


def delta_tssim(pred, gt, lag, use_pool8=True):
    if pred.shape[0] <= lag:
        return float("nan")
    p, g = _pool(pred, use_pool8), _pool(gt, use_pool8)
    d = np.array([_ssim(p[t], p[t - lag]) - _ssim(g[t], g[t - lag]) for t in range(lag, p.shape[0])], dtype=np.float32)
    return float(d.mean(dtype=np.float32))


def pss(pred_sel, gt_sel, bins=50, min_value=0.5):
    p32, g32 = pred_sel.astype(np.float32), gt_sel.astype(np.float32)
    if p32.size == 0 or g32.size == 0:
        return float("nan")
    both = np.concatenate([p32.ravel(), g32.ravel()])
    both = both[np.isfinite(both) & (both > min_value)]
    if both.size == 0:
        return float("nan")
    vmin, vmax = float(both.min()), float(both.max())
    if vmin == vmax:
        vmax = vmin + 1e-6
    scores = []
    for i in range(p32.shape[0]):
        p = p32[i][np.isfinite(p32[i]) & (p32[i] > min_value)]
        g = g32[i][np.isfinite(g32[i]) & (g32[i] > min_value)]
        if p.size == 0 or g.size == 0:
            continue
        hp = np.histogram(p, bins=bins, range=(vmin, vmax))[0]
        hg = np.histogram(g, bins=bins, range=(vmin, vmax))[0]
        scores.append(float(np.minimum(hp / (hp.sum() + 1e-12), hg / (hg.sum() + 1e-12)).sum()))
    return float(np.mean(scores)) if scores else float("nan")


def categorical(p, g, thr):
    pb, gb = p >= thr, g >= thr
    h, m = int((pb & gb).sum()), int((~pb & gb).sum())
    f, c = int((pb & ~gb).sum()), int((~pb & ~gb).sum())
    n = np.int64
    h, m, f, c = n(h), n(m), n(f), n(c)
    hss = float("nan")
    if h + m + f + c > 0:
        hss = float(2 * (h * c - m * f) / (m ** 2 + f ** 2 + 2 * h * c + (m + f) * (h + c) + 1e-10))
    return {"POD": float(h / (h + m + 1e-10)), "FAR": float(f / (h + f + 1e-10)), "CSI": float(h / (h + m + f + 1e-10)), "HSS": hss}


def run_exp1(preds, truth, mask, mode, crop_size, thresholds=(0.5, 2.0, 4.0, 8.0), use_pool8=True, divide_by_3=True):
    if isinstance(truth, dict):
        keys = list(truth)
        if not keys:
            return {}
        truth_arr = np.concatenate([truth[k] for k in keys if truth.get(k) is not None], axis=0)
        preds = {name: np.concatenate([src[k] for k in keys if src.get(k) is not None], axis=0)
                 for name, src in preds.items() if isinstance(src, dict)}
        truth = truth_arr
    gt_all = crop(transform(truth, divide_by_3), crop_size)
    mask = np.asarray(mask).astype(bool)
    out = {}
    for name, pred in preds.items():
        p = thw(transform(pred, divide_by_3))
        n = min(p.shape[0], gt_all.shape[0])
        p, g = crop(p[:n], crop_size), gt_all[:n]
        if mode not in ("radar", "gauge"):
            raise ValueError(f"Unknown mode: {mode}")
        if mask.shape != p.shape[1:]:
            raise ValueError(f"Mask shape {mask.shape} != data shape {p.shape[1:]}")
        sel = ~mask if mode == "radar" else mask
        ps, gs = p.reshape(n, -1)[:, sel.ravel()], g.reshape(n, -1)[:, sel.ravel()]
        r = {"MAE": float(np.mean(np.abs(ps - gs))) if ps.size else float("nan"),
             "RMSE": float(np.sqrt(np.mean((ps - gs) ** 2))) if ps.size else float("nan"),
             "PSS": pss(ps, gs),
             "SSIM": ssim_spatial(p, g, use_pool8),
             "DTSSIM_L1": delta_tssim(p, g, 1, use_pool8),
             "DTSSIM_L2": delta_tssim(p, g, 2, use_pool8),
             "NSE": float(1.0 - np.sum((ps - gs) ** 2) / (np.sum((gs - gs.mean()) ** 2) + 1e-10)) if gs.size else 1.0}
        for thr in thresholds:
            r[f"CAT_{thr:g}"] = categorical(ps, gs, thr)
        out[name] = r
    return out


# ---- the fixture's cases: recipe -> (preds, truth, mask, kwargs) --------------------------------------------------------------

CASES = [
    {"name": "radar_dict", "mode": "radar", "crop": 32, "events": [[12, 40, 48], [9, 40, 48], [17, 40, 48]], "input": "dict",
     "mask_frac": 0.3, "methods": {"gan": {"seed": 11, "noise": 10.0, "zero": 0.05, "over": 0.02},
                                   "stdk": {"seed": 12, "noise": 25.0, "skip": [1]}}},
    {"name": "gauge_nopool", "mode": "gauge", "crop": 24, "pool8": False, "thresholds": [0.5, 1.0, 2.0, 4.0, 8.0],
     "events": [[10, 30, 30], [6, 30, 30]], "input": "dict", "mask_frac": 0.1,
     "methods": {"gan": {"seed": 21, "noise": 8.0}, "idw": {"seed": 22, "noise": 30.0, "zero": 0.1}}},
    {"name": "array_long_pred", "mode": "radar", "crop": 32, "events": [[15, 36, 40]], "input": "array", "mask_frac": 0.25,
     "methods": {"gan": {"seed": 31, "noise": 12.0, "t": 20}}},
    {"name": "crop36", "mode": "radar", "crop": 36, "events": [[8, 44, 44]], "input": "array", "mask_frac": 0.2,
     "methods": {"gan": {"seed": 41, "noise": 15.0, "over": 0.05}}},
    {"name": "t2", "mode": "radar", "crop": 16, "events": [[2, 20, 20]], "input": "array", "mask_frac": 0.3,
     "methods": {"gan": {"seed": 51, "noise": 10.0}}},
    {"name": "t1", "mode": "gauge", "crop": 16, "events": [[1, 20, 20]], "input": "array", "mask_frac": 0.5,
     "methods": {"gan": {"seed": 52, "noise": 10.0}}},
    {"name": "below_half", "mode": "radar", "crop": 16, "events": [[5, 20, 20]], "input": "array", "mask_frac": 0.3,
     "truth_hi": 40, "methods": {"gan": {"seed": 61, "noise": 3.0, "cap": 40.0}}},
    {"name": "constant", "mode": "radar", "crop": 16, "events": [[4, 16, 16]], "input": "array", "mask_frac": 0.3,
     "truth_const": 150, "methods": {"gan": {"seed": 71, "const": 150.0}}},
    {"name": "nan_pred", "mode": "radar", "crop": 16, "events": [[6, 24, 24]], "input": "dict", "mask_frac": 0.3,
     "methods": {"gan": {"seed": 81, "noise": 10.0, "nan": 0.01}, "clean": {"seed": 82, "noise": 10.0}}},
    {"name": "empty_sel", "mode": "radar", "crop": 16, "events": [[5, 20, 20]], "input": "array", "mask_frac": 1.1,
     "methods": {"gan": {"seed": 91, "noise": 10.0}}},
]


def build_case(c):
    """(preds, truth, mask, kwargs) of a recipe; dict inputs are {event_01: [T, 1, H, W], ...} as scripts/infer.py writes them."""
    truths = []
    for i, (t, h, w) in enumerate(c["events"]):
        if "truth_const" in c:
            truths.append(np.full((t, 1, h, w), c["truth_const"], dtype=np.uint8))
        else:
            truths.append(seeded.exp1_truth(1000 + i, t, h, w, hi=c.get("truth_hi", 255)))
    keys = [f"event_{i + 1:02d}" for i in range(len(truths))]
    preds = {}
    for name, m in c["methods"].items():
        evs = {}
        for i, (k, g) in enumerate(zip(keys, truths)):
            if i in m.get("skip", []):
                continue
            if "const" in m:
                p = np.full(g.shape, m["const"], dtype=np.float32)
            else:
                p = seeded.exp1_pred(m["seed"] * 100 + i, g, m.get("noise", 10.0), m.get("zero", 0.0), m.get("over", 0.0),
                                     m.get("nan", 0.0), t=m.get("t"))
                if "cap" in m:
                    p = np.minimum(p, np.float32(m["cap"]))
            evs[k] = p
        preds[name] = evs if c["input"] == "dict" else evs[keys[0]]
    truth = dict(zip(keys, truths)) if c["input"] == "dict" else truths[0]
    s = c["crop"]
    mask = seeded.exp1_mask(2000 + s, s, s, c["mask_frac"])
    kw = {"mode": c["mode"], "crop_size": s, "thresholds": tuple(c.get("thresholds", (0.5, 2.0, 4.0, 8.0))),
          "use_pool8": c.get("pool8", True)}
    return preds, truth, mask, kw


def flatten(res):
    """{method: {...}} -> {'method/KEY' or 'method/CAT_x/SUB': float}."""
    out = {}
    for name, r in res.items():
        for k, v in r.items():
            if isinstance(v, dict):
                for sk, sv in v.items():
                    out[f"{name}/{k}/{sk}"] = float(sv)
            else:
                out[f"{name}/{k}"] = float(v)
    return out


def recipe_json(c):
    return json.dumps(c, sort_keys=True)
