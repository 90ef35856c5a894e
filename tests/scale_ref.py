"""A float64 numpy restatement of the scale-aware verification: window counts from a padded summed-area
table in int64, the FSS sums as Python ints, the radially averaged power spectrum through np.fft.fft2, and the seeded inputs the
tests share.  It imports nothing from p2igan_bench.evaluation: the CPU tests check it against scipy and hand-computed values, the
GPU tests use it as the arbiter."""
import numpy as np


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


def window_counts(ind, n):
    """ind [..., S, S] of 0 / 1 -> int64 counts over rows y - n//2 .. y - n//2 + n - 1 and the same columns; outside counts 0."""
    ind = np.asarray(ind).astype(np.int64)
    S = ind.shape[-1]
    sat = np.zeros(ind.shape[:-2] + (S + 1, S + 1), np.int64)
    sat[..., 1:, 1:] = ind.cumsum(-2).cumsum(-1)
    lo = np.clip(np.arange(S) - n // 2, 0, S)
    hi = np.clip(np.arange(S) - n // 2 + n, 0, S)
    return (sat[..., hi[:, None], hi[None, :]] - sat[..., lo[:, None], hi[None, :]] - sat[..., hi[:, None], lo[None, :]]
            + sat[..., lo[:, None], lo[None, :]])


def fss_sums(pred_mm, truth_mm, thresholds, scales):
    """[T, S, S] rain rates -> int64 [K, 3 N + 1]: per scale A, B, C, then the truth's hits (NaN compares false)."""
    out = []
    with np.errstate(invalid="ignore"):
        for q in thresholds:
            ip, ig = pred_mm >= q, truth_mm >= q
            row = []
            for n in scales:
                cp, cg = window_counts(ip, n), window_counts(ig, n)
                row += [int((cp * cp).sum()), int((cg * cg).sum()), int((cp * cg).sum())]
            out.append(row + [int(ig.sum())])
    return np.array(out, dtype=np.int64)


def fss_value(A, B, C):
    A, B, C = int(A), int(B), int(C)
    return float("nan") if A + B == 0 else 1.0 - (A + B - 2 * C) / (A + B)


def useful_scale(fss_by_n, hits, pixels):
    target = 0.5 + (int(hits) / int(pixels)) / 2
    ok = [n for n, v in fss_by_n.items() if v >= target]
    return min(ok) if ok else None


def ring_index(S):
    k = np.fft.fftfreq(S) * S
    return np.rint(np.sqrt(k[:, None] ** 2 + k[None, :] ** 2)).astype(np.int64)


def ring_counts(S):
    return np.bincount(ring_index(S).ravel())[:S // 2 + 1]


def rapsd(frame):
    """One S x S float64 frame -> P(r), r = 0 .. S // 2: the ring means of |fft2|^2 / S^2."""
    S = frame.shape[0]
    psd = np.abs(np.fft.fft2(frame)) ** 2 / (S * S)
    r = ring_index(S).ravel()
    keep = r <= S // 2
    return np.bincount(r[keep], weights=psd.ravel()[keep], minlength=S // 2 + 1) / ring_counts(S)


def spectra(pred_mm, truth_mm):
    """(P_method, P_truth, skipped): the frame means in frame order over the frames without a NaN in either field."""
    S = pred_mm.shape[-1]
    sp, sg, n = np.zeros(S // 2 + 1), np.zeros(S // 2 + 1), 0
    for p, g in zip(pred_mm, truth_mm):
        if np.isnan(p).any() or np.isnan(g).any():
            continue
        sp, sg, n = sp + rapsd(p), sg + rapsd(g), n + 1
    with np.errstate(all="ignore"):
        return sp / n, sg / n, len(pred_mm) - n


def spectrum_scores(pm, pt, S):
    r = np.arange(len(pm))
    with np.errstate(all="ignore"):
        d = 10.0 * np.log10(pm[1:]) - 10.0 * np.log10(pt[1:])
        lsd = float(np.sqrt(np.mean(d * d))) if d.size else float("nan")
        hf = (pm / pt)[r > S / 4]
        return lsd, float(np.mean(hf)) if hf.size else float("nan")


def run_scale(preds, truth, crop_size, thresholds=(0.5, 2.0, 4.0, 8.0), scales=(1, 3, 5, 9, 17, 33, 65), divide_by_3=True):
    """preds {name: [T, H, W]}, truth [T, H, W] (arrays, one event) -> the product's dict."""
    S = crop_size
    res = {}
    for name, p in preds.items():
        n = min(len(p), len(truth))
        pm, gm = transform(crop(p[:n], S), divide_by_3), transform(crop(truth[:n], S), divide_by_3)
        sums = fss_sums(pm, gm, thresholds, scales)
        fss, useful = {}, {}
        for j, q in enumerate(thresholds):
            by_n = {m: fss_value(*sums[j, 3 * i:3 * i + 3]) for i, m in enumerate(scales)}
            fss[f"thr_{q:g}"] = {f"n_{m}": v for m, v in by_n.items()}
            useful[f"thr_{q:g}"] = useful_scale(by_n, sums[j, -1], n * S * S)
        sp, sg, skipped = spectra(pm, gm)
        lsd, hf = spectrum_scores(sp, sg, S)
        res[name] = {"FSS": fss, "useful_scale": useful, "LSD": lsd, "HF_ratio": hf, "spectrum": sp.tolist(),
                     "truth_spectrum": sg.tolist(), "wavelength_px": [S / r for r in range(1, S // 2 + 1)], "frames": n,
                     "frames_skipped": skipped}
    return res


# ---- seeded inputs: clip(gamma(0.3, 60), 0, 255) fields on the 0-255 scale; the smoother method is 0.5 g + 0.5 box3(g) ----
def field(seed, T, H, W):
    return np.clip(np.random.default_rng(seed).gamma(0.3, 60.0, size=(T, H, W)), 0.0, 255.0)


def box3(g):
    p = np.pad(g, ((0, 0), (1, 1), (1, 1)), mode="edge")
    return sum(p[:, dy:dy + g.shape[1], dx:dx + g.shape[2]] for dy in range(3) for dx in range(3)) / 9.0


def smoother(g):
    return 0.5 * g + 0.5 * box3(g)


def as_dtype(x, dtype):
    """A 0-255 float field as uint8 (rounded), float32 or float64."""
    return np.rint(x).astype(np.uint8) if np.dtype(dtype) == np.uint8 else x.astype(dtype)


def threshold_margin(x, thresholds, divide_by_3=True):
    """The smallest relative distance of a transformed value to a threshold (float inputs must stay clear of the thresholds: the
    device's pow may differ from numpy's in the last bits)."""
    v = transform(x, divide_by_3).ravel()
    v = v[~np.isnan(v)]
    return min(float(np.min(np.abs(v - q) / q)) for q in thresholds) if v.size else float("inf")
