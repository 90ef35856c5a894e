"""Scale-aware verification on csrc/eval_scale.hip: the fractions skill score (Roberts & Lean 2008) over thresholds x neighbourhood
sizes and the radially averaged power spectral density, per method against the truth.  ``ScaleEvaluator`` streams aligned pieces
and syncs once in ``compute``; ``run_scale`` takes event dicts with run_exp1's rules.  Inputs are exp1's; every pixel of the crop
counts (no mask).  DESIGN.md section 15 holds the definitions; tests/scale_ref.py restates them in numpy."""
from __future__ import annotations

import os
import warnings
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from ._common import Streaming, bounded_crop, cat, event_lists, radar_thresholds
from .exp1 import DEFAULT_THRESHOLDS

DEFAULT_SCALES = (1, 3, 5, 9, 17, 33, 65)
MAX_SCALES = ops.SCALE_MAX_SCALES
_WORK_DOUBLES = 1 << 25          # spectra workspace (the row transform's output) per launch: 256 MB
_WORK_COUNTS = 1 << 26           # FSS table workspace of the large-crop path per launch: 256 MB


def ring_index(S: int) -> np.ndarray:
    """[S, S] int: r = rint(sqrt(k_y^2 + k_x^2)) with k = np.fft.fftfreq(S) * S (the square root of an integer is never a tie)."""
    k = np.rint(np.fft.fftfreq(S) * S).astype(np.int64)
    return np.rint(np.sqrt((k[:, None] ** 2 + k[None, :] ** 2).astype(np.float64))).astype(np.int64)


def ring_counts(S: int) -> np.ndarray:
    """The populations of rings 0 .. S // 2 over the full plane."""
    return np.bincount(ring_index(S).ravel(), minlength=S // 2 + 1)[:S // 2 + 1]


def ring_list(S: int):
    """The half plane k_x <= S // 2 as the kernel reads it: (order, weight, offsets, count).  ``order`` lists the bins
    ky * (S // 2 + 1) + kx of rings 0 .. S // 2 sorted by ring (raster order inside a ring), ``weight`` is 2 where the bin's mirror
    (-ky, -kx) lies outside the half plane, ``offsets`` [R + 1] delimits the rings and ``count`` is the full-plane population."""
    R = S // 2 + 1
    r = ring_index(S)[:, :R]
    w = np.full((S, R), 2.0)
    w[:, 0] = 1.0
    if S % 2 == 0:
        w[:, S // 2] = 1.0
    keep = np.flatnonzero(r.ravel() < R)
    keep = keep[np.argsort(r.ravel()[keep], kind="stable")]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(r.ravel()[keep], minlength=R))])
    return keep.astype(np.int32), w.ravel()[keep], offsets.astype(np.int32), ring_counts(S).astype(np.float64)


def twiddle(S: int) -> np.ndarray:
    """[2, S] float64: cos, sin(2 pi m / S)."""
    a = 2.0 * np.pi * np.arange(S, dtype=np.float64) / S
    return np.stack([np.cos(a), np.sin(a)])


def check_overflow(frames: int, S: int, scales: Sequence[int]) -> None:
    """The FSS sums are exact 64-bit integers: sum c^2 <= frames * S^2 * min(n, S)^4 must stay below 2^63."""
    n = min(max(int(s) for s in scales), S)
    if frames * S * S * n ** 4 >= 2 ** 63:
        raise OverflowError(f"FSS sums of {frames} frames of {S}x{S} at window {n} may exceed 64 bits")


def fss_value(A: int, B: int, C: int) -> float:
    """FSS = 1 - (A + B - 2 C) / (A + B) from the exact integer sums; NaN when nothing exceeds the threshold in either field."""
    if A + B == 0:
        return float("nan")
    return 1.0 - (A + B - 2 * C) / (A + B)


def useful_scale(fss: Dict[int, float], hits: int, pixels: int) -> Optional[int]:
    """The smallest listed n with FSS >= 0.5 + f0 / 2, f0 = the truth's fraction of pixels at or above the threshold."""
    target = 0.5 + (hits / pixels) / 2
    ok = [n for n, v in fss.items() if v >= target]
    return min(ok) if ok else None


def spectrum_scores(pm: np.ndarray, pt: np.ndarray, S: int) -> Tuple[float, float]:
    """(LSD in dB over rings r >= 1, HF_ratio = mean P_m / P_t over rings r > S / 4); NaN where no ring qualifies."""
    r = np.arange(len(pm))
    with np.errstate(all="ignore"):
        d = 10.0 * np.log10(pm[1:]) - 10.0 * np.log10(pt[1:])
        lsd = float(np.sqrt(np.mean(d * d))) if d.size else float("nan")
        hf = pm[4 * r > S] / pt[4 * r > S]
        hfr = float(np.mean(hf)) if hf.size else float("nan")
    return lsd, hfr


def _check_scales(scales):
    scales = tuple(int(n) for n in scales)
    if not 0 < len(scales) <= MAX_SCALES:
        raise ValueError(f"1 to {MAX_SCALES} scales")
    if any(n < 1 for n in scales) or len(set(scales)) != len(scales):
        raise ValueError(f"scales are distinct window sizes >= 1, got {scales}")
    return scales


class ScaleEvaluator(Streaming):
    """Streaming FSS and spectra.  ``update(method, pred, truth)`` adds one piece whose frames pair one for one (the longer side is
    truncated, as align_length does); ``compute()`` syncs once and returns ``{method: {...}}`` (see ``run_scale``)."""

    what = "scale verification runs"

    def __init__(self, crop_size: int, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, scales: Sequence[int] = DEFAULT_SCALES,
                 divide_by_3: bool = True, device=None, mode: str = "radar"):
        self.thresholds = radar_thresholds(mode, thresholds, "scale verification scores neighbourhoods")
        self.scales = _check_scales(scales)
        self.size = bounded_crop(crop_size)
        self._start(device, divide_by_3)
        self.use_workspace = self.size > ops.SCALE_LDS_CROP      # tests set it to run a small crop through the large-crop path
        with torch.cuda.device(self.device):
            self._tw = torch.from_numpy(twiddle(self.size)).to(self.device)
            self._rings = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in ring_list(self.size))

    def _new_state(self):
        words = len(self.thresholds) * (3 * len(self.scales) + 1)
        return SimpleNamespace(acc=torch.zeros(words, device=self.device, dtype=torch.int64), P=[], flag=[], T=0)

    def _launch_frames(self):
        S, R = self.size, self.size // 2 + 1
        step = max(1, _WORK_DOUBLES // (4 * S * R))
        if self.use_workspace:
            step = min(step, max(1, _WORK_COUNTS // (len(self.thresholds) * 2 * S * S)))
        return step

    def update(self, method: str, pred_event, truth_event):
        S, R, K, N = self.size, self.size // 2 + 1, len(self.thresholds), len(self.scales)
        with torch.cuda.device(self.device):
            pred, truth, ptl, gtl, n, st = self._open(method, pred_event, truth_event)
            check_overflow(st.T + n, S, self.scales)
            for t0, tn in self._cuts(n):
                p, g = pred[t0:t0 + tn], truth[t0:t0 + tn]
                part = torch.empty(tn, K, 3 * N + 1, device=self.device, dtype=torch.int64)
                ws = self._buf("tables", tn * K * 2 * S * S, torch.int32) if self.use_workspace else None
                ops.scale_fss(p, g, ptl, gtl, S, self._lut, self.thresholds, self.scales, self.divide_by_3, part, ws)
                ops.scale_fss_merge(part, st.acc)
                P = torch.empty(tn, 2, R, device=self.device, dtype=torch.float64)
                flag = torch.empty(tn, 2, device=self.device, dtype=torch.int32)
                ops.scale_spectra(p, g, ptl, gtl, S, self._lut, self.divide_by_3, self._tw, self._rings,
                                  self._buf("G", tn * 4 * S * R, torch.float64), self._buf("psd", tn * 2 * S * R, torch.float64), P, flag)
                st.P.append(P)
                st.flag.append(flag)
                st.T += tn

    def compute(self) -> Dict[str, Dict[str, object]]:
        names = list(self._methods)
        if not names:
            return {}
        S, R, K, N = self.size, self.size // 2 + 1, len(self.thresholds), len(self.scales)
        rows = []
        with torch.cuda.device(self.device):
            for name in names:
                st = self._methods[name]
                if st.T == 0:
                    raise ValueError(f"method {name!r} has no frames to score")
                # the frames' ring means of all pieces in frame order, folded in that order: where pieces were cut does not matter
                spec = ops.scale_spectrum_merge(cat(st.P), cat(st.flag))
                rows.append(torch.cat([spec, st.acc.view(torch.float64)]))       # the integers travel as their bits
            host = torch.stack(rows).cpu().numpy()         # the one host sync
        res = {}
        for name, row in zip(names, host):
            T = self._methods[name].T
            pm, pt, skipped = row[:R], row[R:2 * R], int(row[2 * R])
            acc = np.ascontiguousarray(row[2 * R + 1:]).view(np.int64).reshape(K, 3 * N + 1)
            fss, useful = {}, {}
            for j, q in enumerate(self.thresholds):
                by_n = {n: fss_value(*(int(v) for v in acc[j, 3 * i:3 * i + 3])) for i, n in enumerate(self.scales)}
                fss[f"thr_{q:g}"] = {f"n_{n}": v for n, v in by_n.items()}
                useful[f"thr_{q:g}"] = useful_scale(by_n, int(acc[j, 3 * N]), T * S * S)
            lsd, hfr = spectrum_scores(pm, pt, S)
            res[name] = {"FSS": fss, "useful_scale": useful, "LSD": lsd, "HF_ratio": hfr, "spectrum": [float(v) for v in pm],
                         "truth_spectrum": [float(v) for v in pt], "wavelength_px": [S / r for r in range(1, R)], "frames": T,
                         "frames_skipped": skipped}
        return res

    def sums(self, method: str) -> np.ndarray:
        """The method's exact integer sums so far, [thresholds, 3 * scales + 1] int64 (A, B, C per scale, then the truth's hits);
        syncs.  For checks: ``compute`` is the product path."""
        st = self._methods[method]
        return st.acc.cpu().numpy().reshape(len(self.thresholds), 3 * len(self.scales) + 1)


def run_scale(preds, truth, crop_size: int, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, scales: Sequence[int] = DEFAULT_SCALES,
              divide_by_3: bool = True, device=None, mode: str = "radar") -> Dict[str, Dict[str, object]]:
    """FSS and radial spectra of every method against the truth, with run_exp1's handling of event dicts (the truth's key order, an
    event a method lacks is skipped for that method, a method that is not a dict is left out).  Returns per method
    ``{"FSS": {"thr_<q:g>": {"n_<n>": v}}, "useful_scale": {"thr_<q:g>": n or None}, "LSD": dB, "HF_ratio": v, "spectrum": [...],
    "truth_spectrum": [...], "wavelength_px": [...], "frames": T, "frames_skipped": k}``."""
    truth_events, methods = event_lists(preds, truth)
    if not truth_events:
        return {}
    ev = ScaleEvaluator(crop_size, thresholds, scales, divide_by_3, device=device, mode=mode)
    for name, p, g, _ in ev.pieces(truth_events, methods):
        ev.update(name, p, g)
    return ev.compute()


def scale_lines(metrics) -> List[str]:
    """metrics.txt: ``FSS_<name>_thr<q>_n<n>: v`` and ``LSD_<name>: v`` lines, 6 decimals."""
    lines = []
    for name, m in metrics.items():
        for tk, by_n in m["FSS"].items():
            for nk, v in by_n.items():
                lines.append(f"FSS_{name}_{tk.replace('_', '')}_{nk.replace('_', '')}: {v:.6f}")
        lines.append(f"LSD_{name}: {m['LSD']:.6f}")
    return lines


def write_scale_figure(metrics, path: str) -> Optional[str]:
    """One FSS-against-n panel per threshold and one log-log spectrum panel (matplotlib, no display needed).  Without matplotlib it
    warns and writes nothing."""
    try:
        from matplotlib.figure import Figure
    except ImportError:
        warnings.warn("matplotlib is not importable: the scale figure is skipped (the numbers are in scale_data.npz)")
        return None
    names = list(metrics)
    thr = list(metrics[names[0]]["FSS"]) if names else []
    fig = Figure(figsize=(4 * (len(thr) + 1), 3.5), dpi=200)
    axes = fig.subplots(1, len(thr) + 1, squeeze=False)[0]
    for ax, tk in zip(axes, thr):
        for name in names:
            by_n = metrics[name]["FSS"][tk]
            ax.plot([int(k[2:]) for k in by_n], list(by_n.values()), marker="o", markersize=3, label=name)
        ax.set_xscale("log", base=2)
        ax.set_ylim(0.0, 1.02)
        ax.set_xlabel("neighbourhood n (px)")
        ax.set_ylabel("FSS")
        ax.set_title(f">= {tk[4:]} mm/h", fontsize=10)
    ax = axes[-1]
    for i, name in enumerate(names):
        m = metrics[name]
        r = np.arange(1, len(m["spectrum"]))
        if i == 0 and len(r):
            ax.loglog(r, np.asarray(m["truth_spectrum"])[1:], color="k", linewidth=1.5, label="truth")
        if len(r):
            ax.loglog(r, np.asarray(m["spectrum"])[1:], label=name)
    ax.set_xlabel("wavenumber r (cycles per crop)")
    ax.set_ylabel("P(r)")
    ax.set_title("radially averaged power", fontsize=10)
    if names:
        ax.legend(frameon=True, fontsize=8)
    fig.tight_layout()
    fig.savefig(path, format="pdf", bbox_inches="tight")
    return path


def write_scale_outputs(out_dir: str, metrics) -> None:
    """DIR/metrics.json (indent 2, sorted keys), DIR/metrics.txt (``scale_lines``), DIR/scale_data.npz and DIR/scale_panels.pdf."""
    import json
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "metrics.json"), "w", encoding="utf-8") as f:
        json.dump(metrics, f, indent=2, sort_keys=True)
    with open(os.path.join(out_dir, "metrics.txt"), "w", encoding="utf-8") as f:
        for line in scale_lines(metrics):
            f.write(line + "\n")
    arrays = {"methods": np.array(list(metrics))}
    for name, m in metrics.items():
        thr = list(m["FSS"])
        arrays[f"{name}/fss"] = np.array([[v for v in m["FSS"][tk].values()] for tk in thr], dtype=np.float64)
        arrays[f"{name}/thresholds"] = np.array([float(tk[4:]) for tk in thr])
        arrays[f"{name}/scales"] = np.array([int(k[2:]) for k in m["FSS"][thr[0]]]) if thr else np.zeros(0, np.int64)
        arrays[f"{name}/useful_scale"] = np.array([-1 if m["useful_scale"][tk] is None else m["useful_scale"][tk] for tk in thr])
        for k in ("spectrum", "truth_spectrum", "wavelength_px"):
            arrays[f"{name}/{k}"] = np.asarray(m[k], dtype=np.float64)
        arrays[f"{name}/scores"] = np.array([m["LSD"], m["HF_ratio"], m["frames"], m["frames_skipped"]], dtype=np.float64)
    np.savez(os.path.join(out_dir, "scale_data.npz"), **arrays)
    write_scale_figure(metrics, os.path.join(out_dir, "scale_panels.pdf"))
