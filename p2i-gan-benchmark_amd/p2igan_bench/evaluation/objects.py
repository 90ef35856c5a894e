"""Object-based verification on csrc/eval_objects.hip: the connected rain objects of thresholded frames, their population (count,
area, largest object) and SAL (Structure, Amplitude, Location; Wernli et al. 2008), per method against the truth.  The device
returns integers only (quantised rain Q = rint(R * 2^24), areas, first moments); the scores are float64 numpy from those integers.
``ObjectEvaluator`` streams aligned pieces; ``run_objects`` takes event dicts with run_exp1's rules.  Inputs are exp1's; every pixel
of the crop counts (no mask).  DESIGN.md section 23 holds the definitions; tests/objects_ref.py restates them in numpy."""
from __future__ import annotations

import os
import warnings
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ._common import Streaming, bounded_crop, event_lists, radar_thresholds
from .exp1 import DEFAULT_THRESHOLDS

DEFAULT_SAL_FACTOR = 1.0 / 15.0      # Wernli et al. 2008: R* = Rmax / 15
DEFAULT_SAL_FLOOR = 0.1              # mm/h: a dry frame sits at transform(0.001) ~ 0.036 mm/h everywhere
RELATIVE_LEVEL = "rel"
_WORK_BYTES = 1 << 28                # label workspace per launch: 256 MB
_HOST_THREADS = 4                    # pieces scored at a time in compute (numpy and the copies release the interpreter lock)
SCORES = ("S", "A", "L", "L1", "L2")


def level_keys(thresholds: Sequence[float]) -> List[str]:
    """The levels' names in the device's order: ``thr_<q:g>`` per absolute threshold, then the relative level."""
    return [f"thr_{q:g}" for q in thresholds] + [RELATIVE_LEVEL]


def _check_sal(connectivity, sal_factor, sal_floor):
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity is 4 or 8, got {connectivity!r}")
    sal_factor, sal_floor = float(sal_factor), float(sal_floor)
    if not 0.0 < sal_factor <= 1.0:
        raise ValueError(f"the SAL factor lies in (0, 1], got {sal_factor}")
    if not sal_floor >= 0.0:
        raise ValueError(f"the SAL floor is a rain rate >= 0, got {sal_floor}")
    return int(connectivity), sal_factor, sal_floor


class _Segments:
    """Sums and maxima over the records' consecutive runs of table rows (offsets [n + 1]); an empty run gives 0."""

    def __init__(self, offsets):
        self.n = len(offsets) - 1
        self.some = np.diff(offsets) > 0
        self.starts = offsets[:-1][self.some]

    def _spread(self, v, dtype):
        out = np.zeros(self.n, dtype)
        out[self.some] = v
        return out

    def sum(self, w):
        return self._spread(np.add.reduceat(w, self.starts) if len(self.starts) else [], w.dtype)

    def max(self, w):
        return self._spread(np.maximum.reduceat(w, self.starts) if len(self.starts) else [], w.dtype)


def sal_frames(S: int, rec: np.ndarray, lev: np.ndarray, offsets: np.ndarray, table: np.ndarray) -> Dict[str, np.ndarray]:
    """The per-frame scores from the device's integers, float64 numpy: rec [T, 2, 5] (sum Q, sum Q y, sum Q x, max Q, NaN flag; field 0
    = prediction, 1 = truth), lev [T, 2, L, 5] (objects, area, sum Q, sum Q y, sum Q x over object pixels), offsets [T * 2 * L + 1]
    and table [N, 6] (label, area, sum Q, max Q, sum Q y, sum Q x per object).  Returns ``valid`` [T] (no NaN in either crop),
    ``S, A, L, L1, L2`` [T, L] (NaN where a frame is not scored at that level: it is skipped or a field has no object), ``count``,
    ``area``, ``largest``, ``single`` [T, 2, L] (objects, rain area, largest object's area, single-pixel objects).  With R_n = sum Q of
    object n and D = sum Q / S^2 of the whole crop: A = (D_p - D_g) / ((D_p + D_g) / 2); V = sum_n R_n (R_n / Qmax_n) / sum_n R_n and
    S = (V_p - V_g) / ((V_p + V_g) / 2); with xbar the centre of mass of all pixels, x_n the object centroids and d = sqrt(2) S:
    L1 = |xbar_p - xbar_g| / d, r = sum_n R_n |xbar - x_n| / sum_n R_n, L2 = 2 |r_p - r_g| / d, L = L1 + L2."""
    T, _, L, _ = lev.shape
    nrec = T * 2 * L
    segs = _Segments(offsets)
    tf = np.repeat(np.arange(nrec) // L, np.diff(offsets))
    valid = rec[:, :, 4].sum(axis=1) == 0
    with np.errstate(all="ignore"):
        tot = rec[:, :, 0].astype(np.float64)
        ybar, xbar = rec[:, :, 1] / tot, rec[:, :, 2] / tot                       # [T, 2]
        area, rn, qmax, my, mx = (np.ascontiguousarray(table[:, k]) for k in range(1, 6))      # one strided pass per column
        rn = rn.astype(np.float64)
        dy, dx = my / rn - ybar.ravel()[tf], mx / rn - xbar.ravel()[tf]
        sum_r = segs.sum(rn)
        V = (segs.sum(rn * (rn / qmax)) / sum_r).reshape(T, 2, L)
        r = (segs.sum(rn * np.sqrt(dy * dy + dx * dx)) / sum_r).reshape(T, 2, L)
        D = tot / float(S * S)
        d = np.sqrt(2.0) * S
        A = np.repeat(((D[:, 0] - D[:, 1]) / (0.5 * (D[:, 0] + D[:, 1])))[:, None], L, axis=1)
        Sv = (V[:, 0] - V[:, 1]) / (0.5 * (V[:, 0] + V[:, 1]))
        ey, ex = ybar[:, 0] - ybar[:, 1], xbar[:, 0] - xbar[:, 1]
        L1 = np.repeat((np.sqrt(ey * ey + ex * ex) / d)[:, None], L, axis=1)
        L2 = 2.0 * np.abs(r[:, 0] - r[:, 1]) / d
    count = lev[:, :, :, 0]
    scored = valid[:, None] & (count[:, 0] > 0) & (count[:, 1] > 0)
    out = {"valid": valid, "count": count, "area": lev[:, :, :, 1]}
    for k, v in (("S", Sv), ("A", A), ("L", L1 + L2), ("L1", L1), ("L2", L2)):
        out[k] = np.where(scored, v, np.nan)
    out["largest"] = segs.max(area).reshape(T, 2, L)
    out["single"] = segs.sum((area == 1).astype(np.int64)).reshape(T, 2, L)
    return out


def _mean(v):
    return float(np.mean(v)) if len(v) else float("nan")


def sal_summary(frames: Dict[str, np.ndarray], keys: Sequence[str]) -> Dict[str, Dict[str, object]]:
    """Per level: mean and median of S, A, L, L1, L2 over the scored frames, mean |S| and |A|, ``frames_scored`` and the frames that
    cannot be scored (``frames_pred_only``, ``frames_truth_only``, ``frames_no_object``), and per side the object population over the
    frames without a NaN: objects per frame (mean, max), mean object area, the share of single-pixel objects and the mean share of
    the rain area that the largest object holds (over the frames with an object)."""
    valid, count = frames["valid"], frames["count"]
    res = {}
    for j, key in enumerate(keys):
        has_p, has_g = count[valid, 0, j] > 0, count[valid, 1, j] > 0
        scored = ~np.isnan(frames["S"][:, j])
        m: Dict[str, object] = {"frames_scored": int(scored.sum()), "frames_pred_only": int((has_p & ~has_g).sum()),
                                "frames_truth_only": int((~has_p & has_g).sum()), "frames_no_object": int((~has_p & ~has_g).sum())}
        for k in SCORES:
            v = frames[k][scored, j]
            m[f"{k}_mean"] = _mean(v)
            m[f"{k}_median"] = float(np.median(v)) if len(v) else float("nan")
        m["S_abs_mean"], m["A_abs_mean"] = _mean(np.abs(frames["S"][scored, j])), _mean(np.abs(frames["A"][scored, j]))
        for f, side in enumerate(("pred", "truth")):
            n, area = count[valid, f, j], frames["area"][valid, f, j]
            big, one = frames["largest"][valid, f, j], frames["single"][valid, f, j]
            some = n > 0
            m[side] = {"objects_mean": _mean(n), "objects_max": int(n.max()) if len(n) else 0,
                       "area_mean": float(area.sum() / n.sum()) if n.sum() else float("nan"),
                       "single_pixel_share": float(one.sum() / n.sum()) if n.sum() else float("nan"),
                       "largest_share_mean": _mean(big[some] / area[some])}
        res[key] = m
    return res


class ObjectEvaluator(Streaming):
    """Streaming object verification.  ``update(method, pred, truth)`` adds one piece whose frames pair one for one (the longer side is
    truncated, as align_length does), syncs once per launch to size the object table and sends the launch's results to pinned host
    memory; ``compute()`` waits for those copies and returns ``{method: {...}}`` (see
    ``run_objects``)."""

    what = "object verification runs"

    def __init__(self, crop_size: int, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, connectivity: int = 8,
                 sal_factor: float = DEFAULT_SAL_FACTOR, sal_floor: float = DEFAULT_SAL_FLOOR, divide_by_3: bool = True, device=None,
                 mode: str = "radar"):
        self.thresholds = radar_thresholds(mode, thresholds, "object verification labels connected pixels")
        self.connectivity, self.sal_factor, self.sal_floor = _check_sal(connectivity, sal_factor, sal_floor)
        self.size = bounded_crop(crop_size)
        self._start(device, divide_by_3)
        self.keys = level_keys(self.thresholds)
        self.use_workspace = self.size > ops.OBJECTS_LDS_CROP      # tests set it to run a small crop through the large-crop path

    def _new_state(self):
        return SimpleNamespace(rec=[], lev=[], offsets=[], table=[], origin=[], T=0)

    def _launch_frames(self):
        return _WORK_BYTES // (2 * len(self.keys) * self.size * self.size * (4 if self.use_workspace else 2))

    def update(self, method: str, pred_event, truth_event, origin=(0, 0)):
        """``origin`` = (event index, first frame) of the piece in the truth, recorded with its frames."""
        S, L = self.size, len(self.keys)
        with torch.cuda.device(self.device):
            pred, truth, ptl, gtl, n, st = self._open(method, pred_event, truth_event)
            wide = bool(self.use_workspace)
            ldt = torch.int32 if wide else torch.int16
            for t0, tn in self._cuts(n):
                q = self._buf("q", tn * 2 * S * S, torch.int32)
                bits = self._buf("bits", tn * 2 * S * S, torch.int16)
                labels = self._buf("labels", tn * 2 * L * S * S, ldt)
                rec = torch.empty(tn, 2, 5, device=self.device, dtype=torch.int64)
                lev = torch.empty(tn, 2, L, 5, device=self.device, dtype=torch.int64)
                counts = torch.empty(tn * 2 * L, device=self.device, dtype=torch.int64)
                offsets = torch.empty(tn * 2 * L + 1, device=self.device, dtype=torch.int64)
                for field, (x, tl) in enumerate(((pred[t0:t0 + tn], ptl), (truth[t0:t0 + tn], gtl))):
                    ops.objects_quantize(x, tl, field, S, self._lut, self.thresholds, self.sal_factor, self.sal_floor, self.divide_by_3,
                                         q, bits, rec)
                ops.objects_label(bits, tn, S, L, self.connectivity, labels, wide)
                ops.objects_count(labels, wide, q, tn, S, L, lev, counts)
                ops.objects_scan(counts, offsets)
                rows = int(offsets[-1].item())          # the one host read: the table holds every object, none is capped
                table = torch.zeros(rows, 6, device=self.device, dtype=torch.int64)
                ops.objects_fill(labels, wide, q, tn, S, L, offsets, table)
                # the results leave for pinned host memory behind the fill, so neither the device's memory nor compute's wait
                # grows with the number of objects
                for kept, t in ((st.rec, rec), (st.lev, lev), (st.offsets, offsets), (st.table, table)):
                    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                    host.copy_(t, non_blocking=True)
                    kept.append(host)
                st.origin.append((int(origin[0]), int(origin[1]) + t0, tn))
                st.T += tn

    def records(self, method: str) -> Dict[str, np.ndarray]:
        """The method's integers so far on the host (syncs): ``rec`` [T, 2, 5], ``lev`` [T, 2, L, 5], ``offsets`` [T * 2 * L + 1],
        ``table`` [N, 6] (see ``sal_frames``), and ``event``, ``frame`` [T]: where each frame lies in the truth."""
        st = self._methods[method]
        L = len(self.keys)
        self._arrived()
        offs, base = [np.zeros(1, np.int64)], 0
        for o in st.offsets:
            o = o.numpy()
            offs.append(o[1:] + base)
            base += int(o[-1])
        cat = lambda xs, shape: (torch.cat(xs).numpy() if xs else np.zeros(shape, np.int64))      # noqa: E731
        return {"rec": cat(st.rec, (0, 2, 5)), "lev": cat(st.lev, (0, 2, L, 5)), "offsets": np.concatenate(offs),
                "table": cat(st.table, (0, 6)),
                "event": np.concatenate([np.full(k, e, np.int64) for e, _, k in st.origin] or [np.zeros(0, np.int64)]),
                "frame": np.concatenate([np.arange(a, a + k, dtype=np.int64) for _, a, k in st.origin] or [np.zeros(0, np.int64)])}

    def _arrived(self):
        """Waits for the copies that the updates left in flight."""
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()

    def _score(self, job):
        st, i = job
        return sal_frames(self.size, *(x.numpy() for x in (st.rec[i], st.lev[i], st.offsets[i], st.table[i])))

    def compute(self, frames_out: Optional[dict] = None) -> Dict[str, Dict[str, object]]:
        """The metrics per method; with a dict ``frames_out`` the per-frame arrays of every method are left there as well.  Frames are
        scored independently, so every launch's tables are scored on their own (a piece's columns stay in cache, where
        a method's would stream from memory), a few pieces at a time on host threads."""
        from concurrent.futures import ThreadPoolExecutor
        for name, st in self._methods.items():
            if st.T == 0:
                raise ValueError(f"method {name!r} has no frames to score")
        self._arrived()
        jobs = [(st, i) for st in self._methods.values() for i in range(len(st.table))]
        with ThreadPoolExecutor(max_workers=_HOST_THREADS) as pool:
            parts = iter(list(pool.map(self._score, jobs)))
        res = {}
        for name, st in self._methods.items():
            mine = [next(parts) for _ in st.table]
            fr = {k: np.concatenate([p[k] for p in mine]) for k in mine[0]}
            fr["event"] = np.concatenate([np.full(k, e, np.int64) for e, _, k in st.origin])
            fr["frame"] = np.concatenate([np.arange(a, a + k, dtype=np.int64) for _, a, k in st.origin])
            res[name] = {"levels": sal_summary(fr, self.keys), "frames": st.T, "frames_skipped": int((~fr["valid"]).sum()),
                         "connectivity": self.connectivity, "sal_factor": self.sal_factor, "sal_floor": self.sal_floor}
            if frames_out is not None:
                frames_out[name] = fr
        return res


def run_objects(preds, truth, crop_size: int, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, connectivity: int = 8,
                sal_factor: float = DEFAULT_SAL_FACTOR, sal_floor: float = DEFAULT_SAL_FLOOR, divide_by_3: bool = True, device=None,
                mode: str = "radar", frames_out: Optional[dict] = None) -> Dict[str, Dict[str, object]]:
    """SAL and the object population of every method against the truth, with run_exp1's handling of event dicts (the truth's key
    order, an event a method lacks is skipped for that method, a method that is not a dict is left out).  Returns per method
    ``{"levels": {"thr_<q:g>" | "rel": {"S_mean", "S_median", ... "L2_median", "S_abs_mean", "A_abs_mean", "frames_scored",
    "frames_pred_only", "frames_truth_only", "frames_no_object", "pred": {...}, "truth": {...}}}, "frames": T, "frames_skipped": k,
    "connectivity", "sal_factor", "sal_floor"}`` (see ``sal_summary``); ``frames_out`` receives the per-frame arrays."""
    truth_events, methods = event_lists(preds, truth)
    if not truth_events:
        return {}
    ev = ObjectEvaluator(crop_size, thresholds, connectivity, sal_factor, sal_floor, divide_by_3, device=device, mode=mode)
    for name, p, g, origin in ev.pieces(truth_events, methods):
        ev.update(name, p, g, origin=origin)
    return ev.compute(frames_out)


def objects_lines(metrics) -> List[str]:
    """metrics.txt: ``SAL_<name>_<level>: S=.. A=.. L=..`` (medians) and ``OBJ_<name>_<level>: pred=.. truth=..`` (mean objects per
    frame) lines, 6 decimals."""
    lines = []
    for name, m in metrics.items():
        for key, v in m["levels"].items():
            tag = key.replace("_", "")
            lines.append(f"SAL_{name}_{tag}: S={v['S_median']:.6f} A={v['A_median']:.6f} L={v['L_median']:.6f}")
            lines.append(f"OBJ_{name}_{tag}: pred={v['pred']['objects_mean']:.6f} truth={v['truth']['objects_mean']:.6f}")
    return lines


def write_objects_figure(metrics, frames, path: str) -> Optional[str]:
    """One SAL diagram per level: S against A of every scored frame coloured by L, each method's medians marked (matplotlib, no display
    needed).  Without matplotlib, or without the per-frame arrays, it warns and writes nothing."""
    try:
        from matplotlib.figure import Figure
    except ImportError:
        warnings.warn("matplotlib is not importable: the SAL diagrams are skipped (the numbers are in objects_data.npz)")
        return None
    names = [n for n in metrics if frames and n in frames]
    if not names:
        warnings.warn("no per-frame scores were kept: the SAL diagrams are skipped")
        return None
    keys = list(metrics[names[0]]["levels"])
    fig = Figure(figsize=(4 * len(keys), 3.8), dpi=200)
    axes = fig.subplots(1, len(keys), squeeze=False)[0]
    markers = "osD^vP*X"
    for j, (ax, key) in enumerate(zip(axes, keys)):
        sc = None
        for i, name in enumerate(names):
            fr = frames[name]
            ok = ~np.isnan(fr["S"][:, j])
            sc = ax.scatter(fr["S"][ok, j], fr["A"][ok, j], c=fr["L"][ok, j], s=6, vmin=0.0, vmax=1.0, cmap="viridis",
                            marker=markers[i % len(markers)], linewidths=0)
            m = metrics[name]["levels"][key]
            ax.plot([m["S_median"]], [m["A_median"]], marker=markers[i % len(markers)], markersize=8, markerfacecolor="none",
                    markeredgecolor="k", linestyle="none", label=name)
        ax.axhline(0.0, color="0.6", linewidth=0.5)
        ax.axvline(0.0, color="0.6", linewidth=0.5)
        ax.set_xlim(-2.0, 2.0)
        ax.set_ylim(-2.0, 2.0)
        ax.set_xlabel("S")
        ax.set_ylabel("A")
        ax.set_title("R >= R*" if key == RELATIVE_LEVEL else f">= {key[4:]} mm/h", fontsize=10)
        if sc is not None and j == len(keys) - 1:
            fig.colorbar(sc, ax=ax, label="L")
    if names:
        axes[0].legend(frameon=True, fontsize=8)
    fig.tight_layout()
    fig.savefig(path, format="pdf", bbox_inches="tight")
    return path


def write_objects_outputs(out_dir: str, metrics, frames=None) -> None:
    """DIR/metrics.json (indent 2, sorted keys), DIR/metrics.txt (``objects_lines``), DIR/objects_data.npz (per method the per-frame
    S, A, L, L1, L2 [T, levels], counts, areas, largest and single-pixel objects [T, 2, levels], valid, event, frame) and
    DIR/objects_panels.pdf."""
    import json
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "metrics.json"), "w", encoding="utf-8") as f:
        json.dump(metrics, f, indent=2, sort_keys=True)
    with open(os.path.join(out_dir, "metrics.txt"), "w", encoding="utf-8") as f:
        for line in objects_lines(metrics):
            f.write(line + "\n")
    arrays = {"methods": np.array(list(metrics))}
    for name, m in metrics.items():
        arrays[f"{name}/levels"] = np.array(list(m["levels"]))
        for k, v in (frames or {}).get(name, {}).items():
            arrays[f"{name}/{k}"] = np.asarray(v)
    np.savez(os.path.join(out_dir, "objects_data.npz"), **arrays)
    write_objects_figure(metrics, frames, os.path.join(out_dir, "objects_panels.pdf"))
