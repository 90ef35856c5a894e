"""Probabilistic verification on csrc/eval_prob.hip: a prediction and its variance as the Gaussian N(mu, sigma^2), left-censored at
0 by default, scored against the truth on the 0-255 scale: CRPS, the PIT histogram, coverage and sharpness of central intervals, the
standardised error, spread against skill per sigma-bin, and Brier score / reliability / ROC area of the rain-rate exceedances.
``ProbEvaluator`` streams aligned pieces and syncs once in ``compute``; ``run_prob`` scores every method "dressed" (one variance,
its own in-sample MSE) and, where it has a variance map, with the map; ``run_prob_points`` does the same for flat cross-validation
columns.  DESIGN.md section 22 holds the definitions; tests/prob_ref.py restates them in numpy / scipy."""
from __future__ import annotations

import math
import os
import warnings
from statistics import NormalDist
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ._common import Streaming, _pieces, _thw, _to_device, crop_origin, eval_device, selection, transform_mmhr, upload_events
from .exp1 import DEFAULT_THRESHOLDS

DEFAULT_LEVELS = (0.5, 0.8, 0.9, 0.95)
DEFAULT_SIGMA_EDGES = tuple(float(v) for v in np.geomspace(0.5, 64.0, 12))
DEFAULT_PIT_BINS = 20
DEFAULT_REL_BINS = 10
_FIX = 2.0 ** 32
_PART_WORDS = 1 << 24            # partial records per launch: at most 128 MB


def half_width(level: float) -> float:
    """h = Phi^-1((1 + level) / 2): the central interval of that nominal level is mu -+ h sigma."""
    if not 0.0 < level < 1.0:
        raise ValueError(f"an interval level lies in (0, 1), got {level}")
    return NormalDist().inv_cdf((1.0 + float(level)) / 2.0)


def pixel_threshold(q: float, divide_by_3: bool = True) -> float:
    """x_q on the 0-255 scale with transform_mmhr(x) >= q <=> x >= x_q (the transform is monotone there).  Refuses a threshold at or
    below the transform's floor transform_mmhr(0.001) (every pixel exceeds it) or above its cap of 200 mm/h (none does)."""
    floor = float(transform_mmhr(0.001, divide_by_3))
    if not floor < q <= 200.0:
        raise ValueError(f"threshold {q} mm/h: exceedance probabilities need {floor:.6g} < q <= 200")
    return (48.0 if divide_by_3 else 16.0) * math.log10(q / 0.036)


class _Layout:
    """Word offsets of the record's sections (include/p2i_hip.h): fp64 sections first, then int64."""

    def __init__(self, K, L, E, NB, RB):
        NS = E + 1
        self.K, self.L, self.NS, self.NB, self.RB = K, L, NS, NB, RB
        f = 7
        self.f_w, f = f, f + L
        self.f_p, f = f, f + K
        self.f_br, f = f, f + K
        self.f_sv, f = f, f + NS
        self.f_se, f = f, f + NS
        self.nf = f
        i = 3
        self.i_in, i = i, i + L
        self.i_o, i = i, i + K
        self.i_pit, i = i, i + NB
        self.i_pre, i = i, i + NB
        self.i_sn, i = i, i + NS
        self.i_rn, i = i, i + K * RB
        self.i_ro, i = i, i + K * RB
        self.i_rp, i = i, i + K * RB
        self.ni = i


def _div(a, b) -> float:
    return float(a) / float(b) if b else float("nan")


def roc_area(count: Sequence[int], events: Sequence[int]) -> float:
    """The ROC area by the trapezoid rule over the reliability table's bin edges: "warn when p falls in bin >= c", c = RB .. 0."""
    n, o = np.asarray(count, np.float64), np.asarray(events, np.float64)
    ev, ne = o.sum(), (n - o).sum()
    if ev == 0 or ne == 0:
        return float("nan")
    pod = np.concatenate([[0.0], np.cumsum(o[::-1]) / ev])
    pofd = np.concatenate([[0.0], np.cumsum((n - o)[::-1]) / ne])
    return float(np.sum(0.5 * (pod[1:] + pod[:-1]) * np.diff(pofd)))


def unpack_record(F: np.ndarray, I: np.ndarray, lay: _Layout) -> Dict[str, object]:
    """The accumulator's sections by name; the fixed-point sections as floats, the PIT prefix table folded into the histogram."""
    K, L, NS, NB, RB = lay.K, lay.L, lay.NS, lay.NB, lay.RB
    pit = I[lay.i_pit:lay.i_pit + NB].astype(np.float64) + np.cumsum(I[lay.i_pre:lay.i_pre + NB][::-1].astype(np.float64))[::-1]
    return {"crps": F[0], "e": F[1], "ae": F[2], "e2": F[3], "s2": F[4], "z": F[5], "z2": F[6], "width": F[lay.f_w:lay.f_w + L],
            "p": F[lay.f_p:lay.f_p + K], "brier": F[lay.f_br:lay.f_br + K], "sb_s2": F[lay.f_sv:lay.f_sv + NS],
            "sb_e2": F[lay.f_se:lay.f_se + NS], "n": int(I[0]), "n_skipped": int(I[1]), "n_zero_var": int(I[2]),
            "inside": I[lay.i_in:lay.i_in + L], "o": I[lay.i_o:lay.i_o + K], "pit": pit / _FIX, "sb_n": I[lay.i_sn:lay.i_sn + NS],
            "rel_n": I[lay.i_rn:lay.i_rn + K * RB].reshape(K, RB), "rel_o": I[lay.i_ro:lay.i_ro + K * RB].reshape(K, RB),
            "rel_p": I[lay.i_rp:lay.i_rp + K * RB].reshape(K, RB).astype(np.float64) / _FIX}


def prob_scores(s: Dict[str, object], thresholds, levels, sigma_edges) -> Dict[str, object]:
    """The reported scores from the named sums.  Means over the scored pixels (the z moments over those with sigma > 0); NaN where
    nothing was scored."""
    n, nz = s["n"], s["n"] - s["n_zero_var"]
    with np.errstate(all="ignore"):
        res = {"n": n, "n_skipped": s["n_skipped"], "n_zero_var": s["n_zero_var"], "CRPS": _div(s["crps"], n), "ME": _div(s["e"], n),
               "MAE": _div(s["ae"], n), "MSE": _div(s["e2"], n), "RMSE": math.sqrt(_div(s["e2"], n)) if n else float("nan"), "mean_var": _div(s["s2"], n),
               "z_mean": _div(s["z"], nz), "MSDR": _div(s["z2"], nz)}
        res["z_var"] = res["MSDR"] - res["z_mean"] ** 2
        res["coverage"] = {f"{lev:g}": _div(s["inside"][k], n) for k, lev in enumerate(levels)}
        res["sharpness"] = {f"{lev:g}": _div(s["width"][k], n) for k, lev in enumerate(levels)}
        tot = float(np.sum(s["pit"]))
        res["pit"] = [_div(v, tot) for v in s["pit"]]
        res["spread_skill"] = {"edges": [float(v) for v in sigma_edges], "count": [int(v) for v in s["sb_n"]],
                               "spread": [float(np.sqrt(_div(a, c))) for a, c in zip(s["sb_s2"], s["sb_n"])],
                               "rmse": [float(np.sqrt(_div(a, c))) for a, c in zip(s["sb_e2"], s["sb_n"])]}
        res["exceedance"] = {}
        for k, q in enumerate(thresholds):
            base, bs = _div(s["o"][k], n), _div(s["brier"][k], n)
            res["exceedance"][f"thr_{q:g}"] = {
                "base_rate": base, "mean_p": _div(s["p"][k], n), "brier": bs,
                "bss": 1.0 - bs / (base * (1.0 - base)) if n and 0.0 < base < 1.0 else float("nan"),
                "roc_area": roc_area(s["rel_n"][k], s["rel_o"][k]),
                "reliability": {"count": [int(v) for v in s["rel_n"][k]],
                                "mean_p": [_div(a, c) for a, c in zip(s["rel_p"][k], s["rel_n"][k])],
                                "obs_freq": [_div(a, c) for a, c in zip(s["rel_o"][k], s["rel_n"][k])]}}
    return res


def _crop_shape(crop_size):
    rows, cols = (crop_size, crop_size) if np.isscalar(crop_size) else crop_size
    rows, cols = int(rows), int(cols)
    if rows < 1 or cols < 1:
        raise ValueError(f"crop {rows}x{cols}")
    return rows, cols


class ProbEvaluator(Streaming):
    """Streaming probabilistic scores.  ``update(method, pred, truth, var)`` adds one piece whose frames pair one for one (the
    longer side is truncated); ``var`` is an array aligned with ``pred`` or a float (one variance for every pixel).  ``crop_size`` is
    an int or (rows, cols): the centre crop of every input.  ``mask`` [rows, cols] with ``mode`` selects exp1's pixels (radar: mask
    False, gauge: mask True); without a mask every pixel counts.  ``compute()`` syncs once and returns ``{method: scores}``."""

    what = "probabilistic verification runs"

    def __init__(self, crop_size, mask=None, mode: str = "radar", thresholds: Sequence[float] = DEFAULT_THRESHOLDS,
                 levels: Sequence[float] = DEFAULT_LEVELS, sigma_edges: Sequence[float] = DEFAULT_SIGMA_EDGES,
                 pit_bins: int = DEFAULT_PIT_BINS, rel_bins: int = DEFAULT_REL_BINS, censor: bool = True, divide_by_3: bool = True,
                 device=None):
        if mode not in ("radar", "gauge"):
            raise ValueError(f"Unknown mode: {mode}")
        self.size = self.rows, self.cols = _crop_shape(crop_size)
        self.divide_by_3, self.censor = bool(divide_by_3), bool(censor)
        self.thresholds = tuple(float(q) for q in thresholds)
        self.levels = tuple(float(v) for v in levels)
        self.sigma_edges = tuple(float(v) for v in sigma_edges)
        self.pit_bins, self.rel_bins = int(pit_bins), int(rel_bins)
        if len(self.thresholds) > ops.EXP1_MAX_THR:
            raise ValueError(f"at most {ops.EXP1_MAX_THR} thresholds")
        if len(self.levels) > ops.PROB_MAX_LEVELS:
            raise ValueError(f"at most {ops.PROB_MAX_LEVELS} interval levels")
        if len(self.sigma_edges) > ops.PROB_MAX_EDGES or any(b <= a for a, b in zip(self.sigma_edges, self.sigma_edges[1:])):
            raise ValueError(f"sigma_edges: at most {ops.PROB_MAX_EDGES} ascending edges")
        if not 1 <= self.pit_bins <= ops.PROB_MAX_PIT_BINS or not 1 <= self.rel_bins <= ops.PROB_MAX_REL_BINS:
            raise ValueError(f"pit_bins in 1..{ops.PROB_MAX_PIT_BINS}, rel_bins in 1..{ops.PROB_MAX_REL_BINS}")
        self.xq = tuple(pixel_threshold(q, self.divide_by_3) for q in self.thresholds)
        self.halfwidths = tuple(half_width(v) for v in self.levels)
        self._start(device, divide_by_3, None if mask is None else selection(mask, mode, self.size))
        self.layout = _Layout(len(self.thresholds), len(self.levels), len(self.sigma_edges), self.pit_bins, self.rel_bins)
        if ops.prob_record(len(self.thresholds), len(self.levels), len(self.sigma_edges), self.pit_bins, self.rel_bins) != \
                (self.layout.nf, self.layout.ni):
            raise RuntimeError("the record layout of prob.py and csrc/eval_prob.hip differ")

    def _new_state(self):
        """The method's accumulator: one record."""
        return torch.zeros(self.layout.nf + self.layout.ni, device=self.device, dtype=torch.float64)

    def _launch_frames(self):
        return (_PART_WORDS // (self.layout.nf + self.layout.ni)) * ops.PROB_WG_PIXELS // (self.rows * self.cols)

    def update(self, method, pred_event, truth_event, var):
        rows, cols, lay = self.rows, self.cols, self.layout
        nw = lay.nf + lay.ni
        with torch.cuda.device(self.device):
            # its own opening: the variance rides along, and here the prediction's crop is checked ahead of the truth's
            pred, truth = self._upload(pred_event, truth_event)
            scalar = not (isinstance(var, (torch.Tensor, np.ndarray)) and getattr(var, "ndim", 0) > 0)
            v = float(var) if scalar else _to_device(_thw(var), self.device)
            if not scalar and v.shape[0] != pred.shape[0]:
                raise ValueError(f"the variance has {v.shape[0]} frames, the prediction {pred.shape[0]}")
            n = min(pred.shape[0], truth.shape[0])
            ptl = crop_origin(pred.shape[1], pred.shape[2], self.size)
            gtl = crop_origin(truth.shape[1], truth.shape[2], self.size)
            vtl = None if scalar else crop_origin(v.shape[1], v.shape[2], self.size)
            acc = self._state(method)
            for t0, tn in self._cuts(n):
                nwg = -(-tn * rows * cols // ops.PROB_WG_PIXELS)
                part = torch.empty(nwg * nw, device=self.device, dtype=torch.float64)
                ops.prob_accumulate(pred[t0:t0 + tn], v if scalar else v[t0:t0 + tn], truth[t0:t0 + tn], ptl, vtl, gtl, rows, cols,
                                    self._rank, self._lut, self.thresholds, self.xq, self.halfwidths, self.sigma_edges, self.pit_bins,
                                    self.rel_bins, self.censor, self.divide_by_3, part)
                ops.prob_merge(part, lay.nf, lay.ni, acc)

    def raw(self, method) -> torch.Tensor:
        """The method's accumulator on the device: nf fp64 words, then ni int64 words as their bits."""
        return self._methods[method]

    def sums(self, method) -> Dict[str, object]:
        """The method's sums so far by name (``unpack_record``); syncs.  For checks: ``compute`` is the product path."""
        row = self._methods[method].cpu().numpy()
        return unpack_record(row[:self.layout.nf], np.ascontiguousarray(row[self.layout.nf:]).view(np.int64), self.layout)

    def compute(self) -> Dict[object, Dict[str, object]]:
        names = list(self._methods)
        if not names:
            return {}
        with torch.cuda.device(self.device):
            host = torch.stack([self._methods[k] for k in names]).cpu().numpy()         # the one host sync
        nf = self.layout.nf
        return {name: prob_scores(unpack_record(row[:nf], np.ascontiguousarray(row[nf:]).view(np.int64), self.layout),
                                  self.thresholds, self.levels, self.sigma_edges) for name, row in zip(names, host)}


def _score_methods(ev_args, pieces_of, names, has_map):
    """Both passes over every method.  pieces_of(name) yields aligned (pred, truth, var-or-None) pieces on the device."""
    first = ProbEvaluator(**ev_args)
    cache = {name: list(pieces_of(name)) for name in names}
    for name in names:
        for p, g, _ in cache[name]:
            first.update(name, p, g, 0.0)             # sigma^2 = 0: the point-forecast pass that yields the method's own MSE
    point = first.compute()
    ev = ProbEvaluator(**ev_args)
    mse = {}
    for name in names:
        if name not in point or point[name]["n"] == 0:
            raise ValueError(f"method {name!r} has no pixels to score")
        mse[name] = point[name]["MSE"]
        for p, g, v in cache[name]:
            ev.update((name, "dressed"), p, g, mse[name])
            if has_map(name):
                ev.update((name, "map"), p, g, v)
    scored = ev.compute()
    res = {}
    for name in names:
        d = scored[(name, "dressed")]
        d["sigma0_sq"], d["sigma0_sq_in_sample"] = mse[name], True
        res[name] = {"dressed": d}
        if (name, "map") in scored:
            res[name]["map"] = scored[(name, "map")]
            res[name]["CRPSS_map_vs_dressed"] = 1.0 - _div(res[name]["map"]["CRPS"], d["CRPS"])
    return res


def run_prob(preds, variances, truth, mask=None, mode: str = "radar", crop_size=None, thresholds: Sequence[float] = DEFAULT_THRESHOLDS,
             levels: Sequence[float] = DEFAULT_LEVELS, sigma_edges: Sequence[float] = DEFAULT_SIGMA_EDGES,
             pit_bins: int = DEFAULT_PIT_BINS, rel_bins: int = DEFAULT_REL_BINS, censor: bool = True, divide_by_3: bool = True,
             device=None) -> Dict[str, Dict[str, object]]:
    """Every method of ``preds`` scored twice against ``truth`` (arrays or event dicts, run_exp1's rules), on the 0-255 scale:
    "dressed" -- the Gaussian N(pred, sigma0^2) with sigma0^2 the method's own MSE over its scored pixels, which is IN-SAMPLE (the
    same pixels fit it and are scored with it; ``sigma0_sq_in_sample`` says so in the output) -- and, where ``variances`` has the
    method, "map" -- N(pred, variance map).  ``CRPSS_map_vs_dressed`` = 1 - CRPS_map / CRPS_dressed tells whether the variance
    pattern carries information beyond one global error bar.  Returns ``{method: {"dressed": scores, ["map": scores,
    "CRPSS_map_vs_dressed": v]}}``."""
    dev = eval_device(device, "probabilistic verification runs")
    if crop_size is None:
        raise ValueError("crop_size is required")
    variances = variances or {}
    unknown = [k for k in variances if k not in preds]
    if unknown:
        raise ValueError(f"variance for unknown method(s) {unknown}")
    if isinstance(truth, dict):
        keys = [k for k in truth if truth.get(k) is not None]
        for name, src in preds.items():
            if not isinstance(src, dict):
                raise TypeError(f"method {name!r}: a per-event truth needs per-event predictions")
            if name in variances:
                missing = [k for k in keys if src.get(k) is not None and variances[name].get(k) is None]
                if missing:
                    raise ValueError(f"variance of {name!r} lacks event(s) {missing}")
        truth_events = [truth[k] for k in keys]
        events = {name: ([src[k] for k in keys if src.get(k) is not None],
                         [variances[name][k] for k in keys if src.get(k) is not None] if name in variances else None)
                  for name, src in preds.items()}
    else:
        truth_events = [truth]
        events = {name: ([src], [variances[name]] if name in variances else None) for name, src in preds.items()}
    if not truth_events:
        return {}
    truth_dev = upload_events(truth_events, dev)

    def pieces_of(name):
        pe, ve = events[name]
        pd = upload_events(pe, dev)
        if ve is None:
            for p, g in _pieces(pd, truth_dev):
                yield p, g, None
            return
        vd = upload_events(ve, dev)
        for p, v in zip(pd, vd):
            if p.shape[0] != v.shape[0]:
                raise ValueError(f"method {name!r}: a variance event has {v.shape[0]} frames, its prediction {p.shape[0]}")
        # predictions and variances share their event boundaries, so the same cuts align both with the truth
        for (p, g), (v, _) in zip(_pieces(pd, truth_dev), _pieces(vd, truth_dev)):
            yield p, g, v

    args = dict(crop_size=crop_size, mask=mask, mode=mode, thresholds=thresholds, levels=levels, sigma_edges=sigma_edges,
                pit_bins=pit_bins, rel_bins=rel_bins, censor=censor, divide_by_3=divide_by_3, device=dev)
    names = [n for n in preds if events[n][0]]
    return _score_methods(args, pieces_of, names, lambda n: events[n][1] is not None)


def run_prob_points(z, pred, var=None, output_scale: float = 1.0, name: str = "cv", thresholds: Sequence[float] = DEFAULT_THRESHOLDS,
                    levels: Sequence[float] = DEFAULT_LEVELS, sigma_edges: Sequence[float] = DEFAULT_SIGMA_EDGES,
                    pit_bins: int = DEFAULT_PIT_BINS, rel_bins: int = DEFAULT_REL_BINS, censor: bool = True, divide_by_3: bool = True,
                    device=None) -> Dict[str, Dict[str, object]]:
    """``run_prob`` for flat cross-validation columns (observed z, predicted, predictive variance, any shape, NaN where a point has
    none): values * output_scale, variance * output_scale^2, scored as one 1 x n piece.  ``var=None`` gives the dressed entry only."""
    dev = eval_device(device, "probabilistic verification runs")
    s = float(output_scale)
    flat = lambda a: (np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64).reshape(1, 1, -1))   # noqa: E731
    zz, pp = flat(z) * s, flat(pred) * s
    vv = None if var is None else flat(var) * (s * s)
    n = zz.shape[-1]
    if n == 0 or pp.shape != zz.shape or (vv is not None and vv.shape != zz.shape):
        raise ValueError("z, pred and var are columns of one length >= 1")
    zd, pd = _to_device(zz, dev), _to_device(pp, dev)
    vd = None if vv is None else _to_device(vv, dev)
    args = dict(crop_size=(1, n), mask=None, mode="radar", thresholds=thresholds, levels=levels, sigma_edges=sigma_edges,
                pit_bins=pit_bins, rel_bins=rel_bins, censor=censor, divide_by_3=divide_by_3, device=dev)
    return _score_methods(args, lambda _: iter([(pd, zd, vd)]), [name], lambda _: vd is not None)


def _entries(result):
    """(label, scores) of every scored entry: ``<method>_dressed`` and ``<method>_map``."""
    for name, m in result.items():
        for kind in ("dressed", "map"):
            if kind in m:
                yield f"{name}_{kind}", m[kind]


def prob_lines(result) -> List[str]:
    """metrics.txt: ``CRPS_<name>_<kind>: v``, ``COV<level %>_<..>``, ``MSDR_<..>``, ``BRIER_<..>_thr<q>``, ``BSS``, ``ROC`` and
    ``CRPSS_<name>`` lines, 6 decimals."""
    lines = []
    for label, s in _entries(result):
        lines.append(f"CRPS_{label}: {s['CRPS']:.6f}")
        lines.append(f"RMSE_{label}: {s['RMSE']:.6f}")
        lines.append(f"MSDR_{label}: {s['MSDR']:.6f}")
        for lev, v in s["coverage"].items():
            lines.append(f"COV{float(lev) * 100:g}_{label}: {v:.6f}")
        for lev, v in s["sharpness"].items():
            lines.append(f"WIDTH{float(lev) * 100:g}_{label}: {v:.6f}")
        for tk, e in s["exceedance"].items():
            t = tk.replace("_", "")
            lines.append(f"BRIER_{label}_{t}: {e['brier']:.6f}")
            lines.append(f"BSS_{label}_{t}: {e['bss']:.6f}")
            lines.append(f"ROC_{label}_{t}: {e['roc_area']:.6f}")
        lines.append(f"NSKIPPED_{label}: {s['n_skipped']}")
        lines.append(f"NZEROVAR_{label}: {s['n_zero_var']}")
    for name, m in result.items():
        if "CRPSS_map_vs_dressed" in m:
            lines.append(f"CRPSS_{name}: {m['CRPSS_map_vs_dressed']:.6f}")
    return lines


def prob_arrays(result) -> Dict[str, np.ndarray]:
    """prob_data.npz: per entry the PIT histogram, the coverage, spread-skill and reliability tables and the scalar scores."""
    arrays = {"entries": np.array([label for label, _ in _entries(result)])}
    for label, s in _entries(result):
        arrays[f"{label}/pit"] = np.asarray(s["pit"], dtype=np.float64)
        arrays[f"{label}/levels"] = np.array([float(k) for k in s["coverage"]])
        arrays[f"{label}/coverage"] = np.array(list(s["coverage"].values()), dtype=np.float64)
        arrays[f"{label}/sharpness"] = np.array(list(s["sharpness"].values()), dtype=np.float64)
        for k in ("edges", "count", "spread", "rmse"):
            arrays[f"{label}/spread_skill_{k}"] = np.asarray(s["spread_skill"][k], dtype=np.float64)
        thr = list(s["exceedance"])
        arrays[f"{label}/thresholds"] = np.array([float(tk[4:]) for tk in thr])
        for k in ("count", "mean_p", "obs_freq"):
            arrays[f"{label}/reliability_{k}"] = np.array([s["exceedance"][tk]["reliability"][k] for tk in thr], dtype=np.float64)
        arrays[f"{label}/exceedance"] = np.array([[s["exceedance"][tk][k] for k in ("base_rate", "mean_p", "brier", "bss", "roc_area")]
                                                  for tk in thr], dtype=np.float64).reshape(len(thr), 5)
        arrays[f"{label}/scores"] = np.array([s[k] for k in ("CRPS", "ME", "MAE", "RMSE", "mean_var", "z_mean", "z_var", "MSDR", "n",
                                                             "n_skipped", "n_zero_var")], dtype=np.float64)
    return arrays


def write_prob_figure(result, path: str) -> Optional[str]:
    """Four panels: PIT histograms, reliability diagrams (the first threshold), spread against skill, coverage against nominal
    (matplotlib, no display needed).  Without matplotlib it warns and writes nothing."""
    try:
        from matplotlib.figure import Figure
    except ImportError:
        warnings.warn("matplotlib is not importable: the probability figure is skipped (the numbers are in prob_data.npz)")
        return None
    entries = list(_entries(result))
    fig = Figure(figsize=(16, 3.6), dpi=200)
    ax_pit, ax_rel, ax_ss, ax_cov = fig.subplots(1, 4)
    for label, s in entries:
        nb = len(s["pit"])
        ax_pit.step((np.arange(nb) + 0.5) / nb, np.asarray(s["pit"]) * nb, where="mid", label=label)
        if s["exceedance"]:
            tk = next(iter(s["exceedance"]))
            r = s["exceedance"][tk]["reliability"]
            ax_rel.plot(r["mean_p"], r["obs_freq"], marker="o", markersize=3, label=label)
            ax_rel.set_title(f"reliability, >= {tk[4:]} mm/h", fontsize=10)
        ax_ss.loglog(s["spread_skill"]["spread"], s["spread_skill"]["rmse"], marker="o", markersize=3, label=label)
        lev = [float(k) for k in s["coverage"]]
        ax_cov.plot(lev, list(s["coverage"].values()), marker="o", markersize=3, label=label)
    ax_pit.axhline(1.0, color="k", linewidth=0.8)
    ax_pit.set_xlabel("PIT")
    ax_pit.set_ylabel("density")
    ax_pit.set_title("PIT histogram", fontsize=10)
    for ax in (ax_rel, ax_cov):
        ax.plot([0, 1], [0, 1], color="k", linewidth=0.8)
    ax_rel.set_xlabel("forecast probability")
    ax_rel.set_ylabel("observed frequency")
    lim = [v for _, s in entries for k in ("spread", "rmse") for v in s["spread_skill"][k] if np.isfinite(v) and v > 0]
    if lim:
        ax_ss.plot([min(lim), max(lim)], [min(lim), max(lim)], color="k", linewidth=0.8)
    ax_ss.set_xlabel("RMS spread per sigma-bin")
    ax_ss.set_ylabel("RMSE per sigma-bin")
    ax_ss.set_title("spread - skill", fontsize=10)
    ax_cov.set_xlabel("nominal level")
    ax_cov.set_ylabel("coverage")
    ax_cov.set_title("central intervals", fontsize=10)
    if entries:
        ax_pit.legend(frameon=True, fontsize=7)
    fig.tight_layout()
    fig.savefig(path, format="pdf", bbox_inches="tight")
    return path


def write_prob_outputs(out_dir: str, result, stem: str = "metrics", figure: bool = True) -> None:
    """DIR/<stem>.json (indent 2, sorted keys), DIR/<stem>.txt (``prob_lines``), DIR/prob_data.npz and DIR/prob_panels.pdf."""
    import json
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{stem}.json"), "w", encoding="utf-8") as f:
        json.dump(result, f, indent=2, sort_keys=True)
    with open(os.path.join(out_dir, f"{stem}.txt"), "w", encoding="utf-8") as f:
        for line in prob_lines(result):
            f.write(line + "\n")
    np.savez(os.path.join(out_dir, "prob_data.npz"), **prob_arrays(result))
    if figure:
        write_prob_figure(result, os.path.join(out_dir, "prob_panels.pdf"))
