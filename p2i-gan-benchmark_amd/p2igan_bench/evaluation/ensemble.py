"""Ensemble verification on csrc/eval_ens.hip: M members scored against the truth on the 0-255 scale.  Per point (a pixel, or the
mean over an s x s box): CRPS and fair CRPS, the error of the ensemble mean, spread against skill, the rank histogram with a
deterministic tie rule, and Brier score / reliability / ROC area of the rain-rate exceedances from the member counts.  Per frame: the
energy score and the variogram score of order 1/2.  A deterministic field is a one-member ensemble.  ``EnsembleEvaluator`` streams
pieces and syncs once in ``compute``; ``run_ensemble`` scores named ensembles.  DESIGN.md section 25 holds the definitions;
tests/ens_ref.py restates them in numpy.  Box values are means on the 0-255 scale, not areal rain rates."""
from __future__ import annotations

import math
import os
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ._common import Streaming, _thw, _to_device, crop_origin, selection
from .exp1 import DEFAULT_THRESHOLDS
from .prob import DEFAULT_SIGMA_EDGES, _crop_shape, _div, pixel_threshold, roc_area

DEFAULT_BOX_SIZES = (1, 4, 16)
DEFAULT_OFFSETS = tuple(o for h in (1, 2, 4, 8) for o in ((0, h), (h, 0), (h, h), (h, -h)))
_FIX = 1 << 32
_PART_WORDS = 1 << 24            # partial records per launch: at most 128 MB
_ENERGY_FRAMES = 1 << 16


class _Layout:
    """Word offsets of the per-point record's sections (include/p2i_ens.h): fp64 sections first, then int64."""

    def __init__(self, M, K, E):
        NS = E + 1
        self.M, self.K, self.NS = M, K, NS
        f = 6
        self.f_p, f = f, f + K
        self.f_br, f = f, f + K
        self.f_sv, f = f, f + NS
        self.f_se, f = f, f + NS
        self.nf = f
        i = 2
        self.i_o, i = i, i + K
        self.i_rk, i = i, i + M + 2
        self.i_sn, i = i, i + NS
        self.i_rn, i = i, i + K * (M + 1)
        self.i_ro, i = i, i + K * (M + 1)
        self.ni = i


def unpack_record(F: np.ndarray, I: np.ndarray, lay: _Layout) -> Dict[str, object]:
    """The accumulator's sections by name; the rank histogram (units of 2^-32 points) is the running sum of its stored differences."""
    M, K, NS = lay.M, lay.K, lay.NS
    return {"crps": F[0], "crps_fair": F[1], "e": F[2], "ae": F[3], "e2": F[4], "s2": F[5], "p": F[lay.f_p:lay.f_p + K],
            "brier": F[lay.f_br:lay.f_br + K], "sb_s2": F[lay.f_sv:lay.f_sv + NS], "sb_e2": F[lay.f_se:lay.f_se + NS],
            "n": int(I[0]), "n_skipped": int(I[1]), "o": I[lay.i_o:lay.i_o + K], "rank": np.cumsum(I[lay.i_rk:lay.i_rk + M + 1]),
            "sb_n": I[lay.i_sn:lay.i_sn + NS], "rel_n": I[lay.i_rn:lay.i_rn + K * (M + 1)].reshape(K, M + 1),
            "rel_o": I[lay.i_ro:lay.i_ro + K * (M + 1)].reshape(K, M + 1)}


def ens_scores(s: Dict[str, object], M: int, thresholds, sigma_edges) -> Dict[str, object]:
    """The reported scores of one box size from the named sums: means over the scored points, NaN where nothing was scored; the fair
    CRPS, the variance and what follows from it are NaN for one member."""
    n = s["n"]
    nan = float("nan")
    with np.errstate(all="ignore"):
        mse = _div(s["e2"], n)
        var = _div(s["s2"], n) if M > 1 else nan
        res = {"M": int(M), "n": n, "n_skipped": s["n_skipped"], "CRPS": _div(s["crps"], n),
               "CRPS_fair": _div(s["crps_fair"], n) if M > 1 else nan, "ME": _div(s["e"], n), "MAE": _div(s["ae"], n), "MSE": mse,
               "RMSE": math.sqrt(mse) if n else nan, "mean_var": var,
               "spread_skill_ratio": math.sqrt((M + 1) / M * var / mse) if n and M > 1 and mse > 0 else nan}
        tot = float(np.sum(np.asarray(s["rank"], np.float64)))
        hist = [_div(float(v), tot) for v in s["rank"]]
        res["rank_histogram"] = hist
        res["outlier_share"] = hist[0] + hist[-1]
        res["reliability_index"] = float(sum(abs(f - 1.0 / (M + 1)) for f in hist))
        res["spread_skill"] = {"edges": [float(v) for v in sigma_edges], "count": [int(v) for v in s["sb_n"]],
                               "spread": [float(np.sqrt(_div(a, c))) for a, c in zip(s["sb_s2"], s["sb_n"])],
                               "rmse": [float(np.sqrt(_div(a, c))) for a, c in zip(s["sb_e2"], s["sb_n"])]}
        res["exceedance"] = {}
        for k, q in enumerate(thresholds):
            base, bs = _div(s["o"][k], n), _div(s["brier"][k], n)
            res["exceedance"][f"thr_{q:g}"] = {
                "base_rate": base, "mean_p": _div(s["p"][k], n), "brier": bs,
                "bss": 1.0 - bs / (base * (1.0 - base)) if n and 0.0 < base < 1.0 else nan,
                "roc_area": roc_area(s["rel_n"][k], s["rel_o"][k]),
                "reliability": {"count": [int(v) for v in s["rel_n"][k]],
                                "obs_freq": [_div(a, c) for a, c in zip(s["rel_o"][k], s["rel_n"][k])]}}
    return res


def energy_scores(frames: np.ndarray) -> Dict[str, object]:
    """frames [n, 4]: per frame (d, ES, ES_fair, mean distance to the truth).  The means over the frames with d > 0 of ES / sqrt(d)
    and ES_fair / sqrt(d), and the per-frame series."""
    frames = np.asarray(frames, np.float64).reshape(-1, 4)
    keep = frames[:, 0] > 0
    f = frames[keep]
    with np.errstate(all="ignore"):
        rd = np.sqrt(f[:, 0])
        return {"n_frames": int(keep.sum()), "n_frames_skipped": int((~keep).sum()),
                "ES_norm": float(np.mean(f[:, 1] / rd)) if len(f) else float("nan"),
                "ES_fair_norm": float(np.mean(f[:, 2] / rd)) if len(f) else float("nan"),
                "frames": {"d": [int(v) for v in frames[:, 0]], "ES": [float(v) for v in frames[:, 1]],
                           "ES_fair": [float(v) for v in frames[:, 2]], "dist_truth": [float(v) for v in frames[:, 3]]}}


def variogram_scores(frames: np.ndarray, offsets) -> Dict[str, object]:
    """frames [n, nof, 2]: per frame and offset (V_o, n_o).  Per offset sum V_o / sum n_o over the frames, and VS = sum_o w_o times
    that mean over the offsets that have a pair, w_o = 1 / |o|."""
    frames = np.asarray(frames, np.float64).reshape(-1, len(offsets), 2)
    V, n = frames[:, :, 0].sum(axis=0), frames[:, :, 1].sum(axis=0)
    w = [1.0 / math.hypot(dy, dx) for dy, dx in offsets]
    mean = [_div(a, c) for a, c in zip(V, n)]
    have = [m for m in mean if not math.isnan(m)]
    return {"offsets": [[int(dy), int(dx)] for dy, dx in offsets], "weights": w, "pairs": [int(v) for v in n], "mean": mean,
            "VS": float(sum(wi * m for wi, m in zip(w, mean) if not math.isnan(m))) if have else float("nan")}


def _check_offsets(offsets):
    offsets = tuple((int(dy), int(dx)) for dy, dx in offsets)
    if not 1 <= len(offsets) <= ops.ENS_MAX_OFFSETS or any(o == (0, 0) for o in offsets):
        raise ValueError(f"offsets: 1 to {ops.ENS_MAX_OFFSETS} pairs (dy, dx), none of them (0, 0)")
    return offsets


class EnsembleEvaluator(Streaming):
    """Streaming ensemble scores.  ``update(name, members, truth)`` adds one piece: ``members`` is a sequence of M arrays [T, H, W]
    (each its own H, W and dtype) or one (T, M, H, W) array or tensor, whose members are read in place; device tensors are not
    copied to the host.  Frames pair one for one (the longer side is truncated).  ``crop_size`` is an int or (rows, cols): the
    centre crop of every input.  ``mask`` [rows, cols] with ``mode`` selects the pixels (radar: mask False, gauge: mask True).
    ``box_sizes``: the per-point scores are formed at each (1: pixels).  An ensemble keeps its M over its updates.  ``compute()``
    syncs once and returns ``{name: {"box_<s>": scores, "energy": ..., "variogram": ...}}``."""

    what = "ensemble verification runs"

    def __init__(self, crop_size, mask=None, mode: str = "radar", box_sizes: Sequence[int] = DEFAULT_BOX_SIZES,
                 thresholds: Sequence[float] = DEFAULT_THRESHOLDS, sigma_edges: Sequence[float] = DEFAULT_SIGMA_EDGES,
                 offsets=DEFAULT_OFFSETS, divide_by_3: bool = True, device=None):
        if mode not in ("radar", "gauge"):
            raise ValueError(f"Unknown mode: {mode}")
        self.size = self.rows, self.cols = _crop_shape(crop_size)
        self.box_sizes = tuple(int(s) for s in box_sizes)
        if not self.box_sizes or len(set(self.box_sizes)) != len(self.box_sizes) or \
                any(not 1 <= s <= min(self.rows, self.cols) for s in self.box_sizes):
            raise ValueError(f"box_sizes {self.box_sizes}: distinct sizes in 1 .. {min(self.rows, self.cols)} (the crop)")
        self.thresholds = tuple(float(q) for q in thresholds)
        self.sigma_edges = tuple(float(v) for v in sigma_edges)
        if len(self.thresholds) > ops.EXP1_MAX_THR:
            raise ValueError(f"at most {ops.EXP1_MAX_THR} thresholds")
        if len(self.sigma_edges) > ops.PROB_MAX_EDGES or any(b <= a for a, b in zip(self.sigma_edges, self.sigma_edges[1:])):
            raise ValueError(f"sigma_edges: at most {ops.PROB_MAX_EDGES} ascending edges")
        self.offsets = _check_offsets(offsets)
        self.xq = tuple(pixel_threshold(q, bool(divide_by_3)) for q in self.thresholds)
        self._start(device, divide_by_3, None if mask is None else selection(mask, mode, self.size))
        self._layouts = {}
        for M in (1, ops.ENS_MAX_MEMBERS):
            lay = self.layout(M)
            if ops.ens_record(M, len(self.thresholds), len(self.sigma_edges)) != (lay.nf, lay.ni):
                raise RuntimeError("the record layout of ensemble.py and csrc/eval_ens.hip differ")

    def layout(self, M: int) -> _Layout:
        lay = self._layouts.get(M)
        if lay is None:
            lay = self._layouts[M] = _Layout(M, len(self.thresholds), len(self.sigma_edges))
        return lay

    def _new_state(self):
        """An ensemble's state: its M (set by the first update), one record per box size, the per-frame outputs."""
        return {"M": None, "acc": {}, "energy": [], "variogram": []}

    def _launch_frames(self):
        lay = self.layout(ops.ENS_MAX_MEMBERS)
        return min((_PART_WORDS // (lay.nf + lay.ni)) * ops.ENS_WG_PIXELS // (self.rows * self.cols), _ENERGY_FRAMES // len(self.offsets))

    def _members(self, members):
        """(the members as [T, h, w] device views, their frame stride in elements or 0 for each one's own h * w)"""
        if isinstance(members, (torch.Tensor, np.ndarray)):
            if members.ndim != 4:
                raise ValueError(f"one array of members is (T, M, H, W), got shape {tuple(members.shape)}")
            x = _to_device(members, self.device)
            return [x[:, m] for m in range(x.shape[1])], x.shape[1] * x.shape[2] * x.shape[3]
        views = [_to_device(_thw(a), self.device) for a in members]
        return views, 0

    def update(self, name, members, truth_event):
        rows, cols = self.rows, self.cols
        with torch.cuda.device(self.device):
            truth = _to_device(_thw(truth_event), self.device)
            gtl = crop_origin(truth.shape[1], truth.shape[2], self.size)
            views, stride = self._members(members)
            M = len(views)
            if not 1 <= M <= ops.ENS_MAX_MEMBERS:
                raise ValueError(f"an ensemble has 1 to {ops.ENS_MAX_MEMBERS} members, got {M}")
            if any(v.shape[0] != views[0].shape[0] for v in views):
                raise ValueError("the members differ in their frame counts")
            origins = [crop_origin(v.shape[1], v.shape[2], self.size) for v in views]
            st = self._state(name)
            if st["M"] is None:
                st["M"] = M
                lay = self.layout(M)
                st["acc"] = {s: torch.zeros(lay.nf + lay.ni, device=self.device, dtype=torch.float64) for s in self.box_sizes}
            elif st["M"] != M:
                raise ValueError(f"ensemble {name!r} had {st['M']} members, this piece has {M}")
            lay = self.layout(M)
            nw = lay.nf + lay.ni
            n = min(views[0].shape[0], truth.shape[0])
            for t0, tn in self._cuts(n):
                mv, g = [v[t0:t0 + tn] for v in views], truth[t0:t0 + tn]
                for s in self.box_sizes:
                    nwg = -(-tn * (rows // s) * (cols // s) // ops.ENS_WG_PIXELS)
                    part = torch.empty(nwg * nw, device=self.device, dtype=torch.float64)
                    ops.ens_points(mv, origins, stride, g, gtl, rows, cols, s, self._rank, self.xq, self.sigma_edges, part)
                    ops.prob_merge(part, lay.nf, lay.ni, st["acc"][s])
                e = torch.empty(tn, 4, device=self.device, dtype=torch.float64)
                ops.ens_energy(mv, origins, stride, g, gtl, rows, cols, self._rank, e)
                v = torch.empty(tn, len(self.offsets), 2, device=self.device, dtype=torch.float64)
                ops.ens_variogram(mv, origins, stride, g, gtl, rows, cols, self._rank, self.offsets, v)
                st["energy"].append(e)
                st["variogram"].append(v)

    def raw(self, name, box: int = 1) -> torch.Tensor:
        """The ensemble's accumulator at one box size on the device: nf fp64 words, then ni int64 words as their bits."""
        return self._methods[name]["acc"][box]

    def _host(self, names):
        """Every state of ``names`` on the host through ONE copy: {name: ({box: record}, energy [n, 4], variogram [n, nof, 2])}."""
        flat, plan = [], []
        for k in names:
            st = self._methods[k]
            ts = [st["acc"][s] for s in self.box_sizes] + [t.reshape(-1) for t in st["energy"]] + [t.reshape(-1) for t in st["variogram"]]
            plan.append((k, sum(t.shape[0] for t in st["energy"])))
            flat += ts
        with torch.cuda.device(self.device):
            host = torch.cat(flat).cpu().numpy()         # the one host sync
        out, at = {}, 0
        for k, nfr in plan:
            lay = self.layout(self._methods[k]["M"])
            nw, nof = lay.nf + lay.ni, len(self.offsets)
            recs = {}
            for s in self.box_sizes:
                recs[s] = host[at:at + nw]
                at += nw
            en = host[at:at + nfr * 4].reshape(nfr, 4)
            at += nfr * 4
            va = host[at:at + nfr * nof * 2].reshape(nfr, nof, 2)
            at += nfr * nof * 2
            out[k] = (recs, en, va)
        return out

    def sums(self, name) -> Dict[str, object]:
        """The ensemble's sums so far ({"box_<s>": named sums, "energy": [n, 4], "variogram": [n, nof, 2]}); syncs.  For checks."""
        recs, en, va = self._host([name])[name]
        lay = self.layout(self._methods[name]["M"])
        res = {f"box_{s}": unpack_record(r[:lay.nf], np.ascontiguousarray(r[lay.nf:]).view(np.int64), lay) for s, r in recs.items()}
        res["energy"], res["variogram"] = en, va
        return res

    def compute(self) -> Dict[object, Dict[str, object]]:
        names = [k for k, st in self._methods.items() if st["M"] is not None]
        if not names:
            return {}
        res = {}
        for k, (recs, en, va) in self._host(names).items():
            M = self._methods[k]["M"]
            lay = self.layout(M)
            r = {f"box_{s}": ens_scores(unpack_record(rec[:lay.nf], np.ascontiguousarray(rec[lay.nf:]).view(np.int64), lay), M,
                                        self.thresholds, self.sigma_edges) for s, rec in recs.items()}
            r["energy"] = energy_scores(en)
            r["variogram"] = variogram_scores(va, self.offsets)
            res[k] = r
        return res


def run_ensemble(ensembles, truth, mask=None, mode: str = "radar", crop_size=None, box_sizes: Sequence[int] = DEFAULT_BOX_SIZES,
                 thresholds: Sequence[float] = DEFAULT_THRESHOLDS, sigma_edges: Sequence[float] = DEFAULT_SIGMA_EDGES,
                 offsets=DEFAULT_OFFSETS, divide_by_3: bool = True, device=None) -> Dict[str, Dict[str, object]]:
    """Every ensemble of ``ensembles`` ({name: members}) scored against ``truth``.  ``members`` is what ``EnsembleEvaluator.update``
    takes.  With a dict ``truth`` ({event: array}, None-valued events dropped) every ensemble is a dict of the same keys (TypeError
    otherwise; an event an ensemble lacks is skipped for it) and event k's members are scored against event k's truth; otherwise the
    truth and every ensemble are one event, and a dict ensemble is a TypeError.  Returns ``{name: {"box_<s>": scores, "energy": ...,
    "variogram": ...}}``."""
    if crop_size is None:
        raise ValueError("crop_size is required")
    ev = EnsembleEvaluator(crop_size, mask=mask, mode=mode, box_sizes=box_sizes, thresholds=thresholds, sigma_edges=sigma_edges,
                           offsets=offsets, divide_by_3=divide_by_3, device=device)
    if isinstance(truth, dict):
        keys = [k for k in truth if truth.get(k) is not None]
        for name, src in ensembles.items():
            if not isinstance(src, dict):
                raise TypeError(f"ensemble {name!r}: a per-event truth needs per-event members")
        for name, src in ensembles.items():
            for k in keys:
                if src.get(k) is not None:
                    ev.update(name, src[k], truth[k])
    else:
        for name, src in ensembles.items():
            if isinstance(src, dict):
                raise TypeError(f"ensemble {name!r}: per-event members need a per-event truth")
            ev.update(name, src, truth)
    return ev.compute()


def _boxes(m):
    return sorted((int(k[4:]), v) for k, v in m.items() if k.startswith("box_"))


def ens_lines(result) -> List[str]:
    """metrics.txt: per ensemble and box size ``CRPS_<name>_box<s>``, ``CRPSFAIR``, ``RMSE``, ``SSR`` (spread-skill ratio), ``OUTLIER``,
    ``RELIDX`` and per threshold ``BRIER`` / ``BSS`` / ``ROC``; then ``ES_<name>``, ``ESFAIR_<name>``, ``VS_<name>``; 6 decimals."""
    lines = []
    for name, m in result.items():
        for s, b in _boxes(m):
            label = f"{name}_box{s}"
            for key, tag in (("CRPS", "CRPS"), ("CRPS_fair", "CRPSFAIR"), ("RMSE", "RMSE"), ("spread_skill_ratio", "SSR"),
                             ("outlier_share", "OUTLIER"), ("reliability_index", "RELIDX")):
                lines.append(f"{tag}_{label}: {b[key]:.6f}")
            for tk, e in b["exceedance"].items():
                t = tk.replace("_", "")
                lines.append(f"BRIER_{label}_{t}: {e['brier']:.6f}")
                lines.append(f"BSS_{label}_{t}: {e['bss']:.6f}")
                lines.append(f"ROC_{label}_{t}: {e['roc_area']:.6f}")
            lines.append(f"NSKIPPED_{label}: {b['n_skipped']}")
        lines.append(f"ES_{name}: {m['energy']['ES_norm']:.6f}")
        lines.append(f"ESFAIR_{name}: {m['energy']['ES_fair_norm']:.6f}")
        lines.append(f"VS_{name}: {m['variogram']['VS']:.6f}")
    return lines


def ens_arrays(result) -> Dict[str, np.ndarray]:
    """ens_data.npz: per ensemble and box size the rank histogram, the spread-skill and reliability tables and the scalar scores;
    per ensemble the per-frame energy series and the per-offset variogram means."""
    arrays = {"ensembles": np.array(list(result))}
    for name, m in result.items():
        arrays[f"{name}/box_sizes"] = np.array([s for s, _ in _boxes(m)], dtype=np.int64)
        for s, b in _boxes(m):
            label = f"{name}/box_{s}"
            arrays[f"{label}/rank_histogram"] = np.asarray(b["rank_histogram"], dtype=np.float64)
            for k in ("edges", "count", "spread", "rmse"):
                arrays[f"{label}/spread_skill_{k}"] = np.asarray(b["spread_skill"][k], dtype=np.float64)
            thr = list(b["exceedance"])
            arrays[f"{label}/thresholds"] = np.array([float(tk[4:]) for tk in thr])
            for k in ("count", "obs_freq"):
                arrays[f"{label}/reliability_{k}"] = np.array([b["exceedance"][tk]["reliability"][k] for tk in thr],
                                                              dtype=np.float64).reshape(len(thr), -1)
            arrays[f"{label}/exceedance"] = np.array([[b["exceedance"][tk][k] for k in ("base_rate", "mean_p", "brier", "bss", "roc_area")]
                                                      for tk in thr], dtype=np.float64).reshape(len(thr), 5)
            arrays[f"{label}/scores"] = np.array([b[k] for k in ("CRPS", "CRPS_fair", "ME", "MAE", "RMSE", "mean_var", "spread_skill_ratio",
                                                                 "outlier_share", "reliability_index", "n", "n_skipped", "M")],
                                                 dtype=np.float64)
        for k in ("d", "ES", "ES_fair", "dist_truth"):
            arrays[f"{name}/energy_{k}"] = np.asarray(m["energy"]["frames"][k], dtype=np.float64)
        arrays[f"{name}/energy"] = np.array([m["energy"]["ES_norm"], m["energy"]["ES_fair_norm"]], dtype=np.float64)
        arrays[f"{name}/variogram_offsets"] = np.asarray(m["variogram"]["offsets"], dtype=np.int64).reshape(-1, 2)
        for k in ("mean", "weights", "pairs"):
            arrays[f"{name}/variogram_{k}"] = np.asarray(m["variogram"][k], dtype=np.float64)
        arrays[f"{name}/VS"] = np.array(m["variogram"]["VS"], dtype=np.float64)
    return arrays


def write_ens_figure(result, path: str) -> Optional[str]:
    """Four panels: rank histograms (box size 1 or the smallest), reliability diagrams (the first threshold), spread against skill,
    CRPS against box size (matplotlib, no display needed).  Without matplotlib it warns and writes nothing."""
    try:
        from matplotlib.figure import Figure
    except ImportError:
        warnings.warn("matplotlib is not importable: the ensemble figure is skipped (the numbers are in ens_data.npz)")
        return None
    fig = Figure(figsize=(16, 3.6), dpi=200)
    ax_rank, ax_rel, ax_ss, ax_crps = fig.subplots(1, 4)
    lim = []
    for name, m in result.items():
        boxes = _boxes(m)
        s0, b = boxes[0]
        M = b["M"]
        ax_rank.step(np.arange(M + 1), np.asarray(b["rank_histogram"]) * (M + 1), where="mid", label=f"{name} (M={M})")
        if b["exceedance"]:
            tk = next(iter(b["exceedance"]))
            ax_rel.plot(np.arange(M + 1) / M, b["exceedance"][tk]["reliability"]["obs_freq"], marker="o", markersize=3, label=name)
            ax_rel.set_title(f"reliability, >= {tk[4:]} mm/h", fontsize=10)
        ax_ss.loglog(b["spread_skill"]["spread"], b["spread_skill"]["rmse"], marker="o", markersize=3, label=name)
        lim += [v for k in ("spread", "rmse") for v in b["spread_skill"][k] if np.isfinite(v) and v > 0]
        ax_crps.plot([s for s, _ in boxes], [x["CRPS"] for _, x in boxes], marker="o", markersize=3, label=f"{name} CRPS")
        if M > 1:
            ax_crps.plot([s for s, _ in boxes], [x["CRPS_fair"] for _, x in boxes], marker="s", markersize=3, linestyle="--",
                         label=f"{name} fair")
    ax_rank.axhline(1.0, color="k", linewidth=0.8)
    ax_rank.set_xlabel("rank of the truth")
    ax_rank.set_ylabel("relative frequency x (M + 1)")
    ax_rank.set_title("rank histogram", fontsize=10)
    ax_rel.plot([0, 1], [0, 1], color="k", linewidth=0.8)
    ax_rel.set_xlabel("share of members above the threshold")
    ax_rel.set_ylabel("observed frequency")
    if lim:
        ax_ss.plot([min(lim), max(lim)], [min(lim), max(lim)], color="k", linewidth=0.8)
    ax_ss.set_xlabel("RMS spread per sigma-bin")
    ax_ss.set_ylabel("RMSE of the mean per sigma-bin")
    ax_ss.set_title("spread - skill", fontsize=10)
    ax_crps.set_xscale("log", base=2)
    ax_crps.set_xlabel("box size (pixels)")
    ax_crps.set_ylabel("CRPS (0-255 scale)")
    ax_crps.set_title("CRPS of box means", fontsize=10)
    if result:
        ax_rank.legend(frameon=True, fontsize=7)
        ax_crps.legend(frameon=True, fontsize=7)
    fig.tight_layout()
    fig.savefig(path, format="pdf", bbox_inches="tight")
    return path


def write_ens_outputs(out_dir: str, result, stem: str = "metrics", figure: bool = True) -> None:
    """DIR/<stem>.json (indent 2, sorted keys), DIR/<stem>.txt (``ens_lines``), DIR/ens_data.npz and DIR/ens_panels.pdf."""
    import json
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{stem}.json"), "w", encoding="utf-8") as f:
        json.dump(result, f, indent=2, sort_keys=True)
    with open(os.path.join(out_dir, f"{stem}.txt"), "w", encoding="utf-8") as f:
        for line in ens_lines(result):
            f.write(line + "\n")
    np.savez(os.path.join(out_dir, "ens_data.npz"), **ens_arrays(result))
    if figure:
        write_ens_figure(result, os.path.join(out_dir, "ens_panels.pdf"))
