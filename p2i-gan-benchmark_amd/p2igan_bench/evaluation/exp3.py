"""exp3 analysis (reference experiments/exp3.py ``run_exp3``: NSE, per-event NSE, scatter / residual samples and fits, log-frequency
histograms) on csrc/eval_exp3.hip: ``Exp3Evaluator``, ``compute_exp3``, ``run_exp3``, the stored ``Exp3Result`` and the reference's
four figures of it (matplotlib, imported only when a figure is drawn).  DESIGN.md section 11 lists the rules."""
from __future__ import annotations

import json
import os
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from ._common import NO_EVENTS, _pieces, _thw, _to_device, crop_origin, device_tables, eval_device, selection

EXP3_MAX_POINTS = 2000      # the scatter / residual panels' sample size
EXP3_SEED = 42              # np.random.default_rng(42), once per figure, advanced across methods
EXP3_MIN_VALUE = 0.1        # the pool keeps observations >= 0.1 mm/h
LOGFREQ_EDGES = np.linspace(0.0, 32.0, ops.EXP3_BINS + 1)


def linregress(x, y) -> Tuple[float, float, float]:
    """(slope, intercept, r) of scipy.stats.linregress, restated in numpy: the biased moments of np.cov(x, y, bias=1), r = 0 when a
    variance is 0 and clamped to [-1, 1] otherwise.  Raises ValueError where scipy does (empty input, all x identical)."""
    x, y = np.asarray(x), np.asarray(y)
    if x.size == 0 or y.size == 0:
        raise ValueError("Inputs must not be empty.")
    if np.amax(x) == np.amin(x) and len(x) > 1:
        raise ValueError("Cannot calculate a linear regression if all x values are identical")
    xmean, ymean = np.mean(x, None), np.mean(y, None)
    ssxm, ssxym, _, ssym = np.cov(x, y, bias=1).flat
    if ssxm == 0.0 or ssym == 0.0:
        r = 0.0
    else:
        r = ssxym / np.sqrt(ssxm * ssym)
        r = 1.0 if r > 1.0 else (-1.0 if r < -1.0 else r)
    slope = ssxym / ssxm
    return float(slope), float(ymean - slope * xmean), float(r)


@dataclass
class Exp3Result:
    """The numbers of run_exp3 and its figures.  ``per_event``: dict input (the boxplot and log-frequency figures exist);
    ``has_scatter``: the truth stack holds a finite value (the scatter and residual figures exist).  Per method: ``pool`` (points
    before sampling), the sampled ``x`` (observed), ``y_scatter`` (predicted) and ``y_residual`` (predicted - observed), and the
    fits ``fit_scatter`` / ``fit_residual`` = (slope, intercept, r), NaN with fewer than 2 points.  ``freq_truth`` / ``freq``: the
    log-frequency curves over ``logfreq_edges`` (per_event only; a method without a finite value has no curve)."""
    methods: List[str]
    metrics: Dict[str, float]
    nse_by_method: Dict[str, List[float]] = field(default_factory=dict)
    per_event: bool = True
    has_scatter: bool = True
    pool: Dict[str, int] = field(default_factory=dict)
    x: Dict[str, np.ndarray] = field(default_factory=dict)
    y_scatter: Dict[str, np.ndarray] = field(default_factory=dict)
    y_residual: Dict[str, np.ndarray] = field(default_factory=dict)
    fit_scatter: Dict[str, Tuple[float, float, float]] = field(default_factory=dict)
    fit_residual: Dict[str, Tuple[float, float, float]] = field(default_factory=dict)
    logfreq_edges: Optional[np.ndarray] = None
    freq_truth: Optional[np.ndarray] = None
    freq: Dict[str, np.ndarray] = field(default_factory=dict)

    def save(self, path: str) -> None:
        """One .npz: a JSON header (methods, metrics, per-event NSE, pools, fits, flags) and the arrays under x/, y_scatter/,
        y_residual/, freq/ plus logfreq_edges and freq_truth."""
        head = {"methods": self.methods, "metrics": self.metrics, "nse_by_method": self.nse_by_method, "per_event": self.per_event,
                "has_scatter": self.has_scatter, "pool": self.pool, "fit_scatter": self.fit_scatter, "fit_residual": self.fit_residual,
                "freq_methods": list(self.freq)}
        arrays = {"header": np.array(json.dumps(head))}
        for i, name in enumerate(self.methods):
            for key, d in (("x", self.x), ("y_scatter", self.y_scatter), ("y_residual", self.y_residual), ("freq", self.freq)):
                if name in d:
                    arrays[f"{key}/{i}"] = np.asarray(d[name])
        if self.logfreq_edges is not None:
            arrays["logfreq_edges"] = self.logfreq_edges
            arrays["freq_truth"] = self.freq_truth
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path: str) -> "Exp3Result":
        with np.load(path) as z:
            head = json.loads(str(z["header"]))
            r = cls(methods=head["methods"], metrics=head["metrics"], nse_by_method=head["nse_by_method"], per_event=head["per_event"],
                    has_scatter=head["has_scatter"], pool={k: int(v) for k, v in head["pool"].items()},
                    fit_scatter={k: tuple(v) for k, v in head["fit_scatter"].items()},
                    fit_residual={k: tuple(v) for k, v in head["fit_residual"].items()})
            for i, name in enumerate(r.methods):
                for key in ("x", "y_scatter", "y_residual", "freq"):
                    if f"{key}/{i}" in z.files:
                        getattr(r, key)[name] = z[f"{key}/{i}"]
            if "logfreq_edges" in z.files:
                r.logfreq_edges, r.freq_truth = z["logfreq_edges"], z["freq_truth"]
        return r


class _Exp3Method:
    def __init__(self):
        self.pieces = []         # (pred [n, H, W] on the device, crop origin), in event order
        self.full = True         # every truth event present at its full length: the stack pairs are the event pairs
        self.rec, self.rows = [], []
        self.hist = None


class Exp3Evaluator:
    """Streaming exp3 numbers.  ``methods`` fixes the order the reference walks ``preds`` in (the sampling rng advances across it).
    ``add_event(truth_event, {method: pred_event})`` adds one truth event and the methods' predictions for it; with ``per_event``
    (the reference's dict path) a prediction is truncated to the truth's length, and that truncation carries over to the methods
    after it for this event, as in the reference.  Without ``per_event`` (its array path) the pieces are stacked as given and only
    the stack is scored.  ``mask`` is the crop_size x crop_size mask.  ``compute()`` syncs twice (the pool sizes, which the host's
    sampler needs, then the results) and returns an ``Exp3Result``."""

    def __init__(self, mask, mode: str, crop_size: int, methods: Sequence[str], per_event: bool = True, divide_by_3: bool = True,
                 max_points: int = EXP3_MAX_POINTS, seed: int = EXP3_SEED, device=None):
        self.device = eval_device(device, "exp3 analysis runs")
        self.size = int(crop_size)
        self.mode, self.divide_by_3, self.per_event = mode, bool(divide_by_3), bool(per_event)
        self.max_points, self.seed = int(max_points), int(seed)
        self.methods = list(methods)
        if len(set(self.methods)) != len(self.methods):
            raise ValueError(f"method names repeat: {self.methods}")
        self._lut, self._rank = device_tables(self.device, self.divide_by_3, selection(mask, mode, self.size))
        self.reset()

    def reset(self):
        self._truth = []
        self._thist = torch.zeros(ops.EXP3_NHIST, device=self.device, dtype=torch.int64)
        self._m = {}
        for name in self.methods:
            st = self._m[name] = _Exp3Method()
            st.hist = torch.zeros(ops.EXP3_NHIST, device=self.device, dtype=torch.int64)

    def add_event(self, truth_event, preds: Dict[str, object]):
        unknown = [n for n in preds if n not in self._m]
        if unknown:
            raise ValueError(f"unknown method {unknown[0]!r} (methods: {self.methods})")
        S = self.size
        with torch.cuda.device(self.device):
            truth = _to_device(_thw(truth_event), self.device)
            gtl = crop_origin(truth.shape[1], truth.shape[2], S)
            self._truth.append((truth, gtl))
            if truth.shape[0]:
                ops.exp3_truth_hist(truth, gtl, S, self._lut, self.divide_by_3, self._thist)
            n_truth = truth.shape[0]
            for name in self.methods:
                st, src = self._m[name], preds.get(name)
                if src is None:
                    st.full = False
                    continue
                pred = _to_device(_thw(src), self.device)
                if self.per_event:
                    n = min(pred.shape[0], n_truth)
                    pred = pred[:n]
                ptl = crop_origin(pred.shape[1], pred.shape[2], S)
                st.pieces.append((pred, ptl))
                if not self.per_event:
                    continue
                st.full = st.full and n == truth.shape[0]
                rec = torch.empty(n, ops.EXP3_NREC, device=self.device, dtype=torch.float64)
                rows = torch.empty(n, S, device=self.device, dtype=torch.int32)
                if n:
                    ops.exp3_accumulate(pred, truth[:n], ptl, gtl, S, self._rank, self._lut, self.divide_by_3, rec, rows, st.hist)
                st.rec.append(rec)
                st.rows.append(rows)
                n_truth = n                 # the reference's `truth_ev = truth_aligned`

    def _stack_pairs(self, st):
        """(pred piece, origin, truth piece, origin) of stack[k] <-> truth_stack[k], in stack order (align_length of the stacks)."""
        pp, tt = [p for p, _ in st.pieces], [t for t, _ in self._truth]
        # the pieces of _pieces are slices along T: each keeps its source's H, W and so its crop origin
        return [(p, crop_origin(p.shape[1], p.shape[2], self.size), t, crop_origin(t.shape[1], t.shape[2], self.size))
                for p, t in _pieces(pp, tt)]

    def compute(self) -> Exp3Result:
        if not self._truth:
            raise ValueError(NO_EVENTS)
        if not self.methods:
            raise ValueError("Number of columns must be a positive integer, not 0")     # the reference's empty figure row
        S, dev = self.size, self.device
        with torch.cuda.device(dev):
            per = []
            for name in self.methods:
                st = self._m[name]
                if not st.pieces:
                    raise ValueError(NO_EVENTS)
                if self.per_event and st.full:
                    pairs = [(p, po, t, to) for (p, po), (t, to) in zip(st.pieces, self._truth)]
                    srec = torch.cat(st.rec)
                    rows = torch.cat(st.rows)
                else:
                    pairs = self._stack_pairs(st)
                    recs, rws = [], []
                    for p, po, t, to in pairs:
                        recs.append(torch.empty(p.shape[0], ops.EXP3_NREC, device=dev, dtype=torch.float64))
                        rws.append(torch.empty(p.shape[0], S, device=dev, dtype=torch.int32))
                        ops.exp3_accumulate(p, t, po, to, S, self._rank, self._lut, self.divide_by_3, recs[-1], rws[-1])
                    srec = torch.cat(recs) if recs else torch.empty(0, ops.EXP3_NREC, device=dev, dtype=torch.float64)
                    rows = torch.cat(rws) if rws else torch.empty(0, S, device=dev, dtype=torch.int32)
                if self.per_event:
                    off = np.concatenate([[0], np.cumsum([r.shape[0] for r in st.rec])]).astype(np.int32)
                    erec = torch.cat(st.rec) if st.rec else srec
                    nse = ops.exp3_nse(erec, torch.from_numpy(off).to(dev), srec)
                else:
                    nse = ops.exp3_nse(None, None, srec)
                prefix = ops.exp3_scan(rows.reshape(-1))
                per.append((st, pairs, nse, prefix))
            last = [pf[-1:] if pf.numel() else torch.zeros(1, device=dev, dtype=torch.int64) for _, _, _, pf in per]
            sizes = torch.cat(last + [self._thist[ops.EXP3_BINS:]]).cpu().numpy()      # host sync 1: the pool sizes
            has_scatter = bool(sizes[-1] > 0)
            rng = np.random.default_rng(self.seed)
            gathered = []
            for (st, pairs, nse, prefix), n in zip(per, sizes[:-1]):
                n = int(n)
                if not has_scatter:
                    ords = np.empty(0, np.int64)
                elif n > self.max_points:
                    ords = rng.choice(n, size=self.max_points, replace=False).astype(np.int64)
                else:
                    ords = np.arange(n, dtype=np.int64)
                K = ords.size
                og = torch.empty(K, device=dev, dtype=torch.float64)
                op = torch.empty(K, device=dev, dtype=torch.float64)
                if K:
                    od = torch.from_numpy(ords).to(dev)
                    row0 = 0
                    for p, po, t, to in pairs:
                        ops.exp3_gather(p, t, po, to, S, self._lut, self.divide_by_3, prefix, row0, od, og, op)
                        row0 += p.shape[0] * S
                gathered.append((n, K, og, op))
            parts = [nse for _, _, nse, _ in per] + [g for _, _, g, _ in gathered] + [p for _, _, _, p in gathered]
            parts += [self._m[n].hist.double() for n in self.methods] + [self._thist.double()]
            host = torch.cat(parts).cpu().numpy()                                            # host sync 2: the results
        return self._result(host, [g[:2] for g in gathered], has_scatter)

    def _result(self, host, counts, has_scatter) -> Exp3Result:
        names, i = self.methods, 0
        res = Exp3Result(methods=list(names), metrics={}, per_event=self.per_event, has_scatter=has_scatter)
        for name in names:
            E = len(self._m[name].rec) if self.per_event else 0
            res.metrics[f"NSE_{name}"] = float(host[i])
            if self.per_event:
                res.nse_by_method[name] = [float(v) for v in host[i + 1:i + 1 + E]]
            i += 1 + E
        xs = []
        for _, K in counts:
            xs.append(host[i:i + K])
            i += K
        for name, (n, K), x in zip(names, counts, xs):
            y = host[i:i + K].copy()
            i += K
            x = x.copy()
            res.pool[name] = n
            if not has_scatter:
                continue
            res.x[name], res.y_scatter[name], res.y_residual[name] = x, y, y - x
            nan3 = (float("nan"),) * 3
            res.fit_scatter[name] = linregress(x, y) if K >= 2 else nan3
            res.fit_residual[name] = linregress(x, y - x) if K >= 2 else nan3
        hists = []
        for _ in range(len(names) + 1):
            hists.append(host[i:i + ops.EXP3_NHIST].astype(np.int64))
            i += ops.EXP3_NHIST
        if self.per_event and hists[-1][ops.EXP3_BINS] > 0:
            res.logfreq_edges = LOGFREQ_EDGES.copy()
            h = hists[-1][:ops.EXP3_BINS]
            res.freq_truth = h / max(h.sum(), 1)
            for name, hp in zip(names, hists[:-1]):
                if hp[ops.EXP3_BINS] > 0:                 # the reference skips a method without a finite value
                    h = hp[:ops.EXP3_BINS]
                    res.freq[name] = h / max(h.sum(), 1)
        return res


def compute_exp3(preds, truth, mask, mode: str, crop_size: int, divide_by_3: bool = True, device=None) -> Exp3Result:
    """The numbers of the reference's run_exp3 (experiments/exp3.py) on the device, without writing anything.  With a dict ``truth``
    the events are taken in its key order and every method must be a dict (an event it lacks is skipped for it); otherwise
    ``truth`` and every method are whole arrays."""
    if isinstance(truth, dict):
        names = list(preds.keys())
        if any(not isinstance(src, dict) for src in preds.values()):
            raise ValueError(NO_EVENTS)              # the reference stacks nothing for it, then fails on the empty stack
        ev = Exp3Evaluator(mask, mode, crop_size, names, per_event=True, divide_by_3=divide_by_3, device=device)
        for k in truth.keys():
            if truth.get(k) is None:
                continue
            ev.add_event(truth[k], {n: preds[n].get(k) for n in names if preds[n].get(k) is not None})
    else:
        for name, src in preds.items():
            if isinstance(src, dict):
                raise TypeError("float() argument must be a string or a real number, not 'dict'")
        ev = Exp3Evaluator(mask, mode, crop_size, list(preds.keys()), per_event=False, divide_by_3=divide_by_3, device=device)
        ev.add_event(truth, dict(preds))
    return ev.compute()


def run_exp3(preds, truth, mask, mode: str, crop_size: int, out_dir: str, device=None) -> Dict[str, float]:
    """The reference's run_exp3: returns {"NSE_<name>": float}; writes out_dir/exp3_data.npz (Exp3Result.save) and the figures
    (write_exp3_figures)."""
    os.makedirs(out_dir, exist_ok=True)
    res = compute_exp3(preds, truth, mask, mode, crop_size, device=device)
    res.save(os.path.join(out_dir, "exp3_data.npz"))
    write_exp3_figures(res, out_dir)
    return dict(res.metrics)


SCATTER_COLORS = ('#1f77b4', '#ff7f0e', '#2ca02c', '#d62728', '#9467bd', '#8c564b')
_TICKS32 = (0, 4, 8, 12, 16, 20, 24, 28, 32)


def _panels(res: Exp3Result, path: str, residual: bool):
    from matplotlib.figure import Figure
    fig = Figure(figsize=(18, 3), dpi=600)
    axes = fig.subplots(1, len(res.methods), squeeze=False)[0]
    line = np.linspace(0, 32, 200)
    for i, name in enumerate(res.methods):
        ax = axes[i]
        x = res.x[name]
        y = res.y_residual[name] if residual else res.y_scatter[name]
        ax.scatter(x, y, s=10, alpha=0.6, color=SCATTER_COLORS[i % len(SCATTER_COLORS)], edgecolors='none', rasterized=False, zorder=1)
        if x.size >= 2:
            slope, intercept, r = (res.fit_residual if residual else res.fit_scatter)[name]
            ax.plot(line, np.zeros_like(line) if residual else line, color='gray', ls=':', lw=1.0)
            ax.plot(line, intercept + slope * line, 'k--', lw=1.0)
            ax.text(0.04, 0.82, f"R²={r ** 2:.3f}\nslope={slope:.3f}", transform=ax.transAxes, fontsize=11)
        ax.set_title(name, fontsize=13, fontweight='bold', pad=4)
        ax.set_xlim(0, 32)
        if residual:
            ax.set_ylim(-24, 8)
        else:
            ax.set_ylim(0, 32)
            ax.set_aspect('equal', 'box')
        ax.set_xticks(_TICKS32)
        ax.set_yticks((-24, -20, -16, -12, -8, -4, 0, 4, 8) if residual else _TICKS32)
        ax.tick_params(axis='both', labelsize=10, width=1.0, length=3)
        ax.grid(False)
        if residual:
            ax.axhline(0, color='black', lw=1.0, ls='--')
        if i == 0:
            ax.set_ylabel("Residual (Pred - Obs, mm/h)" if residual else "Pred (mm/h)", fontsize=12)
        ax.set_xlabel("Obs (mm/h)", fontsize=12)
    fig.tight_layout(pad=1.0)
    fig.savefig(path, bbox_inches='tight')


def _boxplot(res: Exp3Result, path: str):
    from matplotlib.figure import Figure
    data = [res.nse_by_method[m] for m in res.methods]
    fig = Figure(figsize=(6, 4), dpi=300)
    ax = fig.subplots()
    box = ax.boxplot(data, tick_labels=res.methods, patch_artist=True, showmeans=True, meanline=False,
                     boxprops=dict(linewidth=1.2, color='black'), medianprops=dict(linewidth=2.0, color='black'),
                     whiskerprops=dict(linewidth=1.2, color='black'), capprops=dict(linewidth=1.2, color='black'),
                     flierprops=dict(marker='o', markersize=3, alpha=0.5, color='gray'),
                     meanprops=dict(marker='D', markerfacecolor='white', markeredgecolor='black', markersize=5))
    for patch, color in zip(box['boxes'], SCATTER_COLORS):
        patch.set_facecolor(color)
        patch.set_alpha(0.7)
    ax.set_ylabel('NSE', fontsize=14)
    ax.set_xlabel('Methods', fontsize=13)
    ax.set_title(f'NSE Comparison ({len(data[0])} Rain Events)', fontsize=14, fontweight='bold')
    ax.set_ylim(-0.2, 1.0)
    ax.grid(False)
    ax.tick_params(axis='both', labelsize=11)
    fig.tight_layout()
    fig.savefig(path, format='pdf', bbox_inches='tight')


def _logfreq(res: Exp3Result, path: str):
    from matplotlib.figure import Figure
    fig = Figure(figsize=(6, 4), dpi=300)
    ax = fig.subplots()
    left = res.logfreq_edges[:-1]
    ax.semilogy(left, res.freq_truth, color='black', lw=1.6, label='Obs')
    for name, color in zip(res.methods, SCATTER_COLORS):
        if name in res.freq:
            ax.semilogy(left, res.freq[name], color=color, lw=1.6, label=name)
    ax.set_xlim(0, 32)
    ax.set_xlabel("Rainfall (mm/h)")
    ax.set_ylabel("Relative Frequency (log scale)")
    ax.grid(False)
    ax.legend(frameon=True, fontsize=9)
    fig.tight_layout()
    fig.savefig(path, bbox_inches="tight")


def write_exp3_figures(res: Exp3Result, out_dir: str) -> List[str]:
    """The reference's figures of an Exp3Result (matplotlib, no display needed): scatter_panels.pdf and residual_panels.pdf when the
    truth has a finite value, nse_boxplot.pdf and logfreq.pdf for per-event input.  Without matplotlib it warns once and writes
    nothing.  Returns the paths written."""
    try:
        import matplotlib.figure  # noqa: F401
    except ImportError:
        warnings.warn("matplotlib is not importable: the exp3 figures are skipped (the numbers are in exp3_data.npz)")
        return []
    os.makedirs(out_dir, exist_ok=True)
    written = []
    if res.has_scatter and res.methods:
        for fname, residual in (("scatter_panels.pdf", False), ("residual_panels.pdf", True)):
            _panels(res, os.path.join(out_dir, fname), residual)
            written.append(os.path.join(out_dir, fname))
    if res.per_event and res.nse_by_method:
        _boxplot(res, os.path.join(out_dir, "nse_boxplot.pdf"))
        written.append(os.path.join(out_dir, "nse_boxplot.pdf"))
        if res.freq_truth is not None:
            _logfreq(res, os.path.join(out_dir, "logfreq.pdf"))
            written.append(os.path.join(out_dir, "logfreq.pdf"))
    return written
