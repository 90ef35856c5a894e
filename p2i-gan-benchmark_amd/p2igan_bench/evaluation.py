"""The benchmark's exp1 scoring of inference outputs (reference experiments/exp1.py ``run_exp1`` with experiments/io.py), with the
arithmetic on the device (csrc/eval_exp1.hip), and its exp3 analysis (experiments/exp3.py ``run_exp3``: NSE, per-event NSE,
scatter / residual samples and fits, log-frequency histograms) on csrc/eval_exp3.hip.

``run_exp1`` takes the reference's arguments and returns its table: per method MAE, RMSE, PSS, SSIM, DTSSIM_L1, DTSSIM_L2, NSE and
``CAT_<thr:g>`` = {POD, FAR, CSI, HSS}.  Inputs may be numpy arrays, torch tensors (CPU or device) or dicts of per-event arrays
(``[T, H, W]``, ``[T, 1, H, W]``, ``[T, H, W, 1]`` or ``[1, T, H, W]``, on the 0-255 scale).  ``Exp1Evaluator`` is the streaming form
it is built on: one ``update`` per aligned piece, one host sync in ``compute``.  The rules it reproduces, the reference's quirks
included, are listed in DESIGN.md section 10.  There is no CPU path: without a GPU the evaluator raises RuntimeError.

``run_exp3`` takes the reference's arguments, returns ``{"NSE_<name>": float}`` and writes the reference's four figures plus
``exp3_data.npz`` (the numbers behind them).  ``Exp3Evaluator`` is its streaming form (one ``add_event`` per truth event, two host
syncs in ``compute``); DESIGN.md section 11 lists its rules.

``run_exp2`` takes the reference's arguments (experiments/exp2.py) and writes its comparison GIFs and ``event_ranges.txt`` plus
``exp2_data.npz``; the frames are canvases of palette indices built on csrc/eval_exp2.hip (``compute_exp2``, ``exp2_canvases``).
``run_exp2_paper_zarr`` writes the paper's frame grid.  DESIGN.md section 12 lists the rules.
"""
from __future__ import annotations

import json
import os
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

DEFAULT_THRESHOLDS = (0.5, 2.0, 4.0, 8.0)
PSS_BINS = 50
PSS_MIN_VALUE = 0.5
_METRICS = ("MAE", "RMSE", "PSS", "SSIM", "DTSSIM_L1", "DTSSIM_L2", "NSE")
_CATS = ("POD", "FAR", "CSI", "HSS")
_MAX_FRAMES = 65535          # frames per accumulate launch (grid.y)


def transform_mmhr(arr, divide_by_3: bool = True) -> np.ndarray:
    """The reference's rain-rate transform in float64 (exp1.py transform_mmhr): max(x, 0.001) [/3], then
    10 ** min(x * 0.0625, 38) * 0.036, clipped to [0, 200].  NaN stays NaN (np.maximum propagates it)."""
    arr = np.asarray(arr, dtype=np.float64)
    arr = np.maximum(arr, 0.001)
    if divide_by_3:
        arr = arr / 3.0
    out = 10 ** np.clip(arr * 0.0625, a_min=None, a_max=38.0) * 0.036
    return np.clip(out, 0.0, 200.0)


def truth_lut(divide_by_3: bool = True) -> np.ndarray:
    """transform_mmhr of the 256 uint8 values, computed by numpy on the host: the device looks uint8 inputs up here."""
    return transform_mmhr(np.arange(256, dtype=np.uint8), divide_by_3)


def pss_edges(vmin: float, vmax: float, bins: int = PSS_BINS) -> np.ndarray:
    """np.histogram's float32 bin edges for float32 data over (vmin, vmax), with exp1's ``vmin == vmax -> vmax + 1e-6`` rule.
    Raises ValueError, as np.histogram does, when the edges are not strictly increasing."""
    vmin, vmax = float(vmin), float(vmax)
    if vmin == vmax:
        vmax = vmin + 1e-6
    edges = np.linspace(vmin, vmax, bins + 1, dtype=np.float32)
    if np.any(edges[:-1] >= edges[1:]):
        raise ValueError(f"Too many bins for data range. Cannot create {bins} finite-sized bins.")
    return edges


def pss_bin(x, edges: np.ndarray) -> np.ndarray:
    """np.histogram's bin of each float32 value inside [edges[0], edges[-1]]: edges[i] <= x < edges[i+1]; the last bin is closed."""
    x = np.asarray(x, dtype=np.float32)
    return np.minimum(np.searchsorted(edges, x, side="right") - 1, len(edges) - 2)


def ensure_thw_shape(shape) -> Tuple[int, ...]:
    """io.ensure_thw's rule as an index: () keeps the array, 0 drops a leading 1, 1 drops axis 1, -1 drops a trailing 1."""
    shape = tuple(shape)
    drop = []
    if len(shape) == 5 and shape[0] == 1:
        drop.append(0)
        shape = shape[1:]
    if len(shape) == 4 and shape[1] == 1:
        drop.append(1)
        shape = shape[:1] + shape[2:]
    if len(shape) == 4 and shape[-1] == 1:
        drop.append(-1)
        shape = shape[:-1]
    if len(shape) != 3:
        raise ValueError(f"Expected [T,H,W], got shape {shape}")
    return tuple(drop)


def _thw(x):
    for d in ensure_thw_shape(x.shape):
        x = x[0] if d == 0 else (x[:, 0] if d == 1 else x[..., 0])
    return x


def crop_origin(h: int, w: int, size: int) -> Tuple[int, int]:
    """io.crop_center's (top, left); ValueError when the crop exceeds the input."""
    if size > min(h, w):
        raise ValueError(f"crop size {size} exceeds input {h}x{w}")
    return (h - size) // 2, (w - size) // 2


def crop_mask(mask: np.ndarray, size: int) -> np.ndarray:
    """main._crop_mask: the center size x size window of a full-domain mask (no bounds check, as there)."""
    h, w = mask.shape
    top, left = (h - size) // 2, (w - size) // 2
    return mask[top:top + size, left:left + size]


def selection(mask, mode: str, size: int) -> np.ndarray:
    """The mode's pixels of the crop (io.select_by_mask): radar -> mask False, gauge -> mask True."""
    mask = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
    if mode not in ("radar", "gauge"):
        raise ValueError(f"Unknown mode: {mode}")
    if mask.shape != (size, size):
        raise ValueError(f"Mask shape {mask.shape} != data shape {(size, size)}")
    return ~mask if mode == "radar" else mask


_NATIVE = {torch.uint8, torch.float32, torch.float64}


def _to_device(x, device) -> torch.Tensor:
    """An input array on the device in a dtype the kernels read: uint8 / f32 / f64 as they are; values that those hold exactly are
    widened (bool -> uint8, small ints and half floats -> f32, other ints -> f64)."""
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        a = np.asarray(x)
        if a.dtype == np.bool_:
            a = a.astype(np.uint8)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype not in _NATIVE:
        t = t.to(torch.float32 if t.dtype in (torch.int8, torch.int16, torch.float16, torch.bfloat16) else torch.float64)
    return t.to(device, non_blocking=False).contiguous()


class _Method:
    def __init__(self):
        self.parts, self.pool_p, self.pool_g, self.sel_p, self.sel_g = [], [], [], [], []
        self.T = 0


class Exp1Evaluator:
    """Streaming exp1 scores.  ``update(method, pred, truth)`` adds one piece whose frames pair one for one (the longer side is
    truncated, as align_length does); the pieces of a method form its stack in the order given, and dTSSIM pairs frames across
    piece boundaries, as the reference does on its concatenated stack.  ``mask`` is the crop_size x crop_size mask (already
    cropped, as main.py passes it).  ``compute()`` syncs once and returns ``{method: {...}}`` in the reference's layout."""

    def __init__(self, mask, mode: str, crop_size: int, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, use_pool8: bool = True,
                 divide_by_3: bool = True, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("exp1 scoring runs on the GPU (HIP path); no GPU is visible and there is no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError(f"exp1 scoring runs on the GPU; got device {self.device}")
        self.size = int(crop_size)
        self.pool = 8 if use_pool8 else 1
        if self.size // self.pool == 0:
            raise ValueError(f"crop size {self.size} is smaller than the 8x8 pooling window")
        self.thresholds = tuple(float(t) for t in thresholds)
        if len(self.thresholds) > ops.EXP1_MAX_THR:
            raise ValueError(f"at most {ops.EXP1_MAX_THR} thresholds")
        self.mode, self.divide_by_3 = mode, bool(divide_by_3)
        self._sel = selection(mask, mode, self.size)
        rank = np.full(self._sel.size, -1, dtype=np.int32)
        flat = self._sel.ravel()
        rank[flat] = np.arange(int(flat.sum()), dtype=np.int32)
        self.nsel = int(flat.sum())
        self._rank = torch.from_numpy(rank).to(self.device)
        self._lut = torch.from_numpy(truth_lut(self.divide_by_3)).to(self.device)
        self._methods: Dict[str, _Method] = {}

    def reset(self):
        self._methods = {}

    def update(self, method: str, pred_event, truth_event):
        with torch.cuda.device(self.device):
            truth = _to_device(_thw(truth_event), self.device)
            pred = _to_device(_thw(pred_event), self.device)
            gtl = crop_origin(truth.shape[1], truth.shape[2], self.size)     # the truth is cropped first, as in run_exp1
            n = min(pred.shape[0], truth.shape[0])
            ptl = crop_origin(pred.shape[1], pred.shape[2], self.size)
            st = self._methods.get(method)
            if st is None:
                st = self._methods[method] = _Method()
            S, ps = self.size, self.size // self.pool
            for t0 in range(0, n, _MAX_FRAMES):
                tn = min(_MAX_FRAMES, n - t0)
                part = torch.empty(ops.exp1_workspace(tn, S, self.pool), device=self.device, dtype=torch.float64)
                pp = torch.empty(tn, ps, ps, device=self.device, dtype=torch.float32)
                pg = torch.empty_like(pp)
                sp = torch.empty(tn, self.nsel, device=self.device, dtype=torch.float32)
                sg = torch.empty_like(sp)
                ops.exp1_accumulate(pred[t0:t0 + tn], truth[t0:t0 + tn], ptl, gtl, S, self.pool, self._rank, self.nsel, self._lut,
                                    self.thresholds, self.divide_by_3, pp, pg, sp, sg, part)
                st.parts.append(part)
                st.pool_p.append(pp)
                st.pool_g.append(pg)
                st.sel_p.append(sp)
                st.sel_g.append(sg)
                st.T += tn

    def compute(self) -> Dict[str, Dict[str, object]]:
        names = list(self._methods)
        if not names:
            return {}
        outs = []
        with torch.cuda.device(self.device):
            for name in names:
                st = self._methods[name]
                if st.T == 0:
                    raise ValueError(f"method {name!r} has no frames to score")
                # the partials of all pieces in frame order, folded in one fixed order: where pieces were cut does not matter
                acc = torch.zeros(ops.EXP1_NSTAT, device=self.device, dtype=torch.float64)
                ops.exp1_merge(torch.cat(st.parts) if len(st.parts) > 1 else st.parts[0], acc)
                score = torch.empty(st.T, device=self.device, dtype=torch.float64)
                flag = torch.empty(st.T, device=self.device, dtype=torch.int32)
                edges = torch.empty(PSS_BINS + 2, device=self.device, dtype=torch.float32)
                t0 = 0
                for sp, sg in zip(st.sel_p, st.sel_g):
                    ops.exp1_hist(sp, sg, acc, score[t0:t0 + sp.shape[0]], flag[t0:t0 + sp.shape[0]], edges)
                    t0 += sp.shape[0]
                pp = torch.cat(st.pool_p).reshape(st.T, -1) if len(st.pool_p) > 1 else st.pool_p[0].reshape(st.T, -1)
                pg = torch.cat(st.pool_g).reshape(st.T, -1) if len(st.pool_g) > 1 else st.pool_g[0].reshape(st.T, -1)
                ssim3 = ops.exp1_ssim(pp, pg)
                outs.append(ops.exp1_finalize(acc, self.thresholds, score, flag, edges, ssim3))
            host = torch.stack(outs).cpu().numpy()         # the one host sync
        res = {}
        k = len(self.thresholds)
        for name, row in zip(names, host):
            if row[7 + 4 * k] != 0.0:
                raise ValueError(f"Too many bins for data range. Cannot create {PSS_BINS} finite-sized bins.")
            r = {m: float(row[i]) for i, m in enumerate(_METRICS)}
            for j, thr in enumerate(self.thresholds):
                r[f"CAT_{thr:g}"] = {c: float(row[7 + 4 * j + i]) for i, c in enumerate(_CATS)}
            res[name] = r
        return res


def _frames(x) -> int:
    return int(_thw(x).shape[0])


def _pieces(pred_events, truth_events):
    """Aligned pieces (pred slice, truth slice) of the two concatenations, truncated to the shorter one (align_length)."""
    n = min(sum(_frames(e) for e in pred_events), sum(_frames(e) for e in truth_events))
    i = j = a = b = 0
    while n > 0:
        tp, tt = _frames(pred_events[i]), _frames(truth_events[j])
        k = min(tp - a, tt - b, n)
        if k > 0:
            yield pred_events[i][a:a + k], truth_events[j][b:b + k]
        a, b, n = a + k, b + k, n - k
        if a == tp:
            i, a = i + 1, 0
        if b == tt:
            j, b = j + 1, 0


def run_exp1(preds, truth, mask, mode: str, crop_size: int, thresholds: Tuple[float, ...] = DEFAULT_THRESHOLDS, use_pool8: bool = True,
             divide_by_3: bool = True, device=None) -> Dict[str, Dict[str, object]]:
    """The reference's run_exp1 (experiments/exp1.py) on the device.  With a dict ``truth``, every method's events are taken in
    the truth's key order; an event a method lacks is skipped for that method (its stack then shifts against the truth's, as in
    the reference), and a method that is not a dict is left out."""
    if isinstance(truth, dict):
        keys = list(truth.keys())
        if not keys:
            return {}
        truth_events = [truth[k] for k in keys if truth.get(k) is not None]
        methods = {}
        for name, src in preds.items():
            if isinstance(src, dict):
                methods[name] = [src[k] for k in keys if src.get(k) is not None]
    else:
        truth_events = [truth]
        methods = {}
        for name, src in preds.items():
            if isinstance(src, dict):
                raise TypeError(f"method {name!r}: per-event predictions need a per-event truth")
            methods[name] = [src]
    if not truth_events:
        raise ValueError("Expected [T,H,W], got shape (0,)")
    ev = Exp1Evaluator(mask, mode, crop_size, thresholds, use_pool8, divide_by_3, device=device)
    truth_dev = [_to_device(_thw(e), ev.device) for e in truth_events]
    for t in truth_dev:
        crop_origin(t.shape[1], t.shape[2], ev.size)
    for name, events in methods.items():
        if not events:
            raise ValueError("Expected [T,H,W], got shape (0,)")
        pred_dev = [_to_device(_thw(e), ev.device) for e in events]
        for p, g in _pieces(pred_dev, truth_dev):
            ev.update(name, p, g)
    return ev.compute()


# ---- exp3 (reference experiments/exp3.py run_exp3) -------------------------------------------------------

EXP3_MAX_POINTS = 2000      # the scatter / residual panels' sample size
EXP3_SEED = 42              # np.random.default_rng(42), once per figure, advanced across methods
EXP3_MIN_VALUE = 0.1        # the pool keeps observations >= 0.1 mm/h
LOGFREQ_EDGES = np.linspace(0.0, 32.0, ops.EXP3_BINS + 1)
_SHAPE_ERROR = "Expected [T,H,W], got shape (0,)"


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
        if not torch.cuda.is_available():
            raise RuntimeError("exp3 analysis runs on the GPU (HIP path); no GPU is visible and there is no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError(f"exp3 analysis runs on the GPU; got device {self.device}")
        self.size = int(crop_size)
        self.mode, self.divide_by_3, self.per_event = mode, bool(divide_by_3), bool(per_event)
        self.max_points, self.seed = int(max_points), int(seed)
        self.methods = list(methods)
        if len(set(self.methods)) != len(self.methods):
            raise ValueError(f"method names repeat: {self.methods}")
        sel = selection(mask, mode, self.size)
        rank = np.full(sel.size, -1, dtype=np.int32)
        flat = sel.ravel()
        rank[flat] = np.arange(int(flat.sum()), dtype=np.int32)
        with torch.cuda.device(self.device):
            self._rank = torch.from_numpy(rank).to(self.device)
            self._lut = torch.from_numpy(truth_lut(self.divide_by_3)).to(self.device)
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
            raise ValueError(_SHAPE_ERROR)
        if not self.methods:
            raise ValueError("Number of columns must be a positive integer, not 0")     # the reference's empty figure row
        S, dev = self.size, self.device
        with torch.cuda.device(dev):
            per = []
            for name in self.methods:
                st = self._m[name]
                if not st.pieces:
                    raise ValueError(_SHAPE_ERROR)
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
            raise ValueError(_SHAPE_ERROR)              # the reference stacks nothing for it, then fails on the empty stack
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


# ---- exp2 (reference experiments/exp2.py run_exp2 / run_exp2_paper_zarr) ---------------------------------

PAPER_BOUNDS = (0, 0.5, 1, 2, 4, 8, 16, 200)
PAPER_COLORS = ("#000000", "#46327e", "#277f8e", "#4ac16d", "#a0da39", "#fde725", "#ffffff")
PAPER_SUB = 20
EXP2_MAX_EVENTS = 20        # the path form takes the first 20 events ...
EXP2_MAX_FRAMES = 30        # ... and 30 frames of each
# the GIF's index space: 0 .. 140 the colour table, then "bad" (NaN: transparent in matplotlib, the white figure shows), the gauge
# panel's black background, the discs' edge colour #dddddd, and 16 greys from white to black for the host-drawn text
EXP2_IDX_BAD = ops.EXP2_BAD
EXP2_IDX_BG = 142
EXP2_IDX_EDGE = 143
EXP2_IDX_GREY = 144
EXP2_GREYS = 16
_EXP2_MARGIN, _EXP2_GAP, _EXP2_STRIP, _EXP2_LABEL = 8, 8, 22, 18
_EXP2_BAR_GAP, _EXP2_BAR_H, _EXP2_TICK_H, _EXP2_CBL_H, _EXP2_BOTTOM = 10, 12, 14, 16, 6


def paper_cmap() -> Tuple[np.ndarray, np.ndarray]:
    """(bounds [142] f64, colors [141, 4] f64 RGBA) of the reference's _build_paper_cmap, with its arithmetic: every segment of
    PAPER_BOUNDS is ``np.linspace(lo, hi, 21, endpoint=False)`` (so the coarse bounds 0.5 ... 16 are not among the fine ones), the
    first kept whole and the others without their first point, then 200; 6 x 20 colours interpolated between the hex colours
    with t = k / 19, the last hex colour, and white up to 141."""
    fine = []
    for i in range(len(PAPER_BOUNDS) - 1):
        seg = np.linspace(PAPER_BOUNDS[i], PAPER_BOUNDS[i + 1], PAPER_SUB + 1, endpoint=False)
        fine.extend(seg.tolist() if i == 0 else seg[1:].tolist())
    fine.append(PAPER_BOUNDS[-1])
    bounds = np.asarray(fine, float)
    base = [tuple(int(h[i:i + 2], 16) / 255.0 for i in (1, 3, 5)) for h in PAPER_COLORS]
    colors = []
    for c0, c1 in zip(base[:-1], base[1:]):
        for k in range(PAPER_SUB):
            t = k / float(PAPER_SUB - 1)
            colors.append(tuple((1 - t) * a + t * b for a, b in zip(c0, c1)))
    colors.append(base[-1])
    while len(colors) < len(bounds) - 1:
        colors.append(base[-1])
    rgba = np.ones((len(colors), 4), dtype=np.float64)
    rgba[:, :3] = np.asarray(colors, dtype=np.float64)
    return bounds, rgba


def exp2_palette() -> np.ndarray:
    """The GIF palette [256, 3] uint8: the colour table as matplotlib turns it into bytes (``(rgba * 255).astype(uint8)``), then the
    entries listed at EXP2_IDX_*; the rest is black and unused."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[:EXP2_IDX_BAD] = (paper_cmap()[1][:, :3] * 255).astype(np.uint8)
    pal[EXP2_IDX_BAD] = 255
    pal[EXP2_IDX_BG] = 0
    pal[EXP2_IDX_EDGE] = 0xdd
    for i in range(EXP2_GREYS):
        pal[EXP2_IDX_GREY + i] = 255 - 17 * i
    return pal


def exp2_layout(npanels: int, size: int, zoom: int) -> Dict[str, int]:
    """Where things lie on the canvas: the title strip, the panel labels, the panel row (panel p at column ox + p * step), the
    colour bar.  pitch is the row pitch of the device canvas (the width rounded up to 16)."""
    side = size * zoom
    width = 2 * _EXP2_MARGIN + npanels * side + (npanels - 1) * _EXP2_GAP
    oy = _EXP2_STRIP + _EXP2_LABEL
    bar_y = oy + side + _EXP2_BAR_GAP
    height = bar_y + _EXP2_BAR_H + _EXP2_TICK_H + _EXP2_CBL_H + _EXP2_BOTTOM
    return {"width": width, "height": height, "pitch": ops.exp2_pitch(width), "oy": oy, "ox": _EXP2_MARGIN, "step": side + _EXP2_GAP,
            "side": side, "bar_y": bar_y}


def _exp2_text(text: str, size: int) -> np.ndarray:
    """A line of text as grey indices [h, w] (black on white, nearest of the 16 greys)."""
    from PIL import Image, ImageDraw, ImageFont
    try:
        font = ImageFont.load_default(size)
    except (TypeError, OSError):
        font = ImageFont.load_default()
    l, t, r, b = font.getbbox(text or " ")
    img = Image.new("L", (max(r, 1) + 2, max(b, 1) + 2), 255)
    ImageDraw.Draw(img).text((1, 1), text, fill=0, font=font)
    g = np.asarray(img, dtype=np.int32)
    return (EXP2_IDX_GREY + (255 - g + 8) // 17).astype(np.uint8)


def _exp2_paste(dst: np.ndarray, src: np.ndarray, y: int, cx: int, width: int):
    """src centred on column cx with its top at row y, clipped to dst[:, :width]."""
    x = cx - src.shape[1] // 2
    y0, x0 = max(y, 0), max(x, 0)
    y1, x1 = min(y + src.shape[0], dst.shape[0]), min(x + src.shape[1], width)
    if y1 > y0 and x1 > x0:
        dst[y0:y1, x0:x1] = src[y0 - y:y1 - y, x0 - x:x1 - x]


def exp2_chrome(labels: Sequence[str], size: int, zoom: int) -> np.ndarray:
    """The static part of an event's frames as palette indices [height, pitch]: white, the panel titles, and the colour bar (141
    colours of equal width, as matplotlib spaces a BoundaryNorm bar; ticks at PAPER_BOUNDS; "Rainfall (mm/h)")."""
    lay = exp2_layout(len(labels), size, zoom)
    W = lay["width"]
    img = np.full((lay["height"], lay["pitch"]), EXP2_IDX_GREY, dtype=np.uint8)
    for p, label in enumerate(labels):
        _exp2_paste(img, _exp2_text(label, 11), _EXP2_STRIP + 1, lay["ox"] + p * lay["step"] + lay["side"] // 2, W)
    x0, bw = _EXP2_MARGIN, W - 2 * _EXP2_MARGIN
    ncol = EXP2_IDX_BAD
    img[lay["bar_y"]:lay["bar_y"] + _EXP2_BAR_H, x0:x0 + bw] = (np.arange(bw) * ncol // bw).astype(np.uint8)[None, :]
    bounds = paper_cmap()[0]
    pos = np.interp(np.asarray(PAPER_BOUNDS, float), bounds, np.arange(len(bounds))) / ncol
    for b, f in zip(PAPER_BOUNDS[:-1], pos[:-1]):
        _exp2_paste(img, _exp2_text(f"{b:g}", 8), lay["bar_y"] + _EXP2_BAR_H + 1, x0 + int(f * bw), W)
    _exp2_paste(img, _exp2_text("Rainfall (mm/h)", 10), lay["bar_y"] + _EXP2_BAR_H + _EXP2_TICK_H, W // 2, W)
    return img


@dataclass
class Exp2Event:
    """One event of exp2 as palette indices.  ``panels`` [P, frames, S, S] uint8 in label order; a panel whose ``gauge`` flag is set
    is drawn as discs at ``points`` [K, 2] (row, column; np.argwhere order) over black, and its array holds the source's own
    indices (for the first panel: the observation's, of which ``point_idx`` [frames, K] are the discs' colours).  ``total`` is the
    count event_ranges.txt and the title report; ``frames`` (<= total: the observation may be shorter) is what the GIF holds."""
    key: str
    title: str
    labels: List[str]
    gauge: List[bool]
    panels: np.ndarray
    points: np.ndarray
    point_idx: np.ndarray
    frames: int
    total: int
    dev_panels: Optional[torch.Tensor] = field(default=None, repr=False, compare=False)

    @property
    def range_line(self) -> str:
        return f"{self.key}: frames 1-{self.total} (count={self.total})"


@dataclass
class Exp2Result:
    """The numbers behind run_exp2's files: the events, the palette [256, 3] the indices refer to, the colour table's bounds, and
    ``per_event`` (the path form: event_ranges.txt exists)."""
    events: List[Exp2Event]
    palette: np.ndarray
    bounds: np.ndarray
    per_event: bool = True

    @property
    def range_lines(self) -> List[str]:
        return [e.range_line for e in self.events]

    def save(self, path: str) -> None:
        head = {"per_event": self.per_event,
                "events": [{"key": e.key, "title": e.title, "labels": e.labels, "gauge": e.gauge, "frames": e.frames, "total": e.total}
                           for e in self.events]}
        arrays = {"header": np.array(json.dumps(head)), "palette": self.palette, "bounds": self.bounds}
        for i, e in enumerate(self.events):
            arrays[f"panels/{i}"], arrays[f"points/{i}"], arrays[f"point_idx/{i}"] = e.panels, e.points, e.point_idx
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path: str) -> "Exp2Result":
        with np.load(path) as z:
            head = json.loads(str(z["header"]))
            events = [Exp2Event(key=h["key"], title=h["title"], labels=h["labels"], gauge=h["gauge"], panels=z[f"panels/{i}"],
                                points=z[f"points/{i}"], point_idx=z[f"point_idx/{i}"], frames=h["frames"], total=h["total"])
                      for i, h in enumerate(head["events"])]
            return cls(events=events, palette=z["palette"], bounds=z["bounds"], per_event=head["per_event"])


class _Exp2Source:
    """Where an event's array comes from: a zarr path (zarr_lite), a dict of event arrays, or one array used for every event."""

    def __init__(self, src):
        self.src, self.group = src, None
        if isinstance(src, (str, os.PathLike)):
            from .data import zarr_lite
            self.group = zarr_lite.Group(os.fspath(src), "r")

    def keys(self) -> List[str]:
        return [k for k in (self.group.keys() if self.group is not None else self.src.keys()) if isinstance(k, str)]

    def get(self, key: str):
        if self.group is not None:
            try:
                node = self.group[key]
            except KeyError:
                raise FileNotFoundError(f"Missing event {key} in {self.src}") from None
            return np.asarray(node[:])
        if isinstance(self.src, dict):
            if self.src.get(key) is None:
                raise FileNotFoundError(f"Missing event {key} in the given events")
            return self.src[key]
        return self.src


def _exp2_device(device) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("exp2 renders run on the GPU (HIP path); no GPU is visible and there is no CPU fallback")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError(f"exp2 renders run on the GPU; got device {dev}")
    return dev


class _Exp2Tables:
    def __init__(self, dev, divide_by_3):
        self.dev, self.divide_by_3 = dev, bool(divide_by_3)
        self.bounds = paper_cmap()[0]
        self.bounds_d = torch.from_numpy(self.bounds).to(dev)
        self.lut = torch.from_numpy(truth_lut(self.divide_by_3)).to(dev)

    def index(self, src, tl, size, n, out):
        ops.exp2_index(src, tl, size, n, self.bounds_d, self.lut, self.divide_by_3, out)


def _exp2_mask_points(mask, size: int) -> np.ndarray:
    mask = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
    if mask.shape != (size, size):
        raise ValueError(f"operands could not be broadcast together with shapes ({size},{size}) {mask.shape}")
    return np.ascontiguousarray(np.argwhere(mask).astype(np.int32)).reshape(-1, 2)


def _exp2_event(tab: _Exp2Tables, key, title_of, truth, obs, preds, points, size, cap, input_label, truth_label) -> Exp2Event:
    """One event by the reference's rules: the truth and the observation are cropped and cut to ``cap`` frames; every prediction is
    aligned to the current truth (which it may shorten for the methods after it) before its crop; the common length ``total`` is
    applied to every panel, and the GIF holds min(total, observation frames) of them."""
    dev = tab.dev
    truth = _to_device(_thw(truth), dev)
    obs = _to_device(_thw(obs), dev)
    n_obs = obs.shape[0] if cap is None else min(obs.shape[0], cap)
    total = truth.shape[0] if cap is None else min(truth.shape[0], cap)
    panel_src = {input_label: (obs, crop_origin(obs.shape[1], obs.shape[2], size)),
                 truth_label: (truth, crop_origin(truth.shape[1], truth.shape[2], size))}
    for name, arr in preds:
        p = _to_device(_thw(arr), dev)
        total = min(p.shape[0], total)              # never grows: the last value is the common length
        panel_src[name] = (p, crop_origin(p.shape[1], p.shape[2], size))
    frames = max(min(total, n_obs), 0)
    labels = list(panel_src)
    gauge = [lb.lower() in ("input", "gauge") for lb in labels]
    panels = torch.empty(len(labels), frames, size, size, device=dev, dtype=torch.uint8)
    for i, lb in enumerate(labels):
        src, tl = panel_src[lb]
        tab.index(src, tl, size, frames, panels[i])
    host = panels.cpu().numpy()
    pidx = host[0][:, points[:, 0], points[:, 1]] if frames else np.zeros((0, points.shape[0]), np.uint8)
    return Exp2Event(key=key, title=title_of(total), labels=labels, gauge=gauge, panels=host, points=points,
                     point_idx=np.ascontiguousarray(pidx), frames=frames, total=total, dev_panels=panels)


def _exp2_is_events(x) -> bool:
    return isinstance(x, (str, os.PathLike, dict))


def iter_exp2(preds, truth, observation, mask_train, crop_size: int, divide_by_3: bool = True, mode: str = "radar", device=None):
    """Yields (per_event, Exp2Event) event by event; see compute_exp2."""
    dev = _exp2_device(device)
    size = int(crop_size)
    input_label, truth_label = ("Gauge", "Radar") if mode == "gauge" else ("Input", "Truth")
    with torch.cuda.device(dev):
        tab = _Exp2Tables(dev, divide_by_3)
        if _exp2_is_events(truth) and _exp2_is_events(observation):
            tsrc, osrc = _Exp2Source(truth), _Exp2Source(observation)
            # the reference's numeric key never matches (its pattern is r"event[_-]?(\\d+)"): the order is (10**9, key), plain sorted
            keys = sorted(tsrc.keys())
            if not keys:
                raise FileNotFoundError(f"No event groups found in {truth if not isinstance(truth, dict) else 'the given events'}")
            psrc = [(name, _Exp2Source(src)) for name, src in preds.items()]
            points = None
            for key in keys[:EXP2_MAX_EVENTS]:
                t, o = tsrc.get(key), osrc.get(key)
                # the reference crops truth and observation (ValueError) and applies the mask before it opens the methods
                for a in (t, o):
                    shp = _thw(a).shape
                    crop_origin(shp[1], shp[2], size)
                if points is None:
                    points = _exp2_mask_points(mask_train, size)
                evp = [(name, s.get(key)) for name, s in psrc]
                yield True, _exp2_event(tab, key, lambda n, k=key: f"{k} | total frames {n}", t, o, evp, points, size, EXP2_MAX_FRAMES,
                                        input_label, truth_label)
            return
        for name, src in preds.items():
            if _exp2_is_events(src):
                raise TypeError(f"method {name!r}: per-event predictions need a per-event truth and observation")
        for a in (truth, observation):
            shp = _thw(a).shape
            crop_origin(shp[1], shp[2], size)
        points = _exp2_mask_points(mask_train, size)
        yield False, _exp2_event(tab, "event_01", lambda n: f"Event 01 | total frames {n}", truth, observation, list(preds.items()),
                                 points, size, None, input_label, truth_label)


def compute_exp2(preds, truth, observation, mask_train, crop_size: int, divide_by_3: bool = True, mode: str = "radar",
                 device=None) -> Exp2Result:
    """The index panels of the reference's run_exp2 (experiments/exp2.py) on the device, without writing anything.  *Path form*:
    ``truth`` and ``observation`` are zarr paths or dicts of event arrays; the event keys are taken in lexicographic order, the
    first 20 of them, 30 frames each; a method is a path, a dict, or one array used for every event; an event a source lacks
    raises FileNotFoundError.  *Array form*: whole arrays, no frame cap, one event ``event_01``."""
    events, per_event = [], True
    for per_event, ev in iter_exp2(preds, truth, observation, mask_train, crop_size, divide_by_3, mode, device):
        ev.dev_panels = None
        events.append(ev)
    return Exp2Result(events=events, palette=exp2_palette(), bounds=paper_cmap()[0], per_event=per_event)


def default_zoom(size: int) -> int:
    """The panels' magnification when none is asked for: the smallest that makes a panel at least 256 pixels wide."""
    return max(1, -(-256 // int(size)))


def exp2_canvases(ev: Exp2Event, zoom: Optional[int] = None, device=None, titles: bool = True) -> np.ndarray:
    """The event's GIF frames as palette indices [frames, height, width] uint8: the chrome and the panel row composed on the device
    (p2i_exp2_compose), then the per-frame title strip ``<title> | Frame t/n`` drawn on the host."""
    dev = _exp2_device(device)
    S = ev.panels.shape[-1]
    zoom = default_zoom(S) if zoom is None else int(zoom)
    if zoom < 1:
        raise ValueError(f"zoom must be >= 1, got {zoom}")
    lay = exp2_layout(len(ev.labels), S, zoom)
    if ev.frames <= 0:
        return np.zeros((0, lay["height"], lay["width"]), np.uint8)
    pts = np.ascontiguousarray(ev.points, dtype=np.int32).reshape(-1, 2)
    if pts.size and (pts.min() < 0 or pts.max() >= S):
        raise ValueError("a mask point lies outside the panel")
    bits = sum(1 << i for i, g in enumerate(ev.gauge) if g)
    with torch.cuda.device(dev):
        panels = ev.dev_panels if ev.dev_panels is not None and ev.dev_panels.device == dev else torch.from_numpy(ev.panels).to(dev)
        chrome = torch.from_numpy(exp2_chrome(ev.labels, S, zoom)).to(dev)
        out = torch.empty(ev.frames, lay["height"], lay["pitch"], device=dev, dtype=torch.uint8)
        ops.exp2_compose(panels.contiguous(), zoom, bits, torch.from_numpy(pts).to(dev) if pts.size else None, chrome, lay["oy"], lay["ox"],
                         lay["step"], EXP2_IDX_BG, EXP2_IDX_EDGE, out)
        canv = np.ascontiguousarray(out.cpu().numpy()[:, :, :lay["width"]])
    if titles and ev.title:
        for t in range(ev.frames):
            _exp2_paste(canv[t], _exp2_text(f"{ev.title} | Frame {t + 1}/{ev.frames}", 12), 2, lay["width"] // 2, lay["width"])
    return canv


def write_exp2_gif(canvases: np.ndarray, palette: np.ndarray, path: str, fps: int) -> None:
    """The frames as one GIF of the given palette (no quantisation: the file's colours are the palette's), frame duration
    int(1000 / max(fps, 1)) ms, looping forever, as the reference saves it."""
    from PIL import Image
    imgs = []
    for c in canvases:
        im = Image.fromarray(np.ascontiguousarray(c, dtype=np.uint8))
        im.putpalette(np.asarray(palette, np.uint8).reshape(-1).tobytes())
        imgs.append(im)
    if not imgs:
        return
    duration = int(1000 / max(fps, 1))
    imgs[0].save(path, format="GIF", save_all=True, append_images=imgs[1:], duration=duration, loop=0, optimize=False)


def run_exp2(preds, truth, observation, mask_train, out_dir: str, crop_size: int, frames=None, vmin: float = 0.0, vmax: float = 0.0,
             gif_fps: int = 4, divide_by_3: bool = True, mode: str = "radar", device=None, zoom: Optional[int] = None) -> None:
    """The reference's run_exp2: ``comparison_<event>.gif`` per event and ``event_ranges.txt`` (path form), or
    ``comparison_event_01.gif`` (array form), plus ``exp2_data.npz`` (Exp2Result.save).  ``frames``, ``vmin`` and ``vmax`` are
    accepted and unused, as in the reference.  The GIFs are written event by event: when an event fails, the ones before it exist
    and event_ranges.txt does not, as there."""
    os.makedirs(out_dir, exist_ok=True)
    palette = exp2_palette()
    events, per_event = [], True
    for per_event, ev in iter_exp2(preds, truth, observation, mask_train, crop_size, divide_by_3, mode, device):
        if ev.frames > 0:
            write_exp2_gif(exp2_canvases(ev, zoom, device), palette, os.path.join(out_dir, f"comparison_{ev.key}.gif"), gif_fps)
        ev.dev_panels = None
        events.append(ev)
    res = Exp2Result(events=events, palette=palette, bounds=paper_cmap()[0], per_event=per_event)
    if per_event:
        with open(os.path.join(out_dir, "event_ranges.txt"), "w", encoding="utf-8") as f:
            for line in res.range_lines:
                f.write(line.rstrip() + "\n")
    res.save(os.path.join(out_dir, "exp2_data.npz"))


def paper_panels(observation_path, methods: Dict[str, object], events, mask, crop_size: int, method_order=None, device=None):
    """The paper grid's panels: per event ``(labels, idx [columns, rows, S, S] uint8, points [K, 2])``.  Column order defaults to
    RadarMasked, Nimrod (both the observation), then the methods; a method without a source and a frame beyond a source's length
    give a zero panel (index 0, as the reference's np.zeros maps)."""
    dev = _exp2_device(device)
    size = int(crop_size)
    if method_order is None:
        method_order = ["RadarMasked", "Nimrod"] + list(methods.keys())
    order = list(method_order)
    points = _exp2_mask_points(crop_mask(np.asarray(mask).astype(bool), size), size)
    out = []
    with torch.cuda.device(dev):
        tab = _Exp2Tables(dev, True)
        osrc = _Exp2Source(observation_path)
        msrc = {name: _Exp2Source(p) for name, p in methods.items() if p is not None and not (isinstance(p, str) and not p)}
        for event in events:
            key = f"event_{int(event['event_id']):02d}"
            select = [int(i) for i in event["select_idx"]]
            obs = _to_device(_thw(osrc.get(key)), dev)
            cache = {}                                      # source name -> its index frames [T, S, S] on the host

            def frames_of(sid, src):
                if sid not in cache:
                    idx = torch.empty(src.shape[0], size, size, device=dev, dtype=torch.uint8)
                    tab.index(src, crop_origin(src.shape[1], src.shape[2], size), size, src.shape[0], idx)
                    cache[sid] = idx.cpu().numpy()
                return cache[sid]
            cols = []
            for name in order:
                col = np.zeros((len(select), size, size), np.uint8)
                fr = None
                if name in ("RadarMasked", "Nimrod"):
                    fr = frames_of("", obs)
                elif name in msrc:
                    fr = frames_of("m:" + name, _to_device(_thw(msrc[name].get(key)), dev))
                if fr is not None:
                    for r, i in enumerate(select):
                        if i < fr.shape[0]:
                            col[r] = fr[i]                  # a negative index counts from the end, as source[idx] does there
                cols.append(col)
            out.append((list(order), np.stack(cols) if cols else np.zeros((0, len(select), size, size), np.uint8), points))
    return out


def run_exp2_paper_zarr(observation_path, methods: Dict[str, object], events, mask_path: str, crop_size: int, out_dir: str,
                        output_pdf: str, method_order=None, crop_pdf: bool = False, crop_output: str = "cropped_stitched.pdf",
                        crop_y_ranges=((0.019, 0.5), (0.58, 1.0)), crop_zoom: float = 3.0, crop_margin_left: float = 0.0,
                        crop_margin_right: float = 0.0, device=None) -> None:
    """The reference's run_exp2_paper_zarr: one PDF with, per event, a title row and one row per selected frame, one column per
    entry of the method order.  The panels' colour indices come from the device (paper_panels); matplotlib lays the RGBA panels
    out.  ``crop_pdf=True`` (the PyMuPDF branch) is not implemented."""
    if crop_pdf:
        raise NotImplementedError("crop_pdf needs PyMuPDF; experiments/main.py never asks for it")
    from matplotlib.cm import ScalarMappable
    from matplotlib.colors import BoundaryNorm, ListedColormap
    from matplotlib.figure import Figure
    from matplotlib.gridspec import GridSpec
    os.makedirs(out_dir, exist_ok=True)
    events = list(events)
    mask = np.loadtxt(mask_path).astype(bool)
    blocks = paper_panels(observation_path, methods, events, mask, crop_size, method_order, device)
    bounds, colors = paper_cmap()
    rgba = np.zeros((256, 4), np.uint8)
    rgba[:EXP2_IDX_BAD] = (colors * 255).astype(np.uint8)
    ncols = len(blocks[0][0]) if blocks else 0
    nrows_each = len(list(events[0]["select_idx"]))
    total_rows = (nrows_each + 1) * len(events)
    fig = Figure(figsize=(2.4 * ncols, 1.9 * total_rows))
    gs = GridSpec(nrows=total_rows, ncols=ncols, figure=fig, top=0.93, bottom=0.06, wspace=0.04, hspace=0.02)
    cmap = ListedColormap(colors[:, :3].tolist(), name=f"seg{PAPER_SUB}_smooth")
    sm = ScalarMappable(cmap=cmap, norm=BoundaryNorm(bounds, cmap.N, clip=True))
    sm.set_array([])
    cbar = fig.colorbar(sm, cax=fig.add_axes([0.20, 0.88, 0.60, 0.02]), orientation="horizontal", ticks=list(PAPER_BOUNDS))
    cbar.set_ticklabels([f"{b:g}" for b in PAPER_BOUNDS[:-1]] + [""])
    cbar.set_label("Rainfall (mm/h)", fontsize=13, labelpad=3)
    cbar.ax.tick_params(labelsize=11)

    def face_of(panel):                             # the discs' face colours: the panel's own colour at every mask point
        return (rgba[panel[points[:, 0], points[:, 1]]] / 255.0).reshape(-1, 4)
    row = 0
    for event, (labels, idx, points) in zip(events, blocks):
        ax_title = fig.add_subplot(gs[row, :])
        ax_title.axis("off")
        ax_title.text(-0.015, 0.2, event["title"], fontsize=14, fontweight="bold", ha="left", va="center", transform=ax_title.transAxes)
        row += 1
        for t in range(nrows_each):
            for m, label in enumerate(labels):
                ax = fig.add_subplot(gs[row + t, m])
                if label == "RadarMasked":
                    black = np.zeros(idx[m, t].shape + (4,), np.uint8)
                    black[..., 3] = 255
                    ax.imshow(black)
                    ax.scatter(points[:, 1], points[:, 0], c=face_of(idx[m, t]), s=24, edgecolors="#dddddd", linewidths=0.4, zorder=5)
                else:
                    ax.imshow(rgba[idx[m, t]])
                ax.set_xticks([])
                ax.set_yticks([])
                for s in ax.spines.values():
                    s.set_visible(False)
                if label == "Gauge":
                    ax.scatter(points[:, 1], points[:, 0], c=face_of(idx[m, t]), s=38, edgecolors="black", linewidths=0.7, zorder=5)
                if t == 0:
                    ax.set_title(label, fontsize=13)
                if m == 0:
                    ax.text(-0.12, 0.5, f"{t * 5} min", transform=ax.transAxes, ha="center", va="center", fontsize=12, rotation=90)
        row += nrows_each
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fig.tight_layout(rect=[0, 0, 1, 0.7])
    fig.savefig(os.path.join(out_dir, output_pdf), format="pdf", bbox_inches="tight")
