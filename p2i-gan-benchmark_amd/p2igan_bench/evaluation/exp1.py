"""exp1 scoring (reference experiments/exp1.py ``run_exp1``) on csrc/eval_exp1.hip: ``Exp1Evaluator`` and ``run_exp1``, plus the host's
restatement of np.histogram's PSS bin edges.  The rules it reproduces, the reference's quirks included: DESIGN.md section 10."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from ._common import Streaming, cat, eval_device, event_lists, selection

DEFAULT_THRESHOLDS = (0.5, 2.0, 4.0, 8.0)
PSS_BINS = 50
PSS_MIN_VALUE = 0.5
_METRICS = ("MAE", "RMSE", "PSS", "SSIM", "DTSSIM_L1", "DTSSIM_L2", "NSE")
_CATS = ("POD", "FAR", "CSI", "HSS")
_MAX_FRAMES = 65535          # frames per accumulate launch (grid.y)


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


class Exp1Evaluator(Streaming):
    """Streaming exp1 scores.  ``update(method, pred, truth)`` adds one piece whose frames pair one for one (the longer side is
    truncated, as align_length does); the pieces of a method form its stack in the order given, and dTSSIM pairs frames across
    piece boundaries, as the reference does on its concatenated stack.  ``mask`` is the crop_size x crop_size mask (already
    cropped, as main.py passes it).  ``compute()`` syncs once and returns ``{method: {...}}`` in the reference's layout."""

    what = "exp1 scoring runs"

    def __init__(self, mask, mode: str, crop_size: int, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, use_pool8: bool = True,
                 divide_by_3: bool = True, device=None):
        device = eval_device(device, self.what)          # here the GPU check comes ahead of the arguments'
        self.size = int(crop_size)
        self.pool = 8 if use_pool8 else 1
        if self.size // self.pool == 0:
            raise ValueError(f"crop size {self.size} is smaller than the 8x8 pooling window")
        self.thresholds = tuple(float(t) for t in thresholds)
        if len(self.thresholds) > ops.EXP1_MAX_THR:
            raise ValueError(f"at most {ops.EXP1_MAX_THR} thresholds")
        self.mode = mode
        self._sel = selection(mask, mode, self.size)
        self.nsel = int(self._sel.sum())
        self._start(device, divide_by_3, self._sel)

    def _new_state(self):
        return SimpleNamespace(parts=[], pool_p=[], pool_g=[], sel_p=[], sel_g=[], T=0)

    def _launch_frames(self):
        return _MAX_FRAMES

    def update(self, method: str, pred_event, truth_event):
        with torch.cuda.device(self.device):
            pred, truth, ptl, gtl, n, st = self._open(method, pred_event, truth_event)
            S, ps = self.size, self.size // self.pool
            for t0, tn in self._cuts(n):
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
                ops.exp1_merge(cat(st.parts), acc)
                score = torch.empty(st.T, device=self.device, dtype=torch.float64)
                flag = torch.empty(st.T, device=self.device, dtype=torch.int32)
                edges = torch.empty(PSS_BINS + 2, device=self.device, dtype=torch.float32)
                t0 = 0
                for sp, sg in zip(st.sel_p, st.sel_g):
                    ops.exp1_hist(sp, sg, acc, score[t0:t0 + sp.shape[0]], flag[t0:t0 + sp.shape[0]], edges)
                    t0 += sp.shape[0]
                ssim3 = ops.exp1_ssim(cat(st.pool_p).reshape(st.T, -1), cat(st.pool_g).reshape(st.T, -1))
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


def run_exp1(preds, truth, mask, mode: str, crop_size: int, thresholds: Tuple[float, ...] = DEFAULT_THRESHOLDS, use_pool8: bool = True,
             divide_by_3: bool = True, device=None) -> Dict[str, Dict[str, object]]:
    """The reference's run_exp1 (experiments/exp1.py) on the device.  With a dict ``truth``, every method's events are taken in
    the truth's key order; an event a method lacks is skipped for that method (its stack then shifts against the truth's, as in
    the reference), and a method that is not a dict is left out (``event_lists``)."""
    truth_events, methods = event_lists(preds, truth)
    if not truth_events:
        return {}
    ev = Exp1Evaluator(mask, mode, crop_size, thresholds, use_pool8, divide_by_3, device=device)
    for name, p, g, _ in ev.pieces(truth_events, methods):
        ev.update(name, p, g)
    return ev.compute()
