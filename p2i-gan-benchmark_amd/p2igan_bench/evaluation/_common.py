"""What the evaluation units share: the rain-rate transform and its uint8 table, io.py's shape / crop / selection rules, the inputs'
way onto the device, run_exp1's reading of event dicts and the alignment of two event lists, the GPU check and the upload of the
kernels' tables, the argument rules that more than one unit has, and ``Streaming``, the base of the streaming evaluators."""
from __future__ import annotations

from bisect import bisect_right
from itertools import accumulate
from typing import Tuple

import numpy as np
import torch

from .. import ops


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


def crop_origin(h: int, w: int, size) -> Tuple[int, int]:
    """io.crop_center's (top, left) of a ``size`` x ``size`` crop, or of a (rows, cols) one; ValueError when it exceeds the input."""
    rows, cols = size if isinstance(size, tuple) else (size, size)
    if rows > h or cols > w:
        what = f"crop {rows}x{cols}" if isinstance(size, tuple) else f"crop size {size}"
        raise ValueError(f"{what} exceeds input {h}x{w}")
    return (h - rows) // 2, (w - cols) // 2


def crop_mask(mask: np.ndarray, size: int) -> np.ndarray:
    """main._crop_mask: the center size x size window of a full-domain mask (no bounds check, as there)."""
    h, w = mask.shape
    top, left = (h - size) // 2, (w - size) // 2
    return mask[top:top + size, left:left + size]


def selection(mask, mode: str, size) -> np.ndarray:
    """The mode's pixels of the crop (io.select_by_mask): radar -> mask False, gauge -> mask True.  ``size`` as in ``crop_origin``."""
    mask = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
    if mode not in ("radar", "gauge"):
        raise ValueError(f"Unknown mode: {mode}")
    shape = size if isinstance(size, tuple) else (size, size)
    if mask.shape != shape:
        raise ValueError(f"Mask shape {mask.shape} != data shape {shape}")
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


def eval_device(device, what: str) -> torch.device:
    """The device an experiment runs on (the current one when none is given); ``what`` words the refusal, e.g. "exp1 scoring runs".
    There is no CPU path: without a GPU, or for a device that is none, RuntimeError."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} on the GPU (HIP path); no GPU is visible and there is no CPU fallback")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError(f"{what} on the GPU; got device {dev}")
    return dev


def device_tables(dev, divide_by_3: bool, sel=None):
    """(lut, rank) on the device: truth_lut as f64 [256] and, for a selection ``sel`` [S, S] bool, int32 [S * S] holding a selected
    pixel's ordinal in row-major order and -1 elsewhere (None without ``sel``)."""
    with torch.cuda.device(dev):
        lut = torch.from_numpy(truth_lut(divide_by_3)).to(dev)
        if sel is None:
            return lut, None
        flat = sel.ravel()
        rank = np.full(flat.size, -1, dtype=np.int32)
        rank[flat] = np.arange(int(flat.sum()), dtype=np.int32)
        return lut, torch.from_numpy(rank).to(dev)


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


NO_EVENTS = "Expected [T,H,W], got shape (0,)"      # the reference's error on a stack of no events


def event_lists(preds, truth):
    """run_exp1's reading of its inputs: (the truth's events, {method: its events}).  With a dict ``truth``, every method's events
    are taken in the truth's key order and None-valued events are dropped; an event a method lacks is skipped for that method (its
    stack then shifts against the truth's, as in the reference), and a method that is not a dict is left out.  Otherwise ``truth``
    and every method are one event each, and a dict method is a TypeError.  An empty truth dict gives ([], {}): nothing to score;
    a truth without a single event is the reference's empty stack, ValueError."""
    if isinstance(truth, dict):
        keys = list(truth.keys())
        if not keys:
            return [], {}
        truth_events = [truth[k] for k in keys if truth.get(k) is not None]
        methods = {name: [src[k] for k in keys if src.get(k) is not None] for name, src in preds.items() if isinstance(src, dict)}
    else:
        truth_events = [truth]
        methods = {}
        for name, src in preds.items():
            if isinstance(src, dict):
                raise TypeError(f"method {name!r}: per-event predictions need a per-event truth")
            methods[name] = [src]
    if not truth_events:
        raise ValueError(NO_EVENTS)
    return truth_events, methods


def upload_events(events, device):
    """The events as [T, H, W] tensors on the device."""
    return [_to_device(_thw(e), device) for e in events]


def cat(xs):
    """The launches' tensors as one (no copy of a single one)."""
    return torch.cat(xs) if len(xs) > 1 else xs[0]


def radar_thresholds(mode: str, thresholds, why: str) -> Tuple[float, ...]:
    """The rules of the units that score every pixel of the crop: radar only (``why`` words the refusal of 'gauge') and 1 to
    EXP1_MAX_THR thresholds, returned as floats."""
    if mode == "gauge":
        raise ValueError(f"{why} of the whole crop: mode 'gauge' (isolated gauge pixels) has no meaning")
    if mode != "radar":
        raise ValueError(f"Unknown mode: {mode}")
    thresholds = tuple(float(t) for t in thresholds)
    if not 0 < len(thresholds) <= ops.EXP1_MAX_THR:
        raise ValueError(f"1 to {ops.EXP1_MAX_THR} thresholds")
    return thresholds


def bounded_crop(crop_size) -> int:
    """Those units' crop size: 1 to SCALE_MAX_CROP."""
    size = int(crop_size)
    if not 0 < size <= ops.SCALE_MAX_CROP:
        raise ValueError(f"crop size {size}: 1 to {ops.SCALE_MAX_CROP}")
    return size


class Streaming:
    """What the streaming evaluators share: the device and its tables, the per-method state, the workspaces,
    the opening of ``update`` and the cut of a piece into launches.  An evaluator states ``what`` (it words the refusal to run
    without a GPU), ``size`` (its crop), ``_new_state()`` (a method's empty state) and ``_launch_frames()`` (the frames one launch may
    take), and keeps its own kernel calls and ``compute``."""

    max_frames = None      # tests set it to cut a few frames into several launches; caps the evaluator's own frames per launch

    def _start(self, device, divide_by_3: bool, sel=None):
        self.device = eval_device(device, self.what)
        self.divide_by_3 = bool(divide_by_3)
        self._lut, self._rank = device_tables(self.device, self.divide_by_3, sel)
        self._work, self._methods = {}, {}

    def reset(self):
        self._methods = {}

    def _state(self, method):
        st = self._methods.get(method)
        if st is None:
            st = self._methods[method] = self._new_state()
        return st

    def _buf(self, name: str, n: int, dtype) -> torch.Tensor:
        """The first n elements of the named workspace, grown (or re-typed) on demand."""
        b = self._work.get(name)
        if b is None or b.numel() < n or b.dtype != dtype:
            b = self._work[name] = torch.empty(n, device=self.device, dtype=dtype)
        return b[:n]

    def _upload(self, pred_event, truth_event):
        """(pred, truth) as [T, H, W] on the device; the truth goes first."""
        truth = _to_device(_thw(truth_event), self.device)
        return _to_device(_thw(pred_event), self.device), truth

    def _open(self, method, pred_event, truth_event):
        """An aligned piece: (pred, truth, their crop origins, the frames both have, the method's state).  The truth's crop is
        checked first, as in run_exp1."""
        pred, truth = self._upload(pred_event, truth_event)
        gtl = crop_origin(truth.shape[1], truth.shape[2], self.size)
        n = min(pred.shape[0], truth.shape[0])
        ptl = crop_origin(pred.shape[1], pred.shape[2], self.size)
        return pred, truth, ptl, gtl, n, self._state(method)

    def _cuts(self, n: int):
        """(first frame, frames) of each launch over a piece of n frames: at most ``_launch_frames()``, the evaluator's own rule."""
        step = max(1, self._launch_frames())
        if self.max_frames is not None:
            step = min(step, int(self.max_frames))
        for t0 in range(0, n, step):
            yield t0, min(step, n - t0)

    def pieces(self, truth_events, methods):
        """The aligned pieces of ``event_lists``' output, on the device: (method, pred piece, truth piece, (event, first frame) of
        the piece in the truth).  The truth is uploaded and every event's crop checked ahead of the first method."""
        truth_dev = upload_events(truth_events, self.device)
        for t in truth_dev:
            crop_origin(t.shape[1], t.shape[2], self.size)
        ends = list(accumulate(t.shape[0] for t in truth_dev))
        for name, events in methods.items():
            if not events:
                raise ValueError(NO_EVENTS)
            at = 0
            for p, g in _pieces(upload_events(events, self.device), truth_dev):
                e = bisect_right(ends, at)
                yield name, p, g, (e, at - (ends[e - 1] if e else 0))
                at += g.shape[0]
