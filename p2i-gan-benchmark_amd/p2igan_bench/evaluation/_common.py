"""What the three experiments share: the rain-rate transform and its uint8 table, io.py's shape / crop / selection rules, the inputs'
way onto the device, the alignment of two event lists, the GPU check and the upload of the kernels' tables."""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch


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
