"""Raw (non-autograd) operators over the C ABI of libp2i_hip.so.

Every function takes/returns contiguous fp32 CUDA tensors, validates shapes on the host BEFORE
any launch (a faulting kernel can reset the node), enqueues on torch's current stream and
raises RuntimeError on failure.  No CPU path exists here by design.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _hip
from ._hip import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_TANH, ConvDesc  # noqa: F401


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# HIP stream handle of the calling step.  torch.cuda.current_stream() costs ~1.5 us and a train step asks ~800 times; TrainEngine
# pins the handle for the duration of a step (step_stream), SideStream.run swaps in its own.  None: ask torch (every other caller).
_CUR_STREAM = None


def _stream():
    return _CUR_STREAM if _CUR_STREAM is not None else torch.cuda.current_stream().cuda_stream


class step_stream:
    """with ops.step_stream(): ...  -- every op inside enqueues on the stream that is current at entry."""

    def __enter__(self):
        global _CUR_STREAM
        self.prev = _CUR_STREAM
        _CUR_STREAM = torch.cuda.current_stream().cuda_stream
        return self

    def __exit__(self, *exc):
        global _CUR_STREAM
        _CUR_STREAM = self.prev
        return False


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.is_contiguous()):
            raise RuntimeError("p2i ops need contiguous CUDA tensors (the HIP path has no CPU fallback)")
        if t.dtype not in (torch.float32, torch.int32, torch.uint8, torch.int16):
            raise RuntimeError(f"unsupported dtype {t.dtype}")


class KernelProfile:
    """Optional live timing of the conv-engine launches with HIP events on the launch stream
    (torch's current stream).  Used by bench.py's instrumented pass for the roofline figure; off
    by default so that the measured throughput is unperturbed."""

    def __init__(self):
        self.records = []            # (kernel key, algorithmic flops, start event, end event)

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for key, flops, e0, e1 in self.records:
            a = agg.setdefault(key, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += e0.elapsed_time(e1) * 1e-3
            a[2] += flops
        return {k: {"launches": v[0], "seconds": v[1], "flops": v[2]} for k, v in agg.items()}


PROFILE: Optional[KernelProfile] = None


def _prof_begin():
    if PROFILE is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(e0, kind, spec, desc, stride1):
    if e0 is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    flops = 2.0 * desc.B * desc.Cout * desc.Cin * spec.ntaps * desc.To * desc.Ho * desc.Wo
    if kind == "wgrad":
        import ctypes
        wp = (ctypes.c_int * 4)()
        _hip.load().p2i_wgrad_last_plan(wp)
        key = {0: "wgrad_kernel<64>", 2: "c1_wgrad_kernel<32>", 3: "wgrad_x6_kernel (bf16-split x6)"}.get(wp[0]) or \
            "wgrad_dma_kernel<64, %d, %s, %d>%s" % (wp[1], "true" if wp[2] else "false", wp[3], "" if spec.k[0] == 1 else " (x%d kt slices)" % spec.k[0])
    else:
        import ctypes
        plan = (ctypes.c_int * 6)()
        _hip.load().p2i_conv_last_plan(plan)
        if plan[5] > 10:
            key = "patch_gemm_fused_kernel<%d, %d, %d, %d, %d> (strided dgrad, %d parity classes per workgroup)" % (plan[0], plan[1], plan[2], plan[3], plan[5] - 10, plan[5] - 10)
        elif plan[5] == 7 and plan[3] == 4:        # producer / consumer wave roles
            key = "patch_gemm_x6p_kernel<%d, %d, false> (%d x %d tile, %d taps per stage, producer / consumer waves, bf16-split x6)" % (
                plan[0] // 32, plan[4], plan[0], plan[1], plan[4])
        elif plan[5] == 7:
            key = "patch_gemm_x6c_kernel<%d, %d, false, %d> (%d x %d tile, %d taps per stage, bf16-split x6)" % (
                plan[1] // 32, plan[0] // 32, plan[4], plan[0], plan[1], plan[4])
        elif plan[5] == 3:
            key = "o1_fwd_kernel (single output channel, bandwidth-bound)"
        elif plan[5] == 4:
            key = "c1_dgrad_kernel (single input channel, %d taps)" % plan[4]
        elif plan[5] == 8 and plan[3] == 4:
            key = "patch_gemm_x6p_kernel<1, %d, true> (strided dgrad, 4 parity classes per workgroup, producer / consumer waves, bf16-split x6)" % plan[4]
        elif plan[5] == 8:
            key = "patch_gemm_x6c_kernel<8, 1, true, %d> (strided dgrad, 4 parity classes per workgroup, bf16-split x6)" % plan[4]
        else:
            key = "patch_gemm_dma_kernel<%d, %d, %d, %d, %d, %d>" % tuple(plan)
    PROFILE.records.append((key, flops, e0, e1))


# Convolution engine selection (forward and data gradient).  "auto" (default): the exact-fp32 bf16-split kernel of csrc/conv_x6c.hip
# (3-way bf16 split, six v_mfma_f32_32x32x16_bf16 products) on the layers where it is the faster one (3x3 stride-1 2-D layers with
# >= 200 workgroups: the generator's 64- and 128-channel levels at B=8; measured 63 vs 100 us on the 128-channel level), the
# v_mfma_f32_32x32x2_f32 kernels everywhere else; the choice is made inside the library (x6c_would_take).  "f32": f32 kernels only.
# ("x6" is accepted as an alias of "auto".)  Both are HIP paths.
import os as _os

CONV_ENGINE = _os.environ.get("P2I_CONV_ENGINE", "auto")
_X6_SCRATCH = {}


def _x6_scratch(numel: int, device):
    """uint16 scratch for the split weights of ONE conv call, reused by every call on the same stream (the split
    kernel and its consumer are stream-ordered, so the next call may overwrite it).  Its `_split` is the p2i_conv_split that
    offers it to a call: built with the buffer, so that a conv call constructs no ctypes structure."""
    if CONV_ENGINE not in ("auto", "x6"):
        return None
    key = (device.index, _stream())
    buf = _X6_SCRATCH.get(key)
    if buf is None or buf.numel() < numel:
        buf = torch.empty(max(numel, 1 << 22), device=device, dtype=torch.int16)
        buf._split = _hip.ConvSplit(None, buf.data_ptr(), None, 0)
        _X6_SCRATCH[key] = buf
    return buf


class X6Stack:
    """bf16 split of a stack of same-shape packed weights (n, taps, K, Mpad), made ONCE per weight update and on first need: the
    conv calls of its n layers then skip their per-call split (60 launches of ~5 us per step before).  Attached to the packed
    tensors as `wp._x6s = (stack, layer index)` by the batched fold / pack helpers."""

    def __init__(self, wstack):
        self.w = wstack
        self.wb = None
        self.n, self.taps, self.k, self.mpad = wstack.shape
        self.splits = {}                    # layer -> its p2i_conv_split, built at the layer's first call

    def layer_ptr(self, i):
        if self.wb is None:                 # first layer that the bf16-split kernel takes: split the whole stack in one launch
            self.wb = torch.empty(3 * self.w.numel(), device=self.w.device, dtype=torch.int16)
            _hip.check(_hip.load().p2i_x6_split(_ptr(self.w), _ptr(self.wb), self.n * self.taps, self.k, self.mpad, _stream()), "p2i_x6_split")
        return self.wb.data_ptr() + 2 * i * self.taps * self.k * self.mpad

    def split(self, i):
        sp = self.splits.get(i)
        if sp is None:
            sp = self.splits[i] = _hip.ConvSplit(self.layer_ptr(i), None, None, self.n * self.taps)
        return sp

    @staticmethod
    def attach(wstack, views):
        """views[i] is the caller's view wstack[i] (the attribute lives on the view OBJECT that is handed to the conv calls)."""
        if CONV_ENGINE in ("auto", "x6") and wstack is not None and wstack.shape[2] % 16 == 0 and wstack.shape[3] % 32 == 0:
            st = X6Stack(wstack)
            for i, v in enumerate(views):
                v._x6s = (st, i)


class _X6One:
    """One tensor's pre-split image (see x6_presplit): quacks like an X6Stack of a single layer."""

    def __init__(self, ptr, taps):
        self.ptr, self.n, self.taps = ptr, 1, taps
        self.sp = None

    def layer_ptr(self, i):
        return self.ptr

    def split(self, i):
        if self.sp is None:
            self.sp = _hip.ConvSplit(self.ptr, None, None, self.taps)
        return self.sp


def x6_presplit(tensors, wants, buf=None):
    """bf16 split of several packed weight tensors of DIFFERENT shapes in ONE launch (p2i_x6_split_batched) -- the discriminators'
    layers right after weight_pack_batched; `wants[i]` says whether any conv call of the coming pass would use tensor i's split
    (p2i_x6c_would_take).  Attaches `_x6s` to the tensors like X6Stack.attach does, so that conv_fwd / conv_dgrad skip their
    per-call split (18 launches of ~7 us per train step before).  buf: caller-owned int16 buffer to reuse.  Returns the buffer."""
    if CONV_ENGINE not in ("auto", "x6"):
        return buf
    sel = [t for t, w in zip(tensors, wants) if w and t is not None and t.shape[1] % 16 == 0]
    if not sel:
        return buf
    import ctypes
    need = sum(3 * t.numel() for t in sel)
    if buf is None or buf.numel() < need:
        buf = torch.empty(need, device=sel[0].device, dtype=torch.int16)
    n = len(sel)
    ptrs, off = [], 0
    for t in sel:
        ptrs.append(buf.data_ptr() + 2 * off)
        off += 3 * t.numel()
    arr_i = ctypes.c_int * n
    _hip.check(_hip.load().p2i_x6_split_batched(_ptr_array(sel), (ctypes.c_void_p * n)(*ptrs), arr_i(*[t.shape[0] for t in sel]),
                                                arr_i(*[t.shape[1] for t in sel]), arr_i(*[t.shape[2] for t in sel]), n, _stream()),
               "p2i_x6_split_batched")
    for t, p_ in zip(sel, ptrs):
        t._x6s = (_X6One(p_, t.shape[0]), 0)
        t._x6buf = buf                       # keeps the image alive as long as the packed tensor
    return buf


def _x6s_of(wp, d, dgrad, act=ACT_NONE):
    """The p2i_conv_split of this layer inside a pre-split stack when the call would run on the bf16-split kernel, else None."""
    h = getattr(wp, "_x6s", None)
    if h is None or CONV_ENGINE not in ("auto", "x6") or not _hip.load().p2i_x6c_would_take(d, 1 if dgrad else 0, act):
        return None
    st, i = h
    return st.split(i)


def _conv_split(wp, d, dgrad, act, scratch_ok, device, src_planes):
    """What the split pipe of one conv call may use: the layer's pre-split image, else (scratch_ok: a channel count the pipe can
    take at all) the per-stream scratch, else None = fp32-MFMA kernels only.  src_planes (a tensor of p2i_x6_split_planes,
    experiments only) is the one case that builds a descriptor on the fly."""
    sp = _x6s_of(wp, d, dgrad, act)
    if sp is None and scratch_ok:
        ws = _x6_scratch(3 * wp.numel(), device)
        sp = ws._split if ws is not None else None
    if sp is not None and src_planes is not None:
        sp = _hip.ConvSplit(sp.w_split, sp.w_scratch, src_planes.data_ptr(), sp.w_split_taps)
    return sp


# Weight-gradient partial tiles: stored to a per-stream scratch and summed by a second kernel (deterministic, and faster than
# 256-way float atomics); P2I_WGRAD_SLICES=0 keeps the atomic path.  256 slices * 9 taps * 64 * 64 floats cover every layer.
WGRAD_SLICES = _os.environ.get("P2I_WGRAD_SLICES", "1") != "0"
_WGRAD_WS = {}


def _wgrad_scratch(device):
    if not WGRAD_SLICES:
        return None
    key = (device.index, _stream())
    buf = _WGRAD_WS.get(key)
    if buf is None:
        buf = torch.empty(256 * (9 * 64 * 64 + 512) + 1024, device=device, dtype=torch.float32)      # slices + their bias rows
        _WGRAD_WS[key] = buf
    return buf


# Depth of SideStream.run calls on the Python stack.  A side stream is only ever forked from the step's ORIGIN stream: forking a
# stream from a stream that is itself a fork (a SideStream used inside another SideStream.run) is legal in the CUDA model but ends
# hipGraph capture in a segmentation fault on ROCm 7.2 -- reproduced with torch tensors only by tools/graph_nested_fork.py (cases
# `nested*`: SIGSEGV; `flat*`: fine; gpurun_out/r4a/nested_fork.log).  models/p2igan.py::_side_of therefore hands out no side stream
# while another one is running (depth > 0): the nested work runs in line on the current side stream, eager and captured alike.
_SIDE_DEPTH = 0


def side_depth() -> int:
    return _SIDE_DEPTH


class SideStream:
    """A second HIP stream for work that nothing on the main stream waits for until a join: the weight-gradient kernels of a
    backward pass (each needs only tensors the data-gradient chain has already produced, and its result is consumed once per
    level).  Run beside the data-gradient chain they fill each other's kernel tails (single-round grids: ~10 us of ramp / drain /
    launch gap per kernel) and hide the wgrad slice-reduce kernels.  Dependencies are HIP events; tensors handed to the side
    stream are kept alive until the join (the caching allocator would otherwise hand their memory to the main stream)."""

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device)
        self.keep = []
        self.pending = False

    def run(self, fn, *tensors, after=None):
        # everything enqueued on the forking stream so far (producers of `tensors`) -> this side stream.  after: a token of
        # mark_stream() instead -- the side work then depends on what the forking stream held at THAT point only (TrainEngine enqueues
        # the step's head on the main stream first and lets the side work start beside it, not behind it)
        if after is None:
            fork(_stream(), self.stream.cuda_stream)
        else:
            _hip.check(_hip.load().p2i_event_wait(after, self.stream.cuda_stream), "p2i_event_wait")
        global _CUR_STREAM, _SIDE_DEPTH
        prev, _CUR_STREAM = _CUR_STREAM, self.stream.cuda_stream
        _SIDE_DEPTH += 1
        try:
            with torch.cuda.stream(self.stream):
                out = fn()
        finally:
            _CUR_STREAM = prev
            _SIDE_DEPTH -= 1
        self.keep.extend(tensors)
        self.pending = True
        return out

    def mark(self):
        """A wait token after everything enqueued on the side stream so far (the main stream can wait for PART of the side work):
        call it -- token() -- on the thread of control whose current stream shall wait."""
        slot = _next_slot()
        _hip.check(_hip.load().p2i_event_record(slot, self.stream.cuda_stream), "p2i_event_record")
        return lambda: _hip.check(_hip.load().p2i_event_wait(slot, _stream()), "p2i_event_wait")

    def join(self):
        if self.pending:
            fork(self.stream.cuda_stream, _stream())
            self.pending = False
        self.keep.clear()


# Cross-stream dependencies go through the library's event table (p2i_event_record / p2i_event_wait: 256 slots of events without
# timing, include/p2i_hip.h) instead of torch.cuda.Event objects: a launch tape (p2i_tape_*) sees them, and a fork costs two ctypes
# calls instead of an event allocation + record + wait through torch.  Slots are handed out round-robin; a step uses ~40.
_SLOT = 0


def _next_slot() -> int:
    global _SLOT
    _SLOT = (_SLOT + 1) % 256
    return _SLOT


def mark_stream() -> int:
    """A token for "everything enqueued on the current launch stream so far" (SideStream.run(..., after=token))."""
    slot = _next_slot()
    _hip.check(_hip.load().p2i_event_record(slot, _stream()), "p2i_event_record")
    return slot


def fork(src_stream: int, dst_stream: int):
    """dst_stream waits for everything enqueued on src_stream so far (raw HIP stream handles)."""
    lib = _hip.load()
    slot = _next_slot()
    _hip.check(lib.p2i_event_record(slot, src_stream), "p2i_event_record")
    _hip.check(lib.p2i_event_wait(slot, dst_stream), "p2i_event_wait")


# Run-to-run reproducibility: the scratch of the library's deterministic reductions (include/p2i_hip.h, p2i_det_workspace), registered
# once per process and device at the first backward op.  P2I_DETERMINISTIC=0 keeps the float atomics (A/B runs).
_DET = {}


def det_ready(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key in _DET:
        return
    if _os.environ.get("P2I_DETERMINISTIC", "1") == "0":
        _DET[key] = None
        return
    mb = int(_os.environ.get("P2I_DET_SCRATCH_MB", "128"))
    part = torch.empty(mb << 18, device=device, dtype=torch.float32)
    cnt = torch.zeros(8192, device=device, dtype=torch.int32)
    torch.cuda.current_stream(device).synchronize()          # the counters are zero before any kernel of any stream can use them
    _hip.check(_hip.load().p2i_det_workspace(part.data_ptr(), part.numel(), cnt.data_ptr(), cnt.numel()), "p2i_det_workspace")
    _DET[key] = (part, cnt)


def pad32(n: int) -> int:
    return (n + 31) // 32 * 32


@dataclass(frozen=True)
class ConvSpec:
    """Static description of one convolution layer (2-D layers have kt = st = 1, pt = 0)."""
    cin: int
    cout: int
    k: Tuple[int, int, int]
    stride: Tuple[int, int, int] = (1, 1, 1)
    pad: Tuple[int, int, int] = (0, 0, 0)

    @property
    def ntaps(self) -> int:
        return self.k[0] * self.k[1] * self.k[2]

    def out_dims(self, t, h, w):
        return tuple((d + 2 * p - k) // s + 1 for d, p, k, s in zip((t, h, w), self.pad, self.k, self.stride))

    def desc(self, b, t, h, w) -> ConvDesc:
        return _conv_desc(self, b, t, h, w)

    def wp_f_shape(self):
        return (self.ntaps, self.cin, pad32(self.cout))

    def wp_d_shape(self):
        return (self.ntaps, self.cout, pad32(self.cin))


import functools


@functools.lru_cache(maxsize=512)
def _conv_desc(spec: ConvSpec, b, t, h, w) -> ConvDesc:
    """The (read-only) descriptor of one layer at one input size: built once, ~3 us of ctypes work per call otherwise."""
    to, ho, wo = spec.out_dims(t, h, w)
    return ConvDesc(b, spec.cin, spec.cout, t, h, w, to, ho, wo, *spec.k, *spec.stride, *spec.pad)


def _dims5(x: torch.Tensor):
    if x.dim() == 4:
        b, c, h, w = x.shape
        return b, c, 1, h, w
    b, c, t, h, w = x.shape
    return b, c, t, h, w


def conv_fwd(spec: ConvSpec, x, wp_f, bias=None, residual=None, act=ACT_NONE, out=None, src_planes=None):
    lib = _hip.load()
    b, c, t, h, w = _dims5(x)
    if c != spec.cin or tuple(wp_f.shape) != spec.wp_f_shape():
        raise RuntimeError(f"conv_fwd: shape mismatch x={tuple(x.shape)} wp={tuple(wp_f.shape)} spec={spec}")
    to, ho, wo = spec.out_dims(t, h, w)
    oshape = (b, spec.cout, ho, wo) if x.dim() == 4 else (b, spec.cout, to, ho, wo)
    y = out if out is not None else torch.empty(oshape, device=x.device, dtype=torch.float32)
    if tuple(y.shape) != oshape or (residual is not None and tuple(residual.shape) != oshape):
        raise RuntimeError("conv_fwd: output/residual shape mismatch")
    if bias is not None and bias.numel() != spec.cout:
        raise RuntimeError("conv_fwd: bias size mismatch")
    _chk(x, wp_f, bias, residual, y)
    d = spec.desc(b, t, h, w)
    e0 = _prof_begin()
    sp = _conv_split(wp_f, d, False, act, spec.cin % 16 == 0, x.device, src_planes)
    _hip.check(lib.p2i_conv_fwd(d, _ptr(x), _ptr(wp_f), sp, _ptr(bias), _ptr(residual), _ptr(y), act, _stream()), "p2i_conv_fwd")
    _prof_end(e0, "fwd", spec, d, True)
    return y


def conv_dgrad(spec: ConvSpec, dy, wp_d, in_shape, y_act=None, act=ACT_NONE, add=None, mask_y=None, mask_act=ACT_NONE, src_planes=None):
    """dx for input of shape in_shape; if y_act is given dy is first multiplied by act'(y_act) (fp32-MFMA kernels only)."""
    lib = _hip.load()
    if len(in_shape) == 4:
        b, c, h, w = in_shape
        t = 1
    else:
        b, c, t, h, w = in_shape
    to, ho, wo = spec.out_dims(t, h, w)
    eshape = (b, spec.cout, ho, wo) if len(in_shape) == 4 else (b, spec.cout, to, ho, wo)
    if tuple(dy.shape) != eshape or c != spec.cin or tuple(wp_d.shape) != spec.wp_d_shape():
        raise RuntimeError(f"conv_dgrad: shape mismatch dy={tuple(dy.shape)} expected {eshape}")
    if y_act is not None and y_act.shape != dy.shape:
        raise RuntimeError("conv_dgrad: y_act shape mismatch")
    if add is not None and tuple(add.shape) != tuple(in_shape):
        raise RuntimeError("conv_dgrad: add shape mismatch")
    if mask_y is not None and tuple(mask_y.shape) != tuple(in_shape):
        raise RuntimeError("conv_dgrad: mask_y shape mismatch")
    dx = torch.empty(in_shape, device=dy.device, dtype=torch.float32)
    _chk(dy, wp_d, y_act, dx, add, mask_y)
    d = spec.desc(b, t, h, w)
    e0 = _prof_begin()
    sp = _conv_split(wp_d, d, True, ACT_NONE, spec.cout % 16 == 0 and spec.cin > 1, dy.device, src_planes) if y_act is None else None
    _hip.check(lib.p2i_conv_dgrad(d, _ptr(dy), _ptr(y_act), act, _ptr(wp_d), sp, _ptr(add), _ptr(mask_y), mask_act, _ptr(dx), _stream()),
               "p2i_conv_dgrad")
    _prof_end(e0, "dgrad", spec, d, spec.stride == (1, 1, 1))
    return dx


class ZeroArena:
    """One zero-filled buffer carved into the (atomically accumulated) gradient outputs of a backward pass:
    a single memset instead of one fill kernel per weight tensor."""

    def __init__(self, numel: int, device, buf: Optional[torch.Tensor] = None):
        """buf: a caller-owned buffer of >= numel floats to reuse (zeroed here by p2i_zero, no ATen fill kernel)."""
        if buf is not None and buf.numel() >= numel:
            self.buf = buf
            zero_(buf[:numel])
        else:
            self.buf = torch.zeros(numel, device=device, dtype=torch.float32)
        self.off = 0

    def take(self, shape):
        n = 1
        for d in shape:
            n *= d
        n4 = (n + 3) // 4 * 4                       # keep every carve 16-B aligned
        if self.off + n4 > self.buf.numel():
            return zero_(torch.empty(shape, device=self.buf.device, dtype=torch.float32))
        t = self.buf[self.off:self.off + n].view(shape)
        self.off += n4
        return t


def conv_wgrad(spec: ConvSpec, x, dy, y_act=None, act=ACT_NONE, want_bias=False, arena: Optional["ZeroArena"] = None, db_out=None,
               dwp_out=None):
    """Packed weight gradient dwp_f [ntaps][cin][pad32(cout)] (+ bias gradient).  db_out: caller-owned (cout,) tensor the bias
    gradient is ADDED to (e.g. the parameter's view of the flat gradient buffer)."""
    lib = _hip.load()
    det_ready(x.device)
    b, c, t, h, w = _dims5(x)
    to, ho, wo = spec.out_dims(t, h, w)
    eshape = (b, spec.cout, ho, wo) if x.dim() == 4 else (b, spec.cout, to, ho, wo)
    if tuple(dy.shape) != eshape or c != spec.cin:
        raise RuntimeError(f"conv_wgrad: shape mismatch dy={tuple(dy.shape)} expected {eshape}")
    if y_act is not None and y_act.shape != dy.shape:
        raise RuntimeError("conv_wgrad: y_act shape mismatch")
    if db_out is not None and (tuple(db_out.shape) != (spec.cout,) or not want_bias):
        raise RuntimeError("conv_wgrad: db_out must be (cout,) and want_bias set")
    if dwp_out is not None:                      # caller-owned, zeroed packed-gradient target
        if tuple(dwp_out.shape) != spec.wp_f_shape() or (want_bias and db_out is None):
            raise RuntimeError("conv_wgrad: dwp_out shape mismatch (and a bias gradient needs db_out with it)")
        dwp, db = dwp_out, db_out
    elif arena is not None:
        dwp = arena.take(spec.wp_f_shape())
        db = db_out if db_out is not None else (arena.take((spec.cout,)) if want_bias else None)
    else:
        dwp = zero_(torch.empty(spec.wp_f_shape(), device=x.device, dtype=torch.float32))
        db = db_out if db_out is not None else (zero_(torch.empty(spec.cout, device=x.device, dtype=torch.float32)) if want_bias else None)
    _chk(x, dy, y_act, dwp, db)
    d = spec.desc(b, t, h, w)
    e0 = _prof_begin()
    ws = _wgrad_scratch(x.device)
    _hip.check(lib.p2i_conv_wgrad(d, _ptr(x), _ptr(dy), _ptr(y_act), act, _ptr(dwp), _ptr(db), _ptr(ws), ws.numel() if ws is not None else 0,
                                  _stream()), "p2i_conv_wgrad")
    _prof_end(e0, "wgrad", spec, d, True)
    return dwp, db


# --------------------------------------------------------------------------- weights
def doconv_fold(W, D, D_diag, out_ch, in_ch, groups, ksz, identity_rep=0, need_d=True):
    lib = _hip.load()
    nt = ksz * ksz
    exp_w = (out_ch, in_ch // groups, nt)
    if tuple(W.shape) != exp_w:
        raise RuntimeError(f"doconv_fold: W shape {tuple(W.shape)} != {exp_w}")
    if ksz == 3 and (tuple(D.shape) != (in_ch, 9, 9) or tuple(D_diag.shape) != (in_ch, 9, 9)):
        raise RuntimeError("doconv_fold: D/D_diag shape mismatch")
    wp_f = torch.empty((nt, in_ch, pad32(out_ch)), device=W.device, dtype=torch.float32)
    wp_d = torch.empty((nt, out_ch, pad32(in_ch)), device=W.device, dtype=torch.float32) if need_d else None
    _chk(W, D, D_diag)
    _hip.check(lib.p2i_doconv_fold_fwd(_ptr(W), _ptr(D), _ptr(D_diag), out_ch, in_ch, groups, ksz, identity_rep,
                                       _ptr(wp_f), _ptr(wp_d), _stream()), "p2i_doconv_fold_fwd")
    return wp_f, wp_d


def doconv_fold_bwd(dwp_f, W, D, D_diag, out_ch, in_ch, groups, ksz, out=None):
    """out = (dW target, dD target or None): written in place (caller-owned, e.g. views of the flat gradient buffer)."""
    lib = _hip.load()
    if tuple(dwp_f.shape) != (ksz * ksz, in_ch, pad32(out_ch)):
        raise RuntimeError("doconv_fold_bwd: dwp shape mismatch")
    if out is not None:
        dW, dD = out
        if dW.shape != W.shape or (ksz == 3 and (dD is None or dD.shape != D.shape)):
            raise RuntimeError("doconv_fold_bwd: output target shape mismatch")
        _chk(dW, dD)
    else:
        dW = torch.empty_like(W)
        dD = torch.empty_like(D) if ksz == 3 else None
    _chk(dwp_f, W, D, D_diag)
    _hip.check(lib.p2i_doconv_fold_bwd(_ptr(dwp_f), _ptr(W), _ptr(D), _ptr(D_diag), out_ch, in_ch, groups, ksz,
                                       _ptr(dW), _ptr(dD), _stream()), "p2i_doconv_fold_bwd")
    return dW, dD


def _ptr_array(ts):
    import ctypes
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def doconv_fold_batched(layers, out_ch, in_ch, need_d=True):
    """doconv_fold for a list of same-shape 3x3 layers [(W, D, D_diag), ...] (groups 1) in ONE launch.
    Returns [(wp_f, wp_d), ...] (views of two stacked buffers)."""
    lib = _hip.load()
    n = len(layers)
    for W, D, Dd in layers:
        if tuple(W.shape) != (out_ch, in_ch, 9) or tuple(D.shape) != (in_ch, 9, 9) or tuple(Dd.shape) != (in_ch, 9, 9):
            raise RuntimeError("doconv_fold_batched: shape mismatch")
        _chk(W, D, Dd)
    dev = layers[0][0].device
    wf = torch.empty((n, 9, in_ch, out_ch), device=dev, dtype=torch.float32)
    wd = torch.empty((n, 9, out_ch, in_ch), device=dev, dtype=torch.float32) if need_d else None
    _hip.check(lib.p2i_doconv_fold_fwd_batched(_ptr_array([l[0] for l in layers]), _ptr_array([l[1] for l in layers]),
                                               _ptr_array([l[2] for l in layers]), n, out_ch, in_ch, _ptr_array([wf[i] for i in range(n)]),
                                               _ptr_array([wd[i] for i in range(n)]) if need_d else None, _stream()),
               "p2i_doconv_fold_fwd_batched")
    wfs = [wf[i] for i in range(n)]
    wds = [wd[i] for i in range(n)] if need_d else [None] * n
    X6Stack.attach(wf, wfs)
    if need_d:
        X6Stack.attach(wd, wds)
    return list(zip(wfs, wds))


def doconv_fold_bwd_batched(dwps, layers, out_ch, in_ch, outs=None):
    """doconv_fold_bwd for same-shape layers in TWO launches.  Returns ([dW...], [dD...]).  outs = ([dW targets], [dD targets])
    writes the results straight into caller-owned tensors (the flat gradient buffer's views)."""
    lib = _hip.load()
    n = len(layers)
    if len(dwps) != n:
        raise RuntimeError("doconv_fold_bwd_batched: list length mismatch")
    for g in dwps:
        if tuple(g.shape) != (9, in_ch, out_ch):
            raise RuntimeError("doconv_fold_bwd_batched: dwp shape mismatch")
        _chk(g)
    dev = dwps[0].device
    if outs is not None:
        dWs, dDs = outs
        for t, shp in [(t, (out_ch, in_ch, 9)) for t in dWs] + [(t, (in_ch, 9, 9)) for t in dDs]:
            if tuple(t.shape) != shp:
                raise RuntimeError("doconv_fold_bwd_batched: output target shape mismatch")
            _chk(t)
    else:
        dW = torch.empty((n, out_ch, in_ch, 9), device=dev, dtype=torch.float32)
        dD = torch.empty((n, in_ch, 9, 9), device=dev, dtype=torch.float32)
        dWs, dDs = [dW[i] for i in range(n)], [dD[i] for i in range(n)]
    _hip.check(lib.p2i_doconv_fold_bwd_batched(_ptr_array(dwps), _ptr_array([l[0] for l in layers]), _ptr_array([l[1] for l in layers]),
                                               _ptr_array([l[2] for l in layers]), n, out_ch, in_ch, _ptr_array(dWs),
                                               _ptr_array(dDs), _stream()), "p2i_doconv_fold_bwd_batched")
    return dWs, dDs


def weight_pack(w, sigma=None, need_f=True, need_d=True):
    """w (O, I, *k) -> packed wp_f / wp_d, optionally divided by the device scalar sigma."""
    lib = _hip.load()
    O, I = w.shape[0], w.shape[1]
    nt = w[0, 0].numel()
    wp_f = torch.empty((nt, I, pad32(O)), device=w.device, dtype=torch.float32) if need_f else None
    wp_d = torch.empty((nt, O, pad32(I)), device=w.device, dtype=torch.float32) if need_d else None
    _chk(w, sigma)
    _hip.check(lib.p2i_weight_pack(_ptr(w), O, I, nt, _ptr(sigma), _ptr(wp_f), _ptr(wp_d), _stream()), "p2i_weight_pack")
    return wp_f, wp_d


def weight_pack_batched(ws, sigmas=None, need_d=True, buf=None):
    """weight_pack for a list of (O, I, ntaps) weights (different shapes) in ONE launch; one zero-filled buffer holds every
    packed output (the padded columns must read 0).  Returns [(wp_f, wp_d), ...].  buf: a caller-owned buffer that was
    zero-filled ONCE and is only ever used for this same list of shapes (the pack kernel rewrites exactly the non-padding
    entries, so the padding stays zero): saves the per-call fill."""
    import ctypes
    lib = _hip.load()
    n = len(ws)
    Os, Is, NTs = [w.shape[0] for w in ws], [w.shape[1] for w in ws], [w.shape[2] for w in ws]
    for w in ws:
        if w.dim() != 3:
            raise RuntimeError("weight_pack_batched: weights must be (O, I, ntaps)")
        _chk(w)
    sizes_f = [nt * i * pad32(o) for o, i, nt in zip(Os, Is, NTs)]
    sizes_d = [nt * o * pad32(i) for o, i, nt in zip(Os, Is, NTs)] if need_d else [0] * n
    need = sum(sizes_f) + sum(sizes_d)
    if buf is None:
        buf = zero_(torch.empty(need, device=ws[0].device, dtype=torch.float32))
    elif buf.numel() != need:
        raise RuntimeError("weight_pack_batched: reused buffer has the wrong size")
    outs, off = [], 0
    for k in range(n):
        f = buf[off:off + sizes_f[k]].view(NTs[k], Is[k], pad32(Os[k]))
        off += sizes_f[k]
        d = None
        if need_d:
            d = buf[off:off + sizes_d[k]].view(NTs[k], Os[k], pad32(Is[k]))
            off += sizes_d[k]
        outs.append((f, d))
    arr_i = ctypes.c_int * n
    _hip.check(lib.p2i_weight_pack_batched(_ptr_array(ws), arr_i(*Os), arr_i(*Is), arr_i(*NTs),
                                           _ptr_array(sigmas) if sigmas is not None else None, _ptr_array([o[0] for o in outs]),
                                           _ptr_array([o[1] for o in outs]) if need_d else None, n, _stream()), "p2i_weight_pack_batched")
    return outs


def weight_unpack_grad_batched(dwps, likes, w_origs=None, sigmas=None, us=None, vs=None, outs=None, accumulate=False):
    """weight_unpack_grad for a list of layers (different shapes) in two launches.  Returns [dw, ...] shaped like `likes`.
    outs: caller-owned targets (numel must match); accumulate: dw += instead of dw = (second backward of a D step)."""
    import ctypes
    lib = _hip.load()
    det_ready(dwps[0].device)
    n = len(dwps)
    Os, Is, NTs = [l.shape[0] for l in likes], [l.shape[1] for l in likes], [l.shape[2] for l in likes]
    for g, o, i, nt in zip(dwps, Os, Is, NTs):
        if tuple(g.shape) != (nt, i, pad32(o)):
            raise RuntimeError("weight_unpack_grad_batched: dwp shape mismatch")
        _chk(g)
    if outs is not None:
        if len(outs) != n or any(o.numel() != l.numel() for o, l in zip(outs, likes)):
            raise RuntimeError("weight_unpack_grad_batched: output targets do not match")
        _chk(*outs)
        dws = outs
    else:
        if accumulate:
            raise RuntimeError("weight_unpack_grad_batched: accumulate needs caller-owned targets")
        dws = [torch.empty_like(l) for l in likes]
    dots = torch.empty(n, device=dwps[0].device, dtype=torch.float32)
    arr_i = ctypes.c_int * n
    none = [None] * n
    _hip.check(lib.p2i_weight_unpack_grad_batched(_ptr_array(dwps), arr_i(*Os), arr_i(*Is), arr_i(*NTs), _ptr_array(w_origs or none),
                                                  _ptr_array(sigmas or none), _ptr_array(us or none), _ptr_array(vs or none),
                                                  _ptr(dots), _ptr_array(dws), n, int(accumulate), _stream()),
               "p2i_weight_unpack_grad_batched")
    return dws


def weight_unpack_grad(dwp_f, like, w_orig=None, sigma=None, u=None, v=None, out=None):
    lib = _hip.load()
    det_ready(dwp_f.device)
    O, I = like.shape[0], like.shape[1]
    nt = like[0, 0].numel()
    if tuple(dwp_f.shape) != (nt, I, pad32(O)):
        raise RuntimeError("weight_unpack_grad: dwp shape mismatch")
    if out is not None and out.numel() != like.numel():
        raise RuntimeError("weight_unpack_grad: output target size mismatch")
    dw = out if out is not None else torch.empty_like(like)
    _chk(dw)
    scratch = torch.empty(4, device=like.device, dtype=torch.float32) if sigma is not None else None
    _chk(dwp_f, w_orig, sigma, u, v)
    _hip.check(lib.p2i_weight_unpack_grad(_ptr(dwp_f), O, I, nt, _ptr(w_orig), _ptr(sigma), _ptr(u), _ptr(v),
                                          _ptr(scratch), _ptr(dw), _stream()), "p2i_weight_unpack_grad")
    return dw


def spectral_norm(w, u, v, training: bool):
    """In-place power iteration on u, v (training) and sigma (device scalar tensor of shape (1,))."""
    lib = _hip.load()
    O = w.shape[0]
    K = w.numel() // O
    if u.numel() != O or v.numel() != K:
        raise RuntimeError("spectral_norm: u/v size mismatch")
    sigma = torch.empty(1, device=w.device, dtype=torch.float32)
    scratch = torch.empty(O + K + 4, device=w.device, dtype=torch.float32)
    _chk(w, u, v)
    _hip.check(lib.p2i_spectral_norm(_ptr(w), O, K, _ptr(u), _ptr(v), int(training), _ptr(sigma), _ptr(scratch), _stream()),
               "p2i_spectral_norm")
    return sigma


def spectral_norm_batched(ws, us, vs, training: bool, snapshot: bool = False):
    """spectral_norm() for a list of layers in 4 launches (these kernels are launch-latency bound).  Returns the list of
    sigma tensors (views of one buffer); with snapshot=True also (u copies, v copies) of the updated vectors (the backward
    pass needs the u, v of THIS forward; the next forward overwrites them in place)."""
    import ctypes
    lib = _hip.load()
    n = len(ws)
    if not (1 <= n <= 16 and len(us) == n and len(vs) == n):
        raise RuntimeError("spectral_norm_batched: 1..16 layers")
    Os = [w.shape[0] for w in ws]
    Ks = [w.numel() // w.shape[0] for w in ws]
    for w, u, v, O, K in zip(ws, us, vs, Os, Ks):
        if u.numel() != O or v.numel() != K:
            raise RuntimeError("spectral_norm_batched: u/v size mismatch")
        _chk(w, u, v)
    dev = ws[0].device
    sig = torch.empty(n, device=dev, dtype=torch.float32)
    offs = [0]
    for O, K in zip(Os, Ks):
        offs.append(offs[-1] + (O + K + 4 + 3) // 4 * 4)
    scratch = torch.empty(offs[-1], device=dev, dtype=torch.float32)
    arr_p = ctypes.c_void_p * n
    arr_i = ctypes.c_int * n
    wp, up, vp = arr_p(*[w.data_ptr() for w in ws]), arr_p(*[u.data_ptr() for u in us]), arr_p(*[v.data_ptr() for v in vs])
    sp = arr_p(*[sig.data_ptr() + 4 * i for i in range(n)])
    cp = arr_p(*[scratch.data_ptr() + 4 * o for o in offs[:-1]])
    usn = vsn = None
    usp = vsp = None
    if snapshot and training:
        uo, vo = [0], [0]
        for O, K in zip(Os, Ks):
            uo.append(uo[-1] + O)
            vo.append(vo[-1] + K)
        ubuf = torch.empty(uo[-1], device=dev, dtype=torch.float32)
        vbuf = torch.empty(vo[-1], device=dev, dtype=torch.float32)
        usn = [ubuf[uo[i]:uo[i + 1]] for i in range(n)]
        vsn = [vbuf[vo[i]:vo[i + 1]] for i in range(n)]
        usp, vsp = arr_p(*[t.data_ptr() for t in usn]), arr_p(*[t.data_ptr() for t in vsn])
    _hip.check(lib.p2i_spectral_norm_batched(wp, arr_i(*Os), arr_i(*Ks), up, vp, int(training), sp, cp, usp, vsp, n, _stream()),
               "p2i_spectral_norm_batched")
    sigs = [sig[i:i + 1] for i in range(n)]
    if snapshot:
        if not training:
            usn, vsn = [u.clone() for u in us], [v.clone() for v in vs]
        return sigs, usn, vsn
    return sigs


# --------------------------------------------------------------------------- generator glue
def attn_fwd(x, w0, b0, w1, b1):
    lib = _hip.load()
    B, T, H, W = x.shape
    out = torch.empty_like(x)
    _chk(x, w0, b0, w1, b1)
    if w0.numel() != T * T or b0.numel() != T or w1.numel() != T * T or b1.numel() != T:
        raise RuntimeError("attn_fwd: parameter size mismatch")
    _hip.check(lib.p2i_attn_fwd(_ptr(x), _ptr(w0), _ptr(b0), _ptr(w1), _ptr(b1), _ptr(out), B, T, H * W, _stream()), "p2i_attn_fwd")
    return out


def attn_bwd(x, w0, b0, w1, b1, dout, out=None):
    """out: four caller-owned, ZEROED targets shaped like (w0, b0, w1, b1) (the kernel adds atomically)."""
    lib = _hip.load()
    det_ready(x.device)
    B, T, H, W = x.shape
    if dout.shape != x.shape:
        raise RuntimeError("attn_bwd: dout shape mismatch")
    if out is not None:
        if len(out) != 4 or any(o.numel() != p_.numel() for o, p_ in zip(out, (w0, b0, w1, b1))):
            raise RuntimeError("attn_bwd: output targets do not match")
        g = list(out)
        _chk(*g)
    else:
        g = [zero_(torch.empty_like(p_)) for p_ in (w0, b0, w1, b1)]
    _chk(x, w0, b0, w1, b1, dout)
    _hip.check(lib.p2i_attn_bwd(_ptr(x), _ptr(w0), _ptr(b0), _ptr(w1), _ptr(b1), _ptr(dout), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                                _ptr(g[3]), B, T, H * W, _stream()), "p2i_attn_bwd")
    return g


_LINSPACE = {}


def _grid_tables(T, H, W, device):
    """torch.linspace(0,1,n) tables of layer.py:246-256, computed on the host CPU exactly as the
    reference's CPU path does (CPU and GPU linspace kernels differ in the last bit)."""
    key = (T, H, W, str(device))
    if key not in _LINSPACE:
        _LINSPACE[key] = tuple(torch.linspace(0, 1, n).to(device) for n in (W, H, T))
    return _LINSPACE[key]


def _idw_strict(pt_count):
    """A sample with 1..3 mask points: the reference raises in torch.topk(k=4) (layer.py:282); the kernels write zeros for it
    (include/p2i_hip.h) because raising needs the point counts on the host -- a device sync in the middle of the step.
    P2I_IDW_STRICT=1 pays that sync and raises the reference's error."""
    if _os.environ.get("P2I_IDW_STRICT", "0") == "1":
        n = pt_count.cpu()
        if bool(((n > 0) & (n < 4)).any()):
            raise RuntimeError("selected index k out of range (idw_3d_knn needs at least 4 mask points per sample, got %s)" % n.tolist())


def idw_amb_counts(amb, B, Q):
    """(voxels per sample that pass 1 left to pass 2, voxels per sample that pass 2's fixed-bound phase left to the exact replay) of
    the work buffer ops.idw_fwd(..., _amb_out=[...]) hands out (tests, tools)."""
    per = Q + 1 + (Q + 255) // 256
    return amb[:B * per].view(B, per)[:, 0].cpu(), amb[B * per:B * per + B * (Q + 1)].view(B, Q + 1)[:, 0].cpu()


def idw_fwd(vals_src, mask, tau=0.05, save=True, _amb_out=None):
    """vals_src, mask: (B,T,H,W).  Returns out and the saved selection (pt_pos, sel_idx, sel_w)."""
    lib = _hip.load()
    B, T, H, W = vals_src.shape
    if mask.shape != vals_src.shape:
        raise RuntimeError("idw_fwd: mask shape mismatch")
    dev = vals_src.device
    Q = T * H * W
    gx, gy, gz = _grid_tables(T, H, W, dev)
    out = torch.empty_like(vals_src)
    pt_pos = torch.empty(B * Q, device=dev, dtype=torch.int32)
    pt_count = torch.empty(B, device=dev, dtype=torch.int32)
    frame_count = torch.empty(B * T, device=dev, dtype=torch.int32)
    row_start = torch.empty(B * T * (H + 1), device=dev, dtype=torch.int32)
    pt_xyzn = torch.empty(B * Q * 4, device=dev, dtype=torch.float32)
    sel_idx = torch.empty(B * Q * 4, device=dev, dtype=torch.int32) if save else None
    sel_w = torch.empty(B * Q * 4, device=dev, dtype=torch.float32) if save else None
    _chk(vals_src, mask)
    amb = None                                          # no work buffer: the reference's scan for every voxel (P2I_IDW_FAST=0: A/B, tests)
    if _os.environ.get("P2I_IDW_FAST", "1") != "0":     # two-pass search (p2i_hip.h)
        amb = torch.empty(B * (2 * Q + 2 + (Q + 255) // 256), device=dev, dtype=torch.int32)
        if _amb_out is not None:                        # tests: the per-sample count of voxels left to the replay pass
            _amb_out.append(amb)
    _hip.check(lib.p2i_idw_fwd(_ptr(vals_src), _ptr(mask), _ptr(gx), _ptr(gy), _ptr(gz), _ptr(out), _ptr(pt_pos), _ptr(pt_count),
                               _ptr(frame_count), _ptr(row_start), _ptr(pt_xyzn), _ptr(sel_idx), _ptr(sel_w), _ptr(amb), B, T, H, W,
                               float(tau), _stream()), "p2i_idw_fwd")
    _idw_strict(pt_count)
    return out, (pt_pos, pt_count, sel_idx, sel_w)


def idw_bwd(dout, saved):
    lib = _hip.load()
    det_ready(dout.device)
    B, T, H, W = dout.shape
    pt_pos, pt_count, sel_idx, sel_w = saved
    dvals = torch.empty_like(dout)
    _chk(dout)
    _hip.check(lib.p2i_idw_bwd(_ptr(dout), _ptr(pt_pos), _ptr(pt_count), _ptr(sel_idx), _ptr(sel_w), _ptr(dvals), B, T, H, W, _stream()),
               "p2i_idw_bwd")
    return dvals


def pooldup_fwd(x):
    lib = _hip.load()
    B, Cc, H, W = x.shape
    y = torch.empty((B, 2 * Cc, H // 2, W // 2), device=x.device, dtype=torch.float32)
    _chk(x)
    _hip.check(lib.p2i_pooldup_fwd(_ptr(x), _ptr(y), B, Cc, H, W, _stream()), "p2i_pooldup_fwd")
    return y


def pooldup_bwd(x, dy):
    lib = _hip.load()
    B, Cc, H, W = x.shape
    if tuple(dy.shape) != (B, 2 * Cc, H // 2, W // 2):
        raise RuntimeError("pooldup_bwd: dy shape mismatch")
    dx = torch.empty_like(x)
    _chk(x, dy)
    _hip.check(lib.p2i_pooldup_bwd(_ptr(x), _ptr(dy), _ptr(dx), B, Cc, H, W, _stream()), "p2i_pooldup_bwd")
    return dx


def upmod_fwd(x, pos, bias=None, act=ACT_NONE):
    """bilinear x2 (align_corners) * 2 sigmoid(pos); with `bias`: act(that + bias[c]) -- UPPos's tail when the 1x1 projection has
    already been applied at the low resolution (p2i_upmod_fwd in p2i_hip.h has the algebra)."""
    lib = _hip.load()
    B, Cc, Sh, Sw = x.shape
    if pos.numel() != 4 * Sh * Sw:
        raise RuntimeError(f"upmod_fwd: pos has {pos.numel()} elements, expected {4 * Sh * Sw}")
    u = torch.empty((B, Cc, 2 * Sh, 2 * Sw), device=x.device, dtype=torch.float32)
    _chk(x, pos, bias)
    if bias is not None and bias.numel() != Cc:
        raise RuntimeError("upmod_fwd: bias size mismatch")
    _hip.check(lib.p2i_upmod_fwd(_ptr(x), _ptr(pos), _ptr(bias), act, _ptr(u), B, Cc, Sh, Sw, _stream()), "p2i_upmod_fwd")
    return u


def upmod_bwd(x, pos, du, need_dx=True, dpos_out=None):
    """dpos_out: caller-owned ZEROED target shaped like pos (the kernel adds atomically)."""
    lib = _hip.load()
    det_ready(x.device)
    B, Cc, Sh, Sw = x.shape
    if tuple(du.shape) != (B, Cc, 2 * Sh, 2 * Sw):
        raise RuntimeError("upmod_bwd: du shape mismatch")
    dx = torch.empty_like(x) if need_dx else None
    if dpos_out is not None and dpos_out.numel() != pos.numel():
        raise RuntimeError("upmod_bwd: dpos target size mismatch")
    dpos = dpos_out if dpos_out is not None else zero_(torch.empty_like(pos))
    _chk(dpos)
    _chk(x, pos, du)
    _hip.check(lib.p2i_upmod_bwd(_ptr(x), _ptr(pos), _ptr(du), _ptr(dx), _ptr(dpos), B, Cc, Sh, Sw, _stream()), "p2i_upmod_bwd")
    return dx, dpos


# --------------------------------------------------------------------------- discriminator tail
def dtail_fwd(out2d, out3d, alpha2d):
    lib = _hip.load()
    B, c2, H2, W2 = out2d.shape
    B3, c3, T3, H3, W3 = out3d.shape
    if c2 != 1 or c3 != 1 or B3 != B:
        raise RuntimeError("dtail_fwd: expects single-channel branch outputs")
    fused = torch.empty((B, H2 * W2), device=out2d.device, dtype=torch.float32)
    _chk(out2d, out3d, alpha2d)
    _hip.check(lib.p2i_dtail_fwd(_ptr(out2d), _ptr(out3d), _ptr(alpha2d), _ptr(fused), B, H2, W2, T3, H3, W3, _stream()), "p2i_dtail_fwd")
    return fused


def dtail_bwd(out2d, out3d_shape, alpha2d, dfused, need_alpha=True, da_out=None):
    """da_out: caller-owned (1,) target the alpha2d gradient is ADDED to."""
    lib = _hip.load()
    det_ready(out2d.device)
    B, _, H2, W2 = out2d.shape
    _, _, T3, H3, W3 = out3d_shape
    d2 = torch.empty_like(out2d)
    d3 = torch.empty(out3d_shape, device=out2d.device, dtype=torch.float32)
    da = (da_out if da_out is not None else zero_(torch.empty_like(alpha2d))) if need_alpha else None
    _chk(da)
    _chk(out2d, alpha2d, dfused)
    _hip.check(lib.p2i_dtail_bwd(_ptr(out2d), _ptr(alpha2d), _ptr(dfused), _ptr(d2), _ptr(d3), _ptr(da), B, H2, W2, T3, H3, W3,
                                 _stream()), "p2i_dtail_bwd")
    return d2, d3, da


# --------------------------------------------------------------------------- losses / optimiser
def recloss(pred, target, k1_alpha):
    """Returns (out3 device tensor [pool, reg, pool+k1*reg], dpred)."""
    lib = _hip.load()
    B, T = pred.shape[0], pred.shape[1]
    HW = pred[0, 0].numel()
    if pred.shape != target.shape:
        raise RuntimeError("recloss: shape mismatch")
    out3 = torch.empty(3, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred)
    scratch = torch.empty(B * (T - 1) * HW + 4096, device=pred.device, dtype=torch.float32)
    _chk(pred, target)
    _hip.check(lib.p2i_recloss(_ptr(pred), _ptr(target), float(k1_alpha), _ptr(out3), _ptr(dpred), _ptr(scratch), B, T, HW, _stream()),
               "p2i_recloss")
    return out3, dpred


_LOSS_TYPES = {"hinge": 0, "lsgan": 1, "nsgan": 2}


def _check_bce(loss, loss_type):
    """nn.BCELoss (the reference's 'nsgan', losses.py:201-202) raises for inputs outside [0, 1]; the kernel flags that with a NaN
    loss.  Costs a host sync, on the nsgan path only (the named configs use hinge)."""
    if loss_type == "nsgan" and bool(torch.isnan(loss).any()):
        raise RuntimeError("all elements of input should be between 0 and 1")


def gan_loss_d(logits_real, logits_fake, loss_type="hinge", real_label=1.0, fake_label=0.0):
    lib = _hip.load()
    if loss_type not in _LOSS_TYPES:
        raise ValueError(f"Unsupported GAN loss type: {loss_type}")
    n = logits_real.numel()
    loss = torch.empty(1, device=logits_real.device, dtype=torch.float32)
    da, db = torch.empty_like(logits_real), torch.empty_like(logits_fake)
    _chk(logits_real, logits_fake)
    _hip.check(lib.p2i_gan_loss(_ptr(logits_real), _ptr(logits_fake), n, _LOSS_TYPES[loss_type], 0, 1.0, real_label, fake_label,
                                _ptr(loss), _ptr(da), _ptr(db), _stream()), "p2i_gan_loss")
    _check_bce(loss, loss_type)
    return loss, da, db


def gan_loss_g(logits, weight, loss_type="hinge", real_label=1.0):
    lib = _hip.load()
    if loss_type not in _LOSS_TYPES:
        raise ValueError(f"Unsupported GAN loss type: {loss_type}")
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    da = torch.empty_like(logits)
    _chk(logits)
    _hip.check(lib.p2i_gan_loss(_ptr(logits), None, logits.numel(), _LOSS_TYPES[loss_type], 1, float(weight), real_label, 0.0,
                                _ptr(loss), _ptr(da), None, _stream()), "p2i_gan_loss")
    _check_bce(loss, loss_type)
    return loss, da


# --------------------------------------------------------------------------- the reference's other objectives (csrc/loss_ext.hip)
def _chk_f32(*ts):
    _chk(*ts)
    for t in ts:
        if t.dtype != torch.float32:
            raise RuntimeError(f"the loss kernels are fp32 only (got {t.dtype})")


def _same(a, b, what):
    if a.shape != b.shape:
        raise RuntimeError(f"{what}: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")


def loss_transform_fwd(x):
    _chk_f32(x)
    y = torch.empty_like(x)
    if x.numel():
        _hip.check(_hip.load().p2i_loss_transform_fwd(_ptr(x), _ptr(y), x.numel(), _stream()), "p2i_loss_transform_fwd")
    return y


def loss_transform_bwd(x, dy):
    _chk_f32(x, dy)
    _same(x, dy, "loss_transform_bwd")
    dx = torch.empty_like(x)
    if x.numel():
        _hip.check(_hip.load().p2i_loss_transform_bwd(_ptr(x), _ptr(dy), _ptr(dx), x.numel(), _stream()), "p2i_loss_transform_bwd")
    return dx


def _btinner(shape, what):
    if len(shape) < 2 or shape[1] < 2:
        raise RuntimeError(f"{what}: needs [B, T >= 2, ...], got {tuple(shape)}")
    inner = 1
    for s in shape[2:]:
        inner *= s
    return shape[0], shape[1], inner


def fdiff_fwd(x):
    """x[:, 1:] - x[:, :-1]."""
    _chk_f32(x)
    B, T, inner = _btinner(x.shape, "fdiff_fwd")
    out = torch.empty((B, T - 1) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    if out.numel():
        _hip.check(_hip.load().p2i_fdiff_fwd(_ptr(x), _ptr(out), B, T, inner, _stream()), "p2i_fdiff_fwd")
    return out


def fdiff_bwd(dy, T):
    _chk_f32(dy)
    if dy.dim() < 2 or dy.shape[1] != T - 1:
        raise RuntimeError(f"fdiff_bwd: gradient {tuple(dy.shape)} is not that of {T} frames")
    dx = torch.empty((dy.shape[0], T) + tuple(dy.shape[2:]), device=dy.device, dtype=torch.float32)
    if dx.numel():
        _hip.check(_hip.load().p2i_fdiff_bwd(_ptr(dy), _ptr(dx), dy.shape[0], T, dx[0, 0].numel(), _stream()), "p2i_fdiff_bwd")
    return dx


def wl1_fwd(pred, target):
    """mean(w(target) * |pred - target|) as a 0-dim device tensor."""
    _chk_f32(pred, target)
    _same(pred, target, "wl1_fwd")
    det_ready(pred.device)
    out = torch.empty((), device=pred.device, dtype=torch.float32)
    _hip.check(_hip.load().p2i_wl1_fwd(_ptr(pred), _ptr(target), _ptr(out), pred.numel(), _stream()), "p2i_wl1_fwd")
    return out


def wl1_bwd(pred, target, gout):
    _chk_f32(pred, target, gout)
    dpred = torch.empty_like(pred)
    _hip.check(_hip.load().p2i_wl1_bwd(_ptr(pred), _ptr(target), _ptr(gout), _ptr(dpred), pred.numel(), _stream()), "p2i_wl1_bwd")
    return dpred


def _rows(shape, what):
    if len(shape) < 2:
        raise RuntimeError(f"{what}: needs at least 2 dims, got {tuple(shape)}")
    L = 1
    for s in shape[2:]:
        L *= s
    if shape[0] * shape[1] == 0 or L == 0:
        raise RuntimeError(f"{what}: empty tensor {tuple(shape)}")
    return shape[0] * shape[1], L


def softmax_t_fwd(x, temperature):
    _chk_f32(x)
    rows, L = _rows(x.shape, "softmax_t_fwd")
    y = torch.empty_like(x)
    _hip.check(_hip.load().p2i_softmax_t_fwd(_ptr(x), _ptr(y), rows, L, float(temperature), _stream()), "p2i_softmax_t_fwd")
    return y


def softmax_t_bwd(y, dy, temperature):
    _chk_f32(y, dy)
    _same(y, dy, "softmax_t_bwd")
    rows, L = _rows(y.shape, "softmax_t_bwd")
    dx = torch.empty_like(y)
    _hip.check(_hip.load().p2i_softmax_t_bwd(_ptr(y), _ptr(dy), _ptr(dx), rows, L, float(temperature), _stream()), "p2i_softmax_t_bwd")
    return dx


def kl_fwd(p, q):
    _chk_f32(p, q)
    _same(p, q, "kl_fwd")
    _rows(p.shape, "kl_fwd")
    det_ready(p.device)
    out = torch.empty((), device=p.device, dtype=torch.float32)
    _hip.check(_hip.load().p2i_kl_fwd(_ptr(p), _ptr(q), _ptr(out), p.numel(), p.shape[0], _stream()), "p2i_kl_fwd")
    return out


def kl_bwd(p, q, gout):
    _chk_f32(p, q, gout)
    dp = torch.empty_like(p)
    _hip.check(_hip.load().p2i_kl_bwd(_ptr(p), _ptr(q), _ptr(gout), _ptr(dp), p.numel(), p.shape[0], _stream()), "p2i_kl_bwd")
    return dp


def _planes(x, what, dims=(3, 4)):
    if x.dim() not in dims or x.numel() == 0:
        raise RuntimeError(f"{what}: needs a non-empty {' or '.join(str(d) + '-D' for d in dims)} tensor, got {tuple(x.shape)}")
    H, W = x.shape[-2], x.shape[-1]
    return x.numel() // (H * W), H, W


def spool_out(n):
    return (n - 1) // 4 + 1


def spool_fwd(x, want_idx=True):
    """MaxPool2d(5, 4, 2) on the last two dims; returns (out, argmax plane indices or None)."""
    _chk_f32(x)
    N, H, W = _planes(x, "spool_fwd")
    oshape = tuple(x.shape[:-2]) + (spool_out(H), spool_out(W))
    out = torch.empty(oshape, device=x.device, dtype=torch.float32)
    idx = torch.empty(oshape, device=x.device, dtype=torch.int32) if want_idx else None
    _hip.check(_hip.load().p2i_spool_fwd(_ptr(x), _ptr(out), _ptr(idx), N, H, W, _stream()), "p2i_spool_fwd")
    return out, idx


def spool_bwd(idx, dout, in_shape, scale=None):
    _chk(idx)
    _chk_f32(dout, *([] if scale is None else [scale]))
    _same(idx, dout, "spool_bwd")
    dx = torch.empty(tuple(in_shape), device=dout.device, dtype=torch.float32)
    N, H, W = _planes(dx, "spool_bwd")
    if tuple(dout.shape) != tuple(in_shape[:-2]) + (spool_out(H), spool_out(W)):
        raise RuntimeError(f"spool_bwd: gradient {tuple(dout.shape)} is not the pool of {tuple(in_shape)}")
    _hip.check(_hip.load().p2i_spool_bwd(_ptr(idx), _ptr(dout), _ptr(scale), _ptr(dx), N, H, W, _stream()), "p2i_spool_bwd")
    return dx


def tdm_fwd(pred_diff, true_diff, true, beta, eps, save=True):
    """Temporal-difference matching loss; returns (0-dim loss, coef, idx) -- the backward pass is spool_bwd(idx, coef, ., gout)."""
    _chk_f32(pred_diff, true_diff, true)
    _same(pred_diff, true_diff, "tdm_fwd")
    if pred_diff.dim() != 4 or pred_diff.numel() == 0:
        raise RuntimeError(f"tdm_fwd: needs non-empty [B, T-1, H, W] differences, got {tuple(pred_diff.shape)}")
    B, Tm1, H, W = pred_diff.shape
    if tuple(true.shape) != (B, Tm1 + 1, H, W):
        raise RuntimeError(f"tdm_fwd: true {tuple(true.shape)} is not [B, T, H, W] for differences {tuple(pred_diff.shape)}")
    det_ready(pred_diff.device)
    out = torch.empty((), device=pred_diff.device, dtype=torch.float32)
    oshape = (B, Tm1, spool_out(H), spool_out(W))
    coef = torch.empty(oshape, device=out.device, dtype=torch.float32) if save else None
    idx = torch.empty(oshape, device=out.device, dtype=torch.int32) if save else None
    _hip.check(_hip.load().p2i_tdm_fwd(_ptr(pred_diff), _ptr(true_diff), _ptr(true), float(beta), float(eps), _ptr(out), _ptr(coef),
                                       _ptr(idx), B, Tm1, H, W, _stream()), "p2i_tdm_fwd")
    return out, coef, idx


def _shock_dims(x, pool, border, what):
    if x.dim() != 4 or x.numel() == 0:
        raise RuntimeError(f"{what}: needs a non-empty [B, T, H, W] tensor, got {tuple(x.shape)}")
    B, T, H, W = x.shape
    if pool < 1 or border < 0:
        raise ValueError(f"{what}: pool >= 1 and border_ignore >= 0")
    Hp, Wp = (H // pool, W // pool) if pool > 1 else (H, W)
    if Hp < 2 or Wp < 2:
        raise RuntimeError(f"{what}: the reflect padding of 1 needs a (pooled) height and width of at least 2, got {Hp} x {Wp}")
    if Hp - 2 * border < 1 or Wp - 2 * border < 1:
        raise ValueError(f"{what}: border_ignore={border} leaves nothing of a {Hp} x {Wp} map")
    if B * T > 65535:
        raise RuntimeError(f"{what}: at most 65535 planes")
    return B, T, H, W, Hp, Wp


def shock_map_fwd(x, beta, eps):
    _chk_f32(x)
    B, T, H, W, _, _ = _shock_dims(x, 1, 0, "shock_map")
    out = torch.empty_like(x)
    _hip.check(_hip.load().p2i_shock_map_fwd(_ptr(x), _ptr(out), B * T, H, W, float(beta), float(eps), _stream()), "p2i_shock_map_fwd")
    return out


def shock_map_bwd(x, dout, beta, eps):
    _chk_f32(x, dout)
    _same(x, dout, "shock_map_bwd")
    B, T, H, W, _, _ = _shock_dims(x, 1, 0, "shock_map")
    dx = torch.empty_like(x)
    scratch = torch.empty(3 * x.numel(), device=x.device, dtype=torch.float32)
    _hip.check(_hip.load().p2i_shock_map_bwd(_ptr(x), _ptr(dout), _ptr(dx), _ptr(scratch), B * T, H, W, float(beta), float(eps),
                                             _stream()), "p2i_shock_map_bwd")
    return dx


def shock_loss_fwd(pred, true, beta, pool, border, eps):
    """relu(|shock(P true)| - |shock(P pred)|) cropped by `border`: [B, T, Hp - 2 border, Wp - 2 border]."""
    _chk_f32(pred, true)
    _same(pred, true, "shock_loss_fwd")
    B, T, H, W, Hp, Wp = _shock_dims(pred, pool, border, "shock_map_loss")
    out = torch.empty((B, T, Hp - 2 * border, Wp - 2 * border), device=pred.device, dtype=torch.float32)
    _hip.check(_hip.load().p2i_shock_loss_fwd(_ptr(pred), _ptr(true), _ptr(out), B * T, H, W, int(pool), int(border), float(beta),
                                              float(eps), _stream()), "p2i_shock_loss_fwd")
    return out


def shock_loss_bwd(pred, true, dout, beta, pool, border, eps):
    _chk_f32(pred, true, dout)
    B, T, H, W, Hp, Wp = _shock_dims(pred, pool, border, "shock_map_loss")
    if tuple(dout.shape) != (B, T, Hp - 2 * border, Wp - 2 * border):
        raise RuntimeError(f"shock_loss_bwd: gradient {tuple(dout.shape)} does not match the loss tensor")
    dpred = torch.empty_like(pred)
    scratch = torch.empty(3 * B * T * Hp * Wp, device=pred.device, dtype=torch.float32)
    _hip.check(_hip.load().p2i_shock_loss_bwd(_ptr(pred), _ptr(true), _ptr(dout), _ptr(dpred), _ptr(scratch), B * T, H, W, int(pool),
                                              int(border), float(beta), float(eps), _stream()), "p2i_shock_loss_bwd")
    return dpred


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step):
    lib = _hip.load()
    n = p.numel()
    if not (g.numel() == n and m.numel() == n and v.numel() == n):
        raise RuntimeError("adam_step: buffer size mismatch")
    _chk(p, g, m, v)
    _hip.check(lib.p2i_adam(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, lr, beta1, beta2, eps, step, _stream()), "p2i_adam")


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, step_dev, coef):
    """Adam with the step counter on the device (int32 tensor, incremented by the call): capturable in a hipGraph."""
    lib = _hip.load()
    n = p.numel()
    if not (g.numel() == n and m.numel() == n and v.numel() == n) or step_dev.dtype != torch.int32 or coef.numel() < 2:
        raise RuntimeError("adam_step_dev: bad buffers")
    _chk(p, g, m, v, step_dev, coef)
    _hip.check(lib.p2i_adam_dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, lr, beta1, beta2, eps, _ptr(step_dev), _ptr(coef), _stream()),
               "p2i_adam_dev")


def axpy_(y, x, a=1.0):
    lib = _hip.load()
    if y.numel() != x.numel():
        raise RuntimeError("axpy_: size mismatch")
    _chk(y, x)
    _hip.check(lib.p2i_axpy(_ptr(y), _ptr(x), float(a), y.numel(), _stream()), "p2i_axpy")
    return y


def zero_(t):
    """t[...] = 0 (hipMemsetAsync on torch's current stream)."""
    lib = _hip.load()
    _chk(t)
    _hip.check(lib.p2i_zero(_ptr(t), t.numel(), _stream()), "p2i_zero")
    return t


def add2(a, b):
    """a + b (new tensor)."""
    lib = _hip.load()
    if a.shape != b.shape:
        raise RuntimeError("add2: shape mismatch")
    out = torch.empty_like(a)
    _chk(a, b)
    _hip.check(lib.p2i_add2(_ptr(out), _ptr(a), _ptr(b), a.numel(), _stream()), "p2i_add2")
    return out


def act_bwd(dy, y, act):
    """dy * act'(y) for the saved post-activation tensor y."""
    lib = _hip.load()
    if dy.shape != y.shape:
        raise RuntimeError("act_bwd: shape mismatch")
    out = torch.empty_like(dy)
    _chk(dy, y)
    _hip.check(lib.p2i_act_bwd(_ptr(dy), _ptr(y), act, _ptr(out), dy.numel(), _stream()), "p2i_act_bwd")
    return out


def act_bwd_bias(dy, y, act, db_out=None):
    """(dy * act'(y), its per-channel sum) in one pass; db_out: caller-owned ZEROED (C,) target the kernel adds into."""
    lib = _hip.load()
    det_ready(dy.device)
    B, Cc = dy.shape[0], dy.shape[1]
    inner = dy[0, 0].numel()
    if inner % 4:
        dz = act_bwd(dy, y, act)
        return dz, bias_grad(dz, out=db_out)
    out = torch.empty_like(dy)
    db = db_out if db_out is not None else zero_(torch.empty(Cc, device=dy.device, dtype=torch.float32))
    _chk(dy, y, db)
    _hip.check(lib.p2i_act_bwd_bias(_ptr(dy), _ptr(y), act, _ptr(out), _ptr(db), B, Cc, inner, _stream()), "p2i_act_bwd_bias")
    return out, db


def bias_grad(dy, y_act=None, act=ACT_NONE, out=None):
    """out: caller-owned ZEROED (Cc,) target the kernel adds into."""
    lib = _hip.load()
    det_ready(dy.device)
    B, Cc = dy.shape[0], dy.shape[1]
    inner = dy[0, 0].numel()
    if out is not None and out.numel() != Cc:
        raise RuntimeError("bias_grad: target size mismatch")
    db = out if out is not None else zero_(torch.empty(Cc, device=dy.device, dtype=torch.float32))
    _chk(dy, y_act)
    _hip.check(lib.p2i_bias_grad(_ptr(dy), _ptr(y_act), act, _ptr(db), B, Cc, inner, _stream()), "p2i_bias_grad")
    return db


# --------------------------------------------------------------------------- sliding-window inference
def window_gather(a, b, L, w0, nw, win, step):
    """Windows w0 .. w0+nw-1 (win frames every `step`, the last frame repeated past the end) of the (L, ...) tensors a and b
    (b may be None) as (nw, win, ...) tensors."""
    lib = _hip.load()
    hw = a[0].numel()
    wa = torch.empty((nw, win) + tuple(a.shape[1:]), device=a.device, dtype=torch.float32)
    wb = torch.empty_like(wa) if b is not None else None
    _chk(a, b)
    _hip.check(lib.p2i_window_gather(_ptr(a), _ptr(b), _ptr(wa), _ptr(wb), L, hw, w0, nw, win, step, _stream()), "p2i_window_gather")
    return wa, wb


def window_mean(pred_windows, L, win, step, scale):
    """(nwin, win, ...) predictions of all windows of an event -> (L, ...): mean over the windows that hold each frame, * scale, >= 0."""
    lib = _hip.load()
    nwin = pred_windows.shape[0]
    hw = pred_windows[0, 0].numel()
    out = torch.empty((L,) + tuple(pred_windows.shape[2:]), device=pred_windows.device, dtype=torch.float32)
    _chk(pred_windows)
    _hip.check(lib.p2i_window_mean(_ptr(pred_windows), _ptr(out), L, hw, nwin, win, step, float(scale), _stream()), "p2i_window_mean")
    return out


# --------------------------------------------------------------------------- batch assembly
def assemble_batch(frames_u8, mask_u8):
    """uint8 frames (B,T,H,W) + uint8 mask (H,W) | (T,H,W) | (B,T,H,W) -> (frames, masked, masks), each (B,T,1,H,W) fp32:
    the loader's /255, video*mask and channel permute (sti_dataset.py:209,223-224; train.py:468-473) in one pass."""
    lib = _hip.load()
    if frames_u8.dtype != torch.uint8 or mask_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
        raise RuntimeError("assemble_batch: expects uint8 frames (B,T,H,W) and a uint8 mask")
    B, T, H, W = frames_u8.shape
    if tuple(mask_u8.shape) not in ((H, W), (T, H, W), (B, T, H, W)):
        raise RuntimeError(f"assemble_batch: mask shape {tuple(mask_u8.shape)} does not match frames {tuple(frames_u8.shape)}")
    _chk(frames_u8, mask_u8)
    out = [torch.empty((B, T, 1, H, W), device=frames_u8.device, dtype=torch.float32) for _ in range(3)]
    _hip.check(lib.p2i_assemble_batch(_ptr(frames_u8), _ptr(mask_u8), mask_u8.numel(), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                      B, T, H, W, _stream()), "p2i_assemble_batch")
    return out[0], out[1], out[2]


# --------------------------------------------------------------------------- STDK baseline (csrc/stdk.hip)
STDK_K = 79          # visible points per frame (reference models/stdk.py:143-147)
STDK_HID = 100
_STDK_HP = 112


def stdk_basis(knots, theta, h, w):
    """Wendland-C2 basis phi [h*w, K] of the grid (i // w, i % w) for knots [K, 2] (y, x) and per-knot theta [K]."""
    lib = _hip.load()
    K = theta.numel()
    if knots.shape != (K, 2):
        raise RuntimeError("stdk_basis: knots must be [K, 2]")
    phi = torch.empty(h * w, K, device=theta.device, dtype=torch.float32)
    _chk(knots, theta)
    _hip.check(lib.p2i_stdk_basis(_ptr(knots), _ptr(theta), K, h, w, _ptr(phi), _stream()), "p2i_stdk_basis")
    return phi


def stdk_select(masked, mask, k=STDK_K):
    """masked, mask: (B, T, H*W) fp32.  Returns idx (B, T, k) int32 and z (B, T, k): the observed pixels in raster order, then the
    unobserved ones, first k."""
    lib = _hip.load()
    B, T, HW = masked.shape
    if mask.shape != masked.shape:
        raise RuntimeError("stdk_select: mask shape mismatch")
    if HW < k:
        raise ValueError(f"STDK needs at least {k} pixels per frame (got {HW})")
    idx = torch.empty(B, T, k, device=masked.device, dtype=torch.int32)
    z = torch.empty(B, T, k, device=masked.device, dtype=torch.float32)
    _chk(masked, mask)
    _hip.check(lib.p2i_stdk_select(_ptr(masked), _ptr(mask), B * T, HW, k, _ptr(idx), _ptr(z), _stream()), "p2i_stdk_select")
    return idx, z


def stdk_layer1_fwd(phi_s, phi_t, z, w1, b1, B, T):
    """P [HW, 112] and Q [B*T, 112] of the decomposed first layer (columns >= 100 zero)."""
    lib = _hip.load()
    HW, Ks = phi_s.shape
    Kt, Kz = phi_t.shape[1], z.shape[1]
    if phi_t.shape[0] != T or z.shape[0] != B or w1.shape != (STDK_HID, Ks + Kt + Kz) or b1.numel() != STDK_HID:
        raise RuntimeError("stdk_layer1_fwd: shape mismatch")
    dev = phi_s.device
    P = torch.empty(HW, _STDK_HP, device=dev, dtype=torch.float32)
    Q = torch.empty(B * T, _STDK_HP, device=dev, dtype=torch.float32)
    zt = torch.empty(T, _STDK_HP, device=dev, dtype=torch.float32)
    zb = torch.empty(B, _STDK_HP, device=dev, dtype=torch.float32)
    _chk(phi_s, phi_t, z, w1, b1)
    _hip.check(lib.p2i_stdk_layer1_fwd(_ptr(phi_s), _ptr(phi_t), _ptr(z), _ptr(w1), _ptr(b1), B, T, HW, Ks, Kt, Kz, _ptr(P), _ptr(zt),
                                       _ptr(zb), _ptr(Q), _stream()), "p2i_stdk_layer1_fwd")
    return P, Q


def _stdk_mlp_check(P, Q, w2, b2, w3, b3, w4):
    if P.shape[1] != _STDK_HP or Q.shape[1] != _STDK_HP or w2.shape != (STDK_HID, STDK_HID) or w3.shape != (STDK_HID, STDK_HID) \
            or w4.numel() != STDK_HID or b2.numel() != STDK_HID or b3.numel() != STDK_HID:
        raise RuntimeError("stdk MLP: shape mismatch")


def stdk_mlp_fwd(P, Q, w2, b2, w3, b3, w4, b4):
    """y [B*T, HW] of the fused layers 2..4 over every row (b, t, p)."""
    lib = _hip.load()
    _stdk_mlp_check(P, Q, w2, b2, w3, b3, w4)
    HW, BT = P.shape[0], Q.shape[0]
    y = torch.empty(BT, HW, device=P.device, dtype=torch.float32)
    _chk(P, Q, w2, b2, w3, b3, w4, b4)
    _hip.check(lib.p2i_stdk_mlp_fwd(_ptr(P), _ptr(Q), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(w4), _ptr(b4), HW, BT, _ptr(y),
                                    _stream()), "p2i_stdk_mlp_fwd")
    return y


def stdk_mlp_bwd(P, Q, w2, b2, w3, b3, w4, dy, grads=None):
    """dy [B*T, HW] -> dP [HW, 100], dQ [B*T, 100] and (dw2, db2, dw3, db3, dw4, db4) (written into `grads` when given)."""
    import ctypes
    lib = _hip.load()
    _stdk_mlp_check(P, Q, w2, b2, w3, b3, w4)
    HW, BT = P.shape[0], Q.shape[0]
    if dy.shape != (BT, HW):
        raise RuntimeError("stdk_mlp_bwd: dy shape mismatch")
    sz = (ctypes.c_int64 * 4)()
    _hip.check(lib.p2i_stdk_bwd_workspace(HW, BT, sz), "p2i_stdk_bwd_workspace")
    dev = P.device
    ws = [torch.empty(int(n), device=dev, dtype=torch.float32) for n in sz]
    dP = torch.empty(HW, STDK_HID, device=dev, dtype=torch.float32)
    dQ = torch.empty(BT, STDK_HID, device=dev, dtype=torch.float32)
    g = list(grads) if grads is not None else [torch.empty_like(t) for t in (w2, b2, w3, b3, w4)] + [torch.empty(1, device=dev)]
    _chk(P, Q, w2, b2, w3, b3, w4, dy, *g)
    _hip.check(lib.p2i_stdk_mlp_bwd(_ptr(P), _ptr(Q), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(w4), _ptr(dy), HW, BT,
                                    *[_ptr(t) for t in ws], _ptr(dP), _ptr(dQ), *[_ptr(t) for t in g], _stream()), "p2i_stdk_mlp_bwd")
    return dP, dQ, g


def stdk_layer1_bwd(phi_s, phi_t, z, dP, dQ, B, T, dw1=None, db1=None):
    """dw1 [100, F], db1 [100] of the decomposed first layer (fixed-order sums)."""
    lib = _hip.load()
    HW, Ks = phi_s.shape
    Kt, Kz = phi_t.shape[1], z.shape[1]
    dev = phi_s.device
    if dP.shape != (HW, STDK_HID) or dQ.shape != (B * T, STDK_HID):
        raise RuntimeError("stdk_layer1_bwd: shape mismatch")
    F = Ks + Kt + Kz
    splits = max(1, min(64, HW // 256))
    dw1 = torch.empty(STDK_HID, F, device=dev, dtype=torch.float32) if dw1 is None else dw1
    db1 = torch.empty(STDK_HID, device=dev, dtype=torch.float32) if db1 is None else db1
    dqt = torch.empty(T, STDK_HID, device=dev, dtype=torch.float32)
    dqb = torch.empty(B, STDK_HID, device=dev, dtype=torch.float32)
    part = torch.empty(splits * STDK_HID * F, device=dev, dtype=torch.float32)
    _chk(phi_s, phi_t, z, dP, dQ, dw1, db1)
    _hip.check(lib.p2i_stdk_layer1_bwd(_ptr(phi_s), _ptr(phi_t), _ptr(z), _ptr(dP), _ptr(dQ), B, T, HW, Ks, Kt, Kz, _ptr(dqt), _ptr(dqb),
                                       _ptr(part), splits, _ptr(dw1), _ptr(db1), _stream()), "p2i_stdk_layer1_bwd")
    return dw1, db1


# --------------------------------------------------------------------------- classical baselines (csrc/classical.hip)
KRIG_TILE = 32           # systems and per-gauge rows are padded to a multiple of this
KRIG_MAX_CAP = 4096
KRIG_MAX_LAGS = 32
KRIG_CANDIDATES = 25
KRIG_BIN_CHUNKS = 8      # workgroups per frame of the variogram pass (a fixed number: the partials are added in order)
KRIG_MODELS = {"exponential": 0, "spherical": 1}


def _krig_t(what, t, dtype, shape=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
        raise RuntimeError(f"{what}: contiguous CUDA tensors only (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{what}: expected {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _krig_sys(what, f0, R, T, nsys, F, np_, cap):
    if not (R == 1 or (R == T and f0 % T == 0)) or f0 < 0 or nsys < 1 or f0 + nsys * R > F:
        raise RuntimeError(f"{what}: systems {f0} + {nsys} x {R} do not fit {F} frames of {T}-frame samples")
    if np_ < KRIG_TILE or np_ % KRIG_TILE or np_ > cap:
        raise RuntimeError(f"{what}: padded size {np_} must be a multiple of {KRIG_TILE} within cap {cap}")


def _krig_cap(what, cap, ok=True):
    if not ok or cap < KRIG_TILE or cap % KRIG_TILE or cap > KRIG_MAX_CAP:
        raise ValueError(f"{what}: cap must be a multiple of {KRIG_TILE} in [{KRIG_TILE}, {KRIG_MAX_CAP}] (got {cap})")


def _krig_ws(what, ws, nsys, np_, kind="factor"):
    if ws.numel() < nsys * np_ * np_:
        raise RuntimeError(f"{what}: {kind} workspace too small")


def krig_compact(masked, mask, cap):
    """masked, mask: (B, T, H, W) fp32.  Returns pix (B*T, cap) int32 ((y << 16) | x of the frame's mask != 0 pixels in raster order),
    z (B*T, cap) (masked there; both zero past the count) and info (2*B*T,) int32: counts, then 'mask differs from the sample's
    first frame' flags."""
    lib = _hip.load()
    _krig_t("krig_compact", masked, torch.float32)
    _krig_t("krig_compact", mask, torch.float32, masked.shape)
    if masked.dim() != 4:
        raise RuntimeError("krig_compact: (B, T, H, W) expected")
    _krig_cap("krig_compact", cap)
    B, T, H, W = masked.shape
    F = B * T
    pix = torch.empty(F, cap, device=masked.device, dtype=torch.int32)
    z = torch.empty(F, cap, device=masked.device, dtype=torch.float32)
    info = torch.empty(2 * F, device=masked.device, dtype=torch.int32)
    _hip.check(lib.p2i_krig_compact(_ptr(masked), _ptr(mask), B, T, H, W, cap, _ptr(pix), _ptr(z), _ptr(info), _stream()),
               "p2i_krig_compact")
    return pix, z, info


def krig_variogram(pix, z, info, B, T, n_lags, lag_width, model):
    """Empirical variogram pooled per sample and its fit, fp64 on the device.  Returns bins (B, n_lags, 3) fp64 (pairs, sum of
    semivariances, sum of distances), fit (B, 4) fp64 (nugget, psill, range, weighted SSE), cand (B,) int32 (-1: degenerate sample)
    and params (B, 4) fp32 for the kriging calls."""
    lib = _hip.load()
    F = B * T
    cap = pix.shape[1]
    _krig_t("krig_variogram", pix, torch.int32, (F, cap))
    _krig_t("krig_variogram", z, torch.float32, (F, cap))
    _krig_t("krig_variogram", info, torch.int32, (2 * F,))
    if not (1 <= n_lags <= KRIG_MAX_LAGS) or not lag_width > 0:
        raise ValueError(f"krig_variogram: n_lags must be 1..{KRIG_MAX_LAGS} and the lag width positive")
    dev = pix.device
    part = torch.empty(F, KRIG_BIN_CHUNKS, n_lags, 3, device=dev, dtype=torch.float64)
    bins = torch.empty(B, n_lags, 3, device=dev, dtype=torch.float64)
    fit = torch.empty(B, 4, device=dev, dtype=torch.float64)
    cand = torch.empty(B, device=dev, dtype=torch.int32)
    params = torch.empty(B, 4, device=dev, dtype=torch.float32)
    _hip.check(lib.p2i_krig_bins(_ptr(pix), _ptr(z), _ptr(info), F, cap, KRIG_BIN_CHUNKS, n_lags, float(lag_width), _ptr(part), _stream()),
               "p2i_krig_bins")
    _hip.check(lib.p2i_krig_fit(_ptr(part), B, T * KRIG_BIN_CHUNKS, n_lags, float(lag_width), int(model), _ptr(bins), _ptr(fit), _ptr(cand),
                                _ptr(params), _stream()), "p2i_krig_fit")
    return bins, fit, cand, params


class KrigSystems:
    """The systems of one call, stated once for the nine dense stages (p2i_krig_systems of include/p2i_hip.h): pix, z (rows, cap) and
    info (2 * rows,) as krig_compact packs them (or stkrig_gather's stpix, stz, stinfo: the samples stand in for frames, R = T = 1),
    params (rows // T, 4), cand (rows // T,) int32 or None, status (rows // R,) int32 (zeroed by the caller): one entry per system,
    system s being the gauge set of row s * R padded to np_.  Every tensor is checked here, once; chunk() only cuts a range."""

    def __init__(self, pix, z, info, params, cand, model, R, T, np_, status):
        who = "KrigSystems"
        F, cap = _krig_t(who, pix, torch.int32, (pix.shape[0], pix.shape[-1])).shape
        _krig_cap(who, cap)
        _krig_sys(who, 0, R, T, F // max(R, 1), F, np_, cap)
        _krig_t(who, z, torch.float32, (F, cap))
        _krig_t(who, info, torch.int32, (2 * F,))
        _krig_t(who, params, torch.float32, (F // T, 4))
        if cand is not None:
            _krig_t(who, cand, torch.int32, (F // T,))
        _krig_t(who, status, torch.int32, (F // R,))
        self.pix, self.z, self.info, self.params, self.cand, self.status = pix, z, info, params, cand, status
        self.model, self.R, self.T, self.np_, self.F, self.cap = int(model), R, T, np_, F, cap

    def chunk(self, s0, ns):
        """The descriptor of systems s0 .. s0 + ns - 1: f0 = s0 * R and their slice of status."""
        if s0 < 0 or ns < 1 or s0 + ns > self.status.numel():
            raise RuntimeError(f"KrigSystems.chunk: systems {s0} + {ns} are not among the call's {self.status.numel()}")
        return KrigChunk(self, s0, ns)


class KrigChunk:
    """Systems s0 .. s0 + ns - 1 of `of` (a KrigSystems): status is their slice, c the _hip.KrigSystems that the stages take."""

    def __init__(self, of, s0, ns):
        self.of, self.s0, self.ns, self.status = of, s0, ns, of.status[s0:s0 + ns]
        self.c = _hip.KrigSystems(_ptr(of.pix), _ptr(of.z), _ptr(of.info), _ptr(of.params), _ptr(of.cand), _ptr(self.status), of.model,
                                  s0 * of.R, of.R, of.T, ns, of.np_, of.cap)

    def call(self, name, *args):
        _hip.check(getattr(_hip.load(), name)(C.byref(self.c), *args, _stream()), name)


def krig_factor(sys, L):
    """Cholesky factors of the chunk's systems into L (>= nsys * np_ * np_ fp32); its status is set where a pivot was not positive."""
    _krig_t("krig_factor", L, torch.float32)
    _krig_ws("krig_factor", L, sys.ns, sys.of.np_)
    sys.call("p2i_krig_factor", _ptr(L))


def krig_solve(sys, L, alpha, mean):
    """Dual coefficients alpha (F, cap) and mean (F,) of the frames of the chunk's factored systems (written in place).  Returns the
    fp64 solutions sol (nsys, R + 1, np_): row 0 is u = K^-1 1, row 1 + t is K^-1 z of the system's frame t."""
    of = sys.of
    _krig_t("krig_solve", L, torch.float32)
    _krig_t("krig_solve", alpha, torch.float32, (of.F, of.cap))
    _krig_t("krig_solve", mean, torch.float32, (of.F,))
    _krig_ws("krig_solve", L, sys.ns, of.np_)
    sol = torch.empty(sys.ns, of.R + 1, of.np_, device=of.z.device, dtype=torch.float64)
    sys.call("p2i_krig_solve", _ptr(L), _ptr(sol), _ptr(alpha), _ptr(mean))
    return sol


def krig_predict(sys, alpha, mean, H, W, out=None):
    """out (F, H*W) = mean + sum_i alpha_i c0(p, x_i) for the frames of the chunk's sets (a new tensor unless given; the other frames
    are left as they are); R = T: the frames of a sample share frame 0's gauges."""
    of = sys.of
    _krig_t("krig_predict", alpha, torch.float32, (of.F, of.cap))
    _krig_t("krig_predict", mean, torch.float32, (of.F,))
    if out is None:
        out = torch.empty(of.F, H * W, device=of.pix.device, dtype=torch.float32)
    _krig_t("krig_predict", out, torch.float32, (of.F, H * W))
    sys.call("p2i_krig_predict", _ptr(alpha), _ptr(mean), H, W, _ptr(out))
    return out


def idw_all(pix, z, info, H, W, power=2.0):
    """out (F, H*W): inverse-distance weighting over ALL gauges of each frame (the gauge's value on a gauge pixel, 0 without gauges)."""
    lib = _hip.load()
    F, cap = pix.shape
    _krig_t("idw_all", pix, torch.int32)
    _krig_t("idw_all", z, torch.float32, (F, cap))
    _krig_t("idw_all", info, torch.int32, (2 * F,))
    if not power > 0:
        raise ValueError("idw_all: power must be positive")
    out = torch.empty(F, H * W, device=pix.device, dtype=torch.float32)
    _hip.check(lib.p2i_idw_all(_ptr(pix), _ptr(z), _ptr(info), F, H, W, cap, float(power), _ptr(out), _stream()), "p2i_idw_all")
    return out


# ---- space-time ordinary kriging (csrc/stkrig.hip)
STKRIG_MAX_TLAGS = 7
STKRIG_KAPPAS = 17       # anisotropy candidates kappa_q = 2^((q - 6) / 2) px / frame; candidate index = q * KRIG_CANDIDATES + c
STKRIG_BIN_CHUNKS = 16   # workgroups per (sample, temporal lag) of the variogram pass (fixed: the partials are added in order)


def stkrig_gather(pix, z, info, B, T, cap):
    """The per-frame gauges of krig_compact as per-sample space-time point sets, frame-major: stpix, stt (frame index), stz (B, cap)
    (zero past the count) and stinfo (2*B,) int32 whose first B entries are the samples' point counts (the rest is zero, so that it
    stands in for krig_compact's info in krig_solve)."""
    lib = _hip.load()
    F = B * T
    fcap = pix.shape[1]
    _krig_t("stkrig_gather", pix, torch.int32, (F, fcap))
    _krig_t("stkrig_gather", z, torch.float32, (F, fcap))
    _krig_t("stkrig_gather", info, torch.int32, (2 * F,))
    _krig_cap("stkrig_gather", cap)
    dev = pix.device
    stpix = torch.empty(B, cap, device=dev, dtype=torch.int32)
    stt = torch.empty(B, cap, device=dev, dtype=torch.int32)
    stz = torch.empty(B, cap, device=dev, dtype=torch.float32)
    stinfo = torch.zeros(2 * B, device=dev, dtype=torch.int32)
    _hip.check(lib.p2i_stkrig_gather(_ptr(pix), _ptr(z), _ptr(info), B, T, fcap, cap, _ptr(stpix), _ptr(stt), _ptr(stz), _ptr(stinfo),
                                     _stream()), "p2i_stkrig_gather")
    return stpix, stt, stz, stinfo


def stkrig_variogram(pix, z, info, B, T, n_lags, n_tlags, lag_width, model, vel=None, who="stkrig_variogram"):
    """Space-time empirical variogram per sample and its (kappa, range) candidate fit, fp64 on the device.  Returns bins (B, n_tlags + 1,
    n_lags, 3) fp64 (pairs, sum of semivariances, sum of spatial distances), fit (B, 5) fp64 (nugget, psill, range, kappa, weighted
    SSE), cand (B,) int32 (q * 25 + c; -1: degenerate sample) and params (B, 4) fp32 (nugget, psill, range, kappa).
    vel (B, 2) fp64 = (v_y, v_x) per sample: the pairs of temporal lag u are binned by the advected spatial distance |x_j - x_i - v u|
    (DESIGN.md section 19); with vel = 0 the bins are those without it bit for bit.  who: the name that errors report."""
    lib = _hip.load()
    F = B * T
    cap = pix.shape[1]
    _krig_t(who, pix, torch.int32, (F, cap))
    _krig_t(who, z, torch.float32, (F, cap))
    _krig_t(who, info, torch.int32, (2 * F,))
    if vel is not None:
        _lag_vel(who, vel, torch.float64, B)
    if not (1 <= n_lags <= KRIG_MAX_LAGS) or not lag_width > 0:
        raise ValueError(f"{who}: n_lags must be 1..{KRIG_MAX_LAGS} and the lag width positive")
    if not (0 <= n_tlags <= STKRIG_MAX_TLAGS and n_tlags < T):
        raise ValueError(f"{who}: n_tlags must be 0..{STKRIG_MAX_TLAGS} and below T = {T} (got {n_tlags})")
    dev = pix.device
    part = torch.empty(B, n_tlags + 1, STKRIG_BIN_CHUNKS, n_lags, 3, device=dev, dtype=torch.float64)
    bins = torch.empty(B, n_tlags + 1, n_lags, 3, device=dev, dtype=torch.float64)
    fit = torch.empty(B, 5, device=dev, dtype=torch.float64)
    cand = torch.empty(B, device=dev, dtype=torch.int32)
    params = torch.empty(B, 4, device=dev, dtype=torch.float32)
    _hip.check(lib.p2i_stkrig_bins(_ptr(pix), _ptr(z), _ptr(info), _ptr(vel), B, T, cap, STKRIG_BIN_CHUNKS, n_lags, n_tlags,
                                   float(lag_width), _ptr(part), _stream()), "p2i_stkrig_bins")
    _hip.check(lib.p2i_stkrig_fit(_ptr(part), B, STKRIG_BIN_CHUNKS, n_lags, n_tlags, float(lag_width), int(model), _ptr(bins), _ptr(fit),
                                  _ptr(cand), _ptr(params), _stream()), "p2i_stkrig_fit")
    return bins, fit, cand, params


def stkrig_factor(sys, stt, L, velf=None, who="stkrig_factor"):
    """Cholesky factors of the space-time covariance systems of the chunk's samples (sys: stpix, stz, stinfo with R = T = 1) into L
    (>= nsys * np_ * np_ fp32); the chunk's status is set where a pivot was not positive.  stt (B, cap): the points' frames; velf
    (B, 2) fp32 = (v_y, v_x) per sample: the Lagrangian distance.  who: the name that errors report."""
    of = sys.of
    _krig_t(who, stt, torch.int32, (of.F, of.cap))
    _krig_t(who, L, torch.float32)
    _krig_ws(who, L, sys.ns, of.np_)
    if velf is not None:
        _lag_vel(who, velf, torch.float32, of.F)
    sys.call("p2i_stkrig_factor", _ptr(stt), _ptr(velf), _ptr(L))


def stkrig_predict(stpix, stt, alpha, mean, stinfo, params, model, T, H, W, velf=None, who="stkrig_predict"):
    """out (B, T, H*W) = mean_b + sum_i alpha_i c0((t, p), i) over the sample's space-time points.  velf, who: as in stkrig_factor."""
    lib = _hip.load()
    B, cap = stpix.shape
    _krig_t(who, stpix, torch.int32)
    _krig_t(who, stt, torch.int32, (B, cap))
    _krig_t(who, alpha, torch.float32, (B, cap))
    _krig_t(who, mean, torch.float32, (B,))
    _krig_t(who, stinfo, torch.int32, (2 * B,))
    _krig_t(who, params, torch.float32, (B, 4))
    if T < 1 or H < 1 or W < 1 or cap % KRIG_TILE or cap > KRIG_MAX_CAP:
        raise RuntimeError(f"{who}: bad shape T {T}, {H} x {W}, cap {cap}")
    out = torch.empty(B, T, H * W, device=stpix.device, dtype=torch.float32)
    if velf is not None:
        _lag_vel(who, velf, torch.float32, B)
    _hip.check(lib.p2i_stkrig_predict(_ptr(stpix), _ptr(stt), _ptr(alpha), _ptr(mean), _ptr(stinfo), _ptr(params), _ptr(velf), int(model),
                                      B, T, H, W, cap, _ptr(out), _stream()), "p2i_stkrig_predict")
    return out


# ---- leave-one-site-out cross-validation of space-time kriging (csrc/stkrig_loso.hip)
def stkrig_gather_sites(pix, z, info, B, T, cap):
    """The per-frame gauges of krig_compact as per-sample point sets sorted by (pixel, frame), so that a site (the points of one
    pixel) is a contiguous run.  Returns a dict: stpix, stt, stz (B, cap) and stinfo (2*B,) as stkrig_gather returns them, site_start
    (B, cap + 1) int32 (first point of each site; the point count from entry nsites[b] on), nsites (B,), psite (B, cap) (site of a
    sorted point, -1 past the count), back (B, cap) (t * fcap + rank in frame t, -1 past the count) and fsite (B*T, fcap) (site of
    a frame's gauge in krig_compact's layout, -1 past the frame's count)."""
    lib = _hip.load()
    F = B * T
    fcap = pix.shape[1]
    _krig_t("stkrig_gather_sites", pix, torch.int32, (F, fcap))
    _krig_t("stkrig_gather_sites", z, torch.float32, (F, fcap))
    _krig_t("stkrig_gather_sites", info, torch.int32, (2 * F,))
    _krig_cap("stkrig_gather_sites", cap, fcap <= KRIG_MAX_CAP)
    dev = pix.device
    out = {k: torch.empty(B, cap, device=dev, dtype=torch.int32) for k in ("stpix", "stt", "psite", "back")}
    out["stz"] = torch.empty(B, cap, device=dev, dtype=torch.float32)
    out["stinfo"] = torch.zeros(2 * B, device=dev, dtype=torch.int32)
    out["site_start"] = torch.empty(B, cap + 1, device=dev, dtype=torch.int32)
    out["nsites"] = torch.empty(B, device=dev, dtype=torch.int32)
    out["fsite"] = torch.empty(F, fcap, device=dev, dtype=torch.int32)
    _hip.check(lib.p2i_stkrig_gather_sites(_ptr(pix), _ptr(z), _ptr(info), B, T, fcap, cap, _ptr(out["stpix"]), _ptr(out["stt"]),
                                           _ptr(out["stz"]), _ptr(out["stinfo"]), _ptr(out["site_start"]), _ptr(out["nsites"]),
                                           _ptr(out["psite"]), _ptr(out["back"]), _ptr(out["fsite"]), _stream()), "p2i_stkrig_gather_sites")
    return out


def stkrig_site_gram(Winv, nsys, np_):
    """gram (nsys, np_ / 32, 2, 32, 32) fp64: per column tile J the tiles (J, J) and (J + 1, J) of Winv^T Winv, the band that holds
    every run of at most 32 consecutive columns."""
    lib = _hip.load()
    _krig_t("stkrig_site_gram", Winv, torch.float32)
    if nsys < 1 or np_ < KRIG_TILE or np_ % KRIG_TILE or np_ > KRIG_MAX_CAP:
        raise RuntimeError(f"stkrig_site_gram: bad system shape {nsys} x {np_}")
    _krig_ws("stkrig_site_gram", Winv, nsys, np_, "inverse")
    gram = torch.empty(nsys, np_ // KRIG_TILE, 2, KRIG_TILE, KRIG_TILE, device=Winv.device, dtype=torch.float64)
    _hip.check(lib.p2i_stkrig_site_gram(_ptr(Winv), nsys, np_, _ptr(gram), _stream()), "p2i_stkrig_site_gram")
    return gram


def stkrig_loso(sys, gram, sol, alpha, sites, T, pred, var):
    """Leave-one-site-out prediction and variance of every point of the chunk's samples into pred, var (B*T, fcap), in place, at the
    points only (the caller zeroes both).  sys: the systems of stkrig_gather_sites' dict `sites` (stpix, stz, stinfo, R = T = 1); gram,
    sol, alpha as stkrig_site_gram and krig_solve leave them for the same chunk; T: frames per sample."""
    of, ns = sys.of, sys.ns
    B, cap = of.F, of.cap
    F, fcap = pred.shape
    if not 1 <= T <= KRIG_TILE or F != B * T:
        raise ValueError(f"stkrig_loso: a site block is at most {KRIG_TILE} frames wide (got T = {T}, {F} frames of {B} samples)")
    _krig_t("stkrig_loso", gram, torch.float64, (ns, of.np_ // KRIG_TILE, 2, KRIG_TILE, KRIG_TILE))
    _krig_t("stkrig_loso", sol, torch.float64, (ns, 2, of.np_))
    _krig_t("stkrig_loso", alpha, torch.float32, (B, cap))
    for key, shape in (("site_start", (B, cap + 1)), ("nsites", (B,)), ("back", (B, cap))):
        _krig_t("stkrig_loso", sites[key], torch.int32, shape)
    _krig_t("stkrig_loso", pred, torch.float32)
    _krig_t("stkrig_loso", var, torch.float32, (F, fcap))
    if fcap > KRIG_MAX_CAP:
        raise RuntimeError(f"stkrig_loso: frame rows of {fcap} exceed {KRIG_MAX_CAP}")
    sys.call("p2i_stkrig_loso", _ptr(gram), _ptr(sol), _ptr(alpha), _ptr(sites["site_start"]), _ptr(sites["nsites"]), _ptr(sites["back"]),
             T, fcap, _ptr(pred), _ptr(var))


# ---- Lagrangian space-time kriging (the velocity: csrc/lagkrig.hip; the rest: csrc/stkrig.hip with a velocity)
LAGKRIG_MAX_VHALF = 16                                   # candidate velocities (i s, j s), |i|, |j| <= nhalf <= 16
LAGKRIG_MAX_CANDIDATES = (2 * LAGKRIG_MAX_VHALF + 1) ** 2   # 33 x 33 = 1089: the largest grid the velocity kernels take
LAGKRIG_VEL_CHUNKS = 32                                  # workgroups per (sample, candidate block) of the velocity pass (fixed: added in order)


def _lag_vel(who, vel, dtype, B):
    return _krig_t(who, vel, dtype, (B, 2))


def lagkrig_velocity(pix, z, info, B, T, n_tlags, nhalf, vstep, bandwidth):
    """The advection velocity of every sample from its gauges: over the (2 nhalf + 1)^2 candidates v = (i, j) vstep (px / frame) and the
    pairs (gauge a in frame t, gauge b in frame t + u), 1 <= u <= n_tlags, with w = exp(-|x_b - x_a - v u|^2 / (2 bandwidth^2)):
    weight = sum w, score = sum w (z_a - z_b)^2 / 2 / weight (+inf where the weight is 0), support = sum w over the pairs of distinct
    pixels.  The estimate is the candidate of the smallest score among those with support >= support(v = 0) / 2; ties go to the
    smaller |v|^2, then to the lower index.  fp64 on the device.  Returns score, weight, support (B, n, n) fp64 (n = 2 nhalf + 1,
    [i + nhalf][j + nhalf]), vel (B, 2) fp64 = (v_y, v_x), velf its fp32 copy and vcand (B,) int32 = (i + nhalf) n + (j + nhalf)."""
    lib = _hip.load()
    F = B * T
    cap = pix.shape[1]
    _krig_t("lagkrig_velocity", pix, torch.int32, (F, cap))
    _krig_t("lagkrig_velocity", z, torch.float32, (F, cap))
    _krig_t("lagkrig_velocity", info, torch.int32, (2 * F,))
    if not (0 <= n_tlags <= STKRIG_MAX_TLAGS and n_tlags < T):
        raise ValueError(f"lagkrig_velocity: n_tlags must be 0..{STKRIG_MAX_TLAGS} and below T = {T} (got {n_tlags})")
    if not 0 <= nhalf <= LAGKRIG_MAX_VHALF:
        raise ValueError(f"lagkrig_velocity: at most {LAGKRIG_MAX_CANDIDATES} candidates, nhalf <= {LAGKRIG_MAX_VHALF} (got {nhalf})")
    if not (vstep > 0 and bandwidth > 0):
        raise ValueError("lagkrig_velocity: the velocity step and the bandwidth must be positive")
    dev = pix.device
    n = 2 * nhalf + 1
    part = torch.empty(B, LAGKRIG_VEL_CHUNKS, n * n, 3, device=dev, dtype=torch.float64)
    score = torch.empty(B, n, n, device=dev, dtype=torch.float64)
    weight = torch.empty(B, n, n, device=dev, dtype=torch.float64)
    support = torch.empty(B, n, n, device=dev, dtype=torch.float64)
    vel = torch.empty(B, 2, device=dev, dtype=torch.float64)
    velf = torch.empty(B, 2, device=dev, dtype=torch.float32)
    vcand = torch.empty(B, device=dev, dtype=torch.int32)
    _hip.check(lib.p2i_lagkrig_velocity(_ptr(pix), _ptr(z), _ptr(info), B, T, cap, LAGKRIG_VEL_CHUNKS, n_tlags, nhalf, float(vstep),
                                        float(bandwidth), _ptr(part), _stream()), "p2i_lagkrig_velocity")
    _hip.check(lib.p2i_lagkrig_pick(_ptr(part), B, LAGKRIG_VEL_CHUNKS, nhalf, float(vstep), _ptr(score), _ptr(weight), _ptr(support), _ptr(vel),
                                    _ptr(velf), _ptr(vcand), _stream()), "p2i_lagkrig_pick")
    return score, weight, support, vel, velf, vcand


def lagkrig_variogram(pix, z, info, vel, B, T, n_lags, n_tlags, lag_width, model):
    """stkrig_variogram with a velocity that must be there: vel (B, 2) fp64."""
    return stkrig_variogram(pix, z, info, B, T, n_lags, n_tlags, lag_width, model, _lag_vel("lagkrig_variogram", vel, torch.float64, B),
                            "lagkrig_variogram")


def lagkrig_factor(sys, stt, velf, L):
    """stkrig_factor with a velocity that must be there: velf (B, 2) fp32 = (v_y, v_x) per sample."""
    return stkrig_factor(sys, stt, L, _lag_vel("lagkrig_factor", velf, torch.float32, sys.of.F), "lagkrig_factor")


def lagkrig_predict(stpix, stt, alpha, mean, stinfo, params, velf, model, T, H, W):
    """stkrig_predict with a velocity that must be there: out (B, T, H*W), Lagrangian distance."""
    return stkrig_predict(stpix, stt, alpha, mean, stinfo, params, model, T, H, W,
                          _lag_vel("lagkrig_predict", velf, torch.float32, stpix.shape[0]), "lagkrig_predict")


# ---- moving-neighbourhood space-time kriging (csrc/lkrig.hip)
LKRIG_MAX_K = 64         # neighbours per target: one lane of the target's wave each


def _lkrig_args(who, pix, z, info, params, cand, B, T, k, frames):
    F = B * T
    fcap = pix.shape[1]
    _krig_t(who, pix, torch.int32, (F, fcap))
    _krig_t(who, z, torch.float32, (F, fcap))
    _krig_t(who, info, torch.int32, (2 * F,))
    _krig_t(who, params, torch.float32, (B, 4))
    if cand is not None:
        _krig_t(who, cand, torch.int32, (B,))
    if not 1 <= k <= LKRIG_MAX_K:
        raise ValueError(f"{who}: k must be 1..{LKRIG_MAX_K} (got {k})")
    if not 0 <= frames < T:
        raise ValueError(f"{who}: the temporal half-window must be 0..T - 1 = {T - 1} (got {frames})")
    return fcap


def lkrig_predict(pix, z, info, params, cand, model, k, frames, B, T, H, W, variance=False, neighbours=False, velf=None):
    """Moving-neighbourhood space-time ordinary kriging of every pixel of every frame from krig_compact's per-frame arrays: each target
    from its k nearest points (key dy^2 + dx^2 + kappa^2 dt^2, ties by frame then raster index) within `frames` frames of its own.
    params (B, 4) fp32 = (nugget, psill, range, kappa); cand (B,) int32 or None (< 0: degenerate sample).  Returns out (B, T, H*W),
    var (the same shape, or None), status (B,) int32 = targets that met a non-positive pivot, and nbr (B, T, H*W, k) int32 (the
    kernel's own selection as frame * fcap + slot, -1 past the candidates; None unless asked for).
    velf (B, 2) fp32 = (v_y, v_x) per sample: the same in the Lagrangian frame, key (dy - v_y dt)^2 + (dx - v_x
    dt)^2 + kappa^2 dt^2 and lagkrig's distance inside the system."""
    lib = _hip.load()
    fcap = _lkrig_args("lkrig_predict", pix, z, info, params, cand, B, T, k, frames)
    if velf is not None:
        _lag_vel("lkrig_predict", velf, torch.float32, B)
    if H < 1 or W < 1:
        raise RuntimeError(f"lkrig_predict: bad frame shape {H} x {W}")
    dev = pix.device
    stat = torch.empty(B, 2, device=dev, dtype=torch.float64)
    out = torch.empty(B, T, H * W, device=dev, dtype=torch.float32)
    var = torch.empty(B, T, H * W, device=dev, dtype=torch.float32) if variance else None
    nbr = torch.empty(B, T, H * W, k, device=dev, dtype=torch.int32) if neighbours else None
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    _hip.check(lib.p2i_lkrig_predict(_ptr(pix), _ptr(z), _ptr(info), _ptr(params), _ptr(cand), int(model), k, frames, B, T, H, W, fcap,
                                     _ptr(stat), _ptr(out), _ptr(var), _ptr(status), _ptr(nbr), _ptr(velf), _stream()), "p2i_lkrig_predict")
    return out, var, status, nbr


def lkrig_loso(pix, z, info, params, cand, model, k, frames, B, T, velf=None):
    """lkrig_predict with the points as targets and every point at the target's own pixel taken out of the candidates: leave-one-site-out
    without an inverse.  Returns pred, var (B*T, fcap) (0 past the frame's count, NaN where no candidate is left or the sample is
    degenerate) and status (B,) int32.  velf: as in lkrig_predict."""
    lib = _hip.load()
    fcap = _lkrig_args("lkrig_loso", pix, z, info, params, cand, B, T, k, frames)
    if velf is not None:
        _lag_vel("lkrig_loso", velf, torch.float32, B)
    dev = pix.device
    stat = torch.empty(B, 2, device=dev, dtype=torch.float64)
    pred, var = torch.empty_like(z), torch.empty_like(z)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    _hip.check(lib.p2i_lkrig_loso(_ptr(pix), _ptr(z), _ptr(info), _ptr(params), _ptr(cand), int(model), k, frames, B, T, fcap, _ptr(stat),
                                  _ptr(pred), _ptr(var), _ptr(status), _ptr(velf), _stream()), "p2i_lkrig_loso")
    return pred, var, status


# ---- kriging variance and leave-one-out cross-validation (csrc/krig_uq.hip)
LOO_NSUM = 5            # (n, sum e, sum |e|, sum e^2, sum e^2 / var)


def krig_invert(L, nsys, np_, Winv):
    """Winv (>= nsys * np_ * np_ fp32, not L) = the inverse of each system's Cholesky factor: lower triangular, identity on the padding."""
    lib = _hip.load()
    _krig_t("krig_invert", L, torch.float32)
    _krig_t("krig_invert", Winv, torch.float32)
    if nsys < 1 or np_ < KRIG_TILE or np_ % KRIG_TILE or np_ > KRIG_MAX_CAP:
        raise RuntimeError(f"krig_invert: bad system shape {nsys} x {np_}")
    if min(L.numel(), Winv.numel()) < nsys * np_ * np_ or L.data_ptr() == Winv.data_ptr():
        raise RuntimeError("krig_invert: workspace too small, or the inverse would overwrite the factor")
    _hip.check(lib.p2i_krig_invert(_ptr(L), nsys, np_, _ptr(Winv), _stream()), "p2i_krig_invert")


def krig_variance(sys, Winv, sol, H, W, var):
    """Kriging variance of the R frames of each of the chunk's systems into var (F, H*W), in place: c00 - |Winv k(p)|^2 +
    (1 - u^T k(p))^2 / s clamped at 0, exactly 0 on a gauge pixel, NaN for a system without a model."""
    of = sys.of
    _krig_t("krig_variance", Winv, torch.float32)
    _krig_t("krig_variance", sol, torch.float64, (sys.ns, of.R + 1, of.np_))
    _krig_t("krig_variance", var, torch.float32, (of.F, H * W))
    _krig_ws("krig_variance", Winv, sys.ns, of.np_, "inverse")
    sys.call("p2i_krig_variance", _ptr(Winv), _ptr(sol), H, W, _ptr(var))


def krig_loo(sys, Winv, sol, alpha, pred, var):
    """Leave-one-out prediction and variance of every gauge of the chunk's systems' frames into pred, var (F, cap), in place."""
    of = sys.of
    _krig_t("krig_loo", Winv, torch.float32)
    _krig_t("krig_loo", sol, torch.float64, (sys.ns, of.R + 1, of.np_))
    for t in (alpha, pred, var):
        _krig_t("krig_loo", t, torch.float32, (of.F, of.cap))
    _krig_ws("krig_loo", Winv, sys.ns, of.np_, "inverse")
    colsq = torch.empty(sys.ns, of.np_, device=of.z.device, dtype=torch.float64)
    sys.call("p2i_krig_loo", _ptr(Winv), _ptr(sol), _ptr(alpha), _ptr(colsq), _ptr(pred), _ptr(var))


# ---- conditional simulation of ordinary kriging (csrc/krig_cs.hip)
KRIG_CS_MAX_SIDE = 512       # side of the embedding torus
KRIG_CS_MAX_MEMBERS = 64
KRIG_CS_EMBEDS = (2, 3, 4)
_KRIG_CS_P_BYTES = 1 << 28   # the stage-1 workspace of one p2i_krig_cs_fields call stays under this
_KRIG_CS_TABLES = {}


def krig_cs_torus(H, W, embed):
    """(Sy, Sx) = (embed H, embed W) of the embedding torus; ValueError for an embed outside 2..4 or a side past 512."""
    if isinstance(embed, bool) or not isinstance(embed, int) or embed not in KRIG_CS_EMBEDS:
        raise ValueError(f"model.ensemble.embed must be an integer in {list(KRIG_CS_EMBEDS)} (got {embed!r})")
    Sy, Sx = embed * H, embed * W
    if max(Sy, Sx) > KRIG_CS_MAX_SIDE:
        raise ValueError(f"conditional simulation: the embedding torus {Sy} x {Sx} (embed {embed} of {H} x {W} frames) exceeds "
                         f"{KRIG_CS_MAX_SIDE} on a side")
    return Sy, Sx


def _krig_cs_members(who, M):
    if isinstance(M, bool) or not isinstance(M, int) or not 1 <= M <= KRIG_CS_MAX_MEMBERS:
        raise ValueError(f"{who}: members must be an integer in [1, {KRIG_CS_MAX_MEMBERS}] (got {M!r})")


def _cs_twiddles(S, n, device):
    """(2, S, n) fp32 = cos, sin of 2 pi (a b mod S) / S, a < S, b < n, rounded from fp64 of the reduced argument."""
    ang = (torch.arange(S, dtype=torch.int64)[:, None] * torch.arange(n, dtype=torch.int64)[None, :]) % S
    ang = ang.double() * (2.0 * math.pi / S)
    return torch.stack([torch.cos(ang), torch.sin(ang)]).float().contiguous().to(device)


def krig_cs_tables(H, W, embed, device):
    """The host-built fp64 twiddles of one (H, W, embed), on `device` (kept): tw (Sy + Sx,) fp64 = cos(2 pi m / Sy), cos(2 pi m / Sx)
    for the spectrum; tx (2, Sx, W) and ty (2, Sy, H) fp32 = cos, sin of 2 pi k w / Sx and 2 pi j h / Sy for the fields."""
    key = (H, W, embed, str(device))
    if key not in _KRIG_CS_TABLES:
        Sy, Sx = krig_cs_torus(H, W, embed)
        tw = torch.cat([torch.cos(torch.arange(S, dtype=torch.float64) * (2.0 * math.pi / S)) for S in (Sy, Sx)])
        _KRIG_CS_TABLES[key] = {"Sy": Sy, "Sx": Sx, "tw": tw.contiguous().to(device), "tx": _cs_twiddles(Sx, W, device),
                                "ty": _cs_twiddles(Sy, H, device)}
    return _KRIG_CS_TABLES[key]


def krig_cs_spectrum(params, cand, model, H, W, embed):
    """amp (B, Sy, Sx) fp32, the amplitude of the circulant embedding of every sample's covariance, and clip (B,) fp64, the share of
    the spectrum that was negative and clipped (0 where the embedding is exact; NaN for a degenerate sample)."""
    lib = _hip.load()
    _krig_t("krig_cs_spectrum", params, torch.float32)
    B = params.shape[0]
    if tuple(params.shape) != (B, 4):
        raise RuntimeError("krig_cs_spectrum: params (B, 4) expected")
    if cand is not None:
        _krig_t("krig_cs_spectrum", cand, torch.int32, (B,))
    tab = krig_cs_tables(H, W, embed, params.device)
    Sy, Sx = tab["Sy"], tab["Sx"]
    work = torch.empty(2, B, Sy, Sx, device=params.device, dtype=torch.float64)
    amp = torch.empty(B, Sy, Sx, device=params.device, dtype=torch.float32)
    clip = torch.empty(B, device=params.device, dtype=torch.float64)
    _hip.check(lib.p2i_krig_cs_spectrum(_ptr(params), _ptr(cand), int(model), B, Sy, Sx, _ptr(tab["tw"]), _ptr(work), _ptr(amp), _ptr(clip),
                                        _stream()), "p2i_krig_cs_spectrum")
    return amp, clip


def krig_cs_noise(seed, stream_id, q0, npairs, Sy, Sx, device):
    """xi (npairs, Sy, Sx, 2) fp32: the complex standard normal of the member pairs q0 .. q0 + npairs - 1 of frame id stream_id."""
    lib = _hip.load()
    if torch.device(device).type != "cuda":
        raise RuntimeError("krig_cs_noise runs on the HIP path only (a CUDA device)")
    if not (1 <= Sy <= KRIG_CS_MAX_SIDE and 1 <= Sx <= KRIG_CS_MAX_SIDE) or q0 < 0 or npairs < 1:
        raise ValueError(f"krig_cs_noise: bad torus {Sy} x {Sx} or pairs {q0} + {npairs}")
    xi = torch.empty(npairs, Sy, Sx, 2, device=device, dtype=torch.float32)
    _hip.check(lib.p2i_krig_cs_noise(int(seed) & (2 ** 64 - 1), int(stream_id), int(q0), int(npairs), Sy, Sx, _ptr(xi), _stream()),
               "p2i_krig_cs_noise")
    return xi


def krig_cs_fields(amp, streams, seed, T, M, H, W, embed, ens):
    """The unconditional members U of every frame into ens (F, M, H*W), in place: pair q of frame f is DFT2(amp[f // T] xi)[:H, :W]
    with xi of (seed, streams[f], q); member 2q is its real part, member 2q + 1 its imaginary part."""
    lib = _hip.load()
    _krig_cs_members("krig_cs_fields", M)
    tab = krig_cs_tables(H, W, embed, ens.device)
    Sy, Sx = tab["Sy"], tab["Sx"]
    F = ens.shape[0]
    _krig_t("krig_cs_fields", ens, torch.float32, (F, M, H * W))
    _krig_t("krig_cs_fields", amp, torch.float32, (F // T, Sy, Sx))
    _krig_t("krig_cs_fields", streams, torch.int64, (F,))
    npairs = (M + 1) // 2
    per = max(1, min(F, _KRIG_CS_P_BYTES // (npairs * 2 * Sy * W * 4)))
    P = torch.empty(per * npairs * 2 * Sy * W, device=ens.device, dtype=torch.float32)
    for f0 in range(0, F, per):
        _hip.check(lib.p2i_krig_cs_fields(_ptr(amp), _ptr(streams), _ptr(tab["tx"]), _ptr(tab["ty"]), int(seed) & (2 ** 64 - 1), f0,
                                          min(per, F - f0), T, M, H, W, Sy, Sx, _ptr(P), _ptr(ens), _stream()), "p2i_krig_cs_fields")


def krig_cs_weights(sys, Winv, sol, ens, M, H, W):
    """(alpha (nsys, R*M, cap), mu (nsys, R*M)): the kriging of the residuals z - U(gauges) of every member of the chunk's systems'
    frames, ens (F, M, H*W) holding U; column t*M + m of a system is member m of its frame t."""
    of, ns = sys.of, sys.ns
    _krig_cs_members("krig_cs_weights", M)
    _krig_t("krig_cs_weights", ens, torch.float32, (of.F, M, H * W))
    _krig_t("krig_cs_weights", Winv, torch.float32)
    _krig_t("krig_cs_weights", sol, torch.float64, (ns, of.R + 1, of.np_))
    _krig_ws("krig_cs_weights", Winv, ns, of.np_, "inverse")
    alpha = torch.empty(ns, of.R * M, of.cap, device=of.z.device, dtype=torch.float32)
    mu = torch.empty(ns, of.R * M, device=of.z.device, dtype=torch.float32)
    sys.call("p2i_krig_cs_weights", _ptr(Winv), _ptr(sol), _ptr(ens), M, H, W, _ptr(alpha), _ptr(mu))
    return alpha, mu


def krig_cs_predict(sys, alpha, mu, M, H, W, ens):
    """ens[f][m] = U + mu + sum_i alpha_i c0(p, x_i) for the members of the chunk's systems' frames, in place; z on a gauge pixel; NaN
    for a system without a model."""
    of, ns = sys.of, sys.ns
    _krig_cs_members("krig_cs_predict", M)
    _krig_t("krig_cs_predict", ens, torch.float32, (of.F, M, H * W))
    _krig_t("krig_cs_predict", alpha, torch.float32, (ns, of.R * M, of.cap))
    _krig_t("krig_cs_predict", mu, torch.float32, (ns, of.R * M))
    sys.call("p2i_krig_cs_predict", _ptr(alpha), _ptr(mu), M, H, W, _ptr(ens))


# ---- conditional simulation of space-time kriging (csrc/stkrig_cs.hip, include/p2i_stcs.h)
STCS_MAX_ST = 128            # temporal side of the embedding torus
_STCS_WORK_BYTES = 1 << 28   # the spectrum's fp64 workspace and each of the fields' workspaces of one call stay under this, except that a
                             # chunk is never less than one sample: 16 St Sy Sx bytes, above the bound past 16 Mi cells (512 MiB at most)
_STCS_TABLES = {}
STCS_STAGES_ALL = 7          # the three transforms of p2i_stcs_fields: along k, along j, along l


def stcs_abi_version() -> int:
    return int(_hip.load().p2i_stcs_abi_version())


def stcs_torus(T, H, W, embed, embed_time):
    """(St, Sy, Sx) = (embed_time T, embed H, embed W) of the space-time embedding torus; ValueError for an embed outside 2..4, a
    spatial side past 512 or more than 128 temporal cells."""
    if isinstance(embed_time, bool) or not isinstance(embed_time, int) or embed_time not in KRIG_CS_EMBEDS:
        raise ValueError(f"model.ensemble.embed_time must be an integer in {list(KRIG_CS_EMBEDS)} (got {embed_time!r})")
    Sy, Sx = krig_cs_torus(H, W, embed)
    St = embed_time * T
    if St > STCS_MAX_ST:
        raise ValueError(f"conditional simulation: the embedding torus has {St} temporal cells (embed_time {embed_time} of {T} frames), "
                         f"more than {STCS_MAX_ST}: use shorter chunks (scripts/infer.py --stride)")
    return St, Sy, Sx


def stcs_tables(T, H, W, embed, embed_time, device):
    """The host-built fp64 twiddles of one (T, H, W, embed, embed_time), on `device` (kept): tw (St + Sy + Sx,) fp64 = cos(2 pi m / S) of
    the three sides for the spectrum; tx (2, Sx, W), ty (2, Sy, H) and tt (2, St, T) fp32 = cos, sin of 2 pi (a b mod S) / S."""
    key = (T, H, W, embed, embed_time, str(device))
    if key not in _STCS_TABLES:
        St, Sy, Sx = stcs_torus(T, H, W, embed, embed_time)
        tw = torch.cat([torch.cos(torch.arange(S, dtype=torch.float64) * (2.0 * math.pi / S)) for S in (St, Sy, Sx)])
        _STCS_TABLES[key] = {"St": St, "Sy": Sy, "Sx": Sx, "tw": tw.contiguous().to(device), "tx": _cs_twiddles(Sx, W, device),
                             "ty": _cs_twiddles(Sy, H, device), "tt": _cs_twiddles(St, T, device)}
    return _STCS_TABLES[key]


def stcs_spectrum(params, cand, model, T, H, W, embed, embed_time):
    """amp (B, St, Sy, Sx) fp32, the amplitude of the circulant embedding of every sample's space-time covariance (params (B, 4) =
    nugget, psill, range, kappa), and clip (B,) fp64, the share of the spectrum that was negative and clipped (0 where the embedding
    is exact; NaN for a degenerate sample).  The samples go through the fp64 workspace a chunk at a time (at least one sample: 16 bytes
    per torus cell); amp is held whole, 4 bytes per cell and sample, because the fields of every sample read it."""
    lib = _hip.load()
    _krig_t("stcs_spectrum", params, torch.float32)
    B = params.shape[0]
    if tuple(params.shape) != (B, 4):
        raise RuntimeError("stcs_spectrum: params (B, 4) expected")
    if cand is not None:
        _krig_t("stcs_spectrum", cand, torch.int32, (B,))
    tab = stcs_tables(T, H, W, embed, embed_time, params.device)
    St, Sy, Sx = tab["St"], tab["Sy"], tab["Sx"]
    cells = St * Sy * Sx
    per = max(1, min(B, _STCS_WORK_BYTES // (2 * cells * 8), 65535 // St))
    work = torch.empty(2, per, cells, device=params.device, dtype=torch.float64)
    amp = torch.empty(B, St, Sy, Sx, device=params.device, dtype=torch.float32)
    clip = torch.empty(B, device=params.device, dtype=torch.float64)
    for b0 in range(0, B, per):
        nb = min(per, B - b0)
        _hip.check(lib.p2i_stcs_spectrum(_ptr(params[b0:]), _ptr(cand[b0:]) if cand is not None else None, int(model), nb, St, Sy, Sx,
                                         _ptr(tab["tw"]), _ptr(work), _ptr(amp[b0:]), _ptr(clip[b0:]), _stream()), "p2i_stcs_spectrum")
    return amp, clip


def stcs_noise(seed, stream_id, q0, npairs, St, Sy, Sx, device):
    """xi (npairs, St, Sy, Sx, 2) fp32: the complex standard normal of the member pairs q0 .. q0 + npairs - 1 of sample id stream_id."""
    lib = _hip.load()
    if torch.device(device).type != "cuda":
        raise RuntimeError("stcs_noise runs on the HIP path only (a CUDA device)")
    if not (1 <= St <= STCS_MAX_ST and 1 <= Sy <= KRIG_CS_MAX_SIDE and 1 <= Sx <= KRIG_CS_MAX_SIDE) or q0 < 0 or npairs < 1:
        raise ValueError(f"stcs_noise: bad torus {St} x {Sy} x {Sx} or pairs {q0} + {npairs}")
    xi = torch.empty(npairs, St, Sy, Sx, 2, device=device, dtype=torch.float32)
    _hip.check(lib.p2i_stcs_noise(int(seed) & (2 ** 64 - 1), int(stream_id), int(q0), int(npairs), St, Sy, Sx, _ptr(xi), _stream()),
               "p2i_stcs_noise")
    return xi


def stcs_fields(amp, streams, seed, M, T, H, W, embed, embed_time, ens, stages=STCS_STAGES_ALL):
    """The unconditional members U of every sample into ens (B, T, M, H*W), in place: pair q of sample b is DFT3(amp[b] xi)[:T, :H, :W]
    with xi of (seed, streams[b], q); member 2q is its real part, member 2q + 1 its imaginary part.  The (sample, pair) units go
    through the two workspaces a chunk at a time.  stages: a subset of the three transforms (bit 0 along k, bit 1 along j, bit 2 along
    l), meaningful on its own only where all units fit one chunk: the bench tool times a stage with it."""
    lib = _hip.load()
    _krig_cs_members("stcs_fields", M)
    tab = stcs_tables(T, H, W, embed, embed_time, ens.device)
    St, Sy, Sx = tab["St"], tab["Sy"], tab["Sx"]
    B = ens.shape[0]
    _krig_t("stcs_fields", ens, torch.float32, (B, T, M, H * W))
    _krig_t("stcs_fields", amp, torch.float32, (B, St, Sy, Sx))
    _krig_t("stcs_fields", streams, torch.int64, (B,))
    units = B * ((M + 1) // 2)
    per = max(1, min(units, _STCS_WORK_BYTES // (2 * St * Sy * W * 4), 65535))
    P = torch.empty(per * 2 * St * Sy * W, device=ens.device, dtype=torch.float32)
    P2 = torch.empty(per * 2 * St * H * W, device=ens.device, dtype=torch.float32)
    for u0 in range(0, units, per):
        _hip.check(lib.p2i_stcs_fields(_ptr(amp), _ptr(streams), _ptr(tab["tx"]), _ptr(tab["ty"]), _ptr(tab["tt"]),
                                       int(seed) & (2 ** 64 - 1), u0, min(per, units - u0), M, T, H, W, St, Sy, Sx, int(stages), _ptr(P), _ptr(P2),
                                       _ptr(ens), _stream()), "p2i_stcs_fields")


def _stcs_sys(who, sys, stt, ens, M, T, H, W):
    of = sys.of
    _krig_cs_members(who, M)
    if of.R != 1 or of.T != 1:
        raise RuntimeError(f"{who}: a space-time system is one sample (R = T = 1)")
    if not 1 <= T <= STCS_MAX_ST:
        raise ValueError(f"{who}: frames per sample must be in [1, {STCS_MAX_ST}] (got {T})")
    _krig_t(who, stt, torch.int32, (of.F, of.cap))
    _krig_t(who, ens, torch.float32, (of.F, T, M, H * W))


def stcs_weights(sys, stt, Winv, sol, ens, M, T, H, W):
    """(alpha (nsys, M, cap), mu (nsys, M)): the space-time kriging of the residuals z_i - U_m(stt_i, stpix_i) of every member of the
    chunk's samples (sys: stpix, stz, stinfo with R = T = 1), ens (B, T, M, H*W) holding U."""
    of, ns = sys.of, sys.ns
    _stcs_sys("stcs_weights", sys, stt, ens, M, T, H, W)
    _krig_t("stcs_weights", Winv, torch.float32)
    _krig_t("stcs_weights", sol, torch.float64, (ns, 2, of.np_))
    _krig_ws("stcs_weights", Winv, ns, of.np_, "inverse")
    alpha = torch.empty(ns, M, of.cap, device=of.z.device, dtype=torch.float32)
    mu = torch.empty(ns, M, device=of.z.device, dtype=torch.float32)
    sys.call("p2i_stcs_weights", _ptr(stt), _ptr(Winv), _ptr(sol), _ptr(ens), M, T, H, W, _ptr(alpha), _ptr(mu))
    return alpha, mu


def stcs_predict(sys, stt, alpha, mu, M, T, H, W, ens):
    """ens[b][t][m] = U + mu + sum_i alpha_i c0((t, p), i) for the members of the chunk's samples, in place; z at a point's own frame
    and pixel; NaN for a sample without a model."""
    of, ns = sys.of, sys.ns
    _stcs_sys("stcs_predict", sys, stt, ens, M, T, H, W)
    _krig_t("stcs_predict", alpha, torch.float32, (ns, M, of.cap))
    _krig_t("stcs_predict", mu, torch.float32, (ns, M))
    sys.call("p2i_stcs_predict", _ptr(stt), _ptr(alpha), _ptr(mu), M, T, H, W, _ptr(ens))


def idw_loo(pix, z, info, power=2.0):
    """pred (F, cap): all-gauge IDW at each gauge from the frame's other gauges (NaN with fewer than 2, 0 past the count)."""
    lib = _hip.load()
    F, cap = pix.shape
    _krig_t("idw_loo", pix, torch.int32)
    _krig_t("idw_loo", z, torch.float32, (F, cap))
    _krig_t("idw_loo", info, torch.int32, (2 * F,))
    if not power > 0:
        raise ValueError("idw_loo: power must be positive")
    pred = torch.empty(F, cap, device=pix.device, dtype=torch.float32)
    _hip.check(lib.p2i_idw_loo(_ptr(pix), _ptr(z), _ptr(info), F, cap, float(power), _ptr(pred), _stream()), "p2i_idw_loo")
    return pred


def loo_scores(z, pred, var, counts):
    """(LOO_NSUM,) fp64 on the device: n, sum e, sum |e|, sum e^2, sum e^2 / var with e = z - pred over the entries i < counts[f] of
    the (F, cap) arrays whose pred (and var; None: the last sum is 0) is not NaN."""
    lib = _hip.load()
    F, cap = z.shape
    _krig_t("loo_scores", z, torch.float32)
    _krig_t("loo_scores", pred, torch.float32, (F, cap))
    if var is not None:
        _krig_t("loo_scores", var, torch.float32, (F, cap))
    _krig_t("loo_scores", counts, torch.int32)
    if counts.numel() < F:
        raise RuntimeError("loo_scores: one count per frame expected")
    part = torch.empty(F, LOO_NSUM, device=z.device, dtype=torch.float64)
    out = torch.empty(LOO_NSUM, device=z.device, dtype=torch.float64)
    _hip.check(lib.p2i_loo_scores(_ptr(z), _ptr(pred), _ptr(var), _ptr(counts), F, cap, _ptr(part), _ptr(out), _stream()), "p2i_loo_scores")
    return out


# ---- evaluation: exp1 scoring, exp3 analysis, exp2 renders (csrc/eval_exp{1,3,2}.hip; p2igan_bench/evaluation/ drives these) ----
EXP1_MAX_THR = 8
EXP1_NSTAT = 8 + 3 * EXP1_MAX_THR
EXP1_BINS = 50
EXP3_NREC = 4
EXP3_BINS = 64
EXP3_NHIST = EXP3_BINS + 1
EXP2_NBOUNDS = 142
EXP2_BAD = 141
_EVAL_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.float64: 2}


def _eval_code(t: torch.Tensor) -> int:
    if not (t.is_cuda and t.is_contiguous()):
        raise RuntimeError("evaluation ops need contiguous CUDA tensors (the HIP path has no CPU fallback)")
    if t.dtype not in _EVAL_DTYPES:
        raise RuntimeError(f"evaluation ops: unsupported dtype {t.dtype}")
    return _EVAL_DTYPES[t.dtype]


def _eval_input(t: torch.Tensor, tl):
    """An input [T, H, W] (uint8 / f32 / f64) and its crop origin (top, left) as the ABI's descriptor p2i_eval_input; an entry point
    takes it by reference, and the caller's name or argument list keeps it alive across the call."""
    if t.dim() != 3:
        raise RuntimeError(f"evaluation ops: expected [T, H, W], got {tuple(t.shape)}")
    return _hip.EvalInput(_ptr(t), _eval_code(t), t.shape[1], t.shape[2], int(tl[0]), int(tl[1]))


def _eval_bufs(what, *bufs):
    """Every (tensor, dtype, numel) is a contiguous device tensor of that dtype and size."""
    for t, dt, n in bufs:
        if not (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() == n):
            raise RuntimeError(f"{what}: bad buffer")


def _f64s(vals):
    vals = [float(v) for v in vals]
    return (C.c_double * max(1, len(vals)))(*vals)


def exp1_transform(x: torch.Tensor, divide_by_3: bool = True) -> torch.Tensor:
    """transform_mmhr of a uint8 / f32 / f64 device tensor, in fp64 on the device."""
    code = _eval_code(x)
    out = torch.empty(x.shape, device=x.device, dtype=torch.float64)
    if x.numel():
        _hip.check(_hip.load().p2i_exp1_transform(_ptr(x), code, x.numel(), int(divide_by_3), _ptr(out), _stream()),
                   "p2i_exp1_transform")
    return out


def exp1_workspace(T: int, S: int, pool: int) -> int:
    n = C.c_int64(0)
    _hip.check(_hip.load().p2i_exp1_workspace(T, S, pool, C.byref(n)), "p2i_exp1_workspace")
    return int(n.value)


def exp1_accumulate(pred, truth, ptl, gtl, S, pool, rank, nsel, lut, thresholds, divide_by_3, pool_p, pool_g, sel_p, sel_g, part):
    """One aligned piece: pred, truth [T, H, W] (their own H, W), crop origins ptl / gtl = (top, left) of the S x S crop.  Writes the
    piece's per-workgroup statistics to part [exp1_workspace(T, S, pool)] (fp64), pool_* [T, S/pool, S/pool] and sel_* [T, nsel]."""
    T = pred.shape[0]
    if truth.shape[0] != T or len(thresholds) > EXP1_MAX_THR:
        raise RuntimeError("exp1_accumulate: frame count / thresholds")
    pin, gin = _eval_input(pred, ptl), _eval_input(truth, gtl)
    if part.numel() != exp1_workspace(T, S, pool):
        raise RuntimeError("exp1_accumulate: workspace size")
    npool = T * (S // pool) ** 2
    _eval_bufs("exp1_accumulate", (rank, torch.int32, S * S), (lut, torch.float64, 256), (pool_p, torch.float32, npool),
               (pool_g, torch.float32, npool), (sel_p, torch.float32, T * nsel), (sel_g, torch.float32, T * nsel),
               (part, torch.float64, part.numel()))
    _hip.check(_hip.load().p2i_exp1_accumulate(
        pin, gin, T, S, pool, _ptr(rank), nsel, _ptr(lut), _f64s(thresholds), len(thresholds), int(divide_by_3), _ptr(pool_p),
        _ptr(pool_g), _ptr(sel_p) if nsel else None, _ptr(sel_g) if nsel else None, _ptr(part), _stream()), "p2i_exp1_accumulate")


def exp1_merge(part, acc):
    """acc [EXP1_NSTAT] (+)= the partial records of part (a multiple of EXP1_NSTAT doubles), folded in a fixed order."""
    if part.numel() % EXP1_NSTAT:
        raise RuntimeError("exp1_merge: bad buffer")
    _eval_bufs("exp1_merge", (part, torch.float64, part.numel()), (acc, torch.float64, EXP1_NSTAT))
    _hip.check(_hip.load().p2i_exp1_merge(_ptr(part), part.numel() // EXP1_NSTAT, _ptr(acc), _stream()), "p2i_exp1_merge")


def exp1_hist(sel_p, sel_g, acc, score, flag, edges):
    """Per-frame PSS histograms of the compacted selections [T, nsel] over acc's range: score [T] f64, flag [T] int32, edges [52]."""
    T, nsel = sel_p.shape
    _eval_bufs("exp1_hist", (sel_p, torch.float32, T * nsel), (sel_g, torch.float32, T * nsel), (acc, torch.float64, EXP1_NSTAT),
               (score, torch.float64, T), (flag, torch.int32, T), (edges, torch.float32, EXP1_BINS + 2))
    _hip.check(_hip.load().p2i_exp1_hist(_ptr(sel_p) if nsel else None, _ptr(sel_g) if nsel else None, T, nsel, _ptr(acc), _ptr(score),
                                         _ptr(flag), _ptr(edges), _stream()), "p2i_exp1_hist")


def exp1_ssim(pool_p, pool_g):
    """pool_* [T, npix] f32 -> (SSIM(p_t, g_t), lag-1 and lag-2 dTSSIM terms), each [T] f64."""
    T, npix = pool_p.shape
    _eval_bufs("exp1_ssim", (pool_p, torch.float32, T * npix), (pool_g, torch.float32, T * npix))
    out = torch.empty(3, T, device=pool_p.device, dtype=torch.float64)
    _hip.check(_hip.load().p2i_exp1_ssim(_ptr(pool_p), _ptr(pool_g), T, npix, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream()),
               "p2i_exp1_ssim")
    return out


def exp1_finalize(acc, thresholds, score, flag, edges, ssim3):
    """The table's numbers of one method as a [8 + 4 k] f64 device tensor (see include/p2i_hip.h)."""
    T = score.shape[0]
    _eval_bufs("exp1_finalize", (acc, torch.float64, EXP1_NSTAT), (score, torch.float64, T), (flag, torch.int32, T),
               (edges, torch.float32, EXP1_BINS + 2), (ssim3, torch.float64, 3 * T))
    out = torch.empty(8 + 4 * len(thresholds), device=acc.device, dtype=torch.float64)
    _hip.check(_hip.load().p2i_exp1_finalize(_ptr(acc), _f64s(thresholds), len(thresholds), T, _ptr(score), _ptr(flag), _ptr(edges),
                                             _ptr(ssim3[0]), _ptr(ssim3[1]), _ptr(ssim3[2]), _ptr(out), _stream()), "p2i_exp1_finalize")
    return out


def exp3_accumulate(pred, truth, ptl, gtl, S, rank, lut, divide_by_3, rec, rows, hist=None):
    """One aligned piece: pred, truth [T, H, W] (their own H, W), crop origins ptl / gtl = (top, left) of the S x S crop.  Writes the
    per-frame records rec [T, EXP3_NREC] (f64) and scatter-pool row counts rows [T, S] (int32); adds the prediction's log-frequency
    counts to hist [EXP3_NHIST] (int64) when it is given."""
    T = pred.shape[0]
    if truth.shape[0] != T:
        raise RuntimeError("exp3_accumulate: frame count")
    pin, gin = _eval_input(pred, ptl), _eval_input(truth, gtl)
    _eval_bufs("exp3_accumulate", (rank, torch.int32, S * S), (lut, torch.float64, 256), (rec, torch.float64, T * EXP3_NREC),
               (rows, torch.int32, T * S), *([(hist, torch.int64, EXP3_NHIST)] if hist is not None else []))
    _hip.check(_hip.load().p2i_exp3_accumulate(pin, gin, T, S, _ptr(rank), _ptr(lut), int(divide_by_3), _ptr(rec), _ptr(rows),
                                               _ptr(hist), _stream()), "p2i_exp3_accumulate")


def exp3_truth_hist(truth, gtl, S, lut, divide_by_3, hist):
    """Adds the log-frequency counts of every cropped frame of truth [T, H, W] to hist [EXP3_NHIST] (int64)."""
    gin = _eval_input(truth, gtl)
    _eval_bufs("exp3_truth_hist", (lut, torch.float64, 256), (hist, torch.int64, EXP3_NHIST))
    _hip.check(_hip.load().p2i_exp3_truth_hist(gin, truth.shape[0], S, _ptr(lut), int(divide_by_3), _ptr(hist), _stream()),
               "p2i_exp3_truth_hist")


def exp3_scan(rows: torch.Tensor) -> torch.Tensor:
    """The inclusive prefix (int64) of int32 row counts, on the device."""
    _eval_bufs("exp3_scan", (rows, torch.int32, rows.numel()))
    out = torch.empty(rows.numel(), device=rows.device, dtype=torch.int64)
    if rows.numel():
        _hip.check(_hip.load().p2i_exp3_scan(_ptr(rows), rows.numel(), _ptr(out), _stream()), "p2i_exp3_scan")
    return out


def exp3_gather(pred, truth, ptl, gtl, S, lut, divide_by_3, prefix, row0, ords, out_g, out_p):
    """For the pool ordinals ords [K] (int64) that fall in this piece's rows [row0, row0 + T * S) of the method's prefix, writes the
    transformed (truth, prediction) of the pool pixel to out_g / out_p [K] (f64)."""
    T, K = pred.shape[0], ords.numel()
    if truth.shape[0] != T or row0 + T * S > prefix.numel():
        raise RuntimeError("exp3_gather: frame count / rows")
    pin, gin = _eval_input(pred, ptl), _eval_input(truth, gtl)
    _eval_bufs("exp3_gather", (lut, torch.float64, 256), (prefix, torch.int64, prefix.numel()), (ords, torch.int64, K),
               (out_g, torch.float64, K), (out_p, torch.float64, K))
    if K == 0 or T == 0:
        return
    _hip.check(_hip.load().p2i_exp3_gather(pin, gin, T, S, _ptr(lut), int(divide_by_3), _ptr(prefix), int(row0), _ptr(ords), K,
                                           _ptr(out_g), _ptr(out_p), _stream()), "p2i_exp3_gather")


def exp3_nse(event_rec, event_off, stack_rec) -> torch.Tensor:
    """[1 + E] f64 on the device: the whole-stack NSE of stack_rec [T, EXP3_NREC], then per event e the nanmean of the clipped
    per-frame NSEs of event_rec rows event_off[e] .. event_off[e + 1] - 1 (event_off: int32 [E + 1] on the device)."""
    E = event_off.numel() - 1 if event_off is not None else 0
    T = stack_rec.shape[0]
    out = torch.empty(1 + E, device=stack_rec.device, dtype=torch.float64)
    if E:
        _eval_bufs("exp3_nse", (event_off, torch.int32, E + 1), (event_rec, torch.float64, event_rec.numel()))
    _eval_bufs("exp3_nse", (stack_rec, torch.float64, T * EXP3_NREC))
    _hip.check(_hip.load().p2i_exp3_nse(_ptr(event_rec) if E else None, _ptr(event_off) if E else None, E, _ptr(stack_rec) if T else None,
                                        T, _ptr(out), _stream()), "p2i_exp3_nse")
    return out


def exp2_index(x, tl, S, n, bounds, lut, divide_by_3, out):
    """The colour indices of the first n frames of x [T, H, W] (uint8 / f32 / f64), cropped to S x S at tl = (top, left), into out
    [n, S, S] (uint8): see include/p2i_hip.h.  bounds [EXP2_NBOUNDS] and lut [256] are f64 on the device."""
    xin = _eval_input(x, tl)
    _eval_bufs("exp2_index", (bounds, torch.float64, EXP2_NBOUNDS), (lut, torch.float64, 256), (out, torch.uint8, n * S * S))
    if n == 0:
        return
    _hip.check(_hip.load().p2i_exp2_index(xin, x.shape[0], S, n, _ptr(bounds), _ptr(lut), int(divide_by_3), _ptr(out), _stream()),
               "p2i_exp2_index")


def exp2_pitch(width: int) -> int:
    """The canvas row pitch: the width rounded up to 16 bytes."""
    return (int(width) + 15) // 16 * 16


def exp2_compose(panels, zoom, gauge_bits, points, chrome, oy, ox, step, bg, edge, out):
    """Index panels [P, n, S, S] (uint8) over the chrome [Hc, pitch] (uint8) into out [n, Hc, pitch] (uint8): see include/p2i_hip.h.
    points: int32 [K, 2] (row, column) on the device, each inside the panel (the caller checks that on the host)."""
    P, n, S, _ = panels.shape
    Hc, pitch = chrome.shape
    K = 0 if points is None else points.shape[0]
    _eval_bufs("exp2_compose", (panels, torch.uint8, P * n * S * S), (chrome, torch.uint8, Hc * pitch), (out, torch.uint8, n * Hc * pitch),
               *([(points, torch.int32, K * 2)] if K else []))
    if n == 0:
        return
    _hip.check(_hip.load().p2i_exp2_compose(_ptr(panels), P, n, S, int(zoom), int(gauge_bits), _ptr(points) if K else None, K, _ptr(chrome),
                                            Hc, pitch, int(oy), int(ox), int(step), int(bg), int(edge), _ptr(out), _stream()),
               "p2i_exp2_compose")


# ---- scale-aware verification: FSS and radial spectra (csrc/eval_scale.hip; p2igan_bench/evaluation/scale.py drives these) ----
SCALE_MAX_SCALES = 16
SCALE_LDS_CROP = 128
SCALE_MAX_CROP = 1024


def scale_fss(pred, truth, ptl, gtl, S, lut, thresholds, scales, divide_by_3, part, workspace=None):
    """One aligned piece: pred, truth [T, H, W] (their own H, W), crop origins ptl / gtl.  Writes part [T, nthr, 3 * nscales + 1]
    (int64): per scale sum c_p^2, sum c_g^2, sum c_p c_g, then the truth's hits.  Without ``workspace`` the tables live in LDS
    (S <= SCALE_LDS_CROP); with it (uint32 [T * nthr * 2 * S * S]) in global memory."""
    T, K, N = pred.shape[0], len(thresholds), len(scales)
    if truth.shape[0] != T or not 0 < K <= EXP1_MAX_THR or not 0 < N <= SCALE_MAX_SCALES:
        raise RuntimeError("scale_fss: frame count / thresholds / scales")
    pin, gin = _eval_input(pred, ptl), _eval_input(truth, gtl)
    _eval_bufs("scale_fss", (lut, torch.float64, 256), (part, torch.int64, T * K * (3 * N + 1)),
               *([(workspace, torch.int32, T * K * 2 * S * S)] if workspace is not None else []))
    sc = (C.c_int * N)(*[min(int(n), 2 ** 31 - 1) for n in scales])
    _hip.check(_hip.load().p2i_scale_fss(pin, gin, T, S, _ptr(lut), _f64s(thresholds), K, sc, N, int(divide_by_3),
                                         _ptr(workspace) if workspace is not None else None, _ptr(part), _stream()), "p2i_scale_fss")


def scale_fss_merge(part, acc):
    """acc [n] (int64) += the sums over the frames of part [T, ...] (n values per frame)."""
    n = acc.numel()
    _eval_bufs("scale_fss_merge", (part, torch.int64, part.shape[0] * n), (acc, torch.int64, n))
    _hip.check(_hip.load().p2i_scale_fss_merge(_ptr(part), part.shape[0], n, _ptr(acc), _stream()), "p2i_scale_fss_merge")


def scale_spectra(pred, truth, ptl, gtl, S, lut, divide_by_3, tw, rings, G, psd, P, nanflag):
    """One aligned piece of T frames: P [T, 2, R] (fp64) = the ring means of the power spectra of the transformed S x S crops of pred
    (field 0) and truth (field 1), nanflag [T, 2] (int32, zeroed here) = 1 where a crop holds a NaN.  tw [2, S] = cos, sin(2 pi m /
    S); rings = (order, weight, offsets, count) as p2i_scale_rings takes them; G [T, 2, S, R, 2] and psd [T, 2, S, R] are workspace."""
    T, R = pred.shape[0], S // 2 + 1
    if truth.shape[0] != T or not 0 < S <= SCALE_MAX_CROP:
        raise RuntimeError("scale_spectra: frame count / crop")
    order, weight, offsets, count = rings
    _eval_bufs("scale_spectra", (lut, torch.float64, 256), (tw, torch.float64, 2 * S), (order, torch.int32, order.numel()),
               (weight, torch.float64, order.numel()), (offsets, torch.int32, R + 1), (count, torch.float64, R),
               (G, torch.float64, T * 4 * S * R), (psd, torch.float64, T * 2 * S * R), (P, torch.float64, T * 2 * R),
               (nanflag, torch.int32, T * 2))
    if not 0 < order.numel() <= S * R:
        raise RuntimeError("scale_spectra: ring list")
    nanflag.zero_()
    lib = _hip.load()
    for field, (x, tl) in enumerate(((pred, ptl), (truth, gtl))):
        _hip.check(lib.p2i_scale_dft_rows(_eval_input(x, tl), T, S, field, _ptr(lut), int(divide_by_3), _ptr(tw), _ptr(G), _ptr(nanflag),
                                          _stream()), "p2i_scale_dft_rows")
    _hip.check(lib.p2i_scale_dft_cols(_ptr(G), T, S, _ptr(tw), _ptr(psd), _stream()), "p2i_scale_dft_cols")
    _hip.check(lib.p2i_scale_rings(_ptr(psd), T, S, _ptr(order), _ptr(weight), _ptr(offsets), _ptr(count), R, _ptr(P), _stream()),
               "p2i_scale_rings")


def scale_spectrum_merge(P, nanflag):
    """P [T, 2, R], nanflag [T, 2] -> [2 * R + 1] fp64: the two mean spectra over the frames without a NaN (frame order), then the
    number of frames left out."""
    T, _, R = P.shape
    _eval_bufs("scale_spectrum_merge", (P, torch.float64, T * 2 * R), (nanflag, torch.int32, T * 2))
    out = torch.empty(2 * R + 1, device=P.device, dtype=torch.float64)
    _hip.check(_hip.load().p2i_scale_spectrum_merge(_ptr(P), _ptr(nanflag), T, R, _ptr(out), _stream()), "p2i_scale_spectrum_merge")
    return out


# ---- object-based verification: connected rain objects (csrc/eval_objects.hip; p2igan_bench/evaluation/objects.py drives these) ----
OBJECTS_LDS_CROP = 128
OBJECTS_TILE = 64


def _objects_labels(labels, wide, n):
    _eval_bufs("objects labels", (labels, torch.int32 if wide else torch.int16, n))


def objects_quantize(x, tl, field, S, lut, thresholds, sal_factor, sal_floor, divide_by_3, q, bits, rec):
    """Field 0 (prediction) / 1 (truth) of one aligned piece x [T, H, W]: q [T, 2, S * S] (int32 holding uint32) = rint(R * 2^24),
    bits [T, 2, S * S] (int16) = the level masks (bit j: threshold j; bit len(thresholds): the relative level), rec [T, 2, 5] (int64) =
    sum Q, sum Q y, sum Q x, max Q, NaN flag."""
    T, K = x.shape[0], len(thresholds)
    if field not in (0, 1) or not 0 < K <= EXP1_MAX_THR or not 0 < S <= SCALE_MAX_CROP:
        raise RuntimeError("objects_quantize: field / thresholds / crop")
    _eval_bufs("objects_quantize", (lut, torch.float64, 256), (q, torch.int32, T * 2 * S * S), (bits, torch.int16, T * 2 * S * S),
               (rec, torch.int64, T * 2 * 5))
    _hip.check(_hip.load().p2i_objects_quantize(_eval_input(x, tl), T, S, field, _ptr(lut), _f64s(thresholds), K, float(sal_factor),
                                                float(sal_floor), int(divide_by_3), _ptr(q), _ptr(bits), _ptr(rec), _stream()),
               "p2i_objects_quantize")


def objects_label(bits, T, S, nlev, connectivity, labels, wide):
    """labels [T, 2, nlev, S * S] (int16 holding uint16, or int32 holding uint32 when ``wide``) = the canonical object label of every
    set pixel, all ones elsewhere.  Not ``wide``: labels in LDS (S <= OBJECTS_LDS_CROP); ``wide``: tiles, border merge and flatten."""
    _eval_bufs("objects_label", (bits, torch.int16, T * 2 * S * S))
    _objects_labels(labels, wide, T * 2 * nlev * S * S)
    _hip.check(_hip.load().p2i_objects_label(_ptr(bits), T, S, nlev, int(connectivity), int(bool(wide)), _ptr(labels), _stream()),
               "p2i_objects_label")


def objects_count(labels, wide, q, T, S, nlev, lev, counts):
    """lev [T, 2, nlev, 5] (int64) = objects, area, sum Q, sum Q y, sum Q x over object pixels; counts [T * 2 * nlev] (int64)."""
    _objects_labels(labels, wide, T * 2 * nlev * S * S)
    _eval_bufs("objects_count", (q, torch.int32, T * 2 * S * S), (lev, torch.int64, T * 2 * nlev * 5), (counts, torch.int64, T * 2 * nlev))
    _hip.check(_hip.load().p2i_objects_count(_ptr(labels), int(bool(wide)), _ptr(q), T, S, nlev, _ptr(lev), _ptr(counts), _stream()),
               "p2i_objects_count")


def objects_scan(counts, offsets):
    """offsets [n + 1] (int64) = the exclusive prefix of counts [n] and, last, their total."""
    n = counts.numel()
    _eval_bufs("objects_scan", (counts, torch.int64, n), (offsets, torch.int64, n + 1))
    _hip.check(_hip.load().p2i_objects_scan(_ptr(counts), n, _ptr(offsets), _stream()), "p2i_objects_scan")


def objects_fill(labels, wide, q, T, S, nlev, offsets, table):
    """table [rows, 6] (int64, zeroed, rows = offsets[-1]): per record its objects in ascending label order as label, area, sum Q,
    max Q, sum Q y, sum Q x.  Overwrites labels."""
    rows = table.shape[0]
    _objects_labels(labels, wide, T * 2 * nlev * S * S)
    _eval_bufs("objects_fill", (q, torch.int32, T * 2 * S * S), (offsets, torch.int64, T * 2 * nlev + 1), (table, torch.int64, rows * 6))
    _hip.check(_hip.load().p2i_objects_fill(_ptr(labels), int(bool(wide)), _ptr(q), T, S, nlev, _ptr(offsets), rows,
                                            _ptr(table) if rows else None, _stream()), "p2i_objects_fill")


# ---- probabilistic verification of variance maps (csrc/eval_prob.hip; p2igan_bench/evaluation/prob.py drives these) ----
PROB_MAX_LEVELS = 8
PROB_MAX_EDGES = 16
PROB_MAX_PIT_BINS = 64
PROB_MAX_REL_BINS = 32
PROB_WG_PIXELS = 1024


def prob_record(nthr: int, nlevels: int, nedges: int, pit_bins: int, rel_bins: int):
    """(nf, ni): the fp64 and int64 word counts of a record for these sizes (layout: include/p2i_hip.h)."""
    nf, ni = C.c_int(0), C.c_int(0)
    _hip.check(_hip.load().p2i_prob_record(nthr, nlevels, nedges, pit_bins, rel_bins, C.byref(nf), C.byref(ni)), "p2i_prob_record")
    return int(nf.value), int(ni.value)


def prob_accumulate(pred, var, truth, ptl, vtl, gtl, rows, cols, rank, lut, thresholds, xq, halfwidths, edges, pit_bins, rel_bins,
                    censor, divide_by_3, part):
    """One aligned piece: pred, truth [T, H, W] (their own H, W) with crop origins ptl / gtl of the rows x cols crop; ``var`` is a
    third such input with origin vtl, or a float (one variance for every pixel).  rank [rows * cols] int32 or None (every pixel).
    Writes ceil(T * rows * cols / PROB_WG_PIXELS) records to part (fp64 words; the int64 sections travel as their bits)."""
    T = pred.shape[0]
    if truth.shape[0] != T or len(xq) != len(thresholds):
        raise RuntimeError("prob_accumulate: frame count / thresholds")
    pin, gin = _eval_input(pred, ptl), _eval_input(truth, gtl)
    if isinstance(var, torch.Tensor):
        if var.shape[0] != T:
            raise RuntimeError("prob_accumulate: the variance's frame count")
        vin, v0 = _eval_input(var, vtl), 0.0
    else:
        vin, v0 = None, float(var)
    nf, ni = prob_record(len(thresholds), len(halfwidths), len(edges), pit_bins, rel_bins)
    nwg = -(-T * rows * cols // PROB_WG_PIXELS)
    bufs = [(lut, torch.float64, 256), (part, torch.float64, nwg * (nf + ni))]
    if rank is not None:
        bufs.append((rank, torch.int32, rows * cols))
    _eval_bufs("prob_accumulate", *bufs)
    _hip.check(_hip.load().p2i_prob_accumulate(
        pin, vin, v0, gin, T, rows, cols, _ptr(rank) if rank is not None else None, _ptr(lut), _f64s(thresholds), _f64s(xq),
        len(thresholds), _f64s(halfwidths), len(halfwidths), _f64s(edges), len(edges), pit_bins, rel_bins, int(bool(censor)),
        int(divide_by_3), _ptr(part), part.numel(), _stream()), "p2i_prob_accumulate")


def prob_merge(part, nf, ni, acc):
    """acc [nf + ni] += the records of part (a multiple of nf + ni words), summed in a fixed order: fp64 words as fp64, the rest as int64."""
    if part.numel() == 0 or part.numel() % (nf + ni):
        raise RuntimeError("prob_merge: bad buffer")
    _eval_bufs("prob_merge", (part, torch.float64, part.numel()), (acc, torch.float64, nf + ni))
    _hip.check(_hip.load().p2i_prob_merge(_ptr(part), part.numel() // (nf + ni), nf, ni, _ptr(acc), _stream()), "p2i_prob_merge")


# ---- ensemble verification (csrc/eval_ens.hip, include/p2i_ens.h; p2igan_bench/evaluation/ensemble.py drives these) ----
ENS_MAX_MEMBERS = 64
ENS_MAX_OFFSETS = 16
ENS_WG_PIXELS = 256


def ens_abi_version() -> int:
    return int(_hip.load().p2i_ens_abi_version())


def ens_record(M: int, nthr: int, nedges: int):
    """(nf, ni): the fp64 and int64 word counts of a per-point record for M members (layout: include/p2i_ens.h)."""
    nf, ni = C.c_int(0), C.c_int(0)
    _hip.check(_hip.load().p2i_ens_record(M, nthr, nedges, C.byref(nf), C.byref(ni)), "p2i_ens_record")
    return int(nf.value), int(ni.value)


def _ens_inputs(what, members, origins, frame_stride, truth, gtl):
    """The member descriptors as one ctypes array, M, the stride and the truth's descriptor.  ``members`` are [T, h, w] views whose
    frames lie ``frame_stride`` elements apart (0: each member's own h * w, which needs contiguous members)."""
    M, T = len(members), truth.shape[0]
    if not 1 <= M <= ENS_MAX_MEMBERS or len(origins) != M:
        raise RuntimeError(f"{what}: 1 to {ENS_MAX_MEMBERS} members, one crop origin each")
    descs = (_hip.EvalInput * M)()
    for m, (x, tl) in enumerate(zip(members, origins)):
        if x.dim() != 3 or x.shape[0] != T or not x.is_cuda or x.dtype not in _EVAL_DTYPES:
            raise RuntimeError(f"{what}: member {m} is not a device [T, h, w] (uint8 / f32 / f64) of the truth's {T} frames")
        want = int(frame_stride) if frame_stride else x.shape[1] * x.shape[2]
        if x.stride(2) != 1 or x.stride(1) != x.shape[2] or (T > 1 and x.stride(0) != want):
            raise RuntimeError(f"{what}: member {m} has strides {tuple(x.stride())}, frame stride {want} expected")
        descs[m] = _hip.EvalInput(_ptr(x), _EVAL_DTYPES[x.dtype], x.shape[1], x.shape[2], int(tl[0]), int(tl[1]))
    return descs, M, int(frame_stride), _eval_input(truth, gtl)


def ens_points(members, origins, frame_stride, truth, gtl, rows, cols, box, rank, xq, edges, part):
    """One piece of T frames at one box size: writes ceil(T * (rows // box) * (cols // box) / ENS_WG_PIXELS) records to part (fp64
    words; the int64 sections travel as their bits)."""
    descs, M, fs, gin = _ens_inputs("ens_points", members, origins, frame_stride, truth, gtl)
    nf, ni = ens_record(M, len(xq), len(edges))
    nwg = -(-truth.shape[0] * (rows // box) * (cols // box) // ENS_WG_PIXELS)
    bufs = [(part, torch.float64, nwg * (nf + ni))]
    if rank is not None:
        bufs.append((rank, torch.int32, rows * cols))
    _eval_bufs("ens_points", *bufs)
    _hip.check(_hip.load().p2i_ens_points(descs, M, fs, gin, truth.shape[0], rows, cols, box, _ptr(rank) if rank is not None else None,
                                          _f64s(xq), len(xq), _f64s(edges), len(edges), _ptr(part), part.numel(), _stream()),
               "p2i_ens_points")


def ens_energy(members, origins, frame_stride, truth, gtl, rows, cols, rank, out):
    """out [T, 4] f64: per frame (d, ES, ES_fair, the mean distance to the truth) over the valid pixels."""
    descs, M, fs, gin = _ens_inputs("ens_energy", members, origins, frame_stride, truth, gtl)
    bufs = [(out, torch.float64, truth.shape[0] * 4)]
    if rank is not None:
        bufs.append((rank, torch.int32, rows * cols))
    _eval_bufs("ens_energy", *bufs)
    _hip.check(_hip.load().p2i_ens_energy(descs, M, fs, gin, truth.shape[0], rows, cols, _ptr(rank) if rank is not None else None,
                                          _ptr(out), _stream()), "p2i_ens_energy")


def ens_variogram(members, origins, frame_stride, truth, gtl, rows, cols, rank, offsets, out):
    """out [T, len(offsets), 2] f64: per frame and offset (dy, dx) the pair (V_o, n_o)."""
    descs, M, fs, gin = _ens_inputs("ens_variogram", members, origins, frame_stride, truth, gtl)
    flat = [int(v) for o in offsets for v in o]
    if len(flat) != 2 * len(offsets):
        raise RuntimeError("ens_variogram: offsets are (dy, dx) pairs")
    bufs = [(out, torch.float64, truth.shape[0] * len(offsets) * 2)]
    if rank is not None:
        bufs.append((rank, torch.int32, rows * cols))
    _eval_bufs("ens_variogram", *bufs)
    _hip.check(_hip.load().p2i_ens_variogram(descs, M, fs, gin, truth.shape[0], rows, cols, _ptr(rank) if rank is not None else None,
                                             (C.c_int * max(1, len(flat)))(*flat), len(offsets), _ptr(out), _stream()),
               "p2i_ens_variogram")
