"""The convolution entry points take what the bf16-split pipe may use as one p2i_conv_split descriptor and the weight gradient's
slice scratch as plain arguments (ABI v4): no twin entry points, no call-to-call state.  Every argument check below returns before
the first HIP call, so the built library answers all of this without a GPU: the pointers are host buffers that nothing dereferences
before the refusal under test."""
import ctypes as C
import glob
import os
import re

import pytest

from p2igan_bench import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p2i-gan-benchmark_amd", "csrc")
_buf = (C.c_double * 64)()
P = C.addressof(_buf)            # stands for every buffer
CHANGED = {"p2i_conv_fwd": 9, "p2i_conv_dgrad": 11, "p2i_conv_wgrad": 10, "p2i_idw_fwd": 20, "p2i_weight_unpack_grad_batched": 13,
           "p2i_upmod_fwd": 10}
REMOVED = ("p2i_conv_fwd_x6", "p2i_conv_fwd_x6s", "p2i_conv_dgrad_x6", "p2i_conv_dgrad_x6s", "p2i_conv_wgrad_ws",
           "p2i_x6_next_source_planes", "p2i_idw_fwd_ws", "p2i_weight_unpack_grad_batched_acc", "p2i_upmod_fwd_ba")


def _desc(**over):
    """3x3 stride-1 pad-1 2-D layer, 32 -> 32 channels, B = 2, 16 x 16: one the split pipe takes with P2I_X6C_MIN_WG=1"""
    f = dict(B=2, Cin=32, Cout=32, Ti=1, Hi=16, Wi=16, To=1, Ho=16, Wo=16, kt=1, kh=3, kw=3, st=1, sh=1, sw=1, pt=0, ph=1, pw=1)
    f.update(over)
    return _hip.ConvDesc(**f)


def _fwd(d, x=P, wp=P, sp=None, y=P):
    return _hip.load().p2i_conv_fwd(d, x, wp, sp, None, None, y, _hip.ACT_NONE, None)


def _dgrad(d, dy=P, y_act=None, wp_d=P, sp=None, mask_y=None, dx=P):
    return _hip.load().p2i_conv_dgrad(d, dy, y_act, _hip.ACT_RELU, wp_d, sp, None, mask_y, _hip.ACT_RELU, dx, None)


def _wgrad(d, x=P, dy=P, dwp=P, ws=None, ws_floats=0):
    return _hip.load().p2i_conv_wgrad(d, x, dy, None, _hip.ACT_NONE, dwp, None, ws, ws_floats, None)


def _err():
    return _hip.load().p2i_last_error().decode()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2i_hip.h")).read(), flags=re.S)


def test_split_descriptor_layout():
    """The constants of csrc/conv_common.h's static_assert."""
    names = [n for n, _ in _hip.ConvSplit._fields_]
    assert names == ["w_split", "w_scratch", "src_planes", "w_split_taps"]
    offsets = [getattr(_hip.ConvSplit, n).offset for n in names]
    assert C.sizeof(_hip.ConvSplit) == 32 and offsets == [0, 8, 16, 24]
    src = open(os.path.join(CSRC, "conv_common.h")).read()
    m = re.search(r"static_assert\((sizeof\(p2i_conv_split\).*?),\s*\"", src, re.S)
    assert m and [int(v) for v in re.findall(r"== (\d+)", m.group(1))] == [32] + offsets
    body = re.search(r"typedef struct p2i_conv_split \{(.*?)\} p2i_conv_split;", _header(), re.S).group(1)
    assert re.findall(r"(\w+);", body) == names


def test_changed_signatures_and_removed_names():
    header = _header()
    for name, n in CHANGED.items():
        proto = re.search(rf"\bint {name}\s*\(([^;]*)\);", header)
        assert proto and len(proto.group(1).split(",")) == len(_hip.SIGNATURES[name]) == n, name
    assert _hip.SIGNATURES["p2i_conv_fwd"][3] is _hip.SIGNATURES["p2i_conv_dgrad"][5] is C.POINTER(_hip.ConvSplit)
    lib = _hip.load()
    for name in REMOVED:
        assert not re.search(rf"\b{name}\b", header) and name not in _hip.SIGNATURES and not hasattr(lib, name), name
    assert len(_hip.SIGNATURES) == 134
    assert lib.p2i_abi_version() == 4


@pytest.mark.parametrize("call", [_fwd, _dgrad, _wgrad], ids=["fwd", "dgrad", "wgrad"])
def test_bad_descriptor_is_refused(call):
    assert call(None) == -1 and _err() == "null conv desc"
    for bad, msg in (({"B": 0}, "bad channel/batch dims"), ({"kt": 4}, "kernel taps > 27"), ({"sh": 0}, "bad stride"),
                     ({"To": 2}, "To inconsistent"), ({"Ho": 15}, "Ho inconsistent"), ({"Wo": 17}, "Wo inconsistent"),
                     ({"B": 1 << 16, "Cin": 1 << 8}, "tensor too large for 32-bit indexing")):
        assert call(_desc(**bad)) == -1 and _err() == msg, bad


@pytest.mark.parametrize("sp", [None, _hip.ConvSplit(None, None, None, 0), _hip.ConvSplit(None, None, P, 0), _hip.ConvSplit(P, None, None, 9)],
                         ids=["null", "empty", "planes_only", "w_split"])
def test_null_pointers_are_refused(sp, monkeypatch):
    """With no weight split in the descriptor, and with a pre-split image (nothing is launched for it)."""
    monkeypatch.setenv("P2I_X6C_MIN_WG", "1")
    d = _desc()
    for arg in ("x", "wp", "y"):
        assert _fwd(d, sp=sp, **{arg: None}) == -1 and _err() == "null pointer", arg
    for arg in ("dy", "wp_d", "dx"):
        assert _dgrad(d, sp=sp, **{arg: None}) == -1 and _err() == "null pointer", arg
    for arg in ("x", "dy", "dwp"):
        assert _wgrad(d, **{arg: None}) == -1 and _err() == "null pointer", arg


def test_split_descriptor_refusals(monkeypatch):
    """A pre-split image with fewer taps than the layer; a scratch without weights to split into it (refused before the split is
    launched).  A layer the split pipe declines (24 channels) does not look at either."""
    monkeypatch.setenv("P2I_X6C_MIN_WG", "1")
    d = _desc()
    assert _hip.load().p2i_x6c_would_take(d, 0, 0) == 1 and _hip.load().p2i_x6c_would_take(d, 1, 0) == 1
    short, scratch = _hip.ConvSplit(P, P, None, 8), _hip.ConvSplit(None, P, None, 0)
    assert _fwd(d, sp=short) == -1 and _err() == "ntaps_w smaller than the layer's tap count"
    assert _dgrad(d, sp=short) == -1 and _err() == "ntaps_w smaller than the layer's tap count"
    assert _fwd(d, wp=None, sp=scratch) == -1 and _err() == "null pointer"
    assert _dgrad(d, wp_d=None, sp=scratch) == -1 and _err() == "null pointer"
    d24 = _desc(Cin=24, Cout=24)
    assert _fwd(d24, x=None, sp=short) == -1 and _err() == "null pointer"
    assert _dgrad(d24, dx=None, sp=short) == -1 and _err() == "null pointer"


@pytest.mark.parametrize("sp", [None, _hip.ConvSplit(P, None, None, 8)], ids=["null", "short_w_split"])
def test_dgrad_mask_with_prologue_is_refused(sp, monkeypatch):
    """... and a call with the act'(y) prologue ignores the split descriptor: its short image is not looked at."""
    monkeypatch.setenv("P2I_X6C_MIN_WG", "1")
    assert _dgrad(_desc(), y_act=P, mask_y=P, sp=sp) == -1
    assert _err() == "dgrad: use either the act'(y) prologue or the epilogue mask"


def test_no_hidden_arguments_in_the_library():
    """What a convolution call computes stands in its argument list: the thread-local context of the old twin entry points is gone,
    thread_local holds outputs and process state only, and no entry point of conv.hip / wgrad.hip calls a public convolution."""
    tls = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        src = open(path).read()
        for gone in ("X6Ctx", "x6_ctx", "g_wgrad_ws", "g_next_splanes"):
            assert gone not in src, (gone, path)
        for m in re.finditer(r"thread_local[^;=]*?(\w+)\s*(?:\[[^\]]*\])*\s*(?:=|;)", src):
            tls.setdefault(os.path.basename(path), []).append(m.group(1))
    assert tls == {"conv.hip": ["g_last_plan"], "wgrad.hip": ["g_wgrad_plan"], "weights.hip": ["g_err"],
                   "tape.hip": ["g_rec", "g_events", "g_event_ok"]}
    for name in ("conv.hip", "wgrad.hip"):
        src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
        defs = list(re.finditer(r'extern "C" int (\w+)\s*\(', src))
        assert defs
        for m, nxt in zip(defs, defs[1:] + [None]):
            body = src[m.end():nxt.start() if nxt else len(src)]
            assert not re.search(r"\bp2i_conv_\w+\s*\(", body), (name, m.group(1))
