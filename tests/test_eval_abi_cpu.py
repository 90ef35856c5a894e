"""The evaluation entry points take each input as one p2i_eval_input descriptor, and the space-time kriging stages have one entry
point each.  Every argument check returns before the first HIP call, so the built library answers all of this without a GPU: the
pointers below are host buffers that nothing dereferences before the refusal under test."""
import ctypes as C
import os
import re

import pytest

from p2igan_bench import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, S = 2, 4                      # frames; the crop is S x S (prob: rows = cols = S)
H, W = 4, 8                      # every input's extent: H != W, so that a transposed reading shows
U8, F32, F64 = 0, 1, 2

_buf = (C.c_double * 64)()
P = C.addressof(_buf)            # stands for every buffer that is not an input
ONE = (C.c_double * 1)(1.0)
ONE_I = (C.c_int * 1)(1)


def _input(top=0, left=0, dtype=F32, data=P, h=H, w=W):
    return _hip.EvalInput(data, dtype, h, w, top, left)


def _exp1(i, nsel=0):
    return (i["pred"], i["truth"], T, S, 1, P, nsel, P, ONE, 1, 1, P, P, P, P, P, None)


def _exp3(i):
    return (i["pred"], i["truth"], T, S, P, P, 1, P, P, P, None)


def _exp3_hist(i):
    return (i["truth"], T, S, P, 1, P, None)


def _exp3_gather(i):
    return (i["pred"], i["truth"], T, S, P, 1, P, 0, P, 1, P, P, None)


def _exp2(i):
    return (i["in"], T, S, 1, P, P, 1, P, None)


def _fss(i, nthr=1):
    return (i["pred"], i["truth"], T, S, P, ONE, nthr, ONE_I, 1, 1, None, P, None)


def _dft(i):
    return (i["in"], T, S, 0, P, 1, P, P, P, None)


def _prob(i, pit_bins=8):
    return (i["pred"], i["var"], 1.0, i["truth"], T, S, S, None, P, ONE, ONE, 1, ONE, 1, ONE, 1, pit_bins, 4, 0, 1, P, 1 << 20, None)


def _objects(i, nthr=1):
    return (i["in"], T, S, 0, P, ONE, nthr, 0.5, 0.0, 1, P, P, P, None)


PRED, TRUTH, VAR, IN = "crop outside the prediction", "crop outside the truth", "crop outside the variance", "crop outside the input"
# entry point -> (argument builder, {input: its crop message}, text for a missing input, text for a bad dtype,
#                 a later check to stop at: (builder keywords, the start of its message) or None)
CALLS = {
    "p2i_exp1_accumulate": (_exp1, {"pred": PRED, "truth": TRUTH}, "bad arguments", "unsupported dtype", ({"nsel": S * S + 1}, "bad selection")),
    "p2i_exp3_accumulate": (_exp3, {"pred": PRED, "truth": TRUTH}, "bad arguments", "unsupported dtype", None),
    "p2i_exp3_truth_hist": (_exp3_hist, {"truth": TRUTH}, "bad arguments", "bad arguments", None),
    "p2i_exp3_gather": (_exp3_gather, {"pred": PRED, "truth": TRUTH}, "bad arguments", "unsupported dtype", None),
    "p2i_exp2_index": (_exp2, {"in": IN}, "bad arguments", "bad arguments", None),
    "p2i_scale_fss": (_fss, {"pred": PRED, "truth": TRUTH}, "bad arguments", "unsupported dtype", ({"nthr": 0}, "1 to 8 thresholds")),
    "p2i_scale_dft_rows": (_dft, {"in": IN}, "bad arguments", "bad arguments", None),
    "p2i_prob_accumulate": (_prob, {"pred": PRED, "var": VAR, "truth": TRUTH}, "bad arguments", "unsupported dtype",
                            ({"pit_bins": 65}, "at most 8 thresholds, 8 levels, 16 edges, 64 PIT bins")),
    "p2i_objects_quantize": (_objects, {"in": IN}, "bad arguments", "bad arguments", ({"nthr": 0}, "1 to 8 thresholds")),
}
INPUTS = [(name, which) for name, spec in CALLS.items() for which in spec[1]]
TWINS = ("p2i_lagkrig_bins", "p2i_lagkrig_factor", "p2i_lagkrig_predict", "p2i_lkrig_predict_lag", "p2i_lkrig_loso_lag")


def _refused(name, which, desc, **kw):
    """The message entry point `name` refuses with when its input `which` is `desc` and its other inputs are valid."""
    lib = _hip.load()
    build, inputs = CALLS[name][:2]
    args = build({k: desc if k == which else _input() for k in inputs}, **kw)
    assert getattr(lib, name)(*args) == -1, f"{name} took {which} = {desc}"       # P2I_EINVAL
    return lib.p2i_last_error().decode()


def test_layout_is_the_c_struct():
    """The constants of csrc/eval_common.h's static_assert."""
    assert C.sizeof(_hip.EvalInput) == 32
    assert [(n, getattr(_hip.EvalInput, n).offset) for n, _ in _hip.EvalInput._fields_] == [
        ("data", 0), ("dtype", 8), ("h", 12), ("w", 16), ("top", 20), ("left", 24)]
    src = open(os.path.join(ROOT, "p2i-gan-benchmark_amd", "csrc", "eval_common.h")).read()
    m = re.search(r"static_assert\((sizeof\(p2i_eval_input\).*?),\s*\"", src, re.S)
    assert m and [int(v) for v in re.findall(r"== (\d+)", m.group(1))] == [32, 0, 8, 12, 16, 20, 24]
    assert len(INPUTS) == 15 and sum(len(_hip.SIGNATURES[n]) for n in CALLS) == 117


@pytest.mark.parametrize("name,which", INPUTS)
def test_crop_outside_is_refused_per_input(name, which):
    """One axis at a time: rows 1 .. 4 of 4, then columns 5 .. 8 of 8."""
    for top, left in ((1, 0), (0, 5)):
        assert _refused(name, which, _input(top, left)) == CALLS[name][1][which]


@pytest.mark.parametrize("name,which", [(n, w) for n, w in INPUTS if CALLS[n][4]])
def test_crop_inside_reaches_the_next_check(name, which):
    """(top, left) = (0, 4) lies inside 4 x 8 and the call stops at a later check; read with h / w or top / left exchanged it lies
    outside, as (4, 0) does."""
    kw, later = CALLS[name][4]
    assert _refused(name, which, _input(0, 4), **kw).startswith(later)
    assert _refused(name, which, _input(4, 0), **kw) == CALLS[name][1][which]


@pytest.mark.parametrize("name,which", INPUTS)
def test_bad_descriptor_is_refused(name, which):
    _, _, missing, bad_dtype, later = CALLS[name]
    assert _refused(name, which, _input(dtype=3)) == bad_dtype
    for desc in (None, _input(data=None)):
        if which == "var":       # no variance array means var_scalar: the call goes on to the later check
            assert _refused(name, which, desc, **later[0]).startswith(later[1])
        else:
            assert _refused(name, which, desc) == missing


def test_lagrangian_twins_are_gone():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2i_hip.h")).read(), flags=re.S)
    lib = C.CDLL(_hip.lib_path())
    for name in TWINS:
        assert not re.search(rf"\b{name}\b", header) and not hasattr(lib, name) and name not in _hip.SIGNATURES
    for name, vel in (("p2i_stkrig_bins", "const double* vel"), ("p2i_stkrig_factor", "const float* velf"),
                      ("p2i_stkrig_predict", "const float* velf"), ("p2i_lkrig_predict", "const float* velf"),
                      ("p2i_lkrig_loso", "const float* velf")):
        proto = re.search(rf"\bint {name}\s*\(([^;]*)\);", header)
        assert proto and vel in [" ".join(a.split()) for a in proto.group(1).split(",")] and hasattr(lib, name)
        assert len(proto.group(1).split(",")) == len(_hip.SIGNATURES[name])
    assert len(set(re.findall(r"\b(p2i_[a-z0-9_]+)\s*\(", header))) == 136 and len(_hip.SIGNATURES) == 134
