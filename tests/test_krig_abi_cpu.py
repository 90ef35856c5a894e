"""The nine dense kriging stages take their chunk of systems as one p2i_krig_systems descriptor (ABI v3).  Every argument check returns
before the first HIP call, so the built library answers all of this without a GPU: the pointers below are host buffers that nothing
dereferences before the refusal under test."""
import ctypes as C
import os
import re

import pytest

from p2igan_bench import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_buf = (C.c_double * 64)()
P = C.addressof(_buf)            # stands for every buffer
POINTERS = ("pix", "z", "counts", "params", "cand", "status")
MODEL = "variogram model must be 0 (exponential) or 1 (spherical)"
RANGE, SPAN = "bad system range", "a system spans one frame or one whole sample"
ONE_SAMPLE = "a space-time system is one sample: R = T = 1"

# entry point -> (its arguments after the descriptor, the pointer fields it reads (cand: NULL allowed wherever read), whether it checks
#                 model and reads np, the check after the null pointers: (descriptor fields or argument positions to set, its message))
# An argument position is a digit string, counted after the descriptor.
CALLS = {
    "p2i_krig_factor": ((P,), ("pix", "counts", "params", "status"), True, True, ({"model": 2}, MODEL)),
    "p2i_krig_solve": ((P, P, P, P), ("z", "counts", "status"), False, True, ({"nsys": 0}, RANGE)),
    "p2i_krig_predict": ((P, P, 8, 8, P), ("pix", "counts", "params"), True, False, ({"2": 0}, "bad frame shape")),
    "p2i_krig_variance": ((P, P, 8, 8, P), ("pix", "counts", "params", "status"), True, True, ({"2": 0}, "bad frame shape")),
    "p2i_krig_loo": ((P, P, P, P, P, P), ("z", "counts", "status"), False, True, ({"nsys": 0}, RANGE)),
    "p2i_krig_cs_weights": ((P, P, P, 4, 8, 8, P, P), ("pix", "z", "counts", "status"), False, True, ({"3": 0}, "members must be in 1..64 (got 0)")),
    "p2i_krig_cs_predict": ((P, P, 4, 8, 8, P), ("pix", "z", "counts", "params", "status"), True, True, ({"2": 0}, "members must be in 1..64 (got 0)")),
    "p2i_stkrig_factor": ((P, None, P), ("pix", "counts", "params", "status"), True, True, ({"model": 2}, MODEL)),
    "p2i_stkrig_loso": ((P, P, P, P, P, P, 4, 8, P, P), ("z", "counts", "status"), False, True,
                        ({"6": 33}, "a site block is at most 32 frames wide (got T = 33)")),
}
SPACE_TIME = ("p2i_stkrig_factor", "p2i_stkrig_loso")


def _sys(**fields):
    d = dict({n: P for n in POINTERS}, model=0, f0=0, R=1, T=1, nsys=1, np=32, cap=64)
    d.update(fields)
    return _hip.KrigSystems(**d)


def _refused(name, desc=True, later=False, **fields):
    """The message `name` refuses with: desc None is the NULL descriptor; string keys set descriptor fields, digit keys arguments;
    later: with the entry point's next check armed, for a call that is to pass the null-pointer check."""
    lib = _hip.load()
    args = list(CALLS[name][0])
    fields = dict(CALLS[name][4][0] if later else {}, **{str(k): v for k, v in fields.items()})
    for k in [k for k in fields if k.isdigit()]:
        args[int(k)] = fields.pop(k)
    assert getattr(lib, name)(None if desc is None else C.byref(_sys(**fields)), *args, None) == -1, f"{name} took {fields}"   # P2I_EINVAL
    return lib.p2i_last_error().decode()


def _arg(k, v):
    return {str(k): v}


def test_layout_and_parameter_counts():
    """The constants of csrc/krig_common.h's static_assert; 150 parameters before the descriptor."""
    assert C.sizeof(_hip.KrigSystems) == 80
    offsets = [getattr(_hip.KrigSystems, n).offset for n, _ in _hip.KrigSystems._fields_]
    assert [n for n, _ in _hip.KrigSystems._fields_] == list(POINTERS) + ["model", "f0", "R", "T", "nsys", "np", "cap"]
    assert offsets == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72]
    src = open(os.path.join(ROOT, "p2i-gan-benchmark_amd", "csrc", "krig_common.h")).read()
    m = re.search(r"static_assert\((sizeof\(p2i_krig_systems\).*?),\s*\"", src, re.S)
    assert m and [int(v) for v in re.findall(r"== (\d+)", m.group(1))] == [80] + offsets
    assert len(CALLS) == 9 and sum(len(_hip.SIGNATURES[n]) for n in CALLS) == 66
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2i_hip.h")).read(), flags=re.S)
    for name, (args, *_) in CALLS.items():
        proto = re.search(rf"\bint {name}\s*\(([^;]*)\);", header)
        assert proto and proto.group(1).split(",")[0].strip() == "const p2i_krig_systems* sys", name
        assert len(proto.group(1).split(",")) == len(_hip.SIGNATURES[name]) == len(args) + 2, name
    assert _hip.load().p2i_abi_version() == 4


@pytest.mark.parametrize("name", CALLS)
def test_null_descriptor_and_needed_fields_are_refused(name):
    reads, nxt = CALLS[name][1], CALLS[name][4][1]
    assert _refused(name, None) == "null pointer"
    for field in POINTERS:        # a field that is not read (or cand) may be NULL: the call goes on to the next check
        assert _refused(name, later=True, **{field: None}) == ("null pointer" if field in reads else nxt), field
    assert _refused(name, later=True, **{f: None for f in POINTERS if f not in reads}) == nxt
    for k, a in enumerate(CALLS[name][0]):
        if a == P:                # the entry point's own pointers
            assert _refused(name, **_arg(k, None)) == "null pointer", k


@pytest.mark.parametrize("name", CALLS)
def test_range_is_refused_one_field_at_a_time(name):
    """With the messages the loose arguments had."""
    for bad in ({"f0": -1}, {"nsys": 0}, {"nsys": 65536}, {"R": 0}, {"T": 0}):
        assert _refused(name, **bad) == RANGE, bad
    assert _refused(name, R=2, T=4) == SPAN
    assert _refused(name, R=4, T=4, f0=2) == SPAN
    assert _refused(name, cap=4128) == "padded size 32 must be a multiple of 32 within cap 4128"
    for np_, cap in ((33, 64), (0, 64), (64, 32)):
        if CALLS[name][3]:
            assert _refused(name, np=np_, cap=cap) == f"padded size {np_} must be a multiple of 32 within cap {cap}"
        else:                     # p2i_krig_predict does not read np: one tile stands in, and the call stops at its own limit
            assert _refused(name, np=np_, cap=cap, R=1 << 19, T=1 << 19) == "too many frames per set"
    if name in SPACE_TIME:
        assert _refused(name, R=4, T=4, f0=4) == ONE_SAMPLE


@pytest.mark.parametrize("name", CALLS)
def test_exchanged_r_and_t_are_refused(name):
    """T = 4, R = 1, f0 = 2 is frame 2 of a per-frame call; read with R and T exchanged, R is neither 1 nor T."""
    assert _refused(name, R=4, T=1, f0=2) == SPAN
    if name.startswith("p2i_krig_cs_"):      # these have a check after the range: the descriptor as meant passes the range
        assert _refused(name, later=True, R=1, T=4, f0=2) == CALLS[name][4][1]


@pytest.mark.parametrize("name", CALLS)
def test_bad_model_is_refused_where_it_is_read(name):
    for model in (-1, 2):
        assert _refused(name, later=True, model=model) == (MODEL if CALLS[name][2] else CALLS[name][4][1]), model
