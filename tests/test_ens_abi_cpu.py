"""The ensemble-verification entry points of include/p2i_ens.h: exported, bound through _hip.ENS_SIGNATURES, versioned on their own,
and every argument check returns before the first HIP call, so the built library answers all of this without a GPU: the pointers
below are host buffers that nothing dereferences before the refusal under test."""
import ctypes as C
import os
import re

import pytest

from p2igan_bench import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, ROWS, COLS = 2, 3, 4          # frames; the crop
H, W = 4, 8                      # every input's extent: H != W, so that a transposed reading shows
F32, F64 = 1, 2

_buf = (C.c_double * 64)()
P = C.addressof(_buf)            # stands for every buffer
ONE = (C.c_double * 1)(1.0)
OFF = (C.c_int * 40)(*([0, 1] * 20))


def _input(top=0, left=0, dtype=F32, data=P, h=H, w=W):
    return _hip.EvalInput(data, dtype, h, w, top, left)


def _members(M, special=None, at=0):
    arr = (_hip.EvalInput * max(M, 1))()
    for m in range(M):
        arr[m] = _input()
    if special is not None:
        arr[at] = special
    return arr


def _points(members, M, truth, stride=0, box=1):
    return (members, M, stride, truth, T, ROWS, COLS, box, None, ONE, 1, ONE, 1, P, 1 << 20, None)


def _energy(members, M, truth, stride=0):
    return (members, M, stride, truth, T, ROWS, COLS, None, P, None)


def _variogram(members, M, truth, stride=0, nof=2):
    return (members, M, stride, truth, T, ROWS, COLS, None, OFF, nof, P, None)


CALLS = {"p2i_ens_points": _points, "p2i_ens_energy": _energy, "p2i_ens_variogram": _variogram}


def _refused(name, *args, **kw):
    lib = _hip.load()
    assert getattr(lib, name)(*CALLS[name](*args, **kw)) == -1, f"{name} took {args} {kw}"        # P2I_EINVAL
    return lib.p2i_last_error().decode()


def test_every_declared_name_is_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2i_ens.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\bint (p2i_[a-z0-9_]+)\s*\(([^;]*)\);", header))
    assert sorted(protos) == sorted(_hip.ENS_SIGNATURES) and len(protos) == 5
    lib = C.CDLL(_hip.lib_path())
    for name, args in protos.items():
        assert hasattr(lib, name), name
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert len(_hip.ENS_SIGNATURES[name]) == count, name
    assert not set(_hip.ENS_SIGNATURES) & set(_hip.SIGNATURES)
    assert '#include "p2i_hip.h"' in header


def test_versions():
    lib = _hip.load()
    assert lib.p2i_ens_abi_version() == 1


def test_record_sizes():
    lib = _hip.load()
    nf, ni = C.c_int(0), C.c_int(0)
    assert lib.p2i_ens_record(5, 2, 3, C.byref(nf), C.byref(ni)) == 0
    assert (nf.value, ni.value) == (6 + 2 * 2 + 2 * 4, 2 + 2 + 7 + 4 + 2 * 2 * 6)
    for M, nthr, nedges in ((0, 1, 1), (65, 1, 1), (4, 9, 1), (4, 1, 17)):
        assert lib.p2i_ens_record(M, nthr, nedges, C.byref(nf), C.byref(ni)) == -1
        assert lib.p2i_last_error().decode() == "bad arguments"


@pytest.mark.parametrize("name", list(CALLS))
@pytest.mark.parametrize("M", [1, 3, 64])
def test_crop_outside_is_refused_per_input(name, M):
    """One axis at a time: rows 2 .. 4 of 4 are one too low, columns 5 .. 8 of 8 one too far right; for member 0, for member M - 1
    and for the truth."""
    for top, left in ((2, 0), (0, 5)):
        for at in sorted({0, M - 1}):
            assert _refused(name, _members(M, _input(top, left), at), M, _input()) == f"crop outside member {at}"
        assert _refused(name, _members(M), M, _input(top, left)) == "crop outside the truth"
    # (1, 4) lies inside 4 x 8 and the call goes on to a later check; read transposed it would lie outside
    assert _refused(name, _members(M, _input(1, 4), M - 1), M, _input(1, 4), stride=-1) == "bad frame stride"


@pytest.mark.parametrize("name", list(CALLS))
def test_bad_descriptors_are_refused(name):
    M = 3
    assert _refused(name, None, M, _input()) == "bad arguments"
    assert _refused(name, _members(M), M, None) == "bad arguments"
    assert _refused(name, _members(M), M, _input(data=None)) == "bad arguments"
    for at in (0, M - 1):
        assert _refused(name, _members(M, _input(data=None), at), M, _input()) == "bad arguments"
        assert _refused(name, _members(M, _input(dtype=3), at), M, _input()) == "unsupported dtype"
    assert _refused(name, _members(M), M, _input(dtype=3)) == "unsupported dtype"


@pytest.mark.parametrize("name", list(CALLS))
def test_member_count_is_bounded(name):
    for M in (0, 65, -1):
        assert _refused(name, _members(65), M, _input()) == "1 to 64 members"


def test_offset_count_is_bounded():
    for nof in (0, 17):
        assert _refused("p2i_ens_variogram", _members(2), 2, _input(), nof=nof) == "1 to 16 offsets"
    zero = (C.c_int * 4)(0, 1, 0, 0)
    lib = _hip.load()
    assert lib.p2i_ens_variogram(_members(2), 2, 0, _input(), T, ROWS, COLS, None, zero, 2, P, None) == -1
    assert lib.p2i_last_error().decode() == "an offset is not (0, 0)"


@pytest.mark.parametrize("name", list(CALLS))
def test_frame_stride_rules(name):
    """A stride other than h * w needs members of one dtype, h and w, and is no less than h * w."""
    M, msg = 3, "a frame stride other than h * w needs members of one dtype, h and w, and is at least h * w"
    assert _refused(name, _members(M, _input(dtype=F64), 1), M, _input(), stride=M * H * W) == msg
    assert _refused(name, _members(M, _input(h=H + 1), 2), M, _input(), stride=M * (H + 1) * W) == msg
    assert _refused(name, _members(M), M, _input(), stride=H * W - 1) == msg
    # accepted strides reach the next check (points: the box size; the others have none left, so only points is asked)
    if name == "p2i_ens_points":
        for stride in (0, H * W, M * H * W):
            assert _refused(name, _members(M), M, _input(), stride=stride, box=0) == "a box size lies in 1 .. min(rows, cols)"
        assert _refused(name, _members(M, _input(dtype=F64), 1), M, _input(), stride=H * W, box=4).startswith("a box size")
