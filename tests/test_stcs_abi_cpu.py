"""The space-time conditional simulation's entry points of include/p2i_stcs.h: exported, bound through _hip.STCS_SIGNATURES, versioned
on their own, and every argument check returns before the first HIP call, so the built library answers all of this without a GPU: the
pointers below are host buffers that nothing dereferences before the refusal under test."""
import ctypes as C
import os
import re

import pytest

from p2igan_bench import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, W = 3, 17, 23                 # a sample
ST, SY, SX = 6, 34, 46              # its torus at embed = embed_time = 2
M = 5

_buf = (C.c_double * 64)()
P = C.addressof(_buf)               # stands for every buffer


def _sys(**kw):
    f = dict(pix=P, z=P, counts=P, params=P, cand=None, status=P, model=0, f0=0, R=1, T=1, nsys=1, np=32, cap=32)
    f.update(kw)
    return C.byref(_hip.KrigSystems(*[f[n] for n in "pix z counts params cand status model f0 R T nsys np cap".split()]))


def _spectrum(St=ST, Sy=SY, Sx=SX, B=1, model=0, params=P, work=P):
    return (params, None, model, B, St, Sy, Sx, P, work, P, P, None)


def _noise(St=ST, Sy=SY, Sx=SX, q0=0, npairs=1, xi=P):
    return (1, 2, q0, npairs, St, Sy, Sx, xi, None)


def _fields(members=M, t=T, h=H, w=W, St=ST, Sy=SY, Sx=SX, nunits=1, stages=7, amp=P, ens=P):
    return (amp, P, P, P, P, 1, 0, nunits, members, t, h, w, St, Sy, Sx, stages, P, P, ens, None)


def _weights(k=None, members=M, t=T, h=H, w=W, stt=P):
    return (_sys() if k is None else k, stt, P, P, P, members, t, h, w, P, P, None)


def _predict(k=None, members=M, t=T, h=H, w=W, stt=P):
    return (_sys() if k is None else k, stt, P, P, members, t, h, w, P, None)


CALLS = {"p2i_stcs_spectrum": _spectrum, "p2i_stcs_noise": _noise, "p2i_stcs_fields": _fields, "p2i_stcs_weights": _weights,
         "p2i_stcs_predict": _predict}


def _refused(name, **kw):
    lib = _hip.load()
    assert getattr(lib, name)(*CALLS[name](**kw)) == -1, f"{name} took {kw}"        # P2I_EINVAL
    return lib.p2i_last_error().decode()


def test_every_declared_name_is_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2i_stcs.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\bint (p2i_[a-z0-9_]+)\s*\(([^;]*)\);", header))
    assert sorted(protos) == sorted(_hip.STCS_SIGNATURES) and len(protos) == 6
    assert sorted(set(protos) - {"p2i_stcs_abi_version"}) == sorted(CALLS)
    lib = C.CDLL(_hip.lib_path())
    for name, args in protos.items():
        assert hasattr(lib, name), name
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert len(_hip.STCS_SIGNATURES[name]) == count, name
    assert not set(_hip.STCS_SIGNATURES) & (set(_hip.SIGNATURES) | set(_hip.ENS_SIGNATURES))
    assert '#include "p2i_hip.h"' in header


def test_versions():
    from p2igan_bench import ops
    lib = _hip.load()
    assert lib.p2i_stcs_abi_version() == 1 and ops.stcs_abi_version() == 1
    lib.p2i_abi_version.restype = C.c_int
    assert lib.p2i_abi_version() == 4 and lib.p2i_ens_abi_version() == 1          # the other headers' versions stand


@pytest.mark.parametrize("name", ["p2i_stcs_fields", "p2i_stcs_weights", "p2i_stcs_predict"])
@pytest.mark.parametrize("members", [0, 65, -1])
def test_member_count_is_bounded(name, members):
    assert _refused(name, members=members) == f"members must be in 1..64 (got {members})"


@pytest.mark.parametrize("name", ["p2i_stcs_spectrum", "p2i_stcs_noise", "p2i_stcs_fields"])
def test_the_torus_is_bounded(name):
    for St in (129, 0, -1):
        assert _refused(name, St=St) == f"embedding torus: {St} temporal cells, must be in 1..128"
    for Sy, Sx in ((513, SX), (SY, 513), (0, SX), (SY, 0)):
        assert _refused(name, Sy=Sy, Sx=Sx) == f"embedding torus {Sy} x {Sx}: sides must be in 1..512"


def test_a_sample_fits_its_torus():
    for kw in (dict(t=ST + 1), dict(h=SY + 1), dict(w=SX + 1), dict(t=0)):
        assert _refused("p2i_stcs_fields", **kw).endswith(f"does not fit the torus {ST} x {SY} x {SX}")
    for nunits in (0, 65536):
        assert _refused("p2i_stcs_fields", nunits=nunits) == f"bad unit range 0 + {nunits}"
    for stages in (0, 8, -1):
        assert _refused("p2i_stcs_fields", stages=stages) == f"stages must be a non-empty subset of 7 (got {stages})"


@pytest.mark.parametrize("name", ["p2i_stcs_weights", "p2i_stcs_predict"])
def test_the_frame_is_bounded(name):
    assert _refused(name, t=129) == "frames per sample must be in 1..128 (got 129)"
    assert _refused(name, t=0) == "frames per sample must be in 1..128 (got 0)"
    for h, w in ((513, W), (H, 513), (0, W)):
        assert _refused(name, h=h, w=w) == "bad frame shape"


@pytest.mark.parametrize("name", ["p2i_stcs_weights", "p2i_stcs_predict"])
def test_null_descriptors_are_refused(name):
    lib = _hip.load()
    args = list(CALLS[name]())
    args[0] = None
    assert getattr(lib, name)(*args) == -1 and lib.p2i_last_error().decode() == "null pointer"
    assert _refused(name, stt=None) == "null pointer"
    for field in ("pix", "z", "counts", "status"):
        assert _refused(name, k=_sys(**{field: None})) == "null pointer", field
    assert _refused("p2i_stcs_predict", k=_sys(params=None)) == "null pointer"
    assert _refused("p2i_stcs_predict", k=_sys(model=2)) == "variogram model must be 0 (exponential) or 1 (spherical)"
    # a space-time system is one sample
    assert _refused(name, k=_sys(R=2, T=2)) == "a space-time system is one sample: R = T = 1"
    assert _refused(name, k=_sys(np=48)) == "padded size 48 must be a multiple of 32 within cap 32"


def test_null_buffers_are_refused():
    assert _refused("p2i_stcs_spectrum", params=None) == "null pointer"
    assert _refused("p2i_stcs_spectrum", work=None) == "null pointer"
    assert _refused("p2i_stcs_noise", xi=None) == "null pointer"
    assert _refused("p2i_stcs_fields", amp=None) == "null pointer"
    assert _refused("p2i_stcs_fields", ens=None) == "null pointer"
    assert _refused("p2i_stcs_spectrum", model=2) == "variogram model must be 0 (exponential) or 1 (spherical)"
    assert _refused("p2i_stcs_spectrum", B=0) == "bad batch 0"
    assert _refused("p2i_stcs_spectrum", B=10923) == "bad batch 10923"              # B St = 65538 planes
    assert _refused("p2i_stcs_noise", npairs=0) == "bad member pairs 0 + 0"
    assert _refused("p2i_stcs_noise", q0=-1) == "bad member pairs -1 + 1"
