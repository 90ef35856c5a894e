"""CPU companion of tests/test_conv_sweep_gpu.py: the case list is deterministic and covers the table, every case passes the
descriptor check's arithmetic and the exactness bounds, the expected-refusal list follows from the stated rule, the split pipe
accepts the cases meant for it, and the planners' index-division helper is exact for every divisor it accepts."""
import ctypes

import numpy as np
import pytest

import conv_sweep_cases as cs


def _lib():
    from p2igan_bench import _hip
    return _hip.load()


def test_case_list_is_deterministic_and_unique():
    a, ta = list(cs.exact_cases()), list(cs.tolerance_cases())
    cs._CACHE.clear()
    b, tb = cs.exact_cases(), cs.tolerance_cases()
    assert a == b and ta == tb
    ids = [c.id for c in a] + [c.id for c in ta]
    assert len(ids) == len(set(ids))
    assert 200 <= len(a) <= 400 and len(ta) == len(cs.combos())
    assert cs.SEED == 20261016 and cs.PER_COMBO == 2


def test_case_list_covers_the_table():
    ex = cs.exact_cases()
    for nd, ks, ss in ((2, cs.K2, cs.S2), (3, cs.K3, cs.S3)):
        for k in ks:
            for s in ss:
                assert sum(1 for c in ex if (c.nd, c.k, c.s) == (nd, k, s)) >= cs.PER_COMBO, (nd, k, s)
    for c in ex:
        assert (c.k in (cs.K2 if c.nd == 2 else cs.K3) and c.s in (cs.S2 if c.nd == 2 else cs.S3)) or not c.id.startswith("r")
    assert {(1, 2, 2), (1, 3, 3), (1, 1, 2), (1, 2, 1)} <= set(cs.S2)
    assert {(2, 2, 2), (1, 3, 3), (3, 2, 2), (2, 1, 1), (1, 2, 1), (1, 1, 2)} <= set(cs.S3)
    assert set(cs.HW) == {c.sp[1] for c in ex} & set(cs.HW) == {c.sp[2] for c in ex} & set(cs.HW)
    assert set(cs.TS) <= {c.sp[0] for c in ex if c.nd == 3}
    assert set(cs.CH) <= {c.Cin for c in ex} and set(cs.CH) <= {c.Cout for c in ex}
    assert set(cs.BATCH) <= {c.B for c in ex}
    for axis in range(3):                                            # padding 0, k // 2, k - 1 and k on an axis with k >= 2
        pads = {("zero" if c.p[axis] == 0 else "half" if c.p[axis] == c.k[axis] // 2 else "full" if c.p[axis] == c.k[axis] - 1
                 else "k" if c.p[axis] == c.k[axis] else "other") for c in ex if c.k[axis] >= 2}
        assert {"zero", "half", "full", "k"} <= pads, (axis, pads)
    assert {(b, r, a) for c in ex for b, r, a in [(c.bias, c.res, c.act)]} == {(b, r, a) for b in (False, True) for r in (False, True)
                                                                                 for a in ("none", "relu")}
    od = [cs.out_dims(c) for c in ex]
    assert any(o[0] == 1 and min(o[1:]) > 1 for c, o in zip(ex, od) if c.nd == 3)      # outputs of extent 1: each axis in turn ...
    assert any(o[1] == 1 and o[2] > 1 for o in od) and any(o[2] == 1 and o[1] > 1 for o in od)
    assert any(o == (1, 1, 1) for o in od)                                              # ... and all
    assert any(o[2] > 32 for o in od)                                                   # several column tiles
    assert any(c.sp[2] % 4 == 0 for c in ex) and any(c.sp[2] % 4 != 0 for c in ex)       # 16-byte and 4-byte patch DMA
    assert any(c.sp[2] % 2 == 1 and c.s[2] == 2 and c.k[1:] == (3, 3) for c in ex)       # odd Wi with stride 2
    assert any(c.s[0] * c.s[1] * c.s[2] == 8 for c in ex) and any(c.s[0] * c.s[1] * c.s[2] > 8 for c in ex)
    # the size-1 patch axes: one tap and one output row / column on an axis
    assert any(c.k[1] == 1 and o[1] == 1 and c.k[0] == 1 for c, o in zip(ex, od))
    assert any(c.k[2] == 1 and o[2] == 1 and c.sp[2] % 4 != 0 for c, o in zip(ex, od))
    for cid in ("mg_1x1_h1", "mg_1x1_w1", "mg_1x3_h1", "mg_1x1x1_t4"):
        assert cid in {c.id for c in ex}
    tol = cs.tolerance_cases()
    assert {(c.nd, c.k, c.s) for c in tol} == set(cs.combos())
    assert {c.act for c in tol} == {"leaky", "tanh"}


def test_cases_pass_the_descriptor_check_and_the_exactness_bounds():
    for c in cs.exact_cases() + cs.tolerance_cases():
        assert cs.desc_ok(c), c
        assert max(cs.in_elems(c), cs.out_elems(c)) <= cs.MAX_ELEMS and cs.macs(c) <= 2 * cs.MAX_MACS, c
        assert c.k[1] * c.k[2] <= 9 or cs.expected_refusal(c, "wgrad", True)
    for c in cs.exact_cases():
        assert c.act in ("none", "relu")
        assert max(cs.exact_bounds(c).values()) < cs.EXACT_LIMIT, c
    assert cs.X_MAX <= 255 and cs.W_MAX <= 255          # inside the high bf16 plane of the 3-way split


def test_exactness_bounds_dominate_the_reference():
    """exact_bounds are range bounds; spot-check (a thinned list: the float64 reference of every case belongs to the GPU test)
    that the reference of |x|, |w| stays below them and that the expectation is integral."""
    import torch
    for c in cs.exact_cases()[::9]:
        t = cs.exact_inputs(c)
        r = cs.reference(c, {k: (v.abs() if v is not None and k != "mask" else v) for k, v in t.items()}, "relu")
        b = cs.exact_bounds(c)
        assert float(r["out"].max()) <= b["fwd"] and float(r["dx_e"].abs().max()) <= b["dgrad"]
        assert float(r["dw"].max()) <= b["wgrad"] and float(r["db"].max()) <= b["bgrad"]
        for v in cs.reference(c, t, "relu").values():
            assert torch.equal(v, v.round()) and torch.equal(v.float().double(), v)


def test_expected_refusals_follow_from_the_stated_limit():
    ref = {(c.id, pro) for c in cs.exact_cases() for pro in (False, True) if cs.expected_refusal(c, "wgrad", pro)}
    assert ref == {("k2x5_wgrad_limit", False), ("k2x5_wgrad_limit", True)}
    for c in cs.exact_cases():
        assert cs.expected_refusal(c, "fwd", False) is None and cs.expected_refusal(c, "dgrad", True) is None
        assert (cs.expected_refusal(c, "wgrad", True) is not None) == (c.k[1] * c.k[2] > 9)
    assert not any(cs.expected_refusal(c, "wgrad", p) for c in cs.tolerance_cases() for p in (False, True))


def test_split_pipe_accepts_the_cases_meant_for_it(monkeypatch):
    """p2i_x6c_would_take is host-only (it reads switches and does arithmetic, csrc/conv_x6c.hip): with the tile-count threshold
    lowered as the GPU sweep's `x6c` engine does, every case the generator means for the bf16-split pipe is accepted."""
    from p2igan_bench import _hip
    lib = _lib()
    monkeypatch.setenv("P2I_X6C_MIN_WG", "1")
    by_id = {c.id: c for c in cs.exact_cases()}
    took = 0
    for cid, dgrad in cs.X6C_INTENDED:
        c = by_id[cid]
        d = _hip.ConvDesc(c.B, c.Cin, c.Cout, *c.sp, *cs.out_dims(c), *c.k, *c.s, *c.p)
        took += lib.p2i_x6c_would_take(ctypes.byref(d), dgrad, 0)
    assert took == len(cs.X6C_INTENDED) >= 10
    c = by_id["mg_1x1_h1"]
    d = _hip.ConvDesc(c.B, c.Cin, c.Cout, *c.sp, *cs.out_dims(c), *c.k, *c.s, *c.p)
    assert lib.p2i_x6c_would_take(ctypes.byref(d), 0, 0) == 0


def test_fast_div_multiplier_is_exact_or_refused():
    """The planners' index division (csrc/common.h: magic_u16 / fast_div) is umulhi(n, magic): for every divisor the library hands
    out a multiplier for, (n * magic) >> 32 == n // d for all n < 65536; a divisor without such a multiplier -- d = 1 above all:
    2^32 + 1 wraps to 1 and every quotient comes out 0 -- must be refused, not answered."""
    lib = _lib()
    n = np.arange(65536, dtype=np.uint64)
    m = ctypes.c_uint32(0)
    for d in (1, 0, -1, 65536, 1 << 20):
        rc = lib.p2i_fast_div_magic(d, ctypes.byref(m))
        if rc == 0:                                       # answered: then it has to be right
            assert d >= 1 and np.array_equal((n * np.uint64(m.value)) >> np.uint64(32), n // np.uint64(d)), d
        else:
            assert b"fast_div" in lib.p2i_last_error()
    assert lib.p2i_fast_div_magic(1, ctypes.byref(m)) != 0
    bad = []
    for d in range(2, 65536):
        assert lib.p2i_fast_div_magic(d, ctypes.byref(m)) == 0, d
        if not np.array_equal((n * np.uint64(m.value)) >> np.uint64(32), n // np.uint64(d)):
            bad.append(d)
    assert not bad, bad[:10]
