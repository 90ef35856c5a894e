"""The case tables of tests/weightprep_cases.py have the properties that test_weightprep_gpu.py relies on: every fold / pack sum is
an integer below 2^24 (so float32 results do not depend on the order of summation and the comparison can be torch.equal), every
listed reason -- which kernel the planner picks, second trips, ragged column and row groups -- is true of its case, the restatements
agree with the oracle's own fold, and the three-term bf16 split is exact on the case values."""
import numpy as np
import pytest
import torch

import weightprep_cases as wc


# ------------------------------------------------------------------------------------------------ fold
@pytest.mark.parametrize("c", wc.FOLD_CASES, ids=wc.case_id)
def test_fold_case_is_exact_and_matches_the_oracle_fold(c):
    from oracle import p2i_oracle as orc
    O, I, g, ksz, rep, _ = c
    W, D, Dd, dwp = wc.fold_inputs(c)
    for t in (W, D, Dd, dwp):
        if t is not None:
            assert torch.equal(t, t.round())
    fwd, dw, dd = wc.fold_bounds(c)                # from the case's own O, I, groups (dD sums over O / g)
    assert max(fwd, dw, dd) < wc.EXACT
    wp_f, wp_d, dW, dD = wc.fold_expected(c, W, D, Dd, dwp)
    assert float(wp_f.abs().max()) <= fwd and float(dW.abs().max()) <= dw
    assert dD is None or float(dD.abs().max()) <= dd
    for t in (wp_f, wp_d, dW, dD):
        if t is not None:
            assert torch.equal(t, t.round())
    # the dense weight of the packed layout is the oracle's DoW placed in its group (+ the identity skip)
    dow = orc.doconv_fold(W.double(), None if D is None else D.double(), None if Dd is None else Dd.double(), O, I, g, ksz)
    dense = wp_f[:, :, :O].permute(2, 1, 0).double()           # (O, I, nt)
    Ig, Og = I // g, O // g
    inside = torch.zeros(O, I, dtype=torch.bool)
    for o in range(O):
        lo = (o // Og) * Ig
        inside[o, lo:lo + Ig] = True
        want = dow[o].reshape(Ig, -1).clone()
        if rep:
            want[o // rep - lo, 4] += 1
        assert torch.equal(dense[o, lo:lo + Ig], want)
    assert not bool(dense[~inside].any())                       # zeros outside the group
    assert not bool(wp_f[:, :, O:].any()) and not bool(wp_d[:, :, I:].any())      # zeros in the padded columns
    assert torch.equal(wp_d[:, :, :I].permute(1, 2, 0), wp_f[:, :, :O].permute(2, 1, 0))
    # the packed gradient is non-zero where nothing may be read: padded columns, entries outside the group
    if wc.pad32(O) != O:
        assert bool(dwp[:, :, O:].any())
    if g > 1:
        assert bool(dwp[:, :, :O].permute(2, 1, 0)[~inside].any())


def test_fold_gradients_are_the_autograd_of_the_fold():
    """dW, dD of the restatement = float64 autograd of sum(DoW * dDoW) through the oracle's fold (one grouped, one plain case)"""
    from oracle import p2i_oracle as orc
    for c in [(24, 12, 3, 3, 0, "eye"), (33, 65, 1, 3, 0, "eye"), (64, 32, 1, 3, 0, "int")]:
        O, I, g, ksz, _, _ = c
        W, D, Dd, dwp = wc.fold_inputs(c)
        _, _, dW, dD = wc.fold_expected(c, W, D, Dd, dwp)
        Wg, Dg = W.double().requires_grad_(True), D.double().requires_grad_(True)
        dow = orc.doconv_fold(Wg, Dg, Dd.double(), O, I, g, ksz).reshape(O, I // g, 9)
        gd = dwp[:, :, :O].permute(2, 1, 0).double()
        gin = torch.stack([gd[o, (o // (O // g)) * (I // g):(o // (O // g) + 1) * (I // g)] for o in range(O)])
        (dow * gin).sum().backward()
        assert torch.equal(Wg.grad.float(), dW) and torch.equal(Dg.grad.float(), dD)


def test_fold_reasons_hold():
    tile_both = [c for c in wc.FOLD_CASES if wc.fold_fwd_is_tile(c)]
    assert {(32, 64), (64, 32), (96, 32), (32, 160), (288, 32)} == {c[:2] for c in tile_both}
    assert all(c[0] != c[1] for c in tile_both)                                   # O != I everywhere on the tile kernels
    assert any(c[5] == "int" for c in tile_both)
    assert all(wc.fold_bwd_is_tile(c) == wc.fold_fwd_is_tile(c) for c in wc.FOLD_CASES if c[4] == 0)      # one planner, both ways
    generic = [c for c in wc.FOLD_CASES if not wc.fold_bwd_is_tile(c) and c[2] == 1 and c[3] == 3]
    assert {(48, 16), (16, 48), (33, 65), (1, 8), (8, 1)} <= {c[:2] for c in generic}
    assert all(wc.pad32(c[0]) != c[0] or wc.pad32(c[1]) != c[1] for c in generic)
    ragged_i = [c for c in generic if c[0] % 32 == 0 and c[4] == 0]               # whole tiles in O, none in I: generic all the same,
    assert {(32, 24), (64, 40), (288, 24)} == {c[:2] for c in ragged_i}           # with an unpadded pitch (pad32(O) == O) in dwp
    assert all(c[1] % 32 != 0 and c[1] % 16 != 0 for c in ragged_i)
    assert sum(c[2] > 1 for c in wc.FOLD_CASES) == 4 and {1, 3} == {c[3] for c in wc.FOLD_CASES if c[2] > 1}
    assert any(c[4] > 0 and c[2] == 1 and not wc.fold_fwd_is_tile(c) and c[0] % 32 == 0 for c in wc.FOLD_CASES)
    assert any(c[0] // c[2] > 256 and c[3] == 3 and not wc.fold_bwd_is_tile(c) for c in wc.FOLD_CASES)      # second trip of fold_bwd_d_kernel's 256 threads
    assert any(c[0] > 256 and wc.fold_bwd_is_tile(c) for c in wc.FOLD_CASES)
    for c in wc.FOLD_CASES:
        assert c[4] == 0 or (c[3] == 3 and c[1] * c[4] == c[0])
    for c in wc.FOLD_REFUSED:
        assert c[4] > 0 and not (c[3] == 3 and c[1] * c[4] == c[0])
    assert wc.fold_fwd_is_tile(wc.FOLD_NO_D[0]) and not wc.fold_fwd_is_tile(wc.FOLD_NO_D[1])
    assert all(o % 32 == 0 and i % 32 == 0 for o, i in wc.FOLD_BATCHED_SHAPES)
    assert sum(o != i for o, i in wc.FOLD_BATCHED_SHAPES) == 3 and max(wc.FOLD_BATCHED_N) == wc.FOLD_MAX_LAYERS


def test_fold_layers_of_a_batch_differ():
    a, b = wc.fold_inputs((32, 64, 1, 3, 0, "eye"), seed=0), wc.fold_inputs((32, 64, 1, 3, 0, "eye"), seed=1)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) and not torch.equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------ pack / unpack
@pytest.mark.parametrize("shape", wc.PACK_SHAPES, ids=wc.case_id)
def test_pack_cases_are_exact(shape):
    O, I, nt = shape
    w = wc.pack_weight(shape)
    assert torch.equal(w, w.round()) and float(w.abs().max()) <= wc.PACK_W_MAX
    for sigma in wc.PACK_SIGMAS:
        f, d = wc.pack_expected(w, sigma)
        assert f.shape == (nt, I, wc.pad32(O)) and d.shape == (nt, O, wc.pad32(I))
        s = 1.0 if sigma is None else sigma
        assert torch.equal(f[:, :, :O].permute(2, 1, 0).double() * s, w.double())          # the division lost nothing
        assert torch.equal(d[:, :, :I].permute(1, 2, 0), f[:, :, :O].permute(2, 1, 0))
        assert not bool(f[:, :, O:].any()) and not bool(d[:, :, I:].any())
    g1, g2 = wc.packed_grad(shape, 1, 7), wc.packed_grad(shape, 2, -5)
    if wc.pad32(O) != O:
        assert bool((g1[:, :, O:] == 7).all()) and bool((g2[:, :, O:] == -5).all())
    assert float((wc.unpack_expected(g1, O) + wc.unpack_expected(g2, O)).abs().max()) < wc.EXACT


def test_pack_tables():
    assert len(wc.PACK_SHAPES) <= wc.PACK_MAX_LAYERS
    assert any(wc.pad32(o) == o for o, _, _ in wc.PACK_SHAPES) and any(wc.pad32(i) == i for _, i, _ in wc.PACK_SHAPES)
    assert all(s is None or np.log2(s) == int(np.log2(s)) for s in wc.PACK_SIGMAS)
    assert set(wc.SN_UNPACK_SHAPES) <= set(wc.PACK_SHAPES)


def test_sn_unpack_reference_is_the_formula_of_the_header():
    """dw = g / sigma - (sum(g .* w) / sigma^2) u v^T, against the float64 autograd of the oracle"""
    for shape in wc.SN_UNPACK_SHAPES:
        O, I, nt = shape
        w, u, v, sigma, g = wc.sn_unpack_inputs(shape)
        ref = wc.sn_unpack_expected(w, u, v, g)
        gd, wd, sg = wc.unpack_expected(g, O).double(), w.double(), sigma.double()
        want = gd / sg - ((gd * wd).sum() / sg ** 2) * (u.double().reshape(O, 1, 1) * v.double().reshape(1, I, nt))
        assert float((ref - want).abs().max()) <= 1e-6 * float(ref.abs().max())      # sigma was rounded to float32: 6e-8


# ------------------------------------------------------------------------------------------------ bf16 split
@pytest.mark.parametrize("shape", wc.SPLIT_SHAPES + [wc.SPLIT_STRIDE_SHAPE], ids=wc.case_id)
def test_split_is_exact_on_the_case_values(shape):
    a = wc.split_values(shape)
    assert a.shape == shape and shape[1] % 8 == 0 and shape[2] % 32 == 0
    assert np.isfinite(a).all()
    bits = a.view(np.uint32)
    expo = (bits >> 23) & 0xFF
    assert ((expo == 0) == ((bits & 0x7FFFFFFF) == 0)).all()                         # no subnormal: exponent 0 only for +-0
    assert (np.abs(expo[expo != 0].astype(np.int64) - 127) <= wc.SPLIT_EXP).all()
    flat = bits.reshape(-1)
    assert {0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x3F800001} <= set(int(b) for b in flat[:9])
    hi, mid, lo = wc.split_terms(a)
    assert (hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64) == a.astype(np.float64)).all()
    for t in (hi, mid, lo):
        assert ((t.view(np.uint32) & 0xFFFF) == 0).all()                             # each term is a bf16 value
    assert (lo != 0).any() and (mid != 0).any()                                      # dropping a plane changes the image
    one = np.array([0x3F800001], dtype=np.uint32).view(np.float32)
    h1, m1, l1 = wc.split_terms(one)
    assert h1[0] == 1.0 and m1[0] == 2.0 ** -23 and l1[0] == 0.0                     # the last bit alone: the mid plane carries it
    h2, m2, l2 = wc.split_terms(np.array([0x3F800101], dtype=np.uint32).view(np.float32))
    assert h2[0] == 1.0 and m2[0] == 2.0 ** -15 and l2[0] == 2.0 ** -23              # behind another bit: only the lo plane does


def test_split_is_not_exact_on_subnormals():
    """the documented limit: 1e-40 loses bits (the remainder's significant bits fall in the lower half-word)"""
    a = np.array([1e-40], dtype=np.float32)
    hi, mid, lo = wc.split_terms(a)
    assert float(hi[0]) + float(mid[0]) + float(lo[0]) != float(a[0])


def test_split_image_layout():
    """Wb[plane][tap][k/8][m][k%8], checked element by element on a small tensor"""
    shape = (2, 16, 32)
    a = wc.split_values(shape, seed=5)
    img = wc.split_image(a).reshape(3, 2, 2, 32, 8)
    terms = wc.split_terms(a)
    for plane in range(3):
        for tap, k, m in [(0, 0, 0), (1, 7, 3), (0, 8, 31), (1, 15, 17), (1, 9, 0)]:
            assert int(img[plane, tap, k // 8, m, k % 8]) == int(terms[plane][tap, k, m].view(np.uint32)) >> 16


def test_split_tables():
    assert all(wc.split_units(s) <= wc.SPLIT_GRID_UNITS for s in wc.SPLIT_SHAPES)
    assert wc.split_units(wc.SPLIT_STRIDE_SHAPE) > wc.SPLIT_GRID_UNITS              # a second grid-stride trip
    assert wc.split_units(wc.SPLIT_STRIDE_SHAPE) < 2 * wc.SPLIT_GRID_UNITS          # ... that only part of the grid takes


# ------------------------------------------------------------------------------------------------ spectral norm
def test_spectral_norm_reasons_hold():
    groups = {k: -(-k // wc.SN_WTU_COLS) for _, k in wc.SN_SHAPES}              # workgroups of W^T u per layer
    assert groups[65] == 2 and groups[1030] == 17 and groups[4100] == 65           # more than one, the last one ragged
    assert all(k % wc.SN_WTU_COLS != 0 for k in (65, 1030, 4100)) and any(k % wc.SN_WTU_COLS == 0 for _, k in wc.SN_SHAPES)
    assert any(k < wc.SN_WTU_COLS and o > 1 for o, k in wc.SN_SHAPES)
    # rows: the 4 row groups take unequal shares (O % 4 != 0), some take none (O < 4), and O = 1030 gives each more than 256 trips
    assert {1, 2, 3} <= {o % wc.SN_WTU_ROW_GROUPS for o, _ in wc.SN_SHAPES} and any(o < wc.SN_WTU_ROW_GROUPS for o, _ in wc.SN_SHAPES)
    assert all(o in {o for o, _ in wc.SN_SHAPES} for o in (33, 40, 70, 1030))                  # the row counts of the earlier sweep stay
    assert any(o > wc.SN_NORM_THREADS for o, _ in wc.SN_SHAPES) and any(k > wc.SN_NORM_THREADS for _, k in wc.SN_SHAPES)
    assert any(k > 4 * wc.SN_NORM_THREADS for _, k in wc.SN_SHAPES)
    assert 2 * len(wc.SN_SHAPES) == wc.SN_MAX_LAYERS


def test_spectral_norm_reference():
    for shape in wc.SN_SHAPES:
        w, u, v = wc.sn_inputs(shape)
        un, vn, sigma = wc.sn_expected(w, u, v, True)
        assert abs(float(un.norm()) - 1) < 1e-12 and abs(float(vn.norm()) - 1) < 1e-12
        assert float(sigma) > 0
        ue, ve, se = wc.sn_expected(w, u, v, False)
        assert torch.equal(ue, u.double()) and torch.equal(ve, v.double())
    w = torch.zeros(wc.SN_ZERO_SHAPE)
    _, u, v = wc.sn_inputs(wc.SN_ZERO_SHAPE)
    un, vn, sigma = wc.sn_expected(w, u, v, True)
    assert not bool(un.any()) and not bool(vn.any()) and float(sigma) == 0.0      # F.normalize(0, eps=1e-12) = 0, nothing NaN
