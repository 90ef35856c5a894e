"""CPU companion of tests/test_loss_ext_edges_gpu.py (no GPU, no library load): the tables of tests/loss_ext_cases.py hold every
value the sweep lists, each case has the size that puts it on the path of csrc/loss_ext.hip it is there for (predicates restated
from ext_grid, EXT_VEC and the launch lines: sizes, not device counters), the exact family is exact in float32, distinct-valued
inputs have unique window maxima, the kink cap holds, the float64 restatement equals torch.nn.functional on the pooled pieces, and
the float32 restatement's max e_i per operation is what loss_ext_cases.F32_E records (printed; the kernels' bound is 4 x, floor 8).

  second grid-stride trips   transform / wl1_bwd / kl_bwd at 4,197,396 (16-byte path, one trip covers 4,194,304) and 1,049,349
                             (scalar path, 1,048,576); fdiff at inner 1,049,348 / 1,049,349; spool_fwd at 2,099,601 pooled
                             outputs, spool_bwd and shock_gather at 2,099,601 stored pixels (2,097,152); tdm_fwd at 151,500
                             pooled positions (131,072)
  scalar path on n % 4 == 0  views with storage offset 1: a pointer 4 bytes past an allocation
  softmax block size         L = 1023 / 1024 / 1025 either side of the switch to 1024 threads; 65,537 rows
  shock tiles                maps one short of, equal to and one past the 32 x 8 tile, and twice that; 2- and 3-wide maps"""
import numpy as np
import torch
import torch.nn.functional as F

import loss_ext_cases as C
import losses_ext_ref as R


def _numel(shape):
    return int(np.prod(shape))


def test_tables_cover_every_listed_value():
    assert C.elem_sizes() == [1, 3, 4, 5, 1023, 1024, 1025, 4197396, 1049349]
    assert {C.kl_batch(n) for n in C.elem_sizes()} == {1, 3}
    fd = C.fdiff_cases()
    assert {c.B for c in fd} == {1, 3} and {c.T for c in fd} == {2, 3, 17} and {c.inner for c in fd} == {1, 3, 4, 5, 28, 1028}
    assert len([c for c in fd if not c.shift]) == 2 * 3 * 6
    assert {(c.B, c.T, c.inner) for c in fd if c.shift} == {(b, t, i) for b in (1, 3) for t in (2, 3, 17) for i in (4, 28, 1028)}
    assert [(c.B, c.T, c.inner) for c in C.fdiff_cases(True)] == [(2, 3, 1049348), (2, 3, 1049349)]
    sp = C.spool_cases()
    hw = {tuple(c.shape[-2:]) for c in sp}
    assert hw == {(h, w) for h in range(1, 10) for w in range(1, 10)} | {(13, 66), (66, 13)} and len(sp) == 83
    assert {(len(c.shape), _numel(c.shape[:-2])) for c in sp} == {(3, 1), (3, 5), (4, 1), (4, 5)}
    assert [s[2] for s in C.softmax_shapes()[:-1]] == [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 4097]
    assert all(s[0] * s[1] == 3 for s in C.softmax_shapes()[:-1]) and C.softmax_shapes()[-1] == (65537, 1, 3) and C.TEMP == 0.1
    td = C.tdm_cases()
    assert {c.shape for c in td} == {(1, 1, 2, 3), (2, 2, 4, 4), (1, 3, 5, 5), (2, 2, 6, 9), (1, 2, 8, 8), (1, 2, 33, 7), (3, 5, 400, 404)}
    assert {c.beta for c in td} == {1.0, 30.0}
    sizes = {(h, w) for h in (2, 3, 4) for w in (2, 3, 4)} | {(7, 31), (8, 32), (9, 33), (16, 64), (17, 65), (3, 33), (9, 2)}
    sl = C.shock_loss_cases()
    assert {(c.hp, c.wp) for c in sl[:-2]} == sizes and {(c.hp, c.wp) for c in C.shock_map_cases()} == sizes
    assert {c.pool for c in sl} == {1, 2, 3, 4} and {c.beta for c in sl} == {0.02, 1.0, 30.0} == {c.beta for c in C.shock_map_cases()}
    assert {c.bt[0] * c.bt[1] for c in sl[:-2]} == {1, 4}
    assert {0, 1} <= {c.border for c in sl}
    assert any(c.border == C.max_border(c.hp, c.wp) and c.border >= 2 for c in sl), "border_ignore at its largest legal value"
    assert all(0 <= c.border <= C.max_border(c.hp, c.wp) for c in sl)
    assert (sl[-2].bt[0] * sl[-2].bt[1], sl[-2].hp, sl[-2].wp) == (300, 3, 2)
    assert (sl[-1].bt[0] * sl[-1].bt[1], sl[-1].hp, sl[-1].wp) == (65535, 2, 2) == (C.SHOCK_MAX_PLANES, 2, 2)
    assert _numel(C.SHOCK_OVER_LIMIT[:2]) == 65536
    ids = [c.id for c in sl] + [c.id for c in C.shock_map_cases()]
    assert len(ids) == len(set(ids))
    for c in sl:
        assert C.shock_stored(c) == (c.hp * c.pool + c.pool - 1, c.wp * c.pool + c.pool - 1)
        assert C.shock_stored(c)[0] // c.pool == c.hp and C.shock_stored(c)[1] // c.pool == c.wp


def test_cases_land_on_their_paths():
    # element-wise kernels: 16-byte path iff n % 4 == 0 and aligned; second trip iff more items than 4096 * 256
    vec_n, scalar_n = C.ELEM_N_SECOND_TRIP
    assert vec_n % 4 == 0 and vec_n > C.ELEM_ONE_TRIP_VEC == 4194304 and vec_n // 4 > C.ELEM_CAP * C.WG
    assert scalar_n % 4 != 0 and scalar_n > C.ELEM_ONE_TRIP_SCALAR == 1048576
    assert max(C.ELEM_N) < C.ELEM_ONE_TRIP_SCALAR
    assert vec_n % 3 == 0 and scalar_n % 3 == 0 and C.kl_batch(1024) == 1          # KL's B = 3 rows on both second-trip sizes
    x = torch.zeros(1024)
    assert C.is_vec_path(1024, x) and not C.is_vec_path(1024, C.misaligned(x)) and not C.is_vec_path(1023, x[:1023])
    v = C.misaligned(torch.arange(8.0).reshape(2, 4))
    assert v.is_contiguous() and v.storage_offset() == 1 and v.contiguous() is v and torch.equal(v, torch.arange(8.0).reshape(2, 4))
    assert not C.is_vec_path(1024, x, C.misaligned(x))                           # one misaligned pointer is enough
    (bv, tv, iv), (bs, ts, isc) = C.FDIFF_SECOND_TRIP
    assert iv % 4 == 0 and bv * (tv - 1) * iv // 4 > C.ELEM_CAP * C.WG and bv * tv * iv // 4 > C.ELEM_CAP * C.WG
    assert isc % 4 != 0 and bs * (ts - 1) * isc > C.ELEM_CAP * C.WG
    # pools
    n, h, w = C.SPOOL_SECOND_TRIP_FWD
    assert n * ((h - 1) // 4 + 1) * ((w - 1) // 4 + 1) == 2099601 > C.POOL_ONE_TRIP == 2097152
    assert _numel(C.SPOOL_SECOND_TRIP_BWD) == 2099601 > C.POOL_ONE_TRIP and _numel(C.SHOCK_SECOND_TRIP) == 2099601
    assert max(_numel(c.shape) for c in C.spool_cases()) < C.POOL_ONE_TRIP
    pos = [C.tdm_positions(c.shape) for c in C.tdm_cases()]
    assert max(pos) == 151500 > C.TDM_ONE_TRIP == 131072 and sorted(pos)[-2] < C.TDM_ONE_TRIP
    # softmax: 256 threads below L = 1024, 1024 from there on; rows beyond 65,535
    Ls = [s[2] for s in C.softmax_shapes()]
    assert {1023, 1024, 1025} <= set(Ls) and {255, 256, 257} <= set(Ls)
    assert any(L < C.SOFTMAX_WIDE_L and L > 256 for L in Ls) and any(L > 4 * 1024 for L in Ls)      # several elements per thread on both
    assert C.softmax_shapes()[-1][0] > 65535
    # shock tiles: ceil(Wp / 32) x ceil(Hp / 8)
    tiles = {(c.hp, c.wp): C.shock_tiles(c.hp, c.wp) for c in C.shock_loss_cases()}
    assert tiles[(7, 31)] == (1, 1) and tiles[(8, 32)] == (1, 1) and tiles[(9, 33)] == (2, 2)
    assert tiles[(16, 64)] == (2, 2) and tiles[(17, 65)] == (3, 3) and tiles[(3, 33)] == (2, 1) and tiles[(9, 2)] == (1, 2)
    assert any(c.wp == 3 for c in C.shock_loss_cases()) and any(c.hp == 3 for c in C.shock_loss_cases())
    assert any(c.wp == 2 and c.hp > 2 for c in C.shock_loss_cases())


def test_exact_family_is_exact_in_float32():
    for c in C.fdiff_cases():
        x, dy = C.fdiff_inputs(c)
        assert float(x.abs().max()) <= 1000 and torch.equal(x, x.round()) and torch.equal(dy, dy.round())
        out, dx = C.fdiff_ref(x, dy)
        o64, d64 = C.fdiff_ref(x.double(), dy.double())
        assert torch.equal(out.double(), o64) and torch.equal(dx.double(), d64)
        assert torch.equal(out, R.compute_forward_difference(x))
    for c in C.spool_cases():
        x, dy = C.spool_inputs(c.shape)
        assert x.unique().numel() == x.numel() and float(x.min()) < 0 or x.numel() == 1
        assert C.window_maxima_unique(x), c.shape
        out, idx, dx = C.spool_ref(x, dy)
        assert torch.equal(out, R.spatial_pool(x)) and torch.equal(dx.double().sum(), dy.double().sum())
        flat = x.reshape(-1, x.shape[-2] * x.shape[-1])
        assert torch.equal(flat.gather(1, idx.reshape(flat.shape[0], -1).long()).reshape(out.shape), out)


def test_inputs_repeat_and_hold_their_special_values():
    for n in (5, 1025):
        pred, true = C.wl1_inputs(n)
        assert torch.equal(pred, C.wl1_inputs(n)[0])
        assert float(true[0]) == float(C.WL1_XMAX) and float(true[2]) < float(true[0]) < float(true[1])
        assert float(true[1]) - float(true[2]) < 1.3e-7
        assert int((pred == true).sum()) == 2
        _, _, dp, sdp = C.wl1_ref(pred, true)
        assert float(dp[1]) == 0.0 and float(dp[4]) == 0.0
        p, q = C.kl_inputs(n)
        assert float(p.min()) > 0 and int((q == 0).sum()) >= n // 3 and abs(float(p.double().sum()) - C.kl_batch(n)) < 1e-5
    for shape in C.softmax_shapes()[2:]:
        x, _ = C.softmax_inputs(shape)
        z = x.reshape(shape[0] * shape[1], -1) / np.float32(C.TEMP)
        zm = z - z.max(dim=1, keepdim=True).values
        assert float(zm.min()) < -104.0 and bool((torch.exp(zm) == 0).any()), shape          # float32 exp underflows to exactly 0
    for c in C.tdm_cases():
        pd, td, tr = C.tdm_inputs(c.shape)
        assert pd.unique().numel() == pd.numel() and C.window_maxima_unique(pd) and float(tr.min()) >= 0


def test_kink_cap_holds():
    """Outside the corners at most 1% of a case's elements sit within the band of a relu / |s| kink and get dout = 0."""
    total = zeroed = corners = 0
    for c in C.shock_loss_cases():
        pred, true, dout = C.shock_inputs(c)
        ref = C.shock_loss_ref(pred, true, dout, c.beta, c.pool, c.border)
        off = ref["near"] & ~ref["corner"]
        assert int(off.sum()) <= C.KINK_CAP * off.numel(), (c.id, int(off.sum()), off.numel())
        assert bool(ref["near"][ref["corner"]].all()), c.id                 # corners always qualify: gx = gy = 0, |s| <= sqrt(eps)
        assert bool((ref["dout"][ref["near"]] == 0).all()) and torch.equal(ref["dout"][~ref["near"]], dout[~ref["near"]])
        total, zeroed, corners = total + off.numel(), zeroed + int(off.sum()), corners + int(ref["corner"].sum())
    print(f"kinks: {zeroed} of {total} elements zeroed outside the corners, {corners} corner elements")


def test_restatement_equals_functional_on_the_pooled_pieces():
    for c in C.tdm_cases()[:6]:
        pd, td, tr = C.tdm_inputs(c.shape)
        ref = C.tdm_ref(pd, td, tr, c.beta)
        want = R.temporal_difference_matching_loss(pd.double(), td.double(), tr.double(), c.beta, C.TDM_EPS)
        assert abs(float(ref["loss"]) - float(want)) <= 1e-14 * abs(float(want))
        _, idx = F.max_pool2d(pd, 5, 4, 2, return_indices=True)
        assert torch.equal(ref["idx"], idx.int())
        assert abs(float(ref["dpred"].sum()) - float(ref["coef"].sum()) * C.TDM_GOUT) <= 1e-12
    for c in C.shock_loss_cases()[:-1]:
        pred, true, dout = C.shock_inputs(c)
        ref = C.shock_loss_ref(pred, true, dout, c.beta, c.pool, c.border)
        want = R.shock_map_loss(pred.double(), true.double(), beta=c.beta, border_ignore=c.border, pool=c.pool, eps=C.SHOCK_EPS)
        assert tuple(ref["out"].shape) == tuple(want.shape) == tuple(dout.shape)
        assert float((ref["out"] - want).abs().max()) <= 1e-15, c.id
        assert bool((ref["sout"] > 0).all()) and bool((ref["sdx"] >= ref["dx"].abs()).all())
        dropped, border_only = C.shock_zero_sets(c, pred.shape)
        assert bool((ref["dx"][..., dropped] == 0).all()) and bool((ref["dx"][..., border_only] == 0).all()), c.id
        assert bool((ref["dx"][C.pool_non_argmax(pred, c.pool)] == 0).all()), c.id
    assert any(bool(C.shock_zero_sets(c, (1, 1) + C.shock_stored(c))[1].any()) for c in C.shock_loss_cases())
    for c in C.shock_map_cases():
        x, _, dout = C.shock_inputs(c)
        s, ss, dx, sdx = C.shock_map_ref(x, dout, c.beta)
        assert float((s - R.shock_map(x.double(), c.beta, C.SHOCK_EPS)).abs().max()) <= 1e-15
    x, dy = C.softmax_inputs((1, 3, 257))
    y, sy, dx, sdx = C.softmax_ref(x, dy)
    want, wgrad = R.value_and_grad(lambda t: R.softmax_temperature(t, C.TEMP), [x.numpy()], dy.numpy(), torch.float64)
    assert float((y - want).abs().max()) <= 1e-15 and float((dx - wgrad).abs().max()) <= 1e-12 * float(wgrad.abs().max())
    for n, fn, inputs, ref, g in ((1025, R.transform, C.transform_inputs(1025)[:1], C.transform_ref(*C.transform_inputs(1025)), C.transform_inputs(1025)[1].numpy()),
                                  (1025, R.weighted_l1_distance, C.wl1_inputs(1025), C.wl1_ref(*C.wl1_inputs(1025)), C.WL1_GOUT),
                                  (1023, R.kl_divergence, C.kl_inputs(1023), C.kl_ref(*C.kl_inputs(1023)), C.KL_GOUT)):
        want, wgrad = R.value_and_grad(fn, [t.numpy() for t in inputs], g, torch.float64)
        assert float((ref[0] - want).abs().max()) <= 1e-13 * float(want.abs().max())
        assert float((ref[2] - wgrad).abs().max()) <= 1e-13 * float(wgrad.abs().max())


def test_non_finite_cases_against_torch():
    """torch keeps a NaN of a pool window and gives the argmax to the window's last NaN in raster order; the reach sets cover
    every NaN of the restatement's gradients."""
    names = [n for n, _ in C.NF_CASES]
    assert names[:5] == ["nan-first", "nan-interior", "nan-last", "nan-shared", "nan-two"] and {"pos-inf", "neg-inf"} <= set(names)
    H, W = C.NF_PLANE
    for name, poison in C.NF_CASES:
        x = C.nf_inputs(poison)
        out, idx = F.max_pool2d(x, 5, 4, 2, return_indices=True)
        hit = F.max_pool2d(torch.isnan(x).float(), 5, 4, 2) > 0
        assert torch.equal(torch.isnan(out), hit), name
        if name == "nan-two":
            assert int(idx[0, 1, 1, 1]) == 4 * W + 5
        if name == "nan-shared":
            assert int(hit.sum()) == 4 and bool((idx[0, 1, 1:, 1:] == 6 * W + 6).all())
        for pool in (1, 2):
            p64 = x.double().requires_grad_(True)
            t64 = C.nf_inputs([]).double().flip(-1)
            R.shock_map_loss(p64, t64, beta=1.0, pool=pool, eps=C.SHOCK_EPS).nan_to_num(nan=1.0, posinf=1.0).sum().backward()
            bad = ~torch.isfinite(p64.grad)
            assert not bool(bad[0, 0].any()) and not bool((bad[0, 1] & ~C.nf_reach(poison, pool, "shock")).any()), (name, pool)
    assert torch.isnan(F.relu(torch.tensor(float("nan"))))


def test_float32_restatement_errors():
    """max e_i of the restatement run in float32 on the CPU, per operation, over the whole table: what F32_E records."""
    e = C.f32_errors()
    for k, v in e.items():
        print(f"{k}: float32 restatement max e = {v:.3f}, recorded {C.F32_E[k]}, kernel bound {C.bound(k):g}")
    assert set(e) == set(C.F32_E)
    for k, v in e.items():
        assert v <= C.F32_E[k] <= 1.5 * v + 0.1, (k, v, C.F32_E[k])        # recorded rounded up; sums depend a little on the thread count
        assert C.bound(k) == max(8.0, 4.0 * C.F32_E[k])
