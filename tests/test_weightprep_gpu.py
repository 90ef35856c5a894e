"""Shape sweep of the weight-preparation kernels (csrc/weights.hip) and of the bf16 weight split (wsplit_kernel and
wsplit_batched_kernel of csrc/conv_x6c.hip).  Fold, pack, plain unpack and the split are compared EXACTLY: the inputs of
tests/weightprep_cases.py are integer valued (or, for the split, compared bit for bit), so the expected tensors do not depend on
summation order and the comparison is torch.equal -- padded columns and out-of-group entries included.  Spectral norm and the
spectral-norm unpack cannot be exact; they are compared with the float64 oracle under the bounds test_ops_gpu.py uses for the same
quantities (TOL_OP, TOL_WGRAD).  test_weightprep_cpu.py checks the case tables on the CPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import weightprep_cases as wc
from conftest import rel_err
from test_ops_gpu import TOL_OP, TOL_WGRAD

pytestmark = pytest.mark.gpu

POISON = 12345.0          # what an output holds before a call that must refuse (and so must not write)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from p2igan_bench import ops as o
    o._hip.load()
    return o


@pytest.fixture(params=["det", "atomic"])
def reduce(request, ops):
    """How the cross-workgroup sums end: "det" = partials in the registered scratch, added in a fixed order (the default);
    "atomic" = the scratch unregistered for the test, the kernels fall back to float atomics."""
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.det_ready(dev)
    orig = ops._DET[dev.index]
    if request.param == "det":
        if orig is None:
            raise RuntimeError("the deterministic scratch is not registered (P2I_DETERMINISTIC=0?)")
        yield "det"
        return
    lib = ops._hip.load()
    torch.cuda.synchronize()
    ops._hip.check(lib.p2i_det_workspace(None, 0, None, 0), "p2i_det_workspace")
    ops._DET[dev.index] = None
    try:
        yield "atomic"
    finally:
        torch.cuda.synchronize()
        if orig is not None:
            ops._hip.check(lib.p2i_det_workspace(orig[0].data_ptr(), orig[0].numel(), orig[1].data_ptr(), orig[1].numel()), "p2i_det_workspace")
        ops._DET[dev.index] = orig


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _eq(got, want):
    return torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------ DO-Conv fold
@functools.lru_cache(maxsize=None)
def _fold_ref(c, seed=0):
    inp = wc.fold_inputs(c, seed)
    return inp, wc.fold_expected(c, *inp)


@pytest.mark.parametrize("c", wc.FOLD_CASES, ids=wc.case_id)
def test_fold_exact(ops, c):
    O, I, g, ksz, rep, _ = c
    (W, D, Dd, dwp), (ef, ed, edW, edD) = _fold_ref(c)
    Wg, Dg, Ddg, gg = _cuda(W, D, Dd, dwp)
    wp_f, wp_d = ops.doconv_fold(Wg, Dg, Ddg, O, I, g, ksz, identity_rep=rep)
    assert _eq(wp_f, ef), "wp_f"                     # zeros in the padded columns and outside the group included
    assert _eq(wp_d, ed), "wp_d"
    dW, dD = ops.doconv_fold_bwd(gg, Wg, Dg, Ddg, O, I, g, ksz)
    assert _eq(dW, edW), "dW"
    if ksz == 3:
        assert _eq(dD, edD), "dD"
    else:
        assert dD is None
    # caller-owned gradient targets are written in place
    tW = torch.full_like(Wg, POISON)
    tD = torch.full_like(Dg, POISON) if ksz == 3 else None
    ops.doconv_fold_bwd(gg, Wg, Dg, Ddg, O, I, g, ksz, out=(tW, tD))
    assert _eq(tW, edW) and (tD is None or _eq(tD, edD))


@pytest.mark.parametrize("c", wc.FOLD_NO_D, ids=wc.case_id)
def test_fold_without_the_dgrad_layout(ops, c):
    O, I, g, ksz, rep, _ = c
    (W, D, Dd, _), (ef, _, _, _) = _fold_ref(c)
    wp_f, wp_d = ops.doconv_fold(*_cuda(W, D, Dd), O, I, g, ksz, identity_rep=rep, need_d=False)
    assert wp_d is None and _eq(wp_f, ef)


@pytest.mark.parametrize("c", wc.FOLD_REFUSED, ids=wc.case_id)
def test_fold_refuses_an_identity_skip_that_does_not_exist(ops, c):
    """identity_rep stands for `+ x.repeat_interleave(rep, dim=1)`: defined for a 3x3 layer with I * rep == O only"""
    O, I, g, ksz, rep, _ = c
    W, D, Dd, _ = wc.fold_inputs(c)
    lib = ops._hip.load()
    Wg, Dg, Ddg = _cuda(W, D, Dd)
    nt = ksz * ksz
    f = torch.full((nt, I, wc.pad32(O)), POISON, device="cuda")
    d = torch.full((nt, O, wc.pad32(I)), POISON, device="cuda")
    rc = lib.p2i_doconv_fold_fwd(Wg.data_ptr(), None if Dg is None else Dg.data_ptr(), None if Ddg is None else Ddg.data_ptr(), O, I, g,
                                 ksz, rep, f.data_ptr(), d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"identity_rep" in lib.p2i_last_error()
    assert bool((f == POISON).all()) and bool((d == POISON).all())
    with pytest.raises(RuntimeError):
        ops.doconv_fold(Wg, Dg, Ddg, O, I, g, ksz, identity_rep=rep)


@pytest.mark.parametrize("need_d", [True, False], ids=["need_d", "no_d"])
@pytest.mark.parametrize("n", wc.FOLD_BATCHED_N)
@pytest.mark.parametrize("shape", wc.FOLD_BATCHED_SHAPES, ids=wc.case_id)
def test_fold_batched_exact(ops, shape, n, need_d):
    """against the exact restatement, not against the per-layer call; different seeded data per layer"""
    O, I = shape
    c = (O, I, 1, 3, 0, "eye")
    refs = [_fold_ref(c, seed) for seed in range(n)]
    layers = [tuple(_cuda(W, D, Dd)) for (W, D, Dd, _), _ in refs]
    out = ops.doconv_fold_batched(layers, O, I, need_d=need_d)
    assert len(out) == n
    for L, ((f, d), (_, (ef, ed, _, _))) in enumerate(zip(out, refs)):
        assert _eq(f, ef), ("wp_f", L)
        assert (d is None and not need_d) or _eq(d, ed), ("wp_d", L)
    if need_d:                                       # the backward has no such switch: once per (shape, n)
        dwps = [inp[3].cuda() for inp, _ in refs]
        dWs, dDs = ops.doconv_fold_bwd_batched(dwps, layers, O, I)
        for L, (dW, dD, (_, (_, _, edW, edD))) in enumerate(zip(dWs, dDs, refs)):
            assert _eq(dW, edW), ("dW", L)
            assert _eq(dD, edD), ("dD", L)
        tW = [torch.full((O, I, 9), POISON, device="cuda") for _ in range(n)]
        tD = [torch.full((I, 9, 9), POISON, device="cuda") for _ in range(n)]
        ops.doconv_fold_bwd_batched(dwps, layers, O, I, outs=(tW, tD))
        for L, (_, (_, _, edW, edD)) in enumerate(refs):
            assert _eq(tW[L], edW) and _eq(tD[L], edD), L


@pytest.mark.parametrize("O,I,n", [(48, 32, 2), (32, 48, 2), (32, 64, 17)], ids=["O48", "I48", "n17"])
def test_fold_batched_refusals_leave_the_outputs_untouched(ops, O, I, n):
    lib = ops._hip.load()
    st = torch.cuda.current_stream().cuda_stream
    W = [wc.ints(O, I, 9, lo=-3, hi=3, seed=L).cuda() for L in range(n)]
    D = [wc.ints(I, 9, 9, lo=-2, hi=2, seed=50 + L).cuda() for L in range(n)]
    Dd = [torch.eye(9).reshape(1, 9, 9).repeat(I, 1, 1).cuda() for _ in range(n)]
    g = [wc.ints(9, I, wc.pad32(O), lo=-3, hi=3, seed=90 + L).cuda() for L in range(n)]
    f = [torch.full((9, I, wc.pad32(O)), POISON, device="cuda") for _ in range(n)]
    d = [torch.full((9, O, wc.pad32(I)), POISON, device="cuda") for _ in range(n)]
    dW = [torch.full((O, I, 9), POISON, device="cuda") for _ in range(n)]
    dD = [torch.full((I, 9, 9), POISON, device="cuda") for _ in range(n)]
    pa = ops._ptr_array
    assert lib.p2i_doconv_fold_fwd_batched(pa(W), pa(D), pa(Dd), n, O, I, pa(f), pa(d), st) != 0
    assert lib.p2i_doconv_fold_bwd_batched(pa(g), pa(W), pa(D), pa(Dd), n, O, I, pa(dW), pa(dD), st) != 0
    torch.cuda.synchronize()
    for t in f + d + dW + dD:
        assert bool((t == POISON).all())
    with pytest.raises(RuntimeError):
        ops.doconv_fold_batched(list(zip(W, D, Dd)), O, I)
    if O % 32 == 0:                                  # (the wrapper's own shape check wants dwp (9, I, O): not the refusal meant here)
        with pytest.raises(RuntimeError):
            ops.doconv_fold_bwd_batched(g, list(zip(W, D, Dd)), O, I)


# ------------------------------------------------------------------------------------------------ pack / unpack
@pytest.mark.parametrize("sigma", wc.PACK_SIGMAS, ids=["plain", "by2", "by0.5"])
@pytest.mark.parametrize("shape", wc.PACK_SHAPES, ids=wc.case_id)
def test_pack_exact(ops, shape, sigma):
    w = wc.pack_weight(shape)
    ef, ed = wc.pack_expected(w, sigma)
    wg = w.cuda()
    sg = None if sigma is None else torch.tensor([sigma], device="cuda")
    f, d = ops.weight_pack(wg, sg)
    assert _eq(f, ef) and _eq(d, ed)                 # the zero padding included
    f, d = ops.weight_pack(wg, sg, need_d=False)
    assert d is None and _eq(f, ef)
    f, d = ops.weight_pack(wg, sg, need_f=False)
    assert f is None and _eq(d, ed)


@pytest.mark.parametrize("need_d", [True, False], ids=["need_d", "no_d"])
def test_pack_batched_exact_and_buffer_reuse(ops, need_d):
    shapes = wc.PACK_SHAPES
    sig = [wc.PACK_SIGMAS[i % 3] for i in range(len(shapes))]
    sg = [None if s is None else torch.tensor([s], device="cuda") for s in sig]
    wa = [wc.pack_weight(sh, seed=1) for sh in shapes]
    out = ops.weight_pack_batched([w.cuda() for w in wa], sg, need_d=need_d)
    for (f, d), w, s in zip(out, wa, sig):
        ef, ed = wc.pack_expected(w, s)
        assert _eq(f, ef) and ((d is None and not need_d) or _eq(d, ed))
    # a reused buffer: zero-filled once, then list A and list B (same shapes, other values) packed into it
    need = sum(nt * i * wc.pad32(o) + (nt * o * wc.pad32(i) if need_d else 0) for o, i, nt in shapes)
    buf = torch.zeros(need, device="cuda")
    ops.weight_pack_batched([w.cuda() for w in wa], sg, need_d=need_d, buf=buf)
    wb = [wc.pack_weight(sh, seed=2) for sh in shapes]
    assert all(not torch.equal(a, b) for a, b in zip(wa, wb) if a.numel() > 1)
    out = ops.weight_pack_batched([w.cuda() for w in wb], sg, need_d=need_d, buf=buf)
    for (f, d), w, s in zip(out, wb, sig):
        ef, ed = wc.pack_expected(w, s)
        assert f.data_ptr() >= buf.data_ptr() and _eq(f, ef) and ((d is None and not need_d) or _eq(d, ed))     # padding still zero, every entry rewritten
    with pytest.raises(RuntimeError):
        ops.weight_pack_batched([w.cuda() for w in wb], sg, need_d=need_d, buf=torch.zeros(need + 1, device="cuda"))


@pytest.mark.parametrize("shape", wc.PACK_SHAPES, ids=wc.case_id)
def test_plain_unpack_exact_and_blind_to_the_padding(ops, shape):
    O = shape[0]
    like = torch.empty(shape, device="cuda")
    g7, g5 = wc.packed_grad(shape, 1, 7), wc.packed_grad(shape, 1, -5)          # same gradient, other garbage in the padding
    want = wc.unpack_expected(g7, O)
    assert _eq(ops.weight_unpack_grad(g7.cuda(), like), want)
    assert _eq(ops.weight_unpack_grad(g5.cuda(), like), want)
    tgt = torch.full(shape, POISON, device="cuda")
    assert ops.weight_unpack_grad(g7.cuda(), like, out=tgt) is tgt and _eq(tgt, want)


def test_plain_unpack_of_one_layer_needs_no_dot_product_scratch(ops, reduce):
    """without sigma the single-layer call hands the launch helper a NULL dot-product slot: nothing is zeroed, summed or read there,
    with the fixed-order scratch registered or not, and the caller's target gets exactly the expected integers"""
    shape = (65, 33, 4)
    g = wc.packed_grad(shape, 1, 7)
    tgt = torch.full(shape, POISON, device="cuda")
    assert ops.weight_unpack_grad(g.cuda(), torch.empty(shape, device="cuda"), out=tgt) is tgt
    torch.cuda.synchronize()
    assert _eq(tgt, wc.unpack_expected(g, shape[0]))


def test_plain_unpack_batched_and_accumulate_exact(ops, reduce):
    shapes = wc.PACK_SHAPES
    likes = [torch.empty(sh, device="cuda") for sh in shapes]
    g1 = [wc.packed_grad(sh, 1, 7) for sh in shapes]
    g1b = [wc.packed_grad(sh, 1, -5) for sh in shapes]
    g2 = [wc.packed_grad(sh, 2, 3) for sh in shapes]
    w1 = [wc.unpack_expected(g, sh[0]) for g, sh in zip(g1, shapes)]
    w2 = [wc.unpack_expected(g, sh[0]) for g, sh in zip(g2, shapes)]
    for gs in (g1, g1b):
        got = ops.weight_unpack_grad_batched([g.cuda() for g in gs], likes)
        for a, b in zip(got, w1):
            assert _eq(a, b)
    tg = [torch.full(sh, POISON, device="cuda") for sh in shapes]
    assert ops.weight_unpack_grad_batched([g.cuda() for g in g1], likes, outs=tg) is tg
    ops.weight_unpack_grad_batched([g.cuda() for g in g2], likes, outs=tg, accumulate=True)
    for t, a, b in zip(tg, w1, w2):
        assert _eq(t, a + b)                         # integers: g1 + g2 exactly
    with pytest.raises(RuntimeError):
        ops.weight_unpack_grad_batched([g.cuda() for g in g2], likes, accumulate=True)
    with pytest.raises(RuntimeError):
        ops.weight_unpack_grad_batched([g.cuda() for g in g2] * 3, likes * 3)                 # 21 layers > 16


@functools.lru_cache(maxsize=None)
def _sn_unpack_ref(shape):
    w, u, v, sigma, g = wc.sn_unpack_inputs(shape)
    return (w, u, v, sigma, g), wc.sn_unpack_expected(w, u, v, g)


def test_spectral_norm_unpack_matches_float64_autograd(ops, reduce):
    """per layer, batched, and batched-accumulate on top of a non-zero target, under both endings of the dot product; the list also
    holds layers WITHOUT sigma, which are unpacked (and accumulated) exactly"""
    shapes = wc.SN_UNPACK_SHAPES
    refs = [_sn_unpack_ref(sh) for sh in shapes]
    plain = [(64, 16, 9), (65, 33, 4)]
    gp = [wc.packed_grad(sh, 3, 9) for sh in plain]
    wp = [wc.unpack_expected(g, sh[0]) for g, sh in zip(gp, plain)]

    def per_layer():
        return [ops.weight_unpack_grad(g.cuda(), w.cuda(), w.cuda(), s.cuda(), u.cuda(), v.cuda()) for (w, u, v, s, g), _ in refs]

    # interleaved: sigma, plain, sigma, plain, sigma
    order = [("s", 0), ("p", 0), ("s", 1), ("p", 1), ("s", 2)]
    dwps = [(refs[i][0][4] if k == "s" else gp[i]).cuda() for k, i in order]
    likes = [torch.empty(shapes[i] if k == "s" else plain[i], device="cuda") for k, i in order]
    col = lambda j: [refs[i][0][j].cuda() if k == "s" else None for k, i in order]
    w_o, us, vs, sg = col(0), col(1), col(2), col(3)
    want = [refs[i][1] if k == "s" else wp[i].double() for k, i in order]

    def batched():
        return ops.weight_unpack_grad_batched(dwps, likes, w_o, sg, us, vs)

    def accumulated():
        tg = [torch.full(tuple(l.shape), 0.5, device="cuda") for l in likes]
        ops.weight_unpack_grad_batched(dwps, likes, w_o, sg, us, vs, outs=tg, accumulate=True)
        return tg

    one = per_layer()
    for got, (_, ref), sh in zip(one, refs, shapes):
        print("sn unpack", sh, reduce, rel_err(got.cpu().numpy(), ref.numpy()))
        assert rel_err(got.cpu().numpy(), ref.numpy()) < TOL_WGRAD
    bat, acc = batched(), accumulated()
    for (k, i), b, a, ref in zip(order, bat, acc, want):
        if k == "p":
            assert _eq(b, ref.float()) and _eq(a, ref.float() + 0.5)        # integers + 0.5: exact
        else:
            print("sn unpack batched", shapes[i], reduce, rel_err(b.cpu().numpy(), ref.numpy()), rel_err(a.cpu().numpy(), (ref + 0.5).numpy()))
            assert rel_err(b.cpu().numpy(), ref.numpy()) < TOL_WGRAD
            assert rel_err(a.cpu().numpy(), (ref + 0.5).numpy()) < TOL_WGRAD
    if reduce == "det":                              # the fixed-order ending: the same bits on a second run
        for x, y in zip(one + bat + acc, per_layer() + batched() + accumulated()):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ bf16 split
def _u16(t):
    return t.cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _split_ref(shape, seed=0):
    a = wc.split_values(shape, seed)
    return a, wc.split_image(a)


@pytest.mark.parametrize("shape", wc.SPLIT_SHAPES + [wc.SPLIT_STRIDE_SHAPE], ids=wc.case_id)
def test_split_bit_for_bit(ops, shape):
    ntaps, K, Mpad = shape
    a, img = _split_ref(shape)
    wp = torch.from_numpy(a).cuda()
    wb = torch.zeros(3 * wp.numel() + 64, device="cuda", dtype=torch.int16)       # 64 guard elements behind the image
    lib = ops._hip.load()
    ops._hip.check(lib.p2i_x6_split(wp.data_ptr(), wb.data_ptr(), ntaps, K, Mpad, torch.cuda.current_stream().cuda_stream), "p2i_x6_split")
    got = _u16(wb)
    assert np.array_equal(got[:img.size], img)
    assert not got[img.size:].any()


def _split_batched(ops, arrays, wbs=None):
    n = len(arrays)
    wps = [torch.from_numpy(a).cuda() for a in arrays]
    if wbs is None:
        wbs = [torch.zeros(3 * w.numel() + 64, device="cuda", dtype=torch.int16) for w in wps]
    arr = ctypes.c_int * n
    rc = ops._hip.load().p2i_x6_split_batched(ops._ptr_array(wps), ops._ptr_array(wbs), arr(*[a.shape[0] for a in arrays]),
                                              arr(*[a.shape[1] for a in arrays]), arr(*[a.shape[2] for a in arrays]), n,
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, wbs


def test_split_batched_bit_for_bit(ops):
    refs = [_split_ref(sh) for sh in wc.SPLIT_SHAPES]
    rc, wbs = _split_batched(ops, [a for a, _ in refs])
    assert rc == 0
    for wb, (_, img) in zip(wbs, refs):
        got = _u16(wb)
        assert np.array_equal(got[:img.size], img) and not got[img.size:].any()
    # the limit of 24 tensors (different data in each), 25 refused, K = 12 refused
    many = [_split_ref(wc.SPLIT_SHAPES[i % 4], seed=i) for i in range(wc.SPLIT_BATCH_MAX)]
    rc, wbs = _split_batched(ops, [a for a, _ in many])
    assert rc == 0
    for wb, (_, img) in zip(wbs, many):
        assert np.array_equal(_u16(wb)[:img.size], img)
    arrays = [a for a, _ in many] + [many[0][0]]
    poison = [torch.full((3 * a.size,), 77, device="cuda", dtype=torch.int16) for a in arrays]
    rc, _ = _split_batched(ops, arrays, poison)
    assert rc != 0 and all(bool((p == 77).all()) for p in poison)
    bad = [refs[0][0], np.ones((1, 12, 32), dtype=np.float32)]
    poison = [torch.full((3 * a.size,), 77, device="cuda", dtype=torch.int16) for a in bad]
    rc, _ = _split_batched(ops, bad, poison)
    assert rc != 0 and all(bool((p == 77).all()) for p in poison)
    wb = torch.full((3 * 12 * 32,), 77, device="cuda", dtype=torch.int16)
    assert ops._hip.load().p2i_x6_split(torch.ones(1, 12, 32, device="cuda").data_ptr(), wb.data_ptr(), 1, 12, 32,
                                        torch.cuda.current_stream().cuda_stream) != 0
    torch.cuda.synchronize()
    assert bool((wb == 77).all())


def test_presplit_helpers_hand_the_convolution_the_same_image(ops, monkeypatch):
    """ops.X6Stack (a stack of same-shape layers split as ntaps = n * taps) and ops.x6_presplit (tensors of different shapes): the
    pointer of layer i holds exactly the restated planes of layer i"""
    monkeypatch.setattr(ops, "CONV_ENGINE", "auto")          # the helpers do nothing when the split pipe is switched off
    n, (taps, K, Mpad) = 3, (9, 16, 64)
    layers = [wc.split_values((taps, K, Mpad), seed=10 + i) for i in range(n)]
    stack = torch.from_numpy(np.stack(layers)).cuda()
    st = ops.X6Stack(stack)
    per = taps * K * Mpad
    for i in (1, 0, 2):
        off = (st.layer_ptr(i) - st.wb.data_ptr()) // 2
        assert off == i * per
        got = _u16(st.wb)
        img = wc.split_image(layers[i]).reshape(3, per)
        for plane in range(3):                       # the planes of the stack lie n * per apart
            assert np.array_equal(got[plane * n * per + off:plane * n * per + off + per], img[plane]), (i, plane)
    views = [stack[i] for i in range(n)]
    ops.X6Stack.attach(stack, views)
    assert all(v._x6s[1] == i and v._x6s[0].n == n for i, v in enumerate(views))
    tensors = [torch.from_numpy(_split_ref(sh)[0]).cuda() for sh in wc.SPLIT_SHAPES]
    wants = [True, True, False, True]
    buf = ops.x6_presplit(tensors, wants)
    assert not hasattr(tensors[2], "_x6s")
    assert not hasattr(tensors[0], "_x6s")           # K = 8: the split pipe wants K % 16 == 0, the helper leaves the tensor out
    full = _u16(buf)
    for t, sh in [(tensors[1], wc.SPLIT_SHAPES[1]), (tensors[3], wc.SPLIT_SHAPES[3])]:
        h, i = t._x6s
        off = (h.layer_ptr(i) - buf.data_ptr()) // 2
        img = _split_ref(sh)[1]
        assert h.taps == sh[0] and np.array_equal(full[off:off + img.size], img)


# ------------------------------------------------------------------------------------------------ spectral norm
@functools.lru_cache(maxsize=None)
def _sn_ref(shape, seed=0):
    w, u, v = wc.sn_inputs(shape, seed)
    return (w, u, v), wc.sn_expected(w, u, v, True), wc.sn_expected(w, u, v, False)


def _sn_close(got, ref, what):
    e = rel_err(got.cpu().numpy(), ref.numpy())
    print("spectral norm", what, e)
    assert e < TOL_OP, (what, e)


@pytest.mark.parametrize("shape", wc.SN_SHAPES, ids=wc.case_id)
def test_spectral_norm_matches_float64(ops, shape):
    """p2i_spectral_norm is a batch of one of the batched kernels: no sum crosses a workgroup (a column of W^T u is summed by the four
    row groups of ONE workgroup, whatever O is; K > 64 only adds workgroups with columns of their own), nothing is atomic and no
    scratch of the fixed-order sums is read -- a single ending, and a second run from the same inputs gives the same bits."""
    (w, u, v), (un, vn, sn), (_, _, se) = _sn_ref(shape)
    wg, ug, vg = _cuda(w, u, v)
    sigma = ops.spectral_norm(wg, ug, vg, True)
    _sn_close(ug, un, "u"), _sn_close(vg, vn, "v"), _sn_close(sigma, sn.reshape(1), "sigma")
    u2, v2 = u.cuda(), v.cuda()
    assert torch.equal(ops.spectral_norm(wg, u2, v2, True), sigma) and torch.equal(u2, ug) and torch.equal(v2, vg)
    ue, ve = u.cuda(), v.cuda()
    s2 = ops.spectral_norm(wg, ue, ve, False)
    assert _eq(ue, u) and _eq(ve, v)                 # eval: u, v untouched
    _sn_close(s2, se.reshape(1), "sigma (eval)")
    assert torch.equal(ops.spectral_norm(wg, ue, ve, False), s2)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_spectral_norm_single_call_is_the_batched_call(ops, training):
    """a layer's arithmetic does not depend on what else is in the batch: every SN_SHAPES layer alone == the whole list at once,
    bit for bit"""
    refs = [_sn_ref(sh) for sh in wc.SN_SHAPES]
    ws = [r[0][0].cuda() for r in refs]
    u1, v1 = [r[0][1].cuda() for r in refs], [r[0][2].cuda() for r in refs]
    ub, vb = [r[0][1].cuda() for r in refs], [r[0][2].cuda() for r in refs]
    s1 = [ops.spectral_norm(w, u, v, training) for w, u, v in zip(ws, u1, v1)]
    sb = ops.spectral_norm_batched(ws, ub, vb, training)
    for i, sh in enumerate(wc.SN_SHAPES):
        assert torch.equal(s1[i], sb[i]) and torch.equal(u1[i], ub[i]) and torch.equal(v1[i], vb[i]), sh


def test_spectral_norm_of_a_zero_weight(ops):
    O, K = wc.SN_ZERO_SHAPE
    _, u, v = wc.sn_inputs(wc.SN_ZERO_SHAPE)
    for batched in (False, True):
        wg, ug, vg = torch.zeros(O, K, device="cuda"), u.cuda(), v.cuda()
        sigma = ops.spectral_norm_batched([wg], [ug], [vg], True)[0] if batched else ops.spectral_norm(wg, ug, vg, True)
        for t in (ug, vg, sigma):                    # F.normalize(0, eps=1e-12) = 0 / 1e-12 = 0: zeros, nothing NaN
            assert _eq(t, torch.zeros(t.shape)), batched


@pytest.mark.parametrize("n", [len(wc.SN_SHAPES), wc.SN_MAX_LAYERS], ids=["list", "16_layers"])
def test_spectral_norm_batched_matches_float64(ops, n):
    cases = [(wc.SN_SHAPES[i % len(wc.SN_SHAPES)], i // len(wc.SN_SHAPES)) for i in range(n)]
    refs = [_sn_ref(sh, seed) for sh, seed in cases]
    ws = [r[0][0].cuda() for r in refs]
    us, vs = [r[0][1].cuda() for r in refs], [r[0][2].cuda() for r in refs]
    sig, usn, vsn = ops.spectral_norm_batched(ws, us, vs, True, snapshot=True)
    for i, (_, (un, vn, sn), _) in enumerate(refs):
        _sn_close(us[i], un, ("u", cases[i])), _sn_close(vs[i], vn, ("v", cases[i])), _sn_close(sig[i], sn.reshape(1), ("sigma", cases[i]))
        assert torch.equal(usn[i], us[i]) and torch.equal(vsn[i], vs[i])          # the snapshots: the updated vectors bit for bit
        assert usn[i].data_ptr() != us[i].data_ptr()
    ue, ve = [r[0][1].cuda() for r in refs], [r[0][2].cuda() for r in refs]
    sig = ops.spectral_norm_batched(ws, ue, ve, False)
    for i, (inp, _, (_, _, se)) in enumerate(refs):
        assert _eq(ue[i], inp[1]) and _eq(ve[i], inp[2])                          # eval: u, v untouched
        _sn_close(sig[i], se.reshape(1), ("sigma (eval)", cases[i]))


def test_spectral_norm_batched_refuses_17_layers(ops):
    w, u, v = _cuda(*wc.sn_inputs((5, 3)))
    n = wc.SN_MAX_LAYERS + 1
    us, vs = [u.clone() for _ in range(n)], [v.clone() for _ in range(n)]
    with pytest.raises(RuntimeError):
        ops.spectral_norm_batched([w] * n, us, vs, True)
    lib = ops._hip.load()
    sig, scr = torch.full((n,), POISON, device="cuda"), torch.zeros(n, 16, device="cuda")
    arr_p, arr_i = ctypes.c_void_p * n, ctypes.c_int * n
    rc = lib.p2i_spectral_norm_batched(arr_p(*[w.data_ptr()] * n), arr_i(*[5] * n), arr_i(*[3] * n), arr_p(*[t.data_ptr() for t in us]),
                                       arr_p(*[t.data_ptr() for t in vs]), 1, arr_p(*[sig.data_ptr() + 4 * i for i in range(n)]),
                                       arr_p(*[scr[i].data_ptr() for i in range(n)]), None, None, n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and bool((sig == POISON).all())
    assert all(torch.equal(t, u) for t in us) and all(torch.equal(t, v) for t in vs)
