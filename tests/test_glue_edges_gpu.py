"""Edge shapes of the glue and loss kernels (csrc/glue.hip, csrc/loss.hip): second trips of strided loops, workgroups that walk
several chunks, partial last chunks, unaligned fallbacks, non-square and odd maps, and BOTH ends of every cross-workgroup sum -- the
deterministic scratch and the float atomics.  The reference is the same operation in float64 torch on the CPU, gradients by autograd;
pure copy / select operations are compared bit for bit with float32 torch.  Every bound is one the project already uses: TOL_OP and
TOL_WGRAD of test_ops_gpu.py, the per-scalar bounds of its loss and Adam tests, TOL / GTOL of the end-to-end tests.  The inputs come
from tests/glue_cases.py; test_glue_cases_cpu.py checks their margins."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as gc
from conftest import rel_err
from fullsize import GTOL, TOL
from test_ops_gpu import TOL_OP, TOL_WGRAD

pytestmark = pytest.mark.gpu

F64 = torch.float64


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


def _flat(r):
    return [t for t in (r if isinstance(r, (tuple, list)) else (r,)) if t is not None]


def _run(reduce, fn):
    """fn's result; with the deterministic sums a second run must give the same bits."""
    r = fn()
    if reduce == "det":
        again = fn()
        for a, b in zip(_flat(r), _flat(again)):
            assert torch.equal(a, b), float((a - b).abs().max())
    return r


def _err(got, ref):
    return rel_err(got.detach().cpu().numpy(), ref.detach().numpy())


def _act_code(ops, act):
    return {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY, "tanh": ops.ACT_TANH}[act]


# ------------------------------------------------------------------------------------------------ discriminator tail
@functools.lru_cache(maxsize=None)
def _dtail_ref(dims):
    inp = gc.dtail_inputs(dims)
    o2, o3, alpha = (inp[k].to(F64).requires_grad_(True) for k in ("o2", "o3", "alpha"))
    z2 = o3.mean(dim=2)
    if z2.shape[-2:] != o2.shape[-2:]:
        z2 = F.interpolate(z2, size=o2.shape[-2:], mode="bilinear", align_corners=False)
    fused = (torch.sigmoid(alpha) * o2 + z2).view(gc.DTAIL_B, -1)
    fused.backward(inp["gout"].to(F64))
    return inp, fused.detach(), o2.grad, o3.grad, float(alpha.grad)


@pytest.mark.parametrize("dims", gc.DTAIL_CASES, ids=gc.case_id)
def test_dtail(ops, reduce, dims):
    inp, fused, d2r, d3r, dar = _dtail_ref(dims)
    o2, o3, alpha, gout = (inp[k].cuda() for k in ("o2", "o3", "alpha", "gout"))
    print("dtail", dims, "fused", _err(ops.dtail_fwd(o2, o3, alpha), fused))
    assert _err(ops.dtail_fwd(o2, o3, alpha), fused) < TOL_OP
    d2, d3, da = _run(reduce, lambda: ops.dtail_bwd(o2, tuple(o3.shape), alpha, gout))
    print("dtail", dims, reduce, "d2", _err(d2, d2r), "d3", _err(d3, d3r), "dalpha", float(da), dar)
    assert _err(d2, d2r) < TOL_OP
    assert _err(d3, d3r) < TOL_OP
    assert abs(float(da) - dar) < TOL_WGRAD * abs(dar) + 1e-7
    d2n, d3n, dan = ops.dtail_bwd(o2, tuple(o3.shape), alpha, gout, need_alpha=False)
    assert dan is None and torch.equal(d2n, d2) and torch.equal(d3n, d3)
    # a caller-owned alpha gradient is ADDED to
    held = torch.full((1,), 0.5, device="cuda")
    _, _, da2 = ops.dtail_bwd(o2, tuple(o3.shape), alpha, gout, da_out=held)
    assert da2 is held
    if reduce == "det":
        assert torch.equal(held, 0.5 + da)
    assert abs(float(held) - (0.5 + dar)) < TOL_WGRAD * abs(dar) + 1e-7


def test_discriminator_on_a_clip_whose_maps_are_no_integer_multiple(ops):
    """P2IDiscriminator on a 36 x 28 clip (both = 4 mod 8): the 2-D branch ends at 9 x 7, the 3-D branch at 5 x 4, and the tail
    upsamples 5 x 4 to 9 x 7.  Logits, input gradient and every parameter gradient against the oracle in float64, at the end-to-end
    tests' bounds for these quantities (logits TOL, gradients GTOL)."""
    from oracle import p2i_oracle as orc
    from p2igan_bench.models.p2igan import P2IDiscriminator
    from p2igan_bench.utils import seeded
    B, T, _, H, W = gc.DISC_CLIP
    frames = seeded.synthetic_batch(B, T, H, W, seeded.gauge_mask(H, W, 20))[0]
    gout = gc.rand(B, 9 * 7, seed=5)
    state = {k: v.to(F64).clone() for k, v in seeded.seeded_discriminator_state().items()}
    for k, v in state.items():
        if not k.endswith(("weight_u", "weight_v")):
            v.requires_grad_(True)
    xr = frames.to(F64).requires_grad_(True)
    lref = orc.discriminator_forward(state, xr, training=True)
    assert lref.shape == (B, 9 * 7)
    lref.backward(gout.to(F64))

    D = P2IDiscriminator(T).cuda()
    D.load_state_dict(seeded.seeded_discriminator_state())
    D.train()
    xg = frames.cuda().requires_grad_(True)
    logits = D(xg)
    logits.backward(gout.cuda())
    print("disc logits", _err(logits, lref.detach()), "dx", _err(xg.grad, xr.grad))
    assert _err(logits, lref.detach()) < TOL
    assert _err(xg.grad, xr.grad) < GTOL
    checked = 0
    for n, p in D.named_parameters():
        if state[n].grad is None:                                   # alpha3d: declared, unused by the forward
            assert p.grad is None or float(p.grad.abs().sum()) == 0.0, n
            continue
        print("disc grad", n, _err(p.grad, state[n].grad))
        assert _err(p.grad, state[n].grad) < GTOL, n
        checked += 1
    assert checked == 21                                            # ten layers' weight and bias, alpha2d


# ------------------------------------------------------------------------------------------------ attention
@functools.lru_cache(maxsize=None)
def _attn_ref(case):
    inp = gc.attn_inputs(case)
    out, grads, _, _ = gc.attn_reference(inp)
    return inp, out, grads


@pytest.mark.parametrize("case", gc.ATTN_CASES, ids=gc.attn_id)
def test_attention(ops, reduce, case):
    inp, out, grads = _attn_ref(case)
    args = [inp[k].cuda().contiguous() for k in ("x", "w0", "b0", "w1", "b1")]
    assert _err(ops.attn_fwd(*args), out) < TOL_OP
    gout = inp["gout"].cuda().contiguous()
    got = _run(reduce, lambda: ops.attn_bwd(*args, gout))
    print("attn", case, reduce, [_err(g, r) for g, r in zip(got, grads)])
    for g, r in zip(got, grads):
        assert g.shape == r.shape and _err(g, r) < TOL_WGRAD


# ------------------------------------------------------------------------------------------------ pool + duplicate
def _pooldup_check(ops, inp):
    from oracle import p2i_oracle as orc
    x, gout = inp["x"], inp["gout"]
    assert torch.equal(ops.pooldup_fwd(x.cuda()).cpu(), orc.pool_dup(x, 1))
    xr = x.to(F64).requires_grad_(True)
    orc.pool_dup(xr, 1).backward(gout.to(F64))
    dx = ops.pooldup_bwd(x.cuda(), gout.cuda())
    assert _err(dx, xr.grad) < TOL_OP
    assert torch.equal(dx.cpu() != 0, xr.grad != 0)                 # the gradient lands on the first maximum in scan order, nowhere else


@pytest.mark.parametrize("shape", gc.POOLDUP_CASES + [gc.POOLDUP_BIG], ids=gc.case_id)
def test_pooldup(ops, shape):
    _pooldup_check(ops, gc.pooldup_inputs(shape))


def test_pooldup_ties_at_every_window_position(ops):
    _pooldup_check(ops, gc.pooldup_all_ties())


@pytest.mark.parametrize("shape", [(1, 1, 3, 2), (1, 2, 2, 5)], ids=gc.case_id)
def test_pooldup_refuses_odd_maps(ops, shape):
    B, C, H, W = shape
    x = torch.zeros(shape, device="cuda")
    with pytest.raises(RuntimeError):
        ops.pooldup_fwd(x)
    with pytest.raises(RuntimeError):
        ops.pooldup_bwd(x, torch.zeros(B, 2 * C, H // 2, W // 2, device="cuda"))


# ------------------------------------------------------------------------------------------------ upsample + modulate
@functools.lru_cache(maxsize=None)
def _upmod_ref(case):
    inp = gc.upmod_inputs(case)
    x, pos = inp["x"].to(F64).requires_grad_(True), inp["pos"].to(F64).requires_grad_(True)
    u = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    u = u + u * (2 * torch.sigmoid(pos) - 1)
    u.backward(inp["gout"].to(F64))
    with torch.no_grad():
        acts = {a: gc.act_torch(u + inp["bias"].to(F64).view(1, -1, 1, 1), a) for a in gc.ACTS}
    return inp, u.detach(), acts, x.grad, pos.grad


@pytest.mark.parametrize("case", gc.UPMOD_CASES, ids=gc.case_id)
def test_upmod_fwd(ops, case):
    inp, u, acts, _, _ = _upmod_ref(case)
    x, pos, bias = inp["x"].cuda(), inp["pos"].cuda(), inp["bias"].cuda()
    assert _err(ops.upmod_fwd(x, pos), u) < TOL_OP
    for a in gc.ACTS:
        assert _err(ops.upmod_fwd(x, pos, bias=bias, act=_act_code(ops, a)), acts[a]) < TOL_OP, a


@pytest.mark.parametrize("case", gc.UPMOD_CASES, ids=gc.case_id)
def test_upmod_bwd(ops, reduce, case):
    inp, _, _, dxr, dposr = _upmod_ref(case)
    x, pos, gout = inp["x"].cuda(), inp["pos"].cuda(), inp["gout"].cuda()
    dx, dpos = _run(reduce, lambda: ops.upmod_bwd(x, pos, gout))
    print("upmod", case, reduce, "dx", _err(dx, dxr), "dpos", _err(dpos, dposr))
    assert _err(dx, dxr) < TOL_OP
    assert dpos.shape == pos.shape and _err(dpos, dposr) < TOL_WGRAD
    none, dpos2 = ops.upmod_bwd(x, pos, gout, need_dx=False)
    assert none is None and _err(dpos2, dposr) < TOL_WGRAD
    if reduce == "det":
        assert torch.equal(dpos2, dpos)


# ------------------------------------------------------------------------------------------------ bias / activation gradients
@functools.lru_cache(maxsize=None)
def _bias_ref(case, act):
    inp = gc.bias_inputs(case, act)
    pre = inp["pre"].to(F64).requires_grad_(True)
    gc.act_torch(pre, act).backward(inp["dy"].to(F64))
    dims = [d for d in range(pre.dim()) if d != 1]
    return inp, pre.grad, pre.grad.sum(dim=dims), inp["dy"].to(F64).sum(dim=dims)


def _act_bwd_f32(dy, y, act):
    """the selecting activations' backward in float32 torch: what act_bwd must give bit for bit"""
    return {"none": dy, "relu": torch.where(y > 0, dy, torch.zeros_like(dy)), "leaky": torch.where(y > 0, dy, dy * 0.2)}[act]


@pytest.mark.parametrize("case", gc.BIAS_CASES, ids=gc.case_id)
def test_bias_grad_and_act_bwd_bias(ops, reduce, case):
    for act in gc.ACTS:
        inp, dzr, dbr, dyr = _bias_ref(case, act)
        dy, y, code = inp["dy"].cuda(), inp["y"].cuda(), _act_code(ops, act)
        if act == "none":
            db0 = _run(reduce, lambda: ops.bias_grad(dy))
            assert db0.shape == dyr.shape and _err(db0, dyr) < TOL_WGRAD
        db1 = _run(reduce, lambda: ops.bias_grad(dy, y, code))
        dz, db2 = _run(reduce, lambda: ops.act_bwd_bias(dy, y, code))
        print("bias", case, act, reduce, _err(db1, dbr), _err(db2, dbr), _err(dz, dzr))
        assert _err(db1, dbr) < TOL_WGRAD, act
        assert _err(db2, dbr) < TOL_WGRAD, act
        assert dz.shape == dy.shape and _err(dz, dzr) < TOL_OP, act
        if act != "tanh":
            assert torch.equal(dz.cpu(), _act_bwd_f32(inp["dy"], inp["y"], act)), act
        # a caller-owned target is added into
        held = ops.zero_(torch.empty(case[1], device="cuda"))
        assert ops.bias_grad(dy, y, code, out=held) is held and _err(held, dbr) < TOL_WGRAD


@pytest.mark.parametrize("n", gc.ACT_BWD_N)
def test_act_bwd(ops, n):
    dy, pre = gc.rand(n, seed=20), gc.kinked(n, seed=21)
    for act in gc.ACTS:
        y = gc.act_torch(pre, act)
        got = ops.act_bwd(dy.cuda(), y.cuda(), _act_code(ops, act)).cpu()
        if act != "tanh":
            assert torch.equal(got, _act_bwd_f32(dy, y, act)), act
        else:
            p64 = pre.to(F64).requires_grad_(True)
            torch.tanh(p64).backward(dy.to(F64))
            assert _err(got, p64.grad) < TOL_OP


@pytest.mark.parametrize("n", gc.ADD2_N)
def test_add2_aligned_and_unaligned(ops, n):
    a, b = gc.rand(n + 2, seed=30).cuda(), gc.rand(n + 2, seed=31).cuda()
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    assert torch.equal(ops.add2(a[:n], b[:n]), a[:n] + b[:n])                     # float4 body + tail
    for va, vb in ((a[1:1 + n], b[1:1 + n]), (a[:n], b[1:1 + n]), (a[1:1 + n], b[:n])):
        assert (va.data_ptr() | vb.data_ptr()) % 16 != 0
        assert torch.equal(ops.add2(va, vb), va + vb)                              # the scalar fallback


@pytest.mark.parametrize("n", [1, 1027, 8192 * 256 + 5])
def test_zero_and_axpy_touch_only_their_slice(ops, n):
    base, other = gc.rand(n + 8, seed=32).cuda(), gc.rand(n + 8, seed=33).cuda()
    y0, x = base.clone(), other[1:1 + n]
    y = base[5:5 + n]
    assert ops.axpy_(y, x, 1.0) is y
    assert torch.equal(y, y0[5:5 + n] + x)
    assert torch.equal(base[:5], y0[:5]) and torch.equal(base[5 + n:], y0[5 + n:])
    y1 = base.clone()
    ops.axpy_(y, x, -0.37)
    ref = y1[5:5 + n].cpu().to(F64) - 0.37 * x.cpu().to(F64)
    assert _err(y, ref) < TOL_OP
    assert torch.equal(base[:5], y0[:5]) and torch.equal(base[5 + n:], y0[5 + n:])
    y2 = base.clone()
    ops.zero_(base[3:3 + n])
    assert float(base[3:3 + n].abs().max()) == 0.0 and float(y2[3:3 + n].abs().min()) > 0.0
    assert torch.equal(base[:3], y2[:3]) and torch.equal(base[3 + n:], y2[3 + n:])


# ------------------------------------------------------------------------------------------------ Adam
@functools.lru_cache(maxsize=None)
def _adam_ref(n, betas):
    inp = gc.adam_inputs(n)
    ref = inp["p"].to(F64).clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-4, betas=betas)
    for g in inp["grads"]:
        ref.grad = g.to(F64)
        opt.step()
    return inp, ref.detach()


@pytest.mark.parametrize("betas", gc.ADAM_BETAS, ids=gc.case_id)
@pytest.mark.parametrize("n", gc.ADAM_N)
def test_adam(ops, n, betas):
    inp, ref = _adam_ref(n, betas)
    z = lambda: torch.zeros(n, device="cuda")
    p, m, v = inp["p"].cuda(), z(), z()
    pd, md, vd = inp["p"].cuda(), z(), z()
    step_dev, coef = torch.zeros(1, device="cuda", dtype=torch.int32), torch.zeros(2, device="cuda")
    for step, g in enumerate(inp["grads"], 1):
        gg = g.cuda()
        ops.adam_step(p, gg, m, v, 1e-4, betas[0], betas[1], 1e-8, step)
        ops.adam_step_dev(pd, gg, md, vd, 1e-4, betas[0], betas[1], 1e-8, step_dev, coef)
        assert int(step_dev) == step
    print("adam", n, betas, _err(p, ref), _err(pd, ref), _err(pd, p.cpu()))
    assert _err(p, ref) < 1e-6
    assert _err(pd, ref) < 1e-6
    assert _err(pd, p.cpu()) < 1e-6 and _err(md, m.cpu()) < 1e-6 and _err(vd, v.cpu()) < 1e-6
    assert float((p.cpu() - inp["p"]).abs().max()) > 1e-5
    zero = inp["grads"][0] == 0                                                    # no gradient in any step: the parameter stays
    assert torch.equal(p.cpu()[zero], inp["p"][zero]) and torch.equal(pd.cpu()[zero], inp["p"][zero])


# ------------------------------------------------------------------------------------------------ reconstruction loss
@pytest.mark.parametrize("shape", gc.RECLOSS_CASES, ids=gc.case_id)
def test_recloss(ops, shape):
    from oracle import p2i_oracle as orc
    inp = gc.recloss_inputs(shape)
    pred = inp["pred"].to(F64).requires_grad_(True)
    loss, pool, reg = orc.reconstruction_loss(pred, inp["true"].to(F64), 0.05)
    loss.backward()
    out3, dpred = ops.recloss(inp["pred"].cuda(), inp["true"].cuda(), 0.05)
    o = out3.cpu().numpy().astype(np.float64)
    print("recloss", shape, o, float(pool), float(reg), float(loss), _err(dpred, pred.grad))
    assert abs(o[0] - float(pool)) < 1e-5 * abs(float(pool))
    assert abs(o[1] - float(reg)) < 1e-4 * abs(float(reg))
    assert abs(o[2] - float(loss)) < 1e-4 * abs(float(loss))
    assert _err(dpred, pred.grad) < 1e-4


def test_recloss_refuses_a_batch_beyond_its_scratch_tail(ops):
    B, T, H, W = gc.RECLOSS_REFUSED
    z = torch.zeros(B, T, 1, H, W, device="cuda")
    with pytest.raises(RuntimeError, match="scratch tail"):
        ops.recloss(z, z, 0.05)


# ------------------------------------------------------------------------------------------------ GAN losses
@pytest.mark.parametrize("labels", gc.GAN_LABELS, ids=gc.case_id)
@pytest.mark.parametrize("lt", ["hinge", "lsgan", "nsgan"])
@pytest.mark.parametrize("n", gc.GAN_N)
def test_gan_losses(ops, n, lt, labels):
    """Discriminator and generator terms with their gradients; nsgan's logits hold exact 0.0 and 1.0, where torch's BCELoss clamps
    the logs at -100 and its backward divides by max(x (1 - x), 1e-12)."""
    from oracle import p2i_oracle as orc
    real, fake = labels
    a0, b0, c0 = gc.gan_logits(n, lt, 3, 1.0), gc.gan_logits(n, lt, 4, -1.0), gc.gan_logits(n, lt, 5)
    inner = lambda t: (t > 0) & (t < 1) if lt == "nsgan" else torch.ones_like(t, dtype=torch.bool)

    def check_grad(got, x, what):
        print("gan", n, lt, labels, what, _err(got, x.grad))
        assert _err(got, x.grad) < 1e-5, what
        sel = inner(x.detach())
        if lt == "nsgan" and bool(sel.any()):                       # the 1e12 at x = 0 / 1 must not hide the other logits
            assert rel_err(got.cpu()[sel].numpy(), x.grad[sel].numpy()) < 1e-5, what

    a, b = a0.to(F64).requires_grad_(True), b0.to(F64).requires_grad_(True)
    ld = (orc.gan_loss(a, True, lt, True, real, fake) + orc.gan_loss(b, False, lt, True, real, fake)) * 0.5
    ld.backward()
    l, da, db = ops.gan_loss_d(a0.cuda(), b0.cuda(), lt, real, fake)
    print("gan", n, lt, labels, "loss_d", float(l), float(ld))
    assert abs(float(l) - float(ld)) < 1e-5 * abs(float(ld))
    check_grad(da, a, "d real")
    check_grad(db, b, "d fake")
    c = c0.to(F64).requires_grad_(True)
    lg = orc.gan_loss(c, True, lt, False, real, fake) * 0.01
    lg.backward()
    l2, dc = ops.gan_loss_g(c0.cuda(), 0.01, lt, real)
    assert abs(float(l2) - float(lg)) < 1e-5 * abs(float(lg)) + 1e-9
    check_grad(dc, c, "g")


def test_nsgan_refuses_a_logit_out_of_range(ops):
    x = gc.gan_logits(1025, "nsgan", 3)
    bad = x.clone()
    bad[700] = 1.5
    with pytest.raises(RuntimeError):
        ops.gan_loss_d(bad.cuda(), x.cuda(), "nsgan")
    with pytest.raises(RuntimeError):
        ops.gan_loss_d(x.cuda(), (-bad).cuda(), "nsgan")
    with pytest.raises(RuntimeError):
        ops.gan_loss_g(bad.cuda(), 0.01, "nsgan")


# ------------------------------------------------------------------------------------------------ the other users of the scratch
def test_idw_bwd_both_reductions(ops, reduce):
    from oracle import p2i_oracle as orc
    from p2igan_bench.utils import seeded
    T, H, W = 16, 32, 32
    mk = seeded.block_mask(H, W, 4, seed=9).reshape(1, 1, H, W).expand(2, T, H, W).contiguous()
    src = gc.rand(2, T, H, W, seed=3).abs().requires_grad_(True)
    outs = []
    for b in range(2):
        tz, ty, tx, pts = orc.mask_points(mk[b])
        outs.append(orc.idw_3d_knn(pts, src[b][tz, ty, tx], (T, H, W)))
    gout = gc.rand(2, T, H, W, seed=4)
    torch.stack(outs).backward(gout)
    _, saved = ops.idw_fwd(src.detach().cuda(), mk.cuda())
    dv = _run(reduce, lambda: ops.idw_bwd(gout.cuda(), saved))
    assert _err(dv, src.grad) < TOL_WGRAD


def test_weight_unpack_grad_both_reductions(ops, reduce):
    from oracle import p2i_oracle as orc
    shape = (64, 16, 3, 3)
    O, I, nt = 64, 16, 9
    w = gc.rand(*shape, seed=1, scale=0.1)
    u, v = F.normalize(gc.rand(O, seed=2), dim=0), F.normalize(gc.rand(I * nt, seed=3), dim=0)
    p = {"l.weight_orig": w.clone().requires_grad_(True), "l.weight_u": u.clone(), "l.weight_v": v.clone()}
    gw = gc.rand(*shape, seed=4)
    orc.spectral_norm_weight(p, "l", True).backward(gw)
    ug, vg, wg = u.cuda(), v.cuda(), w.cuda()
    sigma = ops.spectral_norm(wg, ug, vg, True)
    wflat = wg.reshape(O, I, nt)
    dwp = torch.zeros(nt, I, ops.pad32(O))
    dwp[:, :, :O] = gw.reshape(O, I, nt).permute(2, 1, 0)
    dwp = dwp.cuda()
    dw = _run(reduce, lambda: ops.weight_unpack_grad(dwp, wflat, wflat, sigma, ug, vg))
    assert _err(dw, p["l.weight_orig"].grad.reshape(O, I, nt)) < TOL_WGRAD
