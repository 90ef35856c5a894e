"""Edge-shape, second-trip, misaligned-pointer and non-finite sweep of the loss family's kernels (csrc/loss_ext.hip) through the
public functions of p2igan_bench.modules.losses, and through ops.* where an intermediate (idx, coef) or one misaligned pointer is
the thing under test.  Cases, float64 expectations and error scales come from tests/loss_ext_cases.py; tests/
test_loss_ext_cases_cpu.py shows from sizes alone that each case reaches the path it is there for.

Exact family (fdiff on integers, spatial_pool on distinct integers, 16-byte path against scalar path): torch.equal.
Tolerance family: per element e_i = |got_i - ref_i| / (2^-24 scale_i) against the float64 restatement on the same float32 inputs,
max e_i <= bound(op) = max(8, 4 x the float32 restatement's own max e_i).  Every case runs twice and the runs are bit-equal.

max e_i: float32 restatement on the CPU (loss_ext_cases.F32_E) / the kernels on an MI355X (this module's printout) / bound
  transform   fwd 2.6 / 2.63 / 10.4      bwd 2.2 / 2.42 / 8.8
  wl1         fwd 0.35 / 0.95 / 8        bwd 1.2 / 1.18 / 8
  kl          fwd 0.3 / 0.85 / 8         bwd 0.45 / 0.43 / 8
  softmax     fwd 2.3 / 2.68 / 9.2       bwd 1.25 / 1.05 / 8
  tdm         loss 0.2 / 0.43 / 8        coef 0.65 / 0.80 / 8       dpred 0.45 / 0.78 / 8
  shock map   fwd 1.15 / 1.10 / 8        bwd 0.65 / 0.59 / 8
  shock loss  fwd 1.3 / 1.25 / 8         bwd 1.15 / 1.09 / 8
The 16-byte and the scalar path gave the same bits in every operation compared.  Before the NaN rule of csrc/loss_ext.hip
(`v > m || v != v` in the pool scans, `d <= 0 ? 0 : d` in the shock loss) the four *_keeps_nan tests of the pool, the matching loss
and the shock loss failed; test_shock_map_keeps_nan passed.  The module's 82 tests run in 6 s on an MI355X (slowest: 1.3 s)."""
import pytest
import torch
import torch.nn.functional as F

import loss_ext_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from p2igan_bench import _hip
    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from p2igan_bench.modules import losses
    return losses


@pytest.fixture(scope="module")
def ops():
    from p2igan_bench import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _twice(fn):
    """fn() -> tuple of tensors, run twice; the two runs must agree bit for bit (NaN included)."""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v)), "two runs differ"
    return a


PEAK = {}          # operation -> the largest e seen by the tests run so far


def _hold(op, tag, got, ref, scale):
    e = C.err(got.cpu(), ref.cpu(), scale.cpu())
    PEAK[op] = max(PEAK.get(op, 0.0), e)
    print(f"{op} {tag}: max e = {e:.3f} (bound {C.bound(op):g})")
    assert tuple(got.shape) == tuple(ref.shape), (op, tag)
    assert e <= C.bound(op), (op, tag, e)
    return e


def _grad(fn, x, g):
    """(fn(x), d sum(fn(x) * g) / dx) with x a leaf on its own storage (misaligned views stay misaligned)."""
    x = x.detach().requires_grad_(True)
    out = fn(x)
    out.backward(g)
    return out.detach(), x.grad


# ---------------------------------------------------------------- exact family
def _fdiff(L, ops, dev, c):
    x, dy = C.fdiff_inputs(c)
    want_out, want_dx = C.fdiff_ref(x, dy)
    x, dy = x.to(dev), dy.to(dev)
    if c.shift:
        x, dy = C.misaligned(x), C.misaligned(dy)
    assert C.is_vec_path(c.inner, x, dy) == (c.inner % 4 == 0 and not c.shift)
    out, dx = _twice(lambda: (L.compute_forward_difference(x), ops.fdiff_bwd(dy, c.T)))
    assert torch.equal(out.cpu(), want_out) and torch.equal(dx.cpu(), want_dx), c
    _, dx2 = _grad(L.compute_forward_difference, x, dy)
    assert torch.equal(dx2.cpu(), want_dx), c


def test_fdiff_is_exact_on_integers(dev, L, ops):
    for c in C.fdiff_cases():
        _fdiff(L, ops, dev, c)


@pytest.mark.parametrize("c", C.fdiff_cases(second_trip=True), ids=lambda c: f"inner{c.inner}")
def test_fdiff_second_grid_stride_trip(dev, L, ops, c):
    _fdiff(L, ops, dev, c)


def _spool(L, ops, dev, shape):
    x, dy = C.spool_inputs(shape)
    want_out, want_idx, want_dx = C.spool_ref(x, dy)
    x, dy = x.to(dev), dy.to(dev)
    out, idx = _twice(lambda: ops.spool_fwd(x))
    assert torch.equal(out.cpu(), want_out) and torch.equal(idx.cpu(), want_idx), shape
    out2, dx = _twice(lambda: _grad(L.spatial_pool, x, dy))
    assert torch.equal(out2.cpu(), want_out) and torch.equal(dx.cpu(), want_dx), shape
    assert torch.equal(L.spatial_pool(x), out)                       # the path that saves no index


def test_spatial_pool_is_exact_on_distinct_integers(dev, L, ops):
    for c in C.spool_cases():
        _spool(L, ops, dev, c.shape)


def test_spatial_pool_backward_second_trip(dev, L, ops):
    _spool(L, ops, dev, C.SPOOL_SECOND_TRIP_BWD)


def test_spatial_pool_forward_second_trip(dev, L):
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randint(-2 ** 23, 2 ** 23, C.SPOOL_SECOND_TRIP_FWD, generator=g, device=dev).float()
    (out,) = _twice(lambda: (L.spatial_pool(x),))
    assert out.numel() > C.POOL_ONE_TRIP
    assert torch.equal(out.cpu(), F.max_pool2d(x.cpu(), 5, 4, 2))


def test_vector_and_scalar_paths_give_the_same_bits(dev, ops):
    """The Vec<4> and Vec<1> instantiations evaluate the same expression per element: the same values at a 16-byte-aligned
    address and 4 bytes further give bit-equal outputs, also when only dy or only the target is misaligned."""
    mis = C.misaligned
    for n in (4, 1024, 1028):
        x, dy = (t.to(dev) for t in C.transform_inputs(n))
        assert C.is_vec_path(n, x, dy) and not C.is_vec_path(n, mis(x)) and not C.is_vec_path(n, x, mis(dy))
        assert torch.equal(ops.loss_transform_fwd(x), ops.loss_transform_fwd(mis(x)))
        want = ops.loss_transform_bwd(x, dy)
        assert torch.equal(want, ops.loss_transform_bwd(mis(x), mis(dy))) and torch.equal(want, ops.loss_transform_bwd(x, mis(dy)))
        pred, true = (t.to(dev) for t in C.wl1_inputs(n))
        g = torch.tensor(C.WL1_GOUT, device=dev)
        want = ops.wl1_bwd(pred, true, g)
        assert torch.equal(want, ops.wl1_bwd(mis(pred), mis(true), g)) and torch.equal(want, ops.wl1_bwd(pred, mis(true), g))
        p, q = (t.to(dev) for t in C.kl_inputs(n))
        g = torch.tensor(C.KL_GOUT, device=dev)
        want = ops.kl_bwd(p, q, g)
        assert torch.equal(want, ops.kl_bwd(mis(p), mis(q), g)) and torch.equal(want, ops.kl_bwd(p, mis(q), g))
        c = C.FdiffCase(3, 3, n, False)
        x, dy = (t.to(dev) for t in C.fdiff_inputs(c))
        assert torch.equal(ops.fdiff_fwd(x), ops.fdiff_fwd(mis(x))) and torch.equal(ops.fdiff_bwd(dy, 3), ops.fdiff_bwd(mis(dy), 3))


# ---------------------------------------------------------------- tolerance family: element-wise kernels and their sums
def _elementwise(L, dev, n, shift):
    big = n > 100000
    rdev = dev if big else "cpu"                   # the float64 expectation of the large cases is evaluated on the device
    put = (lambda t: C.misaligned(t.to(dev))) if shift else (lambda t: t.to(dev))
    tag = f"n={n}{' misaligned' if shift else ''}"
    x, dy = C.transform_inputs(n)
    y, sy, dx, sdx = C.transform_ref(x.to(rdev), dy.to(rdev))
    xd, dyd = put(x), put(dy)
    assert C.is_vec_path(n, xd, dyd) == (n % 4 == 0 and not shift)
    out, grad = _twice(lambda: _grad(L.transform, xd, dyd))
    _hold("transform_fwd", tag, out, y, sy)
    _hold("transform_bwd", tag, grad, dx, sdx)

    pred, true = C.wl1_inputs(n)
    loss, sloss, dp, sdp = C.wl1_ref(pred.to(rdev), true.to(rdev))
    pd, td = put(pred), put(true)
    g = torch.tensor(C.WL1_GOUT, device=dev)
    out, grad = _twice(lambda: _grad(lambda t: L.weighted_l1_distance(t, td), pd, g))
    _hold("wl1_fwd", tag, out, loss, sloss)
    _hold("wl1_bwd", tag, grad, dp, sdp)
    same = (pred == true)
    assert bool((grad.cpu()[same] == 0).all()) and int(same.sum()) >= (2 if n >= 5 else 0)        # sign(0) = 0, exactly

    p, q = C.kl_inputs(n)
    loss, sloss, dp, sdp = C.kl_ref(p.to(rdev), q.to(rdev))
    pd, qd = put(p), put(q)
    g = torch.tensor(C.KL_GOUT, device=dev)
    out, grad = _twice(lambda: _grad(lambda t: L.kl_divergence(t, qd), pd, g))
    _hold("kl_fwd", tag, out, loss, sloss)
    _hold("kl_bwd", tag, grad, dp, sdp)
    assert bool((grad.cpu()[q == 0] == 0).all())


@pytest.mark.parametrize("n", C.elem_sizes())
def test_transform_wl1_kl(dev, L, n):
    _elementwise(L, dev, n, False)
    if n % 4 == 0 and n < 100000:
        _elementwise(L, dev, n, True)               # n % 4 == 0 on the scalar path; its sums against the same float64 bound


@pytest.mark.parametrize("shape", C.softmax_shapes(), ids=lambda s: f"{s[0] * s[1]}x{s[2]}")
def test_softmax_temperature(dev, L, shape):
    x, dy = C.softmax_inputs(shape)
    y, sy, dx, sdx = C.softmax_ref(x, dy)
    xd, dyd = x.to(dev), dy.to(dev)
    out, grad = _twice(lambda: _grad(lambda t: L.softmax_temperature(t, C.TEMP), xd, dyd))
    tag = f"rows={shape[0] * shape[1]} L={shape[2]}"
    _hold("softmax_fwd", tag, out, y, sy)
    _hold("softmax_bwd", tag, grad, dx, sdx)
    if shape[2] >= 63:
        assert bool((out == 0).any()), "arguments under -104 underflow to exactly 0"
    rows = out.cpu().double().reshape(shape[0] * shape[1], -1).sum(dim=1)
    slack = C.bound("softmax_fwd") * C.U * sy.reshape(shape[0] * shape[1], -1).sum(dim=1)
    assert bool(((rows - 1.0).abs() <= slack).all()), float((rows - 1.0).abs().max())


@pytest.mark.parametrize("c", C.tdm_cases(), ids=lambda c: "x".join(map(str, c.shape)) + f"-b{c.beta:g}")
def test_temporal_difference_matching(dev, L, ops, c):
    pd, td, tr = C.tdm_inputs(c.shape)
    big = pd.numel() > 100000
    ref = C.tdm_ref(*((t.to(dev) for t in (pd, td, tr)) if big else (pd, td, tr)), c.beta)
    pdd, tdd, trd = pd.to(dev), td.to(dev), tr.to(dev)
    loss, coef, idx = _twice(lambda: ops.tdm_fwd(pdd, tdd, trd, c.beta, C.TDM_EPS))
    tag = "x".join(map(str, c.shape))
    _hold("tdm_loss", tag, loss, ref["loss"], ref["sloss"])
    _hold("tdm_coef", tag, coef, ref["coef"], ref["scoef"])
    assert torch.equal(idx.cpu(), ref["idx"].cpu())
    g = torch.tensor(C.TDM_GOUT, device=dev)
    out, grad = _twice(lambda: _grad(lambda t: L.temporal_difference_matching_loss(t, tdd, trd, beta=c.beta, eps=C.TDM_EPS), pdd, g))
    assert torch.equal(out, loss)
    _hold("tdm_bwd", tag, grad, ref["dpred"], ref["sdpred"])
    assert bool((grad[ref["dpred"].to(dev) == 0] == 0).all())            # only argmax pixels get a gradient


# ---------------------------------------------------------------- shock map and shock loss
def test_shock_map(dev, L):
    for c in C.shock_map_cases():
        x, _, dout = C.shock_inputs(c)
        s, ss, dx, sdx = C.shock_map_ref(x, dout, c.beta)
        xd, dd = x.to(dev), dout.to(dev)
        out, grad = _twice(lambda: _grad(lambda t: L.shock_map(t, c.beta, C.SHOCK_EPS), xd, dd))
        _hold("shock_map_fwd", c.id, out, s, ss)
        _hold("shock_map_bwd", c.id, grad, dx, sdx)


def _shock_loss(L, dev, c, on_device=False):
    pred, true, dout = C.shock_inputs(c)
    ref = C.shock_loss_ref(*((t.to(dev) for t in (pred, true, dout)) if on_device else (pred, true, dout)), c.beta, c.pool, c.border)
    pd, td, dd = pred.to(dev), true.to(dev), ref["dout"].to(dev)
    fn = lambda t: L.shock_map_loss(t, td, beta=c.beta, border_ignore=c.border, pool=c.pool, eps=C.SHOCK_EPS)      # noqa: E731
    out, grad = _twice(lambda: _grad(fn, pd, dd))
    _hold("shock_loss_fwd", c.id, out, ref["out"], ref["sout"])
    _hold("shock_loss_bwd", c.id, grad, ref["dx"], ref["sdx"])
    assert torch.equal(fn(pd), out)                                    # the path without autograd
    g = grad.cpu()
    dropped, border_only = C.shock_zero_sets(c, pred.shape)
    assert bool((g[..., dropped] == 0).all()), "dropped trailing pixels"
    assert bool((g[..., border_only] == 0).all()), "pixels only the ignored border reads"
    assert bool((g[C.pool_non_argmax(pred, c.pool)] == 0).all()), "non-argmax pixels of a pool window"


@pytest.mark.parametrize("c", C.shock_loss_cases(), ids=lambda c: c.id)
def test_shock_loss(dev, L, c):
    _shock_loss(L, dev, c)


def test_shock_loss_second_trip_of_the_gather(dev, L):
    assert torch.empty(C.SHOCK_SECOND_TRIP, device="meta").numel() > C.POOL_ONE_TRIP
    _shock_loss(L, dev, C.ShockCase("second-trip", C.SHOCK_SECOND_TRIP[:2], 483, 483, 1, 30.0, 0, 0), on_device=True)


def test_shock_plane_limit(dev, L):
    x = torch.rand(C.SHOCK_OVER_LIMIT, device=dev)
    with pytest.raises(RuntimeError):
        L.shock_map_loss(x, x, pool=1)
    with pytest.raises(RuntimeError):
        L.shock_map(x)


# ---------------------------------------------------------------- non-finite inputs
def _nf_grad_rules(tag, grad, ref, reach):
    """Every NaN of the restatement is a NaN here; no NaN outside the reach of the poisoned pixels (a superset rule: the order of
    0 * NaN products is free inside it); returns the mask of elements finite on both sides."""
    got_nan, ref_nan = torch.isnan(grad), torch.isnan(ref)
    assert bool(got_nan[ref_nan].all()), f"{tag}: a NaN of the restatement's gradient is finite here"
    assert not bool(got_nan[0, 0].any()) and not bool((got_nan[0, 1] & ~reach).any()), f"{tag}: NaN outside the poisoned pixels' reach"
    return torch.isfinite(grad) & torch.isfinite(ref)


def _nf_scale(scale, ref):
    """Where a poisoned neighbour makes the scale itself non-finite but the expectation is finite: |ref|, the tightest choice."""
    return torch.where(torch.isfinite(scale), scale, ref.abs().double())


def _finite_err(op, tag, got, ref, scale, both):
    scale = _nf_scale(scale, ref)
    ref = torch.where(both, ref, torch.full_like(ref, float("nan")))          # C.err skips the elements where ref is not finite
    return _hold(op, tag, torch.where(both, got.double(), torch.zeros_like(ref)), ref, scale)


def test_spatial_pool_keeps_nan_and_gives_it_the_argmax(dev, L, ops):
    for name, poison in C.NF_CASES:
        x = C.nf_inputs(poison)
        want, widx = F.max_pool2d(x, 5, 4, 2, return_indices=True)
        dy = torch.arange(1.0, 1.0 + want.numel()).reshape(want.shape)
        out, idx = _twice(lambda: ops.spool_fwd(x.to(dev)))
        assert C.same_nonfinite(out, want), name
        assert torch.equal(torch.nan_to_num(out.cpu()), torch.nan_to_num(want)) and torch.equal(idx.cpu(), widx.int()), name
        assert C.same_nonfinite(L.spatial_pool(x.to(dev)), want), name
        x64 = x.double().requires_grad_(True)
        F.max_pool2d(x64, 5, 4, 2).backward(dy.double())
        _, grad = _twice(lambda: _grad(L.spatial_pool, x.to(dev), dy.to(dev)))
        assert torch.equal(grad.cpu().double(), x64.grad), name           # the last NaN of a window takes the window's gradient


def test_matching_loss_keeps_nan(dev, L, ops):
    td, tr = 0.3 * C.nf_inputs([]).flip(-1), C.nf_inputs([]).flip(-2).repeat(1, 2, 1, 1)[:, :3]
    for name, poison in C.NF_CASES:
        pd = C.nf_inputs(poison)
        ref = C.tdm_ref(pd, td, tr, 1.0)
        loss, coef, idx = _twice(lambda: ops.tdm_fwd(pd.to(dev), td.to(dev), tr.to(dev), 1.0, C.TDM_EPS))
        assert C.same_nonfinite(loss, ref["loss"]) and C.same_nonfinite(coef, ref["coef"]), name
        assert torch.equal(idx.cpu(), ref["idx"]), name
        _hold("tdm_loss", name, loss, ref["loss"], ref["sloss"])
        _hold("tdm_coef", name, coef, ref["coef"], ref["scoef"])
        g = torch.tensor(C.TDM_GOUT, device=dev)
        out, grad = _twice(lambda: _grad(lambda t: L.temporal_difference_matching_loss(t, td.to(dev), tr.to(dev), eps=C.TDM_EPS), pd.to(dev), g))
        assert C.same_nonfinite(out, ref["loss"]), name
        both = _nf_grad_rules(name, grad.cpu(), ref["dpred"], C.nf_reach(poison, 1, "pool"))
        _finite_err("tdm_bwd", name, grad.cpu(), ref["dpred"], ref["sdpred"], both)


def test_shock_map_keeps_nan(dev, L):
    for name, poison in C.NF_CASES:
        x = C.nf_inputs(poison)
        dout = torch.linspace(-1.0, 1.0, x.numel()).reshape(x.shape)
        s, ss, dx, sdx = C.shock_map_ref(x, dout, 1.0)
        out, grad = _twice(lambda: _grad(lambda t: L.shock_map(t, 1.0, C.SHOCK_EPS), x.to(dev), dout.to(dev)))
        assert C.same_nonfinite(out, s), name
        _hold("shock_map_fwd", name, out, s, _nf_scale(ss, s))
        both = _nf_grad_rules(name, grad.cpu(), dx, C.nf_reach(poison, 1, "shock"))
        _finite_err("shock_map_bwd", name, grad.cpu(), dx, sdx, both)


@pytest.mark.parametrize("pool", [1, 2])
def test_shock_loss_keeps_nan(dev, L, pool):
    true = C.nf_inputs([]).flip(-1)
    for name, poison in C.NF_CASES:
        pred = C.nf_inputs(poison)
        dout = torch.linspace(-1.0, 1.0, pred.numel() // pool ** 2).reshape(1, 2, C.NF_PLANE[0] // pool, C.NF_PLANE[1] // pool)
        ref = C.shock_loss_ref(pred, true, dout, 1.0, pool, 0)
        fn = lambda t: L.shock_map_loss(t, true.to(dev), beta=1.0, pool=pool, eps=C.SHOCK_EPS)          # noqa: E731
        out, grad = _twice(lambda: _grad(fn, pred.to(dev), ref["dout"].to(dev)))
        tag = f"{name} pool {pool}"
        assert C.same_nonfinite(out, ref["out"]), tag
        assert C.same_nonfinite(fn(pred.to(dev)), ref["out"]), tag
        _hold("shock_loss_fwd", tag, out, ref["out"], _nf_scale(ref["sout"], ref["out"]))
        both = _nf_grad_rules(tag, grad.cpu(), ref["dx"], C.nf_reach(poison, pool, "shock"))
        _finite_err("shock_loss_bwd", tag, grad.cpu(), ref["dx"], ref["sdx"], both)


def test_print_the_largest_error_per_operation(dev):
    """Last in the module: the figures of the docstring's table, from whichever tests ran before."""
    for op in sorted(PEAK):
        print(f"largest e, {op}: {PEAK[op]:.3f} (float32 restatement {C.F32_E[op]}, bound {C.bound(op):g})")
        assert PEAK[op] <= C.bound(op)
