"""Edge-shape sweep of the STDK kernels (csrc/stdk.hip) at the ops level -- P, Q, the bases, z, dP, dQ and dy are plain inputs of
any shape the ABI accepts -- over the cases of tests/stdk_cases.py; test_stdk_cases_cpu.py proves on the CPU which guarded path
every named case reaches.

Exact family (fused MLP forward / backward / weight gradients, layer 1 forward / backward): integer data, every sum below 2^24 in
any order, torch.equal against the float64 CPU result; every case runs twice and the second run must give the same bits.  The MLP
cases cover partial and wholly invalid wave tiles, a single pixel, row counts that are no multiple of 4, single / partial / > 256
row weight-gradient chunks, and ragged last frame splits in both directions; the layer-1 cases cover ragged and empty k-splits of
the three weight-gradient products (checked per split in sentinel-filled buffers) and M, N ragged against the thread tile.
Selection: bit-exact against tests/stdk_ref.visible, H*W from 79 to 1000, 0 .. all observed, the 79th hit on 256-pixel pass
boundaries, mask values 1 / 0.5 / -1 / 0.0 / -0.0, k = 1, 79 and H*W.  Bases: the Wendland formula in float64, 1e-6 absolute.
Model level: STDKGenerator forward and all eight parameter gradients on maps of 79 .. 1139 pixels and T in {1, 2, 3, 5, 7} against
tests/stdk_ref.py in float64 on the CPU, with the tolerances of test_stdk_gpu.py.

73 tests (13 MLP cases + 2 pre-filled, 8 layer-1 cases + 3 carved, 29 selection, 11 basis and 6 model cases, 1 of refusals): 3.9 s
on an MI355X, the float64 CPU references included; the slowest is hw877-bt300 with 0.35 s.  The sweep found no difference: every
exact case ended in torch.equal at the first run and no kernel was changed.  (Bases: at most 2.6e-7 off; model level: predictions
at most 1.2e-6 and gradients at most 5.1e-7 of max-abs.)"""
import ctypes

import numpy as np
import pytest
import torch

import stdk_cases as sc
from conftest import rel_err
from test_stdk_gpu import GTOL, PARAMS, TOL, _cfg

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5       # no integer: an exact result cannot equal it
GAP = 64                  # floats between two buffers carved from one sentinel-filled tensor (keeps them 16-byte aligned)
_REF = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from p2igan_bench import ops as o
    o._hip.load()
    return o


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same(got, exp64, cid, what):
    """torch.equal against the float64 expectation (exact in float32: asserted here); reports the differing elements."""
    exp = exp64.float()
    assert torch.equal(exp.double(), exp64), f"{cid}: the expectation of {what} is not exact in float32"
    got = got.detach().cpu().reshape(exp.shape)
    if torch.equal(got, exp):
        return
    bad = (got != exp) | torch.isnan(got)
    idx = bad.nonzero()
    first = ["%s: got %g, expected %g" % (tuple(i.tolist()), float(got[tuple(i)]), float(exp[tuple(i)])) for i in idx[:6]]
    raise AssertionError(f"{cid} {what}: {int(bad.sum())} of {exp.numel()} elements differ (shape {tuple(exp.shape)}); "
                         + "; ".join(first))


def _carve(sizes, dev):
    """Buffers of the given sizes inside one SENTINEL-filled tensor, GAP floats before, between and after them."""
    offs, n = [], GAP
    for s in sizes:
        offs.append(n)
        n += (s + 3) // 4 * 4 + GAP
    whole = torch.full((n,), SENTINEL, device=dev)
    return whole, [whole[o:o + s] for o, s in zip(offs, sizes)]


def _gaps_untouched(whole, sizes):
    keep = torch.ones(whole.numel(), dtype=torch.bool)
    n = GAP
    for s in sizes:
        keep[n:n + s] = False
        n += (s + 3) // 4 * 4 + GAP
    w = whole.cpu()
    return bool((w[keep] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ exact family: fused MLP
MLP_OUT = ("y", "dP", "dQ", "dw2", "db2", "dw3", "db3", "dw4", "db4")


def _mlp_ref(c):
    if c.id not in _REF:
        t = sc.mlp_inputs(c)
        r, bound = sc.mlp_reference(t)
        assert max(bound.values()) < sc.EXACT_LIMIT
        _REF[c.id] = (t, r)
    return _REF[c.id]


def _mlp_run(ops, g):
    y = ops.stdk_mlp_fwd(g["P"], g["Q"], g["w2"], g["b2"], g["w3"], g["b3"], g["w4"], g["b4"])
    dP, dQ, grads = ops.stdk_mlp_bwd(g["P"], g["Q"], g["w2"], g["b2"], g["w3"], g["b3"], g["w4"], g["dy"])
    torch.cuda.synchronize()
    return dict(zip(MLP_OUT, [y, dP, dQ] + list(grads)))


@pytest.mark.parametrize("case", sc.mlp_cases(), ids=[c.id for c in sc.mlp_cases()])
def test_mlp_exact(ops, case):
    t, r = _mlp_ref(case)
    g = {k: v.cuda() for k, v in t.items()}
    first = _mlp_run(ops, g)
    for k in MLP_OUT:
        _same(first[k], r[k], case.id, k)
    second = _mlp_run(ops, g)
    for k in MLP_OUT:
        assert torch.equal(first[k], second[k]), f"{case.id} {k}: the second run gave other bits"


@pytest.mark.parametrize("cid", ["hw79-bt1", "hw65-bt5"])
def test_mlp_overwrites_every_output_element(ops, cid):
    """y, dP, dQ (natural sizes: there are no rows beyond H*W), the weight gradients and the workspace pre-filled with a sentinel:
    every output element is overwritten with the expected value, also where a wave tile is partial or wholly invalid."""
    case = {c.id: c for c in sc.mlp_cases()}[cid]
    t, r = _mlp_ref(case)
    g = {k: v.cuda() for k, v in t.items()}
    lib, dev, HW, BT = ops._hip.load(), g["P"].device, case.HW, case.BT
    y = torch.full((BT, HW), SENTINEL, device=dev)
    ops._hip.check(lib.p2i_stdk_mlp_fwd(*[g[k].data_ptr() for k in ("P", "Q", "w2", "b2", "w3", "b3", "w4", "b4")], HW, BT, y.data_ptr(),
                                        _stream()), "p2i_stdk_mlp_fwd")
    sz = (ctypes.c_int64 * 4)()
    ops._hip.check(lib.p2i_stdk_bwd_workspace(HW, BT, sz), "p2i_stdk_bwd_workspace")
    gx, _, _, gy = sc.bwd_plan(HW, BT)
    chunks = sc.wgrad_plan(HW * BT)[1]
    assert list(sz) == [5 * HW * BT * sc.HP, gy * HW * sc.HID, gx * 4 * BT * sc.HID, chunks * (2 * (sc.HID * sc.HID + sc.HID) + sc.HID + 1)]
    ws = [torch.full((int(n),), SENTINEL, device=dev) for n in sz]
    out = {k: torch.full(tuple(r[k].shape), SENTINEL, device=dev) for k in MLP_OUT[1:]}
    ops._hip.check(lib.p2i_stdk_mlp_bwd(*[g[k].data_ptr() for k in ("P", "Q", "w2", "b2", "w3", "b3", "w4", "dy")], HW, BT,
                                        *[w.data_ptr() for w in ws], *[out[k].data_ptr() for k in MLP_OUT[1:]], _stream()),
                   "p2i_stdk_mlp_bwd")
    torch.cuda.synchronize()
    _same(y, r["y"], cid, "y (pre-filled)")
    for k in MLP_OUT[1:]:
        _same(out[k], r[k], cid, k + " (pre-filled)")
    for name, w in zip(("row planes", "dP partials", "dQ partials", "weight-gradient partials"), ws):
        assert not bool((w == SENTINEL).any()), f"{cid}: the {name} keep elements that no workgroup wrote"


# ------------------------------------------------------------------------------------------------ exact family: layer 1
def _l1_ref(c):
    if c.id not in _REF:
        t = sc.l1_inputs(c)
        r, bound = sc.l1_reference(c, t)
        assert max(bound.values()) < sc.EXACT_LIMIT
        _REF[c.id] = (t, r)
    return _REF[c.id]


@pytest.mark.parametrize("case", sc.l1_cases(), ids=[c.id for c in sc.l1_cases()])
def test_layer1_exact(ops, case):
    c = case
    t, r = _l1_ref(c)
    g = {k: v.cuda() for k, v in t.items()}
    runs = []
    for _ in range(2):
        P, Q = ops.stdk_layer1_fwd(g["phi_s"], g["phi_t"], g["z"], g["w1"], g["b1"], c.B, c.T)
        dw1, db1 = ops.stdk_layer1_bwd(g["phi_s"], g["phi_t"], g["z"], g["dP"], g["dQ"], c.B, c.T)
        torch.cuda.synchronize()
        runs.append(dict(P=P, Q=Q, dw1=dw1, db1=db1))
    for k in ("P", "Q", "dw1", "db1"):                   # P, Q: all 112 columns, the pads exactly 0
        _same(runs[0][k], r[k], c.id, k)
        assert torch.equal(runs[0][k], runs[1][k]), f"{c.id} {k}: the second run gave other bits"
    assert not bool(runs[0]["P"][:, sc.HID:].any()) and not bool(runs[0]["Q"][:, sc.HID:].any())


@pytest.mark.parametrize("cid", sc.L1_SENTINEL)
def test_layer1_writes_inside_its_buffers(ops, cid):
    """The ABI called with every output and scratch buffer carved from one sentinel-filled tensor: P, Q, dw1, db1 are exact, the
    [splits][100][F] partials are all written, add up to dw1, are exactly 0 in the blocks of an empty k-split, and nothing between
    or beyond the buffers is touched."""
    c = {x.id: x for x in sc.l1_cases()}[cid]
    t, r = _l1_ref(c)
    g = {k: v.cuda() for k, v in t.items()}
    lib, dev, F = ops._hip.load(), g["w1"].device, c.Ks + c.Kt + c.Kz
    BT, HP, HID = c.B * c.T, sc.HP, sc.HID
    sizes = [c.HW * HP, c.T * HP, c.B * HP, BT * HP]
    whole, (P, zt, zb, Q) = _carve(sizes, dev)
    ops._hip.check(lib.p2i_stdk_layer1_fwd(*[g[k].data_ptr() for k in ("phi_s", "phi_t", "z", "w1", "b1")], c.B, c.T, c.HW, c.Ks, c.Kt,
                                           c.Kz, P.data_ptr(), zt.data_ptr(), zb.data_ptr(), Q.data_ptr(), _stream()),
                   "p2i_stdk_layer1_fwd")
    torch.cuda.synchronize()
    _same(P, r["P"], cid, "P (carved)")
    _same(Q, r["Q"], cid, "Q (carved)")
    assert not bool((zt == SENTINEL).any()) and not bool((zb == SENTINEL).any())
    assert _gaps_untouched(whole, sizes), f"{cid}: layer-1 forward wrote outside its buffers"

    splits = sc.l1_splits(c.HW)
    sizes = [c.T * HID, c.B * HID, splits * HID * F, HID * F, HID]
    whole, (dqt, dqb, part, dw1, db1) = _carve(sizes, dev)
    ops._hip.check(lib.p2i_stdk_layer1_bwd(*[g[k].data_ptr() for k in ("phi_s", "phi_t", "z", "dP", "dQ")], c.B, c.T, c.HW, c.Ks, c.Kt,
                                           c.Kz, dqt.data_ptr(), dqb.data_ptr(), part.data_ptr(), splits, dw1.data_ptr(), db1.data_ptr(),
                                           _stream()), "p2i_stdk_layer1_bwd")
    torch.cuda.synchronize()
    _same(dw1, r["dw1"], cid, "dw1 (carved)")
    _same(db1, r["db1"], cid, "db1 (carved)")
    dq = t["dQ"].double().reshape(c.B, c.T, HID)
    _same(dqt, dq.sum(0), cid, "dQ summed over the samples")
    _same(dqb, dq.sum(1), cid, "dQ summed over the frames")
    p = part.cpu().reshape(splits, HID, F)
    assert not bool((p == SENTINEL).any()), f"{cid}: partials that no thread wrote"
    _same(p.double().sum(0), r["dw1"], cid, "partials summed over the k-splits")
    for (lo, hi), K in (((0, c.Ks), c.HW), ((c.Ks, c.Ks + c.Kt), c.T), ((c.Ks + c.Kt, F), c.B)):
        for s, rows in enumerate(sc.gemm_chunks(K, splits)):
            if rows == 0:
                assert not bool(p[s, :, lo:hi].any()), f"{cid}: the empty k-split {s} of the K = {K} product is not zero"
    assert _gaps_untouched(whole, sizes), f"{cid}: layer-1 backward wrote outside its buffers"


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("case", sc.sel_cases(), ids=[c.id for c in sc.sel_cases()])
def test_select_exact(ops, case):
    x, m = sc.sel_inputs(case)
    want_idx, want_z = sc.sel_reference(case, x, m)
    idx, z = ops.stdk_select(x.cuda(), m.cuda(), case.k)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and idx.shape == want_idx.shape and z.shape == want_z.shape
    idx, z = idx.cpu(), z.cpu()
    if not torch.equal(idx, want_idx):
        bad = (idx != want_idx).nonzero()
        first = ["%s: got %d, expected %d" % (tuple(i.tolist()), int(idx[tuple(i)]), int(want_idx[tuple(i)])) for i in bad[:6]]
        raise AssertionError(f"{case.id} idx: {len(bad)} of {idx.numel()} differ; " + "; ".join(first))
    assert torch.equal(z.view(torch.int32), want_z.view(torch.int32)), f"{case.id}: z is not the gathered bits"


# ------------------------------------------------------------------------------------------------ bases
@pytest.mark.parametrize("case", sc.basis_cases(), ids=[c.id for c in sc.basis_cases()])
def test_basis_matches_the_formula(ops, case):
    want = sc.wendland(case, np.float64)
    phi = ops.stdk_basis(case.knots.cuda(), case.theta.cuda(), case.H, case.W)
    torch.cuda.synchronize()
    assert phi.shape == want.shape and phi.dtype == torch.float32
    got = phi.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{case.id}: max abs err {err:.3g} (bound {sc.BASIS_TOL:g})")
    assert err <= sc.BASIS_TOL, f"{case.id}: {int((np.abs(got - want) > sc.BASIS_TOL).sum())} of {want.size} elements off, max {err:.3g}"
    if case.id == "79x1-k4-hand":
        assert got[15, 0] == 0 and got[5, 0] == 0 and got[10, 0] == 1          # d = 1 exactly is the edge of the support, d = 0


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("case", sc.model_cases(), ids=[c.id for c in sc.model_cases()])
def test_model_matches_float64_restatement(ops, case):
    from p2igan_bench.models import build_generator
    inputs = sc.model_inputs(case)
    sd, masked, masks, dy = inputs
    yr, grads = sc.model_reference(case, inputs)
    dev = torch.device("cuda:0")
    G = build_generator(_cfg(case.H, case.W, case.T)).to(dev)
    G.load_state_dict(sd, strict=True)
    y = G(masked.to(dev), masks.to(dev))
    (y * dy.to(dev)).sum().backward()
    params = dict(G.named_parameters())
    errs = {n: rel_err(params[n].grad.cpu().numpy(), g.numpy()) for n, g in zip(PARAMS, grads)}
    ey = rel_err(y.detach().cpu().numpy(), yr.numpy())
    print(f"{case.id}: preds {ey:.2e}, gradients " + ", ".join(f"{n[9:]} {e:.2e}" for n, e in errs.items()))
    assert ey < TOL
    for n, e in errs.items():
        assert e < GTOL, (case.id, n, e)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_any_launch(ops):
    """Only calls that the argument checks reject: nothing here reaches a kernel."""
    dev = torch.device("cuda:0")
    x = torch.zeros(1, 2, 78, device=dev)
    with pytest.raises(ValueError):
        ops.stdk_select(x, x.clone())
    with pytest.raises(ValueError):
        ops.stdk_select(torch.zeros(1, 1, 100, device=dev), torch.zeros(1, 1, 100, device=dev), 101)
    with pytest.raises(RuntimeError):
        ops.stdk_select(torch.zeros(1, 2, 100, device=dev), torch.zeros(1, 1, 100, device=dev))
    lib = ops._hip.load()
    idx = torch.zeros(2, 79, dtype=torch.int32, device=dev)
    z = torch.zeros(2, 79, device=dev)
    rc = lib.p2i_stdk_select(x.data_ptr(), x.data_ptr(), 2, 78, 79, idx.data_ptr(), z.data_ptr(), _stream())
    assert rc != 0 and b"stdk_select needs H*W >= k" in lib.p2i_last_error()
    assert lib.p2i_stdk_select(x.data_ptr(), x.data_ptr(), 2, 78, 0, idx.data_ptr(), z.data_ptr(), _stream()) != 0
    assert lib.p2i_last_error()
    c = sc.mlp_cases()[0]
    g = {k: v.to(dev) for k, v in sc.mlp_inputs(c).items()}
    args = [g[k] for k in ("P", "Q", "w2", "b2", "w3", "b3", "w4")]
    for bad in (g["dy"].t().contiguous() if c.BT != c.HW else g["dy"][:, :-1], torch.zeros(c.BT + 1, c.HW, device=dev),
                torch.zeros(c.BT, c.HW + 1, device=dev)):
        with pytest.raises(RuntimeError):
            ops.stdk_mlp_bwd(*args, bad)
    with pytest.raises(RuntimeError):
        ops.stdk_mlp_fwd(g["P"][:, :sc.HID].contiguous(), *args[1:], g["b4"])
    l1 = sc.l1_cases()[1]
    t = {k: v.to(dev) for k, v in sc.l1_inputs(l1).items()}
    with pytest.raises(RuntimeError):
        ops.stdk_layer1_bwd(t["phi_s"], t["phi_t"], t["z"], t["dP"][:-1], t["dQ"], l1.B, l1.T)
    with pytest.raises(RuntimeError):
        ops.stdk_layer1_fwd(t["phi_s"], t["phi_t"], t["z"], t["w1"][:, :-1].contiguous(), t["b1"], l1.B, l1.T)
    with pytest.raises(RuntimeError):
        ops.stdk_basis(torch.zeros(3, 3, device=dev), torch.ones(3, device=dev), 4, 4)
    torch.cuda.synchronize()
