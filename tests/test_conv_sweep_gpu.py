"""Exact-integer shape sweep of the conv engines (forward / data gradient / weight gradient) over the descriptor space the ABI
accepts, not only the model's layers: kernels 1x1 .. 3x3x3 incl. 1x2, 2x1, 2x2, 1x3, 3x1, 2x3, 3x1x1, 1x3x3, 2x2x2, 3x3x1;
strides 1, 2, 3 and mixed (8 merged parity classes, more than 8: one launch per class); padding 0, k//2, k-1, k; extents 1 .. 40
incl. outputs of extent 1 on every axis; channel counts 1 .. 65; batch 1 .. 5 (tests/conv_sweep_cases.py).

Exact family: x, w, bias, residual, dy, add, mask are small INTEGERS stored as float32, so every product and partial sum is an
integer below 2^24 and the result does not depend on summation order, split-K, atomics or the engine (on the bf16-split pipe an
integer <= 255 sits entirely in the high plane of the 3-way split).  The expectation is the float64 CPU result, cast to float32
without rounding, and the comparison is torch.equal: a wrong tap, a missed border, a zeroed batch slot or a shifted parity class is
an integer difference no tolerance can hide.  Every case ends in torch.equal; the only accepted alternative is a refusal (return
code + p2i_last_error message) that conv_sweep_cases.expected_refusal derives from a limit the source states.

Tolerance family: the same geometry, one case per (kernel, stride) combination, randn data and the two non-integral activations
(leaky, tanh) against float64 with the suite's TOL_OP / TOL_WGRAD.

The last test of the module asserts that the sweep reached every kernel family the planners can select.

What the sweep found when it was added (MI355X, 762 tests, 7.5 s), fixed in the same change:
  * forward / data gradient: 116 comparisons of 69 cases wrong wherever a patch axis had extent 1 (one tap, one output row or
    column per tile): the planners handed the kernels an index divisor of 1, for which no 32-bit multiplier exists (mg_1x1_h1
    conv_fwd: 629 of 1280 elements, every batch slot of a tile but the first bias-only);
  * conv_wgrad, plain kernel: wrong sums in 29 exact cases whenever the output is one column wide (a one-column tile paired every
    position with its neighbour in the next row; mg_1x1_w1: 505 of 512 elements, about twice the expectation; mg_3x1x1_h1w1:
    NaN), and `wgrad tile does not fit LDS` for eleven small stride-3 / stride-(2,3) shapes (o1_all, c1_3x3_s3, s133_3x3x3, ...)
    whose 64-position tile spans a patch above 160 KB; tiles are now at least two columns wide and shrink to 32 / 16 positions."""
import ctypes

import pytest
import torch

import conv_sweep_cases as cs
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_OP = 2e-5       # as tests/test_ops_gpu.py: single fp32 kernel, summation-order noise only
TOL_WGRAD = 1e-4    # long atomically-combined reductions

CONV_PLANS = {}     # plan tuple -> (case id, engine, call) that reached it first
WGRAD_PLANS = {}
REFUSED = []        # (case id, engine, call, message)
_REF = {}           # case id -> (inputs, float64 reference): shared by the engines


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from p2igan_bench import ops as o
    o._hip.load()
    return o


@pytest.fixture(params=["f32", "x6c"])
def engine(request, ops, monkeypatch):
    """As tests/test_ops_gpu.py's fixture: the f32-MFMA kernels only, or the library's choice with the bf16-split kernels' tile-count
    threshold lowered to one workgroup (P2I_X6C_MIN_WG, read per call) so that the small layers they cover run on them."""
    old = ops.CONV_ENGINE
    ops.CONV_ENGINE = "f32" if request.param == "f32" else "auto"
    if request.param != "f32":
        monkeypatch.setenv("P2I_X6C_MIN_WG", "1")
    yield request.param
    ops.CONV_ENGINE = old


def _plan(ops, wgrad=False):
    p = (ctypes.c_int * (4 if wgrad else 6))()
    (ops._hip.load().p2i_wgrad_last_plan if wgrad else ops._hip.load().p2i_conv_last_plan)(p)
    return tuple(p)


def _spec(ops, c):
    return ops.ConvSpec(c.Cin, c.Cout, c.k, c.s, c.p)


class _Runner:
    """Runs one call of a case; a RuntimeError is accepted only as the refusal expected_refusal predicts."""

    def __init__(self, ops, c, eng):
        self.ops, self.c, self.eng = ops, c, eng

    def __call__(self, op, what, fn, with_y_act=False):
        want = cs.expected_refusal(self.c, op, with_y_act)
        try:
            out = fn()
        except RuntimeError as e:
            assert want is not None and want in str(e), f"{self.c.id} [{self.eng}] {what}: unexpected refusal: {e}"
            REFUSED.append((self.c.id, self.eng, what, str(e)))
            return None
        plans, p = (WGRAD_PLANS, _plan(self.ops, True)) if op == "wgrad" else (CONV_PLANS, _plan(self.ops))
        plans.setdefault(p, (self.c.id, self.eng, what))
        return out


def _same(got, exp64, c, eng, what):
    """torch.equal against the float64 expectation (exact in float32: asserted by the caller); reports the differing elements."""
    exp = exp64.float()
    assert torch.equal(exp.double(), exp64), f"{c.id}: the expectation of {what} is not exact in float32"
    got = got.detach().cpu().reshape(exp.shape)
    if torch.equal(got, exp):
        return
    bad = (got != exp) | torch.isnan(got)
    idx = bad.nonzero()
    first = ["%s: got %g, expected %g" % (tuple(i.tolist()), float(got[tuple(i)]), float(exp[tuple(i)])) for i in idx[:6]]
    raise AssertionError(f"{c.id} [{eng}] {what}: {int(bad.sum())} of {exp.numel()} elements differ (shape {tuple(exp.shape)}); "
                         + "; ".join(first))


def _packed(dw64):
    """(Cout, Cin, *k) weight gradient -> the valid part of the packed layout [tap][Cin][Cout]."""
    return dw64.reshape(dw64.shape[0], dw64.shape[1], -1).permute(2, 1, 0).contiguous()


def _ref_of(c, exact):
    if c.id not in _REF:
        t = cs.exact_inputs(c) if exact else cs.randn_inputs(c)
        _REF[c.id] = (t, cs.reference(c, t, "relu" if exact else c.act))
    return _REF[c.id]


def _act_code(ops, act):
    return {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY, "tanh": ops.ACT_TANH}[act]


@pytest.mark.parametrize("case", cs.exact_cases(), ids=[c.id for c in cs.exact_cases()])
def test_conv_sweep_exact(ops, engine, case):
    c = case
    # conditions of the exact family, from the reference side alone
    assert c.act in ("none", "relu"), "only multipliers that keep integers integral"
    assert cs.desc_ok(c) and max(cs.in_elems(c), cs.out_elems(c)) <= cs.MAX_ELEMS
    assert max(cs.exact_bounds(c).values()) < cs.EXACT_LIMIT
    t, r = _ref_of(c, True)
    bounds = cs.exact_bounds(c)
    for key, lim in (("out", "fwd"), ("dx", "dgrad"), ("dx_p", "dgrad"), ("dx_e", "dgrad"), ("dw", "wgrad"), ("dw_p", "wgrad"),
                     ("db", "bgrad"), ("db_p", "bgrad")):
        assert float(r[key].abs().max()) <= bounds[lim] < cs.EXACT_LIMIT, (c.id, key)

    dev = "cuda"
    g = {k: (v.to(dev) if v is not None else None) for k, v in t.items()}
    spec, run = _spec(ops, c), _Runner(ops, c, engine)
    xs = tuple(t["x"].shape)
    wp_f, wp_d = ops.weight_pack(g["w"])
    _same(wp_f[:, :, :c.Cout], _packed(t["w"].double()).permute(0, 1, 2), c, engine, "weight_pack (forward layout)")
    _same(wp_d[:, :, :c.Cin], _packed(t["w"].double()).permute(0, 2, 1), c, engine, "weight_pack (data-gradient layout)")

    y = run("fwd", "conv_fwd", lambda: ops.conv_fwd(spec, g["x"], wp_f, g["bias"], g["res"], _act_code(ops, c.act)))
    if y is not None:
        _same(y, r["out"], c, engine, "conv_fwd")

    y_act = r["y_act"].float().to(dev).contiguous()
    dx = run("dgrad", "conv_dgrad", lambda: ops.conv_dgrad(spec, g["dy"], wp_d, xs))
    if dx is not None:
        _same(dx, r["dx"], c, engine, "conv_dgrad")
    dx = run("dgrad", "conv_dgrad (relu'(y) prologue)", lambda: ops.conv_dgrad(spec, g["dy"], wp_d, xs, y_act, ops.ACT_RELU), True)
    if dx is not None:
        _same(dx, r["dx_p"], c, engine, "conv_dgrad (relu'(y) prologue)")
    dx = run("dgrad", "conv_dgrad (add + relu' mask epilogue)",
             lambda: ops.conv_dgrad(spec, g["dy"], wp_d, xs, add=g["add"], mask_y=g["mask"], mask_act=ops.ACT_RELU))
    if dx is not None:
        _same(dx, r["dx_e"], c, engine, "conv_dgrad (add + relu' mask epilogue)")

    old_slices = ops.WGRAD_SLICES
    unpacked = False
    try:
        for slices in (True, False):
            ops.WGRAD_SLICES = slices
            for pro in (False, True):
                for want_bias in (False, True):
                    what = "conv_wgrad (slices %d, relu'(y) prologue %d, bias %d)" % (slices, pro, want_bias)
                    res = run("wgrad", what, lambda: ops.conv_wgrad(spec, g["x"], g["dy"], y_act if pro else None,
                                                                     ops.ACT_RELU if pro else ops.ACT_NONE, want_bias=want_bias), pro)
                    if res is None:
                        continue
                    dwp, db = res
                    _same(dwp[:, :, :c.Cout], _packed(r["dw_p" if pro else "dw"]), c, engine, what)
                    if want_bias:
                        _same(db, r["db_p" if pro else "db"], c, engine, what + ": bias gradient")
                    else:
                        assert db is None
                    if not unpacked:
                        _same(ops.weight_unpack_grad(dwp, g["w"]), r["dw_p" if pro else "dw"], c, engine, "weight_unpack_grad")
                        unpacked = True
    finally:
        ops.WGRAD_SLICES = old_slices


@pytest.mark.parametrize("case", cs.tolerance_cases(), ids=[c.id for c in cs.tolerance_cases()])
def test_conv_sweep_tolerance(ops, engine, case):
    c = case
    assert c.act in ("leaky", "tanh") and cs.desc_ok(c) and min(cs.in_elems(c), cs.out_elems(c)) >= cs.TOL_MIN_ELEMS
    t, r = _ref_of(c, False)
    dev = "cuda"
    g = {k: (v.to(dev) if v is not None else None) for k, v in t.items()}
    spec, run, act = _spec(ops, c), _Runner(ops, c, engine), _act_code(ops, c.act)
    xs = tuple(t["x"].shape)

    def close(got, exp64, tol, what):
        err = rel_err(got.detach().cpu().numpy().reshape(exp64.shape), exp64.numpy())
        print(f"{c.id} [{engine}] {what}: rel err {err:.3e} (tolerance {tol:g})")
        assert err < tol, f"{c.id} [{engine}] {what}: rel err {err:.3e} >= {tol:g}"

    wp_f, wp_d = ops.weight_pack(g["w"])
    close(run("fwd", "conv_fwd", lambda: ops.conv_fwd(spec, g["x"], wp_f, g["bias"], g["res"], act)), r["out"], TOL_OP, "conv_fwd")
    y_act = r["y_act"].float().to(dev).contiguous()
    close(run("dgrad", "conv_dgrad", lambda: ops.conv_dgrad(spec, g["dy"], wp_d, xs)), r["dx"], TOL_OP, "conv_dgrad")
    close(run("dgrad", "conv_dgrad (act'(y) prologue)", lambda: ops.conv_dgrad(spec, g["dy"], wp_d, xs, y_act, act), True),
          r["dx_p"], TOL_OP, "conv_dgrad (act'(y) prologue)")
    close(run("dgrad", "conv_dgrad (add + act' mask epilogue)",
              lambda: ops.conv_dgrad(spec, g["dy"], wp_d, xs, add=g["add"], mask_y=g["mask"], mask_act=act)),
          r["dx_e"], TOL_OP, "conv_dgrad (add + act' mask epilogue)")
    for pro in (False, True):
        what = "conv_wgrad (act'(y) prologue %d)" % pro
        dwp, db = run("wgrad", what, lambda: ops.conv_wgrad(spec, g["x"], g["dy"], y_act if pro else None,
                                                            act if pro else ops.ACT_NONE, want_bias=True), pro)
        close(ops.weight_unpack_grad(dwp, g["w"]), r["dw_p" if pro else "dw"], TOL_WGRAD, what)
        close(db, r["db_p" if pro else "db"], TOL_WGRAD, what + ": bias gradient")


def test_conv_sweep_refusals_are_the_expected_ones():
    """Every refusal the sweep met was predicted by expected_refusal (asserted where it happened); here: the predicted set is met
    in full, i.e. no case of the list escaped its comparison by an error that the rules did not ask for, and the list is short."""
    assert CONV_PLANS, "run the whole module: this test reads what the sweep recorded"
    want = {(c.id, pro) for c in cs.exact_cases() for pro in (False, True) if cs.expected_refusal(c, "wgrad", pro)}
    got = {(cid, "prologue 1" in what) for cid, _, what, _ in REFUSED}
    assert got == want, (sorted(got), sorted(want))
    assert len({cid for cid, _ in want}) <= 2


def test_conv_sweep_reached_every_kernel_family():
    """Dispatch coverage from p2i_conv_last_plan / p2i_wgrad_last_plan (include/p2i_hip.h), recorded after every call above.  The
    single-input-channel data gradient reports its own plan (KG = 4), so nothing here reads a stale plan."""
    assert CONV_PLANS and WGRAD_PLANS, "run the whole module: this test reads what the sweep recorded"
    kinds = {
        "patch_gemm_kernel (act'(y) prologue)": lambda p: p[5] == 0 and p[4] == -1,
        "patch_gemm_dma_kernel, KG = 1": lambda p: p[5] == 1 and p[1] in (128, 256),
        "patch_gemm_dma_kernel, KG = 2": lambda p: p[5] == 2,
        "o1_fwd_kernel": lambda p: p == (1, 64, 8, 1, 9, 3),
        "c1_dgrad_kernel": lambda p: p[5] == 4,
        "patch_gemm_x6c / x6p kernel (split pipe)": lambda p: p[5] == 7,
        "split pipe, fused strided data gradient": lambda p: p[5] == 8,
        "patch_gemm_fused_kernel, four classes": lambda p: p[5] == 14,
        "c1_fwd_kernel": lambda p: p == (32, 64, 1, 2, 27, 1),
    }
    missing = [name for name, f in kinds.items() if not any(f(p) for p in CONV_PLANS)]
    wmissing = [k for k in (0, 1, 2, 3) if not any(p[0] == k for p in WGRAD_PLANS)]
    tiles = sorted({p[:4] + (p[5],) for p in CONV_PLANS if p[5] in (1, 2) and p[1] in (128, 256)})
    pro_tiles = sorted({p[:4] for p in CONV_PLANS if p[5] == 0 and p[4] == -1})
    print("patch_gemm_dma_kernel tile instances (MB, NPIX, WM, CK, KG) reached:", tiles)
    print("patch_gemm_kernel tile instances (MB, NPIX, WM, CK) reached:", pro_tiles)
    print("all conv plans:", sorted(CONV_PLANS))
    print("all wgrad plans:", sorted(WGRAD_PLANS))
    assert not missing and not wmissing, (missing, wmissing, sorted(CONV_PLANS), sorted(WGRAD_PLANS))
