"""Epilogues of the split-pipe conv kernels (csrc/conv_common.h: the tile, the 16-byte tile and the pair form, as
patch_gemm_x6p_kernel pipelines them), every operand combination on every epilogue-bearing instance, compared exactly.

Method of tests/conv_sweep_cases.py: x, w, bias, residual, dy, add, mask are small INTEGERS stored as float32 (|.| <= 4,
|w| <= 3), so the convolution sums are integers below 2^24 and the float64 CPU result is exact in float32.  What follows the sum is
reproduced on the CPU in float32, operation by operation in the kernels' order (acc + bias -> act -> + residual -> mask): ReLU
keeps integers; LeakyReLU multiplies negatives by float32(0.2), one rounding that both sides make alike, and the residual added
after it is one more float32 addition.  Every comparison is torch.equal.

Instances are forced the way tests/test_ops_gpu.py's engine fixture does (P2I_X6C_MIN_WG=1, P2I_X6C_TILE) and checked against
p2i_conv_last_plan: (channels, positions, split, 4 = producer / consumer kernel, taps per stage, 7 = split pipe | 8 = fused
strided data gradient).  Shapes are the smallest that reach each path:
  * 3x3 stride 1, Cin 64, Cout 64 / 48 (48: the `o < Cm` guard of a half-filled channel tile), B 1 / 2, maps 8x12 (groups of four
    destination columns: the 64-channel tile takes its 16-byte epilogue) and 7x9 (ragged: clipped lanes, plain epilogue), on the
    32 x 256 (two position blocks per wave pair: the exchange through LDS), 32 x 128 and 64 x 256 tiles;
  * 3x3x3 with t stride 2 (tap slices along t, destination frames strided), 128 -> 128, T 4, 8x8: data gradient with mask, on the
    32 x 128 tile (the only one that holds two 8x8 images);
  * fused strided data gradient, 64 -> 32 channels, stride (1,2,2), 2-D and 3-D (T 3), destination 10x14 (class extents 5x7: the
    pair store clips inside the 8x8 class tile) and 9x13.  The split-pipe kernel takes even destinations only (its four parity
    classes must have equal extents), so 9x13 runs, and is asserted to run, on the f32 engine: same expectation, other kernel.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_sweep_cases as cs

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from p2igan_bench import ops as o
    o._hip.load()
    return o


@pytest.fixture
def x6c(ops, monkeypatch):
    old = ops.CONV_ENGINE
    ops.CONV_ENGINE = "auto"
    monkeypatch.setenv("P2I_X6C_MIN_WG", "1")
    yield monkeypatch
    ops.CONV_ENGINE = old


def _plan(ops):
    p = (ctypes.c_int * 6)()
    ops._hip.load().p2i_conv_last_plan(p)
    return tuple(p)


def _case(cid, nd, B, Cin, Cout, sp, k, s, p):
    c = cs._mk(cid, nd, B, Cin, Cout, sp, k, s, p, "none", True, True)
    assert cs.desc_ok(c) and max(cs.exact_bounds(c)["fwd"], cs.exact_bounds(c)["dgrad"]) < cs.EXACT_LIMIT
    return c


def _ints(gen, shape, m):
    return torch.randint(-m, m + 1, shape, generator=gen).float()


def _inputs(c):
    """Integer data in the sweep's ranges and the float64 sums conv(x, w) and the data gradient of dy, cast to float32 exactly."""
    if c.id not in _REF:
        g = torch.Generator().manual_seed(4242 + sum(map(ord, c.id)))
        xs, ws, ys = cs._shapes(c)
        t = {"x": _ints(g, xs, cs.X_MAX), "w": _ints(g, ws, cs.W_MAX), "bias": _ints(g, (c.Cout,), cs.X_MAX),
             "res": _ints(g, ys, cs.X_MAX), "dy": _ints(g, ys, cs.X_MAX), "add": _ints(g, xs, cs.X_MAX), "mask": _ints(g, xs, cs.X_MAX)}
        conv = F.conv2d if c.nd == 2 else F.conv3d
        st, pd = (c.s[1:], c.p[1:]) if c.nd == 2 else (c.s, c.p)
        x64 = t["x"].double().requires_grad_(True)
        pre = conv(x64, t["w"].double(), None, st, pd)
        dx = torch.autograd.grad(pre, x64, t["dy"].double())[0]
        for name, v in (("pre", pre.detach()), ("dx", dx)):
            assert torch.equal(v.float().double(), v) and float(v.abs().max()) + 2 * cs.X_MAX < cs.EXACT_LIMIT
            t[name] = v.float()
        _REF[c.id] = t
    return _REF[c.id]


def _leaky32(v):
    return torch.where(v > 0, v, v * 0.2)               # float32 throughout: 0.2 becomes float32(0.2), one rounding per product


def _act32(v, act):
    return {"none": lambda u: u, "relu": F.relu, "leaky": _leaky32}[act](v)


def _mask32(v, m, act):
    one = torch.ones_like(v)
    return {"relu": lambda: torch.where(m > 0, v, 0 * one), "leaky": lambda: torch.where(m > 0, v, v * 0.2)}[act]()


def _same(got, exp, what):
    got = got.detach().cpu().reshape(exp.shape)
    if torch.equal(got, exp):
        return
    bad = (got != exp) | torch.isnan(got)
    idx = bad.nonzero()
    first = ["%s: got %r, expected %r" % (tuple(i.tolist()), float(got[tuple(i)]), float(exp[tuple(i)])) for i in idx[:6]]
    raise AssertionError(f"{what}: {int(bad.sum())} of {exp.numel()} elements differ (shape {tuple(exp.shape)}); " + "; ".join(first))


FWD_COMBOS = [("none", False, False), ("relu", True, False), ("none", False, True), ("leaky", True, True)]   # act, bias, residual
DGRAD_COMBOS = [(False, False), (True, False), (False, True), (True, True)]                                  # add, mask


def _run_fwd(ops, c, t, g, want_plan, tag):
    spec = ops.ConvSpec(c.Cin, c.Cout, c.k, c.s, c.p)
    wp_f, _ = ops.weight_pack(g["w"])
    code = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY}
    for act, bias, res in FWD_COMBOS:
        y = ops.conv_fwd(spec, g["x"], wp_f, g["bias"] if bias else None, g["res"] if res else None, code[act])
        plan = _plan(ops)
        assert want_plan(plan), (tag, "fwd", plan)
        exp = t["pre"] + t["bias"].reshape((1, -1) + (1,) * (t["pre"].dim() - 2)) if bias else t["pre"]
        exp = _act32(exp, act)
        if res:
            exp = exp + t["res"]
        _same(y, exp, f"{tag} conv_fwd act={act} bias={bias} residual={res} plan={plan}")


def _run_dgrad(ops, c, t, g, want_plan, tag, mask_act, combos=DGRAD_COMBOS):
    spec = ops.ConvSpec(c.Cin, c.Cout, c.k, c.s, c.p)
    _, wp_d = ops.weight_pack(g["w"])
    code = {"relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY}[mask_act]
    xs = tuple(t["x"].shape)
    for add, mask in combos:
        dx = ops.conv_dgrad(spec, g["dy"], wp_d, xs, add=g["add"] if add else None, mask_y=g["mask"] if mask else None,
                            mask_act=code if mask else ops.ACT_NONE)
        plan = _plan(ops)
        assert want_plan(plan), (tag, "dgrad", plan)
        exp = t["dx"] + t["add"] if add else t["dx"]
        if mask:
            exp = _mask32(exp, t["mask"], mask_act)
        _same(dx, exp, f"{tag} conv_dgrad add={add} mask={mask_act if mask else None} plan={plan}")


TILES = {"82": (64, 256), "81": (32, 256), "41": (32, 128)}        # P2I_X6C_TILE -> (channels, positions) of the plan


@pytest.mark.parametrize("hw", [(8, 12), (7, 9)], ids=["8x12", "7x9"])
@pytest.mark.parametrize("Cout", [64, 48])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("tile", sorted(TILES))
def test_stride1_tiles_every_operand_combination(ops, x6c, tile, B, Cout, hw):
    c = _case("e_s1_b%d_o%d_%dx%d" % (B, Cout, hw[0], hw[1]), 2, B, 64, Cout, hw, (3, 3), (1, 1), (1, 1))
    t = _inputs(c)
    g = {k: v.cuda() for k, v in t.items()}
    x6c.setenv("P2I_X6C_TILE", tile)
    want = lambda p: p[5] == 7 and p[:2] == TILES[tile] and p[2] == 1 and p[3] == 4      # noqa: E731
    _run_fwd(ops, c, t, g, want, f"{c.id} tile {tile}")
    _run_dgrad(ops, c, t, g, want, f"{c.id} tile {tile}", "relu")


@pytest.mark.parametrize("tile", ["41", "auto"])
def test_3d_tap_slices_dgrad_with_mask(ops, x6c, tile):
    """Two 8x8 images per t-parity class: only the 32 x 128 tile holds them (256 positions would span four images, a patch above
    the kernels' 384-pixel limit), forced and as the planner's own choice."""
    c = _case("e_3d_t4", 3, 1, 128, 128, (4, 8, 8), (3, 3, 3), (2, 1, 1), (1, 1, 1))
    t = _inputs(c)
    g = {k: v.cuda() for k, v in t.items()}
    if tile != "auto":
        x6c.setenv("P2I_X6C_TILE", tile)
    want = lambda p: p[5] == 7 and p[:2] == TILES["41"] and p[3] == 4                    # noqa: E731
    _run_dgrad(ops, c, t, g, want, f"{c.id} tile {tile}", "leaky", [(False, True)])


@pytest.mark.parametrize("hw", [(10, 14), (9, 13)], ids=["10x14", "9x13"])
@pytest.mark.parametrize("nd", [2, 3])
def test_fused_strided_dgrad_every_operand_combination(ops, x6c, nd, hw):
    if nd == 2:
        c = _case("e_s2_2d_%dx%d" % hw, 2, 2, 32, 64, hw, (3, 3), (2, 2), (1, 1))
    else:
        c = _case("e_s2_3d_%dx%d" % hw, 3, 2, 32, 64, (3,) + hw, (3, 3, 3), (1, 2, 2), (1, 1, 1))
    t = _inputs(c)
    g = {k: v.cuda() for k, v in t.items()}
    even = hw[0] % 2 == 0 and hw[1] % 2 == 0
    # even destination: the split pipe's fused kernel, producer / consumer form, 32 channels x 256 class positions, no split-K
    want = (lambda p: p[5] == 8 and p[:4] == (32, 256, 1, 4)) if even else (lambda p: p[5] not in (7, 8))
    _run_dgrad(ops, c, t, g, want, c.id, "leaky")
