"""Case generator and CPU reference of the conv-engine sweep (tests/test_conv_sweep_gpu.py, tests/test_conv_sweep_cpu.py).

The sweep walks the descriptor space that check_desc (csrc/conv_common.h) accepts -- kernels up to 27 taps, any stride, any
padding, any extent -- instead of the model's own layers, and it does so with INTEGER-valued float32 data: every product and
every partial sum is then an integer below 2^24, exactly representable, so the expected tensor does not depend on summation
order, split-K, atomics or the engine, and the comparison is torch.equal.

Everything here is deterministic (explicit lists, one seeded random.Random for the thinned product) and needs no GPU.
All geometry is written as 3-tuples (t, h, w); a 2-D case has kt = st = Ti = 1, pt = 0 and is run on 4-D tensors.
"""
import random
from collections import namedtuple

import torch
import torch.nn.functional as F

Case = namedtuple("Case", "id nd B Cin Cout sp k s p act bias res")

# ---- the value table of the sweep (the CPU test asserts that the generated list covers every entry)
K2 = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (1, 2, 2), (1, 1, 3), (1, 3, 1), (1, 3, 3), (1, 2, 3)]
K3 = [(1, 1, 1), (3, 1, 1), (1, 3, 3), (2, 2, 2), (3, 3, 3), (3, 3, 1)]
S2 = [(1, 1, 1), (1, 2, 2), (1, 3, 3), (1, 1, 2), (1, 2, 1), (1, 3, 2), (1, 2, 3), (1, 1, 3)]
S3 = [(1, 1, 1), (2, 2, 2), (1, 3, 3), (3, 2, 2), (2, 1, 1), (1, 2, 1), (1, 1, 2), (1, 2, 2)]
HW = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 40]
TS = [1, 2, 3, 4, 5, 6, 7, 8, 9]
CH = [1, 2, 3, 5, 8, 16, 17, 32, 33, 48, 64, 65]
BATCH = [1, 2, 3, 5]
PAD_MODES = ("zero", "half", "full")          # 0, k // 2, k - 1 per axis; padding = k comes from explicit cases

X_MAX, W_MAX = 4, 3                           # |activations|, |gradients|, |bias|, |residual|, |add| <= 4; |weights| <= 3
MAX_ELEMS = 1 << 22                           # cap on any tensor of a case
MAX_MACS = 12_000_000                         # cap on B*Cout*Cin*taps*To*Ho*Wo: keeps the float64 CPU reference cheap
EXACT_LIMIT = 1 << 24                         # integers below it are exact in float32
SEED = 20261016
PER_COMBO = 2                                 # random exact cases per (kernel, stride) combination


def out_dims(c):
    return tuple((d + 2 * p - k) // s + 1 for d, p, k, s in zip(c.sp, c.p, c.k, c.s))


def taps(c):
    return c.k[0] * c.k[1] * c.k[2]


def macs(c):
    to, ho, wo = out_dims(c)
    return c.B * c.Cout * c.Cin * taps(c) * to * ho * wo


def in_elems(c):
    return c.B * c.Cin * c.sp[0] * c.sp[1] * c.sp[2]


def out_elems(c):
    to, ho, wo = out_dims(c)
    return c.B * c.Cout * to * ho * wo


def desc_ok(c):
    """The arithmetic of check_desc (csrc/conv_common.h), plus what the descriptor leaves to the caller: every extent >= 1."""
    to, ho, wo = out_dims(c)
    return (c.B > 0 and c.Cin > 0 and c.Cout > 0 and min(c.k) >= 1 and taps(c) <= 27 and min(c.s) >= 1 and min(c.p) >= 0
            and min(c.sp) >= 1 and min(to, ho, wo) >= 1
            and all(d + 2 * p >= k for d, p, k in zip(c.sp, c.p, c.k))
            and in_elems(c) < (1 << 31) and out_elems(c) < (1 << 31))


def exact_bounds(c):
    """Upper bounds of the largest intermediate magnitude of each direction with the integer data of exact_inputs.  They are
    computed from the value ranges alone and dominate conv(|x|, |w|) + |bias| + |residual| (and the analogous sums of the
    gradients) for any data inside those ranges."""
    to, ho, wo = out_dims(c)
    npos = c.B * to * ho * wo
    return {"fwd": X_MAX * W_MAX * c.Cin * taps(c) + X_MAX + X_MAX,          # + |bias| + |residual|
            "dgrad": X_MAX * W_MAX * c.Cout * taps(c) + X_MAX,               # + |add|
            "wgrad": X_MAX * X_MAX * npos,                                   # sum over B*To*Ho*Wo of x * dy
            "bgrad": X_MAX * npos}


def expected_refusal(c, op, with_y_act):
    """The one limit the source states for these shapes: `wgrad supports kh*kw <= 9` (csrc/wgrad.hip), checked after the
    single-input-channel kernel (Cin == 1, Cout <= 32, taps <= 32, no act'(y) prologue) has had its turn.  The LDS refusals
    (`does not fit LDS`) need patches far above the sweep's extents (<= 40 pixels per axis, stride <= 3): none is expected.
    Returns the message fragment a refusal of (case, op) must carry, or None when the call has to succeed."""
    if op == "wgrad" and c.k[1] * c.k[2] > 9:
        c1 = c.Cin == 1 and c.Cout <= 32 and taps(c) <= 32 and not with_y_act
        if not c1:
            return "kh*kw <= 9"
    return None


def _mk(cid, nd, B, Cin, Cout, sp, k, s, p, act="none", bias=False, res=False):
    if nd == 2:
        sp, k, s, p = (1,) + tuple(sp), (1,) + tuple(k), (1,) + tuple(s), (0,) + tuple(p)
    return Case(cid, nd, B, Cin, Cout, tuple(sp), tuple(k), tuple(s), tuple(p), act, bias, res)


def explicit_cases():
    """Hand-written cases: the size-1 tile axes (a kernel axis with one tap and one output row / column of it: the planners'
    index divisor would be 1), every kernel family of the dispatch, padding = k, and the wgrad limit."""
    m = _mk
    return [
        # ---- size-1 patch axes: eH == 1 (kh == 1, Ho == 1), eth == 1 (+ kt == 1), eW == 1 (kw == 1, Wo == 1, 4-byte DMA)
        m("mg_1x1_h1", 2, 2, 16, 32, (1, 20), (1, 1), (1, 1), (0, 0), "none", True, False),
        m("mg_1x1_w1", 2, 3, 16, 32, (7, 1), (1, 1), (1, 1), (0, 0), "relu", False, True),
        m("mg_1x3_h1", 2, 2, 16, 32, (1, 20), (1, 3), (1, 1), (0, 1), "none", True, True),
        m("mg_1x1x1_t4", 3, 2, 16, 32, (4, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0), "relu", True, False),
        m("mg_1x1_h1_odd", 2, 5, 5, 3, (1, 33), (1, 1), (1, 1), (0, 0), "none", False, False),
        m("mg_3x1_w1", 2, 2, 8, 8, (9, 1), (3, 1), (1, 1), (1, 0), "relu", True, False),
        m("mg_1x1_h1_s2", 2, 3, 32, 17, (1, 31), (1, 1), (1, 2), (0, 0), "none", True, True),
        m("mg_1x1_1x1", 2, 5, 48, 33, (1, 1), (1, 1), (1, 1), (0, 0), "relu", True, True),
        m("mg_1x1x1_h1", 3, 2, 8, 16, (3, 1, 16), (1, 1, 1), (1, 1, 1), (0, 0, 0), "none", False, True),
        m("mg_3x1x1_h1w1", 3, 1, 16, 16, (6, 1, 1), (3, 1, 1), (2, 1, 1), (1, 0, 0), "none", True, False),
        # ---- outputs of extent 1 on each axis in turn, and on all
        m("o1_all", 2, 3, 8, 5, (3, 3), (3, 3), (1, 1), (0, 0), "relu", True, False),
        m("o1_h", 2, 2, 17, 8, (3, 16), (3, 3), (1, 1), (0, 1), "none", False, True),
        m("o1_w", 2, 2, 8, 17, (15, 2), (2, 2), (1, 1), (0, 0), "none", True, False),
        m("o1_t", 3, 2, 8, 8, (3, 8, 8), (3, 3, 3), (1, 1, 1), (0, 1, 1), "relu", True, True),
        m("o1_all3", 3, 5, 3, 2, (2, 2, 2), (2, 2, 2), (2, 2, 2), (0, 0, 0), "none", True, False),
        # ---- padding = k: a whole tap row / column / frame outside the tensor
        m("pad_k_3x3", 2, 2, 5, 8, (5, 7), (3, 3), (1, 1), (3, 3), "relu", True, True),
        m("pad_k_3x3_s2", 2, 1, 16, 16, (8, 8), (3, 3), (2, 2), (3, 3), "none", False, False),
        m("pad_k_2x2x2", 3, 2, 3, 5, (3, 4, 5), (2, 2, 2), (1, 2, 1), (2, 2, 2), "none", True, False),
        # ---- several column tiles
        m("wide_3x3", 2, 1, 8, 16, (4, 40), (3, 3), (1, 1), (1, 1), "relu", True, True),
        m("wide_1x3_s1x3", 2, 2, 3, 33, (2, 40), (1, 3), (1, 1), (0, 2), "none", False, False),
        # ---- the split pipe (kind 7), the fused strided data gradients (kinds 8 and 14), odd Wi with stride 2 (pair_w off)
        m("x6_3x3_16", 2, 2, 16, 32, (16, 16), (3, 3), (1, 1), (1, 1), "relu", True, True),
        m("x6_3x3_64", 2, 1, 64, 64, (8, 16), (3, 3), (1, 1), (1, 1), "none", True, False),
        m("x6_3x3_48_odd", 2, 3, 48, 17, (7, 17), (3, 3), (1, 1), (1, 1), "none", False, True),
        m("x6_3x3x3_t1", 3, 1, 16, 32, (5, 8, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1), "none", True, True),
        m("x6_3x3x3_t2", 3, 2, 32, 48, (6, 8, 8), (3, 3, 3), (2, 1, 1), (1, 1, 1), "relu", True, False),
        m("x6_3x3x3_64", 3, 1, 64, 64, (3, 4, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1), "none", True, False),
        m("s2_3x3_16", 2, 2, 16, 32, (16, 16), (3, 3), (2, 2), (1, 1), "relu", True, False),
        m("s2_3x3_odd", 2, 2, 32, 16, (15, 17), (3, 3), (2, 2), (1, 1), "none", True, False),
        m("s2_3x3_oddw", 2, 3, 8, 16, (8, 7), (3, 3), (2, 2), (1, 1), "none", False, False),
        m("s2_3x3x3_32", 3, 2, 32, 64, (2, 16, 16), (3, 3, 3), (1, 2, 2), (1, 1, 1), "relu", True, False),
        m("s2_2x2_16", 2, 2, 8, 16, (8, 8), (2, 2), (2, 2), (0, 0), "none", True, False),
        # ---- single input channel (c1_fwd / c1_dgrad / c1_wgrad), single output channel (o1_fwd_kernel)
        m("c1_3x3x3", 3, 2, 1, 32, (4, 16, 16), (3, 3, 3), (1, 2, 2), (1, 1, 1), "relu", True, False),
        m("c1_3x3x3_odd", 3, 1, 1, 17, (5, 17, 22), (3, 3, 3), (1, 2, 2), (1, 1, 1), "none", True, False),
        m("c1_3x3_s3", 2, 3, 1, 8, (16, 17), (3, 3), (3, 3), (1, 1), "none", True, True),
        m("c1_2x2x2_65", 3, 2, 1, 65, (3, 5, 7), (2, 2, 2), (1, 1, 2), (1, 0, 1), "relu", False, False),
        m("to1_3x3", 2, 2, 40, 1, (9, 20), (3, 3), (1, 1), (1, 1), "none", True, False),
        m("to1_3x3_wide", 2, 1, 16, 1, (1, 40), (3, 3), (1, 1), (1, 1), "relu", True, False),
        m("to1_1x1", 2, 2, 33, 1, (5, 5), (1, 1), (1, 1), (0, 0), "none", True, True),
        m("c1_to1", 2, 2, 1, 1, (8, 8), (3, 3), (1, 1), (1, 1), "none", True, False),
        # ---- the stride product above eight classes (one launch per class), t strides
        m("s133_3x3x3", 3, 1, 8, 8, (3, 9, 10), (3, 3, 3), (1, 3, 3), (1, 1, 1), "none", True, False),
        m("s322_3x3x3", 3, 2, 5, 8, (7, 8, 8), (3, 3, 3), (3, 2, 2), (1, 1, 1), "relu", False, False),
        m("s222_2x2x2", 3, 2, 16, 16, (4, 8, 8), (2, 2, 2), (2, 2, 2), (0, 0, 0), "none", True, False),
        m("s3_1x1", 2, 2, 16, 16, (8, 8), (1, 1), (3, 3), (0, 0), "none", True, True),       # classes without any tap
        # ---- the one stated limit: wgrad supports kh*kw <= 9 (forward and data gradient take the layer)
        m("k2x5_wgrad_limit", 2, 2, 8, 8, (6, 9), (2, 5), (1, 1), (0, 2), "none", True, False),
    ]


# cases the generator MEANS for the bf16-split pipe under P2I_X6C_MIN_WG=1: (id, dgrad) pairs p2i_x6c_would_take must accept
X6C_INTENDED = [("x6_3x3_16", 0), ("x6_3x3_16", 1), ("x6_3x3_64", 0), ("x6_3x3_64", 1), ("x6_3x3_48_odd", 0),
                ("x6_3x3x3_t1", 0), ("x6_3x3x3_t1", 1), ("x6_3x3x3_t2", 0), ("x6_3x3x3_64", 0),
                ("s2_3x3_16", 1), ("s2_3x3x3_32", 1)]


def _pad_of(mode, k):
    return {"zero": 0, "half": k // 2, "full": k - 1}[mode]


def _draw(rng, nd, k, s, tag, min_elems=1):
    """One case of this kernel and stride, the other dimensions drawn from the table and redrawn (deterministically) until the
    case is valid, below the size caps and has at least min_elems input and output elements."""
    for _ in range(1000):
        B, Cin, Cout = rng.choice(BATCH), rng.choice(CH), rng.choice(CH)
        sp = (rng.choice(TS) if nd == 3 else 1, rng.choice(HW), rng.choice(HW))
        p = tuple(_pad_of(rng.choice(PAD_MODES), kk) for kk in k)
        act, bias, res = rng.choice(("none", "relu")), rng.random() < 0.5, rng.random() < 0.5
        cid = "r%d_k%s_s%s_%s" % (nd, "x".join(map(str, k[3 - nd:])), "x".join(map(str, s[3 - nd:])), tag)
        c = Case(cid, nd, B, Cin, Cout, sp, k, s, p, act, bias, res)
        if (desc_ok(c) and macs(c) <= MAX_MACS and max(in_elems(c), out_elems(c)) <= MAX_ELEMS
                and min(in_elems(c), out_elems(c)) >= min_elems):
            return c
    raise AssertionError("no valid case for %s %s" % (k, s))


def combos():
    return [(nd, k, s) for nd, ks, ss in ((2, K2, S2), (3, K3, S3)) for k in ks for s in ss]


def random_cases():
    """PER_COMBO cases per (kernel, stride) combination of the table, drawn by one seeded generator."""
    rng = random.Random(SEED)
    return [_draw(rng, nd, k, s, str(rep)) for nd, k, s in combos() for rep in range(PER_COMBO)]


_CACHE = {}


def exact_cases():
    if "exact" not in _CACHE:
        _CACHE["exact"] = explicit_cases() + random_cases()
    return _CACHE["exact"]


TOL_MIN_ELEMS = 256       # the max-abs-relative measure needs a population: tolerance cases have >= 256 inputs and outputs


def tolerance_cases():
    """Thinned subset for the randn / leaky / tanh family: for every (kernel, stride) combination the first exact case (random
    cases in generation order, then explicit ones) with at least TOL_MIN_ELEMS input and output elements per batch; activation
    alternates leaky / tanh, bias on, residual alternates."""
    if "tol" in _CACHE:
        return _CACHE["tol"]
    seen, out = set(), []
    pool = [c for c in random_cases() + explicit_cases() if expected_refusal(c, "wgrad", True) is None]
    for c in pool:
        key = (c.nd, c.k, c.s)
        if key in seen or min(in_elems(c), out_elems(c)) < TOL_MIN_ELEMS:
            continue
        seen.add(key)
        n = len(out)
        out.append(c._replace(id="tol_" + c.id, act=("leaky", "tanh")[n % 2], bias=True, res=(n // 2) % 2 == 1))
    rng = random.Random(SEED + 1)                 # combinations whose exact cases are all too small: one more draw each
    for nd, k, s in combos():
        if (nd, k, s) not in seen:
            n = len(out)
            c = _draw(rng, nd, k, s, "t", TOL_MIN_ELEMS)
            out.append(c._replace(id="tol_" + c.id, act=("leaky", "tanh")[n % 2], bias=True, res=(n // 2) % 2 == 1))
    _CACHE["tol"] = out
    return out


# ------------------------------------------------------------------------------------------------ data and reference

def _shapes(c):
    to, ho, wo = out_dims(c)
    if c.nd == 2:
        return (c.B, c.Cin) + c.sp[1:], (c.Cout, c.Cin) + c.k[1:], (c.B, c.Cout, ho, wo)
    return (c.B, c.Cin) + c.sp, (c.Cout, c.Cin) + c.k, (c.B, c.Cout, to, ho, wo)


def _seed_of(c, cases):
    return 1000 + [x.id for x in cases].index(c.id)


def _ints(gen, shape, m):
    return torch.randint(-m, m + 1, shape, generator=gen).float()


def exact_inputs(c):
    """Integer-valued float32 tensors (zeros included): x, w, bias, residual, dy, add, mask."""
    g = torch.Generator().manual_seed(_seed_of(c, exact_cases()))
    xs, ws, ys = _shapes(c)
    return {"x": _ints(g, xs, X_MAX), "w": _ints(g, ws, W_MAX), "bias": _ints(g, (c.Cout,), X_MAX) if c.bias else None,
            "res": _ints(g, ys, X_MAX) if c.res else None, "dy": _ints(g, ys, X_MAX), "add": _ints(g, xs, X_MAX),
            "mask": _ints(g, xs, X_MAX)}


def randn_inputs(c):
    g = torch.Generator().manual_seed(_seed_of(c, tolerance_cases()))
    xs, ws, ys = _shapes(c)
    fan = c.Cin * taps(c)

    def rn(shape, scale=1.0):
        return (torch.randn(shape, generator=g) * scale).float()
    return {"x": rn(xs), "w": rn(ws, fan ** -0.5), "bias": rn((c.Cout,), 0.1) if c.bias else None, "res": rn(ys) if c.res else None,
            "dy": rn(ys), "add": rn(xs), "mask": rn(xs)}


def act_fn(v, act):
    return {"none": lambda t: t, "relu": F.relu, "leaky": lambda t: F.leaky_relu(t, 0.2), "tanh": torch.tanh}[act](v)


def act_grad_of(y, act):
    """d act / d pre-activation expressed through the post-activation y (csrc/common.h: act_grad)."""
    one = torch.ones_like(y)
    return {"none": one, "relu": (y > 0).to(y.dtype), "leaky": torch.where(y > 0, one, 0.2 * one), "tanh": 1 - y * y}[act]


def reference(c, t, pro_act):
    """float64 CPU reference of everything the sweep runs.  pro_act: the activation whose derivative the act'(y) prologues
    and the epilogue mask apply (relu in the exact family, the case's own in the tolerance family).
      out      act(conv(x, w) + bias) + residual
      y_act    act_pro(conv(x, w) + bias): the saved activation handed to the prologue calls
      dx, dw, db          gradients of conv for the output gradient dy
      dx_p, dw_p, db_p    the same for dy * act_pro'(y_act)
      dx_e     (dx + add) * act_pro'(mask)"""
    conv = F.conv2d if c.nd == 2 else F.conv3d
    st, pd = (c.s[1:], c.p[1:]) if c.nd == 2 else (c.s, c.p)
    x = t["x"].double().requires_grad_(True)
    w = t["w"].double().requires_grad_(True)
    b = t["bias"].double().requires_grad_(True) if t["bias"] is not None else None
    pre = conv(x, w, b, st, pd)
    leaves = [x, w] + ([b] if b is not None else [])
    out = act_fn(pre, c.act).detach()
    if t["res"] is not None:
        out = out + t["res"].double()
    y_act = act_fn(pre, pro_act).detach()
    dy = t["dy"].double()
    g = torch.autograd.grad(pre, leaves, dy, retain_graph=True)
    gp = torch.autograd.grad(pre, leaves, dy * act_grad_of(y_act, pro_act))
    r = {"out": out, "y_act": y_act, "dx": g[0], "dw": g[1], "db": g[2] if b is not None else None,
         "dx_p": gp[0], "dw_p": gp[1], "db_p": gp[2] if b is not None else None}
    r["dx_e"] = (g[0] + t["add"].double()) * act_grad_of(t["mask"].double(), pro_act)
    if b is None:                                  # the bias gradient does not need a bias in the forward
        red = [0] + list(range(2, dy.dim()))
        r["db"], r["db_p"] = dy.sum(red), (dy * act_grad_of(y_act, pro_act)).sum(red)
    return r
