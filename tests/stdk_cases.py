"""Case tables, seeded inputs and float64 CPU references of the edge-shape sweep of the STDK kernels (csrc/stdk.hip):
test_stdk_kernels_gpu.py runs them on the GPU at the ops level, test_stdk_cases_cpu.py checks on the CPU that the cases reach the
paths they are meant for and that the inputs have the properties the comparisons rely on.  Everything here is torch / numpy on the
CPU and a function of the case alone; nothing is taken from the kernels' output.

Exact family (MLP, layer 1): every input is a small INTEGER stored as float32, so every pre-activation, product and partial sum is
an integer below 2^24 in any summation order; ReLU keeps integers integral and many pre-activations are exactly 0, which pins the
kernels' `> 0` gates to relu'(0) = 0.  The expectation is the float64 result cast to float32 without rounding, the comparison
torch.equal.  Every reference also returns the largest SUM OF ABSOLUTE TERMS of each of its reductions: that bounds every partial
sum of every order, and test_stdk_cases_cpu.py asserts it below EXACT_LIMIT for every case.

The planners of csrc/stdk.hip (frame splits of the forward and backward grids, row chunks of the weight-gradient pass) and of
ops.stdk_layer1_bwd (k-splits of its three products) are restated below from their formulas, so that the CPU test can prove which
guarded path a case reaches."""
from collections import namedtuple

import numpy as np
import torch

import stdk_ref

EXACT_LIMIT = 1 << 24
HID, HP = 100, 112            # hidden width and its padding to 7 tiles of 16
ROWS_WG, ROWS_WAVE = 64, 16   # rows (pixels) of a workgroup and of one of its four waves
K_VISIBLE = 79


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ planners, restated
def fwd_plan(HW, BT):
    """(gx, planned splits, bt_per, grid y) of p2i_stdk_mlp_fwd."""
    gx = ceil_div(HW, ROWS_WG)
    splits = min(BT, max(1, ceil_div(2048, gx)))
    bt_per = ceil_div(BT, splits)
    return gx, splits, bt_per, ceil_div(BT, bt_per)


def bwd_plan(HW, BT):
    """(gx, planned splits, bt_per, grid y = number of dP partials) of p2i_stdk_mlp_bwd."""
    gx = ceil_div(HW, ROWS_WG)
    splits = min(BT, max(1, ceil_div(1024, gx)))
    bt_per = ceil_div(BT, splits)
    return gx, splits, bt_per, ceil_div(BT, bt_per)


def wgrad_plan(nrows):
    """(chunk_rows, chunks, rows of the last chunk) of the weight-gradient pass."""
    chunk_rows = max(256, (ceil_div(nrows, 1024) + 3) // 4 * 4)
    chunks = ceil_div(nrows, chunk_rows)
    return chunk_rows, chunks, nrows - (chunks - 1) * chunk_rows


def wave_rows(HW):
    """Valid rows of every launched 16-row wave tile (four per workgroup): 16 = full, 1..15 = partial, 0 = wholly invalid."""
    return [max(0, min(ROWS_WAVE, HW - ROWS_WAVE * w)) for w in range(4 * ceil_div(HW, ROWS_WG))]


def l1_splits(HW):
    """k-splits that ops.stdk_layer1_bwd hands to its three products (K = H*W, T and B)."""
    return max(1, min(64, HW // 256))


def gemm_chunks(K, splits):
    """Rows of every k-split of stdk_gemm_kernel: kchunk = ceil(K / splits), the last ones ragged or empty."""
    kchunk = ceil_div(max(K, 1), splits)
    return [max(0, min(K, (s + 1) * kchunk) - s * kchunk) for s in range(splits)]


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _sparse_signs(g, shape, density):
    """Values from {-1, 0, 1}, about `density` of them non-zero."""
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * (torch.rand(shape, generator=g) < density).float()


# ------------------------------------------------------------------------------------------------ exact family: fused MLP
MlpCase = namedtuple("MlpCase", "id HW BT seed density")
W_DENSITY = 0.15              # non-zero share of w2 / w3

# (HW, BT); see the module docstring of test_stdk_cases_cpu.py for the path every named case is there for
_MLP = [(79, 1), (81, 3), (65, 5), (64, 2), (16, 4), (1, 7), (257, 7), (1000, 3), (333, 40),
        (1000, 131), (1000, 67), (79, 1030), (877, 300)]
MLP_LARGE = {(1000, 131), (1000, 67), (79, 1030), (877, 300)}        # one GPU test each, the reference is computed in frame chunks


def mlp_cases():
    return [MlpCase("hw%d-bt%d" % (hw, bt), hw, bt, 1000 + i, W_DENSITY) for i, (hw, bt) in enumerate(_MLP)]


def mlp_inputs(c):
    """P [HW, 112], Q [BT, 112] (pad columns zero), w2, b2, w3, b3, w4, b4, dy [BT, HW]: integers as float32."""
    g = torch.Generator().manual_seed(c.seed)
    P, Q = torch.zeros(c.HW, HP), torch.zeros(c.BT, HP)
    P[:, :HID] = _ints(g, (c.HW, HID), -3, 3)
    Q[:, :HID] = _ints(g, (c.BT, HID), -3, 3)
    return dict(P=P, Q=Q, w2=_sparse_signs(g, (HID, HID), c.density), b2=_ints(g, (HID,), -2, 2),
                w3=_sparse_signs(g, (HID, HID), c.density), b3=_ints(g, (HID,), -2, 2), w4=_sparse_signs(g, (1, HID), 0.5),
                b4=_ints(g, (1,), -2, 2), dy=_ints(g, (c.BT, c.HW), -2, 2))


def mlp_reference(t, frames_per_pass=None):
    """float64 forward and hand-written backward of y = w4 relu(W3 relu(W2 relu(P[p] + Q[bt]) + b2) + b3) + b4 over every row
    (bt, p), in passes of a few frames so that the large cases stay cheap (no graph is kept).  Returns (results, bounds): the
    results are y, dP, dQ, dw2, db2, dw3, db3, dw4, db4; bounds[name] is the largest sum of absolute terms of the reductions that
    make `name` (h2, h3, g2, g1 are the inner products of the hidden layers and of the two transposed ones).
    test_stdk_cases_cpu.py checks the backward against autograd."""
    d = {k: v.double() for k, v in t.items()}
    P, Q, w2, b2, w3, b3, w4, b4, dy = (d[k] for k in ("P", "Q", "w2", "b2", "w3", "b3", "w4", "b4", "dy"))
    P, Q, w4 = P[:, :HID], Q[:, :HID], w4.reshape(HID)
    HW, BT = P.shape[0], Q.shape[0]
    step = frames_per_pass or max(1, 32768 // HW)
    r = dict(y=torch.empty(BT, HW, dtype=torch.float64), dP=torch.zeros(HW, HID, dtype=torch.float64),
             dQ=torch.empty(BT, HID, dtype=torch.float64))
    for n, ref in (("dw2", w2), ("db2", b2), ("dw3", w3), ("db3", b3), ("dw4", w4), ("db4", b4)):
        r[n] = torch.zeros_like(ref)
    a = {n: torch.zeros_like(v) for n, v in r.items() if n not in ("y", "dQ")}      # sums of absolute terms, accumulated over passes
    bound = dict(h1=float((P.abs().max(0).values + Q.abs().max(0).values).max()), h2=0.0, h3=0.0, y=0.0, g2=0.0, g1=0.0, dQ=0.0)
    aw2, aw3, aw4 = w2.abs(), w3.abs(), w4.abs()
    for f0 in range(0, BT, step):
        f1 = min(BT, f0 + step)
        nf = f1 - f0
        h1 = torch.relu(P[None] + Q[f0:f1, None]).reshape(nf * HW, HID)
        h2 = torch.relu(h1 @ w2.t() + b2)
        h3 = torch.relu(h2 @ w3.t() + b3)
        r["y"][f0:f1] = (h3 @ w4 + b4).reshape(nf, HW)
        dyr = dy[f0:f1].reshape(nf * HW, 1)
        g3 = dyr * w4 * (h3 > 0)
        g2 = (g3 @ w3) * (h2 > 0)
        g1 = (g2 @ w2) * (h1 > 0)
        r["dw4"] += (dyr * h3).sum(0)
        r["db4"] += dyr.sum()
        r["dw3"] += g3.t() @ h2
        r["db3"] += g3.sum(0)
        r["dw2"] += g2.t() @ h1
        r["db2"] += g2.sum(0)
        r["dP"] += g1.reshape(nf, HW, HID).sum(0)
        r["dQ"][f0:f1] = g1.reshape(nf, HW, HID).sum(1)
        ag3, ag2, ag1 = g3.abs(), g2.abs(), g1.abs()
        bound["h2"] = max(bound["h2"], float((h1 @ aw2.t() + b2.abs()).max()))
        bound["h3"] = max(bound["h3"], float((h2 @ aw3.t() + b3.abs()).max()))
        bound["y"] = max(bound["y"], float((h3 @ aw4 + b4.abs()).max()))
        bound["g2"] = max(bound["g2"], float((ag3 @ aw3).max()))
        bound["g1"] = max(bound["g1"], float((ag2 @ aw2).max()))
        bound["dQ"] = max(bound["dQ"], float(ag1.reshape(nf, HW, HID).sum(1).max()))
        a["dw4"] += (dyr.abs() * h3).sum(0)
        a["db4"] += dyr.abs().sum()
        a["dw3"] += ag3.t() @ h2
        a["db3"] += ag3.sum(0)
        a["dw2"] += ag2.t() @ h1
        a["db2"] += ag2.sum(0)
        a["dP"] += ag1.reshape(nf, HW, HID).sum(0)
    bound.update({n: float(v.max()) for n, v in a.items()})
    r["dw4"] = r["dw4"].reshape(1, HID)
    return r, bound


def mlp_alive(t):
    """Share of units > 0 in h1, h2, h3 and of pre-activations that are exactly 0 in layers 2 and 3 (float64, whole case)."""
    d = {k: v.double() for k, v in t.items()}
    h1 = torch.relu(d["P"][None, :, :HID] + d["Q"][:, None, :HID]).reshape(-1, HID)
    p2 = h1 @ d["w2"].t() + d["b2"]
    p3 = torch.relu(p2) @ d["w3"].t() + d["b3"]
    return [float((v > 0).double().mean()) for v in (h1, p2, p3)], [float((v == 0).double().mean()) for v in (p2, p3)]


# ------------------------------------------------------------------------------------------------ exact family: layer 1
L1Case = namedtuple("L1Case", "id HW B T Ks Kt Kz seed")
# the last one: H*W >= 768 with B = 1 and T = 2, so the three k-splits exceed both small K's (empty splits must write zeros)
_L1 = [(79, 1, 1, 1, 1, 1), (81, 3, 2, 5, 3, 7), (257, 2, 5, 17, 20, 395), (1000, 5, 3, 139, 12, 237), (530, 1, 7, 33, 25, 553),
       (777, 1, 2, 19, 8, 158), (255, 2, 1, 16, 4, 79), (64, 1, 1, 139, 4, 79)]
L1_SENTINEL = ("hw81-b3-t2-k5x3x7", "hw1000-b5-t3-k139x12x237", "hw777-b1-t2-k19x8x158")     # run inside sentinel-filled buffers


def l1_cases():
    return [L1Case("hw%d-b%d-t%d-k%dx%dx%d" % c, *c, 2000 + i) for i, c in enumerate(_L1)]


def l1_inputs(c):
    g = torch.Generator().manual_seed(c.seed)
    F = c.Ks + c.Kt + c.Kz
    return dict(phi_s=_ints(g, (c.HW, c.Ks), -3, 3), phi_t=_ints(g, (c.T, c.Kt), -3, 3), z=_ints(g, (c.B, c.Kz), -3, 3),
                w1=_ints(g, (HID, F), -3, 3), b1=_ints(g, (HID,), -3, 3), dP=_ints(g, (c.HW, HID), -4, 4),
                dQ=_ints(g, (c.B * c.T, HID), -4, 4))


def l1_reference(c, t):
    """float64: P [HW, 112], Q [B*T, 112] with zero pad columns, dw1 [100, F], db1 [100]; and the absolute-term bounds."""
    d = {k: v.double() for k, v in t.items()}
    ws, wt, wz = d["w1"][:, :c.Ks], d["w1"][:, c.Ks:c.Ks + c.Kt], d["w1"][:, c.Ks + c.Kt:]
    P = torch.zeros(c.HW, HP, dtype=torch.float64)
    Q = torch.zeros(c.B * c.T, HP, dtype=torch.float64)
    P[:, :HID] = d["phi_s"] @ ws.t()
    zt, zb = d["phi_t"] @ wt.t(), d["z"] @ wz.t()
    Q[:, :HID] = (zb[:, None] + zt[None] + d["b1"]).reshape(c.B * c.T, HID)
    dq = d["dQ"].reshape(c.B, c.T, HID)
    dqt, dqb = dq.sum(0), dq.sum(1)
    dw1 = torch.cat([d["dP"].t() @ d["phi_s"], dqt.t() @ d["phi_t"], dqb.t() @ d["z"]], dim=1)
    adqt, adqb = dq.abs().sum(0), dq.abs().sum(1)
    bound = dict(P=float((d["phi_s"].abs() @ ws.abs().t()).max()),
                 Q=float((d["phi_t"].abs() @ wt.abs().t()).max() + (d["z"].abs() @ wz.abs().t()).max() + d["b1"].abs().max()),
                 dw1=float(torch.cat([d["dP"].abs().t() @ d["phi_s"].abs(), adqt.t() @ d["phi_t"].abs(), adqb.t() @ d["z"].abs()],
                                     dim=1).max()),
                 db1=float(dq.abs().sum((0, 1)).max()))
    return dict(P=P, Q=Q, dw1=dw1, db1=dq.sum((0, 1))), bound


# ------------------------------------------------------------------------------------------------ visible-point selection
SelCase = namedtuple("SelCase", "id HW B T k frames")      # frames: one pattern name per (b, t) frame, b-major

OBSERVED = (1.0, 0.5, -1.0)       # `!= 0` is the rule, not `== 1` or `> 0`
UNOBSERVED = (0.0, -0.0)          # -0.0 == 0: unobserved


def _spread(n, lo, hi):
    """n distinct pixels spread over [lo, hi)."""
    return sorted({lo + (i * (hi - lo)) // n for i in range(n)}) if n else []


def sel_pattern(name, HW):
    """Observed pixels (ascending) of a named pattern, or None where H*W is too small for it."""
    if name == "none":
        return []
    if name == "all":
        return list(range(HW))
    if name == "last":                                     # 1 observed, the frame's last pixel
        return [HW - 1]
    if name in ("n78", "n79", "n80"):                      # spread over the frame, HW - 1 among them
        n = int(name[1:])
        return None if HW < n else sorted(set(_spread(n - 1, 0, HW - 1)) | {HW - 1})
    if name.startswith("end"):                             # the 79th observed pixel is pixel int(name[3:]); one more at the end
        e = int(name[3:])
        return None if HW < e + 1 else _spread(78, 0, e) + [e] + ([HW - 1] if HW - 1 > e else [])
    if name == "p70+15":                                   # 70 in the first 256-pixel pass of the scan, 15 in later ones
        return None if HW < 513 else _spread(70, 0, 256) + _spread(15, 256, HW)
    if name == "tail":                                     # the last 40 pixels: the scan walks every pass before the first hit
        return list(range(HW - 40, HW))
    raise KeyError(name)


SEL_HW = (79, 80, 255, 256, 257, 513, 1000)
SEL_PATTERNS = ("none", "last", "n78", "n79", "n80", "all", "end255", "end256", "end511", "end512", "p70+15", "tail")
SEL_SINGLE = {79: ("all", "none"), 80: ("n79",), 255: ("n78",), 256: ("none",), 257: ("end255",), 513: ("end511", "end512"),
              1000: ("end256", "p70+15")}


def sel_cases():
    out = []
    for hw in SEL_HW:
        pats = [p for p in SEL_PATTERNS if sel_pattern(p, hw) is not None]
        for lo in range(0, len(pats), 7):                  # BT = 7, another pattern per frame (79 pixels allow six: one comes twice)
            fr = tuple((pats + pats)[lo:lo + 7])
            b, t = ((7, 1), (1, 7))[len(out) % 2]
            out.append(SelCase("hw%d-bt7-%s" % (hw, fr[0]), hw, b, t, K_VISIBLE, fr))
        for p in SEL_SINGLE[hw]:                           # BT = 1
            out.append(SelCase("hw%d-bt1-%s" % (hw, p), hw, 1, 1, K_VISIBLE, (p,)))
    # other k through ops.stdk_select.  k = H*W: every pixel is taken, so the unobserved fill crosses the 256-pixel pass
    # boundaries (with k = 79 it cannot: 256 pixels with fewer than 79 observed hold 79 unobserved)
    for hw, fr in ((79, ("n78", "none", "all")), (257, ("last", "end255", "n80")), (513, ("p70+15", "tail", "none")),
                   (1000, ("n79", "p70+15", "all"))):
        out.append(SelCase("hw%d-bt3-k1" % hw, hw, 3, 1, 1, fr))
        out.append(SelCase("hw%d-bt3-kall" % hw, hw, 1, 3, hw, fr))
    return out


def sel_inputs(c):
    """(x, mask), each (B, T, HW) float32: x is seeded noise (no two pixels alike), observed pixels hold 1, 0.5 or -1 in turn, the
    others 0.0 or -0.0 in turn."""
    g = torch.Generator().manual_seed(3000 + c.HW)
    x = torch.randn(c.B * c.T, c.HW, generator=g)
    m = torch.tensor(UNOBSERVED, dtype=torch.float32).repeat(ceil_div(c.HW, 2))[:c.HW].repeat(c.B * c.T, 1).clone()
    for f, name in enumerate(c.frames):
        obs = sel_pattern(name, c.HW)
        m[f, obs] = torch.tensor(OBSERVED, dtype=torch.float32).repeat(ceil_div(len(obs), 3) + 1)[f % 3:f % 3 + len(obs)]
    return x.reshape(c.B, c.T, c.HW), m.reshape(c.B, c.T, c.HW)


def sel_reference(c, x, m):
    """(idx int32 (B, T, k), z (B, T, k)) by tests/stdk_ref.visible."""
    z, order = stdk_ref.visible(x, m, c.k)
    return order.to(torch.int32), z.reshape(c.B, c.T, c.k)


# ------------------------------------------------------------------------------------------------ Wendland bases
BasisCase = namedtuple("BasisCase", "id H W knots theta")
BASIS_TOL = 1e-6              # absolute, as test_stdk_gpu.test_basis_matches_reference
BASIS_F32_MARGIN = 5e-7       # the float32 evaluation of the formula must itself stay within this of float64

SPACE_GRIDS = ((1, 79), (7, 13), (9, 9), (17, 67))
TIME_LENGTHS = (1, 2, 3, 5, 7)
# H = 79, W = 1: knot 0 on the grid with pixel 15 at d = 1 exactly (and pixel 5 on the other side), knot 1 off the grid in both
# coordinates, knot 2 outside the map, knot 3 with a support that covers one pixel only
HAND_KNOTS = ((10.0, 0.0), (30.5, 0.25), (-3.0, 0.0), (78.0, 0.0))
HAND_THETA = (5.0, 7.5, 16.0, 1.0)


def basis_cases():
    from p2igan_bench.models.stdk import space_knots, time_knots
    out = [BasisCase("1x1-k1", 1, 1, torch.zeros(1, 2), torch.tensor([4.0])),
           BasisCase("79x1-k4-hand", 79, 1, torch.tensor(HAND_KNOTS), torch.tensor(HAND_THETA))]
    for h, w in SPACE_GRIDS:
        k, th = space_knots(h, w)
        out.append(BasisCase("%dx%d-k%d-space" % (h, w, th.numel()), h, w, k, th))
    for t in TIME_LENGTHS:
        k, th = time_knots(t)
        out.append(BasisCase("t%d-k%d-time" % (t, th.numel()), t, 1, k, th))
    return out


def wendland(c, dtype):
    """phi [H*W, K] = (1 - d)^6 (35 d^2 + 18 d + 3) / 3 for d = |pos - knot| / theta <= 1, else 0, evaluated in numpy `dtype`."""
    f = np.dtype(dtype).type
    i = np.arange(c.H * c.W)
    dy = (i // c.W).astype(dtype)[:, None] - c.knots.numpy().astype(dtype)[None, :, 0]
    dx = (i % c.W).astype(dtype)[:, None] - c.knots.numpy().astype(dtype)[None, :, 1]
    d = np.sqrt(dy * dy + dx * dx) / c.theta.numpy().astype(dtype)[None]
    a = f(1) - d
    a2 = a * a
    out = a2 * a2 * a2 * (f(35) * (d * d) + f(18) * d + f(3)) / f(3)
    out = np.where(d <= f(1), out, f(0))
    assert out.dtype == np.dtype(dtype)
    return out


# ------------------------------------------------------------------------------------------------ model-level tolerance family
ModelCase = namedtuple("ModelCase", "id B T H W gauges seed")
KINK_MARGIN = 1e-5            # of a layer's max-abs pre-activation
KT_OF_T = {1: 4, 2: 8, 3: 12, 5: 20, 7: 25}

# (B, T, H, W, gauges, seed): the seeds are the first ones (of a plain upward search) at which the case keeps KINK_MARGIN
_MODEL = [(1, 1, 9, 9, 20, 32), (3, 2, 7, 13, 79, 381), (2, 5, 10, 8, 33, 1785), (1, 3, 1, 79, 12, 36), (2, 3, 79, 1, 40, 64),
          (2, 7, 17, 67, 100, 36)]
# 15946 rows x 100 units x 3 layers of continuous values: some lie within KINK_MARGIN of zero under every seed (about a hundred
# per layer).  For this case the CPU test asserts instead that flipping EVERY such gate at once moves no result by a quarter of its
# tolerance (float32 rounding reaches the few of them that lie within about 1e-6, not all): a flipped gate is then invisible at this
# size, which is what the margin is there to ensure for the small maps.
KINK_BY_FLIP = ("b2-t7-17x67",)
KINK_FLIP_SHARE = 0.25


def model_cases():
    return [ModelCase("b%d-t%d-%dx%d" % c[:4], *c) for c in _MODEL]


def model_inputs(c):
    """(state dict, masked, masks, dy): seeded weights, a synthetic batch under a gauge mask, a one-signed upstream gradient."""
    from p2igan_bench.utils import seeded
    sd = seeded.seeded_stdk_state(c.T, c.seed)
    _, masked, masks = seeded.synthetic_batch(c.B, c.T, c.H, c.W, seeded.gauge_mask(c.H, c.W, c.gauges, c.seed), c.seed)
    dy = torch.rand(masked.shape, generator=torch.Generator().manual_seed(c.seed))
    return sd, masked, masks, dy


def model_bases64(c):
    """(phi_s, phi_t) in float64 from the model's knot tables and the formula above."""
    from p2igan_bench.models.stdk import space_knots, time_knots
    ks, ths = space_knots(c.H, c.W)
    kt, tht = time_knots(c.T)
    return (torch.from_numpy(wendland(BasisCase("s", c.H, c.W, ks, ths), np.float64)),
            torch.from_numpy(wendland(BasisCase("t", c.T, 1, kt, tht), np.float64)))


PARAM_KEYS = tuple("_mlp.net.%d.%s" % (i, n) for i in (0, 2, 4, 6) for n in ("weight", "bias"))


def model_reference(c, inputs=None):
    """tests/stdk_ref.forward in float64 on the CPU: (y, the eight parameter gradients of sum(y * dy))."""
    sd, masked, masks, dy = inputs or model_inputs(c)
    phi_s, phi_t = model_bases64(c)
    params = [sd[k].double().clone().requires_grad_(True) for k in PARAM_KEYS]
    y = stdk_ref.forward(params, phi_s, phi_t, masked, masks)
    (y * dy.double()).sum().backward()
    return y.detach(), [p.grad for p in params]


def model_preacts(c, inputs=None):
    """The float64 pre-activations of the three hidden layers, [rows, 100] each, and y -- the arithmetic of stdk_ref.forward."""
    sd, masked, masks, _ = inputs or model_inputs(c)
    phi_s, phi_t = model_bases64(c)
    w1, b1, w2, b2, w3, b3, w4, b4 = [sd[k].double() for k in PARAM_KEYS]
    z, _ = stdk_ref.visible(masked.double(), masks)
    hw = c.H * c.W
    feats = torch.cat([phi_s.reshape(1, 1, hw, -1).expand(c.B, c.T, hw, -1), phi_t.reshape(1, c.T, 1, -1).expand(c.B, c.T, hw, -1),
                       z.reshape(c.B, 1, 1, -1).expand(c.B, c.T, hw, -1)], dim=3).reshape(c.B * c.T * hw, -1)
    p1 = feats @ w1.t() + b1
    p2 = torch.relu(p1) @ w2.t() + b2
    p3 = torch.relu(p2) @ w3.t() + b3
    return [p1, p2, p3], (torch.relu(p3) @ w4.t() + b4).reshape(c.B, c.T, 1, c.H, c.W)


def kink_margins(pre):
    """min |pre-activation| / max |pre-activation| of every layer."""
    return [float(p.abs().min() / p.abs().max()) for p in pre]


def model_flip_effect(c, inputs=None):
    """(gates within KINK_MARGIN of their kink, change of y, largest change of a parameter gradient) when every such gate of the
    float64 restatement is flipped at once; the changes are relative to max-abs, as the tolerances are."""
    sd, masked, masks, dy = inputs or model_inputs(c)
    yr, gr = model_reference(c, (sd, masked, masks, dy))
    phi_s, phi_t = model_bases64(c)
    params = [sd[k].double().clone().requires_grad_(True) for k in PARAM_KEYS]
    w1, b1, w2, b2, w3, b3, w4, b4 = params
    z, _ = stdk_ref.visible(masked.double(), masks)
    hw = c.H * c.W
    h = torch.cat([phi_s.reshape(1, 1, hw, -1).expand(c.B, c.T, hw, -1), phi_t.reshape(1, c.T, 1, -1).expand(c.B, c.T, hw, -1),
                   z.reshape(c.B, 1, 1, -1).expand(c.B, c.T, hw, -1)], dim=3).reshape(c.B * c.T * hw, -1)
    near = 0
    for w, b in ((w1, b1), (w2, b2), (w3, b3)):
        p = h @ w.t() + b
        flip = p.detach().abs() <= KINK_MARGIN * p.detach().abs().max()
        near += int(flip.sum())
        h = p * ((p.detach() > 0) ^ flip).double()
    y = (h @ w4.t() + b4).reshape(yr.shape)
    (y * dy.double()).sum().backward()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    return near, rel(y.detach(), yr), max(rel(p.grad, g) for p, g in zip(params, gr))
