"""Case tables, seeded inputs, float64 expectations and error scales of the edge sweep of the loss family (csrc/loss_ext.hip).
test_loss_ext_edges_gpu.py runs the cases on the GPU; test_loss_ext_cases_cpu.py checks on the CPU that every case has the sizes
it is there for.  Everything here is torch on the device of its inputs and a function of the case alone: explicit lists and seeded
generators, nothing taken from a kernel's output.

Three families.
  exact       integer-valued data (fdiff) and distinct integers (spatial_pool): torch.equal against torch on the CPU.
  tolerance   per element, e_i = |got_i - ref_i| / (2^-24 scale_i), ref the float64 restatement (losses_ext_ref.py) on the same
              float32 inputs and scale_i the first-order size of a correctly rounded float32 evaluation's error: the sum over the
              operands of the formula of |partial derivative| |operand|, plus |ref_i|, from float64 intermediates only.  Each
              formula stands next to its function.  scale_i is never below 2^-102: a float32 result under the smallest normal
              number (2^-126 = 2^-24 2^-102) may be flushed to 0, which is an absolute error of that size.
  non-finite  NaN / Inf at chosen places of a pool window; the non-finite pattern is compared, finite elements as above.

The bound on max e_i is one number per operation and direction: F32_E below is that maximum for the restatement itself run in
float32 on the CPU over the operation's whole case table (test_loss_ext_cases_cpu.py recomputes it), and the kernels are held to
bound(op) = max(8, 4 F32_E[op]).  The factor 4 is for what a CPU float32 run does not share with the kernels: the device's tanhf,
expf, exp2f and logf, each a few ulp from torch's CPU routines, and the kernels' own order of additions.

Caps and sizes restate ext_grid and the launch lines of csrc/loss_ext.hip."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import losses_ext_ref as R

U = 2.0 ** -24                    # unit roundoff of float32
SCALE_FLOOR = 2.0 ** -102
LN10 = math.log(10.0)
TEMP = R.TEMP

# ---------------------------------------------------------------- launch geometry (csrc/loss_ext.hip)
WG = 256
ELEM_CAP = 4096                   # workgroups of transform / fdiff / wl1_bwd / kl_bwd
POOL_CAP = 8192                   # spool_fwd, spool_bwd, shock_gather
TDM_CAP = 512
ELEM_ONE_TRIP_VEC = ELEM_CAP * WG * 4        # 4,194,304 floats on the 16-byte path
ELEM_ONE_TRIP_SCALAR = ELEM_CAP * WG         # 1,048,576
POOL_ONE_TRIP = POOL_CAP * WG                # 2,097,152
TDM_ONE_TRIP = TDM_CAP * WG                  # 131,072
SOFTMAX_WIDE_L = 1024             # block of 1024 threads from this row length on, 256 below
STW, STH = 32, 8                  # shock tile
SHOCK_MAX_PLANES = 65535

# restatement in float32 on the CPU: max e_i over the whole table of each operation (printed by test_loss_ext_cases_cpu.py)
F32_E = {
    "transform_fwd": 2.6, "transform_bwd": 2.2, "wl1_fwd": 0.35, "wl1_bwd": 1.2, "kl_fwd": 0.3, "kl_bwd": 0.45,
    "softmax_fwd": 2.3, "softmax_bwd": 1.25, "tdm_loss": 0.2, "tdm_coef": 0.65, "tdm_bwd": 0.45,
    "shock_map_fwd": 1.15, "shock_map_bwd": 0.65, "shock_loss_fwd": 1.3, "shock_loss_bwd": 1.15,
}


def bound(op):
    return max(8.0, 4.0 * F32_E[op])


def err(got, ref, scale):
    """max e_i over the elements where ref is finite (0.0 when there is none)."""
    ref = ref.double()
    ok = torch.isfinite(ref)
    if not bool(ok.any()):
        return 0.0
    s = torch.clamp(scale.double().expand_as(ref)[ok], min=SCALE_FLOOR)
    return float(((got.double()[ok] - ref[ok]).abs() / (U * s)).max())


def misaligned(t):
    """The same values 4 bytes past a fresh allocation: a contiguous view with storage offset 1."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def is_vec_path(n, *tensors):
    """EXT_VEC: n % 4 == 0 and every pointer 16-byte aligned (allocations are; a view adds 4 bytes per element of offset)."""
    return n % 4 == 0 and all((t.storage_offset() * t.element_size()) % 16 == 0 for t in tensors)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================ element-wise: transform, weighted L1, KL
ELEM_N = [1, 3, 4, 5, 1023, 1024, 1025]
ELEM_N_SECOND_TRIP = [4197396, 1049349]          # aligned 16-byte path; scalar path
WL1_XMAX = torch.tensor(0.70, dtype=torch.float32)


def elem_sizes():
    return ELEM_N + ELEM_N_SECOND_TRIP


def transform_inputs(n):
    g = _gen(1000 + n % 9973)
    return torch.rand(n, generator=g) * 1.2 - 0.1, torch.randn(n, generator=g)


def transform_ref(x, dy):
    """y = 0.036 * 10^e, e = x * 255 / 3 * 0.0625.  scale(y) = |y| (1 + |e| ln 10): the exponent's rounding, |dy/de| |e|, plus |y|.
    dx = dy * y * ln 10 * de/dx.  scale(dx) = |dx| (2 + |e| ln 10): the same through y, |dx| for the operand dy, plus |dx|."""
    x, dy = x.double(), dy.double()
    e = x * 255.0 / 3.0 * 0.0625
    y = R.transform(x)
    dx = dy * y * (LN10 * 255.0 / 3.0 * 0.0625)
    return y, y.abs() * (1 + e.abs() * LN10), dx, dx.abs() * (2 + e.abs() * LN10)


def wl1_inputs(n):
    """pred, true in [0, 1); targets at 0.70f and its two float32 neighbours (the weight clamps there), pred == true at two places."""
    g = _gen(2000 + n % 9973)
    pred, true = torch.rand(n, generator=g), torch.rand(n, generator=g)
    if n >= 3:
        true[0] = WL1_XMAX
        true[1] = torch.nextafter(WL1_XMAX, torch.tensor(1.0))
        true[2] = torch.nextafter(WL1_XMAX, torch.tensor(0.0))
    if n >= 5:
        pred[1] = true[1]
        pred[4] = true[4]
    return pred, true


WL1_GOUT = 0.75


def wl1_ref(pred, true, gout=WL1_GOUT):
    """loss = mean(w |p - y|), w = 0.5 exp(5.14 min(y, 0.7)) + 0.12.  scale(w) = (w - 0.12)(1 + 5.14 |c|) + 0.12 with c the clamped
    target: the exponential's argument 5.14 c, the product with 0.5, the constant.  Term t = w |p - y|:
    scale(t) = scale(w) |p - y| + w (|p| + |y|) + |t|.  scale(loss) = mean(scale(t)) + |loss|, the terms being the sum's operands.
    dpred = gout / n * sign(p - y) * w.  scale(dpred) = |gout| / n * scale(w) + |dpred| (0 where p == y, and there the gradient is
    exactly 0: the difference of two float32 numbers has the right sign)."""
    p, y = pred.double(), true.double()
    n = p.numel()
    c = torch.clamp(y, max=0.7)
    w = 0.5 * torch.exp(5.14 * c) + 0.12
    sw = (w - 0.12) * (1 + 5.14 * c.abs()) + 0.12
    d = p - y
    t = w * d.abs()
    loss = t.mean()
    sloss = (sw * d.abs() + w * (p.abs() + y.abs()) + t).mean() + loss.abs()
    dp = gout / n * torch.sign(d) * w
    sdp = abs(gout) / n * sw * (d != 0) + dp.abs()
    return loss, sloss, dp, sdp


def kl_batch(n):
    return 3 if n % 3 == 0 else 1


def kl_inputs(n):
    """p = float64 softmax (never 0) rounded to float32, q a distribution with exact zeros; shape (B, n / B)."""
    g = _gen(3000 + n % 9973)
    B = kl_batch(n)
    p = torch.softmax(2.0 * torch.randn(B, n // B, generator=g, dtype=torch.float64), dim=1).float()
    q = torch.softmax(2.0 * torch.randn(B, n // B, generator=g, dtype=torch.float64), dim=1).float()
    q[:, ::3] = 0.0
    return p, q


KL_GOUT = -1.5


def kl_ref(p, q, gout=KL_GOUT):
    """loss = sum(t) / B, t = xlogy(q, q) - q log p.  scale(t) = 2 |q log q| + 2 |q log p| + 2 |q| + |t|: each logarithm's rounding
    and that of its product with q, the argument's rounding seen through the logarithm (q each), the difference.
    scale(loss) = sum(scale(t)) / B + |loss|.  dp = -gout q / (p B): three operands of relative weight 1, scale(dp) = 4 |dp|."""
    p, q = p.double(), q.double()
    B = p.shape[0]
    qlq, qlp = torch.xlogy(q, q), q * p.log()
    t = qlq - qlp
    loss = t.sum() / B
    sloss = (2 * qlq.abs() + 2 * qlp.abs() + 2 * q.abs() + t.abs()).sum() / B + loss.abs()
    dp = -gout * q / (p * B)
    return loss, sloss, dp, 4 * dp.abs()


# ================================================================ forward difference (exact)
FDIFF_B, FDIFF_T, FDIFF_INNER = [1, 3], [2, 3, 17], [1, 3, 4, 5, 28, 1028]
FDIFF_SECOND_TRIP = [(2, 3, 1049348), (2, 3, 1049349)]        # vector path; scalar path

FdiffCase = namedtuple("FdiffCase", "B T inner shift")        # shift: build the tensor one float into a longer buffer


def fdiff_cases(second_trip=False):
    if second_trip:
        return [FdiffCase(B, T, inner, False) for B, T, inner in FDIFF_SECOND_TRIP]
    out = []
    for B in FDIFF_B:
        for T in FDIFF_T:
            for inner in FDIFF_INNER:
                out.append(FdiffCase(B, T, inner, False))
                if inner % 4 == 0:
                    out.append(FdiffCase(B, T, inner, True))
    return out


def fdiff_inputs(c):
    """x (B, T, inner) and dy (B, T - 1, inner): integers of magnitude <= 1000 as float32, so every difference is exact."""
    g = _gen(4000 + 97 * c.B + 13 * c.T + c.inner % 9973)
    x = torch.randint(-1000, 1001, (c.B, c.T, c.inner), generator=g).float()
    dy = torch.randint(-1000, 1001, (c.B, c.T - 1, c.inner), generator=g).float()
    return x, dy


def fdiff_ref(x, dy):
    out = x[:, 1:] - x[:, :-1]
    dx = torch.zeros_like(x)
    dx[:, 1:] += dy
    dx[:, :-1] -= dy
    return out, dx


# ================================================================ MaxPool2d(5, 4, 2) (exact)
SPOOL_SMALL = list(range(1, 10))
SPOOL_EXTRA = [(13, 66), (66, 13)]
SPOOL_SECOND_TRIP_FWD = (9, 1932, 1932)          # 9 * 483 * 483 = 2,099,601 pooled outputs
SPOOL_SECOND_TRIP_BWD = (9, 483, 483)            # 2,099,601 stored pixels

SpoolCase = namedtuple("SpoolCase", "shape")


def spool_cases():
    hw = [(h, w) for h in SPOOL_SMALL for w in SPOOL_SMALL] + SPOOL_EXTRA
    out = []
    for i, (h, w) in enumerate(hw):
        n = (1, 5)[i % 2]
        four = (i // 2) % 2 == 1
        out.append(SpoolCase(((1, n, h, w) if i % 3 else (n, 1, h, w)) if four else (n, h, w)))
    return out


def spool_inputs(shape, seed=5000):
    """Distinct integers, about half of them negative, in a seeded order; an integer upstream gradient."""
    n = 1
    for s in shape:
        n *= s
    g = _gen(seed + n % 9973)
    x = (torch.randperm(n, generator=g) - n // 2).float().reshape(shape)
    ho, wo = (shape[-2] - 1) // 4 + 1, (shape[-1] - 1) // 4 + 1
    dy = torch.randint(-9, 10, tuple(shape[:-2]) + (ho, wo), generator=g).float()
    return x, dy


def spool_ref(x, dy):
    """(out, plane index h * W + w of the argmax, dx) from torch on the CPU; dx from float64 autograd."""
    x4 = x.reshape((-1, 1) + tuple(x.shape[-2:])).cpu()
    out, idx = F.max_pool2d(x4, 5, 4, 2, return_indices=True)
    x64 = x.cpu().double().requires_grad_(True)
    (R.spatial_pool(x64) * dy.cpu().double()).sum().backward()
    return out.reshape(dy.shape), idx.reshape(dy.shape).int(), x64.grad.float()


def window_maxima_unique(x):
    """Every 5/4/2 window of every plane holds its maximum once."""
    x4 = x.reshape((-1, 1) + tuple(x.shape[-2:])).double()
    m = F.max_pool2d(x4, 5, 4, 2)
    cols = F.unfold(F.pad(x4, (2, 2, 2, 2), value=float("-inf")), 5, stride=4)          # (N, 25, windows)
    return bool(((cols == m.reshape(m.shape[0], 1, -1)).sum(dim=1) == 1).all())


# ================================================================ row softmax with temperature
SOFTMAX_L = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 4097]
SOFTMAX_ROWS = 3
SOFTMAX_MANY_ROWS = (65537, 3)


def softmax_shapes():
    return [(1, SOFTMAX_ROWS, L) for L in SOFTMAX_L] + [(SOFTMAX_MANY_ROWS[0], 1, SOFTMAX_MANY_ROWS[1])]


def softmax_inputs(shape):
    """x in [-12, 0] with the row maximum at 0, so z - max z = 10 x reaches -120: arguments under -104 give expf = 0 exactly."""
    g = _gen(6000 + shape[0] + 7 * shape[2])
    x = -12.0 * torch.rand(shape, generator=g)
    if shape[2] >= 2:
        x[..., 0] = 0.0
        x[..., 1] = -11.5
    return x, torch.randn(shape, generator=g)


def softmax_ref(x, dy):
    """y = exp(z - m) / sum, z = x / temperature, m = max z.  scale(y) = y (1 + |z - m|): the exponential's argument, plus y.
    dx = y (dy - dot) / temperature, dot = sum(y dy), with y the forward's float32 output:
    scale(dx) = |dx| (2 + |z - m|) + y / temperature * (|dy| + sum_j |y_j dy_j| (2 + |z_j - m|))."""
    x64, dy = x.double(), dy.double()
    z = x64.reshape(x.shape[0], x.shape[1], -1) / TEMP
    zm = (z - z.max(dim=-1, keepdim=True).values).reshape(x.shape).abs()
    y = R.softmax_temperature(x64, TEMP)
    sy = y * (1 + zm)
    dot = (y * dy).sum(dim=-1, keepdim=True)
    dx = y * (dy - dot) / TEMP
    sdot = ((y * dy).abs() * (2 + zm)).sum(dim=-1, keepdim=True)
    sdx = dx.abs() * (2 + zm) + y / TEMP * (dy.abs() + sdot)
    return y, sy, dx, sdx


# ================================================================ temporal-difference matching
TDM_SHAPES = [(1, 1, 2, 3), (2, 2, 4, 4), (1, 3, 5, 5), (2, 2, 6, 9), (1, 2, 8, 8), (1, 2, 33, 7), (3, 5, 400, 404)]
TDM_BETAS = [1.0, 30.0]
TDM_EPS = 1e-6
TDM_GOUT = 0.75

TdmCase = namedtuple("TdmCase", "shape beta")


def tdm_cases():
    return [TdmCase(s, TDM_BETAS[(i + 1) % 2]) for i, s in enumerate(TDM_SHAPES)] + [TdmCase(TDM_SHAPES[3], 1.0), TdmCase(TDM_SHAPES[1], 30.0)]


def tdm_positions(shape):
    B, t, H, W = shape
    return B * t * ((H - 1) // 4 + 1) * ((W - 1) // 4 + 1)


def tdm_inputs(shape):
    """pred_diff: distinct values in [-0.5, 0.5) (unique argmax); true_diff ~ 0.3 N(0, 1); true in [0, 1), one frame longer."""
    B, t, H, W = shape
    n = B * t * H * W
    g = _gen(7000 + n % 9973)
    pd = ((torch.randperm(n, generator=g).double() - n // 2) / n).float().reshape(shape)
    td = 0.3 * torch.randn(shape, generator=g)
    tr = torch.rand((B, t + 1, H, W), generator=g)
    return pd, td, tr


def tdm_ref(pd, td, tr, beta, eps=TDM_EPS, gout=TDM_GOUT):
    """d = P - Q (pools), den = 1 + beta base + eps, w = 1 / den, term = d^2 w, loss = mean(term), coef = 2 d w / count.
    scale(w) = w + w (1 + beta |base| + eps) / |den|: the denominator's three operands, plus w.
    scale(coef) = 2 w (|P| + |Q|) / count + 2 |d| scale(w) / count + |coef|.
    scale(loss) = mean(2 |d| w (|P| + |Q|) + d^2 scale(w) + term) + |loss|.
    dpred = gout * coef at each window's argmax, summed where a pixel is the argmax of several windows:
    scale(dpred) = |gout| * (the same sum of scale(coef)) + |dpred|.
    Returns a dict; idx is torch's plane index of the argmax of pred_diff's windows."""
    pd64 = pd.double().requires_grad_(True)
    td, tr = td.double(), tr.double()
    P, idx = F.max_pool2d(pd64, 5, 4, 2, return_indices=True)
    Q, base = R.spatial_pool(td), R.spatial_pool(tr[:, :-1])
    den = 1.0 + beta * base + eps
    w = 1.0 / den
    d = P - Q
    term = d * d * w
    loss = term.mean()
    (dpred,) = torch.autograd.grad(loss * gout, pd64)
    count = term.numel()
    P, d = P.detach(), d.detach()
    sw = w + w * (1 + beta * base.abs() + eps) / den.abs()
    coef = 2 * d * w / count
    scoef = 2 * w * (P.abs() + Q.abs()) / count + 2 * d.abs() * sw / count + coef.abs()
    sloss = (2 * d.abs() * w * (P.abs() + Q.abs()) + d * d * sw + term.detach()).mean() + loss.detach().abs()
    H, W = pd.shape[-2:]
    flat = (torch.arange(P.shape[0] * P.shape[1], device=pd.device).reshape(P.shape[0], P.shape[1], 1, 1) * (H * W) + idx).reshape(-1)
    sd = torch.zeros(pd.numel(), dtype=torch.float64, device=pd.device).index_add_(0, flat, (scoef * abs(gout)).reshape(-1))
    return dict(loss=loss.detach(), sloss=sloss, coef=coef, scoef=scoef, idx=idx.int(), dpred=dpred, sdpred=sd.reshape(pd.shape) + dpred.abs())


# ================================================================ shock map and shock loss
SHOCK_SMALL = [2, 3, 4]
SHOCK_EXTRA = [(7, 31), (8, 32), (9, 33), (16, 64), (17, 65), (3, 33), (9, 2)]
SHOCK_POOLS = [1, 2, 3, 4]
SHOCK_BETAS = [0.02, 1.0, 30.0]
SHOCK_BORDERS = ["0", "1", "max"]
SHOCK_BT = [(1, 1), (2, 2)]
SHOCK_EPS = 1e-12
SHOCK_MANY_3x2 = (20, 15, 3, 2)                 # 300 planes
SHOCK_LIMIT_2x2 = (65535, 1, 2, 2)              # the blockIdx.z limit
SHOCK_OVER_LIMIT = (65536, 1, 2, 2)
SHOCK_SECOND_TRIP = (1, 9, 483, 483)            # 2,099,601 stored pixels through shock_gather_kernel
KINK_BAND = 1e-4
KINK_CAP = 0.01

ShockCase = namedtuple("ShockCase", "id bt hp wp pool beta border seed")


def shock_map_sizes():
    return [(h, w) for h in SHOCK_SMALL for w in SHOCK_SMALL] + SHOCK_EXTRA


def max_border(hp, wp):
    return (min(hp, wp) - 1) // 2


def _border(spec, hp, wp):
    return {"0": 0, "1": min(1, max_border(hp, wp)), "max": max_border(hp, wp)}[spec]


# id -> seed offset of a loss case whose inputs at offset 0 broke the kink cap (none does; test_loss_ext_cases_cpu.py asserts the cap)
SHOCK_RESEED = {}


def shock_loss_cases():
    """Two passes over the map sizes with the other lists cycled at different strides, then the special cases."""
    out = []
    sizes = shock_map_sizes()
    for rnd in range(2):
        for i, (hp, wp) in enumerate(sizes):
            k = i + rnd * len(sizes)
            pool = SHOCK_POOLS[(i + 2 * rnd) % 4]
            beta = SHOCK_BETAS[(i + i // 3 + rnd) % 3]
            bspec = SHOCK_BORDERS[(i // 2 + 2 * rnd + i) % 3]
            bt = SHOCK_BT[(i // 4 + i + rnd) % 2]
            border = _border(bspec, hp, wp)
            cid = f"{hp}x{wp}-p{pool}-b{beta:g}-m{border}-n{bt[0] * bt[1]}"
            out.append(ShockCase(cid, bt, hp, wp, pool, beta, border, SHOCK_RESEED.get(cid, 0) + 100 * k))
    out.append(ShockCase("300-planes-3x2", SHOCK_MANY_3x2[:2], 3, 2, 1, 30.0, 0, 0))
    out.append(ShockCase("65535-planes-2x2", SHOCK_LIMIT_2x2[:2], 2, 2, 1, 1.0, 0, 0))
    return out


def shock_map_cases():
    return [ShockCase(f"map-{hp}x{wp}-b{SHOCK_BETAS[i % 3]:g}", SHOCK_BT[i % 2], hp, wp, 1, SHOCK_BETAS[i % 3], 0, 50 + i)
            for i, (hp, wp) in enumerate(shock_map_sizes())]


def shock_stored(c):
    """Stored plane size: Hp pool + pool - 1, so the floor-mode pool drops pool - 1 trailing rows and columns."""
    return c.hp * c.pool + c.pool - 1, c.wp * c.pool + c.pool - 1


def shock_tiles(hp, wp):
    return -(-wp // STW), -(-hp // STH)


def shock_inputs(c, shape=None):
    """pred, true uniform in [0, 1) and a N(0, 1) upstream gradient of the loss tensor's shape (before kinks are zeroed)."""
    H, W = shock_stored(c)
    shape = shape or (c.bt[0], c.bt[1], H, W)
    g = _gen(8000 + c.seed + 31 * shape[2] + shape[3])
    pred, true = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    m = c.border
    dout = torch.randn((shape[0], shape[1], shape[2] // c.pool - 2 * m, shape[3] // c.pool - 2 * m), generator=g)
    return pred, true, dout


def _shift(p, dy, dx, h, w):
    return p[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def _stencils(x, absolute=False):
    """Sobel / 8, its transpose and the 5-point Laplacian under reflect padding; with `absolute` every weight in absolute value."""
    h, w = x.shape[-2:]
    p = F.pad(x.reshape(-1, 1, h, w), (1, 1, 1, 1), mode="reflect").reshape(x.shape[:-2] + (h + 2, w + 2))
    s = lambda dy, dx: _shift(p, dy, dx, h, w)            # noqa: E731
    sg = 1.0 if absolute else -1.0
    gx = ((s(-1, -1) + sg * s(-1, 1)) + 2.0 * (s(0, -1) + sg * s(0, 1)) + (s(1, -1) + sg * s(1, 1))) / 8.0
    gy = ((s(-1, -1) + sg * s(1, -1)) + 2.0 * (s(-1, 0) + sg * s(1, 0)) + (s(-1, 1) + sg * s(1, 1))) / 8.0
    lap = s(-1, 0) + s(0, -1) + s(0, 1) + s(1, 0) + sg * 4.0 * s(0, 0)
    return gx, gy, lap


def shock_parts(xp, beta, eps=SHOCK_EPS):
    """Float64 intermediates of the map of a (pooled) plane stack xp and the error scale of the map s = th gr:
    scale(s) = |s| + beta (1 - th^2) gr L + |th| (|gx| Sx + |gy| Sy) / gr, with L, Sx, Sy the Laplacian's and the two Sobel
    stencils applied to |xp| with their weights in absolute value (the sums of |w| |v| over the taps), th = tanh(beta lap),
    gr = sqrt(gx^2 + gy^2 + eps).  Also scale(th) = |th| + beta (1 - th^2) L and scale(gr) = gr + (|gx| Sx + |gy| Sy) / gr."""
    gx, gy, lap = _stencils(xp)
    Sx, Sy, L = _stencils(xp.detach().abs(), absolute=True)
    th, gr = torch.tanh(beta * lap), torch.sqrt(gx * gx + gy * gy + eps)
    s = th * gr
    d = dict(gx=gx, gy=gy, lap=lap, th=th, gr=gr, s=s, Sx=Sx, Sy=Sy, L=L)
    thd, grd, gxd, gyd = th.detach(), gr.detach(), gx.detach(), gy.detach()
    d["sth"] = thd.abs() + beta * (1 - thd * thd) * L
    d["sgr"] = grd + (gxd.abs() * Sx + gyd.abs() * Sy) / grd
    d["ss"] = s.detach().abs() + beta * (1 - thd * thd) * grd * L + thd.abs() * (gxd.abs() * Sx + gyd.abs() * Sy) / grd
    return d


def _shock_grad_scale(x64, xp, parts, g, beta):
    """Error scale of the gradient that the map's upstream gradient g sends to the stored pixels x64.  The kernels form, per map
    pixel, cgx = g th gx / gr, cgy = g th gy / gr, cl = g beta (1 - th^2) gr and apply the transposed stencils.
    scale(cgx) = 2 |cgx| + |g gx / gr| scale(th) + |g th / gr| Sx + |cgx| scale(gr) / gr  (operands g, th, gx, gr, plus |cgx|),
    scale(cgy) likewise, scale(cl) = 2 |cl| + 2 |g beta th gr| scale(th) + |g beta (1 - th^2)| scale(gr).
    scale(dx) = the transposed stencils with weights in absolute value applied to scale(c) + |c| (the sum's operands), routed
    through the pool to the argmax as the gradient is; the caller adds |dx|."""
    gx, gy, th, gr = (parts[k].detach() for k in ("gx", "gy", "th", "gr"))
    g = g.abs()
    cgx, cgy, cl = g * (th * gx / gr).abs(), g * (th * gy / gr).abs(), g * beta * (1 - th * th) * gr
    scx = 2 * cgx + g * (gx / gr).abs() * parts["sth"] + g * (th / gr).abs() * parts["Sx"] + cgx * parts["sgr"] / gr
    scy = 2 * cgy + g * (gy / gr).abs() * parts["sth"] + g * (th / gr).abs() * parts["Sy"] + cgy * parts["sgr"] / gr
    scl = 2 * cl + 2 * g * beta * (th * gr).abs() * parts["sth"] + g * beta * (1 - th * th) * parts["sgr"]
    ax, ay, al = _stencils(xp, absolute=True)
    (sc,) = torch.autograd.grad((ax * (scx + cgx) + ay * (scy + cgy) + al * (scl + cl)).sum(), x64)
    return sc


def shock_map_ref(x, dout, beta, eps=SHOCK_EPS):
    """(s, scale(s), dx, scale(dx)) of shock_map on the float32 plane stack x with upstream gradient dout."""
    x64 = x.double().requires_grad_(True)
    parts = shock_parts(x64, beta, eps)
    (dx,) = torch.autograd.grad((parts["s"] * dout.double()).sum(), x64, retain_graph=True)
    sdx = _shock_grad_scale(x64, x64, parts, dout.double(), beta) + dx.abs()
    return parts["s"].detach(), parts["ss"], dx, sdx


def shock_loss_ref(pred, true, dout, beta, pool, border, eps=SHOCK_EPS, zero_kinks=True):
    """The loss tensor relu(|s_t| - |s_p|) (cropped) with scale = scale(s_t) + scale(s_p) + |loss|, and its gradient to `pred` for
    the upstream gradient dout, which is first set to 0 (when zero_kinks) wherever | |s_t| - |s_p| | < 1e-4 max(|s_t|, |s_p|) or
    |beta lap_p| < 1e-4 max |beta lap_p| (maxima over the case), and at the map's corners, where the reflect padding makes
    gx = gy = 0 and |s| <= sqrt(eps): the relu and |s| at s_p = 0 make the gradient discontinuous there, and an element with
    dout = 0 contributes nothing on either side.  Returns a dict with the zeroed dout and the mask of
    zeroed elements as well."""
    p64 = pred.double().requires_grad_(True)
    t64 = true.double()
    pp, tp = (F.max_pool2d(p64, pool, pool), F.max_pool2d(t64, pool, pool)) if pool > 1 else (p64, t64)
    a, b = shock_parts(pp, beta, eps), shock_parts(tp, beta, eps)
    sp, st = a["s"], b["s"].detach()
    diff = st.abs() - sp.abs()
    m = border
    crop = lambda v: v[..., m:v.shape[-2] - m, m:v.shape[-1] - m] if m > 0 else v            # noqa: E731
    out = crop(F.relu(diff))
    sout = crop(a["ss"] + b["ss"]) + out.detach().abs()
    dd = diff.detach()
    finite = dd[torch.isfinite(dd)]
    smax = float(torch.maximum(st.abs(), sp.detach().abs())[torch.isfinite(dd)].max()) if finite.numel() else 0.0
    bl = (beta * a["lap"].detach()).abs()
    blmax = float(bl[torch.isfinite(bl)].max()) if bool(torch.isfinite(bl).any()) else 0.0
    hh, ww = sp.shape[-2:]
    cm = torch.zeros((hh, ww), dtype=torch.bool, device=pred.device)
    cm[0, 0] = cm[0, ww - 1] = cm[hh - 1, 0] = cm[hh - 1, ww - 1] = True
    corner = crop(cm.expand_as(sp))
    near = crop((dd.abs() < KINK_BAND * smax) | (bl < KINK_BAND * blmax)) | corner
    dz = dout.double().clone()
    if zero_kinks:
        dz[near] = 0.0
    gs = torch.zeros_like(sp)
    crop(gs).copy_(dz)
    gmap = torch.where(dd > 0, -gs * torch.sign(sp.detach()), torch.zeros_like(gs))
    gmap = torch.where(torch.isnan(dd), gs, gmap)                   # a NaN difference passes torch's relu backward: scale only
    (dx,) = torch.autograd.grad((out * dz).sum(), p64, retain_graph=True)
    sdx = _shock_grad_scale(p64, pp, a, gmap, beta) + dx.abs()
    return dict(out=out.detach(), sout=sout, dx=dx, sdx=sdx, dout=dz.float(), near=near, corner=corner)


def shock_zero_sets(c, shape):
    """Masks over the stored pixels where the loss's gradient is exactly 0 whatever the values: (dropped trailing rows / columns,
    pixels whose map pixel only the ignored border reads).  A map pixel is read by the outputs within distance 1 of it (the
    reflect padding maps -1 to 1 and n to n - 2, both next to the output that reads them)."""
    H, W = shape[-2:]
    dropped = torch.zeros((H, W), dtype=torch.bool)
    dropped[c.hp * c.pool:, :] = True
    dropped[:, c.wp * c.pool:] = True
    inside = torch.zeros((1, 1, c.hp, c.wp))
    m = c.border
    inside[..., m:c.hp - m, m:c.wp - m] = 1.0
    read = F.max_pool2d(inside, 3, 1, 1)[0, 0] > 0
    unread = ~read.repeat_interleave(c.pool, 0).repeat_interleave(c.pool, 1)
    border_only = torch.zeros((H, W), dtype=torch.bool)
    border_only[:c.hp * c.pool, :c.wp * c.pool] = unread
    return dropped, border_only


def pool_non_argmax(x, pool):
    """Mask over the stored pixels inside the pooled area that are not their pool window's (first) maximum; x on the CPU."""
    if pool == 1:
        return torch.zeros(x.shape, dtype=torch.bool)
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, pool, pool).sum().backward()
    hp, wp = x.shape[-2] // pool, x.shape[-1] // pool
    mask = x64.grad == 0
    mask[..., hp * pool:, :] = False
    mask[..., :, wp * pool:] = False
    return mask


# ================================================================ non-finite inputs
NAN = float("nan")
INF = float("inf")
NF_PLANE = (12, 12)               # three 5/4/2 windows per axis: rows 0-2, 2-6, 6-10
NF_CASES = [                      # (id, [(row, col, value)]) in plane 1 of a (1, 2, 12, 12) tensor
    ("nan-first", [(0, 0, NAN)]),                     # the first element the scan of window (0, 0) reads
    ("nan-interior", [(4, 4, NAN)]),                  # inside window (1, 1) only
    ("nan-last", [(10, 10, NAN)]),                    # the last element of window (2, 2)
    ("nan-shared", [(6, 6, NAN)]),                    # in windows (1, 1), (1, 2), (2, 1), (2, 2)
    ("nan-two", [(3, 3, NAN), (4, 5, NAN)]),          # two in window (1, 1): torch gives the argmax to the last, 4 * 12 + 5
    ("nan-two-pool2", [(4, 4, NAN), (5, 5, NAN)]),    # two in one 2 x 2 window of the shock loss's pool
    ("pos-inf", [(4, 4, INF)]),
    ("neg-inf", [(4, 4, -INF)]),
]


def nf_inputs(poison):
    g = _gen(9000)
    n = 2 * NF_PLANE[0] * NF_PLANE[1]
    x = ((torch.randperm(n, generator=g).double() - n // 2) / n).float().reshape((1, 2) + NF_PLANE) + 0.5
    for r, c, v in poison:
        x[0, 1, r, c] = v
    return x


def nf_reach(poison, pool, kind):
    """Stored pixels of plane 1 a NaN gradient may sit on.  kind "pool": the pixels of the 5/4/2 windows that hold a poisoned
    pixel.  kind "shock": poisoned map pixels, dilated by 1 (the outputs that read them) and by 1 again (the map pixels those
    outputs' stencils touch), then every stored pixel of those pool windows."""
    H, W = NF_PLANE
    m = torch.zeros((1, 1, H, W))
    for r, c, _ in poison:
        m[0, 0, r, c] = 1.0
    if kind == "pool":
        hit = F.max_pool2d(m, 5, 4, 2)
        back = torch.zeros((H, W), dtype=torch.bool)
        for oh in range(hit.shape[-2]):
            for ow in range(hit.shape[-1]):
                if hit[0, 0, oh, ow] > 0:
                    back[max(4 * oh - 2, 0):4 * oh + 3, max(4 * ow - 2, 0):4 * ow + 3] = True
        return back
    pm = F.max_pool2d(m, pool, pool) if pool > 1 else m
    pm = F.max_pool2d(F.max_pool2d(pm, 3, 1, 1), 3, 1, 1)[0, 0] > 0
    out = torch.zeros((H, W), dtype=torch.bool)
    up = pm.repeat_interleave(pool, 0).repeat_interleave(pool, 1)
    out[:up.shape[0], :up.shape[1]] = up
    return out


def same_nonfinite(got, ref):
    """NaN at the same places, and the same infinities."""
    got, ref = got.double().cpu(), ref.double().cpu()
    inf = lambda v: torch.where(torch.isinf(v), torch.sign(v), torch.zeros_like(v))           # noqa: E731
    return bool(torch.equal(torch.isnan(got), torch.isnan(ref))) and bool(torch.equal(inf(got), inf(ref)))


# ================================================================ the restatement in float32 on the CPU
def _f32(fn, inputs, g):
    out, grad = R.value_and_grad(fn, [t.numpy() for t in inputs], g.numpy() if torch.is_tensor(g) else g, torch.float32)
    return out, grad


def f32_errors():
    """max e_i of losses_ext_ref.py run in float32 on the CPU, per operation, over that operation's whole case table."""
    import numpy as np
    e = {k: 0.0 for k in F32_E}

    def up(key, got, ref, scale):
        e[key] = max(e[key], err(got, ref, scale))
    for n in elem_sizes():
        x, dy = transform_inputs(n)
        y, sy, dx, sdx = transform_ref(x, dy)
        out, grad = _f32(R.transform, [x], dy)
        up("transform_fwd", out, y, sy)
        up("transform_bwd", grad, dx, sdx)
        pred, true = wl1_inputs(n)
        loss, sloss, dp, sdp = wl1_ref(pred, true)
        out, grad = _f32(R.weighted_l1_distance, [pred, true], np.float32(WL1_GOUT))
        up("wl1_fwd", out, loss, sloss)
        up("wl1_bwd", grad, dp, sdp)
        p, q = kl_inputs(n)
        loss, sloss, dp, sdp = kl_ref(p, q)
        out, grad = _f32(R.kl_divergence, [p, q], np.float32(KL_GOUT))
        up("kl_fwd", out, loss, sloss)
        up("kl_bwd", grad, dp, sdp)
    for shape in softmax_shapes():
        x, dy = softmax_inputs(shape)
        y, sy, dx, sdx = softmax_ref(x, dy)
        out, grad = _f32(lambda t: R.softmax_temperature(t, TEMP), [x], dy)
        up("softmax_fwd", out, y, sy)
        up("softmax_bwd", grad, dx, sdx)
    for c in tdm_cases():
        pd, td, tr = tdm_inputs(c.shape)
        ref = tdm_ref(pd, td, tr, c.beta)
        pdr = pd.clone().requires_grad_(True)
        P = R.spatial_pool(pdr)
        P.retain_grad()
        d = P - R.spatial_pool(td)
        loss = (d * d / (1.0 + c.beta * R.spatial_pool(tr[:, :-1]) + TDM_EPS)).mean()
        (loss * TDM_GOUT).backward()
        up("tdm_loss", loss.detach(), ref["loss"], ref["sloss"])
        up("tdm_coef", P.grad / TDM_GOUT, ref["coef"], ref["scoef"])
        up("tdm_bwd", pdr.grad, ref["dpred"], ref["sdpred"])
    for c in shock_map_cases():
        x, _, dout = shock_inputs(c)
        s, ss, dx, sdx = shock_map_ref(x, dout, c.beta)
        out, grad = _f32(lambda t: R.shock_map(t, c.beta, SHOCK_EPS), [x], dout)
        up("shock_map_fwd", out, s, ss)
        up("shock_map_bwd", grad, dx, sdx)
    for c in shock_loss_cases() + [ShockCase("second-trip", SHOCK_SECOND_TRIP[:2], 483, 483, 1, 30.0, 0, 0)]:
        pred, true, dout = shock_inputs(c)
        ref = shock_loss_ref(pred, true, dout, c.beta, c.pool, c.border)
        out, grad = _f32(lambda a, b: R.shock_map_loss(a, b, beta=c.beta, border_ignore=c.border, pool=c.pool, eps=SHOCK_EPS),
                         [pred, true], ref["dout"])
        up("shock_loss_fwd", out, ref["out"], ref["sout"])
        up("shock_loss_bwd", grad, ref["dx"], ref["sdx"])
    return e
