"""Case table, seeded inputs and CPU references of the regime sweep of the gauge-point IDW (csrc/idw.hip): whole-frame masks (the
loader's `nowcasting`, `fi` and `stin` types, data/sti_dataset.py create_mask), odd and non-square grids, the replay without its LDS
copy.  test_idw_regimes_gpu.py runs the cases on the GPU, test_idw_cases_cpu.py checks on the CPU that every case has the sizes it
is there for.  Everything here is torch / numpy on the CPU and a function of the case alone; nothing is taken from the kernels'
output except where a function says so (the backward reference scatters over the selection it is handed).

Masks follow create_mask's rules, restated so that nothing depends on numpy's global generator:
  ("now", keep)          ones, mask[keep:] = 0
  ("fi", stride)         zeros, mask[0:T:stride] = 1  -- create_mask writes mask[0:T:step+1] with step drawn from interval = (2, 5),
                         so the loader's strides are 3 and 6; "fi step 3" below is stride 3 (frames 0, 3, 6, ...)
  ("stin", keep, block)  frames < keep full, every other frame the SAME block mask: one random pixel per block x block cell
                         (_sti_matrix's rule, drawn from a seeded RandomState)
  ("shared", n)          n random pixels, the same in every frame (a gauge mask)

Every sample has N >= 256 points: oracle/idw_knn.c models torch.topk's partial-sort branch only."""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import p2i_oracle as orc

Case = namedtuple("Case", "id B T H W samples seed")

IDW_RW_PCAP = 3072        # points of idw_replay_lane_kernel's LDS copy
IDW_LDS_PTS = 8192        # points of the backward kernels' LDS accumulators
LDS_BYTES = 64 * 1024
U = 2.0 ** -24            # unit roundoff of float32


def cases():
    return [
        Case("sq32", 4, 16, 32, 32, (("now", 4), ("fi", 6), ("fi", 3), ("stin", 4, 4)), 101),
        Case("rect", 2, 16, 24, 40, (("now", 4), ("stin", 4, 4)), 102),
        Case("odd", 2, 8, 9, 11, (("now", 4), ("fi", 3)), 103),
        Case("long", 1, 32, 16, 16, (("now", 4),), 104),
        Case("tall", 1, 32, 128, 4, (("shared", 64),), 105),
        Case("big48", 1, 16, 48, 48, (("fi", 3),), 106),
    ]


def by_id(cid):
    return {c.id: c for c in cases()}[cid]


def replay_lds_bytes(c):
    """Dynamic LDS idw_fwd_impl asks for the lane-per-voxel replay: the point copy and the row starts (above 64 KiB: none, global)."""
    return 16 * IDW_RW_PCAP + 4 * c.T * (c.H + 1)


def _block_matrix(rs, H, W, block):
    hh, ww = np.meshgrid(np.arange(0, H, block), np.arange(0, W, block), indexing="ij")
    m = np.zeros((H, W), dtype=np.float32)
    for h0, w0 in zip(hh.ravel(), ww.ravel()):
        m[rs.randint(h0, min(h0 + block, H)), rs.randint(w0, min(w0 + block, W))] = 1.0
    return m


def masks(c):
    """(B, T, H, W) float32, 1 = observed."""
    rs = np.random.RandomState(c.seed)
    out = torch.zeros(c.B, c.T, c.H, c.W)
    for b, spec in enumerate(c.samples):
        if spec[0] == "now":
            out[b, :spec[1]] = 1.0
        elif spec[0] == "fi":
            out[b, 0:c.T:spec[1]] = 1.0
        elif spec[0] == "stin":
            out[b] = torch.from_numpy(_block_matrix(rs, c.H, c.W, spec[2]))
            out[b, :spec[1]] = 1.0
        elif spec[0] == "shared":
            m = np.zeros(c.H * c.W, dtype=np.float32)
            m[rs.permutation(c.H * c.W)[:spec[1]]] = 1.0
            out[b] = torch.from_numpy(m.reshape(c.H, c.W))
        else:
            raise ValueError(spec)
    return out


def values(c):
    """|randn|, as the existing IDW tests draw them."""
    g = torch.Generator().manual_seed(c.seed)
    return torch.randn(c.B, c.T, c.H, c.W, generator=g).float().abs()


def point_counts(c):
    return [int(n) for n in (masks(c) > 0).flatten(1).sum(1)]


def point_positions(c, b):
    """Flat (t, y, x) indices of sample b's points, in the reference's nonzero() order."""
    return torch.nonzero(masks(c)[b].flatten() > 0).flatten()


# ------------------------------------------------------------------------------------------------ forward reference
Forward = namedtuple("Forward", "sel d W R A")


@functools.lru_cache(maxsize=None)
def forward_reference(cid):
    """Per sample: sel (Q, 4) int64 and d (Q, 4) float32 of oracle.idw_select_c (ascending distance), then from THOSE float32
    distances in float64, with float32(tau): inv = 1 / (d + tau), w = inv^2, W = w / (sum w + 1e-12), R = sum v_k W_k and
    A = sum |v_k| W_k (the scale of the output's rounding bound).  Computed once per process, shared by every test, never written."""
    c = by_id(cid)
    mk, vals = masks(c), values(c)
    tau = float(np.float32(orc.IDW_TAU))
    res = []
    for b in range(c.B):
        tz, ty, tx, pts = orc.mask_points(mk[b])
        sel, d = orc.idw_select_c(pts, (c.T, c.H, c.W))
        inv = 1.0 / (d.double() + tau)
        w = inv * inv
        Wn = w / (w.sum(1, keepdim=True) + 1e-12)
        v = vals[b][tz, ty, tx].double()[sel]
        res.append(Forward(sel, d, Wn, (v * Wn).sum(1), (v.abs() * Wn).sum(1)))
    return tuple(res)


# ------------------------------------------------------------------------------------------------ backward reference
def backward_reference(dout, pt_pos, pt_count, sel_idx, sel_w):
    """dout (B, Q) float32, pt_pos (B, Q), pt_count (B,), sel_idx / sel_w (B, Q, 4): numpy arrays, the selection and weights as the
    forward SAVED them (the device's, once they have been checked against the oracle: this isolates the accumulation).
    Returns (S, C, n), each (B, Q) float64 in voxel slots: S the float64 scatter-add of float64(float32(g * w)), C the sum of the
    contributions' absolute values, n their number (voxels with g == 0 contribute nothing, as in the kernels).  numpy's IEEE
    arithmetic: a NaN / Inf in dout reaches exactly the four selected points of its voxel, like the reference's autograd."""
    B, Q = dout.shape
    S, C, n = (np.zeros((B, Q), dtype=np.float64) for _ in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            N = int(pt_count[b])
            if N < 4:
                continue
            live = dout[b] != 0                                             # (NaN != 0 is True)
            c32 = dout[b][live].astype(np.float32)[:, None] * sel_w[b][live].astype(np.float32)
            idx = sel_idx[b][live].astype(np.int64).ravel()
            c64 = c32.astype(np.float64).ravel()
            pos = pt_pos[b][:N].astype(np.int64)
            S[b, pos] = np.bincount(idx, weights=c64, minlength=N)
            C[b, pos] = np.bincount(idx, weights=np.abs(c64), minlength=N)
            n[b, pos] = np.bincount(idx, minlength=N)
    return S, C, n


def fix_exp(max_abs_dout, Q):
    """idw_fix_exp of csrc/idw.hip: the fixed-point scale is 2^k, from the float32 exponent of the call's largest finite |dout|."""
    m = np.float32(max_abs_dout)
    if m == 0:
        return 0
    e = int((m.view(np.uint32) >> 23) & 0xff) - 127
    lq = 2
    while (1 << lq) < 4 * Q:
        lq += 1
    return max(-120, min(120, 61 - (e + 1) - lq))


def dout(c, seed_offset=1):
    """Seeded normal upstream gradient with about 10 % exact zeros (the kernels skip g == 0)."""
    g = torch.Generator().manual_seed(c.seed + 1000 * seed_offset)
    d = torch.randn(c.B, c.T, c.H, c.W, generator=g).float()
    return d * (torch.rand(c.B, c.T, c.H, c.W, generator=g) >= 0.1).float()


# ------------------------------------------------------------------------------------------------ tie statistics
@functools.lru_cache(maxsize=None)
def tie_shares(cid):
    """Per sample (share of voxels pass 1 lists: d4 == d5, share IDW_CONSIDER_FIXED cannot decide), from a float32 restatement of the
    kernel's distance chain: the products of each fma are formed in float64 (exact) and the sum rounded to float64, then to float32
    -- a double rounding that can differ from fmaf in a few voxels.  These numbers only show that a case reaches its path; values are
    judged by the C oracle.  Rule of the second share (csrc/idw.hip): with D the 4th distance and S the points with d <= D in index
    order, the voxel is undecided when a member with d < D follows the first four of S and two or more of those four have d == D."""
    c = by_id(cid)
    mk = masks(c)
    gx, gy, gz = (torch.linspace(0, 1, n) for n in (c.W, c.H, c.T))
    Q = c.T * c.H * c.W
    q = torch.arange(Q)
    qz, qy, qx = gz[q // (c.H * c.W)], gy[(q // c.W) % c.H], gx[q % c.W]
    a0, a1, a2 = -2.0 * qx, -2.0 * qy, -2.0 * qz
    n1 = (qx * qx + qy * qy) + qz * qz
    res = []
    for b in range(c.B):
        _, _, _, pts = orc.mask_points(mk[b])
        px, py, pz = pts[:, 0].contiguous(), pts[:, 1].contiguous(), pts[:, 2].contiguous()
        pn = (px * px + py * py) + pz * pz
        N = pts.shape[0]
        rows = max(1, (1 << 22) // N)
        listed = undecided = 0
        for s in range(0, Q, rows):
            e = min(Q, s + rows)
            acc = a0[s:e, None] * px[None, :]
            acc = (a1[s:e, None].double() * py[None, :].double() + acc.double()).float()
            acc = (a2[s:e, None].double() * pz[None, :].double() + acc.double()).float()
            acc = acc + n1[s:e, None]
            acc = acc + pn[None, :]
            d = acc.clamp_min_(0).sqrt_()
            d5 = torch.topk(d, 5, dim=1, largest=False, sorted=True).values
            tied = d5[:, 3] == d5[:, 4]
            listed += int(tied.sum())
            if bool(tied.any()):
                dt, D = d[tied], d5[tied, 3:4]
                le = dt <= D
                first4 = le & (le.cumsum(1, dtype=torch.int32) <= 4)
                later_lt = (dt < D) & ~first4
                nd = (first4 & (dt == D)).sum(1)
                undecided += int((later_lt.any(1) & (nd >= 2)).sum())
        res.append((listed / Q, undecided / Q))
    return tuple(res)
