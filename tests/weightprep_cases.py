"""Case tables, seeded input builders and exact restatements for the shape sweep of the weight-preparation kernels (csrc/weights.hip)
and of the bf16 weight split (wsplit_kernel / wsplit_batched_kernel of csrc/conv_x6c.hip): test_weightprep_gpu.py runs them on the
GPU, test_weightprep_cpu.py checks on the CPU that the tables have the properties the comparisons rely on (every sum an integer
below 2^24, every listed reason -- tile or generic kernel, second trip, ragged column and row groups -- true of its case, the
split exact on the case values).  Everything here is torch / numpy on the CPU and a function of the case alone; the restatements
follow the formulas of include/p2i_hip.h and oracle/p2i_oracle.py."""
import numpy as np
import torch

F64 = torch.float64
EXACT = 1 << 24            # integers of magnitude <= 2^24 are float32 values; sums of them in any order are exact below it


def pad32(n):
    return (n + 31) // 32 * 32


def ints(*shape, lo, hi, seed):
    """integer-valued float32 in [lo, hi]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def case_id(c):
    return "-".join(str(q) for q in c)


# ------------------------------------------------------------------------------------------------ DO-Conv fold
W_MAX, D_MAX, DD_MAX, G_MAX = 3, 2, 2, 3          # |W| <= 3, |D| <= 2, |integer D_diag| <= 2 (the identity: 1), |dwp| <= 3

# (O, I, groups, ksz, identity_rep, D_diag kind)
FOLD_CASES = [
    # tile kernels forward and backward (3x3, groups 1, O and I multiples of 32) with O != I: an O <-> I swap in a pitch shows
    (32, 64, 1, 3, 0, "eye"), (64, 32, 1, 3, 0, "eye"), (96, 32, 1, 3, 0, "eye"), (32, 160, 1, 3, 0, "eye"),
    (64, 32, 1, 3, 0, "int"),                      # an integer D_diag that is not the identity: D and D_diag are really ADDED
    # O % 32 == 0, I % 32 != 0: the tile kernels want whole 32 x 32 tiles, so forward (padded I) and backward both go generic --
    # fold_bwd_w_kernel reads a packed gradient whose pitch pad32(O) is O itself
    (32, 24, 1, 3, 0, "eye"), (64, 40, 1, 3, 0, "eye"),
    # generic kernels, groups 1, padded O and / or I
    (48, 16, 1, 3, 0, "eye"), (16, 48, 1, 3, 0, "eye"), (33, 65, 1, 3, 0, "eye"), (1, 8, 1, 3, 0, "eye"), (8, 1, 1, 3, 0, "eye"),
    # groups: the model's input layer (identity skip) and output layer (1x1), three groups, two groups 1x1
    (64, 16, 4, 3, 4, "eye"), (16, 64, 4, 1, 0, "eye"), (24, 12, 3, 3, 0, "eye"), (40, 8, 2, 1, 0, "eye"),
    (32, 8, 1, 3, 4, "eye"),                       # identity skip with groups 1: generic path although O % 32 == 0
    (288, 32, 1, 3, 0, "eye"),                     # nine 32-row trips of fold_bwd_d_batched_kernel's loop over O
    (288, 24, 1, 3, 0, "eye"),                     # O/g > 256, generic: the thread-stride loop of fold_bwd_d_kernel takes a second trip
]
# identity_rep asks for `+ x.repeat_interleave(rep, dim=1)`, which exists for I * rep == O and 3x3 only: anything else is refused
FOLD_REFUSED = [(12, 24, 3, 3, 1, "eye"), (16, 64, 4, 1, 4, "eye")]
FOLD_NO_D = [(64, 32, 1, 3, 0, "eye"), (33, 65, 1, 3, 0, "eye")]            # need_d=False: one tile case, one generic case

FOLD_BATCHED_SHAPES = [(32, 64), (64, 32), (96, 32), (128, 128)]
FOLD_BATCHED_N = [1, 3, 16]
FOLD_MAX_LAYERS = 16


def fold_fwd_is_tile(c):
    """the planner of p2i_doconv_fold_fwd, restated"""
    O, I, g, ksz, rep, _ = c
    return ksz == 3 and g == 1 and rep == 0 and O % 32 == 0 and I % 32 == 0


def fold_bwd_is_tile(c):
    """the planner of p2i_doconv_fold_bwd, restated"""
    O, I, g, ksz, _, _ = c
    return ksz == 3 and g == 1 and O % 32 == 0 and I % 32 == 0


def fold_inputs(c, seed=0):
    """W (O, I/g, nt), D, D_diag (I, 9, 9) or None, dwp (nt, I, pad32(O)).  dwp is filled EVERYWHERE -- padded columns and
    out-of-group entries included, as a dense weight gradient is -- and only its in-group entries may be read."""
    O, I, g, ksz, _, dd = c
    nt = ksz * ksz
    s = 1000 * seed + 7 * O + 3 * I + g
    W = ints(O, I // g, nt, lo=-W_MAX, hi=W_MAX, seed=s + 1)
    D = Dd = None
    if ksz == 3:
        D = ints(I, 9, 9, lo=-D_MAX, hi=D_MAX, seed=s + 2)
        Dd = torch.eye(9).reshape(1, 9, 9).repeat(I, 1, 1) if dd == "eye" else ints(I, 9, 9, lo=-DD_MAX, hi=DD_MAX, seed=s + 3)
    dwp = ints(nt, I, pad32(O), lo=-G_MAX, hi=G_MAX, seed=s + 4)
    return W, D, Dd, dwp


def fold_bounds(c):
    """largest magnitude any partial sum of the forward, of dW and of dD can reach"""
    O, I, g, ksz, rep, dd = c
    if ksz == 1:
        return W_MAX, G_MAX, 0
    dm = D_MAX + (1 if dd == "eye" else DD_MAX)
    return 9 * dm * W_MAX + (1 if rep else 0), 9 * G_MAX * dm, (O // g) * G_MAX * W_MAX


def fold_expected(c, W, D, Dd, dwp):
    """(wp_f, wp_d, dW, dD) in float32 from a float64 restatement (every value an integer: exact)."""
    O, I, g, ksz, rep, _ = c
    nt, Ig, Og = ksz * ksz, I // g, O // g
    if ksz == 3:
        Dm = (D + Dd).to(F64)
        Wr = W.to(F64).reshape(Og, I, 9)
        dow = torch.einsum("ims,ois->oim", Dm, Wr).reshape(O, Ig, 9)          # the reference's memory reinterpretation
    else:
        dow = W.to(F64).reshape(O, Ig, 1)
    dense = torch.zeros(O, I, nt, dtype=F64)
    gdense = dwp[:, :, :O].to(F64).permute(2, 1, 0)                            # (O, I, nt)
    ddow = torch.zeros(O, Ig, nt, dtype=F64)
    for o in range(O):
        lo = (o // Og) * Ig
        dense[o, lo:lo + Ig] = dow[o]
        ddow[o] = gdense[o, lo:lo + Ig]
        if rep:
            dense[o, o // rep, 4] += 1.0                                       # + x.repeat_interleave(rep, dim=1)
    wp_f = torch.zeros(nt, I, pad32(O), dtype=F64)
    wp_f[:, :, :O] = dense.permute(2, 1, 0)
    wp_d = torch.zeros(nt, O, pad32(I), dtype=F64)
    wp_d[:, :, :I] = dense.permute(2, 0, 1)
    if ksz == 3:
        dd_ = ddow.reshape(Og, I, 9)
        dW = torch.einsum("oim,ims->ois", dd_, Dm).reshape(O, Ig, 9)
        dD = torch.einsum("oim,ois->ims", dd_, Wr)
    else:
        dW, dD = ddow.reshape(O, Ig, 1), None
    return wp_f.float(), wp_d.float(), dW.float(), (None if dD is None else dD.float())


# ------------------------------------------------------------------------------------------------ pack / unpack
PACK_SHAPES = [(1, 1, 1), (1, 128, 1), (33, 5, 9), (32, 1, 27), (20, 40, 27), (64, 16, 9), (65, 33, 4)]     # (O, I, ntaps)
PACK_SIGMAS = [None, 2.0, 0.5]             # division by a power of two is exact
PACK_W_MAX = 50
SN_UNPACK_SHAPES = [(33, 5, 9), (20, 40, 27), (1, 128, 1)]
PACK_MAX_LAYERS = 16


def pack_weight(shape, seed=0):
    return ints(*shape, lo=-PACK_W_MAX, hi=PACK_W_MAX, seed=100 * seed + sum(shape))


def pack_expected(w, sigma):
    O, I, nt = w.shape
    v = w.to(F64) / (1.0 if sigma is None else sigma)
    f = torch.zeros(nt, I, pad32(O), dtype=F64)
    f[:, :, :O] = v.permute(2, 1, 0)
    d = torch.zeros(nt, O, pad32(I), dtype=F64)
    d[:, :, :I] = v.permute(2, 0, 1)
    return f.float(), d.float()


def packed_grad(shape, seed, garbage):
    """integer packed gradient (nt, I, pad32(O)); the padded columns hold `garbage` (non-zero), which no unpack may read"""
    O, I, nt = shape
    g = torch.full((nt, I, pad32(O)), float(garbage))
    g[:, :, :O] = ints(nt, I, O, lo=-PACK_W_MAX, hi=PACK_W_MAX, seed=200 * seed + sum(shape))
    return g


def unpack_expected(g, O):
    return g[:, :, :O].permute(2, 1, 0).contiguous()


def sn_unpack_inputs(shape, seed=0):
    """float data for the spectral-norm unpack: w, unit u and v, sigma = u^T W v rounded to float32, a packed gradient"""
    O, I, nt = shape
    s = 300 * seed + sum(shape)
    w = rand(O, I, nt, seed=s + 1, scale=0.1)
    u = torch.nn.functional.normalize(rand(O, seed=s + 2), dim=0)
    v = torch.nn.functional.normalize(rand(I * nt, seed=s + 3), dim=0)
    sigma = torch.dot(u.to(F64), torch.mv(w.to(F64).reshape(O, -1), v.to(F64))).float().reshape(1)
    g = torch.full((nt, I, pad32(O)), 7.0)
    g[:, :, :O] = rand(nt, I, O, seed=s + 4)
    return w, u, v, sigma, g


def sn_unpack_expected(w, u, v, g):
    """float64 autograd through oracle.spectral_norm_weight (eval mode: u, v as stored)"""
    from oracle import p2i_oracle as orc
    O = w.shape[0]
    p = {"l.weight_orig": w.to(F64).requires_grad_(True), "l.weight_u": u.to(F64), "l.weight_v": v.to(F64)}
    wn = orc.spectral_norm_weight(p, "l", False)
    wn.backward(unpack_expected(g, O).to(F64))
    return p["l.weight_orig"].grad


# ------------------------------------------------------------------------------------------------ bf16 split
SPLIT_SHAPES = [(1, 8, 32), (9, 16, 64), (27, 24, 32), (9, 64, 96)]          # (ntaps, K, Mpad)
SPLIT_STRIDE_SHAPE = (27, 512, 320)          # 27 * 64 * 320 = 552 960 16-byte units > 2048 * 256: wsplit_kernel grid-strides
SPLIT_GRID_UNITS = 2048 * 256                # wsplit_kernel: at most 2048 workgroups of 256 threads, one unit per thread and trip
SPLIT_BATCH_MAX = 24
SPLIT_EXP = 60                               # exponents in [-60, 60]: the split is exact (no term is subnormal)


def split_units(shape):
    ntaps, K, Mpad = shape
    return ntaps * (K // 8) * Mpad


def split_values(shape, seed=0):
    """float32 (ntaps, K, Mpad): random sign, mantissa and exponent in [-60, 60]; the first entries are +-0, +-1 and numbers with
    only the LAST mantissa bit set below the leading one (1 + 2^-23: the mid plane carries that bit; 1 + 2^-15 + 2^-23: the lo plane
    does).  No subnormal, NaN or Inf."""
    n = int(np.prod(shape))
    rng = np.random.default_rng(1000 + seed + n)
    sign = rng.integers(0, 2, n, dtype=np.uint32) << 31
    expo = rng.integers(127 - SPLIT_EXP, 127 + SPLIT_EXP + 1, n, dtype=np.uint32) << 23
    mant = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    bits = sign | expo | mant
    special = np.array([0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x3F800001, 0xBF800001, 0x3F800101,
                        ((127 + SPLIT_EXP) << 23) | 1, ((127 - SPLIT_EXP) << 23) | 1], dtype=np.uint32)
    bits[:len(special)] = special
    return bits.view(np.float32).reshape(shape)


def split_terms(a):
    """(hi, mid, lo) float32: each term is the remainder truncated to its upper 16 bits"""
    m = np.uint32(0xFFFF0000)
    hi = (a.view(np.uint32) & m).view(np.float32)
    r = a - hi
    mid = (r.view(np.uint32) & m).view(np.float32)
    s = r - mid
    lo = (s.view(np.uint32) & m).view(np.float32)
    return hi, mid, lo


def split_image(a):
    """uint16 image Wb[plane][tap][k/8][m][k%8] of a packed tensor a[tap][k][m], flat"""
    ntaps, K, Mpad = a.shape
    planes = np.stack(split_terms(np.ascontiguousarray(a)))                   # (3, ntaps, K, Mpad)
    h = (planes.view(np.uint32) >> 16).astype(np.uint16)
    return np.ascontiguousarray(h.reshape(3, ntaps, K // 8, 8, Mpad).transpose(0, 1, 2, 4, 3)).reshape(-1)


# ------------------------------------------------------------------------------------------------ spectral norm
SN_SHAPES = [(1, 1), (5, 3), (33, 27), (40, 65), (70, 64), (1030, 8), (8, 1030), (3, 4100)]     # (O, K)
SN_ZERO_SHAPE = (16, 27)
SN_MAX_LAYERS = 16
SN_WTU_COLS = 64           # sn_wtu_batched_kernel: a workgroup owns 64 columns of W^T u (ceil(K / 64) workgroups per layer) ...
SN_WTU_ROW_GROUPS = 4      # ... and its 4 row groups stride over ALL rows o = rg, rg + 4, ...: one fixed order, nothing atomic
SN_NORM_THREADS = 1024     # sn_finish_batched_kernel: one workgroup of 1024 threads per layer strides over the vector


def sn_inputs(shape, seed=0):
    O, K = shape
    s = 400 * seed + 3 * O + K
    w = rand(O, K, seed=s + 1, scale=0.1)
    u = torch.nn.functional.normalize(rand(O, seed=s + 2), dim=0)
    v = torch.nn.functional.normalize(rand(K, seed=s + 3), dim=0)
    return w, u, v


def sn_expected(w, u, v, training):
    """(u, v, sigma) in float64 after oracle.spectral_norm_weight"""
    from oracle import p2i_oracle as orc
    p = {"l.weight_orig": w.to(F64), "l.weight_u": u.to(F64).clone(), "l.weight_v": v.to(F64).clone()}
    if not bool((w != 0).any()):
        # sigma = 0: weight / sigma is not asked for; the power iteration itself (the oracle's lines, eps = 1e-12)
        wm = p["l.weight_orig"]
        vn = torch.nn.functional.normalize(torch.mv(wm.t(), p["l.weight_u"]), dim=0, eps=1e-12)
        un = torch.nn.functional.normalize(torch.mv(wm, vn), dim=0, eps=1e-12)
        return un, vn, torch.dot(un, torch.mv(wm, vn))
    wn = orc.spectral_norm_weight(p, "l", training)
    un, vn = p["l.weight_u"], p["l.weight_v"]
    sigma = torch.dot(un, torch.mv(p["l.weight_orig"], vn))
    assert torch.allclose(wn * sigma, p["l.weight_orig"], rtol=1e-12, atol=0)
    return un, vn, sigma
