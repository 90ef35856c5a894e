"""Case tables and seeded input builders of the edge-shape tests of the glue / loss kernels (csrc/glue.hip, csrc/loss.hip):
test_glue_edges_gpu.py runs them on the GPU against float64 torch, test_glue_cases_cpu.py checks on the CPU that the inputs have
the properties the comparisons rely on (margins around every kink, tied pooling windows, the placed gradient masks).  Everything
here is float32 torch on the CPU, a function of the case alone."""
import torch
import torch.nn.functional as F

KINK_MARGIN = 0.01        # distance of every constructed value from the kink of its activation / hinge
ATTN_MARGIN = 1e-4        # smallest |pre-ReLU value| an attention case may hold at a pixel with a gradient

ACTS = ("none", "relu", "leaky", "tanh")


def rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def kinked(*shape, seed, scale=1.0):
    """randn pushed away from 0 by KINK_MARGIN: v + sign(v) * 0.01, an exact 0 (randn draws some in a few million) counted as
    positive.  The margin comes from the construction, nothing is filtered."""
    v = rand(*shape, seed=seed, scale=scale)
    return torch.where(v >= 0, v + KINK_MARGIN, v - KINK_MARGIN)


def act_torch(v, act):
    return {"none": lambda t: t, "relu": F.relu, "leaky": lambda t: F.leaky_relu(t, 0.2), "tanh": torch.tanh}[act](v)


def case_id(*parts):
    return "-".join("x".join(str(q) for q in p) if isinstance(p, (tuple, list)) else str(p) for p in parts)


# ------------------------------------------------------------------------------------------------ discriminator tail
DTAIL_B = 2
# (H2, W2, T3, H3, W3).  2 H3 - 1 = H2 (any clip height = 4 mod 8: 36 -> 9 / 5, 100 -> 25 / 13) in one or both axes, ratio 1.5 and 3,
# the 1 x 1 maps, an integer ratio with a non-square map, and n = 2 * 96 * 96 = 18 432 > 64 * 256: a second grid-stride trip of
# dtail_bwd2_kernel
DTAIL_CASES = [(9, 9, 2, 5, 5), (13, 7, 3, 7, 4), (25, 25, 2, 13, 13), (5, 3, 2, 3, 2), (3, 3, 1, 2, 2), (2, 2, 1, 1, 1), (1, 1, 2, 1, 1),
               (10, 6, 2, 5, 3), (96, 96, 1, 48, 48)]


def dtail_inputs(dims):
    H2, W2, T3, H3, W3 = dims
    return dict(o2=rand(DTAIL_B, 1, H2, W2, seed=1), o3=rand(DTAIL_B, 1, T3, H3, W3, seed=2), alpha=torch.tensor([0.3]),
                gout=rand(DTAIL_B, H2 * W2, seed=3))


DISC_CLIP = (2, 16, 1, 36, 28)          # P2IDiscriminator on a clip with H = 4 mod 8 and W = 4 mod 8: the tail sees 9 x 7 against 5 x 4


# ------------------------------------------------------------------------------------------------ attention
ATTN_CHUNK = 256


def attn_grid_x(B, HW):
    """workgroups per sample of attn_bwd_kernel (p2i_attn_bwd): 64 workgroups in all, at most one per 256-pixel chunk."""
    nchunk = -(-HW // ATTN_CHUNK)
    return min(nchunk, max(64 // min(B, 64), 1))


# (B, HW) -> {(sample, chunk): pixels with a gradient}; every other chunk has none.
#   2 x 255/256/257: the partial chunk, the full one, a second chunk of one pixel.
#   16 x 1297: 6 chunks on 4 workgroups per sample (workgroups 0 and 1 walk chunks (0, 4) and (1, 5)), the last chunk holds 17 pixels.
#   64 x 300, 70 x 300: one workgroup per sample walks both chunks.
#   64 x 700: one workgroup walks three chunks -- the middle one without any gradient between two that have some.
ATTN_PLANS = {
    (2, 255): {(0, 0): 33, (1, 0): 255},
    (2, 256): {(0, 0): 32, (1, 0): 256},
    (2, 257): {(0, 0): 33, (0, 1): 1, (1, 0): 256},
    (16, 1297): {(0, 0): 32, (0, 4): 33, (0, 1): 1, (0, 5): 17, (7, 4): 5, (7, 1): 256, (15, 2): 1},
    (64, 300): {(0, 0): 256, (0, 1): 44, (31, 1): 1, (63, 0): 32},
    (70, 300): {(0, 0): 256, (0, 1): 44, (31, 1): 1, (63, 0): 32, (69, 0): 33, (69, 1): 3},
    (64, 700): {(0, 0): 1, (0, 2): 33, (5, 1): 2, (63, 0): 32, (63, 2): 188},
}
ATTN_CASES = [(B, HW, T) for (B, HW) in ATTN_PLANS for T in (8, 16, 32)]


def attn_id(case):
    return "B%d-HW%d-T%d" % case


# seeds for which every case keeps ATTN_MARGIN (test_glue_cases_cpu.py), found by counting up from 0: the first one does for all
ATTN_SEEDS = {attn_id(c): 0 for c in ATTN_CASES}


def attn_inputs(case, seed=None):
    """x of both signs, the two layers' parameters, and a gradient that is non-zero exactly at the planned pixels; the first planned
    pixel of every sample has a gradient in ONE frame only."""
    B, HW, T = case
    seed = ATTN_SEEDS[attn_id(case)] if seed is None else seed
    s = 1000 * seed
    x = rand(B, T, 1, HW, seed=s + 1)
    x = x + torch.sign(x) * 0.25                                     # both signs, none close to 0
    ws = 0.25 / T ** 0.5                                             # the gate's spread (about 0.3) does not grow with T: 1 + gate = 0 stays rare
    w0, b0 = rand(T, T, 1, seed=s + 2, scale=ws), rand(T, seed=s + 3, scale=0.1)
    w1, b1 = rand(T, T, 1, seed=s + 4, scale=ws), rand(T, seed=s + 5, scale=0.1)
    g = torch.Generator().manual_seed(s + 6)
    active = torch.zeros(B, HW, dtype=torch.bool)
    single = []
    for (b, c), n in sorted(ATTN_PLANS[(B, HW)].items()):
        lo, size = c * ATTN_CHUNK, min(ATTN_CHUNK, HW - c * ATTN_CHUNK)
        pix = lo + torch.randperm(size, generator=g)[:n].sort().values
        active[b, pix] = True
    gout = rand(B, T, 1, HW, seed=s + 7) * active.view(B, 1, 1, HW)
    for b in range(B):
        idx = torch.nonzero(active[b])
        if idx.numel():
            p, t = int(idx[0]), (b * 5 + 3) % T
            keep = gout[b, t, 0, p].clone()
            gout[b, :, 0, p] = 0
            gout[b, t, 0, p] = keep
            single.append((b, p, t))
    return dict(x=x, w0=w0, b0=b0, w1=w1, b1=b1, gout=gout, active=active, single=single)


def attn_reference(inp, dtype=torch.float64):
    """Both AttentionBlocks through the oracle in `dtype`: output (B, T, 1, HW), the four parameter gradients, and the pre-ReLU
    values (layer, B, HW, T) the margin is measured on."""
    from oracle import p2i_oracle as orc
    x = inp["x"].to(dtype)
    B, T, _, HW = x.shape
    ps = [inp[k].to(dtype).requires_grad_(True) for k in ("w0", "b0", "w1", "b1")]
    xs = x.permute(0, 2, 3, 1).contiguous().view(B * HW, T, 1)
    h1 = orc.attention_block(xs, ps[0], ps[1])
    h2 = orc.attention_block(h1, ps[2], ps[3])
    out = h2.view(B, 1, HW, T).permute(0, 3, 1, 2)
    out.backward(inp["gout"].to(dtype))
    with torch.no_grad():
        pre1 = xs + xs * F.conv1d(xs, ps[0], ps[1])
        pre2 = h1 + h1 * F.conv1d(h1, ps[2], ps[3])
    return out.detach(), [p.grad for p in ps], torch.stack([pre1.view(B, HW, T), pre2.view(B, HW, T)]), \
        torch.stack([xs.view(B, HW, T), h1.detach().view(B, HW, T)])


def attn_margin(inp):
    """min |pre-ReLU value| of both layers over the pixels with a gradient, in float64.  An element whose layer input is exactly 0
    (the first layer's ReLU cut it) has the pre-ReLU value h + h g = 0 in every precision -- no rounding can move it across the
    kink, and both sides give it the gradient 0 -- so it does not count."""
    _, _, pre, hin = attn_reference(inp)
    m = inp["active"].unsqueeze(0).unsqueeze(-1) & (hin != 0)
    return float(pre.abs()[m.expand_as(pre)].min())


# ------------------------------------------------------------------------------------------------ pool + duplicate
POOLDUP_CASES = [(1, 1, 2, 2), (3, 5, 6, 10), (2, 3, 4, 2), (2, 8, 14, 6)]
POOLDUP_BIG = (2, 64, 256, 260)          # 2 129 920 outputs > 8192 * 256: the grid-stride loops take a second trip


POOLDUP_SEEDS = {(1, 1, 2, 2): 10}        # the first seed that ties the only window; every other case has ties at seed 0


def pooldup_inputs(shape):
    """relu(randn): half of the inputs are exactly 0, so one window in sixteen is all zeros -- a tied maximum."""
    B, C, H, W = shape
    return dict(x=F.relu(rand(B, C, H, W, seed=POOLDUP_SEEDS.get(tuple(shape), 0))), gout=rand(B, 2 * C, H // 2, W // 2, seed=2))


def pooldup_tied_windows(x):
    """number of 2 x 2 windows whose maximum is reached more than once"""
    B, C, H, W = x.shape
    win = x.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    return int(((win == win.max(dim=-1, keepdim=True).values).sum(dim=-1) > 1).sum())


def pooldup_all_ties():
    """(1, 1, 6, 10): 15 windows, window k holds the maximum at the positions of the set bits of k + 1 (scan order: bit 0 = top left,
    1 = top right, 2 = bottom left, 3 = bottom right) -- every way a window can tie, and the four untied ones."""
    x = torch.zeros(1, 1, 6, 10)
    for k in range(15):
        wy, wx = divmod(k, 5)
        for bit in range(4):
            if (k + 1) >> bit & 1:
                x[0, 0, 2 * wy + bit // 2, 2 * wx + bit % 2] = 1.0
    return dict(x=x, gout=rand(1, 2, 3, 5, seed=3))


# ------------------------------------------------------------------------------------------------ upsample + modulate
UPMOD_SIZES = [(1, 1), (1, 4), (4, 1), (3, 5), (7, 9), (16, 24)]
UPMOD_BC = [(1, 1), (3, 5), (2, 9)]
UPMOD_CASES = [(B, C, Sh, Sw) for (Sh, Sw) in UPMOD_SIZES for (B, C) in UPMOD_BC]


def upmod_inputs(case):
    B, C, Sh, Sw = case
    pos = rand(1, 1, 2 * Sh, 2 * Sw, seed=2, scale=0.5)
    pos.view(-1)[0], pos.view(-1)[-1] = 20.0, -20.0                  # saturated sigmoid, both ends
    return dict(x=rand(B, C, Sh, Sw, seed=1), pos=pos, bias=rand(C, seed=4, scale=0.3), gout=rand(B, C, 2 * Sh, 2 * Sw, seed=3))


# ------------------------------------------------------------------------------------------------ bias / activation gradients
# inner -> its 4-D and 5-D factorisations.  (3, 8200): two bias_grad chunks (3 * 8200 = 24 600 > 16 384) whose boundary, 12 300, falls
# inside sample 1, and two act_bwd_bias chunks (2050 float4 > 2048); inner = 7 and 1: the inner % 4 fallback of act_bwd_bias.
BIAS_INNER = {7: ((7, 1), (1, 7, 1)), 1: ((1, 1), (1, 1, 1)), 8200: ((8, 1025), (2, 4, 1025)), 9216: ((96, 96), (4, 48, 48))}
BIAS_CASES = [(B, C, inner, nd) for C in (1, 3) for (B, inner) in ((2, 7), (1, 1), (3, 8200), (2, 9216)) for nd in (4, 5)]


def bias_inputs(case, act):
    """dy and the saved post-activation y = act(pre), pre built around the kink."""
    B, C, inner, nd = case
    shape = (B, C) + BIAS_INNER[inner][nd - 4]
    pre = kinked(*shape, seed=11)
    return dict(dy=rand(*shape, seed=12), pre=pre, y=act_torch(pre, act))


ACT_BWD_N = [1, 2, 3, 4, 5, 1027, 4 * (8192 * 256 + 300) + 3]       # the last: a second grid-stride trip and a 3-element tail
ADD2_N = [1, 3, 1026]

# ------------------------------------------------------------------------------------------------ Adam
ADAM_N = [1, 255, 257, 2097411]                                      # the last > 8192 * 256: a second grid-stride trip
ADAM_BETAS = [(0.0, 0.99), (0.5, 0.999), (0.9, 0.999)]
ADAM_STEPS = 3


def adam_inputs(n):
    """parameters and ADAM_STEPS gradients; from n = 8 a block in the middle (an eighth) has a zero gradient in every step.  A lone
    parameter keeps its gradient: it has to move."""
    gs = [rand(n, seed=10 + s) for s in range(1, ADAM_STEPS + 1)]
    for g in gs:
        g[n // 3: n // 3 + n // 8] = 0
    return dict(p=rand(n, seed=1), grads=gs)


# ------------------------------------------------------------------------------------------------ reconstruction loss
# (2, 3, 33, 37): HW = 1221 > 1024, a second, partial trip of kl_row_kernel's loops; (2, 16, 96, 96): 294 912 > 1024 * 256 elements,
# l1_grad_kernel grid-strides
RECLOSS_CASES = [(1, 2, 3, 5), (2, 3, 33, 37), (2, 16, 96, 96)]
RECLOSS_REFUSED = (4090, 2, 2, 2)        # B (T - 1) + blocks = 4090 + 128 > 4096 scratch-tail slots


def recloss_inputs(shape):
    """targets in [0, 1) (a third above the 0.70 where the L1 weight saturates), predictions in (-1, 1), and a block of the first
    sample where the prediction equals the target exactly."""
    B, T, H, W = shape
    true = torch.rand(B, T, 1, H, W, generator=torch.Generator().manual_seed(1))
    pred = torch.tanh(rand(B, T, 1, H, W, seed=2))
    pred[0, :, :, : (H + 1) // 2, : (W + 1) // 2] = true[0, :, :, : (H + 1) // 2, : (W + 1) // 2]
    return dict(pred=pred, true=true)


# ------------------------------------------------------------------------------------------------ GAN losses
GAN_N = [1, 1023, 1024, 1025, 8197]      # around the 1024 threads of the single workgroup, and nine trips
GAN_LABELS = [(1.0, 0.0), (0.9, 0.1)]


def gan_logits(n, loss_type, seed, kink=0.0):
    """hinge: kink + v + sign(v) * 0.01 (the discriminator's terms bend at +1 for real and -1 for fake logits, kink = 0 for the
    generator's term, which has none); lsgan: randn;
    nsgan: uniform in [0.01, 0.99] with exact 0.0 and 1.0 at the ends and, from n = 4, in the middle."""
    if loss_type == "hinge":
        v = kinked(n, seed=seed, scale=1.5)
        if kink:
            v[0] = -kink * v[0].abs()                                # the first logit on the sloped side: the loss is not 0 at n = 1
        return kink + v
    if loss_type == "lsgan":
        return rand(n, seed=seed, scale=1.5)
    x = torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 0.98 + 0.01
    x[0] = float((seed + 1) % 2)
    if n >= 4:
        x[-1], x[n // 2], x[n // 2 + 1] = 1.0 - float(x[0]), 0.0, 1.0
    return x
