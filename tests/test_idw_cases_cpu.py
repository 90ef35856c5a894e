"""CPU companion of tests/test_idw_regimes_gpu.py (no GPU, no library load): the cases of tests/idw_cases.py have the point counts,
grid shapes and LDS sizes that put them on the paths of csrc/idw.hip they are there for, the float32 restatement of the distance
chain says that the whole-frame masks fill pass 1's lists and leave the replay more than its grid covers at once, and the backward
reference is autograd of the oracle.

  sq32   nowcasting / fi stride 6 / fi stride 3 / stin in ONE launch: N = 4096 / 3072 / 6144 / 4864.  3072 is exactly the replay's
         LDS capacity (IDW_RW_PCAP), 4096 and 6144 read the points from global memory; > Q/4 listed, sample 1 leaves > 0.15 Q to
         the replay, whose grid covers Q/8
  rect   24 x 40: rounding breaks the in-frame ties, (almost) nothing is replayed
  odd    H W = 99 (idw_count_kernel's scalar branch; a 256-voxel workgroup spans 3-4 frames), Q = 792 = 3 * 256 + 24, T = 8
  long   T = 32, 28 frames without a point
  tall   T (H + 1) = 4128: 49152 + 16512 bytes > 64 KiB, the replay runs without its LDS copy
  big48  N = 13824 > 8192: the backward's global accumulators"""
import numpy as np
import pytest
import torch

import idw_cases as ic

CASES = ic.cases()


def test_case_ids_are_unique_and_inputs_repeat():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)) and ids == [c.id for c in ic.cases()]
    for c in CASES:
        assert len(c.samples) == c.B
        assert torch.equal(ic.masks(c), ic.masks(c)) and torch.equal(ic.values(c), ic.values(c)) and torch.equal(ic.dout(c), ic.dout(c))
        assert set(ic.masks(c).unique().tolist()) <= {0.0, 1.0}
        assert min(ic.point_counts(c)) >= 256, (c.id, ic.point_counts(c))        # the C restatement models topk's partial sort only


def test_point_counts_and_lds_sizes():
    n = {c.id: ic.point_counts(c) for c in CASES}
    assert n["sq32"] == [4096, 3072, 6144, 4864]
    assert n["sq32"][1] == ic.IDW_RW_PCAP and n["sq32"][0] > ic.IDW_RW_PCAP and n["sq32"][2] > ic.IDW_RW_PCAP
    assert n["rect"] == [3840, 4560]
    assert n["odd"] == [396, 297]
    assert n["long"] == [1024]
    assert n["tall"] == [2048]
    assert n["big48"] == [13824] and n["big48"][0] > ic.IDW_LDS_PTS
    assert max(max(v) for k, v in n.items() if k != "big48") <= ic.IDW_LDS_PTS         # ... and every other case the LDS accumulators
    for c in CASES:
        lds = ic.replay_lds_bytes(c)
        assert lds == 49152 + 4 * c.T * (c.H + 1)
        assert (lds > ic.LDS_BYTES) == (c.id == "tall"), (c.id, lds)
    t = ic.by_id("tall")
    assert t.T * (t.H + 1) == 4128 and ic.replay_lds_bytes(t) == 65664


def test_mask_rules():
    """The masks are create_mask's: whole frames observed, the others empty (nowcasting, fi) or one block mask (stin)."""
    c = ic.by_id("sq32")
    m = ic.masks(c)
    per_frame = m.flatten(2).sum(2)
    HW = c.H * c.W
    assert per_frame[0].tolist() == [HW] * 4 + [0] * 12
    assert per_frame[1].tolist() == [HW if t in (0, 6, 12) else 0 for t in range(16)]
    assert per_frame[2].tolist() == [HW if t % 3 == 0 else 0 for t in range(16)]
    assert per_frame[3].tolist() == [HW] * 4 + [HW // 16] * 12
    assert all(torch.equal(m[3, t], m[3, 4]) for t in range(5, 16))
    cells = m[3, 4].reshape(8, 4, 8, 4).sum((1, 3))
    assert bool((cells == 1).all())                                          # one pixel per 4 x 4 cell
    lg = ic.masks(ic.by_id("long"))[0].flatten(1).sum(1)
    assert int((lg == 0).sum()) == 28
    tl = ic.masks(ic.by_id("tall"))[0]
    assert all(torch.equal(tl[t], tl[0]) for t in range(1, 32)) and int(tl[0].sum()) == 64


def test_odd_grid_shapes():
    c = ic.by_id("odd")
    assert (c.H * c.W) % 4 != 0 and (c.T * c.H * c.W) % 256 != 0
    assert c.H * c.W < 256 and (c.T * c.H * c.W) % 256 == 24                # workgroups across frames; 24 active lanes in the last


@pytest.mark.parametrize("cid", ["sq32", "rect", "tall"])
def test_tie_shares_reach_the_paths(cid):
    """The ranges sit around the float32 restatement's values (sq32: 0.50 / 0.53 / 0.51 listed, 0.18 Q of sample 1 replayed;
    rect sample 0: 0.30 listed, none replayed; tall: 0.009 replayed)."""
    sh = ic.tie_shares(cid)
    print(cid, " ".join("listed %.4f replayed %.4f" % s for s in sh))
    if cid == "sq32":
        assert all(sh[b][0] > 0.25 for b in range(3))
        assert sh[1][1] > 0.15 and sh[1][1] * 8 > 1                        # more than the replay's grid covers at once (Q / 8)
    elif cid == "rect":
        assert sh[0][1] < 0.01 and sh[0][0] > 0
    else:
        assert sh[0][1] > 0


@pytest.mark.parametrize("cid", ["odd", "long"])
def test_backward_reference_is_autograd_of_the_oracle(cid):
    """float64 autograd through oracle.idw_3d_knn (float64 values, the oracle's float32 weights) against backward_reference over the
    oracle's own selection and weights.  The upstream gradient is +-2^j or 0, so float32(g * w) is exact and the two sums differ by
    float64 summation order only: n * 2^-53 * C per point, far inside 1e-12 * C."""
    from oracle import p2i_oracle as orc
    c = ic.by_id(cid)
    mk, vals = ic.masks(c), ic.values(c)
    g = torch.Generator().manual_seed(c.seed + 7)
    shape = (c.B, c.T, c.H, c.W)
    gout = torch.randint(-1, 2, shape, generator=g).double() * torch.pow(2.0, torch.randint(-3, 4, shape, generator=g).double())
    Q = c.T * c.H * c.W
    want = np.zeros((c.B, Q))
    sel_idx, sel_w = np.zeros((c.B, Q, 4), dtype=np.int32), np.zeros((c.B, Q, 4), dtype=np.float32)
    pt_pos, pt_count = np.zeros((c.B, Q), dtype=np.int32), np.zeros(c.B, dtype=np.int32)
    for b in range(c.B):
        tz, ty, tx, pts = orc.mask_points(mk[b])
        v = vals[b][tz, ty, tx].double().requires_grad_(True)
        out = orc.idw_3d_knn(pts, v, (c.T, c.H, c.W))
        out.backward(gout[b])
        pos = ic.point_positions(c, b)
        want[b, pos.numpy()] = v.grad.numpy()
        f = ic.forward_reference(cid)[b]
        inv = 1.0 / (f.d + orc.IDW_TAU)
        w = inv * inv
        sel_idx[b], sel_w[b] = f.sel.numpy(), (w / (w.sum(dim=1, keepdim=True) + 1e-12)).numpy()
        pt_pos[b, :len(pos)], pt_count[b] = pos.numpy(), len(pos)
    S, C, n = ic.backward_reference(gout.float().reshape(c.B, Q).numpy(), pt_pos, pt_count, sel_idx, sel_w)
    assert float(np.abs(want).max()) > 0 and int(n.sum()) == 4 * int((gout != 0).sum())
    assert bool((np.abs(S - want) <= 1e-12 * C).all()), float((np.abs(S - want) / np.maximum(C, 1e-300)).max())
    assert float(np.abs(S - want).max()) <= 1e-12 * float(np.abs(want).max())
    assert bool((S[n == 0] == 0).all())


def test_backward_reference_propagates_non_finite_gradients():
    """A NaN / Inf in dout reaches exactly the four selected points of its voxel."""
    c = ic.by_id("odd")
    Q = c.T * c.H * c.W
    f = ic.forward_reference("odd")[0]
    pos = ic.point_positions(c, 0).numpy()
    d = ic.dout(c).reshape(c.B, Q)[:1].numpy().copy()
    qa, qb = 100, 500
    d[0, qa], d[0, qb] = np.nan, np.inf
    w = f.W.float().numpy()
    S, _, _ = ic.backward_reference(d, pos[None].astype(np.int32), np.array([len(pos)]), f.sel.numpy()[None], w[None])
    nan_at, inf_at = set(pos[f.sel[qa].numpy()]), set(pos[f.sel[qb].numpy()]) - set(pos[f.sel[qa].numpy()])
    assert set(np.nonzero(np.isnan(S[0]))[0]) == nan_at and set(np.nonzero(np.isinf(S[0]))[0]) == inf_at
