"""The gauge-point IDW (csrc/idw.hip) outside the regime it was tuned for: whole-frame masks (nowcasting / fi / stin), odd and
non-square grids, T = 8 and 32, the lane-per-voxel replay past its LDS capacity and without its LDS copy, the backward with LDS and
with global accumulators in both of its modes, and non-finite upstream gradients.  Cases, inputs and references come from
tests/idw_cases.py (test_idw_cases_cpu.py checks their sizes): the selection is compared index by index with oracle/idw_knn.c, the
weights and outputs with a float64 evaluation to a bound counted in float32 roundings, the backward with a float64 scatter-add over
the saved selection to the bound its arithmetic promises."""
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import idw_cases as ic

pytestmark = pytest.mark.gpu

U = ic.U
CASE_IDS = [c.id for c in ic.cases()]
# how the forward is driven: the default two-pass search; the index-order scan for every voxel (p2i_idw_fwd); pass 2 replaying every
# listed voxel; the cooperative replay of the second list in place of the lane-per-voxel one
VARIANTS = {"default": {}, "scan": {"P2I_IDW_FAST": "0"}, "replay_all": {"P2I_IDW_REPLAY_ALL": "1"}, "coop_replay": {"P2I_IDW_LANE_REPLAY": "0"}}
FWD = [(cid, "default") for cid in CASE_IDS] + [(cid, v) for cid in ("sq32", "odd", "tall") for v in ("scan", "replay_all", "coop_replay")]

Run = namedtuple("Run", "out pt_pos pt_count sel selw listed replayed saved")
_RUNS = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from p2igan_bench import ops as o
    o._hip.load()
    return o


@pytest.fixture(params=["det", "atomic"])
def reduce(request, ops):
    """The backward's two modes: "det" = 64-bit fixed point in the registered scratch (the default); "atomic" = the scratch
    unregistered for the test (what a C caller without p2i_det_workspace gets): float atomics."""
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.det_ready(dev)
    orig = ops._DET[dev.index]
    if request.param == "det":
        if orig is None:
            raise RuntimeError("the deterministic scratch is not registered (P2I_DETERMINISTIC=0?)")
        yield "det"
        return
    lib = ops._hip.load()
    torch.cuda.synchronize()
    ops._hip.check(lib.p2i_det_workspace(None, 0, None, 0), "p2i_det_workspace")
    ops._DET[dev.index] = None
    try:
        yield "atomic"
    finally:
        torch.cuda.synchronize()
        if orig is not None:
            ops._hip.check(lib.p2i_det_workspace(orig[0].data_ptr(), orig[0].numel(), orig[1].data_ptr(), orig[1].numel()), "p2i_det_workspace")
        ops._DET[dev.index] = orig


def _forward(ops, monkeypatch, cid, variant="default", fresh=False):
    """One forward of the case on the device (kept per (case, variant) unless `fresh`), everything brought to the host."""
    key = (cid, variant)
    if fresh or key not in _RUNS:
        c = ic.by_id(cid)
        Q = c.T * c.H * c.W
        for k, v in VARIANTS[variant].items():
            monkeypatch.setenv(k, v)
        amb = []
        out, saved = ops.idw_fwd(ic.values(c).cuda(), ic.masks(c).cuda(), _amb_out=amb)
        torch.cuda.synchronize()
        for k in VARIANTS[variant]:
            monkeypatch.delenv(k)
        listed, replayed = ops.idw_amb_counts(amb[0], c.B, Q) if amb else (None, None)
        pt_pos, pt_count, sel, selw = saved
        run = Run(out.cpu().view(c.B, Q), pt_pos.cpu().view(c.B, Q), pt_count.cpu(), sel.cpu().view(c.B, Q, 4), selw.cpu().view(c.B, Q, 4),
                  listed, replayed, saved)
        if fresh:
            return run
        _RUNS[key] = run
    return _RUNS[key]


def _voxels(c, idx, limit=5):
    HW = c.H * c.W
    return [(int(q) // HW, (int(q) % HW) // c.W, int(q) % c.W) for q in idx[:limit]]


@pytest.mark.parametrize("cid", CASE_IDS)
def test_compaction(ops, monkeypatch, cid):
    """pt_count and pt_pos are nonzero(mask > 0) in (t, y, x) order, per sample."""
    c = ic.by_id(cid)
    r = _forward(ops, monkeypatch, cid)
    assert r.pt_count.tolist() == ic.point_counts(c)
    for b in range(c.B):
        want = ic.point_positions(c, b)
        assert torch.equal(r.pt_pos[b, :len(want)].long(), want), (cid, b)


@pytest.mark.parametrize("cid,variant", FWD)
def test_selection_equals_the_oracle_at_every_voxel(ops, monkeypatch, cid, variant):
    """The four selected points of EVERY voxel are the oracle's four.  The index-order scan gives them in the oracle's order as
    well; the two-pass search does wherever the oracle's four distances are pairwise distinct (ties among the four permute equal
    weights)."""
    c = ic.by_id(cid)
    r = _forward(ops, monkeypatch, cid, variant)
    ref = ic.forward_reference(cid)
    for b in range(c.B):
        got, want, d = r.sel[b].long(), ref[b].sel, ref[b].d
        bad = (got.sort(1).values != want.sort(1).values).any(1).nonzero().flatten()
        assert len(bad) == 0, f"{cid}/{variant} sample {b}: {len(bad)} voxels select other points, first (t, y, x): {_voxels(c, bad)}"
        ordered = torch.ones(len(d), dtype=torch.bool) if variant == "scan" else (d[:, 1:] != d[:, :-1]).all(1)
        bad = ((got != want).any(1) & ordered).nonzero().flatten()
        assert len(bad) == 0, f"{cid}/{variant} sample {b}: {len(bad)} voxels in another order, first (t, y, x): {_voxels(c, bad)}"
        if variant != "scan":
            assert int(ordered.sum()) > 0


@pytest.mark.parametrize("cid,variant", FWD)
def test_weights_and_output_against_float64(ops, monkeypatch, cid, variant):
    """sel_w and out against the float64 evaluation from the same float32 distances, to bounds counted in float32 roundings
    (U = 2^-24 each) -- recounted from the kernels' last lines:
      sel_w: h + tau (1), 1 / . (2), i * i (3), the normaliser's four additions ((((w0 + w1) + w2) + w3) + 1e-12: 4..7), the ten
             roundings of the issue's count with the numerator's three (8..10) -- held to 12 U W_k.  (To first order the square
             doubles the two roundings before it, so the provable worst case is 5 U for a w_k, 9 U for the normaliser and 1 U for
             the last division: 15 U.  The bound is a count, not that worst case; the largest ratio seen is printed.)
      out:   one product per term and three additions on top of a weight's 12 U: 16 U sum |v_k| W_k."""
    c = ic.by_id(cid)
    r = _forward(ops, monkeypatch, cid, variant)
    ref = ic.forward_reference(cid)
    worst_w = worst_o = 0.0
    for b in range(c.B):
        f = ref[b]
        got = r.sel[b].long()
        gi, oi = got.argsort(1), f.sel.argsort(1)
        assert torch.equal(got.gather(1, gi), f.sel.gather(1, oi)), (cid, variant, b)          # aligned by point index
        ew = (r.selw[b].double().gather(1, gi) - f.W.gather(1, oi)).abs() / f.W.gather(1, oi)
        eo = (r.out[b].double() - f.R).abs() / f.A
        worst_w, worst_o = max(worst_w, float(ew.max())), max(worst_o, float(eo.max()))
        assert float(ew.max()) <= 12 * U, f"{cid}/{variant} sample {b}: sel_w off by {float(ew.max()) / U:.2f} U"
        assert float(eo.max()) <= 16 * U, f"{cid}/{variant} sample {b}: out off by {float(eo.max()) / U:.2f} U"
    print(f"{cid}/{variant}: max sel_w error {worst_w / U:.2f} U (bound 12), max out error {worst_o / U:.2f} U (bound 16)")


@pytest.mark.parametrize("cid", CASE_IDS)
def test_paths_were_reached(ops, monkeypatch, cid):
    """From the device's own counters: full pass-1 lists, a replay longer than its grid (sq32 sample 1: > Q / 8), the replay without
    its LDS copy (tall), listed voxels where rounding breaks the ties (rect)."""
    c = ic.by_id(cid)
    Q = c.T * c.H * c.W
    r = _forward(ops, monkeypatch, cid)
    cpu = ic.tie_shares(cid)
    for b in range(c.B):
        print(f"{cid} sample {b} {c.samples[b]}: N {int(r.pt_count[b])}  listed {int(r.listed[b])} ({int(r.listed[b]) / Q:.4f} Q, CPU restatement "
              f"{cpu[b][0]:.4f})  replayed {int(r.replayed[b])} ({int(r.replayed[b]) / Q:.4f} Q, CPU restatement {cpu[b][1]:.4f})")
    assert bool((r.replayed <= r.listed).all()) and bool((r.listed <= Q).all())
    if cid == "sq32":
        assert all(int(r.listed[b]) * 4 > Q for b in range(3)), r.listed
        assert int(r.replayed[1]) * 8 > Q, r.replayed
    if cid in ("tall", "big48"):
        assert int(r.replayed[0]) > 0
    if cid == "rect":
        assert int(r.listed.min()) > 0


@pytest.mark.parametrize("cid", ["sq32", "big48"])
def test_two_runs_are_equal(ops, monkeypatch, cid):
    """The second list's blocks are reserved with an atomic and come in another order from run to run; no result may."""
    a = _forward(ops, monkeypatch, cid, fresh=True)
    b = _forward(ops, monkeypatch, cid, fresh=True)
    assert torch.equal(a.out, b.out)
    assert torch.equal(a.sel.sort(2).values, b.sel.sort(2).values)
    assert torch.equal(a.listed, b.listed) and torch.equal(a.replayed, b.replayed)


# ------------------------------------------------------------------------------------------------ backward
def _bwd(ops, r, d):
    dv = ops.idw_bwd(d.cuda().contiguous(), r.saved)
    torch.cuda.synchronize()
    return dv.cpu()


def _bwd_reference(r, d):
    B = d.shape[0]
    return ic.backward_reference(d.reshape(B, -1).numpy(), r.pt_pos.numpy(), r.pt_count.numpy(), r.sel.numpy(), r.selw.numpy())


def _bwd_bound(mode, S, C, n, k):
    """det: one final rounding of the fixed-point sum, half a unit 2^-k per converted contribution, and the float64 reference's own
    summation error; atomic: a float32 sum of n terms in any order."""
    with np.errstate(invalid="ignore", over="ignore"):
        return U * np.abs(S) + n * 2.0 ** (-k - 1) + n * 2.0 ** -53 * C if mode == "det" else n * U * C


def _assert_within(cid, mode, dv, S, bound, where):
    with np.errstate(invalid="ignore"):
        err = np.abs(dv.astype(np.float64) - S)
        bad = where & ~(err <= bound)
    assert not bad.any(), f"{cid}/{mode}: {int(bad.sum())} entries out of bound, worst {float((err[bad] / np.maximum(bound[bad], 1e-300)).max()):.3g} x"


@pytest.mark.parametrize("cid", ["sq32", "odd", "big48"])
def test_backward_accumulation(ops, monkeypatch, reduce, cid):
    """dvals against the float64 scatter-add of float64(float32(g w)) over the device's saved selection (checked against the oracle
    by the tests above).  With C_j = sum |c| and n_j the number of contributions of point j:
      fixed point   |dv - S| <= 2^-24 |S| + n_j 2^(-k-1) + n_j 2^-53 C_j, k from idw_fix_exp's formula; two runs bit-equal; scaling
                    dout by 2^40 / 2^-40 scales dvals bit for bit (k moves with the exponent, every conversion rounds alike)
      float atomics |dv - S| <= n_j 2^-24 C_j
    and voxels that are no points get exactly 0.  sq32 and odd accumulate in LDS, big48 (N > 8192) in global memory."""
    c = ic.by_id(cid)
    Q = c.T * c.H * c.W
    r = _forward(ops, monkeypatch, cid)
    d = ic.dout(c)
    assert 0.05 < float((d == 0).float().mean()) < 0.15
    dv = _bwd(ops, r, d)
    print(f"{cid}/{reduce}: crc32(dvals) = {zlib.crc32(dv.numpy().tobytes()):08x}" + ("" if reduce == "det" else " (float atomics: varies)"))
    S, C, n = _bwd_reference(r, d)
    k = ic.fix_exp(float(d.abs().max()), Q)
    dvn = dv.view(c.B, Q).numpy()
    _assert_within(cid, reduce, dvn, S, _bwd_bound(reduce, S, C, n, k), np.ones_like(S, dtype=bool))
    for b in range(c.B):
        no_point = np.ones(Q, dtype=bool)
        no_point[r.pt_pos[b, :int(r.pt_count[b])].numpy()] = False
        assert no_point.any() and not dvn[b][no_point].any()
    assert float(np.abs(S).max()) > 0
    if reduce == "det":
        assert torch.equal(_bwd(ops, r, d), dv)
        for p in (40, -40):
            assert torch.equal(_bwd(ops, r, d * 2.0 ** p), dv * 2.0 ** p), f"scaling by 2^{p}"


def test_backward_keeps_non_finite_gradients(ops, monkeypatch, reduce):
    """A NaN in dout[0] and a +Inf in dout[1]: the reference's autograd gives NaN / Inf at the four selected points of those two
    voxels and leaves every other entry alone.  So must both modes of the backward; in fixed point the untouched samples 2 and 3
    are bit-equal to the run without the poisoned entries (the scale comes from the largest FINITE |dout|)."""
    cid = "sq32"
    c = ic.by_id(cid)
    Q = c.T * c.H * c.W
    r = _forward(ops, monkeypatch, cid)
    clean = ic.dout(c)
    d = clean.clone()
    qa, qb = 5 * c.H * c.W + 7 * c.W + 9, 13 * c.H * c.W + 30 * c.W + 2
    d.view(c.B, Q)[0, qa] = float("nan")
    d.view(c.B, Q)[1, qb] = float("inf")
    dv = _bwd(ops, r, d).view(c.B, Q).numpy()
    S, C, n = _bwd_reference(r, d)
    assert int(np.isnan(S).sum()) == 4 and int(np.isnan(S[0]).sum()) == 4 and int(np.isposinf(S[1]).sum()) == 4 and int(np.isinf(S).sum()) == 4
    assert np.array_equal(np.isnan(dv), np.isnan(S)), (np.argwhere(np.isnan(dv)).tolist()[:8], np.argwhere(np.isnan(S)).tolist())
    assert np.array_equal(np.isposinf(dv), np.isposinf(S)) and not np.isneginf(dv).any(), np.argwhere(np.isinf(dv)).tolist()[:8]
    finite = np.isfinite(S)
    k = ic.fix_exp(float(clean.abs().max()), Q)
    assert float(clean.abs().max()) == float(d[torch.isfinite(d)].abs().max())
    _assert_within(cid, reduce, dv, S, _bwd_bound(reduce, S, C, n, k), finite)
    assert float(np.abs(dv[finite]).max()) > 0
    if reduce == "det":
        dv0 = _bwd(ops, r, clean).view(c.B, Q)
        assert torch.equal(torch.from_numpy(dv[2:]), dv0[2:])
