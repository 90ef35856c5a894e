"""CPU companion of tests/test_stdk_kernels_gpu.py (no GPU, no library load): the case lists of tests/stdk_cases.py cover the
issue's tables, every exact case stays below 2^24 in its sum of absolute terms and has an integral float64 expectation that casts
to float32 without loss, and -- from the planners' formulas restated in stdk_cases.py -- the named cases reach the guarded paths of
csrc/stdk.hip they are there for:

  hw79-bt1      a wave tile of 15 rows and three wholly invalid waves in the second workgroup; 79 rows (not a multiple of 4) in
                a single weight-gradient chunk shorter than 256 rows
  hw81-bt3      243 rows, not a multiple of 4
  hw65-bt5      one row in the second workgroup, three wholly invalid waves
  hw64-bt2, hw16-bt4, hw1-bt7   exact fits and a single pixel
  hw257-bt7     1799 rows: a partial last 256-row chunk
  hw1000-bt3    1000 = 62 * 16 + 8
  hw1000-bt131  forward bt_per 2 with a one-frame last split, backward bt_per 3 with a two-frame last split
  hw1000-bt67   backward bt_per 2 with a one-frame last split
  hw79-bt1030   forward: 1024 planned splits, 515 launched; backward bt_per 3 with a one-frame last split
  hw877-bt300   263100 rows: chunk_rows 260 > 256, which does not divide the rows

The model-level cases keep every float64 pre-activation away from its ReLU kink, and the float32 evaluation of the Wendland formula
stays within half of the basis tolerance of the float64 one."""
import numpy as np
import pytest
import torch

import stdk_cases as sc
from test_stdk_gpu import GTOL, TOL

_MLP_REF = {}


def _mlp(c):
    if c.id not in _MLP_REF:
        t = sc.mlp_inputs(c)
        _MLP_REF[c.id] = (t, *sc.mlp_reference(t))
    return _MLP_REF[c.id]


def _by_id(cases):
    return {c.id: c for c in cases}


def test_case_ids_are_unique_and_the_lists_deterministic():
    for make in (sc.mlp_cases, sc.l1_cases, sc.sel_cases, sc.basis_cases, sc.model_cases):
        a, b = make(), make()
        ids = [c.id for c in a]
        assert len(ids) == len(set(ids)), make.__name__
        assert ids == [c.id for c in b]
    t1, t2 = sc.mlp_inputs(sc.mlp_cases()[0]), sc.mlp_inputs(sc.mlp_cases()[0])
    assert all(torch.equal(t1[k], t2[k]) for k in t1)


def test_case_lists_cover_the_tables():
    assert {(79, 1), (81, 3), (65, 5), (64, 2), (16, 4), (1, 7), (257, 7), (1000, 3), (1000, 131), (1000, 67), (79, 1030),
            (877, 300)} <= {(c.HW, c.BT) for c in sc.mlp_cases()}
    l1 = {tuple(c[1:7]) for c in sc.l1_cases()}
    assert {(79, 1, 1, 1, 1, 1), (81, 3, 2, 5, 3, 7), (257, 2, 5, 17, 20, 395), (1000, 5, 3, 139, 12, 237),
            (530, 1, 7, 33, 25, 553)} <= l1
    assert any(hw >= 768 and b == 1 and t == 2 for hw, b, t, *_ in l1)
    assert set(sc.L1_SENTINEL) <= set(_by_id(sc.l1_cases()))
    bs = sc.basis_cases()
    assert {(1, 1, 1), (79, 1, 4), (1, 79, 139), (7, 13, 139), (9, 9, 139), (17, 67, 139)} <= {(c.H, c.W, c.theta.numel()) for c in bs}
    for t, kt in sc.KT_OF_T.items():
        assert (t, 1, kt) in {(c.H, c.W, c.theta.numel()) for c in bs}
    assert {tuple(c[1:5]) for c in sc.model_cases()} == {(1, 1, 9, 9), (3, 2, 7, 13), (2, 5, 10, 8), (1, 3, 1, 79), (2, 3, 79, 1),
                                                         (2, 7, 17, 67)}


# ------------------------------------------------------------------------------------------------ exact family: fused MLP
def test_mlp_value_tables():
    t = sc.mlp_inputs(_by_id(sc.mlp_cases())["hw333-bt40"])
    for k, lo, hi in (("P", -3, 3), ("Q", -3, 3), ("w2", -1, 1), ("w3", -1, 1), ("w4", -1, 1), ("b2", -2, 2), ("b3", -2, 2),
                      ("dy", -2, 2)):
        v = t[k][:, :sc.HID] if k in ("P", "Q") else t[k]
        assert set(v.unique().tolist()) == set(range(lo, hi + 1)), k
    assert -2 <= float(t["b4"]) <= 2
    assert not t["P"][:, sc.HID:].any() and not t["Q"][:, sc.HID:].any()
    for k, want in (("w2", 0.15), ("w3", 0.15), ("w4", 0.5)):
        assert abs(float((t[k] != 0).float().mean()) - want) < (0.02 if k != "w4" else 0.15), k


def test_mlp_backward_reference_matches_autograd():
    """The hand-written float64 backward of stdk_cases.mlp_reference against autograd of the same expression, and independent of
    the number of frames per pass."""
    for cid in ("hw81-bt3", "hw65-bt5", "hw257-bt7"):
        t, r, _ = _mlp(_by_id(sc.mlp_cases())[cid])
        d = {k: v.double().requires_grad_(k != "dy") for k, v in t.items()}
        h = torch.relu(d["P"][None, :, :sc.HID] + d["Q"][:, None, :sc.HID])
        h = torch.relu(h @ d["w2"].t() + d["b2"])
        h = torch.relu(h @ d["w3"].t() + d["b3"])
        y = (h @ d["w4"].t() + d["b4"]).squeeze(-1)
        (y * d["dy"]).sum().backward()
        assert torch.equal(y.detach(), r["y"])
        assert torch.equal(d["P"].grad[:, :sc.HID], r["dP"]) and torch.equal(d["Q"].grad[:, :sc.HID], r["dQ"])
        for k in ("w2", "b2", "w3", "b3", "w4", "b4"):
            assert torch.equal(d[k].grad, r["d" + k]), (cid, k)
        r1, _ = sc.mlp_reference(t, frames_per_pass=2)
        assert all(torch.equal(r[k], r1[k]) for k in r)


@pytest.mark.parametrize("case", sc.mlp_cases(), ids=[c.id for c in sc.mlp_cases()])
def test_mlp_case_is_exact_and_alive(case):
    t, r, bound = _mlp(case)
    print(case.id, {k: "%.3g" % v for k, v in bound.items()})
    assert set(bound) == {"h1", "h2", "h3", "y", "g2", "g1", "dP", "dQ", "dw2", "db2", "dw3", "db3", "dw4", "db4"}
    assert max(bound.values()) < sc.EXACT_LIMIT, bound
    for k, v in r.items():
        assert torch.equal(v, v.round()) and torch.equal(v.float().double(), v), k
        assert float(v.abs().max()) <= bound[k]
    rows = case.HW * case.BT
    if rows >= 243:                                             # (smaller cases are there for their shape)
        for k, v in r.items():
            assert float((v != 0).double().mean()) > (0.005 if k in ("dw2", "dw3") else 0.2), (k, "is almost all zero")
    if case.id == "hw333-bt40":
        alive, zero = sc.mlp_alive(t)
        print("alive", alive, "pre-activations == 0", zero)
        assert all(0.3 <= a <= 0.6 for a in alive)
        assert all(z > 0.01 for z in zero)                      # many exact zeros: the `> 0` gates are pinned to relu'(0) = 0


def test_mlp_cases_reach_the_guarded_paths():
    c = _by_id(sc.mlp_cases())
    assert sc.wave_rows(79) == [16, 16, 16, 16, 15, 0, 0, 0]                # a partial wave tile and wholly invalid waves
    assert sc.wave_rows(65) == [16, 16, 16, 16, 1, 0, 0, 0]                 # one row in the second workgroup, three invalid waves
    assert sc.wave_rows(81)[4:] == [16, 1, 0, 0] and sc.wave_rows(257)[-4:] == [1, 0, 0, 0]
    assert sc.wave_rows(64) == [16] * 4 and sc.wave_rows(16) == [16, 0, 0, 0] and sc.wave_rows(1) == [1, 0, 0, 0]
    assert sc.wave_rows(1000) == [16] * 62 + [8, 0] and sc.wave_rows(877)[-4:] == [16, 16, 13, 0]
    assert {64, 16, 1} <= {x.HW for x in c.values()}
    # weight-gradient rows
    assert 79 % 4 == 3 and sc.wgrad_plan(79) == (256, 1, 79)
    assert 243 % 4 == 3 and sc.wgrad_plan(243) == (256, 1, 243)
    assert sc.wgrad_plan(257 * 7) == (256, 8, 7) and (257 * 7) % 4 == 3
    assert sc.wgrad_plan(64 * 2) == (256, 1, 128) and sc.wgrad_plan(7)[2] == 7
    big = c["hw877-bt300"]
    chunk_rows, chunks, last = sc.wgrad_plan(big.HW * big.BT)
    assert big.HW * big.BT == 263100 > 262144 and chunk_rows == 260 > 256 and chunks == 1012 and 0 < last < chunk_rows
    assert (big.HW * big.BT) % chunk_rows != 0 and last % 4 == 0
    # ragged frame splits
    gx, splits, bt_per, gy = sc.fwd_plan(1000, 131)
    assert (gx, splits, bt_per, gy) == (16, 128, 2, 66) and 131 % bt_per == 1
    gx, splits, bt_per, gy = sc.bwd_plan(1000, 131)
    assert (splits, bt_per, gy) == (64, 3, 44) and 131 - 43 * 3 == 2
    gx, splits, bt_per, gy = sc.bwd_plan(1000, 67)
    assert (splits, bt_per, gy) == (64, 2, 34) and 67 % bt_per == 1
    gx, splits, bt_per, gy = sc.fwd_plan(79, 1030)
    assert (gx, splits, bt_per, gy) == (2, 1024, 2, 515) and gy < splits
    gx, splits, bt_per, gy = sc.bwd_plan(79, 1030)
    assert (splits, bt_per, gy) == (512, 3, 344) and 1030 % bt_per == 1 and gy < splits
    for x in c.values():                                        # every other case: one frame per split in both directions
        if (x.HW, x.BT) not in sc.MLP_LARGE:
            assert sc.fwd_plan(x.HW, x.BT)[2] == 1 and sc.bwd_plan(x.HW, x.BT)[2] == 1
    assert sc.bwd_plan(877, 300)[2:] == (5, 60) and sc.fwd_plan(877, 300)[2:] == (3, 100)       # bt_per > 1, even


# ------------------------------------------------------------------------------------------------ exact family: layer 1
@pytest.mark.parametrize("case", sc.l1_cases(), ids=[c.id for c in sc.l1_cases()])
def test_layer1_case_is_exact(case):
    t = sc.l1_inputs(case)
    for k, lim in (("phi_s", 3), ("phi_t", 3), ("z", 3), ("w1", 3), ("b1", 3), ("dP", 4), ("dQ", 4)):
        assert torch.equal(t[k], t[k].round()) and float(t[k].abs().max()) <= lim
        if t[k].numel() >= 100:
            assert float(t[k].abs().max()) == lim
    r, bound = sc.l1_reference(case, t)
    assert max(bound.values()) < sc.EXACT_LIMIT
    for k, v in r.items():
        assert torch.equal(v, v.round()) and torch.equal(v.float().double(), v) and float(v.abs().max()) <= bound[k]
        assert v.abs().max() > 0
    assert not r["P"][:, sc.HID:].any() and not r["Q"][:, sc.HID:].any()
    # against autograd of the materialised feature rows (the arithmetic of tests/stdk_ref.py)
    w1, b1 = t["w1"].double().requires_grad_(True), t["b1"].double().requires_grad_(True)
    feats = torch.cat([t["phi_s"].double().reshape(1, 1, case.HW, -1).expand(case.B, case.T, case.HW, -1),
                       t["phi_t"].double().reshape(1, case.T, 1, -1).expand(case.B, case.T, case.HW, -1),
                       t["z"].double().reshape(case.B, 1, 1, -1).expand(case.B, case.T, case.HW, -1)], dim=3)
    pre = feats @ w1.t() + b1                                   # [B, T, HW, 100] = P[p] + Q[b, t]
    want = r["P"][None, None, :, :sc.HID] + r["Q"].reshape(case.B, case.T, 1, sc.HP)[..., :sc.HID]
    assert torch.equal(pre.detach(), want)
    # backward: autograd of sum(P * dP) + sum(Q * dQ) with P, Q written as the two small products
    w1 = t["w1"].double().requires_grad_(True)
    Pe = t["phi_s"].double() @ w1[:, :case.Ks].t()
    zq = torch.cat([t["phi_t"].double()[None].expand(case.B, case.T, -1), t["z"].double()[:, None].expand(case.B, case.T, -1)], dim=2)
    Qe = zq.reshape(case.B * case.T, -1) @ w1[:, case.Ks:].t() + b1
    assert torch.equal(Pe.detach(), r["P"][:, :sc.HID]) and torch.equal(Qe.detach(), r["Q"][:, :sc.HID])
    b1.grad = None
    ((Pe * t["dP"].double()).sum() + (Qe * t["dQ"].double()).sum()).backward()
    assert torch.equal(w1.grad, r["dw1"]) and torch.equal(b1.grad, r["db1"])


def test_layer1_cases_reach_the_gemm_splits():
    """k-splits of the three weight-gradient products (K = H*W, T, B): 1, 2 even, 3 with a ragged tail, and splits above both small
    K's (empty splits, which must write zeros); M and N ragged against the 16 x 16 thread tile."""
    assert sc.l1_splits(79) == 1 and sc.l1_splits(255) == 1 and sc.l1_splits(257) == 1
    assert sc.l1_splits(530) == 2 and sc.gemm_chunks(530, 2) == [265, 265]
    assert sc.l1_splits(1000) == 3 and sc.gemm_chunks(1000, 3) == [334, 334, 332]
    assert sc.gemm_chunks(3, 3) == [1, 1, 1] and sc.gemm_chunks(5, 3) == [2, 2, 1]              # T = 3, B = 5 of the 1000 case
    assert sc.gemm_chunks(7, 2) == [4, 3] and sc.gemm_chunks(1, 2) == [1, 0]                    # T = 7, B = 1 of the 530 case
    c = [x for x in sc.l1_cases() if x.HW >= 768 and x.B == 1 and x.T == 2]
    assert c and all(sc.l1_splits(x.HW) == 3 for x in c)
    assert sc.gemm_chunks(2, 3) == [1, 1, 0] and sc.gemm_chunks(1, 3) == [1, 0, 0] and sc.gemm_chunks(777, 3) == [259, 259, 259]
    ks = {k for x in sc.l1_cases() for k in (x.Ks, x.Kt, x.Kz)}
    assert any(k < 16 for k in ks) and any(k % 16 == 0 for k in ks) and any(k > 16 and k % 16 for k in ks) and sc.HID % 16 == 4
    ms = {m for x in sc.l1_cases() for m in (x.HW, x.T, x.B)}
    assert 1 in ms and 64 in ms and any(m > 16 and m % 16 for m in ms)
    # q kernels: B = 1, T = 1, and (T + B + 1) * 100 on either side of one 256-thread workgroup
    bt = {(x.B, x.T) for x in sc.l1_cases()}
    assert (1, 1) in bt and any((b + t + 1) * sc.HID > 256 for b, t in bt) and any(b * t * sc.HP > 256 for b, t in bt)
    assert any((b + t + 1) * sc.HID == 300 for b, t in bt) and any(b * t * sc.HP < 256 for b, t in bt)


# ------------------------------------------------------------------------------------------------ selection
def test_selection_cases_cover_the_table():
    cases = sc.sel_cases()
    assert {c.HW for c in cases} == set(sc.SEL_HW) == {79, 80, 255, 256, 257, 513, 1000}
    assert {c.B * c.T for c in cases if "-bt3-" not in c.id} == {1, 7} and all(c.k == sc.K_VISIBLE for c in cases if "-bt3-" not in c.id)
    assert {1, sc.K_VISIBLE} < {c.k for c in cases} and any(c.k == c.HW > sc.K_VISIBLE for c in cases)
    seen, counts, vals, last79 = set(), set(), set(), set()
    for c in cases:
        assert len(c.frames) == c.B * c.T and c.HW >= c.k
        if c.B * c.T == 7:
            assert len(set(c.frames)) >= 6 and (len(set(c.frames)) == 7 or c.HW == 79)
        x, m = sc.sel_inputs(c)
        assert x.shape == m.shape == (c.B, c.T, c.HW) and x.dtype == m.dtype == torch.float32
        mm = m.reshape(-1, c.HW)
        vals |= set(mm.unique().tolist()) | ({"-0"} if bool(((mm == 0) & torch.signbit(mm)).any()) else set())
        for f, name in enumerate(c.frames):
            obs = (mm[f] != 0).nonzero().flatten().tolist()
            assert obs == sc.sel_pattern(name, c.HW)
            seen.add(name)
            counts.add("all" if len(obs) == c.HW else len(obs))
            if c.k == sc.K_VISIBLE and len(obs) >= 79:
                last79.add(obs[78])
            if name == "p70+15":
                assert sum(1 for p in obs if p < 256) == 70 and len(obs) == 85
        idx, z = sc.sel_reference(c, x, m)
        assert idx.dtype == torch.int32 and idx.shape == z.shape == (c.B, c.T, c.k)
        assert torch.equal(z, torch.gather(x, 2, idx.long()))
        for f in range(c.B * c.T):                                                      # the rule, spelled out once more
            want = np.concatenate([np.flatnonzero(mm[f].numpy() != 0), np.flatnonzero(mm[f].numpy() == 0)])[:c.k]
            assert np.array_equal(idx.reshape(-1, c.k)[f].numpy(), want)
    assert seen == set(sc.SEL_PATTERNS)
    assert {0, 1, 78, 79, 80, "all"} <= counts
    assert {255, 256, 511, 512} <= last79
    assert {1.0, 0.5, -1.0, 0.0, "-0"} <= vals
    # k = H*W: the unobserved fill runs across every 256-pixel pass boundary
    assert any(c.k == c.HW > 512 and sc.sel_pattern(f, c.HW) is not None and len(sc.sel_pattern(f, c.HW)) < 79
               for c in cases for f in c.frames)


# ------------------------------------------------------------------------------------------------ bases
@pytest.mark.parametrize("case", sc.basis_cases(), ids=[c.id for c in sc.basis_cases()])
def test_basis_float32_evaluation_stays_inside_the_margin(case):
    p64, p32 = sc.wendland(case, np.float64), sc.wendland(case, np.float32)
    err = float(np.abs(p32.astype(np.float64) - p64).max())
    print(case.id, "float32 vs float64: %.3g" % err)
    assert err <= sc.BASIS_F32_MARGIN < sc.BASIS_TOL
    assert p64.shape == (case.H * case.W, case.theta.numel()) and p64.min() >= 0 and p64.max() <= 1
    assert p64.max() > 0


def test_basis_hand_table_has_the_edges():
    c = _by_id(sc.basis_cases())["79x1-k4-hand"]
    p = sc.wendland(c, np.float64)
    assert p[15, 0] == 0 and p[5, 0] == 0 and p[14, 0] > 0 and p[6, 0] > 0 and p[10, 0] == 1         # d = 1 exactly, d = 0
    assert any(k != round(k) for k in c.knots.flatten().tolist())                                   # a knot off the grid
    assert (p[:, 1] > 0).sum() == 14 and (p[:, 2] > 0).sum() == 13 and (p[:, 3] > 0).sum() == 1
    assert _by_id(sc.basis_cases())["1x1-k1"].theta.numel() == 1 and sc.wendland(_by_id(sc.basis_cases())["1x1-k1"], np.float64)[0, 0] == 1


# ------------------------------------------------------------------------------------------------ model-level family
@pytest.mark.parametrize("case", sc.model_cases(), ids=[c.id for c in sc.model_cases()])
def test_model_case_keeps_away_from_the_kinks(case):
    from p2igan_bench.models.stdk import space_knots, time_knots
    assert case.H * case.W >= sc.K_VISIBLE
    assert space_knots(case.H, case.W)[1].numel() == 139 and time_knots(case.T)[1].numel() == sc.KT_OF_T[case.T]
    inputs = sc.model_inputs(case)
    sd, masked, masks, dy = inputs
    assert sd["_mlp.net.0.weight"].shape == (100, 139 + sc.KT_OF_T[case.T] + 79 * case.T)
    assert int(masks[0, 0].sum()) == case.gauges and float(dy.min()) >= 0
    pre, y = sc.model_preacts(case, inputs)
    yr, grads = sc.model_reference(case, inputs)
    assert torch.equal(y, yr)                                   # model_preacts restates stdk_ref.forward
    assert all(float(g.abs().max()) > 0 for g in grads)
    margins = sc.kink_margins(pre)
    print(case.id, "min |pre-activation| / max-abs per layer:", ["%.3g" % m for m in margins])
    if case.id not in sc.KINK_BY_FLIP:
        assert min(margins) > sc.KINK_MARGIN, margins
        return
    assert case.B * case.T * case.H * case.W > 10000            # only a map this large may take the second way
    near, ey, eg = sc.model_flip_effect(case, inputs)
    print(case.id, "%d gates within the margin; all flipped at once: preds move %.3g, gradients %.3g of max-abs" % (near, ey, eg))
    assert near > 0 and ey < sc.KINK_FLIP_SHARE * TOL and eg < sc.KINK_FLIP_SHARE * GTOL
