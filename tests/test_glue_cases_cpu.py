"""The inputs of test_glue_edges_gpu.py (tests/glue_cases.py) have the properties its comparisons rely on -- checked here on the CPU,
so that a GPU failure there is the kernel's and never a float32 / float64 disagreement about which side of a kink a value is on."""
import pytest
import torch

import glue_cases as gc


@pytest.mark.parametrize("case", gc.ATTN_CASES, ids=gc.attn_id)
def test_attention_inputs_keep_their_margin_and_their_plan(case):
    B, HW, T = case
    inp = gc.attn_inputs(case)
    assert gc.attn_margin(inp) > gc.ATTN_MARGIN
    assert bool((inp["x"] > 0).any()) and bool((inp["x"] < 0).any())
    # the gradient is non-zero exactly at the planned pixels, chunk by chunk
    nz = (inp["gout"] != 0).any(dim=1).view(B, HW)
    assert torch.equal(nz, inp["active"])
    plan = gc.ATTN_PLANS[(B, HW)]
    nchunk = -(-HW // gc.ATTN_CHUNK)
    for b in range(B):
        for c in range(nchunk):
            assert int(nz[b, c * gc.ATTN_CHUNK:(c + 1) * gc.ATTN_CHUNK].sum()) == plan.get((b, c), 0), (b, c)
    # one pixel per sample with a gradient has it in a single frame
    assert {b for b, _, _ in inp["single"]} == {b for b, _ in plan}
    for b, p, t in inp["single"]:
        assert int((inp["gout"][b, :, 0, p] != 0).sum()) == 1 and float(inp["gout"][b, t, 0, p]) != 0.0


def test_attention_plans_reach_the_paths_they_are_for():
    counts = set()
    empty_between = two_chunk_walk = partial_last = False
    for (B, HW), plan in gc.ATTN_PLANS.items():
        nchunk, gx = -(-HW // gc.ATTN_CHUNK), gc.attn_grid_x(B, HW)
        for (b, c), n in plan.items():
            assert 0 <= b < B and 0 <= c < nchunk and 0 < n <= min(gc.ATTN_CHUNK, HW - c * gc.ATTN_CHUNK)
            counts.add(n)
            partial_last |= c == nchunk - 1 and HW % gc.ATTN_CHUNK != 0 and n == HW % gc.ATTN_CHUNK
        for b in {b for b, _ in plan}:
            for wg in range(gx):
                walk = [plan.get((b, c), 0) for c in range(wg, nchunk, gx)]
                two_chunk_walk |= len(walk) >= 2 and all(walk)
                empty_between |= any(walk[i] == 0 and any(walk[:i]) and any(walk[i + 1:]) for i in range(len(walk)))
    assert {1, 32, 33, 256} <= counts
    assert empty_between and two_chunk_walk and partial_last
    assert gc.attn_grid_x(16, 1297) == 4 and gc.attn_grid_x(64, 300) == 1 and gc.attn_grid_x(70, 300) == 1 and gc.attn_grid_x(2, 257) == 2


def test_kinked_values_keep_their_margin_by_construction():
    margin = float(torch.tensor(gc.KINK_MARGIN))                  # the margin as float32 holds it (rounding to nearest is monotonic)
    for act in gc.ACTS:
        for case in gc.BIAS_CASES:
            if case[2] <= 8200:                                    # (the 9216 cases draw from the same stream)
                assert float(gc.bias_inputs(case, act)["pre"].abs().min()) >= margin
    assert float(gc.kinked(4 * (8192 * 256 + 300) + 3, seed=21).abs().min()) >= margin
    for n in gc.GAN_N:
        for kink in (1.0, -1.0):
            x = gc.gan_logits(n, "hinge", 3, kink)
            # (the sum kink + v rounds to float32: half an ulp of the largest logit is far below the margin)
            assert float((x - kink).abs().min()) >= margin - 1e-6
        x = gc.gan_logits(n, "nsgan", 4)
        assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0 and bool(((x == 0) | (x == 1)).any())
        if n >= 4:
            assert bool((x == 0).any()) and bool((x == 1).any())


@pytest.mark.parametrize("shape", gc.POOLDUP_CASES + [gc.POOLDUP_BIG], ids=lambda s: gc.case_id(s))
def test_pooldup_inputs_hold_tied_windows(shape):
    assert gc.pooldup_tied_windows(gc.pooldup_inputs(shape)["x"]) > 0


def test_pooldup_hand_made_ties_cover_every_position():
    x = gc.pooldup_all_ties()["x"]
    win = x.view(1, 1, 3, 2, 5, 2).permute(0, 1, 2, 4, 3, 5).reshape(15, 4)
    assert sorted(int((w * torch.tensor([1., 2., 4., 8.])).sum()) for w in win) == list(range(1, 16))
    assert gc.pooldup_tied_windows(x) == 11


def test_shapes_reach_the_second_trips_they_are_for():
    assert gc.DTAIL_B * 96 * 96 > 64 * 256 and (96, 96, 1, 48, 48) in gc.DTAIL_CASES
    B, C, H, W = gc.POOLDUP_BIG
    assert B * C * (H // 2) * (W // 2) > 8192 * 256 and B * C * H * W * 4 < 40e6
    assert gc.ACT_BWD_N[-1] // 4 > 8192 * 256 and gc.ACT_BWD_N[-1] % 4 == 3
    assert gc.ADAM_N[-1] > 8192 * 256
    assert 3 * 8200 > 16384 and (3 * 8200 + 1) // 2 % 8200 != 0 and 8200 // 4 > 2048
    assert 33 * 37 > 1024 and 2 * 16 * 96 * 96 > 1024 * 256
    B, T, H, W = gc.RECLOSS_REFUSED
    assert B * (T - 1) + (B * T * H * W + 255) // 256 > 4096
    for shape in gc.RECLOSS_CASES:
        inp = gc.recloss_inputs(shape)
        assert bool((inp["true"] > 0.70).any()) and bool((inp["pred"] == inp["true"]).any()) and bool((inp["pred"] != inp["true"]).any())
    for (H2, W2, T3, H3, W3) in gc.DTAIL_CASES:
        assert H3 <= H2 and W3 <= W2
    assert sum(1 for (H2, W2, _, H3, W3) in gc.DTAIL_CASES if H2 == 2 * H3 - 1 or W2 == 2 * W3 - 1) >= 5
    for n in gc.ADAM_N:
        for g in gc.adam_inputs(n)["grads"]:
            assert bool((g != 0).any()) and (n < 8 or bool((g == 0).any()))      # every case moves; the zero block needs eight elements


def test_case_ids_are_unique_and_deterministic():
    tables = [[gc.attn_id(c) for c in gc.ATTN_CASES], [gc.case_id(c) for c in gc.DTAIL_CASES], [gc.case_id(c) for c in gc.POOLDUP_CASES],
              [gc.case_id(c) for c in gc.UPMOD_CASES], [gc.case_id(c) for c in gc.BIAS_CASES], [gc.case_id(c) for c in gc.RECLOSS_CASES],
              [gc.case_id(n, b) for n in gc.ADAM_N for b in gc.ADAM_BETAS]]
    for ids in tables:
        assert len(set(ids)) == len(ids) and all(isinstance(i, str) and i for i in ids)
    assert gc.case_id((3, 5, 6, 10)) == "3x5x6x10" and gc.case_id(257, (0.5, 0.999)) == "257-0.5x0.999"
    a, b = gc.attn_inputs(gc.ATTN_CASES[4]), gc.attn_inputs(gc.ATTN_CASES[4])
    assert all(torch.equal(a[k], b[k]) for k in ("x", "w0", "b0", "w1", "b1", "gout", "active"))
    assert torch.equal(gc.upmod_inputs(gc.UPMOD_CASES[3])["pos"], gc.upmod_inputs(gc.UPMOD_CASES[3])["pos"])
    pos = gc.upmod_inputs(gc.UPMOD_CASES[0])["pos"]
    assert float(pos.max()) == 20.0 and float(pos.min()) == -20.0
