"""CPU companion of tests/test_krig_sys_gpu.py (no GPU, no library load): the cases of tests/krig_sys_cases.py reach what they are
for.  The chunk lists that models/classical.py _Systems makes of every patched _FACTOR_BYTES (more than one chunk, a ragged last one,
a chunk that begins inside a sample, the degenerate sample away from the chunk's first system); the first non-positive pivot of the
failed-factorisation geometry, with its margins in fp32 and fp64; and finite reference compositions for the healthy systems."""
import numpy as np
import pytest

import classical_ref as cr
import krig_sys_cases as kc
import stkriging_ref as sr


def test_case_ids_are_unique_and_inputs_repeat():
    ids = kc.chunk_case_ids()
    assert len(ids) == len(set(ids)) == 19 and ids == kc.chunk_case_ids()
    for name in ("perframe", "shared", "st", "pivot-frames", "pivot-shared", "pivot-table", "pivot-st", "wide9", "wide17"):
        a, b = kc.inputs(name), kc.inputs.__wrapped__(name)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        masked, masks = a
        assert masked.shape == masks.shape and masked.dtype == masks.dtype == np.float32
        assert set(np.unique(masks)) <= {0.0, 1.0} and not masked[masks == 0].any() and (masked[masks != 0] > 0).all()
        assert masked.shape[-2] <= 40 and masked.shape[-1] <= 40


def test_gauge_counts_cross_a_tile_edge_and_differ_from_system_to_system():
    assert kc.counts_of(kc.inputs("perframe")[1]).tolist() == [list(c) for c in kc.PERFRAME_COUNTS]
    assert kc.counts_of(kc.inputs("shared")[1]).tolist() == [[n] * 3 for n in kc.SHARED_COUNTS]
    assert kc.counts_of(kc.inputs("st")[1]).tolist() == [list(c) for c in kc.ST_COUNTS]
    assert kc.st_sample_counts(kc.inputs("st")[1]).tolist() == [5, 31, 33, 40, 64]
    for flat in (np.ravel(kc.PERFRAME_COUNTS), kc.SHARED_COUNTS, kc.st_sample_counts(kc.inputs("st")[1])):
        flat = [int(n) for n in flat]
        assert 0 < min(n for n in flat if n) < 32 < max(flat) == 64 and {31, 33} <= set(flat)
    assert 0 in np.ravel(kc.PERFRAME_COUNTS) and 0 in kc.SHARED_COUNTS and 0 in np.ravel(kc.ST_COUNTS)      # a frame without gauges
    masked, masks = kc.inputs("shared")
    assert all(np.array_equal(masks[b, t], masks[b, 0]) for b in range(5) for t in range(3))                 # one set per sample ...
    assert all(not np.array_equal(masked[b, 1], masked[b, 0]) for b in (0, 1, 4))                            # ... values per frame
    masks = kc.inputs("perframe")[1]
    assert all(not np.array_equal(masks[b, 1], masks[b, 0]) for b in range(3))                               # per-frame sets
    assert [kc.systems_of(c) for c in kc.CHUNK_CASES] == [(9, 1, 64, 3), (5, 3, 64, 3), (15, 1, 64, 3), (5, 1, 64, 3), (5, 1, 64, 3)]


@pytest.mark.parametrize("name", ["perframe", "shared", "st"])
def test_the_fit_is_degenerate_in_one_sample_that_is_not_sample_0(name):
    """The restated fits: cand = -1 exactly where a sample holds one value (or no gauge); everywhere else a fit with a positive psill.
    The Lagrangian fit bins by another distance, but a sample whose semivariances are all zero is degenerate under any binning."""
    masked, masks = kc.inputs(name)
    B, T, _, h, w = masked.shape
    cand = []
    for b in range(B):
        frames = cr._frames_of(masked, masks, b)
        if name == "st":
            fit = sr.fit_st(*sr.st_bins(frames, h, w, 8, 2), cr.lag_width(h, w, 8), "exponential")
        else:
            fit = cr.fit_bins(*cr.variogram_bins(frames, h, w, 8), cr.lag_width(h, w, 8), kc.CHUNK_CASES["krig-" + name][0]["variogram"]["model"])
        cand.append(fit[0])
    print(name, cand)
    want_degenerate = {kc.FLAT[name]} | ({2} if name == "shared" else set())
    assert {b for b in range(B) if cand[b] < 0} == want_degenerate and 0 not in want_degenerate


def test_chunk_lists():
    """For every case and entry point, per takes each of {1, 2, nsys - 1} under the patched _FACTOR_BYTES."""
    for cid, (_, _, entries) in kc.CHUNK_CASES.items():
        nsys, r, np_, T = kc.systems_of(cid)
        for entry in entries:
            plan = kc.chunk_plan(cid, entry)
            assert [p for p, _, _ in plan] == sorted({1, 2, nsys - 1})
            for per, fb, by in plan:
                assert kc.planned_per(cid, entry, fb) == per < nsys == kc.planned_per(cid, entry, 1 << 30)
                chunks = kc.chunk_list(nsys, per)
                assert len(chunks) > 1 and sum(ns for _, ns in chunks) == nsys
                if entry.startswith("ensemble"):
                    a, b = kc.ensemble_bounds(fb, nsys, np_, r, int(entry[8:]), kc.CAP_A)
                    assert (by == "limit") == (b < a)
            if entry.startswith("ensemble"):
                # forward_ensemble's own limit decides the chunk wherever it can: everywhere but for one member of one frame (16 KiB
                # of coefficients at cap = 4096 against the 32 KiB of a 64 x 64 factor and inverse)
                assert [by for _, _, by in plan] == (["limit"] * 3 if r * int(entry[8:]) >= 3 else ["factor"] * 3)
    assert kc.chunk_list(9, 2) == [(0, 2), (2, 2), (4, 2), (6, 2), (8, 1)] and kc.chunk_list(9, 8) == [(0, 8), (8, 1)]
    assert kc.chunk_list(5, 2) == [(0, 2), (2, 2), (4, 1)] and kc.chunk_list(5, 4) == [(0, 4), (4, 1)]
    assert kc.chunk_list(15, 2)[-1] == (14, 1) and kc.chunk_list(15, 14) == [(0, 14), (14, 1)]
    # per frame, per = 2: chunks begin inside samples 0 and 1 (frames 2 and 4 of 3-frame samples), and the degenerate sample 1 (frames
    # 3 .. 5) is the second system of chunk (2, 2) and the whole of chunk (4, 2), which does not start at sample 0
    starts = [s0 for s0, _ in kc.chunk_list(9, 2)]
    assert [s for s in starts if s % 3] == [2, 4, 8] and 4 // 3 == kc.FLAT["perframe"]
    # per sample, per = 2: the degenerate sample 3 is the second system of chunk (2, 2); a chunk-local index would read cand[1] >= 0
    assert (2, 2) in kc.chunk_list(5, 2) and kc.FLAT["shared"] - 2 == 1 and kc.FLAT["st"] - 2 == 1


def test_stage_sub_ranges_are_interior():
    for cid, (name, _, shared, s0, ns, params) in kc.STAGE_CASES.items():
        B, T = kc.inputs(name)[0].shape[:2]
        total = B if shared else B * T
        assert 0 < s0 and s0 + ns < total and len(params) == B and len(set(params)) == B
        assert kc.counts_of(kc.inputs(name)[1]).max() <= kc.STAGE_NP < kc.STAGE_CAP
    name, _, s0, ns, params = kc.ST_STAGE
    assert 0 < s0 and s0 + ns < kc.inputs(name)[0].shape[0] == len(params) == len(set(params))
    s0, ns = kc.PIVOT_SUB
    assert 0 < s0 and s0 + ns < len(kc.PIVOT_FRAMES)
    st = kc.pivot_status()
    assert st[0] == st[-1] == 1 and 1 in st[1:-1] and st[s0] == 1 and 1 in st[s0 + 1:s0 + ns - 1] and 0 in st[s0:s0 + ns]


@pytest.mark.parametrize("cid", sorted(kc.STAGE_CASES))
def test_stage_references_are_finite(cid):
    """NaN only by the frame rules (variance and members of a frame without gauges); the fp32 restatement agrees to fp32 accuracy."""
    name = kc.STAGE_CASES[cid][0]
    n = kc.counts_of(kc.inputs(name)[1]).ravel()
    r64, r32 = kc.stage_reference(cid, "float64"), kc.stage_reference(cid, "float32")
    for k, v in r64.items():
        nan = np.isnan(v).reshape(len(n), -1)
        assert np.array_equal(nan.all(1), nan.any(1))
        assert np.array_equal(nan.any(1), (n == 0) if k in ("var", "ens") else np.zeros(len(n), bool)), k
        assert np.array_equal(np.isnan(r32[k]), np.isnan(v)) and np.isfinite(v[~np.isnan(v)]).all()
        e32 = float(np.nanmax(np.abs(r32[k].astype(np.float64) - v))) / float(np.nanmax(np.abs(v)))
        print(f"{cid} {k}: e32 {e32:.3e}")
        assert e32 < 1e-3
    p64, v64 = kc.st_reference("float64")
    assert np.isfinite(p64).all() and np.isfinite(v64).all() and (v64 >= 0).all()


@pytest.mark.parametrize("npre", kc.PIVOT_NPRE)
def test_first_bad_pivot(npre):
    """The condition of section C: in both number formats the first non-positive pivot is that of the triple's second gauge, every
    earlier pivot is >= 0.1 psill and the bad one <= -0.1 psill."""
    xy, _ = cr.gauges(kc.pivot_mask(npre, True), kc.pivot_mask(npre, True))
    assert len(xy) == npre + 3 and [tuple(p) for p in xy[-3:]] == list(kc.TRIPLE)
    for dt in (np.float64, np.float32):
        K = cr.covariance(xy, xy, *kc.f32(kc.BAD), kc.PIVOT_MODEL, dt)
        j, piv = kc.elimination(K, dt)
        print(f"npre {npre} {np.dtype(dt).name}: first bad pivot at {j} (tile {j // kc.TILE}) = {piv[-1] / kc.PSILL:+.4f} psill, "
              f"smallest earlier pivot {min(piv[:-1]) / kc.PSILL:.4f} psill")
        assert j == npre + 1 == {5: 6, 40: 41, 64: 65}[npre] and j // kc.TILE == kc.PIVOT_NPRE.index(npre)
        assert min(piv[:-1]) >= 0.1 * kc.PSILL and piv[-1] <= -0.1 * kc.PSILL
        healthy = cr.covariance(xy[:npre], xy[:npre], *kc.f32(kc.BAD), kc.PIVOT_MODEL, dt)
        j, piv = kc.elimination(healthy, dt)
        assert j == -1 and min(piv) >= 0.1 * kc.PSILL                     # without the triple the same parameters factor
        j, piv = kc.elimination(cr.covariance(xy, xy, *kc.f32(kc.BENIGN), kc.PIVOT_MODEL, dt), dt)
        assert j == -1 and min(piv) >= 0.1 * kc.PSILL                     # and so does the triple with a benign nugget


def test_pivot_inputs_fail_where_they_should():
    masked, masks = kc.inputs("pivot-frames")
    assert kc.counts_of(masks)[0].tolist() == [8, 40, 43, 64, 67, 5, 33, 67] and kc.counts_of(masks).max() <= kc.PIVOT_NP
    assert kc.pivot_status() == [1, 0, 1, 0, 1, 0, 0, 1] and kc.pivot_healthy() == [1, 3, 5, 6]
    for t, (npre, triple) in enumerate(kc.PIVOT_FRAMES):
        xy, _ = cr.gauges(masked[0, t, 0], masks[0, t, 0])
        for dt in (np.float64, np.float32):
            j, piv = kc.elimination(cr.covariance(xy, xy, *kc.f32(kc.BAD), kc.PIVOT_MODEL, dt), dt)
            assert j == (npre + 1 if triple else -1) and min(piv[:-1] if triple else piv) >= 0.1 * kc.PSILL
    h = kc.inputs("pivot-frames-healthy")
    assert np.array_equal(h[0][0], masked[0, kc.pivot_healthy()]) and kc.counts_of(h[1])[0].tolist() == [40, 64, 5, 33]
    assert kc.counts_of(kc.inputs("pivot-shared")[1]).tolist() == [[43] * 3, [40] * 3]
    assert np.array_equal(kc.inputs("pivot-shared-healthy")[0][0], kc.inputs("pivot-shared")[0][1])


def test_space_time_pivot():
    """time_scale 8 > range 4: frames decouple, and the space-time matrix of sample 1 meets the same pivot at 40 + 6 = 46 (tile 1)."""
    masked, masks = kc.inputs("pivot-st")
    assert kc.PIVOT_KAPPA > kc.BAD[2] and kc.st_sample_counts(masks).tolist() == [45, 48, 38]
    for b, want in enumerate((-1, 46, -1)):
        xy, tt, _ = sr.points(masked[b], masks[b])
        for dt in (np.float64, np.float32):
            K = sr.st_covariance(xy, tt, xy, tt, *kc.f32(kc.BAD), kc.PIVOT_KAPPA, kc.PIVOT_MODEL, dt)
            assert not K[tt[:, None] != tt[None, :]].any()
            j, piv = kc.elimination(K, dt)
            print(f"pivot-st sample {b} {np.dtype(dt).name}: bad pivot {j}, last pivot {piv[-1] / kc.PSILL:+.4f} psill")
            assert j == want and min(piv[:-1] if want >= 0 else piv) >= 0.1 * kc.PSILL and (want < 0 or piv[-1] <= -0.1 * kc.PSILL)
    assert 46 // kc.TILE == 1


def test_truth_table_inputs():
    """pivot-table: samples 0 and 2 fit (cand >= 0), sample 1 holds one value (cand = -1); sample 2's fitted parameters factor with a
    margin in both formats, and the bad parameters fail on sample 0's set."""
    masked, masks = kc.inputs("pivot-table")
    B, T, _, h, w = masked.shape
    fits = [cr.fit_bins(*cr.variogram_bins(cr._frames_of(masked, masks, b), h, w, 8), cr.lag_width(h, w, 8), kc.PIVOT_MODEL) for b in range(B)]
    assert [f[0] >= 0 for f in fits] == [True, False, True]
    xy, _ = cr.gauges(masked[2, 0, 0], masks[2, 0, 0])
    for dt in (np.float64, np.float32):
        j, piv = kc.elimination(cr.covariance(xy, xy, *kc.f32(fits[2][1:4]), kc.PIVOT_MODEL, dt), dt)
        print(f"pivot-table sample 2 {np.dtype(dt).name}: fit {fits[2][1:4]}, smallest pivot {min(piv):.3e} (psill {fits[2][2]:.3e})")
        assert j == -1 and min(piv) >= 0.01 * fits[2][2]
        assert kc.elimination(cr.covariance(xy, xy, *kc.f32(kc.BAD), kc.PIVOT_MODEL, dt), dt)[0] == 41


def test_wide_sets():
    for t in (9, 17):
        masked, masks = kc.inputs(f"wide{t}")
        assert masked.shape == (1, t, 1, 24, 40) and t > kc.RC and t % kc.RC == 1 and (24 * 40) % 256
        assert all(np.array_equal(masks[0, i], masks[0, 0]) for i in range(t)) and int(masks[0, 0].sum()) == 20
        vals = masked[0, :, 0][:, masks[0, 0, 0] != 0]
        assert all(not np.array_equal(vals[i], vals[j]) for i in range(t) for j in range(i))
