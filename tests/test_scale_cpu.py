"""Scale-aware verification on CPU: the numpy restatement (tests/scale_ref.py) against scipy's uniform_filter and hand-computed ring
populations, the properties of the FSS, the host rules of the product (useful scale, refusals, overflow guard, ring list),
scripts/evaluate.py's --scale handling and output layout, and the new ABI symbols."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

import scale_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_counts_equal_scipy_uniform_filter():
    from scipy import ndimage
    S = 13
    ind = (np.random.default_rng(3).random((2, S, S)) < 0.3)
    for n in (1, 2, 3, 4, 6, 13, 14, 27):
        want = np.stack([np.rint(ndimage.uniform_filter(f.astype(np.float64), size=n, mode="constant") * n * n) for f in ind])
        assert np.array_equal(scale_ref.window_counts(ind, n), want.astype(np.int64)), n


def test_ring_populations():
    from p2igan_bench.evaluation import ring_counts, ring_index, ring_list
    want = {7: [1, 8, 12, 16], 8: [1, 8, 12, 16, 22], 12: [1, 8, 12, 16, 32, 28, 30]}
    for S, pop in want.items():
        assert scale_ref.ring_counts(S).tolist() == pop
        assert ring_counts(S).tolist() == pop
        assert np.array_equal(ring_index(S), scale_ref.ring_index(S))
        # the half-plane list with its weights covers every full-plane bin of rings 0 .. S // 2 once
        order, weight, offsets, count = ring_list(S)
        assert offsets[0] == 0 and offsets[-1] == len(order) == len(weight) and count.tolist() == pop
        assert [float(weight[offsets[r]:offsets[r + 1]].sum()) for r in range(len(pop))] == pop
        assert len(set(order.tolist())) == len(order) and order.max() < S * (S // 2 + 1)
        ring = scale_ref.ring_index(S)[:, :S // 2 + 1].ravel()
        for r in range(len(pop)):
            assert np.all(ring[order[offsets[r]:offsets[r + 1]]] == r)


def test_half_plane_ring_sums_equal_full_plane():
    from p2igan_bench.evaluation import ring_list
    for S in (1, 7, 8, 12, 27):
        f = np.random.default_rng(S).random((S, S))
        psd = np.abs(np.fft.fft2(f)) ** 2 / (S * S)
        order, weight, offsets, count = ring_list(S)
        half = psd[:, :S // 2 + 1].ravel()
        got = np.array([np.sum(half[order[offsets[r]:offsets[r + 1]]] * weight[offsets[r]:offsets[r + 1]]) for r in range(len(count))]) / count
        want = scale_ref.rapsd(f)
        assert np.all(np.abs(got - want) <= 1e-13 * want[0])


def _fss(p, g, q, n):
    s = scale_ref.fss_sums(p, g, (q,), (n,))[0]
    return scale_ref.fss_value(*s[:3])


def test_fss_properties():
    S = 16
    g = scale_ref.transform(scale_ref.field(11, 3, S, S))
    p = scale_ref.transform(scale_ref.field(12, 3, S, S))
    for n in (1, 2, 5, 16, 40):
        assert _fss(g, g, 2.0, n) == 1.0                                    # a field against itself
    # n >= 2 S - 1: every window covers the crop, c is the frame's count everywhere: the global-fraction value
    cp, cg = (p >= 2.0).sum(axis=(1, 2)).astype(object), (g >= 2.0).sum(axis=(1, 2)).astype(object)
    A, B, C = S * S * int((cp * cp).sum()), S * S * int((cg * cg).sum()), S * S * int((cp * cg).sum())
    for n in (2 * S - 1, 2 * S, 2 * S + 1, 1000):
        assert scale_ref.fss_sums(p, g, (2.0,), (n,))[0, :3].tolist() == [A, B, C]
        assert _fss(p, g, 2.0, n) == scale_ref.fss_value(A, B, C)
    assert math.isnan(_fss(p, g, 500.0, 3))                                 # nothing reaches the threshold in either field
    assert _fss(p, np.zeros_like(g), 2.0, 3) == 0.0
    nan = p.copy()
    nan[0, 2, 3] = np.nan                                                   # NaN compares false
    hit = p.copy()
    hit[0, 2, 3] = 0.0
    assert np.array_equal(scale_ref.fss_sums(nan, g, (2.0,), (3,)), scale_ref.fss_sums(hit, g, (2.0,), (3,)))


def test_product_host_rules_match_restatement():
    from p2igan_bench.evaluation import fss_value, spectrum_scores, useful_scale
    assert math.isnan(fss_value(0, 0, 0)) and fss_value(5, 5, 5) == 1.0 and fss_value(4, 4, 0) == 0.0
    big = 3 ** 38                                                           # beyond 2^53: the division is exact-integer based
    assert fss_value(big, big + 2, big) == scale_ref.fss_value(big, big + 2, big) == 1.0 - 2 / (2 * big + 2)
    # FSS >= 0.5 + f0 / 2 with f0 = 1000 / 10000: target 0.55
    by_n = {9: 0.9, 1: 0.2, 3: 0.55, 5: 0.7}
    assert useful_scale(by_n, 1000, 10000) == scale_ref.useful_scale(by_n, 1000, 10000) == 3
    assert useful_scale({1: 0.2, 3: 0.5499}, 1000, 10000) is None
    assert useful_scale({1: float("nan")}, 0, 100) is None
    pm, pt = np.array([9.0, 2.0, 1.0, 0.5, 0.1]), np.array([9.0, 1.0, 1.0, 1.0, 1.0])
    lsd, hf = spectrum_scores(pm, pt, 8)
    d = 10 * np.log10(pm[1:] / pt[1:])
    assert abs(lsd - math.sqrt(np.mean(d * d))) < 1e-12 and abs(hf - (0.5 + 0.1) / 2) < 1e-15      # rings 3, 4 lie above S / 4 = 2
    assert scale_ref.spectrum_scores(pm, pt, 8) == (lsd, hf)
    l1, h1 = spectrum_scores(np.array([4.0]), np.array([4.0]), 1)           # S = 1 has ring 0 only
    assert math.isnan(l1) and math.isnan(h1)


def test_refusals_come_before_the_gpu_check(monkeypatch):
    import torch
    from p2igan_bench import evaluation
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match="gauge"):
        evaluation.ScaleEvaluator(16, mode="gauge")
    with pytest.raises(ValueError, match="gauge"):
        evaluation.run_scale({"a": np.zeros((2, 16, 16), np.float32)}, np.zeros((2, 16, 16), np.uint8), 16, mode="gauge")
    with pytest.raises(ValueError, match="Unknown mode"):
        evaluation.ScaleEvaluator(16, mode="satellite")
    with pytest.raises(ValueError, match="16 scales"):
        evaluation.ScaleEvaluator(16, scales=tuple(range(1, 18)))
    with pytest.raises(ValueError, match="thresholds"):
        evaluation.ScaleEvaluator(16, thresholds=tuple(float(i) for i in range(9)))
    with pytest.raises(ValueError, match="window sizes"):
        evaluation.ScaleEvaluator(16, scales=(0, 3))
    with pytest.raises(ValueError, match="crop size"):
        evaluation.ScaleEvaluator(2048)


def test_evaluator_refuses_to_run_without_gpu(monkeypatch):
    import torch
    from p2igan_bench import evaluation
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="scale verification runs on the GPU"):
        evaluation.ScaleEvaluator(16, evaluation.DEFAULT_THRESHOLDS, evaluation.DEFAULT_SCALES)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluation.run_scale({"a": np.zeros((2, 16, 16), np.float32)}, np.zeros((2, 16, 16), np.uint8), 16)


def test_overflow_guard():
    from p2igan_bench.evaluation import check_overflow
    # frames * S^2 * min(n, S)^4 with S = 128, n = 65: lim is the first frame count whose bound reaches 2^63
    lim = -(-2 ** 63 // (128 * 128 * 65 ** 4))
    check_overflow(lim - 1, 128, (1, 65))
    with pytest.raises(OverflowError):
        check_overflow(lim, 128, (1, 65))
    check_overflow(2400, 128, (1, 3, 5, 9, 17, 33, 65))
    # the window is clipped to the crop: n = 10^6 counts as S
    check_overflow(1000, 128, (10 ** 6,))
    with pytest.raises(OverflowError):
        check_overflow(9, 1024, (1025,))            # 9 * 2^20 * 2^40 > 2^63
    check_overflow(7, 1024, (1025,))


def _evaluate_module():
    sys.path.insert(0, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts"))
    try:
        import evaluate
    finally:
        sys.path.pop(0)
    return evaluate


def test_cli_parses_scale_options(tmp_path):
    ev = _evaluate_module()
    base = ["--truth", "t", "--method", "x=y", "--mask", "m", "--output", "o"]
    d = ev.parse_args(base)
    assert d.scale is None and tuple(d.scales) == (1, 3, 5, 9, 17, 33, 65)
    a = ev.parse_args(base + ["--scale", str(tmp_path), "--scales", "2", "4", "8"])
    assert a.scale == str(tmp_path) and a.scales == [2, 4, 8] and a.mode == "radar"
    with pytest.raises(SystemExit):
        ev.parse_args(base + ["--scale", "s", "--mode", "gauge"])
    with pytest.raises(SystemExit):
        ev.parse_args(base + ["--scale", "s", "--scales"] + [str(i) for i in range(1, 18)])
    ev.parse_args(base + ["--mode", "gauge"])                # without --scale the mode is exp1's business


def test_cli_scale_output_layout(tmp_path):
    from p2igan_bench.evaluation import scale_lines, write_scale_outputs
    m = {"gan": {"FSS": {"thr_0.5": {"n_1": 0.25, "n_3": 1 / 3}, "thr_2": {"n_1": float("nan"), "n_3": 1.0}},
                 "useful_scale": {"thr_0.5": None, "thr_2": 3}, "LSD": 1.5, "HF_ratio": 0.5, "spectrum": [4.0, 2.0, 1.0],
                 "truth_spectrum": [4.0, 3.0, 2.0], "wavelength_px": [4.0, 2.0], "frames": 3, "frames_skipped": 1},
         "idw": {"FSS": {"thr_0.5": {"n_1": 0.5, "n_3": 0.75}, "thr_2": {"n_1": 0.0, "n_3": 0.125}},
                 "useful_scale": {"thr_0.5": 3, "thr_2": None}, "LSD": 6.0, "HF_ratio": 0.01, "spectrum": [4.0, 1.0, 0.1],
                 "truth_spectrum": [4.0, 3.0, 2.0], "wavelength_px": [4.0, 2.0], "frames": 3, "frames_skipped": 1}}
    assert scale_lines(m)[:5] == ["FSS_gan_thr0.5_n1: 0.250000", "FSS_gan_thr0.5_n3: 0.333333", "FSS_gan_thr2_n1: nan",
                                  "FSS_gan_thr2_n3: 1.000000", "LSD_gan: 1.500000"]
    write_scale_outputs(str(tmp_path), m)
    assert (tmp_path / "metrics.txt").read_text().splitlines() == scale_lines(m)
    assert (tmp_path / "metrics.json").read_text() == json.dumps(m, indent=2, sort_keys=True)
    z = np.load(tmp_path / "scale_data.npz")
    assert z["methods"].tolist() == ["gan", "idw"] and z["gan/scales"].tolist() == [1, 3] and z["gan/thresholds"].tolist() == [0.5, 2.0]
    assert z["idw/fss"].tolist() == [[0.5, 0.75], [0.0, 0.125]] and z["gan/useful_scale"].tolist() == [-1, 3]
    assert z["idw/spectrum"].tolist() == [4.0, 1.0, 0.1]
    pytest.importorskip("matplotlib")
    assert (tmp_path / "scale_panels.pdf").read_bytes()[:4] == b"%PDF"


def test_scale_abi_is_declared_bound_and_documented():
    from p2igan_bench import _hip, ops
    hdr = open(os.path.join(ROOT, "include", "p2i_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = ("p2i_scale_fss", "p2i_scale_fss_merge", "p2i_scale_dft_rows", "p2i_scale_dft_cols", "p2i_scale_rings",
             "p2i_scale_spectrum_merge")
    for n in names:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _hip.SIGNATURES, n
        assert f"`{n}`" in doc, n
    import ctypes
    lib = ctypes.CDLL(_hip.lib_path())
    for n in names:
        assert hasattr(lib, n), n
    for macro, val in (("P2I_SCALE_MAX_SCALES", ops.SCALE_MAX_SCALES), ("P2I_SCALE_LDS_CROP", ops.SCALE_LDS_CROP),
                       ("P2I_SCALE_MAX_CROP", ops.SCALE_MAX_CROP)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == val
    mk = open(os.path.join(ROOT, "p2i-gan-benchmark_amd", "csrc", "Makefile")).read()
    assert "eval_scale.hip" in mk and re.search(r"eval_scale\.o: FLAGS \+= -ffp-contract=off", mk)


def test_seeded_inputs_are_what_the_gpu_tests_assume():
    """1 - 5 % of the pixels reach 2 mm/h, and no spectrum bin is small against bin 0: the GPU test's LSD bound needs every bin
    >= 1e-6 of bin 0 (a per-bin error of 1e-10 of bin 0 is then 1e-4 relative, 4.3e-4 dB); held here with a factor 100 to spare."""
    for S in (8, 27, 128):
        g = scale_ref.field(100 + S, 5, S, S)
        frac = float((scale_ref.transform(g) >= 2.0).mean())
        assert 0.01 <= frac <= 0.05, (S, frac)
        for x in (g, scale_ref.smoother(g)):
            sp, _, skipped = scale_ref.spectra(scale_ref.transform(x), scale_ref.transform(g))
            assert skipped == 0 and sp.min() >= 1e-4 * sp[0], (S, sp.min() / sp[0])
