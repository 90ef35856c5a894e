"""Probabilistic verification on CPU: the numpy / scipy restatement (tests/prob_ref.py) against the definitions -- the CRPS forms
against numerical integration, their limits, calibration under sampling from the predictive distribution itself -- the host rules of
the product (thresholds on the pixel scale, record layout, derived scores, output files), the refusals of the two scripts and the
new ABI symbols."""
import json
import os
import re
import sys

import numpy as np
import pytest

import prob_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (mu, sigma, y): mu < 0, y == 0, a large sigma, y far in either tail, y == mu
TRIPLES = [(12.0, 3.0, 9.5), (12.0, 3.0, 0.0), (-4.0, 2.5, 0.0), (-4.0, 2.5, 1.75), (0.0, 1.0, 0.0), (0.5, 80.0, 30.0),
           (150.0, 60.0, 255.0), (3.0, 0.4, 7.0), (20.0, 5.0, 20.0), (-30.0, 8.0, 0.0), (2.0, 6.0, 0.25)]


@pytest.mark.parametrize("censor", (False, True))
def test_crps_forms_equal_the_integral(censor):
    """int (F - 1[x >= y])^2 dx by the trapezoid rule, split at the integrand's jumps (y, and 0 under censoring), at steps h =
    sigma / 4 and h / 2.  The bound is the rule's own: on a piece of length b - a the error is at most (b - a) h^2 / 12 max|f''|, and
    for f = (F - c)^2 with c in {0, 1}, f'' = 2 F'^2 + 2 (F - c) F'' where F' = phi / sigma <= 0.3990 / sigma and |F''| <=
    0.2420 / sigma^2 (phi's largest slope, at |z| = 1), so |f''| <= (2 * 0.3990^2 + 2 * 0.2420) / sigma^2 < 0.81 / sigma^2.  The
    tails beyond mu -+ 12 sigma hold less than Phi(-12)^2 sigma < 1e-60 sigma.  Halving the step must shrink the error, down to
    the rounding of the rule's own sum of length / h terms, length / h * eps * CRPS (reached where y lies so far out that the
    integrand's bump is smooth and whole inside one piece: the rule is then exact to rounding at either step)."""
    form = pr.crps_censored if censor else pr.crps_plain
    for mu, sigma, y in TRIPLES:
        want = float(form(mu, sigma, y))
        errs = []
        for h in (sigma / 4.0, sigma / 8.0):
            length = max(mu + 12.0 * sigma, y, 0.0) - min(mu - 12.0 * sigma, y, 0.0) + 2.0
            bound = length * h * h / 12.0 * 0.81 / (sigma * sigma)
            err = abs(pr.crps_numeric(mu, sigma, y, censor, h) - want)
            print(f"censor {censor} (mu, sigma, y) = ({mu}, {sigma}, {y}): CRPS {want:.9g}  step {h:.4g}  error {err:.3e}  bound {bound:.3e}")
            assert err <= bound, (mu, sigma, y, h, err, bound)
            errs.append(err)
        floor = length / (sigma / 8.0) * np.finfo(np.float64).eps * want
        assert errs[1] < errs[0] or errs[1] <= floor, (mu, sigma, y, errs, floor)


def test_censored_crps_tends_to_the_plain_one():
    """mu / sigma -> infinity: Phi(l), phi(l) and Phi(l sqrt 2) underflow to exactly 0 from l = -mu / sigma <= -40 on, which leaves
    the plain form's terms: equal up to the rounding of the two sums, a few ulp of the largest term."""
    for ratio in (40.0, 100.0, 1e4):
        for sigma, dz in ((0.5, -1.3), (3.0, 0.0), (20.0, 2.2)):
            mu = ratio * sigma
            y = mu + dz * sigma
            a, b = float(pr.crps_censored(mu, sigma, y)), float(pr.crps_plain(mu, sigma, y))
            assert abs(a - b) <= 4 * np.finfo(np.float64).eps * sigma * (abs(dz) + 1.0), (ratio, sigma, dz, a, b)
    # and well away from the limit the two differ: the atom at 0 matters
    assert abs(float(pr.crps_censored(1.0, 2.0, 0.5)) - float(pr.crps_plain(1.0, 2.0, 0.5))) > 0.05


def test_sigma_to_zero_gives_the_point_mass_rules():
    """X ~ max(0, N(mu, sigma^2)) lies within E|X - mu'| <= sigma sqrt(2 / pi) < sigma of the point mass at mu' = max(mu, 0) in mean
    absolute distance, and CRPS(F, y) = E|X - y| - E|X - X'| / 2, so |CRPS - |y - mu'|| < 2 sigma."""
    for mu, y in ((7.0, 9.5), (7.0, 2.0), (-3.0, 0.0), (-3.0, 4.0), (0.25, 0.0)):
        for sigma in (1e-3, 1e-6, 1e-9):
            for censor, form in ((True, pr.crps_censored), (False, pr.crps_plain)):
                if not censor and mu < 0:
                    continue
                point = abs(y - (max(mu, 0.0) if censor else mu))
                assert abs(float(form(mu, sigma, y)) - point) < 2.0 * sigma, (mu, y, sigma, censor)
    # every count and table of a tiny variance equals the sigma^2 == 0 rules' (no y == mu among these pixels)
    rng = np.random.default_rng(5)
    mu = rng.uniform(-5.0, 40.0, (2, 9, 9))
    y = np.maximum(0.0, mu + rng.normal(0.0, 6.0, mu.shape))
    y[np.abs(y - np.maximum(mu, 0.0)) < 1e-3] += 1.0
    kw = dict(thresholds=(0.5, 2.0, 8.0), sigma_edges=(0.5, 4.0))
    zero, tiny = pr.prob_sums(mu, 0.0, y, **kw), pr.prob_sums(mu, 1e-24, y, **kw)
    assert zero["n_zero_var"] == mu.size and tiny["n_zero_var"] == 0
    for k in ("n", "inside", "o", "sb_n", "rel_n", "rel_o", "pit"):
        assert np.array_equal(zero[k], tiny[k]), k
    for k in ("crps", "p", "brier", "rel_p"):
        assert np.all(np.abs(np.asarray(zero[k]) - np.asarray(tiny[k])) <= 2e-12 * mu.size), k
    assert np.all(zero["width"] == 0.0) and zero["z"] == 0.0 and zero["z2"] == 0.0
    # y == mu': u = 0.5, inside every interval, CRPS 0
    s = pr.prob_sums(np.array([[[3.0, -2.0]]]), 0.0, np.array([[[3.0, 0.0]]]), thresholds=(2.0,), pit_bins=20)
    assert s["crps"] == 0.0 and s["inside"].tolist() == [2, 2, 2, 2] and s["pit"][10] == 2.0 and s["pit"].sum() == 2.0


def test_calibration_when_truth_is_drawn_from_the_predictive():
    """y ~ max(0, N(mu, sigma^2)), n = 2 * 10^5, fixed seed, scored under censoring.
    PIT: the randomised PIT of a draw from the predictive itself is uniform, so its nb-bin histogram is multinomial with equal cells
    and Pearson's statistic is chi^2 with nb - 1 degrees of freedom.  The non-randomised weights are the conditional expectation of
    the randomised indicators given y; the statistic is convex in the histogram, so by Jensen its mean is no larger.  Bound: the
    chi^2_{nb-1} quantile exceeded with probability 1e-6.
    Coverage: for a pixel whose lower end mu - h sigma is positive the clamp does nothing and the closed interval holds y with the
    nominal probability exactly; over those pixels the hit count is binomial and must lie within 3 standard errors sqrt(L (1 - L) / m)
    of the nominal level L.  Where the lower end is clamped to 0 the atom y == 0 lies inside the closed interval and the exact
    coverage is Phi(h) = (1 + L) / 2 (or Phi(-mu / sigma), larger still, where the upper end is clamped too): over all pixels the
    hits are a sum of Bernoulli(c_i) with these c_i, and the count must lie within 3 standard errors sqrt(sum c_i (1 - c_i)) of
    sum c_i -- and cannot fall below the nominal level by more than 3 of its standard errors."""
    from scipy.special import ndtr, ndtri
    from scipy.stats import chi2
    rng = np.random.default_rng(20250)
    n, nb = 200000, 20
    mu = rng.uniform(-10.0, 30.0, (1, 1, n))
    sigma = rng.uniform(1.0, 15.0, (1, 1, n))
    y = pr.sample_censored(rng, mu, sigma)
    assert 0.1 < float((y == 0.0).mean()) < 0.5                   # the atom is well populated
    s = pr.prob_sums(mu, sigma * sigma, y, thresholds=(2.0,), pit_bins=nb, censor=True)
    assert s["n"] == n and abs(s["pit"].sum() - n) < 1e-6
    stat = float(((s["pit"] - n / nb) ** 2 / (n / nb)).sum())
    bound = float(chi2.isf(1e-6, nb - 1))
    print(f"PIT chi^2 {stat:.2f}  bound {bound:.2f}")
    assert stat <= bound
    for k, lev in enumerate(pr.DEFAULT_LEVELS):
        h = float(ndtri((1.0 + lev) / 2.0))
        lo, hi = mu - h * sigma, mu + h * sigma
        c = np.where(lo > 0.0, lev, np.where(hi > 0.0, ndtr(h), ndtr(-mu / sigma)))
        exp, se = float(c.sum()), float(np.sqrt((c * (1.0 - c)).sum()))
        free = lo > 0.0
        m = int(free.sum())
        hits_free = int(((y >= lo) & (y <= hi) & free).sum())
        print(f"level {lev}: coverage {s['inside'][k] / n:.5f} expected {exp / n:.5f} +- {3 * se / n:.5f};  unclamped {hits_free / m:.5f} "
              f"+- {3 * np.sqrt(lev * (1 - lev) / m):.5f} of {m}")
        assert abs(s["inside"][k] - exp) <= 3.0 * se
        assert abs(hits_free / m - lev) <= 3.0 * np.sqrt(lev * (1.0 - lev) / m)
        assert s["inside"][k] / n >= lev - 3.0 * np.sqrt(lev * (1.0 - lev) / n)
    # the plain Gaussian against its own draws: nominal everywhere
    yp = mu + sigma * rng.standard_normal(mu.shape)
    sp = pr.prob_sums(mu, sigma * sigma, yp, pit_bins=nb, censor=False)
    assert float(((sp["pit"] - n / nb) ** 2 / (n / nb)).sum()) <= bound
    for k, lev in enumerate(pr.DEFAULT_LEVELS):
        assert abs(sp["inside"][k] / n - lev) <= 3.0 * np.sqrt(lev * (1.0 - lev) / n)
    # the standardised error of a calibrated forecast: mean 0, variance 1 (the 4th moment of N(0, 1) is 3: var(z^2) = 2)
    assert abs(sp["z"] / n) <= 3.0 / np.sqrt(n) and abs(sp["z2"] / n - 1.0) <= 3.0 * np.sqrt(2.0 / n)


def test_pit_weights_of_the_atom():
    for nb in (1, 7, 20):
        for P0 in (0.0, 1e-300, 0.013, 0.05, 0.3 + 1e-12, 0.5, 0.999, 1.0):
            w = pr.pit_weights(P0, nb)
            assert abs(w.sum() - 1.0) <= 1e-12 and np.all(w >= 0.0)
            if P0 > 0.0:
                # the kernel's decomposition: m full bins of 1 / (nb P0) and the rest in bin m = min(floor(P0 nb), nb - 1)
                m = min(int(np.floor(P0 * nb)), nb - 1)
                dec = np.zeros(nb)
                dec[:m] = (1.0 / nb) / P0
                dec[m] = (P0 - m / nb) / P0
                assert np.all(np.abs(dec - w) <= 1e-12), (nb, P0)
            else:
                assert w[0] == 1.0


def test_pixel_threshold_inverts_the_transform():
    from p2igan_bench.evaluation import pixel_threshold, transform_mmhr
    for div3 in (True, False):
        for q in (0.04, 0.1, 0.5, 2.0, 8.0, 50.0, 200.0):
            x = pixel_threshold(q, div3)
            assert x == pytest.approx(float(pr.pixel_threshold(q, div3)), rel=1e-15)
            assert abs(float(transform_mmhr(x, div3)) - q) <= 1e-12 * q
            assert float(transform_mmhr(x * (1 + 1e-9) + 1e-9, div3)) >= q > float(transform_mmhr(x * (1 - 1e-9) - 1e-9, div3))
            assert float(pr.transform(x, div3)) == float(transform_mmhr(x, div3))
        floor = float(transform_mmhr(0.001, div3))
        for q in (0.0, -1.0, 0.036, floor, 200.0001, 1e9):
            with pytest.raises(ValueError, match="exceedance"):
                pixel_threshold(q, div3)


def _pack(s, lay):
    """prob_sums' output as the device would hold it: (F, I) of one record."""
    F, I = np.zeros(lay.nf), np.zeros(lay.ni, np.int64)
    F[:7] = [s["crps"], s["e"], s["ae"], s["e2"], s["s2"], s["z"], s["z2"]]
    for off, k in ((lay.f_w, "width"), (lay.f_p, "p"), (lay.f_br, "brier"), (lay.f_sv, "sb_s2"), (lay.f_se, "sb_e2")):
        F[off:off + len(s[k])] = s[k]
    I[:3] = [s["n"], s["n_skipped"], s["n_zero_var"]]
    for off, k in ((lay.i_in, "inside"), (lay.i_o, "o"), (lay.i_sn, "sb_n"), (lay.i_rn, "rel_n"), (lay.i_ro, "rel_o")):
        I[off:off + np.size(s[k])] = np.ravel(s[k])
    I[lay.i_pit:lay.i_pit + lay.NB] = np.rint(s["pit"] * 2.0 ** 32)
    I[lay.i_rp:lay.i_rp + lay.K * lay.RB] = np.rint(np.ravel(s["rel_p"]) * 2.0 ** 32)
    return F, I


def test_host_scores_equal_the_reference():
    from p2igan_bench.evaluation import prob_scores, unpack_record
    from p2igan_bench.evaluation.prob import _Layout
    rng = np.random.default_rng(9)
    mu = rng.uniform(-5.0, 60.0, (3, 8, 8))
    var = rng.uniform(0.1, 300.0, mu.shape)
    y = pr.sample_censored(rng, mu, np.sqrt(var) * 1.3)
    var[0, 0, :3] = np.nan
    var[1, 2, 2] = 0.0
    thr, lev, edges = (0.5, 2.0, 8.0), (0.5, 0.9), (1.0, 4.0, 16.0)
    s = pr.prob_sums(mu, var, y, thresholds=thr, levels=lev, sigma_edges=edges, pit_bins=12, rel_bins=5)
    lay = _Layout(3, 2, 3, 12, 5)
    assert (lay.nf, lay.ni) == (7 + 2 + 6 + 8, 3 + 2 + 3 + 24 + 4 + 45)
    got = prob_scores(unpack_record(*_pack(s, lay), lay), thr, lev, edges)
    want = pr.prob_scores(s, thr, lev, edges)
    assert want["n"] == 3 * 64 - 3 and want["n_skipped"] == 3 and want["n_zero_var"] == 1

    def same(a, b, path=""):
        if isinstance(b, dict):
            assert sorted(a) == sorted(b), path
            for k in b:
                same(a[k], b[k], f"{path}/{k}")
        elif isinstance(b, list):
            assert len(a) == len(b), path
            for i, (x, z) in enumerate(zip(a, b)):
                same(x, z, f"{path}[{i}]")
        elif isinstance(b, float) and np.isnan(b):
            assert np.isnan(a), path
        else:
            assert a == pytest.approx(b, rel=1e-12, abs=want["n"] * 2.0 ** -33), path
    same(got, want)
    # the prefix table: a weight at index i stands in every bin <= i
    F, I = _pack(s, lay)
    I[lay.i_pit:lay.i_pit + 12] = 0
    I[lay.i_pre + 4], I[lay.i_pre + 1], I[lay.i_pit + 5] = 3 << 32, 1 << 32, 2 << 32
    assert unpack_record(F, I, lay)["pit"].tolist() == [4.0, 4.0, 3.0, 3.0, 3.0, 2.0] + [0.0] * 6
    # the ROC area of a table that separates perfectly, and of one that says nothing
    from p2igan_bench.evaluation import roc_area
    assert roc_area([5, 0, 5], [0, 0, 5]) == 1.0 and roc_area([4, 4], [2, 2]) == 0.5 and np.isnan(roc_area([3, 3], [0, 0]))
    assert roc_area([4, 4], [2, 2]) == pr.roc_area([4, 4], [2, 2])


def test_refusals_come_before_the_gpu_check(monkeypatch):
    import torch
    from p2igan_bench import evaluation
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for kw, msg in ((dict(mode="satellite"), "Unknown mode"), (dict(thresholds=tuple(float(i + 1) for i in range(9))), "thresholds"),
                    (dict(thresholds=(0.01,)), "exceedance"), (dict(thresholds=(250.0,)), "exceedance"),
                    (dict(levels=tuple(0.1 * (i + 1) for i in range(9))), "levels"), (dict(levels=(1.0,)), "level"),
                    (dict(sigma_edges=tuple(range(1, 18))), "sigma_edges"), (dict(sigma_edges=(2.0, 1.0)), "ascending"),
                    (dict(pit_bins=65), "pit_bins"), (dict(rel_bins=0), "rel_bins"), (dict(mask=np.zeros((4, 4), bool)), "Mask shape")):
        with pytest.raises(ValueError, match=msg):
            evaluation.ProbEvaluator(16, **kw)


def test_everything_refuses_to_run_without_gpu(monkeypatch):
    import torch
    from p2igan_bench import evaluation
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="probabilistic verification runs on the GPU"):
        evaluation.ProbEvaluator(16)
    p, g = np.zeros((2, 16, 16), np.float32), np.zeros((2, 16, 16), np.uint8)
    with pytest.raises(RuntimeError, match="no GPU is visible"):
        evaluation.run_prob({"a": p}, {"a": p + 1}, g, None, "radar", 16)
    with pytest.raises(RuntimeError, match="no GPU is visible"):
        evaluation.run_prob_points(np.zeros(5), np.zeros(5), np.ones(5), 255.0)


def _script(name):
    sys.path.insert(0, os.path.join(ROOT, "p2i-gan-benchmark_amd", "scripts"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_evaluate_cli_parses_and_refuses(tmp_path, capsys):
    ev = _script("evaluate")
    base = ["--truth", "t", "--method", "krig=p.zarr", "--method", "gan=g.zarr", "--mask", "m", "--output", "o"]
    d = ev.parse_args(base)
    assert d.prob is None and d.variance == [] and tuple(d.levels) == (0.5, 0.8, 0.9, 0.95) and not d.no_censor
    a = ev.parse_args(base + ["--prob", str(tmp_path), "--variance", "krig=v.zarr", "--levels", "0.5", "0.99", "--no-censor"])
    assert a.prob == str(tmp_path) and a.variance == [("krig", "v.zarr")] and a.levels == [0.5, 0.99] and a.no_censor
    ev.parse_args(base + ["--prob", "d"])                                # dressed scores need no variance
    ev.parse_args(base + ["--thresholds", "0.01"])                       # without --prob the thresholds are exp1's business
    for extra, msg in ((["--prob", "d", "--variance", "idw=v.zarr"], "no --method gives"),
                       (["--variance", "krig=v.zarr"], "needs --prob"),
                       (["--prob", "d", "--variance", "krig=v.zarr", "--variance", "krig=w.zarr"], "repeat"),
                       (["--prob", "d", "--thresholds", "0.01", "2"], "exceedance"),
                       (["--prob", "d", "--thresholds", "2", "201"], "exceedance"),
                       (["--prob", "d", "--levels", "0.5", "1.0"], "level"),
                       (["--prob", "d", "--levels"] + ["0.5"] * 9, "1 to 8 levels"),
                       (["--prob", "d", "--variance", "krig"], "NAME=ZARR")):
        with pytest.raises(SystemExit):
            ev.parse_args(base + extra)
        assert msg in capsys.readouterr().err, extra
    ev.check_output_scale("krig", {"output_scale": 255.0}, {"output_scale": 255})
    ev.check_output_scale("krig", {}, {"output_scale": 1.0})
    with pytest.raises(ValueError, match="output_scale"):
        ev.check_output_scale("krig", {"output_scale": 255.0}, {"output_scale": 1.0})


def test_crossvalidate_prob_needs_a_variance(tmp_path):
    cv = _script("crossvalidate")
    from p2igan_bench.evaluation.loo import check_prob
    assert cv.parse_args(["--config", "c", "--output", "o"]).prob is False
    assert cv.parse_args(["--config", "c", "--output", "o", "--prob"]).prob is True
    for name, by_site, ok in (("idw", False, False), ("idw", True, False), ("kriging", False, True), ("kriging", True, True),
                              ("stkriging", True, True), ("localkriging", True, True), ("locallagkriging", True, True),
                              ("p2igan", False, False)):
        if ok:
            check_prob({"model": {"name": name}}, by_site)
        else:
            with pytest.raises(RuntimeError, match="has no variance"):
                check_prob({"model": {"name": name}}, by_site)
    cfg = tmp_path / "idw.json"
    cfg.write_text(json.dumps({"model": {"name": "idw"}, "seed": 1}))
    with pytest.raises(RuntimeError, match="--prob scores the predictive distribution"):
        cv.main(["--config", str(cfg), "--output", str(tmp_path / "out"), "--prob"])
    assert not (tmp_path / "out").exists()


def test_output_layout(tmp_path):
    from p2igan_bench.evaluation import prob_lines, write_prob_outputs
    rng = np.random.default_rng(2)
    mu = rng.uniform(0.0, 40.0, (2, 6, 6))
    y = pr.sample_censored(rng, mu, 5.0)
    thr = (0.5, 2.0)
    score = lambda v: pr.prob_scores(pr.prob_sums(mu, v, y, thresholds=thr), thr)      # noqa: E731
    res = {"krig": {"dressed": {**score(25.0), "sigma0_sq": 25.0, "sigma0_sq_in_sample": True}, "map": score(mu + 1.0),
                    "CRPSS_map_vs_dressed": 0.125}, "gan": {"dressed": {**score(30.0), "sigma0_sq": 30.0, "sigma0_sq_in_sample": True}}}
    lines = prob_lines(res)
    d = res["krig"]["dressed"]
    assert lines[0] == f"CRPS_krig_dressed: {d['CRPS']:.6f}"
    assert f"COV90_krig_map: {res['krig']['map']['coverage']['0.9']:.6f}" in lines
    assert f"BRIER_gan_dressed_thr0.5: {res['gan']['dressed']['exceedance']['thr_0.5']['brier']:.6f}" in lines
    assert "CRPSS_krig: 0.125000" in lines and not any(line.startswith("CRPSS_gan") for line in lines)
    assert f"NSKIPPED_krig_map: {res['krig']['map']['n_skipped']}" in lines and "NZEROVAR_gan_dressed: 0" in lines
    write_prob_outputs(str(tmp_path), res)
    assert (tmp_path / "metrics.txt").read_text().splitlines() == lines
    assert (tmp_path / "metrics.json").read_text() == json.dumps(res, indent=2, sort_keys=True)
    z = np.load(tmp_path / "prob_data.npz")
    assert z["entries"].tolist() == ["krig_dressed", "krig_map", "gan_dressed"]
    assert z["krig_map/pit"].shape == (20,) and abs(z["krig_map/pit"].sum() - 1.0) < 1e-12
    assert z["krig_map/levels"].tolist() == [0.5, 0.8, 0.9, 0.95] and z["gan_dressed/thresholds"].tolist() == [0.5, 2.0]
    assert z["krig_dressed/reliability_count"].shape == (2, 10) and z["krig_dressed/spread_skill_count"].sum() == 72
    assert z["gan_dressed/exceedance"].shape == (2, 5) and z["gan_dressed/scores"][0] == res["gan"]["dressed"]["CRPS"]
    pytest.importorskip("matplotlib")
    assert (tmp_path / "prob_panels.pdf").read_bytes()[:4] == b"%PDF"
    write_prob_outputs(str(tmp_path / "cv"), res, stem="prob", figure=False)
    assert sorted(os.listdir(tmp_path / "cv")) == ["prob.json", "prob.txt", "prob_data.npz"]


def test_prob_abi_is_declared_bound_and_documented():
    from p2igan_bench import _hip, ops
    hdr = open(os.path.join(ROOT, "include", "p2i_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = ("p2i_prob_record", "p2i_prob_accumulate", "p2i_prob_merge")
    import ctypes
    lib = ctypes.CDLL(_hip.lib_path())
    for n in names:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _hip.SIGNATURES, n
        assert f"`{n}`" in doc, n
        assert hasattr(lib, n), n
    for macro, val in (("P2I_PROB_MAX_LEVELS", ops.PROB_MAX_LEVELS), ("P2I_PROB_MAX_EDGES", ops.PROB_MAX_EDGES),
                       ("P2I_PROB_MAX_PIT_BINS", ops.PROB_MAX_PIT_BINS), ("P2I_PROB_MAX_REL_BINS", ops.PROB_MAX_REL_BINS),
                       ("P2I_PROB_WG_PIXELS", ops.PROB_WG_PIXELS)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == val
    mk = open(os.path.join(ROOT, "p2i-gan-benchmark_amd", "csrc", "Makefile")).read()
    assert "eval_prob.hip" in mk and re.search(r"eval_prob\.o: FLAGS \+= -ffp-contract=off", mk)
    # the host's record layout is the library's (p2i_prob_record needs no GPU)
    from p2igan_bench.evaluation.prob import _Layout
    for K, L, E, NB, RB in ((0, 0, 0, 1, 1), (4, 4, 12, 20, 10), (8, 8, 16, 64, 32), (1, 8, 1, 7, 32)):
        lay = _Layout(K, L, E, NB, RB)
        assert ops.prob_record(K, L, E, NB, RB) == (lay.nf, lay.ni)
    with pytest.raises(RuntimeError, match="p2i_prob_record"):
        ops.prob_record(9, 4, 12, 20, 10)
    for doc_name, what in (("DESIGN.md", "## 22."), ("README.md", "--prob"), ("profiles/README.md", "prob_bench")):
        assert what in open(os.path.join(ROOT, doc_name)).read(), (doc_name, what)


def test_seeded_gpu_cases_have_no_element_on_a_decision_edge():
    """tests/test_prob_gpu.py asserts exact counts: that needs every scored element further than 1e-9 from every decision edge in
    the reference, and the planted special pixels where that test expects them."""
    import test_prob_gpu as tg
    for name in tg.CASES:
        ref = tg.build(name)[4]
        assert ref["edge_count"] == 0, name
    assert pr.prob_sums(*tg._far_crop_values(), None, thresholds=tg.THR4)["edge_count"] == 0
    sp = tg.build("special_data")[4]
    assert (sp["n_zero_var"], sp["n_skipped"]) == (5, 150) and tg.build("special_data_plain")[4]["n_skipped"] == 149
    assert tg.build("select_1")[4]["n"] == 3 and tg.build("select_0")[4]["n"] == 0 and tg.build("all_skipped")[4]["n_skipped"] == 50
    big = tg.build("u8_f32_f32_radar_3wg")[4]
    assert big["sb_n"][0] > 0 and big["sb_n"][-1] > 0 and big["pit"].min() > 0         # under- and overflow sigma-bins are populated
