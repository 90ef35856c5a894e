"""tests/ens_ref.py, the numpy restatement of the ensemble scores, pinned against closed forms and hand cases (no GPU)."""
import math

import numpy as np

import ens_ref as er
import prob_ref as pr


def _field(x):
    """M values as members [M, 1, 1, 1]."""
    return np.asarray(x, np.float64).reshape(-1, 1, 1, 1)


def test_crps_is_the_integral_of_the_squared_cdf_difference():
    rng = np.random.default_rng(7)
    for M in (1, 2, 3, 8, 33):
        for _ in range(5):
            x = rng.normal(10.0, 4.0, M)
            x[rng.random(M) < 0.3] = 0.0                 # ties among the members
            for y in (0.0, float(rng.normal(10.0, 4.0)), float(x[0])):
                crps = er.point_scores(x, y)[0]
                assert abs(crps - er.crps_integral(x, y)) <= 1e-12 * max(1.0, crps), (M, x, y)
                s = er.ens_sums(_field(x), np.full((1, 1, 1), y))
                assert abs(s["crps"] - crps) <= 1e-12 * max(1.0, crps)


def test_one_member():
    crps, fair, mean, s2, b, k = er.point_scores([3.5], 1.25)
    assert crps == 2.25 and math.isnan(fair) and math.isnan(s2) and mean == 3.5 and (b, k) == (0, 0)
    sc = er.ens_scores(er.ens_sums(_field([3.5]), np.full((1, 1, 1), 1.25)), 1)
    assert sc["CRPS"] == 2.25 and sc["MAE"] == 2.25
    assert all(math.isnan(sc[key]) for key in ("CRPS_fair", "mean_var", "spread_skill_ratio"))
    e = er.energy_frames(np.full((1, 1, 2, 2), 3.5), np.full((1, 2, 2), 1.25))
    assert e[0, 0] == 4 and e[0, 1] == 4.5 and math.isnan(e[0, 2])        # |X - y| = sqrt(4 * 2.25^2)


def test_energy_score_of_one_pixel_is_the_crps():
    rng = np.random.default_rng(8)
    for M in (2, 5, 16):
        x, y = rng.normal(0.0, 3.0, M), 0.7
        crps, fair = er.point_scores(x, y)[:2]
        e = er.energy_frames(_field(x), np.full((1, 1, 1), y))
        assert e[0, 0] == 1
        assert abs(e[0, 1] - crps) <= 1e-12 * abs(crps) and abs(e[0, 2] - fair) <= 1e-12 * abs(fair)


def test_energy_score_of_identical_members():
    rng = np.random.default_rng(9)
    x, y = rng.normal(5.0, 2.0, (1, 2, 6, 7)), rng.normal(5.0, 2.0, (2, 6, 7))
    e = er.energy_frames(np.repeat(x, 4, axis=0), y)
    for t in range(2):
        d = math.sqrt(float(np.sum((x[0, t] - y[t]) ** 2)))
        assert e[t, 0] == 42 and abs(e[t, 1] - d) <= 1e-12 * d and abs(e[t, 2] - d) <= 1e-12 * d and abs(e[t, 3] - d) <= 1e-12 * d


def test_variogram_score_is_zero_for_the_truth():
    rng = np.random.default_rng(10)
    y = rng.gamma(0.6, 14.0, (2, 9, 11))
    v = er.variogram_frames(np.repeat(y[None], 4, axis=0), y)
    assert np.all(v[:, :, 0] == 0.0)                     # (a + a + a + a) / 4 is a exactly
    v3 = er.variogram_frames(np.repeat(y[None], 3, axis=0), y)
    assert np.all(v3[:, :, 0] <= 99 * (4.0 * 2.0 ** -52) ** 2)       # (a + a + a) / 3 rounds: at most 99 pairs, sqrt <= 16, 2 ulp each
    assert v[0, 0, 1] == 9 * 10 and v[0, 1, 1] == 8 * 11 and v[0, 3, 1] == 8 * 10          # (0, 1), (1, 0), (1, -1)
    assert v[0, 12, 1] == 9 * 3 and v[0, 13, 1] == 1 * 11 and v[0, 15, 1] == 1 * 3         # (0, 8), (8, 0), (8, -8)
    assert er.variogram_scores(v)["VS"] == 0.0
    w = er.variogram_frames(np.repeat(y[None], 3, axis=0) + rng.normal(0, 1, (3, 2, 9, 11)), y)
    assert np.all(w[:, :, 0] > 0.0)


def test_tie_rule_hand_case():
    """y = 0 and three of five members are 0: b = 0, k = 3; 2^32 = 4 * 2^30, so bins 0-3 get 2^30 each and no remainder is left."""
    x = [0.0, 2.0, 0.0, 0.0, 5.0]
    assert er.point_scores(x, 0.0)[4:] == (0, 3)
    assert er.tie_shares(0, 3, 5) == [1 << 30] * 4 + [0, 0]
    s = er.ens_sums(_field(x), np.zeros((1, 1, 1)))
    assert s["rank"].tolist() == [1 << 30] * 4 + [0, 0]
    # k + 1 = 3 does not divide 2^32: the remainder 1 goes to bin b
    assert er.tie_shares(1, 2, 5) == [0, (1 << 32) // 3 + 1, (1 << 32) // 3, (1 << 32) // 3, 0, 0]
    assert sum(er.tie_shares(1, 2, 5)) == 1 << 32


def test_box_values():
    a = np.arange(2 * 5 * 7, dtype=np.float64).reshape(2, 5, 7)
    sel = np.ones((5, 7), bool)
    sel[0:2, 2:4] = False                                # box (0, 1) of size 2 has no selected pixel
    sel[2, 0] = False
    v, has = er.box_values(a, sel, 2)
    assert v.shape == (2, 2, 3) and has.tolist() == [[True, False, True], [True, True, True]]
    assert v[0, 0, 0] == (0 + 1 + 7 + 8) / 4 and v[0, 1, 0] == (15 + 21 + 22) / 3 and v[1, 1, 2] == 35 + (18 + 19 + 25 + 26) / 4


def test_gaussian_ensembles_fair_crps_and_rank_histogram():
    """Calibrated Gaussian ensembles: the fair CRPS is an unbiased estimate of the Gaussian's closed-form CRPS, the plain one is
    not, and the truth's rank is uniform.  The standard error is that of the mean per-point difference to the closed form, from the
    same sample.  With this seed: fair 0.31 SE away, plain 12.50 SE away, chi^2 20.59 against the bound M + 6 sqrt(2 M) = 49.94."""
    rng = np.random.default_rng(2024)
    M, n = 16, 4096
    mu, sigma = rng.normal(20.0, 5.0, n), rng.uniform(1.0, 6.0, n)
    y = rng.normal(mu, sigma)
    x = rng.normal(mu, sigma, (M, n))
    fair = np.empty(n)
    plain = np.empty(n)
    hist = [0] * (M + 1)
    for i in range(n):
        plain[i], fair[i], _, _, b, k = er.point_scores(x[:, i], y[i])
        hist = [h + v for h, v in zip(hist, er.tie_shares(b, k, M))]
    closed = np.mean(pr.crps_plain(mu, sigma, y))
    d_fair, d_plain = fair - pr.crps_plain(mu, sigma, y), plain - pr.crps_plain(mu, sigma, y)
    se_fair, se_plain = d_fair.std(ddof=1) / math.sqrt(n), d_plain.std(ddof=1) / math.sqrt(n)
    z_fair, z_plain = abs(d_fair.mean()) / se_fair, abs(d_plain.mean()) / se_plain
    counts = np.array(hist, np.float64) / er.UNIT
    chi2 = float(np.sum((counts - n / (M + 1)) ** 2 / (n / (M + 1))))
    print(f"closed {closed:.6f} fair {fair.mean():.6f} ({z_fair:.2f} SE) plain {plain.mean():.6f} ({z_plain:.2f} SE) chi2 {chi2:.2f}")
    assert z_fair <= 6.0
    assert z_plain > 6.0
    assert chi2 <= M + 6.0 * math.sqrt(2.0 * M)
    # the vectorised sums give the same means
    s = er.ens_sums(x.reshape(M, 1, 1, n), y.reshape(1, 1, n))
    assert abs(s["crps_fair"] / n - fair.mean()) <= 1e-12 * fair.mean() and abs(s["crps"] / n - plain.mean()) <= 1e-12 * plain.mean()
    assert s["rank"].tolist() == hist
