"""The backtest statistics of copula_var.backtest on cases with closed-form answers (no GPU):
Kupiec, Christoffersen, Acerbi-Szekely Z2, Berkowitz, the pinball score, NaN handling."""
import math

import numpy as np
import pytest
from scipy import stats

from copula_var import backtest as B


def _hits(n, x):
    h = np.zeros(n, dtype=bool)
    h[:x] = True
    return h


# ------------------------------------------------------------------ hits
def test_hits_is_strict_and_drops_nan():
    r = np.array([-1.0, -2.0, -2.0, np.nan, -3.0, 0.5])
    v = np.array([-2.0, -2.0, -1.5, -2.0, np.nan, 1.0])
    k = B.hits(r, v)
    assert k["hit"].tolist() == [False, False, True, True]       # -2 < -2 is no hit; equal is not below
    assert k["keep"].tolist() == [True, True, True, False, False, True]
    assert (k["n"], k["x"], k["dropped"]) == (4, 2, 2)
    with pytest.raises(ValueError):
        B.hits(r, v[:-1])


# ------------------------------------------------------------------ Kupiec
def test_kupiec_closed_forms():
    k = B.kupiec_pof(_hits(200, 10), 0.05)                        # x / n == alpha
    assert k["statistic"] == pytest.approx(0.0, abs=1e-12) and k["p_value"] == pytest.approx(1.0)
    assert (k["n"], k["x"]) == (200, 10)
    n, alpha = 250, 0.05
    k0 = B.kupiec_pof(_hits(n, 0), alpha)                         # 0 ln 0 = 0
    assert k0["statistic"] == pytest.approx(-2.0 * n * math.log(1.0 - alpha), rel=1e-13)
    assert k0["p_value"] == pytest.approx(stats.chi2.sf(k0["statistic"], 1))
    kn = B.kupiec_pof(_hits(40, 40), alpha)                       # every date a hit
    assert kn["statistic"] == pytest.approx(-2.0 * 40 * math.log(alpha), rel=1e-13)
    x = 21
    lr = -2.0 * ((n - x) * math.log(1 - alpha) + x * math.log(alpha) - (n - x) * math.log(1 - x / n)
                 - x * math.log(x / n))
    assert B.kupiec_pof(_hits(n, x), alpha)["statistic"] == pytest.approx(lr, rel=1e-12)
    assert B.kupiec_pof(B.hits(np.r_[-np.ones(x), np.ones(n - x)], np.zeros(n)), alpha)["statistic"] == \
        pytest.approx(lr, rel=1e-12)                              # the hits() dict is accepted too
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            B.kupiec_pof(_hits(10, 1), bad)


# ------------------------------------------------------------------ Christoffersen
def test_christoffersen_hand_counted():
    h = np.array([0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0], dtype=bool)
    # pairs: 00 01 10 00 00 01 11 10 00 00 00
    n00, n01, n10, n11 = 6, 2, 2, 1
    alpha = 0.25                                                  # x / n = 3 / 12: LR_pof = 0
    c = B.christoffersen(h, alpha)
    assert (c["n00"], c["n01"], c["n10"], c["n11"]) == (n00, n01, n10, n11)
    pi, pi01, pi11 = 3 / 11, 2 / 8, 1 / 3
    l0 = 8 * math.log(1 - pi) + 3 * math.log(pi)
    l1 = n00 * math.log(1 - pi01) + n01 * math.log(pi01) + n10 * math.log(1 - pi11) + n11 * math.log(pi11)
    lr_ind = -2.0 * (l0 - l1)
    # by hand: l0 = 8 (-0.318454) + 3 (-1.299283) = -6.445479,
    # l1 = 6 (-0.287682) + 2 (-1.386294) + 2 (-0.405465) - 1.098612 = -6.408223
    assert lr_ind == pytest.approx(0.074510, abs=2e-6)
    assert c["lr_ind"] == pytest.approx(lr_ind, rel=1e-12)
    assert c["lr_pof"] == pytest.approx(0.0, abs=1e-12)
    assert c["lr_cc"] == pytest.approx(lr_ind, rel=1e-12, abs=1e-12)
    assert c["p_ind"] == pytest.approx(stats.chi2.sf(lr_ind, 1)) and c["p_cc"] == pytest.approx(stats.chi2.sf(lr_ind, 2))
    c5 = B.christoffersen(h, 0.05)
    assert c5["lr_cc"] == pytest.approx(B.kupiec_pof(h, 0.05)["statistic"] + lr_ind, rel=1e-12)


def test_christoffersen_zero_counts():
    """0 ln 0 = 0: no hit at all, and hits that never follow one another."""
    c = B.christoffersen(_hits(50, 0), 0.05)
    assert c["lr_ind"] == pytest.approx(0.0, abs=1e-12) and (c["n00"], c["n01"], c["n10"], c["n11"]) == (49, 0, 0, 0)
    h = np.zeros(20, dtype=bool)
    h[[3, 9, 15]] = True                                          # n11 = 0
    c = B.christoffersen(h, 0.05)
    assert (c["n00"], c["n01"], c["n10"], c["n11"]) == (13, 3, 3, 0)
    l0 = 16 * math.log(1 - 3 / 19) + 3 * math.log(3 / 19)
    l1 = 13 * math.log(13 / 16) + 3 * math.log(3 / 16)            # the n10 row: 3 ln 1 + 0 ln 0 = 0
    assert c["lr_ind"] == pytest.approx(-2.0 * (l0 - l1), rel=1e-12)
    assert np.isfinite(c["p_cc"])


# ------------------------------------------------------------------ Z2
def test_z2_zero_by_construction_and_negative():
    n, alpha = 100, 0.05
    var = np.full(n, -2.0)
    es = np.full(n, -2.5)
    r = np.zeros(n)
    r[:5] = -2.5                                                  # n alpha hits, each exactly the ES: sum r/es = 5
    z = B.acerbi_szekely_z2(r, var, es, alpha)
    assert z["statistic"] == pytest.approx(0.0, abs=1e-14) and (z["n"], z["x"], z["dropped"]) == (n, 5, 0)
    r[:5] = -5.0                                                  # every hit twice the ES
    z = B.acerbi_szekely_z2(r, var, es, alpha)
    assert z["statistic"] == pytest.approx(-1.0, rel=1e-14) and z["statistic"] < 0.0
    r[7], es[8] = np.nan, np.nan
    z = B.acerbi_szekely_z2(r, var, es, alpha)
    assert (z["n"], z["dropped"]) == (n - 2, 2)
    assert z["statistic"] == pytest.approx(1.0 - 10.0 / ((n - 2) * alpha), rel=1e-14)
    assert "p_value" not in z


# ------------------------------------------------------------------ Berkowitz
def _berkowitz_by_hand(u):
    z = stats.norm.ppf(np.clip(u, 1e-12, 1 - 1e-12))
    y, x = z[1:], z[:-1]
    rho, c = np.polyfit(x, y, 1)                                   # conditional least squares
    s = math.sqrt(float(np.mean((y - c - rho * x) ** 2)))
    l1 = float(np.sum(stats.norm.logpdf(y, loc=c + rho * x, scale=s)))
    l0 = float(np.sum(stats.norm.logpdf(y)))
    return -2.0 * (l0 - l1), c / (1 - rho), s, rho


def test_berkowitz_against_independent_likelihoods():
    x = np.random.default_rng(20240607).standard_normal(500)
    u = stats.norm.cdf(x)
    b = B.berkowitz(u)
    lr, mu, s, rho = _berkowitz_by_hand(u)
    assert b["statistic"] == pytest.approx(lr, rel=1e-9)
    assert (b["mu"], b["sigma"], b["rho"]) == pytest.approx((mu, s, rho), rel=1e-9, abs=1e-12)
    assert b["p_value"] == pytest.approx(stats.chi2.sf(lr, 3)) and b["p_value"] > 0.01
    assert (b["n"], b["dropped"]) == (500, 0)
    shifted = B.berkowitz(stats.norm.cdf(x + 1.0))
    assert shifted["p_value"] < 1e-6 and shifted["mu"] == pytest.approx(1.0, abs=0.15)


def test_berkowitz_nan_and_clip():
    x = np.random.default_rng(7).standard_normal(300)
    u = stats.norm.cdf(x)
    u2 = np.concatenate((u[:100], [np.nan, np.nan], u[100:]))
    a, b = B.berkowitz(u), B.berkowitz(u2)
    assert (b["n"], b["dropped"]) == (300, 2) and b["statistic"] == a["statistic"]
    u3 = u.copy()
    u3[[5, 50]] = 0.0, 1.0                                        # clipped to 1e-12 / 1 - 1e-12: finite
    c = B.berkowitz(u3)
    assert np.isfinite(c["statistic"]) and c["statistic"] == pytest.approx(_berkowitz_by_hand(u3)[0], rel=1e-9)
    assert np.isnan(B.berkowitz([0.5, np.nan])["statistic"])


# ------------------------------------------------------------------ pinball, table
def test_pinball():
    r = np.array([-3.0, 0.0, 1.0, np.nan])
    v = np.array([-2.0, -2.0, -2.0, -2.0])
    # (alpha - 1)(r - v) on the hit, alpha (r - v) otherwise
    want = (0.95 * 1.0 + 0.05 * 2.0 + 0.05 * 3.0) / 3
    p = B.pinball(r, v, 0.05)
    assert p["statistic"] == pytest.approx(want, rel=1e-14) and (p["n"], p["dropped"]) == (3, 1)


def test_backtest_table_collects_everything():
    rng = np.random.default_rng(3)
    n = 400
    r = rng.standard_normal(n)
    var = np.full(n, stats.norm.ppf(0.05))
    es = np.full(n, -stats.norm.pdf(stats.norm.ppf(0.05)) / 0.05)
    r[11], var[12] = np.nan, np.nan
    u = stats.norm.cdf(r)
    t = B.backtest_table(r, var, es=es, pit=u, alpha=0.05)
    k = B.hits(r, var)
    assert (t["n"], t["hits"], t["dropped"]) == (k["n"], k["x"], 2) and t["hits"] == int(np.nansum(r < var))
    assert t["kupiec"] == B.kupiec_pof(k, 0.05) and t["christoffersen"] == B.christoffersen(k, 0.05)
    assert t["z2"] == B.acerbi_szekely_z2(r, var, es, 0.05) and t["berkowitz"]["dropped"] == 1
    assert t["pinball"] == B.pinball(r, var, 0.05)
    assert t["kupiec"]["p_value"] > 0.01 and abs(t["z2"]["statistic"]) < 0.6
    bare = B.backtest_table(r, var)
    assert "z2" not in bare and "berkowitz" not in bare
    text = B.format_table(t, "x")
    assert f"hits {t['hits']} " in text and "Kupiec" in text and "Berkowitz" in text and "Z2" in text
