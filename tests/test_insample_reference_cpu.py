"""Pins tests/insample_reference.py (the longdouble yardstick of test_insample_kernels_gpu.py)
without a GPU:

* against the reference-run goldens, rounded to double, within the bar the suite's CPU tests
  already give a float64 restatement on the same golden (test_optim_cpu.py / test_insample_cpu.py;
  optim_garch's `ll` is held bit-equal there for the oracle, which a higher-precision value
  cannot be -- its relative bar is test_insample_cpu.py's 1e-12);
* against the float64 oracle on exactly the inputs the GPU tests use, |oracle - ref| <=
  1e-14 * scale.  Measured on the CPU this suite was written on (max over the cases below):
      GARCH(p, q) log-likelihood, 16 orders, N = 96     2.3e-16 * scale
      GARCH(p, q) forecast, 16 orders, n_in = 40        1.7e-16 relative
      MSM log-likelihood, k = 1 .. 7, N = 64            7.3e-16 * scale
      MSM marginals / densities, k = 7 (host float64)   9.0e-16 relative
      UKF log-likelihood, 4 rows, N = 64                5.2e-16 * scale, state paths 6.8e-15 absolute
  so 1e-14 leaves a >= 10x margin, and the device bars (1e-12 * scale; MSM 1e-11) are bars a
  float64 implementation can meet: the oracle meets them 100x over;
* the edge inputs take the branch they are meant to take.
"""
import numpy as np
import pytest

import insample_reference as R
from conftest import load_golden

ORACLE_BAR = 1e-14


def _f64(x):
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------- reference-run goldens
def test_reference_garch_loglik_matches_golden():
    z = load_golden("optim_garch")
    for (p, q), row, want in zip(z["ll_pq"], z["ll_rows"], z["ll"]):
        ll, _, _ = R.garch_loglik_pq(z["returns"], row[0], row[1:1 + p], row[1 + p:1 + p + q])
        np.testing.assert_allclose(_f64(ll), want, rtol=1e-12, err_msg=f"GARCH({p},{q})")


def test_reference_garch_forecast_matches_golden():
    z = load_golden("optim_garch_pq")
    s, n_in = z["returns"], int(z["n_in"])
    for i, (p, q) in enumerate(z["orders"]):
        w = z["params"][i]
        got = [R.garch_forecast_pq(s[t:t + n_in], w[0], w[1:p + 1], w[p + 1:p + 1 + q])[0]
               for t in range(z["forecasts"].shape[1])]
        np.testing.assert_allclose(_f64(got), z["forecasts"][i], rtol=1e-14, err_msg=f"GARCH({p},{q})")


def test_reference_msm_loglik_matches_golden():
    z = load_golden("optim_msm_ll")
    got = [R.msm_loglik(z["returns"], int(z["k"]), *row)[0] for row in z["rows"]]
    np.testing.assert_allclose(_f64(got), z["ll"], rtol=1e-12)


def test_reference_msm_marginals_match_golden():
    z = load_golden("optim_msm_marg")
    for row, mw, dw in zip(z["rows"], z["marginals"], z["densities"]):
        m, d = R.msm_marginals(z["returns"], int(z["k"]), *row)
        np.testing.assert_allclose(_f64(m), mw, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(_f64(d), dw, rtol=1e-12, atol=1e-300)


def test_reference_ukf_matches_golden():
    z = load_golden("optim_ukf")
    for (a, l, q), llw, stw in zip(z["rows"], z["ll"], z["states"]):
        ll, _, st = R.ukf_filter(z["returns"], a, l, q)
        np.testing.assert_allclose(_f64(ll), llw, rtol=1e-12)
        np.testing.assert_allclose(_f64(st), stw, rtol=1e-11, atol=1e-13)


def test_reference_ndtr_matches_scipy():
    """The one special function the module implements itself, against scipy's float64 ndtr across
    both of its branches.  scipy's tail is exp(-x^2 / 2) of a ROUNDED x^2 / 2, a relative error
    of up to (x^2 / 2) eps on scipy's side: 4e-15 at |x| = 6, 1e-13 at |x| = 30 -- hence the
    two bars (4x and 3x that)."""
    from scipy.special import ndtr
    x = np.concatenate((np.linspace(-6, 6, 2401), [-1.5, -1.4142135623730951, 1.4142135623730951, 0.0, 1e-300]))
    np.testing.assert_allclose(_f64(R.ndtr(x)), ndtr(x), rtol=1.6e-14, atol=0)
    x = np.linspace(-30, 30, 601)
    np.testing.assert_allclose(_f64(R.ndtr(x)), ndtr(x), rtol=3e-13, atol=0)


# --------------------------------------------------- the float64 oracle on the GPU tests' inputs
@pytest.mark.parametrize("p,q", R.GARCH_ORDERS)
def test_oracle_garch_within_1e14_of_reference(p, q):
    from oracle.optim import garch_forecast_pq, garch_loglik_pq
    r = R.garch_returns()
    for row in R.garch_rows(p, q):
        w, al, be = row[0], row[1:1 + p], row[1 + p:]
        ll, scale, floored = R.garch_loglik_pq(r, w, al, be)
        ratio = abs(garch_loglik_pq(r, w, al, be) - ll) / scale
        print(f"garch_loglik ({p},{q}) |oracle - ref| / scale = {float(ratio):.2e}")
        assert floored == 0 and ratio <= ORACLE_BAR
        f, _ = R.garch_forecast_pq(r[:40], w, al, be)
        rel = abs(garch_forecast_pq(r[:40], w, al, be) - f) / f
        print(f"garch_forecast ({p},{q}) relative = {float(rel):.2e}")
        assert rel <= ORACLE_BAR


@pytest.mark.parametrize("k", range(1, 8))
def test_oracle_msm_loglik_within_1e14_of_reference(k):
    from oracle.forecast import msm_loglik
    r = R.msm_returns()
    for row in R.msm_rows(k):
        ll, scale = R.msm_loglik(r, k, *row)
        ratio = abs(msm_loglik(r, k, *row) - ll) / scale
        print(f"msm_loglik k={k} |oracle - ref| / scale = {float(ratio):.2e}")
        assert np.isfinite(_f64(ll)) and ratio <= ORACLE_BAR


def test_host_msm_marginals_k7_within_1e14_of_reference():
    from copula_var.insample import msm_marginals_densities
    r, row = R.msm_returns(), R.msm_rows(7)[0]
    m, d = R.msm_marginals(r, 7, *row)
    mh, dh, _ = msm_marginals_densities(r, 7, *row)
    rel = max(float(np.max(np.abs(mh - m) / m)), float(np.max(np.abs(dh - d) / d)))
    print(f"msm_marginals k=7 max relative = {rel:.2e}")
    assert rel <= ORACLE_BAR


def test_oracle_ukf_within_1e14_of_reference():
    """State paths: |oracle - ref| <= 1e-13, the absolute part of the device bar (states are
    ~ -4.5, one float64 rounding of them is 9e-16; measured 6.8e-15)."""
    from oracle.optim import ukf_filter_batch
    r = R.ukf_returns()
    ll_o, st_o = ukf_filter_batch(r, R.UKF_ROWS)
    for b, (a, l, q) in enumerate(R.UKF_ROWS):
        ll, scale, st = R.ukf_filter(r, a, l, q)
        ratio, dst = abs(ll_o[b] - ll) / scale, np.max(np.abs(st_o[b] - st))
        print(f"ukf row {b} |oracle - ref| / scale = {float(ratio):.2e}, states {float(dst):.2e}")
        assert ratio <= ORACLE_BAR and dst <= 1e-13


# --------------------------------------------------------------- the edges land where meant
@pytest.mark.parametrize("p,q", R.EDGE_ORDERS)
def test_garch_edge_inputs_take_their_branch(p, q):
    from oracle.optim import garch_loglik_pq
    r = R.garch_floor_returns()
    row = R.garch_floor_row(p, q)
    ll, scale, floored = R.garch_loglik_pq(r, row[0], row[1:1 + p], row[1 + p:])
    assert floored == R.GARCH_N - 1 == 95                       # the floor binds at every step
    assert abs(garch_loglik_pq(r, row[0], row[1:1 + p], row[1 + p:]) - ll) <= ORACLE_BAR * scale
    row = R.garch_nonstationary_row(p, q)
    assert row[1:].sum() > 1 and R.garch_sigma2_0(row[0], row[1:1 + p], row[1 + p:]) < 0
    r = R.garch_returns()
    ll, scale, floored = R.garch_loglik_pq(r, row[0], row[1:1 + p], row[1 + p:])
    assert np.isfinite(_f64(ll))                                # evaluated from the negative start, not rejected
    assert abs(garch_loglik_pq(r, row[0], row[1:1 + p], row[1 + p:]) - ll) <= ORACLE_BAR * scale


def test_garch_single_term_series():
    """N = max(p, q) + 1: one summed term, so |LL| = scale exactly.  The oracle stays within
    1e-14 * scale here too, with less room: measured 3.8e-15 at (1,1), where log(2 pi s2) and
    r^2 / s2 are each O(1) and cancel to a term of 6e-3 -- the scale counts summed terms, not
    the parts inside one."""
    from oracle.optim import garch_loglik_pq
    worst = 0.0
    for p, q in R.GARCH_ORDERS:
        r = R.garch_returns()[:max(p, q) + 1]
        for row in R.garch_rows(p, q):
            ll, scale, _ = R.garch_loglik_pq(r, row[0], row[1:1 + p], row[1 + p:])
            assert abs(ll) == scale > 0
            worst = max(worst, float(abs(garch_loglik_pq(r, row[0], row[1:1 + p], row[1 + p:]) - ll) / scale))
    print(f"garch one term max |oracle - ref| / scale = {worst:.2e}")
    assert worst <= ORACLE_BAR


def test_ukf_zero_return_fails():
    R_ = R.ukf_failure_series()
    rows = R.ukf_batch_rows(65)
    for b in R.UKF_FAIL_ROWS:
        assert R_[b, R.UKF_FAIL_STEP] == 0.0 and R.ukf_filter(R_[b], *rows[b]) is None
    assert R.ukf_filter(R_[1], *rows[1]) is not None


@pytest.mark.parametrize("k", [1, 4])
def test_msm_spike_series_is_dead(k):
    from copula_var.insample import msm_marginals_densities
    r = R.msm_returns()
    rows = R.msm_dead_rows(k, r)
    for b, row in enumerate(rows):
        ll, _ = R.msm_loglik(r, k, *row)
        assert (ll == -np.inf) == (b in (1, 4))
    with pytest.raises(FloatingPointError):
        R.msm_marginals(r, k, *rows[1])
    with pytest.raises(FloatingPointError):
        msm_marginals_densities(r, k, *rows[1])                 # the float64 host restatement agrees
