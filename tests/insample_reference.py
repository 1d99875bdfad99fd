"""Extended-precision restatements of the in-sample likelihood operations,
the yardstick of tests/test_insample_kernels_gpu.py, pinned without a GPU by
tests/test_insample_reference_cpu.py -- TEST INFRASTRUCTURE ONLY.

Every function works in numpy.longdouble throughout (parameters, returns, pi, exp / log /
sqrt): the x87 64-bit-mantissa type, eps 1.08e-19, ~3.5 digits beyond float64, so against a
float64 result its own rounding is negligible and the difference IS the float64 side's error.
Each returns the value together with its scale, the sum of the absolute values of the summed
terms: |result - ref| <= c * scale is a forward-error bound even when the terms change sign,
which a relative bar on the sum is not.

The float64 inputs convert exactly; the recursions are the oracle's, statement for statement
(oracle/optim.py, oracle/forecast.py, copula_var/insample.py).  Two places are float64 by
contract, not by convenience:
  * the GARCH floor is the float64 constant 1e-7 the reference and the kernels compare with;
  * an MSM normaliser counts as 0 when it ROUNDS to 0 in float64.  The reference's filter
    raises at scale == 0 and the kernel returns -inf there because float64 underflowed; a
    density of 1e-670 is an ordinary longdouble number, so the test on the raw value would
    never fire for the inputs the contract is about.

The second half holds the inputs the CPU and the GPU tests share (fixed default_rng seeds), so
both sides evaluate exactly the same arrays.
"""
import itertools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not the 64-bit-mantissa extended type on this platform"

PI = 4 * np.arctan(LD(1))
SQRT2 = np.sqrt(LD(2))
SQRT_PI = np.sqrt(PI)
SQRT_2PI = np.sqrt(2 * PI)
GARCH_FLOOR = LD(1e-7)                       # the float64 constant epsilon of garch/estimation.py


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


# ----------------------------------------------------------------------------- GARCH
def garch_sigma2_0(omega, alpha, beta):
    """sigma2[0] = omega / (1 - sum(alpha) - sum(beta)), unclamped (negative for a non-stationary row)."""
    alpha, beta = np.atleast_1d(_ld(alpha)), np.atleast_1d(_ld(beta))
    return LD(omega) / (1 - np.sum(alpha) - np.sum(beta))


def _garch_sigma2(r, omega, alpha, beta):
    n, p, q = r.size, alpha.size, beta.size
    s2 = np.zeros(n, dtype=LD)
    s2[0] = garch_sigma2_0(omega, alpha, beta)
    floored = 0
    for t in range(1, n):
        v = LD(omega)
        for i in range(min(p, t)):
            v += alpha[i] * (r[t - i - 1] ** 2)
        for j in range(min(q, t)):
            v += beta[j] * s2[t - j - 1]
        floored += int(v < GARCH_FLOOR)
        s2[t] = max(v, GARCH_FLOOR)
    return s2, floored


def garch_loglik_pq(r, omega, alpha, beta):
    """oracle/optim.py:garch_loglik_pq line by line: unclamped sigma2[0], max(., 1e-7) after, the
    chopped max(p, q) prefix.  -> (LL, scale = 0.5 sum_t |log(2 pi s2_t) + r_t^2 / s2_t|,
    number of steps t = 1 .. n-1 whose variance hit the floor)."""
    r, alpha, beta = _ld(r), np.atleast_1d(_ld(alpha)), np.atleast_1d(_ld(beta))
    s2, floored = _garch_sigma2(r, omega, alpha, beta)
    m = max(alpha.size, beta.size)
    terms = np.log(2 * PI * s2[m:]) + (r[m:] ** 2) / s2[m:]
    return -0.5 * np.sum(terms), 0.5 * np.sum(np.abs(terms)), floored


def garch_forecast_pq(window, omega, alpha, beta):
    """oracle/optim.py:garch_forecast_pq: sqrt(omega + sum(alpha * r[-p:]**2) + sum(beta * s2[-q:])),
    alpha_1 with the OLDEST of the last p returns.  -> (sigma forecast, scale of the radicand)."""
    r, alpha, beta = _ld(window), np.atleast_1d(_ld(alpha)), np.atleast_1d(_ld(beta))
    s2, _ = _garch_sigma2(r, omega, alpha, beta)
    ta, tb = alpha * r[-alpha.size:] ** 2, beta * s2[-beta.size:]
    return np.sqrt(LD(omega) + np.sum(ta) + np.sum(tb)), abs(LD(omega)) + np.sum(np.abs(ta)) + np.sum(np.abs(tb))


# ------------------------------------------------------------------------------- MSM
def _msm_model(k, m0, sig, b, gamma):
    """Transition matrix and vol states of oracle/forecast.py:msm_transition / msm_vol_states."""
    m0, sig, b, gamma = LD(m0), LD(sig), LD(b), LD(gamma)
    M = np.array(list(itertools.product([m0, 2 - m0], repeat=k)), dtype=LD)
    gamma_k = 1 - (1 - gamma) ** (b ** np.arange(k).astype(LD))
    p = 1 - gamma_k / 2
    A = np.prod(np.where(M[:, None, :] == M[None, :, :], p, 1 - p), axis=2)
    vs = np.array([np.sqrt(np.prod(M[i])) * sig for i in range(M.shape[0])], dtype=LD)
    return A, vs


def _cond(r, vs):
    return (1 / (vs[None, :] * SQRT_2PI)) * np.exp(-0.5 * (r[:, None] / vs[None, :]) ** 2)


def _is_zero64(x):
    return not (np.float64(x) > 0.0)


def msm_loglik(r, k, m0, sig, b, gamma):
    """The Hamilton filter of oracle/forecast.py:msm_loglik.  -> (LL, scale = sum_i |log term_i|);
    LL is -inf where a term is <= 0 or a normaliser is 0 (in float64, see the module docstring):
    the oracle raises on a zero normaliser, the kernel's contract is -inf."""
    r = _ld(r)
    A, vs = _msm_model(k, m0, sig, b, gamma)
    cond = _cond(r, vs)
    prev = np.full(vs.size, 1 / LD(vs.size))
    L, scale = LD(0), LD(0)
    for i in range(r.size):
        pr = (A @ prev) * cond[i]
        sc = np.sum(pr)                                       # = dot(A @ probs[i - 1], cond[i]), the term of step i
        if _is_zero64(sc):
            return -np.inf, scale
        if i >= 1:
            L += np.log(sc)
            scale += abs(np.log(sc))
        prev = pr / sc
    return L, scale


def ndtr(a):
    """Standard normal CDF in longdouble: erf's all-positive series below |a| / sqrt 2 = 1, the
    erfc continued fraction beyond (relative accuracy in both tails, as scipy's ndtr has)."""
    a = np.asarray(a, dtype=LD)
    x = a / SQRT2
    z = np.abs(x)
    zs = np.minimum(z, 1)                                     # erf(z) = 2/sqrt(pi) e^{-z^2} sum 2^n z^(2n+1) / (2n+1)!!
    term, tot = zs.copy(), zs.copy()
    for n in range(80):
        term = term * (2 * zs * zs) / (2 * n + 3)
        tot = tot + term
    erf_small = 2 / SQRT_PI * np.exp(-zs * zs) * tot
    zl = np.maximum(z, 1)                                     # erfc(z) = e^{-z^2} / sqrt(pi) / (z + (1/2) / (z + 1 / (z + ...)))
    f = zl.copy()
    for n in range(600, 0, -1):
        f = zl + (LD(n) / 2) / f
    erfc_large = np.exp(-zl * zl) / (SQRT_PI * f)
    small = 0.5 + 0.5 * np.sign(x) * erf_small
    large = np.where(x > 0, 1 - 0.5 * erfc_large, 0.5 * erfc_large)
    return np.where(z < 1, small, large)


def msm_marginals(r, k, m0, sig, b, gamma):
    """copula_var/insample.py:msm_marginals_densities: marg[i-1] = sum_s prob[i][s] Phi(r[i-1] / vs_s),
    dens[i-1] = sum_s prob[i][s] pdf(r[i-1]; vs_s), i = 1 .. N-1.  -> (marginals, densities); raises
    FloatingPointError on a zero normaliser as the host restatement does (all terms are
    non-negative, so each value is its own scale)."""
    r = _ld(r)
    A, vs = _msm_model(k, m0, sig, b, gamma)
    cond = _cond(r, vs)
    probs = np.zeros((r.size, vs.size), dtype=LD)
    prev = np.full(vs.size, 1 / LD(vs.size))
    for i in range(r.size):
        pr = (A @ prev) * cond[i]
        sc = np.sum(pr)
        if _is_zero64(sc):
            raise FloatingPointError(f"MSM filter: zero likelihood at step {i}")
        prev = pr / sc
        probs[i] = prev
    cm = ndtr(r[:, None] / vs[None, :])
    return np.sum(probs[1:] * cm[:-1], axis=1), np.sum(probs[1:] * cond[:-1], axis=1)


# ------------------------------------------------------------------------------- UKF
def ukf_filter(r, a, l, q, alpha=1.6, beta=2.0, kappa=1.75):
    """oracle/forecast.py:ukf_run with init (l, q), one series.  -> (LL, scale = sum_t |log Z_t|,
    state path (N,)), or None on Z <= 0 or Z < 1e-10 or a NaN (estimate.py:219-220, :270-271)."""
    w = _ld(r)
    a, l, q, alpha, beta, kappa = LD(a), LD(l), LD(q), LD(alpha), LD(beta), LD(kappa)
    Ld = 2
    lam = (alpha ** 2) * (Ld + kappa) - Ld
    wm = np.full(2 * Ld + 1, 1 / (2 * (Ld + lam)), dtype=LD)
    wc = wm.copy()
    wm[0] = lam / (Ld + lam)
    wc[0] = wm[0] + (1 - alpha ** 2 + beta)
    wm2 = np.full(Ld + 1, 1 / (2 * (Ld + lam)), dtype=LD)
    wm2[0] = lam / (Ld + lam)
    phi = np.sqrt(Ld + lam)
    x, var = l, q
    LL, scale = LD(0), LD(0)
    state = np.zeros(w.size, dtype=LD)
    X11 = np.array([0, 0, phi, 0, -phi], dtype=LD)
    for t in range(w.size):
        d = var + LD(1e-8) if var <= 0 else var
        c0 = np.sqrt(d)
        X10 = np.array([x, x + phi * c0, x, x - phi * c0, x], dtype=LD)
        X = a * (X10 - l) + l + q * X11
        xmean = np.sum(X * wm)
        diff = X - xmean
        sP = np.sqrt(np.sum(diff * wc * diff))
        X2 = np.array([xmean, xmean + phi * sP, xmean - phi * sP], dtype=LD)
        eta = w[t] / np.exp(X2)
        h = ((1 / SQRT_2PI) * np.exp(-0.5 * eta ** 2)) * np.abs(eta)
        Z = np.sum(wm2 * h)
        if Z <= 0 or Z < LD(1e-10):
            return None
        mean = np.sum((wm2 * X2 * h) / Z)
        var = np.sum(wm2 * ((h / Z) * (X2 - mean) ** 2))
        if np.isnan(mean) or np.isnan(var) or np.isnan(Z):
            return None
        state[t] = mean
        LL += np.log(np.abs(Z))
        scale += abs(np.log(np.abs(Z)))
        x = mean
    return LL, scale, state


# ================================================================== shared test inputs
GARCH_ORDERS = [(p, q) for p in range(1, 5) for q in range(1, 5)]
GARCH_N, MSM_N, UKF_N, BOUNDARY_N = 96, 64, 64, 32
EDGE_ORDERS = [(1, 1), (2, 3), (4, 4)]


def garch_returns(n=GARCH_N):
    """Order-1 returns for omega = 0.05 rows (unconditional variance 0.06 .. 0.25)."""
    return 0.5 * np.random.default_rng(9601).standard_normal(n)


def garch_rows(p, q, n=3):
    """omega = 0.05, coefficients uniform in (0.02, 0.8 / (p + q)): stationary, sum < 0.8."""
    rng = np.random.default_rng(100 + p * 10 + q)
    return np.column_stack((np.full(n, 0.05), rng.uniform(0.02, 0.8 / (p + q), size=(n, p + q))))


def garch_floor_returns(n=GARCH_N):
    return garch_returns(n) * 1e-5


def garch_floor_row(p, q):
    """(1e-9, 0.05, 0.1) at (1,1); the same sums spread over the lags: every variance < 1e-7."""
    return np.concatenate(([1e-9], np.full(p, 0.05 / p), np.full(q, 0.1 / q)))


def garch_nonstationary_row(p, q):
    """(0.05, 0.7, 0.5) at (1,1); sum(alpha) + sum(beta) = 1.2 > 1, so sigma2[0] = -0.25."""
    return np.concatenate(([0.05], np.full(p, 0.7 / p), np.full(q, 0.5 / q)))


def garch11_rows(n):
    rng = np.random.default_rng(1111)
    return np.column_stack((np.full(n, 0.05), rng.uniform(0.02, 0.4, size=(n, 2))))


def msm_returns(n=MSM_N):
    return np.random.default_rng(6401).standard_normal(n)


def msm_rows(k, n=5):
    """Rows (m0, sigma, b, gamma) spanning m0 in (0.2, 0.9), b in (1.5, 6), gamma in (0.05, 0.95):
    each parameter an independently shuffled even grid over its range."""
    rng = np.random.default_rng(700 + k)
    grid = lambda lo, hi: rng.permutation(np.linspace(lo, hi, n + 2)[1:-1])
    return np.column_stack((grid(0.2, 0.9), grid(0.7, 1.4), grid(1.5, 6.0), grid(0.05, 0.95)))


def msm_batch_rows(n, seed=77):
    rng = np.random.default_rng(seed)
    return np.column_stack((rng.uniform(0.2, 0.9, n), rng.uniform(0.7, 1.4, n), rng.uniform(1.5, 6.0, n),
                            rng.uniform(0.05, 0.95, n)))


def msm_dead_rows(k, r):
    """Six rows; rows 1 and 4 have sigma = max|r| / 80 and m0 = 0.8, so the largest return sits at
    >= 80 / 1.2^(k/2) >= 55 sigma of every state (k <= 4) and every density underflows float64."""
    rows = msm_batch_rows(6, seed=90 + k)
    rows[[1, 4], 0] = 0.8
    rows[[1, 4], 1] = float(np.max(np.abs(r))) / 80.0
    return rows


def ukf_returns(n=UKF_N, seed=6402):
    """Returns of order 0.012 = exp(-4.4), the scale of the UKF goldens."""
    return 0.012 * np.random.default_rng(seed).standard_normal(n)


UKF_ROWS = np.array([[0.97, -4.5, 0.15], [0.99, -4.3, 0.1], [0.6, -4.7, 0.3], [0.9, -4.5, 0.05]])


def ukf_batch_rows(n):
    rng = np.random.default_rng(333)
    return np.column_stack((rng.uniform(0.6, 0.999, n), rng.uniform(-4.8, -4.2, n), rng.uniform(0.05, 0.3, n)))


def ukf_series_per_row(b, n, seed=6500):
    return 0.012 * np.random.default_rng(seed).standard_normal((b, n))


UKF_FAIL_ROWS, UKF_FAIL_STEP = (0, 31, 64), 20


def ukf_failure_series(b=65, n=UKF_N):
    """One series per row; rows 0, 31 and 64 hold an exact 0.0 at step 20 (eta = 0 -> Z = 0)."""
    R = ukf_series_per_row(b, n, seed=6501)
    R[list(UKF_FAIL_ROWS), UKF_FAIL_STEP] = 0.0
    return R
