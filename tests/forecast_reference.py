"""Extended-precision restatements of the per-date forecast stage (cvq_msm_filter,
cvq_msm_tables, cvq_sigma_tables of csrc/cvq_forecast.hip), the yardstick of
tests/test_forecast_kernels_gpu.py, pinned without a GPU by tests/test_forecast_reference_cpu.py
-- TEST INFRASTRUCTURE ONLY.

Everything is numpy.longdouble, built on the pieces of tests/insample_reference.py (the MSM model,
the conditional densities, the GARCH(p, q) forecast, the UKF pass); the recursions are the
oracle's (oracle/forecast.py), statement for statement.  As there, an MSM normaliser counts as 0
when it ROUNDS to 0 in float64: that is when the reference's filter raises and the kernels flag.

The comparison rule (check_tiers).  Components of the filtered probabilities, of fbs and of pi
span 1e-1 down to below float64's range, so one rtol does not fit; the project's two existing
bars are tiered by the size of the reference value:
    ref >= 1e-30            relative error <= 1e-12   (TABLE_RTOL of test_gpu_parity.py: what a solve can feel)
    1e-200 <= ref < 1e-30   relative error <= 1e-10   (the goldens' filtered_probs bar)
    ref < 1e-200            value <= 2e-200           (float64 underflows here: no relative claim)
Every element falls in exactly one tier and is checked there.

The second half holds the inputs the CPU and the GPU tests share (fixed default_rng seeds).
"""
import functools

import numpy as np

from insample_reference import LD, UKF_ROWS, _cond, _ld, _msm_model, garch_forecast_pq, ukf_filter  # noqa: F401

TOP_FLOOR, MID_FLOOR = LD("1e-30"), LD("1e-200")
TOP_BAR, MID_BAR, BOTTOM_CAP = 1e-12, 1e-10, 2e-200
SCAN_B, SCAN_C = 16, 8                       # steps per block, blocks per superblock (CVQ_SCAN_B / _C)


# ------------------------------------------------------------------------------- MSM
def msm_window_probs(rc, n_in, k, m0, sig, b, gamma):
    """oracle/forecast.py:msm_filtered_probs in longdouble: the filtered state probabilities at the
    end of each rolling window rc[t:t + n_in], every window started from the uniform vector and
    all T = len(rc) - n_in + 1 windows advanced together.  -> (T, 2**k).  Raises
    FloatingPointError when a normaliser rounds to 0 in float64 (calc_prob.py:64-65)."""
    r = _ld(rc)
    A, vs = _msm_model(k, m0, sig, b, gamma)
    S = vs.size
    T = r.size - n_in + 1
    cond_all = _cond(r, vs)                                    # cond_all[i] = the densities of return i
    prev = np.full((T, S), 1 / LD(S))
    At = np.ascontiguousarray(A.T)
    for i in range(n_in):
        cond = cond_all[i:i + T]                               # step i of window t is return t + i
        tp = prev @ At                                         # calc_prob.py:56-57
        prob = tp * cond
        scale = prob.sum(axis=1, keepdims=True)
        if np.any(~(scale.astype(np.float64) > 0.0)):
            raise FloatingPointError("MSM Bayes update normaliser is 0 (calc_prob.py:64-65)")
        prev = prob / scale
    return prev


def collapse(probs, state_map, q):
    """sum_forecast_by_state (msm_estimation.py:205-248) for one asset with a given state -> unique
    vol map: (T, S) -> (T, q), each unique vol the sum of its states in state order (Q14)."""
    probs, state_map = np.asarray(probs, dtype=LD), np.asarray(state_map)
    out = np.zeros((probs.shape[0], q), dtype=LD)
    for s in range(probs.shape[1]):
        out[:, state_map[s]] += probs[:, s]
    return out


def combinations(fbs):
    """forecast_combinations (msm_estimation.py:392-418): the xy-meshgrid product order, (T, dim, q)
    -> (T, q**dim).  2-D: l = a q + b -> f0[a] f1[b]; 3-D: the permuted order of quirk Q7."""
    fbs = np.asarray(fbs, dtype=LD)
    T, dim, q = fbs.shape
    out = np.zeros((T, q ** dim), dtype=LD)
    for n in range(T):
        rows = [fbs[n, d, :] for d in range(dim)]
        comb = np.array(np.meshgrid(*rows)).T.reshape(-1, dim)
        out[n] = np.prod(comb, axis=1)
    return out


# ------------------------------------------------------------------------------- UKF
def ukf_forecast(window, a, l, q):
    """exp of the LAST step's predicted mean (kalman_mean_reverting/forecast.py:12, quirk Q19), or
    None on the failure rule (any step's Z <= 0 or < 1e-10, the last one included).  The predicted
    mean of step t is sum_i wm_i (a (X10_i - l) + l + q X11_i) over the sigma points of
    oracle/forecast.py:ukf_run; the +-phi columns carry equal weights and sum(wm) = 1, so it is
    a (x_{t-1} - l) + l exactly, x_{t-1} the previous step's filtered state (l before step 0)."""
    res = ukf_filter(window, a, l, q)
    if res is None:
        return None
    state = res[2]
    x = state[-2] if state.size >= 2 else LD(l)
    return np.exp(LD(a) * (x - LD(l)) + LD(l))


# ------------------------------------------------------- the scan filter's window geometry
def scan_middle_class(t, n_in, N):
    """How the full blocks strictly between the first and the last block of window [t, t + n_in)
    fall into superblocks (B = 16 steps per block, C = 8 blocks per superblock, N // B full blocks
    in the series) -> (class, number of stored factors that cross them):
      ("none", 0)          no full block in between
      ("prefix", 1)        they start a superblock: one superblock prefix product
      ("suffix", 1)        they end one (or the series' last, partial one): one suffix product
      ("loose", n)         n blocks inside one superblock, touching neither end: n block products
      ("several", pieces)  they span `pieces` superblocks: a suffix, pieces - 2 whole ones, a prefix
    Used only to assert that the test shapes visit every class."""
    e = t + n_in - 1
    lo_b, hi_b = t // SCAN_B + 1, e // SCAN_B - 1
    if lo_b > hi_b:
        return ("none", 0)
    nfull = N // SCAN_B
    sa, sb = lo_b // SCAN_C, hi_b // SCAN_C
    if sa != sb:
        return ("several", sb - sa + 1)
    if lo_b == sa * SCAN_C:
        return ("prefix", 1)
    if hi_b == min(sa * SCAN_C + SCAN_C, nfull) - 1:
        return ("suffix", 1)
    return ("loose", hi_b - lo_b + 1)


def scan_classes(n_in, T):
    """The classes a (n_in, T) call visits: every window (narrow scan, k <= 4) -- the wide scan
    (k = 5, 6) classifies each group of 16 windows by its first one, a subset of these."""
    N = n_in + T - 1
    return {scan_middle_class(t, n_in, N) for t in range(T)}


# ------------------------------------------------------------------- the comparison rule
def tier_errors(got, ref):
    """-> dict: per tier the element count and the measured figure (largest relative error; for
    the bottom tier the largest device value)."""
    got = np.asarray(got, dtype=np.float64).astype(LD).ravel()
    ref = np.asarray(ref, dtype=LD).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    top, bot = ref >= TOP_FLOOR, ref < MID_FLOOR
    mid = ~top & ~bot
    rel = np.abs(got - ref) / np.where(bot, LD(1), ref)
    fig = lambda m, v: float(np.max(v[m])) if m.any() else 0.0
    return dict(n=(int(top.sum()), int(mid.sum()), int(bot.sum())),
                top=fig(top, rel), mid=fig(mid, rel), bottom=fig(bot, got))


def check_tiers(name, got, ref):
    """Print the measured figures, then hold every element to its tier's requirement."""
    got = np.asarray(got, dtype=np.float64)
    m = tier_errors(got, ref)
    print(f"MEASURED {name}: top {m['top']:.2e} ({m['n'][0]}), middle {m['mid']:.2e} ({m['n'][1]}), "
          f"bottom max {m['bottom']:.2e} ({m['n'][2]})")
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), name
    assert m["top"] <= TOP_BAR, (name, "top tier", m)
    assert m["mid"] <= MID_BAR, (name, "middle tier", m)
    assert m["bottom"] <= BOTTOM_CAP, (name, "bottom tier", m)
    return m


# ================================================================== shared test inputs
BASE_ROW = (0.45, 1.2, 3.0, 0.3)                        # (m0, sigma, b, gamma)
ASSET_ROWS = ((0.45, 1.2, 3.0, 0.3), (0.55, 0.95, 2.2, 0.45), (0.35, 1.5, 4.0, 0.15))
ASSET_ROWS_K7 = ((0.6, 1.2, 3.0, 0.3), (0.7, 0.95, 2.2, 0.45), (0.65, 1.5, 4.0, 0.15))


def base_row(k):
    return (0.6,) + BASE_ROW[1:] if k == 7 else BASE_ROW


def asset_rows(k, dim):
    """Per-asset rows that differ in all four parameters (m0 nearer 1 at k = 7, as the base row)."""
    return (ASSET_ROWS_K7 if k == 7 else ASSET_ROWS)[:dim]


def plain_series(n, seed):
    return 1.1 * np.random.default_rng(seed).standard_normal(n)


def spiky_series(n, seed, sig):
    """The plain series with max(2, n // 20) positions (chosen by the same generator) set to
    +-10 sig, and an exact zero return next to a spike in the middle: components of the filtered
    vector fall through the whole float64 range and below it."""
    rng = np.random.default_rng(seed)
    x = 1.1 * rng.standard_normal(n)
    m = max(2, n // 20)
    pos = rng.choice(n, size=m, replace=False)
    x[pos] = rng.choice([-1.0, 1.0], size=m) * (10 * sig)
    x[n // 2] = 0.0
    x[n // 2 + 1] = 10 * sig
    return x


def series(kind, n, seed, sig):
    return plain_series(n, seed) if kind == "plain" else spiky_series(n, seed, sig)


SERIES_KINDS = ("plain", "spiky")
FILTER_SHAPES = ((1, 5), (7, 19), (8, 19), (9, 19), (32, 130))        # (n_in, T) of cvq_msm_filter
STEP_SHAPES_EDGE_K = ((5, 19), (33, 17), (300, 40))                    # k = 1, 7 (k = 7, n_in = 300: T = 8)
STEP_SHAPES_MID_K = ((1, 5), (32, 33))                                 # k = 2 .. 6, n_in <= 32
SCAN_SHAPES = ((33, 17), (49, 130), (161, 40), (300, 40), (70, 1))     # N % 16 = 1, 2, 8, 3, 6; T % 16 != 0


def step_shapes(k):
    if k in (1, 7):
        return tuple((n, 8 if (k == 7 and n == 300) else T) for n, T in STEP_SHAPES_EDGE_K)
    return STEP_SHAPES_MID_K


def asset_series(kind, n_in, T, k, dim):
    """rc (N, dim), rows: the returns and per-asset parameters of a tables call (seed 4000 + 10 N + d)."""
    N = n_in + T - 1
    rows = asset_rows(k, dim)
    rc = np.column_stack([series(kind, N, 4000 + 10 * N + d, rows[d][1]) for d in range(dim)])
    return rc, rows


@functools.lru_cache(maxsize=None)
def _window_probs_cached(kind, N, seed, n_in, k, row):
    p = msm_window_probs(series(kind, N, seed, row[1]), n_in, k, *row)
    p.setflags(write=False)
    return p


def asset_window_probs(kind, n_in, T, k, d, row):
    """The longdouble filter of asset d of asset_series(kind, n_in, T, k, .), computed once per process."""
    N = n_in + T - 1
    return _window_probs_cached(kind, N, 4000 + 10 * N + d, n_in, k, tuple(row))


def popcount_map(k):
    """The state -> unique-vol map of sum_forecast_by_state for m0 != 1: vol sqrt(m0^a (2 - m0)^(k - a))
    sigma grows with the number of 2 - m0 factors, the popcount of the state index (m0 < 1)."""
    return np.array([bin(s).count("1") for s in range(1 << k)], dtype=np.int32)


def tables_reference(kind, n_in, T, k, dim, state_map=None, q=None):
    """-> (fbs (T, dim, q), pi (T, q**dim)) in longdouble for asset_series(kind, n_in, T, k, dim)."""
    rows = asset_rows(k, dim)
    if state_map is None:
        state_map, q = np.tile(popcount_map(k), (dim, 1)), k + 1
    fbs = np.stack([collapse(asset_window_probs(kind, n_in, T, k, d, rows[d]), state_map[d], q)
                    for d in range(dim)], axis=1)
    return fbs, combinations(fbs)
