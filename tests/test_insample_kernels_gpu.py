"""The batched in-sample kernels of csrc/cvq_forecast.hip on the MI355X against
the longdouble restatements of tests/insample_reference.py -- every compiled instance, the
batch boundaries, the failure lanes, the GARCH floor / non-stationary branches and the
CVQ_MEM_DEVICE staging path.  The goldens stay pinned by test_optim_gpu.py / test_insample_gpu.py.

Bars.  Log-likelihoods: |device - ref| <= 1e-12 * scale (MSM: 1e-11), scale = sum |term_t|, so
the bar bounds the forward error even where the terms change sign.  Forecasts rtol 1e-13, UKF
state paths rtol 1e-11 + atol 1e-13, MSM marginals rtol 1e-12: the project's own bars against the
reference-run goldens.  Batched results are bit-equal to the same rows evaluated one at a time
(B = 1): a candidate's arithmetic does not depend on its neighbours.

Measured max |device - ref| / scale, from one run of this module on an MI355X (gfx950), beside
the float64 oracle's ratio on the same inputs (test_insample_reference_cpu.py, on a CPU):
                                              device      oracle
    k_garch_loglik_pq, 16 orders, N = 96      7.9e-16     2.3e-16
    k_garch_loglik_pq, N = max(p, q) + 1      3.8e-15     3.8e-15
    k_garch_loglik (1,1)                      1.5e-16     2.3e-16
    GARCH floor / non-stationary rows         3.3e-16     (<= 1e-14, asserted)
    k_garch_forecast_pq, 16 orders (relative) 1.7e-16     1.7e-16
    k_msm_loglik, k = 1 .. 7, N = 64          8.8e-16     7.3e-16
    k_msm_marginals<7> (relative)             1.0e-15     9.0e-16
    k_ukf_loglik / k_ukf_filter LL            7.2e-16     5.2e-16
    k_ukf_filter state path (absolute)        7.5e-15     6.8e-15
The bars are the project's, not these figures: one run does not license a tighter one.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import insample_reference as R

pytestmark = pytest.mark.gpu

LL_BAR, MSM_BAR = 1e-12, 1e-11


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


def _split(row, p):
    return row[0], row[1:1 + p], row[1 + p:]


def _check_ll(name, got, refs, bar):
    """refs: (value, scale, ...) per row.  Prints the measured ratio before asserting."""
    ratios = [abs(R.LD(g) - ref[0]) / ref[1] for g, ref in zip(got, refs)]
    print(f"MEASURED {name} max |device - ref| / scale = {float(max(ratios)):.2e}")
    assert len(got) == len(refs) and np.all(np.isfinite(got))
    assert all(x <= bar for x in ratios), (name, [float(x) for x in ratios])


# ------------------------------------------------------------------------------ GARCH
@pytest.mark.parametrize("p,q", R.GARCH_ORDERS)
def test_garch_loglik_pq_every_order(p, q):
    from copula_var import engine
    r, rows = R.garch_returns(), R.garch_rows(p, q)
    got = engine.garch_loglik_pq(r, p, q, rows)
    _check_ll(f"garch_loglik_pq ({p},{q})", got, [R.garch_loglik_pq(r, *_split(row, p)) for row in rows], LL_BAR)
    m = max(p, q)                                              # N = max(p, q) + 1: a single summed term
    one = engine.garch_loglik_pq(r[:m + 1], p, q, rows)
    _check_ll(f"garch_loglik_pq ({p},{q}) one term", one,
              [R.garch_loglik_pq(r[:m + 1], *_split(row, p)) for row in rows], LL_BAR)
    if (p, q) == (1, 1):                                       # the (1,1) entry point agrees
        g11 = engine.garch_loglik(r, rows)
        np.testing.assert_allclose(g11, got, rtol=1e-15)
        _check_ll("garch_loglik (1,1)", g11, [R.garch_loglik_pq(r, *_split(row, 1)) for row in rows], LL_BAR)


@pytest.mark.parametrize("p,q", R.GARCH_ORDERS)
def test_garch_forecast_pq_every_order(p, q):
    from copula_var import engine
    r, prm = R.garch_returns(), R.garch_rows(p, q)[0]
    worst = 0.0
    for n_in, T in ((40, 5), (max(p, q), 3)):                  # and the shortest window the entry point admits
        s = r[:n_in + T - 1]
        got = engine.garch_forecast_pq(s, n_in, p, q, prm)
        want = np.array([R.garch_forecast_pq(s[t:t + n_in], *_split(prm, p))[0] for t in range(T)])
        worst = max(worst, float(np.max(np.abs(got.astype(R.LD) - want) / want)))
        print(f"MEASURED garch_forecast_pq ({p},{q}) n_in={n_in} max relative = {worst:.2e}")
        assert got.shape == (T,)
        np.testing.assert_allclose(got, want.astype(np.float64), rtol=1e-13, atol=0, err_msg=f"n_in {n_in}")
        assert np.all(np.abs(got.astype(R.LD) - want) <= 1e-13 * want)
        if (p, q) == (1, 1):
            np.testing.assert_array_equal(got, engine.garch_forecast(s, n_in, *prm))


@pytest.mark.parametrize("p,q", R.EDGE_ORDERS)
def test_garch_floor_and_nonstationary_rows(p, q):
    """The max(sigma2, 1e-7) floor binding at every step, and a row with sigma2[0] < 0, which the
    likelihood evaluates as the reference does; the forecast entry points reject such a row."""
    from copula_var import engine
    cases = (("floor", R.garch_floor_returns(), R.garch_floor_row(p, q)),
             ("non-stationary", R.garch_returns(), R.garch_nonstationary_row(p, q)))
    for name, r, row in cases:
        ref = R.garch_loglik_pq(r, *_split(row, p))
        _check_ll(f"garch_loglik_pq ({p},{q}) {name}", engine.garch_loglik_pq(r, p, q, row[None, :]), [ref], LL_BAR)
        if (p, q) == (1, 1):
            _check_ll(f"garch_loglik (1,1) {name}", engine.garch_loglik(r, row[None, :]), [ref], LL_BAR)
    row, r = R.garch_nonstationary_row(p, q), R.garch_returns()
    with pytest.raises(ValueError, match="cvq_garch_forecast_pq"):
        engine.garch_forecast_pq(r[:44], 40, p, q, row)
    if (p, q) == (1, 1):
        with pytest.raises(ValueError, match="cvq_garch_forecast"):
            engine.garch_forecast(r[:44], 40, *row)


def test_forecast_entry_points_reject_an_empty_window():
    """n_in = 0 would have k_garch_forecast read w[n_in - 1] = w[-1], one double before the series
    (cvq_garch_forecast and cvq_ukf_forecast took any n_in; cvq_garch_forecast_pq and
    cvq_msm_filter already refused): rejected before any launch."""
    from copula_var import engine
    r = R.garch_returns()[:8]
    with pytest.raises(ValueError, match="n_in and T must be >= 1"):
        engine.garch_forecast(r, 0, 0.05, 0.1, 0.2)
    with pytest.raises(ValueError, match="n_in and T must be >= 1"):
        engine.ukf_forecast(R.ukf_returns()[:8], 0, 0.97, -4.5, 0.15)
    with pytest.raises(ValueError, match="cvq_garch_forecast_pq"):
        engine.garch_forecast_pq(r, 0, 1, 1, [0.05, 0.1, 0.2])


# -------------------------------------------------------------------------------- MSM
@pytest.mark.parametrize("k", range(1, 8))
def test_msm_loglik_every_k(k):
    from copula_var import engine
    r, rows = R.msm_returns(), R.msm_rows(k)
    got = engine.msm_loglik(r, k, rows)
    _check_ll(f"msm_loglik k={k}", got, [R.msm_loglik(r, k, *row) for row in rows], MSM_BAR)


def test_msm_marginals_k7():
    from copula_var import engine
    r, row = R.msm_returns(), R.msm_rows(7)[0]
    m, d = engine.msm_marginals(r, 7, *row)
    mr, dr = R.msm_marginals(r, 7, *row)
    rel = max(float(np.max(np.abs(m.astype(R.LD) - mr) / mr)), float(np.max(np.abs(d.astype(R.LD) - dr) / dr)))
    print(f"MEASURED msm_marginals k=7 max relative = {rel:.2e}")
    assert m.shape == d.shape == (R.MSM_N - 1,)
    np.testing.assert_allclose(m, mr.astype(np.float64), rtol=1e-12, atol=0)
    np.testing.assert_allclose(d, dr.astype(np.float64), rtol=1e-12, atol=0)


# -------------------------------------------------------------------------------- UKF
def test_ukf_against_reference():
    from copula_var import engine
    r, P = R.ukf_returns(), R.UKF_ROWS
    refs = [R.ukf_filter(r, *row) for row in P]
    ll, st = engine.ukf_filter(r, P)
    _check_ll("ukf_filter LL", ll, refs, LL_BAR)
    _check_ll("ukf_loglik", engine.ukf_loglik(r, P), refs, LL_BAR)
    want = np.array([ref[2] for ref in refs])
    print(f"MEASURED ukf_filter states max absolute = {float(np.max(np.abs(st.astype(R.LD) - want))):.2e}")
    np.testing.assert_allclose(st, want.astype(np.float64), rtol=1e-11, atol=1e-13)
    ll2, st2 = engine.ukf_filter(np.broadcast_to(r, (len(P), r.size)), P)        # one series per row: same pass
    np.testing.assert_array_equal(ll2, ll)
    np.testing.assert_array_equal(st2, st)


# ------------------------------------------------------------------- batch boundaries
@functools.lru_cache(maxsize=None)
def _singles(kind):
    """The rows of each boundary case evaluated one at a time (B = 1), once per module."""
    from copula_var import engine
    if kind == "garch_pq":
        r, rows = R.garch_returns(R.BOUNDARY_N), R.garch_rows(2, 2, 65)
        return r, rows, np.array([engine.garch_loglik_pq(r, 2, 2, row[None, :])[0] for row in rows])
    if kind == "garch11":
        r, rows = R.garch_returns(R.BOUNDARY_N), R.garch11_rows(257)
        return r, rows, np.array([engine.garch_loglik(r, row[None, :])[0] for row in rows])
    if kind in ("msm1", "msm4"):
        k, n = (1, 129) if kind == "msm1" else (4, 65)
        r, rows = R.msm_returns(R.BOUNDARY_N), R.msm_batch_rows(n, seed=70 + k)
        return r, rows, np.array([engine.msm_loglik(r, k, row[None, :])[0] for row in rows])
    if kind == "ukf_ll":
        r, rows = R.ukf_returns(R.BOUNDARY_N), R.ukf_batch_rows(65)
        return r, rows, np.array([engine.ukf_loglik(r, row[None, :])[0] for row in rows])
    per = kind == "ukf_per_row"
    assert per or kind == "ukf_shared"
    rows = R.ukf_batch_rows(65)
    r = R.ukf_series_per_row(65, R.BOUNDARY_N) if per else R.ukf_returns(R.BOUNDARY_N)
    one = [engine.ukf_filter(r[b:b + 1] if per else r, rows[b:b + 1]) for b in range(65)]
    return r, rows, (np.array([o[0][0] for o in one]), np.array([o[1][0] for o in one]))


@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_batch_boundary_garch_loglik_pq(B):
    from copula_var import engine
    r, rows, one = _singles("garch_pq")
    np.testing.assert_array_equal(engine.garch_loglik_pq(r, 2, 2, rows[:B]), one[:B])


@pytest.mark.parametrize("B", [255, 256, 257])
def test_batch_boundary_garch_loglik(B):
    from copula_var import engine
    r, rows, one = _singles("garch11")
    np.testing.assert_array_equal(engine.garch_loglik(r, rows[:B]), one[:B])


@pytest.mark.parametrize("k,B", [(1, 127), (1, 128), (1, 129), (4, 63), (4, 64), (4, 65)])
def test_batch_boundary_msm_loglik(k, B):
    from copula_var import engine
    r, rows, one = _singles(f"msm{k}")
    assert np.all(np.isfinite(one))
    np.testing.assert_array_equal(engine.msm_loglik(r, k, rows[:B]), one[:B])


@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_batch_boundary_ukf(B):
    from copula_var import engine
    r, rows, one = _singles("ukf_ll")
    np.testing.assert_array_equal(engine.ukf_loglik(r, rows[:B]), one[:B])
    for kind in ("ukf_shared", "ukf_per_row"):
        r, rows, (ll1, st1) = _singles(kind)
        assert np.all(ll1 != -1e10) and np.all(np.isfinite(st1))
        ll, st = engine.ukf_filter(r[:B] if kind == "ukf_per_row" else r, rows[:B])
        np.testing.assert_array_equal(ll, ll1[:B], err_msg=kind)
        np.testing.assert_array_equal(st, st1[:B], err_msg=kind)


# ---------------------------------------------------------------------- failure lanes
def test_ukf_failure_lanes():
    """A 0.0 return gives eta = 0, h = 0, Z = 0: the pass fails (estimate.py:219-220).  The failed
    columns of the time-major [N][B] path are NaN, LL is -1e10 exactly (optim/ukf.py tests
    `ll == -1e10`), and the neighbouring columns are untouched."""
    from copula_var import engine
    S, rows = R.ukf_failure_series(), R.ukf_batch_rows(65)
    ll, st = engine.ukf_filter(S, rows)
    dead = np.zeros(65, dtype=bool)
    dead[list(R.UKF_FAIL_ROWS)] = True
    assert np.all(ll[dead] == -1e10) and np.all(np.isnan(st[dead]))
    assert np.all(ll[~dead] != -1e10) and np.all(np.isfinite(st[~dead]))
    for b in np.flatnonzero(~dead):
        ll1, st1 = engine.ukf_filter(S[b:b + 1], rows[b:b + 1])
        assert ll[b] == ll1[0], b
        np.testing.assert_array_equal(st[b], st1[0], err_msg=f"row {b}")
    shared = R.ukf_returns().copy()
    shared[R.UKF_FAIL_STEP] = 0.0
    assert np.all(engine.ukf_loglik(shared, rows) == -1e10)
    ll_s, st_s = engine.ukf_filter(shared, rows)
    assert np.all(ll_s == -1e10) and np.all(np.isnan(st_s))


@pytest.mark.parametrize("k", [1, 4])
def test_msm_dead_lanes(k):
    """Rows 1 and 4: every state density of the largest return underflows to 0, the normaliser is
    0, the candidate is dead (-inf).  At k = 1 two candidates share a DPP quad: rows 0 and 5 are
    the quad partners of the dead rows and must not see their NaNs."""
    from copula_var import _native, engine
    r = R.msm_returns()
    rows = R.msm_dead_rows(k, r)
    got = engine.msm_loglik(r, k, rows)
    assert got[1] == -np.inf and got[4] == -np.inf
    for b in (0, 2, 3, 5):
        assert np.isfinite(got[b]) and got[b] == engine.msm_loglik(r, k, rows[b:b + 1])[0], b
    live = [0, 2, 3, 5]
    _check_ll(f"msm_loglik k={k} beside dead lanes", got[live], [R.msm_loglik(r, k, *rows[b]) for b in live], MSM_BAR)
    with pytest.raises(_native.NativeError) as e:
        engine.msm_marginals(r, k, *rows[1])
    assert e.value.code == _native.CVQ_ERR_NUMERIC


# ------------------------------------------------------------- device-memory staging
def test_device_memory_entry_points_match_host_memory():
    """CVQ_MEM_DEVICE: parameters, returns and outputs are device pointers used in place (no
    staging copies); bit-equal to the host-memory call of the same entry point."""
    import torch
    from copula_var import _native as N
    from copula_var import engine
    lib, B, n = N.lib(), 5, R.BOUNDARY_N

    def dev(a):
        return torch.from_numpy(N.f64(a)).cuda()

    def out(*shape):
        return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")

    def p(t):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
        return C.c_void_p(t.data_ptr())

    def call(fn, *args):
        torch.cuda.synchronize()
        N.check(getattr(lib, fn)(*args), fn)
        torch.cuda.synchronize()

    r = R.garch_returns(n)
    rows, d_r, o = R.garch11_rows(B), dev(r), out(B)
    d_p = dev(rows)                                            # named: the tensors outlive the call
    call("cvq_garch_loglik", 0, p(d_p), B, p(d_r), n, p(o), N.MEM_DEVICE)
    np.testing.assert_array_equal(o.cpu().numpy(), engine.garch_loglik(r, rows))

    rows, o = R.garch_rows(2, 3, B), out(B)
    d_p = dev(rows)
    call("cvq_garch_loglik_pq", 0, 2, 3, p(d_p), B, p(d_r), n, p(o), N.MEM_DEVICE)
    np.testing.assert_array_equal(o.cpu().numpy(), engine.garch_loglik_pq(r, 2, 3, rows))

    r = R.msm_returns(n)
    rows, d_r, o = R.msm_rows(3, B), dev(r), out(B)
    d_p = dev(rows)
    call("cvq_msm_loglik", 0, 3, p(d_p), B, p(d_r), n, p(o), N.MEM_DEVICE)
    np.testing.assert_array_equal(o.cpu().numpy(), engine.msm_loglik(r, 3, rows))

    r, rows, o = R.ukf_returns(n), R.ukf_batch_rows(B), out(B)
    d_p, d_r = dev(rows), dev(r)
    call("cvq_ukf_loglik", 0, p(d_p), B, p(d_r), n, p(o), N.MEM_DEVICE)
    np.testing.assert_array_equal(o.cpu().numpy(), engine.ukf_loglik(r, rows))

    S = R.ukf_series_per_row(B, n)
    for series, per in ((r, 0), (S, 1)):
        d_s, o, st = dev(series), out(B), out(n, B)            # path layout [N][B], time-major
        call("cvq_ukf_filter", 0, p(d_p), B, p(d_s), per, n, p(o), p(st), N.MEM_DEVICE)
        ll_h, st_h = engine.ukf_filter(series, rows)
        np.testing.assert_array_equal(o.cpu().numpy(), ll_h)
        np.testing.assert_array_equal(st.cpu().numpy().T, st_h)
