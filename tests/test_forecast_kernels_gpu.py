"""The per-date forecast stage of csrc/cvq_forecast.hip (cvq_msm_filter, cvq_msm_tables,
cvq_sigma_tables) on the MI355X against the longdouble restatements of tests/forecast_reference.py
-- every dispatch path and every compiled instance, the collapse and the combinations, the
zero-normaliser / UKF-failure flags of each path and the clean rerun after a flagged one.

cvq_msm_tables dispatches three ways; each is run here against a reference that is not a device
kernel:
    step by step   k = 1, 7 (any n_in) and k = 2 .. 6 with n_in <= 32:
                   k_msm_cond, k_msm_filter<K>, k_msm_fbs, k_msm_pi
    narrow scan    k = 2, 3, 4, n_in > 32: k_msm_blkscan (z = 2), k_msm_supscan, k_msm_scanwin, k_msm_pi
    wide scan      k = 5, 6, n_in > 32: k_msm_blkscan (z = 1), k_msm_supscan_w, k_msm_scanwin_w, k_msm_pi
The scan shapes visit every way a window's full blocks fall into superblocks
(forecast_reference.scan_middle_class; asserted in test_forecast_reference_cpu.py).

The rule (forecast_reference.check_tiers): relative error <= 1e-12 where the reference is >= 1e-30,
<= 1e-10 down to 1e-200, and a device value <= 2e-200 below that.  GARCH forecasts rtol 1e-13, UKF
forecasts rtol 1e-12.

Measured, from one run of this module on an MI355X (gfx950), beside the float64 oracle's figures
on the same inputs (test_forecast_reference_cpu.py, on a CPU); top / middle tier = largest relative
error, bottom = largest value where the reference is < 1e-200:
                                                        device                          oracle
    cvq_msm_filter, k_msm_filter<1..7>                  3.2e-14 / 7.5e-14 / 1.0e-202    4.6e-14 / 1.6e-13 / 1.1e-202
    step-by-step path, fbs (k_msm_cond/filter/fbs)      2.9e-14 / 1.6e-13 / 3.2e-209    (filtered vectors of every
    step-by-step path, pi (k_msm_pi)                    3.1e-14 / 1.6e-13 / 7.1e-201     asset of every tables call:
    narrow scan k = 2, 3, 4, fbs                        2.5e-14 / 7.7e-14 / 6.6e-232     the line above; fbs / pi on
    narrow scan, pi                                     2.5e-14 / 8.3e-14 / 1.0e-202     five of the shapes:
    wide scan k = 5, 6, fbs                             3.4e-14 / 1.5e-13 / 4.0e-206     3.1e-14 / 1.2e-13)
    wide scan, pi                                       3.5e-14 / 1.6e-13 / 4.5e-201
    q = 1 (m0 = 1), fbs and pi                          4.4e-16
    hand-made state map (s + d) % q, fbs and pi         2.3e-14 / 3.9e-14
    clean rerun after a flagged run, fbs and pi         1.3e-14 / 3.7e-14
    k_garch_sigma<P,Q>, 16 orders (relative)            2.0e-16                         1.7e-16 (GARCH forecast, test_insample_reference_cpu.py)
    k_garch_sigma, floor branch (relative)              1.4e-16
    k_ukf_sigma, dim = 3 (relative)                     7.6e-15
A pi below 1e-200 is a product of components that need not be: the device's largest such value,
7.1e-201, is the reference's own value just under the threshold, inside the 2e-200 cap.
The bars are the project's, not these figures: one run does not license a tighter one.
"""
import functools

import numpy as np
import pytest

import forecast_reference as F
import insample_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


def _dev(rc):
    """(N, dim) host returns -> the [dim][N] device tensor the tables read."""
    import torch
    return torch.tensor(np.ascontiguousarray(np.asarray(rc).T), dtype=torch.float64, device="cuda:0")


def _production_map(k, rows):
    """The state map and q the driver passes: tables.unique_vol_map of the assets' vol states."""
    from copula_var import tables
    vsa = np.array([tables.msm_vol_states(k, row[0], row[1]) for row in rows])
    smap, uvs = tables.unique_vol_map(vsa)
    return smap, uvs.shape[1]


def _tables(rows, k, state_map, q, n_in, T):
    from copula_var import engine
    return engine.MsmTables([list(row) for row in rows], k, state_map, q, n_in, T, 0)


def _run(mt, rc):
    mt.run(_dev(rc))
    mt.status()
    return mt.fbs.cpu().numpy(), mt.pi.cpu().numpy()


def _check_tables(name, kind, n_in, T, k, dim):
    rc, rows = F.asset_series(kind, n_in, T, k, dim)
    smap, q = _production_map(k, rows)
    assert q == k + 1
    fbs, pi = _run(_tables(rows, k, smap, q, n_in, T), rc)
    ref_fbs, ref_pi = F.tables_reference(kind, n_in, T, k, dim)
    assert fbs.shape == (T, dim, q) and pi.shape == (T, q ** dim)
    F.check_tiers(f"{name} fbs k={k} dim={dim} {kind} ({n_in},{T})", fbs, ref_fbs)
    F.check_tiers(f"{name} pi k={k} dim={dim} {kind} ({n_in},{T})", pi, ref_pi)


# --------------------------------------------------------------------- cvq_msm_filter
@pytest.mark.parametrize("kind", F.SERIES_KINDS)
@pytest.mark.parametrize("k", range(1, 8))
def test_msm_filter_every_instance(k, kind):
    """k_msm_filter<1..7> behind cvq_msm_filter: n_in on both sides of the 8-deep prefetch ring,
    T = 130 across a 256-thread block for every lanes-per-window count, clamped inactive lanes."""
    from copula_var import engine
    row = F.base_row(k)
    for n_in, T in F.FILTER_SHAPES:
        N = n_in + T - 1
        x = F.series(kind, N, 3000 + N, row[1])
        got = engine.msm_filter(x, n_in, k, *row)
        assert got.shape == (T, 1 << k)
        F.check_tiers(f"msm_filter k={k} {kind} ({n_in},{T})", got, F.msm_window_probs(x, n_in, k, *row))


# ---------------------------------------------------------- cvq_msm_tables, the three paths
@pytest.mark.parametrize("kind", F.SERIES_KINDS)
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k", range(1, 8))
def test_tables_step_by_step_path(k, dim, kind):
    """k = 1, 7 at any window length and k = 2 .. 6 up to the scan's threshold (n_in = 32):
    k_msm_cond -> k_msm_filter<K> -> k_msm_fbs -> k_msm_pi, per-asset parameters all different.
    k = 7 with 3 assets is q = 8: 512 combinations."""
    for n_in, T in F.step_shapes(k):
        assert k in (1, 7) or n_in <= 2 * F.SCAN_B
        _check_tables("step", kind, n_in, T, k, dim)


@pytest.mark.parametrize("kind", F.SERIES_KINDS)
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k", range(2, 7))
def test_tables_scan_paths(k, dim, kind):
    """The narrow (k = 2, 3, 4) and the wide (k = 5, 6) transfer-matrix scans over window lengths
    that put the middle blocks in every superblock class, series ending in a partial block, T off
    multiples of 16 and T = 1."""
    for n_in, T in F.SCAN_SHAPES:
        assert n_in > 2 * F.SCAN_B
        _check_tables("scan", kind, n_in, T, k, dim)


# ------------------------------------------------------------ collapse and combinations
@pytest.mark.parametrize("k,n_in,T", [(3, 32, 33), (3, 49, 130), (5, 49, 130), (7, 5, 19)])
@pytest.mark.parametrize("dim", [2, 3])
def test_single_unique_vol(k, n_in, T, dim):
    """m0 = 1: every state has the same vol, the production map sends all of them to q = 1 and
    every fbs / pi entry is the sum of a probability vector."""
    rows = [(1.0,) + row[1:] for row in F.asset_rows(k, dim)]
    N = n_in + T - 1
    rc = np.column_stack([F.plain_series(N, 5000 + d) for d in range(dim)])
    smap, q = _production_map(k, rows)
    assert q == 1 and not smap.any()
    fbs, pi = _run(_tables(rows, k, smap, q, n_in, T), rc)
    ref = np.stack([F.collapse(F.msm_window_probs(rc[:, d], n_in, k, *rows[d]), smap[d], 1) for d in range(dim)], axis=1)
    assert fbs.shape == (T, dim, 1) and pi.shape == (T, 1)
    np.testing.assert_allclose(np.asarray(ref, dtype=np.float64), 1.0, rtol=1e-15)
    F.check_tiers(f"q=1 fbs k={k} dim={dim}", fbs, ref)
    F.check_tiers(f"q=1 pi k={k} dim={dim}", pi, F.combinations(ref))


@pytest.mark.parametrize("k,q,n_in,T", [(4, 3, 32, 33), (7, 5, 5, 19), (3, 3, 49, 130), (4, 5, 161, 40),
                                        (6, 3, 49, 130), (5, 8, 161, 40)])
@pytest.mark.parametrize("dim", [2, 3])
def test_hand_made_state_map(k, q, n_in, T, dim):
    """include/cvq.h admits any state_map into [0, q), not only the popcount-shaped one the
    driver derives: asset d collapses state s onto (s + d) % q -- step-by-step, narrow and wide."""
    smap = np.array([[(s + d) % q for s in range(1 << k)] for d in range(dim)], dtype=np.int32)
    rc, rows = F.asset_series("spiky", n_in, T, k, dim)
    fbs, pi = _run(_tables(rows, k, smap, q, n_in, T), rc)
    ref_fbs, ref_pi = F.tables_reference("spiky", n_in, T, k, dim, state_map=smap, q=q)
    F.check_tiers(f"map (s+d)%{q} fbs k={k} dim={dim} ({n_in},{T})", fbs, ref_fbs)
    F.check_tiers(f"map (s+d)%{q} pi k={k} dim={dim} ({n_in},{T})", pi, ref_pi)


# ------------------------------------------------------- zero-normaliser flags, per path
FLAG_PATHS = {"step k=1": (1, 40, 20), "step k=3": (3, 20, 20), "narrow k=2": (2, 49, 20), "wide k=5": (5, 49, 20)}


@pytest.mark.parametrize("dim,asset", [(2, 0), (3, 1), (3, 2)])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("path", list(FLAG_PATHS))
def test_zero_normaliser_flag_and_clean_rerun(path, where, dim, asset):
    """One return of one asset at 1e4 sigma: every state's density underflows to 0, the
    reference's Bayes normaliser is 0 (calc_prob.py:64-65) and status() raises -- from the error
    word of the step-by-step path and from the scans' per-block flags, at the first return, in
    the middle and at the last return of a series that ends in a partial block.  The same object
    run on the clean series afterwards reports OK and matches the reference (no stale flag)."""
    from copula_var import _native as N, engine
    k, n_in, T = FLAG_PATHS[path]
    n = n_in + T - 1
    assert n % 16 != 0
    rc, rows = F.asset_series("plain", n_in, T, k, dim)
    at = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    bad = rc.copy()
    bad[at, asset] = 1e4 * rows[asset][1]
    with pytest.raises(FloatingPointError):
        F.msm_window_probs(bad[:, asset], n_in, k, *rows[asset])
    smap, q = _production_map(k, rows)
    mt = _tables(rows, k, smap, q, n_in, T)
    mt.run(_dev(bad))
    with pytest.raises(N.NativeError):
        mt.status()
    with pytest.raises(N.NativeError):
        engine.msm_filter(bad[:, asset], n_in, k, *rows[asset])
    fbs, pi = _run(mt, rc)                                      # status() inside: the flag is gone
    ref_fbs, ref_pi = F.tables_reference("plain", n_in, T, k, dim)
    F.check_tiers(f"rerun {path} fbs dim={dim}", fbs, ref_fbs)
    F.check_tiers(f"rerun {path} pi dim={dim}", pi, ref_pi)


# --------------------------------------------------------------------- cvq_sigma_tables
def _split(row, p):
    return row[0], row[1:1 + p], row[1 + p:]


def _garch_triples():
    """Every (p, q), three distinct orders per call where three exist with the same max(p, q), so
    the call's shortest legal window n_in = max(p, q) is the shortest for each of its assets."""
    return [((1, 1), (1, 1), (1, 1)), ((1, 2), (2, 1), (2, 2)), ((1, 3), (2, 3), (3, 3)), ((3, 1), (3, 2), (3, 3)),
            ((1, 4), (2, 4), (3, 4)), ((4, 1), (4, 2), (4, 3)), ((4, 4), (1, 4), (4, 1))]


def test_garch_triples_cover_every_order():
    assert {o for tr in _garch_triples() for o in tr} == set(R.GARCH_ORDERS)
    assert all(len({max(o) for o in tr}) == 1 for tr in _garch_triples())


def _check_sigma_garch(name, orders, rows, rc, n_in, T):
    from copula_var import engine
    params = [{"pq": o, "params": tuple(row)} for o, row in zip(orders, rows)]
    st = engine.SigmaTables("garch", params, n_in, T)
    st.run(_dev(rc))
    st.status()
    sig = st.sig.cpu().numpy()
    assert sig.shape == (T, len(orders))
    wants = [np.array([R.garch_forecast_pq(rc[t:t + n_in, d], *_split(row, p))[0] for t in range(T)])
             for d, ((p, q), row) in enumerate(zip(orders, rows))]
    worst = max(float(np.max(np.abs(sig[:, d].astype(R.LD) - want) / want)) for d, want in enumerate(wants))
    print(f"MEASURED sigma_tables {name} {orders} ({n_in},{T}) max relative = {worst:.2e}")
    for d, want in enumerate(wants):
        assert np.all(np.abs(sig[:, d].astype(R.LD) - want) <= 1e-13 * want), (orders, d)


@pytest.mark.parametrize("orders", _garch_triples())
def test_sigma_tables_garch_every_order(orders):
    """k_garch_sigma<P, Q>, all 16 instances, three per 3-asset call (the [T][dim] stride), on the
    shortest legal window and across a 256-thread block."""
    m = max(orders[0])
    for n_in, T in ((m, 5), (12, 257)):
        n = n_in + T - 1
        rc = R.garch_returns(3 * n).reshape(n, 3)
        rows = [R.garch_rows(p, q)[d] for d, (p, q) in enumerate(orders)]
        _check_sigma_garch("garch", orders, rows, rc, n_in, T)


def test_sigma_tables_garch_floor_branch():
    """max(sigma2, 1e-7) binding at every step (returns of order 1e-5, omega = 1e-9)."""
    orders = tuple(R.EDGE_ORDERS)
    for n_in, T in ((4, 5), (12, 257)):
        n = n_in + T - 1
        rc = R.garch_floor_returns(3 * n).reshape(n, 3)
        rows = [R.garch_floor_row(p, q) for p, q in orders]
        for d, ((p, q), row) in enumerate(zip(orders, rows)):
            assert R.garch_loglik_pq(rc[:n_in, d], *_split(row, p))[2] == n_in - 1      # every step floored
        _check_sigma_garch("garch floor", orders, rows, rc, n_in, T)


UKF_N_IN, UKF_T = 64, 65


def _ukf_series():
    n = UKF_N_IN + UKF_T - 1
    return np.column_stack([R.ukf_returns(n, seed=6600 + d) for d in range(3)])


@functools.lru_cache(maxsize=None)
def _ukf_reference():
    rc = _ukf_series()
    return np.array([[F.ukf_forecast(rc[t:t + UKF_N_IN, d], *R.UKF_ROWS[d]) for d in range(3)] for t in range(UKF_T)])


def _ukf_tables():
    from copula_var import engine
    params = [dict(zip(("a", "l", "q"), R.UKF_ROWS[d])) for d in range(3)]
    return engine.SigmaTables("mean_reverting", params, UKF_N_IN, UKF_T)


def _check_ukf(name, sig, ref, mask=None):
    mask = np.ones(ref.shape, dtype=bool) if mask is None else mask
    rel = np.abs(sig[mask].astype(R.LD) - ref[mask]) / ref[mask]
    print(f"MEASURED sigma_tables {name} max relative = {float(np.max(rel)):.2e}")
    assert np.all(rel <= 1e-12), name


def test_sigma_tables_ukf_three_assets():
    """k_ukf_sigma with dim = 3 and three different (a, l, q) rows, T = 65 across its 64-thread block."""
    st = _ukf_tables()
    st.run(_dev(_ukf_series()))
    st.status()
    sig = st.sig.cpu().numpy()
    assert sig.shape == (UKF_T, 3)
    _check_ukf("ukf dim=3", sig, _ukf_reference())


def test_sigma_tables_ukf_failure_and_clean_rerun():
    """An exact 0.0 as the last return of the third asset (eta = 0 -> Z = 0, estimate.py:219-220):
    only the last window of that asset fails -- NaN there, every other entry as the reference,
    status() raises; the same object on the clean series then passes."""
    from copula_var import _native as N
    rc = _ukf_series()
    bad = rc.copy()
    bad[-1, 2] = 0.0
    assert F.ukf_forecast(bad[UKF_T - 1:, 2], *R.UKF_ROWS[2]) is None
    st = _ukf_tables()
    st.run(_dev(bad))
    with pytest.raises(N.NativeError):
        st.status()
    sig = st.sig.cpu().numpy()
    ok = np.ones((UKF_T, 3), dtype=bool)
    ok[-1, 2] = False
    assert np.isnan(sig[-1, 2]) and not np.isnan(sig[ok]).any()
    _check_ukf("ukf failing run, the other entries", sig, _ukf_reference(), ok)
    st.run(_dev(rc))
    st.status()
    _check_ukf("ukf clean rerun", st.sig.cpu().numpy(), _ukf_reference())
