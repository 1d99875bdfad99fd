"""Per-asset risk attribution on the device (cvq_slab_axis_moments, cvq_es_contributions)
against the numpy checker tests/attribution_reference.py, through every layer: plan, device
chaining, band (VaR) contributions, sharding, driver.

Bars (the project's slab bar, as tests/test_tail_moments_gpu.py applies it):
  |mx[c] - ref| <= 1e-10 mx_abs[c]        (x changes sign: mx itself is no error scale)
  m0 rtol 1e-10, atol 1e-15; m0 bit-identical to cvq_slab_moments' m0 on the same bounds
  |contrib[c] - ref| <= 2e-10 wa[c] mx_abs[c] / m0       (mx's and m0's relative errors)
  |sum_c wa[c] mx[c] - m1| <= 1e-12 sum |level x mass|   against the device's own m1
  |sum_c contrib[c] - (es - ptf_mean)| <= 3e-10 sum_c |contrib[c]|  against cvq_expected_shortfall
Every case runs with the golden's own (equal) weights and with unequal ones: equal weights
cannot tell a swapped wa (quirk Q10)."""
import ctypes as C
import functools

import numpy as np
import pytest

import attribution_reference as A
import es_reference as E
import gumbel_reference as G
from conftest import GOLDEN_CASES, golden_kwargs, load_golden
from test_gumbel_gpu import CASES as GUMBEL_CASES, IDS as GUMBEL_IDS

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
SMALL = [c for c in GOLDEN_CASES if c not in ("cfg2_n256", "cfg3_n128")]
UNEQUAL = {2: (0.7, 0.3), 3: (0.5, 0.3, 0.2)}
# a tail slab, a thin one, one reaching positive levels, an empty one, a NaN bound, b above every level
ROWS = [(-100.0, -3.0), (-3.5, -3.0), (-3.0, 0.5), (-2.0, -2.0), (float("nan"), -3.0), (-100.0, 100.0)]
BAND = 0.25                               # var_contributions' default (tests/test_attribution_cpu.py: its premise)
BAND_MAX_EMPTY = 0.10                     # share of cfg1's dates the band test may skip for zero mass


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


def _weighted(z, unequal):
    if unequal:
        z = dict(z)
        z["weights"] = np.array(UNEQUAL[int(z["dim"])])
    return z


@functools.lru_cache(maxsize=None)
def _ref(case, unequal=False, gumbel=None):
    """(golden arrays with the weights in force, checker Problem): built once, shared, unchanged."""
    z = _weighted(load_golden(case), unequal)
    P = G.problem_of(z, *gumbel) if gumbel else E.problem_of(z)
    return z, P


def _plan_of(P, strategy="auto", sl=slice(None)):
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w, P.copula_params,
                       vol_states=P.uvs if P.model == "msm" else None, strategy=strategy)
    p.set_dates((P.fbs[sl], P.pi[sl]) if P.model == "msm" else [P.sigma[sl]])
    return p


def _check_moments(P, p, bounds):
    """Device (m0, mx) of `bounds` against the checker, m0 against cvq_slab_moments bit for bit,
    and sum wa mx against the device's own m1."""
    bounds = np.asarray(bounds, dtype=np.float64)
    m0r, mxr, mxa = A.axis_moments(P, bounds)
    _, _, m1a = E.tail_moments(P, bounds)
    m0, mx = p.axis_moments(bounds)
    t0, t1 = p.tail_moments(bounds)
    wa = A.axis_weights(P)
    assert np.array_equal(p.axis_weights, wa)
    print("mx err / mx_abs", float(np.max(np.abs(mx - mxr) / np.maximum(mxa, 1e-300))),
          "m0 rel", float(np.max(np.abs(m0 - m0r) / np.maximum(np.abs(m0r), 1e-300))),
          "additivity / m1_abs", float(np.max(np.abs(mx @ wa - t1) / np.maximum(m1a, 1e-300))))
    assert mx.shape == (P.T, P.dim)
    np.testing.assert_allclose(m0, m0r, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    assert np.all(np.abs(mx - mxr) <= 1e-10 * mxa)
    assert np.array_equal(m0, t0)
    assert np.all(np.abs(mx @ wa - t1) <= 1e-12 * m1a)
    dead = (bounds[:, 0] != bounds[:, 0]) | (bounds[:, 1] != bounds[:, 1]) | (bounds[:, 0] == bounds[:, 1])
    assert np.all(m0[dead] == 0.0) and np.all(mx[dead] == 0.0)          # NaN / empty: exactly 0
    return m0, mx


def _check_contrib(P, p, var, ptf):
    """Device contributions of `var` against the checker and against cvq_expected_shortfall."""
    ref, m0r, _, mxa = A.es_contributions(P, var, ptf)
    contrib, m0 = p.es_contributions(var, ptf)
    es, m0e = p.expected_shortfall(var, ptf)
    wa = np.abs(A.axis_weights(P))
    assert contrib.shape == (P.T, P.dim)
    assert np.array_equal(np.isnan(contrib), np.isnan(ref))
    ok = ~np.isnan(ref[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        bar = 2e-10 * wa * mxa / m0r[:, None]
    print("contrib err / bar", float(np.max((np.abs(contrib - ref) / bar)[ok], initial=0.0)),
          "sum err / bar", float(np.max((np.abs(contrib.sum(axis=1) - (es - ptf)) /
                                         (3e-10 * np.abs(contrib).sum(axis=1)))[ok], initial=0.0)))
    np.testing.assert_allclose(m0, m0r, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    assert np.array_equal(m0, m0e)
    assert np.all(np.abs(contrib - ref)[ok] <= bar[ok])
    assert np.array_equal(np.isnan(es), ~ok)
    assert np.all(np.abs(contrib.sum(axis=1) - (es - ptf))[ok] <= 3e-10 * np.abs(contrib).sum(axis=1)[ok])
    return contrib, m0


def _tail_bounds(P, var, ptf):
    return np.column_stack((np.full(P.T, -100.0), np.asarray(var) - ptf))


# ------------------------------------------------------------------ 1. every small golden
@pytest.mark.parametrize("unequal", [False, True], ids=["own_weights", "unequal_weights"])
@pytest.mark.parametrize("case", SMALL)
def test_small_goldens(case, unequal):
    z, P = _ref(case, unequal)
    ptf = float(z["ptf_mean"])
    p = _plan_of(P)
    try:
        _check_contrib(P, p, z["var"], ptf)
        _check_moments(P, p, _tail_bounds(P, z["var"], ptf))
    finally:
        p.close()


@pytest.mark.parametrize("unequal", [False, True], ids=["own_weights", "unequal_weights"])
@pytest.mark.parametrize("case,kind,theta", GUMBEL_CASES, ids=GUMBEL_IDS)
def test_gumbel_cases(case, kind, theta, unequal):
    z, P = _ref(case, unequal, (kind, theta))
    ptf = float(z["ptf_mean"])
    p = _plan_of(P)
    try:
        assert p.strategy == "sorted"
        _check_contrib(P, p, z["var"], ptf)           # any levels: the golden's own VaR vector
        _check_moments(P, p, _tail_bounds(P, z["var"], ptf))
    finally:
        p.close()


# ------------------------------------------------------------------ 2. chunk edges, arbitrary bounds
def _garch_problem(dim, n, weights, T=6):
    """The reference's grid at n points (as test_tail_moments_gpu.py::test_3d_garch_n130 builds
    it) on a GARCH golden's sigma forecasts, cycled to T dates."""
    from oracle import forecast as F
    from oracle.quadrature import Problem
    z = load_golden("garch_student_n64" if dim == 2 else "garch3d_student_n16")
    x, step = F.x_grid(n, "garch")
    sig = np.resize(z["sigma_forecasts"], (T, dim))          # whole rows repeat: T x dim from T0 x dim
    return Problem("garch", "student", dim, x, step, np.ones((dim, 1, n)), np.zeros((1, dim)),
                   np.array(weights), z["copula_params"], sig)


@pytest.mark.parametrize("dim,n,weights", [(2, 100, (0.5, 0.5)), (2, 100, (0.7, 0.3)),
                                           (3, 20, (1 / 3, 1 / 3, 1 / 3)), (3, 20, (0.5, 0.3, 0.2))])
def test_chunk_edges(dim, n, weights):
    """2-D n = 100: two 64-row chunks, the second of 36 rows, column ranges not divisible by the
    four waves; 3-D n = 20: 400 rows, two 256-row chunks, the second of 144 rows (a partial wave)."""
    P = _garch_problem(dim, n, weights)
    p = _plan_of(P)
    try:
        _check_moments(P, p, np.array(ROWS))
        _check_moments(P, p, np.tile(ROWS[2], (P.T, 1)))
        var = np.array([-2.6, -2.1, -1.7, np.nan, -3.4, -120.0])       # NaN VaR; below every level: m0 == 0
        contrib, m0 = _check_contrib(P, p, var, 0.0)
        assert np.isnan(contrib[3]).all() and np.isnan(contrib[5]).all() and m0[5] == 0.0
    finally:
        p.close()


@pytest.mark.parametrize("unequal", [False, True], ids=["own_weights", "unequal_weights"])
def test_3d_msm_arbitrary_bounds(unequal):
    """cfg4_k4_n16: q > 1 and the Q6 rows (i1 == 0 carries the axis-0 factor)."""
    z, P = _ref("cfg4_k4_n16", unequal)
    p = _plan_of(P)
    try:
        for off in (0, 2):
            _check_moments(P, p, np.array([ROWS[(t + off) % len(ROWS)] for t in range(P.T)]))
        var = z["var"].copy()
        var[1] = np.nan
        contrib, m0 = _check_contrib(P, p, var, float(z["ptf_mean"]))
        assert np.isnan(contrib[1]).all() and m0[1] == 0.0
    finally:
        p.close()


# ------------------------------------------------------------------ 3. every strategy
@pytest.mark.parametrize("strategy", ["compact", "sorted", "sweep", "direct", "prefix"])
def test_every_strategy(strategy):
    z, P = _ref("cfg2_n64", True)
    ptf = float(z["ptf_mean"])
    z0, P0 = _ref("cfg2_n64")
    p = _plan_of(P0, strategy)
    try:
        assert p.strategy == strategy
        _check_contrib(P0, p, z0["var"], ptf)
        _check_moments(P0, p, np.tile((-3.0, 0.5), (P0.T, 1)))       # above v_cap: no sibling, the plan itself
        assert p._wide is None
        var, _ = p.calc_var(ptf)                                      # the solve state is intact
        assert np.array_equal(var, z0["var"])
    finally:
        p.close()
    p = _plan_of(P, strategy)                                         # unequal weights: the division path
    try:
        _check_contrib(P, p, z["var"], ptf)
    finally:
        p.close()


def test_no_dates_is_a_state_error():
    from copula_var import _native as N
    from copula_var.engine import QuadraturePlan
    z, P = _ref("cfg2_n64")
    p = QuadraturePlan(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w, P.copula_params,
                       vol_states=P.uvs)
    try:
        buf = np.zeros(8)
        a = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-6, 0.0)
        lib = N.lib()
        assert lib.cvq_slab_axis_moments(p._h, N.ptr(buf), N.ptr(buf), N.ptr(buf), N.MEM_HOST) == N.CVQ_ERR_STATE
        assert lib.cvq_es_contributions(p._h, C.byref(a), N.ptr(buf), N.ptr(buf), None, N.MEM_HOST) == \
            N.CVQ_ERR_STATE
        assert lib.cvq_es_contributions(p._h, C.byref(a), N.ptr(buf), None, None, N.MEM_HOST) == N.CVQ_ERR_INVALID
    finally:
        p.close()


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("case", ["cfg2_n64", "garch3d_student_n16"])
def test_deterministic_and_batch_independent(case):
    """Two runs agree bit for bit; a date's row does not depend on the batch around it: T = 1
    against the same date inside a batch of 7 (dates cycled where the golden holds fewer)."""
    z, P = _ref(case, True)
    ptf = float(z["ptf_mean"])
    idx = np.arange(7) % P.T
    per = (P.fbs[idx], P.pi[idx]) if P.model == "msm" else [P.sigma[idx]]
    var = z["var"][idx]
    b = np.array([ROWS[t % 3] for t in range(7)])
    p = _plan_of(P)
    try:
        p.set_dates(per)
        c0, m0 = p.es_contributions(var, ptf)
        c1, m1 = p.es_contributions(var, ptf)
        assert np.array_equal(c0, c1) and np.array_equal(m0, m1)
        a0, ax0 = p.axis_moments(b)
        a1, ax1 = p.axis_moments(b)
        assert np.array_equal(a0, a1) and np.array_equal(ax0, ax1)
        assert np.isfinite(c0).all()
        k = 4
        p.set_dates((per[0][k:k + 1], per[1][k:k + 1]) if P.model == "msm" else [per[0][k:k + 1]])
        c2, m2 = p.es_contributions(var[k:k + 1], ptf)
        a2, ax2 = p.axis_moments(b[k:k + 1])
        assert np.array_equal(c2[0], c0[k]) and m2[0] == m0[k]
        assert a2[0] == a0[k] and np.array_equal(ax2[0], ax0[k])
    finally:
        p.close()


# ------------------------------------------------------------------ 5. device chaining
def test_device_chain_behind_solve_and_es():
    import torch
    from copula_var import engine
    z, P = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    p = _plan_of(P)
    try:
        var_h, _ = p.calc_var(ptf)
        es_h, _ = p.expected_shortfall(var_h, ptf)
        c_h, m0_h = p.es_contributions(var_h, ptf)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        args = engine.solve_args(ptf)
        with torch.cuda.stream(stream):
            var = torch.empty(P.T, dtype=torch.float64, device=dev)
            es = torch.empty(P.T, dtype=torch.float64, device=dev)
            contrib = torch.empty((P.T, P.dim), dtype=torch.float64, device=dev)
            m0 = torch.empty(P.T, dtype=torch.float64, device=dev)
            p.set_stream(stream.cuda_stream)
            p.solve_device(args, var.data_ptr(), check=False)
            p.expected_shortfall_device(args, var.data_ptr(), es.data_ptr())
            p.es_contributions_device(args, var.data_ptr(), contrib.data_ptr(), m0.data_ptr())
        stream.synchronize()
        assert np.array_equal(var.cpu().numpy(), z["var"])
        assert np.array_equal(es.cpu().numpy(), es_h)
        assert np.array_equal(contrib.cpu().numpy(), c_h)
        assert np.array_equal(m0.cpu().numpy(), m0_h)
        with torch.cuda.stream(stream):
            b = torch.tensor(_tail_bounds(P, var_h, ptf), dtype=torch.float64, device=dev)
            mx = torch.empty((P.T, P.dim), dtype=torch.float64, device=dev)
            p.axis_moments_device(b.data_ptr(), m0.data_ptr(), mx.data_ptr())
        stream.synchronize()
        m0_b, mx_b = p.axis_moments(_tail_bounds(P, var_h, ptf))
        assert np.array_equal(m0.cpu().numpy(), m0_b) and np.array_equal(mx.cpu().numpy(), mx_b)
        var2, _ = p.calc_var(ptf)                     # the plan's next solve is unchanged
        assert np.array_equal(var2, z["var"])
    finally:
        p.close()


# ------------------------------------------------------------------ 6. band (VaR) contributions
def test_band_contributions_cfg1():
    """Rows sum to the band's mean level, which lies inside the band on every date that holds
    mass; at most BAND_MAX_EMPTY of the dates may hold none (the checker alone meets that cap:
    tests/test_attribution_cpu.py::test_band_premise_on_cfg1)."""
    z, P = _ref("cfg1")
    ptf = float(z["ptf_mean"])
    var = z["var"]
    ref, mean_r, m0r, _, mxa = A.var_contributions(P, var, ptf, BAND)
    p = _plan_of(P)
    try:
        contrib, mean, m0 = p.var_contributions(var, ptf)            # the default band
        given = p.var_contributions(var, ptf, BAND)
    finally:
        p.close()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(given, (contrib, mean, m0)))
    empty = m0 == 0.0
    print("dates with an empty band", int(empty.sum()), "of", P.T)
    assert np.array_equal(empty, m0r == 0.0) and empty.mean() <= BAND_MAX_EMPTY
    ok = ~empty
    assert np.isnan(contrib[empty]).all() and np.isnan(mean[empty]).all()
    np.testing.assert_allclose(m0, m0r, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    wa = np.abs(A.axis_weights(P))
    assert np.all(np.abs(contrib - ref)[ok] <= (2e-10 * wa * mxa / m0r[:, None])[ok])
    assert np.all(np.abs(contrib.sum(axis=1) - mean)[ok] <= 3e-10 * np.abs(contrib).sum(axis=1)[ok])
    assert np.all(np.abs(mean - mean_r)[ok] <= 3e-10 * np.abs(contrib).sum(axis=1)[ok])
    top = var - ptf
    assert np.all((top - BAND < mean)[ok] & (mean <= top)[ok])


# ------------------------------------------------------------------ 7. sharded, world 1
def test_sharded_world1():
    import torch
    from copula_var import engine
    from copula_var.distributed import device_sharded_var
    z, P = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    p = _plan_of(P)
    try:
        s = device_sharded_var(p, engine.solve_args(ptf), P.T, torch.device("cuda", 0))
        var = s.solve().cpu().numpy()
        contrib = s.es_contributions().cpu().numpy()
        assert np.array_equal(var, z["var"])
        assert contrib.shape == (P.T, P.dim)
        assert np.array_equal(contrib, p.es_contributions(var, ptf)[0])
    finally:
        p.close()


# ------------------------------------------------------------------ 8. driver
@pytest.mark.parametrize("case", ["cfg2_n64", "garch_student_n64"])
def test_driver_calc_contributions(case):
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    z, P = _ref(case)
    ptf = float(z["ptf_mean"])
    ref, m0r, _, mxa = A.es_contributions(P, z["var"], ptf)
    tickers, start, kw = inject(z)
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=str(z["copula"]),
                                                               estimation_type=str(z["model"]))
    v = ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=int(z["num_points"]),
                               weights=z["weights"], copula_params=z["copula_params"], **kw)
    try:
        contrib = v.calc_es_contributions(**golden_kwargs(z))
        m0 = v.last_tail_mass
        given = v.calc_es_contributions(var=z["var"])
        es = v.calc_es(var=z["var"])
        band = v.calc_var_contributions(var=z["var"])
        band_mean = v.last_band_mean
    finally:
        v.close()
    assert contrib.shape == (P.T, P.dim) and np.array_equal(given, contrib)
    np.testing.assert_allclose(m0, m0r, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    assert np.all(np.abs(contrib - ref) <= 2e-10 * np.abs(A.axis_weights(P)) * mxa / m0r[:, None])
    assert np.all(np.abs(contrib.sum(axis=1) - (es - v.ptf_mean)) <= 3e-10 * np.abs(contrib).sum(axis=1))
    ok = ~np.isnan(band_mean)
    assert np.all(np.abs(band.sum(axis=1) - band_mean)[ok] <= 3e-10 * np.abs(band).sum(axis=1)[ok])
