"""Tail moments and Expected Shortfall on the device (cvq_slab_moments,
cvq_expected_shortfall) against the numpy checker tests/es_reference.py, through every
layer: plan, device chaining, sharding, driver.

Tolerances: m0 / m1 at the project's slab bar (rtol 1e-10, atol 1e-15; every term of m1 has
one sign for bounds <= 0); es rtol 3e-10 (two relative errors + the division and the add,
|m1 / m0| >= 0.5 dominates ptf_mean on every case here); a slab that reaches positive
levels: |m1 - ref| <= 1e-10 * sum |level * mass|."""
import functools
import os

import numpy as np
import pytest

import es_reference as E
from conftest import GOLDEN, GOLDEN_CASES, golden_kwargs, load_golden

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
ES_RTOL = 3e-10
SMALL = [c for c in GOLDEN_CASES if c not in ("cfg2_n256", "cfg3_n128")]
ROWS = [(-100.0, -3.0), (-3.5, -3.0), (-3.0, 0.5), (-2.0, -2.0), (float("nan"), -3.0)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@functools.lru_cache(maxsize=None)
def _ref(case):
    """(golden arrays, oracle Problem, (es, m0, m1, m1_abs) of the golden VaR): computed once."""
    z = load_golden(case)
    P = E.problem_of(z)
    return z, P, E.expected_shortfall(P, z["var"], float(z["ptf_mean"]))


def _plan_of(P, copula_params, strategy="auto"):
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w, copula_params,
                       vol_states=P.uvs if P.model == "msm" else None, strategy=strategy)
    p.set_dates((P.fbs, P.pi) if P.model == "msm" else [P.sigma])
    return p


def _plan(case, strategy="auto"):
    z, P, _ = _ref(case)
    return _plan_of(P, z["copula_params"], strategy)


def _check_moments(P, got, bounds):
    """Device (m0, m1) of `bounds` against the checker; rows reaching positive levels take the
    mixed-sign bar for m1."""
    m0, m1, m1a = E.tail_moments(P, bounds)
    print("m0 rel", np.nanmax(np.abs(got[0] - m0) / np.maximum(np.abs(m0), 1e-300)),
          "m1 rel", np.nanmax(np.abs(got[1] - m1) / np.maximum(m1a, 1e-300)))
    np.testing.assert_allclose(got[0], m0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    pos = np.asarray(bounds)[:, 1] > 0.0
    np.testing.assert_allclose(got[1][~pos], m1[~pos], rtol=SLAB_RTOL, atol=SLAB_ATOL)
    assert np.all(np.abs(got[1][pos] - m1[pos]) <= 1e-10 * m1a[pos])


def _check_es(P, p, var, ptf):
    es_ref, m0_ref, m1_ref, _ = E.expected_shortfall(P, var, ptf)
    es, m0 = p.expected_shortfall(var, ptf)
    print("es rel", np.nanmax(np.abs(es - es_ref) / np.abs(es_ref)))
    np.testing.assert_allclose(m0, m0_ref, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    np.testing.assert_allclose(es, es_ref, rtol=ES_RTOL, atol=0.0)
    return es, m0


# ------------------------------------------------------------------ 1. every small golden
@pytest.mark.parametrize("case", SMALL)
def test_small_goldens(case):
    z, P, (es_ref, m0_ref, m1_ref, _) = _ref(case)
    ptf = float(z["ptf_mean"])
    p = _plan(case)
    try:
        var, _ = p.calc_var(ptf, **golden_kwargs(z))
        assert np.array_equal(var, z["var"])
        es, m0 = p.expected_shortfall(var, ptf)
        b = np.column_stack((np.full(P.T, -100.0), var - ptf))
        t0, t1 = p.tail_moments(b)
        slab = p.compute_integral(b)
    finally:
        p.close()
    print("es rel", np.max(np.abs(es - es_ref) / np.abs(es_ref)), "m0 rel", np.max(np.abs(m0 - m0_ref) / m0_ref),
          "m1 rel", np.max(np.abs(t1 - m1_ref) / np.abs(m1_ref)))
    np.testing.assert_allclose(m0, m0_ref, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    np.testing.assert_allclose(t1, m1_ref, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    np.testing.assert_allclose(es, es_ref, rtol=ES_RTOL, atol=0.0)
    assert np.array_equal(t0, m0)                    # both entry points run the same sums
    np.testing.assert_allclose(m0, slab, rtol=1e-10, atol=SLAB_ATOL)
    assert np.all(es < var)


# ------------------------------------------------------------------ 2. arbitrary bounds
@pytest.mark.parametrize("case", ["cfg2_n64", "cfg4_k4_n16"])
def test_arbitrary_bounds(case):
    z, P, _ = _ref(case)
    p = _plan(case)
    try:
        for row in ROWS:
            b = np.tile(row, (P.T, 1))
            got = p.tail_moments(b)
            if row[0] == row[1] or row[0] != row[0]:
                assert np.all(got[0] == 0.0) and np.all(got[1] == 0.0), row      # empty / NaN: exactly 0, 0
            _check_moments(P, got, b)
        b = np.array([ROWS[t % len(ROWS)] for t in range(P.T)])                  # a different row per date
        _check_moments(P, p.tail_moments(b), b)
        var = z["var"].copy()
        var[1] = np.nan
        es, m0 = _check_es(P, p, var, float(z["ptf_mean"]))
        assert np.array_equal(np.isnan(es), np.isnan(var)) and m0[1] == 0.0
    finally:
        p.close()


# ------------------------------------------------------------------ 3. every strategy
@pytest.mark.parametrize("strategy", ["compact", "sorted", "sweep", "direct", "prefix"])
def test_every_strategy(strategy):
    z, P, _ = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    p = _plan("cfg2_n64", strategy)
    try:
        assert p.strategy == strategy
        _check_es(P, p, z["var"], ptf)
        b = np.tile((-3.0, 0.5), (P.T, 1))           # above v_cap: no sibling, the plan itself
        _check_moments(P, p.tail_moments(b), b)
        assert p._wide is None
        var, _ = p.calc_var(ptf)                      # the moments call left the solve state intact
        assert np.array_equal(var, z["var"])
        _check_es(P, p, var, ptf)
    finally:
        p.close()


# ------------------------------------------------------------------ 4. edge geometry
def _fullbatch_problem(cfg, n, T=6):
    """As tests/test_large_grid_gpu.py::_problem: the reference's grid at n points on the first
    dates of a full-batch fixture."""
    from oracle import forecast as F
    from oracle.quadrature import Problem
    z = dict(np.load(os.path.join(GOLDEN, f"fullbatch_cfg{cfg}.npz"), allow_pickle=False))
    model = str(z["model"])
    x, step = F.x_grid(n, model)
    if model == "msm":
        uvs = z["unique_vol_states"]
        dens = F.msm_densities(uvs, x)
        per = (z["forecasts_by_states"][:T], z["forecasts"][:T])
        combos = z["combos"]
    else:
        uvs = None
        dens = np.ones((2, 1, n))
        per = z["sigma_forecasts"][:T]
        combos = np.zeros((1, 2))
    return z, Problem(model, str(z["copula"]), 2, x, step, dens, combos, z["weights"], z["copula_params"], per, uvs)


@pytest.mark.parametrize("cfg,n", [(5, 700), (3, 1024)])
def test_large_2d_grids(cfg, n):
    """n above 512 and not a multiple of 64 (700: 11 chunks, the last one partial); n = 1024 Plackett."""
    from oracle.quadrature import calc_var
    z, P = _fullbatch_problem(cfg, n)
    ptf = float(z["ptf_mean"])
    var, _, _ = calc_var(P.compute_integral, P.T, ptf)
    p = _plan_of(P, z["copula_params"])
    try:
        _check_es(P, p, var, ptf)
        b = np.tile((-3.0, 0.5), (P.T, 1))
        _check_moments(P, p.tail_moments(b), b)
    finally:
        p.close()


@pytest.mark.parametrize("copula,params", [("student", [5.0, 0.5, 0.4, 0.3]), ("gaussian", [0.5, 0.4, 0.3])])
def test_3d_garch_n130(copula, params):
    """16 900 rows: 66 full chunks of 256 rows and one of 4 (a partial last chunk and a partial
    last wave).  Then T = 1, where all parallelism comes from the row chunks: bit-identical to
    the batch's first date."""
    from oracle import forecast as F
    from oracle.quadrature import Problem
    z = load_golden("garch3d_student_n16")
    n, T = 130, 3
    x, step = F.x_grid(n, "garch")
    sig = z["sigma_forecasts"][:T]
    args = ("garch", copula, 3, x, step, np.ones((3, 1, n)), np.zeros((1, 3)), z["weights"], np.array(params))
    P = Problem(*args, sig)
    var = np.array([-2.6, -2.1, -1.7])               # any levels: the moments take arbitrary bounds
    p = _plan_of(P, np.array(params))
    try:
        es, m0 = _check_es(P, p, var, 0.0)
        b = np.tile((-3.0, 0.5), (T, 1))
        _check_moments(P, p.tail_moments(b), b)
        p.set_dates([sig[:1]])
        es1, m01 = p.expected_shortfall(var[:1], 0.0)
        assert es1[0] == es[0] and m01[0] == m0[0]
    finally:
        p.close()


def test_fitted_nu():
    """A fitted Student nu (general node power) on cfg2_n64."""
    from oracle.quadrature import Problem, calc_var
    z = load_golden("cfg2_n64")
    cp = np.array([5.364, 0.5])
    P = Problem("msm", "student", 2, z["x_values"], z["step"], z["densities"], z["combos"], z["weights"], cp,
                (z["forecasts_by_states"], z["forecasts"]), z["unique_vol_states"])
    ptf = float(z["ptf_mean"])
    var, _, _ = calc_var(P.compute_integral, P.T, ptf)
    p = _plan_of(P, cp)
    try:
        _check_es(P, p, var, ptf)
    finally:
        p.close()


# ------------------------------------------------------------------ 5. determinism
def test_deterministic_and_batch_independent():
    z, P, _ = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    b = np.array([ROWS[t % 3] for t in range(P.T)])
    p = _plan("cfg2_n64")
    try:
        a0, a1 = p.tail_moments(b)
        b0, b1 = p.tail_moments(b)
        assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
        es, m0 = p.expected_shortfall(z["var"], ptf)
        es2, m02 = p.expected_shortfall(z["var"], ptf)
        assert np.array_equal(es, es2) and np.array_equal(m0, m02)
        p.set_dates((z["forecasts_by_states"][3:7], z["forecasts"][3:7]))
        c0, c1 = p.tail_moments(b[3:7])
        assert np.array_equal(c0, a0[3:7]) and np.array_equal(c1, a1[3:7])
        es3, m03 = p.expected_shortfall(z["var"][3:7], ptf)
        assert np.array_equal(es3, es[3:7]) and np.array_equal(m03, m0[3:7])
    finally:
        p.close()


# ------------------------------------------------------------------ 6. device chaining
def test_device_chain_behind_solve():
    import torch
    from copula_var import engine
    z, P, _ = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    p = _plan("cfg2_n64")
    try:
        var_h, _ = p.calc_var(ptf)
        es_h, m0_h = p.expected_shortfall(var_h, ptf)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        args = engine.solve_args(ptf)
        with torch.cuda.stream(stream):
            var = torch.empty(P.T, dtype=torch.float64, device=dev)
            es = torch.empty(P.T, dtype=torch.float64, device=dev)
            m0 = torch.empty(P.T, dtype=torch.float64, device=dev)
            p.set_stream(stream.cuda_stream)
            p.solve_device(args, var.data_ptr(), check=False)
            p.expected_shortfall_device(args, var.data_ptr(), es.data_ptr(), m0.data_ptr())
        stream.synchronize()
        assert np.array_equal(var.cpu().numpy(), z["var"])
        assert np.array_equal(es.cpu().numpy(), es_h)
        assert np.array_equal(m0.cpu().numpy(), m0_h)
    finally:
        p.close()


# ------------------------------------------------------------------ 7. sharded, world 1
def test_sharded_world1():
    import torch
    from copula_var import engine
    from copula_var.distributed import device_sharded_var
    z, P, _ = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    p = _plan("cfg2_n64")
    try:
        s = device_sharded_var(p, engine.solve_args(ptf), P.T, torch.device("cuda", 0))
        var = s.solve().cpu().numpy()
        es = s.expected_shortfall().cpu().numpy()
        assert np.array_equal(var, z["var"])
        assert np.array_equal(es, p.expected_shortfall(var, ptf)[0])
    finally:
        p.close()


# ------------------------------------------------------------------ 8. driver
@pytest.mark.parametrize("case", ["cfg2_n64", "garch_student_n64"])
def test_driver_calc_es(case):
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    z, P, (es_ref, m0_ref, _, _) = _ref(case)
    tickers, start, kw = inject(z)
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=str(z["copula"]),
                                                               estimation_type=str(z["model"]))
    v = ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=int(z["num_points"]),
                               weights=z["weights"], copula_params=z["copula_params"], **kw)
    try:
        es = v.calc_es(**golden_kwargs(z))
        m0 = v.last_tail_mass
        es_given = v.calc_es(var=z["var"])
    finally:
        v.close()
    np.testing.assert_allclose(es, es_ref, rtol=ES_RTOL, atol=0.0)
    np.testing.assert_allclose(m0, m0_ref, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    assert np.array_equal(es_given, es)
