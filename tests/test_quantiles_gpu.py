"""Exact multi-level quantiles on the device (cvq_quantiles) against the numpy checker
tests/quantile_reference.py, through every layer: plan, device chaining, sharding, driver.

var is compared with np.array_equal: the device takes the checker's decisions as long as no
evaluated F comes within the summation error of a level, which every test asserts first
(margin >= 1e-7, 1000 x the slab bar of 1e-10; tests/test_quantiles_cpu.py).  m0 at the slab
bar (rtol 1e-10, atol 1e-15); |es - ref| <= 3e-10 (|m1 / m0| + |ptf_mean|): two relative errors,
the division and the add, as the Expected Shortfall's bar.
What the margin-1e-7 comparison cannot see (1e-8 of relative error in F, the narrow passes) is held by tests/test_quantile_probes_gpu.py."""
import functools
import os

import numpy as np
import pytest

import es_reference as E
import quantile_reference as Q
from conftest import GOLDEN, GOLDEN_CASES, load_golden

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
ES_RTOL = 3e-10
MARGIN = 1e-7
LEVELS = (0.01, 0.025, 0.05)
SMALL = [c for c in GOLDEN_CASES if c not in ("cfg2_n256", "cfg3_n128")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@functools.lru_cache(maxsize=None)
def _ref(case):
    """(golden arrays, oracle Problem, checker's (var, es, m0, margin) at LEVELS): computed once."""
    z = load_golden(case)
    P = E.problem_of(z)
    return z, P, Q.quantiles(P, LEVELS, float(z["ptf_mean"]))


def _plan_of(P, copula_params, strategy="auto"):
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w, copula_params,
                       vol_states=P.uvs if P.model == "msm" else None, strategy=strategy)
    p.set_dates((P.fbs, P.pi) if P.model == "msm" else [P.sigma])
    return p


def _compare(got, ref, ptf):
    """Device (var, es, m0) against the checker's (var, es, m0, margin)."""
    var, es, m0 = got
    rvar, res, rm0, margin = ref
    print("margin", margin.min(), "m0 rel", np.max(np.abs(m0 - rm0) / np.maximum(np.abs(rm0), 1e-300)),
          "es err / bar", np.nanmax(np.abs(es - res) / (ES_RTOL * (np.abs(res - ptf) + abs(ptf))), initial=0.0))
    assert margin.min() >= MARGIN                     # the premise of the exact comparison
    assert np.array_equal(np.isnan(var), np.isnan(rvar)) and np.array_equal(np.isnan(es), np.isnan(res))
    assert np.array_equal(var, rvar, equal_nan=True)
    np.testing.assert_allclose(m0, rm0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    ok = ~np.isnan(res)
    assert np.all(np.abs(es[ok] - res[ok]) <= ES_RTOL * (np.abs(res[ok] - ptf) + abs(ptf)))


def _check(P, p, levels, ptf, **kw):
    got = p.quantiles(levels, ptf, **kw)
    _compare(got, Q.quantiles(P, levels, ptf, **kw), ptf)
    return got


# ------------------------------------------------------------------ 1. every small golden
@pytest.mark.parametrize("case", SMALL)
def test_small_goldens(case):
    z, P, ref = _ref(case)
    ptf = float(z["ptf_mean"])
    p = _plan_of(P, z["copula_params"])
    try:
        got = p.quantiles(LEVELS, ptf)
        one = p.quantiles([0.05], ptf)
    finally:
        p.close()
    _compare(got, ref, ptf)
    for a, b in zip(one, got):                        # the levels do not see each other
        assert a.shape == (P.T, 1) and np.array_equal(a[:, 0], b[:, 2], equal_nan=True)


# ------------------------------------------------------------------ 2. every strategy
@pytest.mark.parametrize("strategy", ["compact", "sorted", "sweep", "direct", "prefix"])
def test_every_strategy(strategy):
    z, P, ref = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    p = _plan_of(P, z["copula_params"], strategy)
    try:
        assert p.strategy == strategy
        got = p.quantiles(LEVELS, ptf)
        assert p._wide is None                        # no sibling: the plan itself, whatever v_cap
        var, _ = p.calc_var(ptf)                      # the solve state is intact
        assert np.array_equal(var, z["var"])
        again = p.quantiles(LEVELS, ptf)
    finally:
        p.close()
    _compare(got, ref, ptf)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))


# ------------------------------------------------------------------ 3. chunk and wave edges
def _fullbatch_problem(cfg, n, T):
    """As tests/test_tail_moments_gpu.py::_fullbatch_problem: the reference's grid at n points on
    the first dates of a full-batch fixture."""
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


def _first_date_alone(P, p, got, ptf):
    """T = 1 (all parallelism from the row chunks): bit-identical to the batch's first date."""
    p.set_dates((P.fbs[:1], P.pi[:1]) if P.model == "msm" else [P.sigma[:1]])
    for a, b in zip(p.quantiles(LEVELS, ptf), got):
        assert np.array_equal(a[0], b[0], equal_nan=True)


@pytest.mark.parametrize("cfg,n", [(5, 70), (3, 130)])
def test_2d_partial_chunks(cfg, n):
    """n = 70: 2 chunks of 64 rows, the second with 6 live rows; n = 130 (Plackett): 3 chunks, the
    last with 2 rows."""
    z, P = _fullbatch_problem(cfg, n, 4)
    ptf = float(z["ptf_mean"])
    p = _plan_of(P, z["copula_params"])
    try:
        got = _check(P, p, LEVELS, ptf)
        assert not np.isnan(got[0]).any()
        _first_date_alone(P, p, got, ptf)
    finally:
        p.close()


def test_3d_partial_chunk():
    """3-D GARCH Student n = 17: 289 rows, a second 256-row chunk of 33 (a partial last wave)."""
    from oracle import forecast as F
    from oracle.quadrature import Problem
    z = load_golden("garch3d_student_n16")
    n, T = 17, 3
    x, step = F.x_grid(n, "garch")
    cp = np.array([5.0, 0.5, 0.4, 0.3])
    P = Problem("garch", "student", 3, x, step, np.ones((3, 1, n)), np.zeros((1, 3)), z["weights"], cp,
                z["sigma_forecasts"][:T])
    p = _plan_of(P, cp)
    try:
        got = _check(P, p, LEVELS, 0.0)
        assert not np.isnan(got[0]).any()
        _first_date_alone(P, p, got, 0.0)
    finally:
        p.close()


# ------------------------------------------------------------------ 4. other inputs
def _cfg2_problem(weights=None, copula_params=None):
    from oracle.quadrature import Problem
    z = load_golden("cfg2_n64")
    cp = z["copula_params"] if copula_params is None else np.asarray(copula_params, dtype=np.float64)
    w = z["weights"] if weights is None else np.asarray(weights, dtype=np.float64)
    P = Problem("msm", "student", 2, z["x_values"], z["step"], z["densities"], z["combos"], w, cp,
                (z["forecasts_by_states"], z["forecasts"]), z["unique_vol_states"])
    return z, P, cp


@pytest.mark.parametrize("weights,cp", [((0.3, 0.7), None), (None, (5.364, 0.5))])
def test_unequal_weights_and_fitted_nu(weights, cp):
    """Weights (0.3, 0.7): the division path of inner_coord; nu = 5.364: the general node power."""
    z, P, cp = _cfg2_problem(weights, cp)
    p = _plan_of(P, cp)
    try:
        _check(P, p, LEVELS, float(z["ptf_mean"]))
    finally:
        p.close()


@pytest.mark.parametrize("case,alpha,pattern", [("cfg1", 0.6, "all"), ("msm_plackett_n64", 0.2, "mixed")])
def test_levels_outside_the_bracket(case, alpha, pattern):
    z, P, _ = _ref(case)
    p = _plan_of(P, z["copula_params"])
    try:
        var, es, m0 = _check(P, p, [0.05, alpha], float(z["ptf_mean"]))
    finally:
        p.close()
    nan = np.isnan(var[:, 1])
    assert nan.all() if pattern == "all" else (nan.any() and not nan.all())
    assert np.all(m0[nan, 1] < alpha) and not np.isnan(var[:, 0]).any()


def test_non_default_bracket():
    """(-6, 0.5]: K = 23 again, other mids, and an upper end above v_cap = 0."""
    z, P, _ = _ref("cfg2_n64")
    assert Q.bisection_steps(-6.0, 0.5, 1e-6) == 23
    p = _plan_of(P, z["copula_params"])
    try:
        _check(P, p, LEVELS, float(z["ptf_mean"]), min_var=-6.0, max_var=0.5)
        assert p._wide is None
    finally:
        p.close()


def test_deterministic_batch_independent_and_consistent_with_es():
    z, P, ref = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    p = _plan_of(P, z["copula_params"])
    try:
        a = p.quantiles(LEVELS, ptf)
        b = p.quantiles(LEVELS, ptf)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        for l in range(len(LEVELS)):                  # es / m0 are expected_shortfall's of that var
            es, m0 = p.expected_shortfall(a[0][:, l], ptf)
            np.testing.assert_allclose(a[2][:, l], m0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
            assert np.all(np.abs(a[1][:, l] - es) <= ES_RTOL * (np.abs(es - ptf) + abs(ptf)))
        p.set_dates((z["forecasts_by_states"][3:7], z["forecasts"][3:7]))
        c = p.quantiles(LEVELS, ptf)
        assert all(np.array_equal(x, y[3:7]) for x, y in zip(c, a))
    finally:
        p.close()
    _compare(a, ref, ptf)


# ------------------------------------------------------------------ 5. device chaining, sharding
def test_device_chain_on_a_torch_stream():
    import torch
    from copula_var import engine
    z, P, _ = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    p = _plan_of(P, z["copula_params"])
    try:
        host = p.quantiles(LEVELS, ptf)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        args = engine.solve_args(ptf)
        with torch.cuda.stream(stream):
            out = torch.empty((3, P.T, len(LEVELS)), dtype=torch.float64, device=dev)
            only = torch.empty((P.T, len(LEVELS)), dtype=torch.float64, device=dev)
            p.set_stream(stream.cuda_stream)
            p.quantiles_device(args, LEVELS, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
            p.quantiles_device(args, LEVELS, only.data_ptr())          # es / m0 not asked for
        stream.synchronize()
        for k in range(3):
            assert np.array_equal(out[k].cpu().numpy(), host[k])
        assert np.array_equal(only.cpu().numpy(), host[0])
    finally:
        p.close()


def test_sharded_world1():
    import torch
    from copula_var import engine
    from copula_var.distributed import device_sharded_var
    z, P, _ = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    p = _plan_of(P, z["copula_params"])
    try:
        s = device_sharded_var(p, engine.solve_args(ptf), P.T, torch.device("cuda", 0), levels=LEVELS)
        got = s.quantiles(len(LEVELS)).cpu().numpy()
        host = p.quantiles(LEVELS, ptf)
        assert got.shape == (P.T, len(LEVELS), 3)
        for k in range(3):
            assert np.array_equal(got[:, :, k], host[k])
        bare = device_sharded_var(p, engine.solve_args(ptf), P.T, torch.device("cuda", 0))
        with pytest.raises(RuntimeError, match="quant_local"):
            bare.quantiles(1)
    finally:
        p.close()


# ------------------------------------------------------------------ 6. driver
@pytest.mark.parametrize("case", ["cfg2_n64", "garch_student_n64"])
def test_driver_calc_quantiles(case):
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    z, P, ref = _ref(case)
    tickers, start, kw = inject(z)
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=str(z["copula"]),
                                                               estimation_type=str(z["model"]))
    v = ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=int(z["num_points"]),
                               weights=z["weights"], copula_params=z["copula_params"], **kw)
    try:
        var, es = v.calc_quantiles(LEVELS)
        m0 = v.last_tail_mass
        var1, _ = v.calc_quantiles()
    finally:
        v.close()
    _compare((var, es, m0), ref, float(z["ptf_mean"]))
    assert np.array_equal(var1[:, 0], var[:, 2])
