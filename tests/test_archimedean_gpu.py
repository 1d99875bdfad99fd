"""Frank, Joe and survival-Joe copulas on the device (SORTED) against the longdouble checker
tests/archimedean_reference.py, through every layer: slabs, solve, generic fallback, independence,
widths, grid edges, risk numbers, sharding, driver, strategies, the tables' floor, and one case
per family of attribution, CoVaR, weight batches and per-date parameter paths.

Bars (tests/test_gumbel_gpu.py's): slabs and m0 rtol 1e-10, atol 1e-15; ES |es - ref| <= 3e-10
(|m1 / m0| + |ptf_mean|); VaR, iteration count and exact quantiles np.array_equal.  The premise of
every exact comparison is asserted first: the checker's (var, iterations) does not change when
every integral it sees is scaled by 1 +- 1e-7; for the quantile checkers, their margin >= 1e-7."""
import functools
import os

import numpy as np
import pytest

import archimedean_reference as A
import es_reference as E
import quantile_reference as Q
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
ES_RTOL = 3e-10
MARGIN = 1e-7
LEVELS = (0.01, 0.025, 0.05)

CASES = list(A.TABLE1)
IDS = [f"{c}-{k}-{th:g}" for c, k, th in CASES]
FRANK2, JOES2, JOE2 = CASES[0], CASES[1], CASES[2]           # cfg2_n64 (MSM 2-D)
FRANK5, JOE5 = CASES[5], CASES[7]                            # cfg5_n64 (UKF 2-D, dead table entries), theta at the caps
FRANK3, JOES3 = CASES[10], CASES[11]                         # cfg4_k4_n16 (MSM 3-D)
JOE3G = CASES[12]                                            # garch3d_student_n16 (GARCH 3-D)
FRANK_PATH = np.array([0.25, 1.0, 3.0, 6.0, 12.0, 32.0])
JOE_PATH = np.array([1.0, 1.3, 1.6, 2.5, 5.0, 16.0])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


def _solve_ref(P, ptf):
    """The checker's solve with its calls recorded and the premise of an exact comparison asserted."""
    from oracle.quadrature import calc_var
    calls = []

    def ci(b):
        calls.append(np.array(b, dtype=np.float64))
        return P.compute_integral(b)

    var, it, _ = calc_var(ci, P.T, ptf)
    for f in (1.0 - MARGIN, 1.0 + MARGIN):
        v, i, _ = calc_var(A.scaled(P.compute_integral, f), P.T, ptf)
        assert i == it and np.array_equal(v, var, equal_nan=True), ("premise: decision margin below 1e-7", f)
    return var, it, calls


@functools.lru_cache(maxsize=None)
def _ref(case, kind, theta):
    """(golden arrays, checker problem, (var, iterations, recorded calls)): computed once, shared."""
    z = load_golden(case)
    P = A.problem_of(z, kind, theta)
    return z, P, _solve_ref(P, float(z["ptf_mean"]))


def _plan_of(P, strategy="auto", sl=slice(None), copula=None, params=None, weights=None):
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(P.model, copula or P.copula, P.dim, P.x, P.step, P.dens, P.combos,
                       P.w if weights is None else weights, P.copula_params if params is None else params,
                       vol_states=P.uvs if P.model == "msm" else None, strategy=strategy)
    p.set_dates((P.fbs[sl], P.pi[sl]) if P.model == "msm" else [P.sigma[sl]])
    return p


def _bounds_sets(P, calls):
    T = P.T
    return list(calls[:3]) + [np.column_stack((np.full(T, -100.0), np.zeros(T))),
                              np.column_stack((np.full(T, -3.0), np.full(T, 0.5)))]     # above v_cap: the sibling


def _check_slabs(P, p, bounds_sets):
    worst = 0.0
    for b in bounds_sets:
        got, ref = p.compute_integral(b), P.compute_integral(b)
        worst = max(worst, float(np.max(np.maximum(np.abs(got - ref) - SLAB_ATOL, 0.0) / np.maximum(np.abs(ref), 1e-300))))
        print("slab rel", worst)
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, ref, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    return worst


def _es_ok(es, res, ptf):
    assert np.array_equal(np.isnan(es), np.isnan(res))
    ok = ~np.isnan(res)
    print("es err / bar", float(np.max(np.abs(es[ok] - res[ok]) / (ES_RTOL * (np.abs(res[ok] - ptf) + abs(ptf))),
                                       initial=0.0)))
    assert np.all(np.abs(es[ok] - res[ok]) <= ES_RTOL * (np.abs(res[ok] - ptf) + abs(ptf)))


# ------------------------------------------------------------------ 1. slabs
@pytest.mark.parametrize("case,kind,theta", CASES, ids=IDS)
def test_slabs(case, kind, theta):
    z, P, (_, _, calls) = _ref(case, kind, theta)
    p = _plan_of(P)
    try:
        assert p.strategy == "sorted"
        _check_slabs(P, p, _bounds_sets(P, calls))
        assert p._wide is not None and p._wide.strategy == "sorted"     # 2-D too: no COMPACT instances
    finally:
        p.close()


# ------------------------------------------------------------------ 2. solve
@pytest.mark.parametrize("case,kind,theta", CASES, ids=IDS)
def test_solve(case, kind, theta):
    z, P, (ref, ref_it, _) = _ref(case, kind, theta)
    ptf = float(z["ptf_mean"])
    p = _plan_of(P)
    try:
        var, it = p.calc_var(ptf)
        again, it2 = p.calc_var(ptf)
    finally:
        p.close()
    assert it == ref_it
    assert np.array_equal(var, ref, equal_nan=True), float(np.nanmax(np.abs(var - ref)))
    assert it2 == it and np.array_equal(again, var, equal_nan=True)


# ------------------------------------------------------------------ 3. generic fallback
@pytest.mark.parametrize("case,kind,theta", [FRANK2, JOES2, FRANK3, JOES3], ids=lambda v: str(v))
def test_generic_fallback(case, kind, theta):
    """One pi_t entry scaled by 1 + 1e-3: pi_t is no outer product, every date takes node_value."""
    z = dict(load_golden(case))
    z["forecasts"] = z["forecasts"].copy()
    z["forecasts"][:, 1] *= 1.0 + 1e-3
    P = A.problem_of(z, kind, theta)
    ptf = float(z["ptf_mean"])
    ref, ref_it, calls = _solve_ref(P, ptf)
    p = _plan_of(P)
    try:
        _check_slabs(P, p, _bounds_sets(P, calls))
        var, it = p.calc_var(ptf)
    finally:
        p.close()
    assert it == ref_it and np.array_equal(var, ref, equal_nan=True)


# ------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("case", ["cfg2_n64", "garch_student_n64"])
def test_joe_theta_one_is_the_gaussian_plan_at_rho_zero(case):
    """theta = 1: c = 1 for both Joe kinds, as the (reference-pinned) Gaussian copula at rho = 0."""
    z = load_golden(case)
    P = A.problem_of(z, "joe", 1.0)
    T = P.T
    sets = [np.column_stack((np.full(T, -100.0), np.full(T, -3.0))),
            np.column_stack((np.full(T, -3.0), np.full(T, -2.0))),
            np.column_stack((np.full(T, -100.0), np.zeros(T)))]
    g = _plan_of(P, copula="gaussian", params=np.array([0.0]))
    try:
        want = [g.compute_integral(b) for b in sets]
    finally:
        g.close()
    for kind in ("joe", "joe_survival"):
        p = _plan_of(P, copula=kind)
        try:
            for b, w in zip(sets, want):
                np.testing.assert_allclose(p.compute_integral(b), w, rtol=SLAB_RTOL, atol=SLAB_ATOL)
        finally:
            p.close()


# ------------------------------------------------------------------ 5. widths
@pytest.mark.parametrize("case,kind,theta", [FRANK2, JOES2, JOE3G, CASES[14]], ids=lambda v: str(v))
def test_widths_bit_identical(case, kind, theta):
    z, P, (ref, ref_it, _) = _ref(case, kind, theta)
    ptf = float(z["ptf_mean"])
    p = _plan_of(P, "sorted")
    out = {}
    try:
        for w in ("256", "384", "512", "1024"):
            p.set_sorted_threads(int(w))
            assert p.sorted_threads() == int(w)
            out[w] = p.calc_var(ptf)
    finally:
        p.close()
    for w, (v, it) in out.items():
        assert it == ref_it, (w, it)
        assert np.array_equal(v, ref, equal_nan=True), (w, float(np.nanmax(np.abs(v - ref))))


# ------------------------------------------------------------------ 6. grid edges
def _grid_problem(dim, n, T, kind, theta):
    """The reference's own grid at n points (as tests/test_gumbel_gpu.py builds it) on the first dates
    of a fixture's sigma forecasts: 2-D UKF (fullbatch_cfg5), 3-D GARCH (garch3d_student_n16)."""
    from oracle import forecast as F
    if dim == 2:
        z = dict(np.load(os.path.join(GOLDEN, "fullbatch_cfg5.npz"), allow_pickle=False))
    else:
        z = load_golden("garch3d_student_n16")
    model = str(z["model"])
    x, step = F.x_grid(n, model)
    P = A.ArchimedeanProblem(model, kind, dim, x, step, np.ones((dim, 1, n)), np.zeros((1, dim)), z["weights"],
                             np.array([theta]), z["sigma_forecasts"][:T])
    return float(z["ptf_mean"]) if dim == 2 else 0.0, P


@pytest.mark.parametrize("dim,n,T,kind,theta", [(2, 700, 3, "joe_survival", 2.0), (2, 700, 3, "frank", 8.0),
                                                (3, 130, 2, "frank", 5.0), (3, 130, 2, "joe_survival", 1.5)])
def test_grid_edges(dim, n, T, kind, theta):
    """2-D n = 700: the 1024-thread instance; 3-D n = 130: the large 3-D node layout (n > 128) and,
    for the moments, 16900 rows = 66 chunks of 256 with a last chunk of 4."""
    ptf, P = _grid_problem(dim, n, T, kind, theta)
    ref, ref_it, calls = _solve_ref(P, ptf)
    p = _plan_of(P)
    try:
        assert p.strategy == "sorted"
        _check_slabs(P, p, _bounds_sets(P, calls))
        var, it = p.calc_var(ptf)
        b = np.column_stack((np.full(T, -100.0), np.full(T, -3.0)))
        m0, m1 = p.tail_moments(b)
    finally:
        p.close()
    assert it == ref_it and np.array_equal(var, ref, equal_nan=True)
    r0, r1, _ = E.tail_moments(P, b)
    np.testing.assert_allclose(m0, r0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    np.testing.assert_allclose(m1, r1, rtol=SLAB_RTOL, atol=SLAB_ATOL)


# ------------------------------------------------------------------ 7. risk numbers
@pytest.mark.parametrize("case,kind,theta", [FRANK2, JOES2, FRANK5, JOE5, JOES3, JOE3G], ids=lambda v: str(v))
def test_risk_numbers(case, kind, theta):
    import torch
    from copula_var import engine
    z, P, (ref, ref_it, calls) = _ref(case, kind, theta)
    ptf = float(z["ptf_mean"])
    T = P.T
    qref = Q.quantiles(P, LEVELS, ptf)
    print("quantile margin", float(qref[3].min()))
    assert qref[3].min() >= MARGIN
    p = _plan_of(P)
    try:
        for b in (calls[0], calls[1], np.column_stack((np.full(T, -100.0), np.zeros(T)))):
            m0, m1 = p.tail_moments(b)
            r0, r1, _ = E.tail_moments(P, b)
            np.testing.assert_allclose(m0, r0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
            np.testing.assert_allclose(m1, r1, rtol=SLAB_RTOL, atol=SLAB_ATOL)     # bounds <= 0: one sign
        es, m0 = p.expected_shortfall(ref, ptf)
        res, rm0, _, _ = E.expected_shortfall(P, ref, ptf)
        np.testing.assert_allclose(m0, rm0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
        _es_ok(es, res, ptf)
        qv, qe, qm = p.quantiles(LEVELS, ptf)
        assert np.array_equal(qv, qref[0], equal_nan=True)
        np.testing.assert_allclose(qm, qref[2], rtol=SLAB_RTOL, atol=SLAB_ATOL)
        for l in range(len(LEVELS)):
            _es_ok(qe[:, l], qref[1][:, l], ptf)
        # device mode: solve -> ES -> quantiles chained on one stream, no host synchronisation between
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        args = engine.solve_args(ptf)
        with torch.cuda.stream(stream):
            var_d = torch.empty(T, dtype=torch.float64, device=dev)
            es_d = torch.empty((2, T), dtype=torch.float64, device=dev)
            q_d = torch.empty((3, T, len(LEVELS)), dtype=torch.float64, device=dev)
            p.set_stream(stream.cuda_stream)
            p.solve_device(args, var_d.data_ptr())
            p.expected_shortfall_device(args, var_d.data_ptr(), es_d[0].data_ptr(), es_d[1].data_ptr())
            p.quantiles_device(args, LEVELS, q_d[0].data_ptr(), q_d[1].data_ptr(), q_d[2].data_ptr())
        stream.synchronize()
        assert p.solve_status() == ref_it
        assert np.array_equal(var_d.cpu().numpy(), ref, equal_nan=True)
        assert np.array_equal(es_d[0].cpu().numpy(), es, equal_nan=True)
        assert np.array_equal(es_d[1].cpu().numpy(), m0)
        for k, h in enumerate((qv, qe, qm)):
            assert np.array_equal(q_d[k].cpu().numpy(), h, equal_nan=True)
    finally:
        p.close()


# ------------------------------------------------------------------ 8. sharding
@pytest.mark.parametrize("case,kind,theta", [FRANK2, JOE3G], ids=lambda v: str(v))
def test_packed_two_way_split_equals_one_plan(case, kind, theta):
    import torch
    from copula_var import engine
    from copula_var.distributed import shard
    from copula_var.engine import QuadraturePlan
    z, P, (ref, ref_it, _) = _ref(case, kind, theta)
    T, ranks = P.T, 2
    args = engine.solve_args(float(z["ptf_mean"]))
    per = shard(T, 0, ranks)[2]
    ln, off = QuadraturePlan.packed_block_len(args, per)
    blocks = torch.full((ranks, ln), float("nan"), dtype=torch.float64, device="cuda")
    plans = []
    try:
        one = _plan_of(P, "sorted")
        plans.append(one)
        whole, it = one.calc_var(float(z["ptf_mean"]))
        for r in range(ranks):
            lo, hi, _ = shard(T, r, ranks)
            p = _plan_of(P, "sorted", slice(lo, hi))
            p.set_stream(torch.cuda.current_stream().cuda_stream)
            plans.append(p)
            blk = blocks[r]
            blk[off: off + 2] = 0.0
            p.solve_local(args, blk[off:].data_ptr(), blk.data_ptr())
        for p in plans[1:]:
            var = torch.empty(T, dtype=torch.float64, device="cuda")
            p.solve_finalize_packed(args, blocks.data_ptr(), ranks, per, T, var.data_ptr())
            assert p.solve_status() == it == ref_it
            assert np.array_equal(var.cpu().numpy(), whole, equal_nan=True)
        assert np.array_equal(whole, ref, equal_nan=True)
    finally:
        for p in plans:
            p.close()


# ------------------------------------------------------------------ 9. driver
@pytest.mark.parametrize("case,kind,theta", [FRANK2, CASES[4]], ids=lambda v: str(v))
def test_driver(case, kind, theta):
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    z, P, (ref, ref_it, _) = _ref(case, kind, theta)
    ptf = float(z["ptf_mean"])
    tickers, start, kw = inject(z)
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=kind, estimation_type=str(z["model"]))
    v = ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=int(z["num_points"]),
                               weights=z["weights"], copula_params=np.array([theta]), **kw)
    try:
        assert v.plan.strategy == "sorted"
        var = v.calc_var()
        es = v.calc_es(var=var)
        assert v.last_iterations == ref_it
    finally:
        v.close()
    assert np.array_equal(var, ref, equal_nan=True)
    _es_ok(es, E.expected_shortfall(P, ref, ptf)[0], ptf)


def test_cli_runs_with_es(tmp_path):
    import pandas as pd
    from copula_var.data_loader.load_data import SharedCacheIndexReturns
    from copula_var.main import main
    from copula_var.utils import calc_var_ABC as ABC
    from test_main_cli import _prices_csv
    for c in (ABC.SharedCacheCopulaMSMVaR, ABC.SharedCacheCopulaGarchVaR, ABC.SharedCacheCopulaMRVaR):
        c.cache.clear()
    SharedCacheIndexReturns.returns_cache.clear()
    SharedCacheIndexReturns.insample_cache.clear()
    p, tickers, start = _prices_csv(tmp_path)
    out = tmp_path / "var.csv"
    assert main(["--prices", str(p), "--tickers", *tickers, "--start", start, "--n-in", "1135",
                 "--copula", "frank", "--estimation", "garch", "--num-points", "64", "--es",
                 "--exact-levels", "0.05", "--out", str(out)]) == 0
    f = pd.read_csv(out, index_col=0)
    assert list(f.columns) == ["var_garch", "garch_es", "qvar_garch_0.05", "qes_garch_0.05", "portfolio_return"]
    a = f[["var_garch", "garch_es"]].to_numpy()
    assert len(f) > 10 and np.all(np.isfinite(a)) and np.all(a[:, 1] < a[:, 0]) and np.all(a[:, 0] < 0)


# ------------------------------------------------------------------ 10. strategies and theta limits
@pytest.mark.parametrize("kind", A.KINDS)
def test_strategies_and_theta_refusals(kind):
    z = load_golden("cfg2_n64")
    P = A.problem_of(z, kind, 2.0)
    for strategy in ("prefix", "direct", "compact", "sweep"):
        with pytest.raises(ValueError, match="SORTED"):
            _plan_of(P, strategy)
    p = _plan_of(P, "auto")
    try:
        assert p.strategy == "sorted"
    finally:
        p.close()
    bad = ((0.0, "theta"), (-1.0, "theta"), (32.5, "32")) if kind == "frank" else ((0.5, "theta"), (17.0, "16"))
    for theta, pat in bad:
        with pytest.raises(ValueError, match=pat):
            _plan_of(P, params=np.array([theta]))
    with pytest.raises((ValueError, KeyError)):
        _plan_of(P, copula="clayton")


# ------------------------------------------------------------------ 11. the tables' floor
@pytest.mark.parametrize("kind,theta", [("joe_survival", 16.0), ("joe", 16.0), ("frank", 32.0)])
def test_floored_corner(kind, theta):
    """theta at the cap on an MSM grid whose lowest points have u < 1e-20 on both axes: under survival
    Joe a ~ u^16 < 1e-300 there and the device tables floor it (tests/test_archimedean_cpu.py bounds the
    effect); fast path (slabs), generic path (moments) and a non-rank-1 pi."""
    P = A.corner_problem(kind, theta)
    T = P.T
    sets = [np.column_stack((np.full(T, a), np.full(T, b)))
            for a, b in ((-100.0, -4.5), (-4.9, -4.4), (-100.0, -3.0), (-100.0, -1.0), (-100.0, 0.0))]
    assert float(P.compute_integral(sets[-1]).min()) > 0.1       # the measure is there
    p = _plan_of(P)
    try:
        _check_slabs(P, p, sets)
        for b in sets:
            m0, m1 = p.tail_moments(b)
            r0, r1, _ = E.tail_moments(P, b)
            np.testing.assert_allclose(m0, r0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
            np.testing.assert_allclose(m1, r1, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    finally:
        p.close()
    P2 = A.corner_problem(kind, theta)
    P2.pi[:, 1] *= 1.0 + 1e-3                                      # generic SORTED path
    p = _plan_of(P2)
    try:
        _check_slabs(P2, p, sets)
    finally:
        p.close()


# ------------------------------------------------------------------ 12. attribution
@pytest.mark.parametrize("case,kind,theta", [FRANK2, JOE5, JOES3], ids=lambda v: str(v))
def test_attribution(case, kind, theta):
    """Contributions against attribution_reference and summing to the ES (test_attribution_gpu's checks)."""
    from test_attribution_gpu import _check_contrib, _check_moments, _tail_bounds
    z, P, (ref, _, _) = _ref(case, kind, theta)
    ptf = float(z["ptf_mean"])
    p = _plan_of(P)
    try:
        _check_contrib(P, p, ref, ptf)
        _check_moments(P, p, _tail_bounds(P, ref, ptf))
    finally:
        p.close()


# ------------------------------------------------------------------ 13. CoVaR
COVAR_LEVELS = (0.05, 0.5)


def covar_reference(case, kind, theta, axis=0):
    import conditional_reference as CR
    z = load_golden(case)
    P = A.problem_of(z, kind, theta)
    ptf = float(z["ptf_mean"])
    cond = np.column_stack((np.full(P.T, -np.inf), CR.marginal_quantile(P, axis, 0.05)))
    return P, ptf, cond, CR.conditional_quantiles(P, axis, cond[:, 0], cond[:, 1], COVAR_LEVELS, ptf)


@pytest.mark.parametrize("case,kind,theta", [FRANK2, JOE5, JOES3], ids=lambda v: str(v))
def test_covar(case, kind, theta):
    """Event (-inf, the asset's 5 % marginal quantile], levels (0.05, 0.5), test_conditional_gpu's comparison."""
    from test_conditional_gpu import _compare
    P, ptf, cond, ref = covar_reference(case, kind, theta)
    p = _plan_of(P)
    try:
        got = p.conditional_quantiles(0, cond, COVAR_LEVELS, ptf)
    finally:
        p.close()
    _compare(got, ref, ptf)


# ------------------------------------------------------------------ 14. weight batches
def portfolio_reference_of(case, kind, theta):
    import portfolio_reference as R
    z = load_golden(case)
    dim = int(z["dim"])
    P = A.problem_of(z, kind, theta, slice(0, 6 if dim == 2 else 4))
    w = R.W2 if dim == 2 else R.W3
    return P, w, R.portfolio_quantiles(P, w, R.LEVELS, R.means(len(w)))


@pytest.mark.parametrize("case,kind,theta", [FRANK2, JOE5, JOES3], ids=lambda v: str(v))
def test_weight_batches(case, kind, theta):
    import portfolio_reference as R
    from test_portfolio_gpu import _compare
    P, w, ref = portfolio_reference_of(case, kind, theta)
    p = _plan_of(P)
    try:
        got = p.portfolio_quantiles(w, R.LEVELS, R.means(len(w)))
    finally:
        p.close()
    _compare(got, ref, R.means(len(w)))


# ------------------------------------------------------------------ 15. per-date parameter paths
def dynamic_reference_of(case, kind):
    """(base Problem, copula_params_t, weights_t, ptf_mean_t, per-date Problems, checker result)."""
    import dynamic_reference as R
    z = dict(load_golden(case))
    dim = int(z["dim"])
    T = 6 if dim == 2 else 4
    path = (FRANK_PATH if kind == "frank" else JOE_PATH)[:T]
    w = (R.W2 if dim == 2 else R.W3)[:T]
    P = A.problem_of(z, kind, path[2], slice(0, T))
    dates = []
    for t in range(T):
        z["weights"] = w[t]
        dates.append(A.problem_of(z, kind, path[t], slice(t, t + 1)))
    pm = R.means(T)
    return P, path[:, None].copy(), w.copy(), pm, dates, R.dynamic_quantiles(dates, R.LEVELS, pm)


@pytest.mark.parametrize("case,kind", [("cfg2_n64", "frank"), ("cfg5_n64", "joe"), ("cfg4_k4_n16", "joe_survival"),
                                       ("garch3d_student_n16", "frank")])
def test_per_date_paths(case, kind):
    """cvq_dynamic_quantiles on the theta paths Frank (0.25 .. 32) / Joe (1 .. 16) with per-date weights:
    against the checker (test_dynamic_gpu's comparison) and, bit for bit, against a plan built with
    each date's theta and weights."""
    import dynamic_reference as R
    from test_dynamic_gpu import _compare, _same
    P, cp, w, pm, dates, ref = dynamic_reference_of(case, kind)
    p = _plan_of(P)
    try:
        got = p.dynamic_quantiles(R.LEVELS, cp, w, pm)
    finally:
        p.close()
    _compare(got, ref, pm)
    for t, Pt in enumerate(dates):
        q = _plan_of(Pt)
        try:
            one = q.quantiles(R.LEVELS, float(pm[t]))
        finally:
            q.close()
        assert _same(one, [g[t:t + 1] for g in got]), (case, kind, t)


def test_per_date_theta_refusals():
    from copula_var import _native as N
    P, cp, w, pm, _, _ = dynamic_reference_of("cfg2_n64", "frank")
    p = _plan_of(P)
    try:
        for bad, pat in ((0.0, "at date 3"), (-1.0, "at date 3"), (33.0, "32")):
            th = cp.copy()
            th[3, 0] = bad
            with pytest.raises(ValueError, match=pat):
                p.dynamic_quantiles((0.05,), th, w, pm)
    finally:
        p.close()
    assert N.COPULA_KIND["frank"] == 5
