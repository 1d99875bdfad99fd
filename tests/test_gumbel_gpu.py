"""Gumbel and survival-Gumbel copulas on the device (SORTED) against the numpy checker
tests/gumbel_reference.py, through every layer: slabs, solve, generic fallback, widths, grid
edges, risk numbers, sharding, driver, strategies.

Bars: slabs and m0 rtol 1e-10, atol 1e-15; ES |es - ref| <= 3e-10 (|m1 / m0| + |ptf_mean|) as
tests/test_quantiles_gpu.py; VaR and iteration count np.array_equal.  The premise of every exact
VaR comparison is asserted first: the checker's (var, iterations) does not change when every
integral it sees is scaled by 1 +- 1e-7 (every bisection decision is linear in the slabs, so this
is the decision margin, 1000 x the slab bar); for the quantiles, quantile_reference's margin."""
import functools
import os

import numpy as np
import pytest

import es_reference as E
import gumbel_reference as G
import quantile_reference as Q
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
ES_RTOL = 3e-10
MARGIN = 1e-7
LEVELS = (0.01, 0.025, 0.05)

# golden case (its arrays, the copula swapped), kind, theta
CASES = [
    ("cfg2_n64", "gumbel_survival", 1.6),            # MSM 2-D
    ("cfg2_n64", "gumbel", 3.0),
    ("garch_student_n64", "gumbel_survival", 2.2),   # GARCH 2-D
    ("cfg5_n64", "gumbel_survival", 1.3),            # UKF 2-D, 261 dead table entries
    ("cfg5_n64", "gumbel", 16.0),                    # theta at the cap
    ("cfg5_n64", "gumbel_survival", 16.0),
    ("cfg4_k4_n16", "gumbel_survival", 1.8),         # MSM 3-D
    ("garch3d_student_n16", "gumbel", 2.5),          # GARCH 3-D
    ("garch3d_student_n16", "gumbel_survival", 16.0),
    ("q1_lowvol", "gumbel_survival", 8.0),
    ("cfg1", "gumbel_survival", 4.0),
    ("msm_plackett_n64", "gumbel_survival", 2.0),
    ("ukf_plackett_n64", "gumbel_survival", 6.0),
]
IDS = [f"{c}-{k}-{th:g}" for c, k, th in CASES]
BY_CASE = {"cfg2_n64": CASES[0], "cfg5_n64": CASES[3], "cfg4_k4_n16": CASES[6], "garch3d_student_n16": CASES[7]}


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
        v, i, _ = calc_var(G.scaled(P.compute_integral, f), P.T, ptf)
        assert i == it and np.array_equal(v, var, equal_nan=True), ("premise: decision margin below 1e-7", f)
    return var, it, calls


@functools.lru_cache(maxsize=None)
def _ref(case, kind, theta):
    """(golden arrays, checker problem, (var, iterations, recorded calls)): computed once, shared."""
    z = load_golden(case)
    P = G.problem_of(z, kind, theta)
    return z, P, _solve_ref(P, float(z["ptf_mean"]))


def _plan_of(P, strategy="auto", sl=slice(None), copula=None, params=None):
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(P.model, copula or P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w,
                       P.copula_params if params is None else params,
                       vol_states=P.uvs if P.model == "msm" else None, strategy=strategy)
    p.set_dates((P.fbs[sl], P.pi[sl]) if P.model == "msm" else [P.sigma[sl]])
    return p


def _bounds_sets(P, calls):
    T = P.T
    return list(calls[:3]) + [np.column_stack((np.full(T, -100.0), np.zeros(T))),
                              np.column_stack((np.full(T, -3.0), np.full(T, 0.5)))]     # above v_cap: the sibling


def _check_slabs(P, p, bounds_sets):
    for b in bounds_sets:
        got, ref = p.compute_integral(b), P.compute_integral(b)
        print("slab rel", float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))))
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, ref, rtol=SLAB_RTOL, atol=SLAB_ATOL)


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
@pytest.mark.parametrize("case", ["cfg2_n64", "cfg4_k4_n16"])
def test_generic_fallback(case):
    """One pi_t entry scaled by 1 + 1e-3: pi_t is no outer product, every date takes node_value."""
    _, kind, theta = BY_CASE[case]
    z = dict(load_golden(case))
    z["forecasts"] = z["forecasts"].copy()
    z["forecasts"][:, 1] *= 1.0 + 1e-3
    P = G.problem_of(z, kind, theta)
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
def test_theta_one_is_the_gaussian_plan_at_rho_zero(case):
    """theta = 1: c = 1 for both kinds, as the (reference-pinned) Gaussian copula at rho = 0."""
    z = load_golden(case)
    P = G.problem_of(z, "gumbel", 1.0)
    T = P.T
    sets = [np.column_stack((np.full(T, -100.0), np.full(T, -3.0))),
            np.column_stack((np.full(T, -3.0), np.full(T, -2.0))),
            np.column_stack((np.full(T, -100.0), np.zeros(T)))]
    g = _plan_of(P, copula="gaussian", params=np.array([0.0]))
    try:
        want = [g.compute_integral(b) for b in sets]
    finally:
        g.close()
    for kind in G.KINDS:
        p = _plan_of(P, copula=kind)
        try:
            for b, w in zip(sets, want):
                np.testing.assert_allclose(p.compute_integral(b), w, rtol=SLAB_RTOL, atol=SLAB_ATOL)
        finally:
            p.close()


# ------------------------------------------------------------------ 5. widths
@pytest.mark.parametrize("case", ["cfg2_n64", "garch3d_student_n16"])
def test_widths_bit_identical(case):
    z, P, (ref, ref_it, _) = _ref(*BY_CASE[case])
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
    """The reference's own grid at n points (as tests/test_large_grid_gpu.py builds it) on the first
    dates of a fixture's sigma forecasts: 2-D UKF (fullbatch_cfg5), 3-D GARCH (garch3d_student_n16)."""
    from oracle import forecast as F
    if dim == 2:
        z = dict(np.load(os.path.join(GOLDEN, "fullbatch_cfg5.npz"), allow_pickle=False))
    else:
        z = load_golden("garch3d_student_n16")
    model = str(z["model"])
    x, step = F.x_grid(n, model)
    P = G.GumbelProblem(model, kind, dim, x, step, np.ones((dim, 1, n)), np.zeros((1, dim)), z["weights"],
                        np.array([theta]), z["sigma_forecasts"][:T])
    return float(z["ptf_mean"]) if dim == 2 else 0.0, P


@pytest.mark.parametrize("dim,n,T,kind,theta", [(2, 700, 3, "gumbel_survival", 2.0), (3, 130, 2, "gumbel_survival", 1.5)])
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
@pytest.mark.parametrize("case", ["cfg2_n64", "cfg5_n64", "cfg4_k4_n16"])
def test_risk_numbers(case):
    import torch
    from copula_var import engine
    z, P, (ref, _, calls) = _ref(*BY_CASE[case])
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
        assert p.solve_status() == _ref(*BY_CASE[case])[2][1]
        assert np.array_equal(var_d.cpu().numpy(), ref, equal_nan=True)
        assert np.array_equal(es_d[0].cpu().numpy(), es, equal_nan=True)
        assert np.array_equal(es_d[1].cpu().numpy(), m0)
        for k, h in enumerate((qv, qe, qm)):
            assert np.array_equal(q_d[k].cpu().numpy(), h, equal_nan=True)
    finally:
        p.close()


# ------------------------------------------------------------------ 8. sharding
@pytest.mark.parametrize("case", ["cfg2_n64", "garch3d_student_n16"])
def test_packed_two_way_split_equals_one_plan(case):
    import torch
    from copula_var import engine
    from copula_var.distributed import shard
    from copula_var.engine import QuadraturePlan
    z, P, (ref, ref_it, _) = _ref(*BY_CASE[case])
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
@pytest.mark.parametrize("case", ["cfg2_n64", "garch_student_n64"])
def test_driver(case):
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    c = next(x for x in CASES if x[0] == case)
    z, P, (ref, ref_it, _) = _ref(*c)
    ptf = float(z["ptf_mean"])
    tickers, start, kw = inject(z)
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=c[1], estimation_type=str(z["model"]))
    v = ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=int(z["num_points"]),
                               weights=z["weights"], copula_params=np.array([c[2]]), **kw)
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
    from copula_var.utils import calc_var_ABC as A
    from test_main_cli import _prices_csv
    for c in (A.SharedCacheCopulaMSMVaR, A.SharedCacheCopulaGarchVaR, A.SharedCacheCopulaMRVaR):
        c.cache.clear()
    SharedCacheIndexReturns.returns_cache.clear()
    SharedCacheIndexReturns.insample_cache.clear()
    p, tickers, start = _prices_csv(tmp_path)
    out = tmp_path / "var.csv"
    assert main(["--prices", str(p), "--tickers", *tickers, "--start", start, "--n-in", "1135",
                 "--copula", "gumbel_survival", "--estimation", "garch", "--num-points", "64", "--es",
                 "--exact-levels", "0.05", "--out", str(out)]) == 0
    f = pd.read_csv(out, index_col=0)
    assert list(f.columns) == ["var_garch", "garch_es", "qvar_garch_0.05", "qes_garch_0.05", "portfolio_return"]
    a = f[["var_garch", "garch_es"]].to_numpy()
    assert len(f) > 10 and np.all(np.isfinite(a)) and np.all(a[:, 1] < a[:, 0]) and np.all(a[:, 0] < 0)


# ------------------------------------------------------------------ 10. strategies
@pytest.mark.parametrize("kind", G.KINDS)
def test_strategies(kind):
    z = load_golden("cfg2_n64")
    P = G.problem_of(z, kind, 2.0)
    for strategy in ("prefix", "direct", "compact", "sweep"):
        with pytest.raises(ValueError, match="SORTED"):
            _plan_of(P, strategy)
    p = _plan_of(P, "auto")
    try:
        assert p.strategy == "sorted"
    finally:
        p.close()
    for theta, pat in ((0.5, "theta"), (17.0, "16")):
        with pytest.raises(ValueError, match=pat):
            _plan_of(P, params=np.array([theta]))


# ------------------------------------------------------------------ 11. the tables' floor
@pytest.mark.parametrize("kind", G.KINDS)
def test_floored_corner(kind):
    """theta = 16 on an MSM grid whose lowest points have u < 1e-20 on both axes: under the survival kind
    x^16 < 1e-300 there and the device tables floor it (tests/test_gumbel_cpu.py bounds the effect by
    those nodes' own mass, < 1e-15); fast path (slabs), generic path (moments) and a non-rank-1 pi."""
    P = G.corner_problem(kind)
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
    P2 = G.corner_problem(kind)
    P2.pi[:, 1] *= 1.0 + 1e-3                                      # generic SORTED path
    p = _plan_of(P2)
    try:
        _check_slabs(P2, p, sets)
    finally:
        p.close()
