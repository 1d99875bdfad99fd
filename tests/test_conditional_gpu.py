"""Conditional quantiles on the device (cvq_conditional_quantiles: CoVaR / CoES) against the numpy
checker tests/conditional_reference.py, through every layer: plan, device chaining, sharding,
driver.  The inputs and the checker's results come from tests/conditional_cases.py.

Bars, tests/test_quantiles_gpu.py's: covar with np.array_equal, after asserting the premise
(margin >= 1e-7, tests/test_conditional_cpu.py); m0 and p_event at the slab bar (rtol 1e-10, atol
1e-15); |coes - ref| <= 3e-10 (|ref - ptf_mean| + |ptf_mean|); NaN patterns equal.
What the margin-1e-7 comparison cannot see (1e-8 of relative error in F, the narrow passes) is held by tests/test_quantile_probes_gpu.py."""
import numpy as np
import pytest

import conditional_cases as CC
import conditional_reference as CR
import es_reference as E

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
ES_RTOL = 3e-10
MARGIN = 1e-7
LEVELS = CC.LEVELS
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


def _plan_of(P, copula_params, strategy="auto", sl=slice(None)):
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w, copula_params,
                       vol_states=P.uvs if P.model == "msm" else None, strategy=strategy)
    _set_dates(p, P, sl)
    return p


def _set_dates(p, P, sl=slice(None)):
    p.set_dates((P.fbs[sl], P.pi[sl]) if P.model == "msm" else [P.sigma[sl]])


def _compare(got, ref, ptf):
    """Device (covar, coes, m0, p_event) against the checker's (covar, coes, m0, p_event, margin)."""
    covar, coes, m0, pe = got
    rcovar, rcoes, rm0, rpe, margin = ref
    print("margin", margin.min(), "m0 rel", np.max(np.abs(m0 - rm0) / np.maximum(np.abs(rm0), 1e-300)),
          "p_E rel", np.max(np.abs(pe - rpe) / np.maximum(np.abs(rpe), 1e-300)),
          "coes err / bar", np.nanmax(np.abs(coes - rcoes) / (ES_RTOL * (np.abs(rcoes - ptf) + abs(ptf))), initial=0.0),
          "NaN", int(np.isnan(rcovar).sum()), "of", rcovar.size)
    assert margin.min() >= MARGIN                     # the premise of the exact comparison
    assert covar.shape == rcovar.shape and pe.shape == rpe.shape
    assert np.array_equal(np.isnan(covar), np.isnan(rcovar)) and np.array_equal(np.isnan(coes), np.isnan(rcoes))
    assert np.array_equal(covar, rcovar, equal_nan=True)
    np.testing.assert_allclose(m0, rm0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    np.testing.assert_allclose(pe, rpe, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    assert np.array_equal(pe == 0.0, rpe == 0.0)
    ok = ~np.isnan(rcoes)
    assert np.all(np.abs(coes[ok] - rcoes[ok]) <= ES_RTOL * (np.abs(rcoes[ok] - ptf) + abs(ptf)))


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _run_cases(name, axes_kinds, first_date_alone=False):
    """One plan of `name`; every (axis, event kind) against the checker."""
    P, cp, ptf = CC.problem(name)
    p = _plan_of(P, cp)
    got = {}
    try:
        for axis, kind in axes_kinds:
            cond = CC.reference(name, axis, kind)[3]
            got[axis, kind] = p.conditional_quantiles(axis, cond, LEVELS, ptf)
        if first_date_alone:                          # T = 1: bit-identical to the batch's first date
            _set_dates(p, P, slice(0, 1))
            for (axis, kind), g in got.items():
                cond = CC.reference(name, axis, kind)[3]
                one = p.conditional_quantiles(axis, cond[:1], LEVELS, ptf)
                assert all(np.array_equal(a[0], b[0], equal_nan=True) for a, b in zip(one, g)), (axis, kind)
    finally:
        p.close()
    for (axis, kind), g in got.items():
        print(name, "axis", axis, kind)
        _compare(g, CC.reference(name, axis, kind)[4], ptf)
    return got


# ------------------------------------------------------------------ 1. every small golden, every axis
@pytest.mark.parametrize("case", CC.SMALL)
def test_stress_event_on_every_small_golden(case):
    got = _run_cases(case, [(a, "stress") for a in CC._axes(case)])
    if case == "cfg1_hivol":                          # the event holds no grid node: p_E = 0, all NaN
        covar, coes, m0, pe = got[0, "stress"]
        assert np.all(pe == 0.0) and np.isnan(covar).all() and np.isnan(coes).all() and np.all(m0 == 0.0)
        assert int((got[1, "stress"][3] == 0.0).sum()) == 9


# ------------------------------------------------------------------ 2. band event
@pytest.mark.parametrize("case", ["cfg2_n64", "cfg5_n64", "garch3d_student_n16"])
def test_band_event(case):
    _run_cases(case, [(a, "band") for a in CC._axes(case)])


# ------------------------------------------------------------------ 3. chunk and wave edges
@pytest.mark.parametrize("name,kinds", [("fullbatch5_n70", ("stress", "band")), ("fullbatch3_n130", ("stress",)),
                                        ("garch3d_n17", ("stress",))])
def test_partial_chunks(name, kinds):
    """n = 70: 2 chunks of 64 rows, the second with 6 live rows; n = 130 (Plackett): 3 chunks (stress
    only: the band's p_E is 1e2 - 1e4 there and every level lies outside the bracket); 3-D n = 17: 289
    rows, a second 256-row chunk of 33."""
    got = _run_cases(name, [(a, k) for a in CC._axes(name) for k in kinds], first_date_alone=True)
    assert any(not np.isnan(g[0]).any() for g in got.values())


# ------------------------------------------------------------------ 4. bounds exactly on grid values
@pytest.mark.parametrize("axis", [0, 1])
def test_bounds_on_grid_values_and_empty_events(axis):
    """(x[10], x[25]]: strict below, inclusive above.  Then date 0's s_lo = NaN, date 1's
    s_hi = s_lo, date 2's s_hi = -inf: those rows NaN with p_event == 0, the others untouched."""
    P, cp, ptf = CC.problem("cfg2_n64")
    _, _, _, cond, ref = CC.reference("cfg2_n64", axis, "grid")
    bad = np.array(cond)
    bad[0, 0] = np.nan
    bad[1, 1] = bad[1, 0]
    bad[2, 1] = -INF
    p = _plan_of(P, cp)
    try:
        got = p.conditional_quantiles(axis, cond, LEVELS, ptf)
        dis = p.conditional_quantiles(axis, bad, LEVELS, ptf)
    finally:
        p.close()
    _compare(got, ref, ptf)
    assert not np.isnan(got[0][:, :2]).any() and np.all(got[3] > 0.0)
    # one grid step inwards on either side changes p_E: the comparisons sit exactly on the nodes
    inner = CR.conditional_quantiles(P, axis, P.x[11], P.x[24], LEVELS, ptf)[3]
    assert np.all(ref[3] > inner)
    covar, coes, m0, pe = dis
    assert np.isnan(covar[:3]).all() and np.isnan(coes[:3]).all() and np.all(pe[:3] == 0.0) and np.all(m0[:3] == 0.0)
    assert all(np.array_equal(a[3:], b[3:], equal_nan=True) for a, b in zip(dis, got))


# ------------------------------------------------------------------ 5. full event
def test_full_event_is_the_same_on_both_axes():
    P, cp, ptf = CC.problem("cfg2_n64")
    cond = CC.reference("cfg2_n64", 0, "full")[3]
    p = _plan_of(P, cp)
    try:
        a0 = p.conditional_quantiles(0, cond, LEVELS, ptf)
        a1 = p.conditional_quantiles(1, cond, LEVELS, ptf)
        m0, _ = p.tail_moments(np.column_stack((np.full(P.T, -100.0), np.full(P.T, INF))))
    finally:
        p.close()
    assert _same(a0, a1)
    _compare(a0, CC.reference("cfg2_n64", 0, "full")[4], ptf)
    _compare(a1, CC.reference("cfg2_n64", 1, "full")[4], ptf)
    np.testing.assert_allclose(a0[3], m0, rtol=SLAB_RTOL, atol=0.0)
    rm0, _, _ = E.tail_moments(P, np.column_stack((np.full(P.T, -100.0), np.full(P.T, INF))))
    np.testing.assert_allclose(a0[3], rm0, rtol=SLAB_RTOL, atol=0.0)


# ------------------------------------------------------------------ 6. every strategy
@pytest.mark.parametrize("strategy", ["compact", "sorted", "sweep", "direct", "prefix"])
def test_every_strategy(strategy):
    from conftest import load_golden
    P, cp, ptf = CC.problem("cfg2_n64")
    z = load_golden("cfg2_n64")
    p = _plan_of(P, cp, strategy)
    try:
        assert p.strategy == strategy
        got = [p.conditional_quantiles(a, CC.reference("cfg2_n64", a, "stress")[3], LEVELS, ptf) for a in range(2)]
        assert p._wide is None                        # no sibling: the plan itself, whatever v_cap
        var, _ = p.calc_var(ptf)                      # the solve state is intact
        assert np.array_equal(var, z["var"])
        again = [p.conditional_quantiles(a, CC.reference("cfg2_n64", a, "stress")[3], LEVELS, ptf) for a in range(2)]
    finally:
        p.close()
    for a in range(2):
        _compare(got[a], CC.reference("cfg2_n64", a, "stress")[4], ptf)
        assert _same(got[a], again[a])


# ------------------------------------------------------------------ 7. other inputs
@pytest.mark.parametrize("name", ["cfg2_weights", "cfg2_nu", "cfg2_gumbel_survival"])
def test_unequal_weights_fitted_nu_and_survival_gumbel(name):
    """Weights (0.3, 0.7): the division path of inner_coord; nu = 5.364: the general node power;
    gumbel_survival (theta = 2) against tests/gumbel_reference.py's Problem."""
    _run_cases(name, [(a, "stress") for a in range(2)])


# ------------------------------------------------------------------ 8. determinism and independence
def test_levels_and_dates_do_not_see_each_other():
    P, cp, ptf = CC.problem("cfg2_n64")
    p = _plan_of(P, cp)
    try:
        for axis in range(2):
            cond = CC.reference("cfg2_n64", axis, "stress")[3]
            a = p.conditional_quantiles(axis, cond, LEVELS, ptf)
            one = p.conditional_quantiles(axis, cond, [LEVELS[2]], ptf)
            for x, y in zip(one[:3], a[:3]):
                assert x.shape == (P.T, 1) and np.array_equal(x[:, 0], y[:, 2], equal_nan=True)
            assert np.array_equal(one[3], a[3])
            _set_dates(p, P, slice(3, 7))
            c = p.conditional_quantiles(axis, cond[3:7], LEVELS, ptf)
            assert all(np.array_equal(x, y[3:7], equal_nan=True) for x, y in zip(c, a))
            # m0 is F_E at the returned covar: a call whose bracket ends there, at a level above
            # everything, reports F_E(max_var) from the opening pass alone
            for t in range(3):
                _set_dates(p, P, slice(t, t + 1))
                for l in range(len(LEVELS)):
                    top = p.conditional_quantiles(axis, cond[t:t + 1], [1e6], ptf, max_var=a[0][t, l] - ptf)
                    assert np.isnan(top[0]).all()
                    np.testing.assert_allclose(top[2][0, 0], a[2][t, l], rtol=SLAB_RTOL, atol=SLAB_ATOL)
            _set_dates(p, P)
    finally:
        p.close()


# ------------------------------------------------------------------ 9. device mode, sharding
def test_device_mode_on_a_torch_stream():
    import torch
    from copula_var import engine
    P, cp, ptf = CC.problem("cfg2_n64")
    L = len(LEVELS)
    p = _plan_of(P, cp)
    try:
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        args = engine.solve_args(ptf)
        for axis in range(2):
            cond = CC.reference("cfg2_n64", axis, "stress")[3]
            host = p.conditional_quantiles(axis, cond, LEVELS, ptf)
            with torch.cuda.stream(stream):
                d_cond = torch.from_numpy(np.array(cond)).to(dev)
                out = torch.empty((3, P.T, L), dtype=torch.float64, device=dev)
                pe = torch.empty(P.T, dtype=torch.float64, device=dev)
                only = torch.empty((P.T, L), dtype=torch.float64, device=dev)
                p.set_stream(stream.cuda_stream)
                p.conditional_quantiles_device(args, axis, d_cond.data_ptr(), LEVELS, out[0].data_ptr(),
                                               out[1].data_ptr(), out[2].data_ptr(), pe.data_ptr())
                p.conditional_quantiles_device(args, axis, d_cond.data_ptr(), LEVELS, only.data_ptr())   # the rest NULL
            stream.synchronize()
            for k in range(3):
                assert np.array_equal(out[k].cpu().numpy(), host[k], equal_nan=True)
            assert np.array_equal(pe.cpu().numpy(), host[3])
            assert np.array_equal(only.cpu().numpy(), host[0], equal_nan=True)
    finally:
        p.close()


def test_sharded_world1():
    import torch
    from copula_var import engine
    from copula_var.distributed import device_sharded_var
    P, cp, ptf = CC.problem("cfg2_n64")
    cond = CC.reference("cfg2_n64", 0, "stress")[3]
    p = _plan_of(P, cp)
    try:
        dev = torch.device("cuda", 0)
        s = device_sharded_var(p, engine.solve_args(ptf), P.T, dev, levels=LEVELS,
                               conditional=(0, torch.from_numpy(np.array(cond)).to(dev)))
        got = s.conditional_quantiles(len(LEVELS)).cpu().numpy()
        host = p.conditional_quantiles(0, cond, LEVELS, ptf)
        assert got.shape == (P.T, len(LEVELS), 4)
        for k in range(3):
            assert np.array_equal(got[:, :, k], host[k], equal_nan=True)
        assert np.array_equal(got[:, :, 3], np.repeat(host[3][:, None], len(LEVELS), axis=1))
        bare = device_sharded_var(p, engine.solve_args(ptf), P.T, dev, levels=LEVELS)
        with pytest.raises(RuntimeError, match="cond_local"):
            bare.conditional_quantiles(1)
    finally:
        p.close()


# ------------------------------------------------------------------ 10. driver
@pytest.mark.parametrize("case", ["cfg2_n64", "garch_student_n64"])
def test_driver_calc_covar(case):
    from conftest import load_golden
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    z = load_golden(case)
    ptf = float(z["ptf_mean"])
    tickers, start, kw = inject(z)
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=str(z["copula"]),
                                                               estimation_type=str(z["model"]))
    v = ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=int(z["num_points"]),
                               weights=z["weights"], copula_params=z["copula_params"], **kw)
    try:
        covar, coes, delta = v.calc_covar(tickers[0], levels=LEVELS)
        m0, pe = v.last_tail_mass, v.last_event_mass
        by_index = v.calc_covar(0, levels=LEVELS, benchmark=None)
        base = v.plan.conditional_quantiles(0, CC.reference(case, 0, "driver_band")[3], LEVELS, ptf)
        with pytest.raises(ValueError):
            v.calc_covar("no such ticker")
    finally:
        v.close()
    stress, band = CC.reference(case, 0, "driver_stress")[4], CC.reference(case, 0, "driver_band")[4]
    _compare((covar, coes, m0, pe), stress, ptf)
    _compare(base, band, ptf)
    assert np.array_equal(pe, v.last_event_mass) and pe.shape == (covar.shape[0],)
    assert np.array_equal(delta, covar - base[0], equal_nan=True)
    assert np.array_equal(delta, stress[0] - band[0], equal_nan=True) and np.isfinite(delta).any()
    assert by_index[2] is None and np.array_equal(by_index[0], covar, equal_nan=True)
