"""Gumbel / survival-Gumbel copulas without a GPU: the checker's own formula (against the
mixed finite difference of the copula's CDF), the package's pointwise density, the factory rows,
the C ABI's host-side validation and the IFM fit."""
import ctypes as C

import numpy as np
import pytest

import gumbel_reference as G
from conftest import load_golden


# ------------------------------------------------------------------ checker self-test
def _mixed_difference(u, theta, h):
    """Central mixed finite difference d^d C / du_1 .. du_d of the Gumbel CDF at the points u (P, d)."""
    d = u.shape[1]
    tot = np.zeros(u.shape[0])
    for signs in np.ndindex(*([2] * d)):
        s = np.array([1.0 if b else -1.0 for b in signs])
        tot += np.prod(s) * G.cdf(u + s * h, theta)
    return tot / (2 * h) ** d


@pytest.mark.parametrize("d,h,rtol", [(2, 1e-4, 2e-6), (3, 1e-3, 2e-4)])
@pytest.mark.parametrize("theta", [1.0, 1.7, 4.0])
def test_density_is_the_mixed_derivative_of_the_cdf(d, h, rtol, theta):
    # central differences: truncation h^2 x (fourth derivatives / density) ~ 1e-8 .. 1e-6 x O(10)
    # on [0.15, 0.85]^d, rounding eps / (2h)^d ~ 3e-9 (2-D) / 3e-8 (3-D)
    rng = np.random.default_rng(7)
    u = rng.uniform(0.15, 0.85, size=(40, d))
    np.testing.assert_allclose(G.density(u, theta), _mixed_difference(u, theta, h), rtol=rtol)


@pytest.mark.parametrize("d", [2, 3])
def test_independence_and_rotation(d):
    rng = np.random.default_rng(3)
    u = rng.uniform(1e-6, 1 - 1e-6, size=(200, d))
    for surv in (False, True):
        np.testing.assert_allclose(G.density(u, 1.0, surv), 1.0, rtol=1e-13)
    # survival Gumbel is c(1 - u); 1 - u is exact for these u >= 2^-20 only to an ulp of 1, hence 1e-9
    np.testing.assert_allclose(G.density(u, 2.5, True), G.density(1.0 - u, 2.5, False), rtol=1e-9)
    assert np.isnan(G.density(np.array([[0.0] + [0.5] * (d - 1), [1.0] + [0.5] * (d - 1)]), 2.0)).all()


@pytest.mark.parametrize("kind,theta", [("gumbel_survival", 1.3), ("gumbel", 16.0), ("gumbel_survival", 16.0)])
def test_mass_is_finite_and_zero_on_dead_entries(kind, theta):
    z = load_golden("cfg5_n64")
    P = G.problem_of(z, kind, theta)
    ndead = 0
    for t in range(P.T):
        m = P.mass(t)
        assert np.isfinite(m).all() and (m >= 0).all()
        dead = P.dead_entries(t)
        ndead += int(dead.sum())
        assert (m[dead[0], :] == 0).all() and (m[:, dead[1]] == 0).all()
    assert ndead == 261                       # the case's grid-edge entries with u in {0, 1}
    assert float(np.sum(P.mass(0))) > 0.5     # and the rest of the measure is there


def test_checker_runs_the_inherited_solve_and_risk_checkers():
    import es_reference as E
    import quantile_reference as Q
    from oracle.quadrature import calc_var
    z = load_golden("cfg4_k4_n16")
    P = G.problem_of(z, "gumbel_survival", 1.8)
    var, it, _ = calc_var(P.compute_integral, P.T, float(z["ptf_mean"]))
    assert var.shape == (P.T,) and it > 0
    es, m0, _, _ = E.expected_shortfall(P, var, float(z["ptf_mean"]))
    assert np.isfinite(es[~np.isnan(var)]).all()
    qv, qe, qm, margin = Q.quantiles(P, (0.01, 0.05), float(z["ptf_mean"]))
    assert qv.shape == (P.T, 2)


# ------------------------------------------------------------------ package density
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("survival", [False, True])
def test_package_density_equals_the_checker(d, survival):
    from copula_var import copulas
    rng = np.random.default_rng(11)
    u = rng.uniform(1e-9, 1 - 1e-9, size=(300, d))
    for theta in (1.0, 1.6, 7.0, 16.0):
        np.testing.assert_allclose(copulas.gumbel(u, theta, survival=survival), G.density(u, theta, survival),
                                   rtol=1e-13)
    assert np.isnan(copulas.gumbel(np.array([[0.0] + [0.5] * (d - 1)]), 2.0, survival=survival)).all()


# ------------------------------------------------------------------ factory rows
def test_factory_rows():
    from copula_var.utils.calc_var_class import check_device_adapter
    from copula_var.utils.factory import ValueAtRiskCalculationFactory as F
    from copula_var.utils.model_estimation.copula.gumbel_estimation import GumbelCopulaVaR, GumbelSurvivalCopulaVaR
    for est in ("msm", "garch", "mean_reverting"):
        for name, cls in (("gumbel", GumbelCopulaVaR), ("gumbel_survival", GumbelSurvivalCopulaVaR)):
            a = F.create_var_calculator(copula_type=name, estimation_type=est)
            assert type(a) is cls and a.copula_kind == name
            check_device_adapter(a)
            assert a.copula_integrations_params({"theta": 2.5}) == 2.5
            u = np.array([[0.3, 0.6]])
            np.testing.assert_allclose(a.copula_density(u, 2.0), G.density(u, 2.0, name == "gumbel_survival"),
                                       rtol=1e-13)
    for est in ("msm", "garch", "mean_reverting"):                 # the existing rejections still hold
        with pytest.raises(ValueError, match="Unsupported estimation type"):
            F.create_var_calculator(copula_type="clayton", estimation_type=est)


def test_engine_names():
    from copula_var import _native as N
    from copula_var.engine import auto_strategy
    assert N.COPULA_KIND["gumbel"] == 3 and N.COPULA_KIND["gumbel_survival"] == 4
    for kind in G.KINDS:
        for model in ("msm", "garch", "ukf"):
            assert auto_strategy(model, 2, 64, kind, [2.0]) == "sorted"
            assert auto_strategy(model, 3, 128, kind, [2.0]) == "sorted"
        with pytest.raises(ValueError, match="255"):
            auto_strategy("msm", 3, 256, kind, [2.0])
    assert auto_strategy("msm", 2, 64, "student", [6.0, 0.5]) == "compact"      # unchanged


def test_synthetic_config_packs_theta():
    from copula_var import synthetic
    c = synthetic.baseline_configs()[3].with_(copula="gumbel_survival", theta=2.5)
    assert c.copula_params() == 2.5


# ------------------------------------------------------------------ ABI validation, no device
def _static(N, copula, params, strategy, dim=2):
    n = 4
    keep = dict(x=N.f64(np.linspace(-5, 5, n)), step=N.f64(np.full(n, 10.0 / (n - 1))), dens=N.f64(np.ones((dim, 1, n))),
                combos=np.zeros((1, dim), dtype=np.int32), w=N.f64(np.full(dim, 1.0 / dim)), cp=N.f64(params))
    st = N.CvqStatic()
    st.model, st.copula, st.dim, st.n, st.q, st.n_combos = N.GARCH, copula, dim, n, 1, 1
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    st.x_values, st.step, st.densities, st.weights = dp(keep["x"]), dp(keep["step"]), dp(keep["dens"]), dp(keep["w"])
    st.combos = keep["combos"].ctypes.data_as(C.POINTER(C.c_int32))
    st.vol_states = None
    st.copula_params, st.n_copula_params = dp(keep["cp"]), keep["cp"].size
    st.strategy, st.v_cap = strategy, 0.0
    return st, keep


@pytest.mark.parametrize("copula", [3, 4])
def test_abi_validation_without_gpu(copula):
    from copula_var import _native as N
    lib = N.lib()
    assert lib.cvq_version() >= 10300

    def create(params, strategy=N.STRATEGY_SORTED, dim=2):
        st, keep = _static(N, copula, params, strategy, dim)
        h = C.c_void_p()
        rc = lib.cvq_plan_create(C.byref(st), 0, C.byref(h))
        assert not h.value
        return rc, (lib.cvq_last_error() or b"").decode()

    for dim in (2, 3):
        for theta in (float("nan"), 0.5):
            rc, msg = create([theta], dim=dim)
            assert rc == N.CVQ_ERR_INVALID, (theta, rc, msg)
        rc, msg = create([17.0], dim=dim)
        assert rc == N.CVQ_ERR_UNSUPPORTED and "16" in msg
        rc, msg = create([2.0, 0.5], dim=dim)
        assert rc == N.CVQ_ERR_INVALID and "parameter" in msg
    for strategy in (N.STRATEGY_PREFIX, N.STRATEGY_DIRECT, N.STRATEGY_COMPACT, N.STRATEGY_SWEEP):
        rc, msg = create([2.0], strategy)
        assert rc == N.CVQ_ERR_UNSUPPORTED and "SORTED" in msg, (strategy, rc, msg)


# ------------------------------------------------------------------ fit
def _sample_gumbel(rng, n, theta, d=2):
    """Marshall-Olkin: V positive stable(1 / theta), U_i = exp(-(E_i / V)^(1 / theta))."""
    a = 1.0 / theta
    if theta == 1.0:
        return rng.uniform(size=(n, d))
    th = rng.uniform(0, np.pi, n)
    w = rng.exponential(size=n)
    V = (np.sin(a * th) / np.sin(th) ** (1 / a)) * (np.sin((1 - a) * th) / w) ** ((1 - a) / a)
    E = rng.exponential(size=(n, d))
    return np.exp(-(E / V[:, None]) ** a)


@pytest.fixture(scope="module")
def sample2():
    rng = np.random.default_rng(2024)
    u = np.clip(_sample_gumbel(rng, 1500, 2.2), 1e-12, 1 - 1e-12)
    dens = rng.uniform(0.5, 1.5, size=u.shape)
    return u, dens


def test_fit_minimises_the_nll_on_a_grid(sample2):
    from copula_var.optim.copula_fit import GumbelCopulaOptimizer
    u, dens = sample2
    opt = GumbelCopulaOptimizer(u, dens)
    res = opt.optimize()
    assert set(res) == {"theta", "nll", "optimized_params"}
    assert 1.0001 <= res["theta"] <= 16.0 and abs(res["theta"] - 2.2) < 0.3
    lo, hi = GumbelCopulaOptimizer.BOUNDS
    for th in np.linspace(lo, hi, 200):
        assert res["nll"] <= opt.negative_log_likelihood([th]) + 1e-9, th
    # the NLL is the IFM one: - sum log densities - sum log c
    want = -(np.sum(np.log(dens)) + np.sum(G.log_density(u, res["theta"])))
    assert abs(res["nll"] - want) <= 1e-9 * abs(want)


def test_survival_fit_of_the_rotated_sample_is_the_plain_fit(sample2):
    from copula_var.optim.copula_fit import GumbelCopulaOptimizer
    u, dens = sample2
    plain = GumbelCopulaOptimizer(u, dens).optimize()
    rot = GumbelCopulaOptimizer(1.0 - u, dens, survival=True).optimize()
    # log1p(-(1 - u)) against log u: 1 - (1 - u) differs from u by at most an ulp of 1
    assert abs(rot["theta"] - plain["theta"]) < 1e-6
    assert abs(rot["nll"] - plain["nll"]) < 1e-6 * abs(plain["nll"])


def test_fit_at_independence_sits_at_the_lower_bound():
    from copula_var.optim.copula_fit import GumbelCopulaOptimizer
    rng = np.random.default_rng(5)
    u = rng.uniform(1e-6, 1 - 1e-6, size=(4000, 2))
    res = GumbelCopulaOptimizer(u, np.ones_like(u)).optimize()
    assert res["theta"] < 1.05


def test_fit_three_assets():
    from copula_var.optim.copula_fit import GumbelCopulaOptimizer
    rng = np.random.default_rng(9)
    u = np.clip(_sample_gumbel(rng, 1200, 1.8, d=3), 1e-12, 1 - 1e-12)
    res = GumbelCopulaOptimizer(u, np.ones_like(u)).optimize()
    assert abs(res["theta"] - 1.8) < 0.3
    with pytest.raises(ValueError):
        GumbelCopulaOptimizer(np.full((10, 4), 0.5), np.ones((10, 4)))


def _saturated_sample():
    """In-sample GARCH marginals that hold a value of exactly 0: cfg1's first 1135 returns under the
    GARCH(3, 1) parameters the order search gives them (a poor fit; one residual lies below the erf
    form's double range)."""
    from copula_var import insample
    r = load_golden("cfg1")["returns"][:1135]
    params = [[0.08095905, 0.12499614, 0.125, 0.12499534, 0.08595985],
              [0.07765225, 0.12499498, 0.12499999, 0.124997, 0.08265021]]
    md = [insample.garch_marginals_densities(r[:, d], (3, 1), np.array(params[d])) for d in range(2)]
    return np.column_stack([m for m, _ in md]), np.column_stack([d for _, d in md])


@pytest.mark.parametrize("survival", [False, True])
def test_fit_with_a_marginal_at_the_boundary(survival):
    """A marginal of exactly 0 or 1 is clamped one rounding step of 1 inside (2^-53), at both ends."""
    from copula_var.optim.copula_fit import GumbelCopulaOptimizer
    u, dens = _saturated_sample()
    assert (u == 0.0).sum() == 1 and np.isnan(G.log_density(u, 2.0, survival)).sum() == 1
    opt = GumbelCopulaOptimizer(u, dens, survival=survival)
    res = opt.optimize()
    lo, hi = GumbelCopulaOptimizer.BOUNDS
    assert lo <= res["theta"] <= hi and np.isfinite(res["nll"]) and res["nll"] < 1e10
    for th in np.linspace(lo, hi, 200):
        assert res["nll"] <= opt.negative_log_likelihood([th]) + 1e-9, th
    edge = 2.0 ** -53
    want = -(np.sum(np.log(dens)) + np.sum(G.log_density(np.clip(u, edge, 1 - edge), res["theta"], survival)))
    assert abs(res["nll"] - want) <= 1e-9 * abs(want)
    # the rotated sample (its 0 now a 1) under the other kind: the same likelihood, so the same fit
    rot = GumbelCopulaOptimizer(1.0 - u, dens, survival=not survival).optimize()
    assert abs(rot["theta"] - res["theta"]) < 1e-6 and abs(rot["nll"] - res["nll"]) < 1e-6 * abs(res["nll"])


def test_fit_rejects_nan_marginals_and_zero_densities():
    from copula_var.optim.copula_fit import GumbelCopulaOptimizer
    rng = np.random.default_rng(1)
    u = rng.uniform(0.05, 0.95, size=(50, 2))
    bad = u.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        GumbelCopulaOptimizer(bad, np.ones_like(u)).optimize()
    dens = np.ones_like(u)
    dens[7, 0] = 0.0
    with pytest.raises(ValueError, match="not finite"):
        GumbelCopulaOptimizer(u, dens).optimize()


# ------------------------------------------------------------------ the device tables' floor
def _device_formula_mass(P, t, floor=1.0e-300):
    """numpy restatement of the device's generic path (cvq_quad_kernels.h table_entry / node_value,
    2-D MSM): per-axis A = max(x^theta, floor), B = log(x^(theta-1) / u'), node =
    exp(B0 + B1 - A + (1 - 2 theta) log A) (A + theta - 1) W with A = (A0 + A1)^(1/theta)."""
    th = P.theta
    u, _ = P.axis_cdf(t)
    with np.errstate(all="ignore"):
        l = np.log1p(-u) if P.survival else np.log(u)
        lx = np.log(-l)
        live = (u > 0.0) & (u < 1.0)
        A = np.where(live, np.maximum(np.exp(th * lx), floor), np.nan)
        B = np.where(live, (th - 1.0) * lx - l, 0.0)
        S = A[0][:, None] + A[1][None, :]
        lA = np.log(S) / th
        Av = np.exp(lA)
        v = np.exp((B[0][:, None] + B[1][None, :]) - Av + (1.0 - 2 * th) * lA) * (Av + th - 1.0) * P.delta_weights(t)
    return np.where(np.isfinite(v), v, 0.0), A


def test_table_floor_changes_only_negligible_corner_nodes():
    """Survival Gumbel, theta = 16, MSM with every u_i < 1e-19 at the lower grid edge: x_i^16 < 1e-300
    is floored in the device tables.  There S, hence A, is too large, and since -A and
    (1 - d theta) log A both decrease in A the floored node lies in [0, true node]: the slab error
    is at most the true mass of those nodes, which a consistent model keeps far below the slab
    bar's atol (c ~ 1 / u against W ~ u^2).  Everywhere else the floor is inactive."""
    P = G.corner_problem("gumbel_survival")
    for t in range(P.T):
        ref = P.mass(t)
        dev, A = _device_formula_mass(P, t)
        with np.errstate(all="ignore"):
            exact = np.exp(P.theta * np.log(-np.log1p(-P.axis_cdf(t)[0])))
        fl = exact < 1.0e-300                                   # floored table entries, per axis
        corner = fl[0][:, None] & fl[1][None, :]                # nodes whose every entry is floored
        touched = fl[0][:, None] | fl[1][None, :]               # nodes with a floored entry
        assert fl[0].sum() >= 2 and fl[1].sum() >= 2 and corner.sum() >= 4
        assert np.all(dev[touched] >= 0.0) and np.all(dev[touched] <= ref[touched] * (1 + 1e-9))
        assert ref[corner].max() > 0.0 and dev[corner].max() < 0.5 * ref[corner].max()   # the floor does bite
        print("true mass of the nodes with a floored entry", float(np.sum(ref[touched])))
        assert float(np.sum(ref[touched])) <= 1e-15             # ... on mass under the slab bar's atol
        assert float(np.sum(np.abs(dev - ref)[touched])) <= 1e-15
        # no floored entry: the same value (library rounding only)
        np.testing.assert_allclose(dev[~touched], ref[~touched], rtol=1e-9, atol=0.0)
