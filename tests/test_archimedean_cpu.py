"""Frank / Joe / survival-Joe copulas without a GPU: the checker against mpmath (the stable form
and the mixed partial of the CDFs), its symmetries, a float64 restatement of the device's table
and node formulas against it, the package's densities, the factory rows, the C ABI's host-side
validation, rolling_copula_params and the IFM fits."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import archimedean_reference as A
from conftest import load_golden

LD = np.longdouble
EXTREME = (1e-300, 2.0 ** -54, 0.5, 1.0 - 2.0 ** -53)


def _mp_log1mexp(x):
    return mp.log1p(-mp.exp(-x)) if x > mp.log(2) else mp.log(-mp.expm1(-x))


def _mp_log_density(u, kind, theta):
    """The closed form in mpmath (60 digits), its differences 1 - e^-x and 1 - v^theta taken by
    expm1 / log1p so that 60 digits suffice at the extreme points (v^16 = 1e-4800 at v = 1e-300)."""
    mp.mp.dps = 60
    th = mp.mpf(theta)
    u = [mp.mpf(float(x)) for x in u]
    d = len(u)
    if kind == "frank":
        g = -mp.expm1(-th)
        a = [-mp.log(-mp.expm1(-th * x) / g) for x in u]
        sumB = sum(mp.log(th) - th * x + ai - mp.log(g) for x, ai in zip(u, a))
        p0, q0, kap = g, mp.e ** (-th), mp.mpf(0)
        c2, c3 = (1, 0) if d == 2 else (3, 2)
    else:
        lv = [mp.log1p(-x) if kind == "joe" else mp.log(x) for x in u]       # log v, v = 1 - u (survival: u)
        a = [-_mp_log1mexp(-th * l) for l in lv]                               # -log(1 - v^theta)
        sumB = sum(mp.log(th) + (th - 1) * l + ai for l, ai in zip(lv, a))
        k = 1 - 1 / th
        p0, q0, kap = mp.mpf(1), mp.mpf(0), 1 / th
        c2, c3 = (k, 0) if d == 2 else (3 * k, k * (1 + k))
    S = sum(a)
    om = q0 - p0 * mp.expm1(-S)
    y = p0 * mp.e ** (-S) / om
    return sumB + mp.log(p0) - mp.log(th) - S + (kap - 1) * mp.log(om) + mp.log(1 + y * (c2 + c3 * y))


def _mp_cdf(u, kind, theta):
    th = mp.mpf(theta)
    d = len(u)
    if kind == "frank":
        g = 1 - mp.e ** (-th)
        prod = mp.mpf(1)
        for x in u:
            prod *= 1 - mp.e ** (-th * x)
        return -mp.log(1 - prod / g ** (d - 1)) / th
    prod = mp.mpf(1)
    for x in u:
        prod *= 1 - (1 - x) ** th
    return 1 - (1 - prod) ** (1 / th)


def _points(d, seed):
    rng = np.random.default_rng(seed)
    pts = [rng.uniform(1e-6, 1 - 1e-6, size=d) for _ in range(12)]
    pts += [10.0 ** rng.uniform(-12, -1, size=d) for _ in range(4)]
    pts += [1.0 - 10.0 ** rng.uniform(-12, -1, size=d) for _ in range(4)]
    for e in EXTREME:
        pts.append(np.full(d, e))
        pts.append(np.array([e] + [0.3] * (d - 1)))
        pts.append(np.array([0.7] * (d - 1) + [e]))
    pts.append(np.array([1e-300, 1.0 - 2.0 ** -53, 2.0 ** -54][:d]))
    return np.array(pts)


CASES = [("frank", 0.25), ("frank", 6.0), ("frank", 32.0), ("joe", 1.0), ("joe", 2.5), ("joe", 16.0),
         ("joe_survival", 1.3), ("joe_survival", 16.0)]


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("kind,theta", CASES)
def test_checker_equals_mpmath(kind, theta, d):
    """The longdouble stable form against the same closed form in 60-digit mpmath, random and
    extreme points: 1e-15 max(1, |log c|) (the longdouble's 64-bit mantissa leaves ~1e-19 relative
    per operation; the bar is the issue's)."""
    u = _points(d, 5)
    got = A.log_density(u, kind, theta)
    worst = 0.0
    for i in range(u.shape[0]):
        want = _mp_log_density(u[i], kind, theta)
        assert mp.isfinite(want)
        if not np.isfinite(got[i]):
            # y^2 beyond longdouble's range (y = 1 / S ~ 1e4799 where three margins sit at 1e-300 under
            # survival Joe, theta = 16): log c > 709 there, a node that is not finite in double either
            # way, which the dead rule makes 0
            assert d == 3 and want > 709, (u[i], want, got[i])
            continue
        err = abs(mp.mpf(float(got[i])) + mp.mpf(float(got[i] - LD(float(got[i])))) - want)
        worst = max(worst, float(err / max(1, abs(want))))
    print("max |dlog c| / max(1, |log c|)", kind, theta, d, worst)
    assert worst <= 1e-15


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("kind,theta", [("frank", 0.25), ("frank", 6.0), ("frank", 32.0), ("joe", 1.7),
                                        ("joe", 16.0)])
def test_closed_form_is_the_mixed_partial_of_the_cdf(kind, theta, d):
    """mpmath's numerical mixed partial of the CDF (60 digits) against the closed form: the central
    differences' truncation at mpmath's step leaves ~1e-12 relative here."""
    mp.mp.dps = 60
    rng = np.random.default_rng(8)
    for u in rng.uniform(0.15, 0.85, size=(4, d)):
        f = lambda *x: _mp_cdf(x, kind, theta)
        num = mp.diff(f, tuple(mp.mpf(float(x)) for x in u), (1,) * d)
        want = mp.e ** _mp_log_density(u, kind, theta)
        assert abs(num - want) <= mp.mpf(10) ** -9 * abs(want), (u, num, want)


@pytest.mark.parametrize("d", [2, 3])
def test_symmetries(d):
    rng = np.random.default_rng(3)
    # dyadic u: 1 - u is exact, so the rotation identities hold to rounding
    u = rng.integers(1, 2 ** 20, size=(200, d)) / 2.0 ** 20
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    # the bivariate Frank copula is radially symmetric; no Archimedean copula is for d >= 3
    for th in (0.25, 6.0, 32.0) if d == 2 else ():
        np.testing.assert_allclose(f64(A.log_density(u, "frank", th)), f64(A.log_density(1.0 - u, "frank", th)),
                                   rtol=0, atol=1e-13)
    for th in (1.3, 4.0, 16.0):                                                # survival Joe is c(1 - u)
        np.testing.assert_array_equal(A.log_density(u, "joe_survival", th), A.log_density(1.0 - u, "joe", th))
    for kind in ("joe", "joe_survival"):                                       # theta = 1: independence
        np.testing.assert_allclose(f64(A.log_density(u, kind, 1.0)), 0.0, rtol=0, atol=1e-15)
    for kind, th in (("frank", 5.0), ("joe", 2.0), ("joe_survival", 7.0)):     # exchangeable
        np.testing.assert_allclose(f64(A.log_density(u, kind, th)), f64(A.log_density(u[:, ::-1], kind, th)),
                                   rtol=0, atol=1e-15)
    dead = np.array([[0.0] + [0.5] * (d - 1), [1.0] + [0.5] * (d - 1), [np.nan] + [0.5] * (d - 1)])
    for kind in A.KINDS:
        assert np.isnan(A.log_density(dead, kind, 2.0)).all()


# ------------------------------------------------------------------ the device formulas, float64
FLOOR = 1.0e-300


def _log1mexp64(x):
    with np.errstate(all="ignore"):
        return np.where(x > 0.6931471805599453, np.log1p(-np.exp(-x)), np.log(-np.expm1(-x)))


def _device_tables(P, t):
    """table_entry of the product-form kind (cvq_quad_kernels.h prod_entry), float64: A = max(a, floor),
    B the log factor; dead entries (NaN, 0)."""
    th, kind = P.theta, P.copula
    u, pdf = P.axis_cdf(t)
    with np.errstate(all="ignore"):
        if kind == "frank":
            g, lg = -np.expm1(-th), _log1mexp64(np.float64(th))
            X = np.exp(-th) * np.expm1(th * (1.0 - u)) / g
            a = np.where(X <= 0.5, -np.log1p(-X), lg - _log1mexp64(th * u))
            B = ((np.log(th) - th * u) + a) - lg
        else:
            l = np.log(u) if kind == "joe_survival" else np.log1p(-u)
            a = -_log1mexp64(-th * l)
            B = (np.log(th) + (th - 1.0) * l) + a
        if pdf is not None:
            B = B + np.log(pdf)
    live = (u > 0.0) & (u < 1.0)
    return np.where(live, np.maximum(a, FLOOR), np.nan), np.where(live, B, 0.0), a


def _device_formula_mass(P, t):
    """node_value of the product-form kind: S = sum A, om = q0 - p0 expm1(-S), p = p0 e^-S,
    exp(sum B + lc - S + (kappa - d) log om) poly_d(om, p) W; non-finite -> 0."""
    th, kind, d = P.theta, P.copula, P.dim
    Atab, Btab, a_exact = _device_tables(P, t)
    if kind == "frank":
        p0, q0, kap = -np.expm1(-th), np.exp(-th), 0.0
        c2, c3 = (1.0, 0.0) if d == 2 else (3.0, 2.0)
        lc = float(_log1mexp64(np.float64(th))) - np.log(th)
    else:
        kap = 1.0 / th
        k = 1.0 - kap
        p0, q0 = 1.0, 0.0
        c2, c3 = (k, 0.0) if d == 2 else (3.0 * k, k * (1.0 + k))
        lc = -np.log(th)
    S, sumB = 0.0, 0.0
    for c in range(d):
        S = S + P._broadcast(Atab)[c]
        sumB = sumB + P._broadcast(Btab)[c]
    with np.errstate(all="ignore"):
        om = q0 - p0 * np.expm1(-S)
        p = p0 * np.exp(-S)
        poly = om + c2 * p if d == 2 else om * om + p * (c2 * om + c3 * p)
        v = np.exp((sumB + lc) - S + (kap - d) * np.log(om)) * poly * P.delta_weights(t)
    return np.where(np.isfinite(v), v, 0.0), a_exact


SLABS = ((-100.0, -3.0), (-3.0, -2.0), (-3.5, -3.0), (-100.0, 0.0), (-3.0, 0.5))


@pytest.mark.parametrize("case,kind,theta", A.TABLE1)
def test_device_formulas_reproduce_the_checker_on_table_1(case, kind, theta):
    """The float64 restatement of the device's table and node formulas against the longdouble
    checker, slab by slab: 1e-13 relative beyond an atol of 1e-15 (float64 library rounding in
    logs of magnitude up to ~1e3 leaves ~1e-13 per node, far less in a sum)."""
    z = load_golden(case)
    P = A.problem_of(z, kind, theta, slice(0, 12))
    worst = 0.0
    for t in range(P.T):
        dev, _ = _device_formula_mass(P, t)
        ref = P.mass(t)
        assert np.isfinite(ref).all() and (ref >= 0).all()
        for a, b in SLABS:
            m = P.inner_mask(a, b)
            got, want = float(np.sum(dev[m])), float(np.sum(ref[m]))
            worst = max(worst, max(abs(got - want) - 1e-15, 0.0) / max(abs(want), 1e-300))
    print("max slab relative difference", case, kind, theta, worst)
    assert worst <= 1e-13


@pytest.mark.parametrize("kind,theta", [("joe_survival", 16.0), ("joe", 16.0), ("frank", 32.0)])
def test_table_floor_changes_only_negligible_corner_nodes(kind, theta):
    """corner_problem: every u_i < 1e-19 at the lower grid edge.  Survival Joe at theta = 16 has
    a ~ u^16 < 1e-300 there, floored in the device tables; a floored entry makes S too large and
    the node decreases in S, so it lies in [0, true node].  Slabs stay inside the slab bar
    (rtol 1e-10, atol 1e-15) for every kind."""
    P = A.corner_problem(kind, theta)
    nfloored = 0
    for t in range(P.T):
        ref = P.mass(t)
        dev, a_exact = _device_formula_mass(P, t)
        with np.errstate(invalid="ignore"):
            fl = (a_exact < FLOOR) & ~P.dead_entries(t)
        nfloored += int(fl.sum())
        touched = fl[0][:, None] | fl[1][None, :]
        assert np.all(dev[touched] >= 0.0) and np.all(dev[touched] <= ref[touched] * (1 + 1e-9))
        np.testing.assert_allclose(dev[~touched], ref[~touched], rtol=1e-12, atol=0.0)
        for a, b in SLABS:
            m = P.inner_mask(a, b)
            np.testing.assert_allclose(float(np.sum(dev[m])), float(np.sum(ref[m])), rtol=1e-10, atol=1e-15)
    print("floored table entries", kind, nfloored)
    if kind == "joe_survival":
        assert nfloored >= 4                                                   # the floor does bite there


def test_checker_runs_the_inherited_solve_and_risk_checkers():
    import es_reference as E
    import quantile_reference as Q
    from oracle.quadrature import calc_var
    z = load_golden("cfg4_k4_n16")
    P = A.problem_of(z, "joe_survival", 1.8)
    var, it, _ = calc_var(P.compute_integral, P.T, float(z["ptf_mean"]))
    assert var.shape == (P.T,) and it > 0
    for f in (1 - 1e-7, 1 + 1e-7):                                             # the exact-VaR premise
        v2, it2, _ = calc_var(A.scaled(P.compute_integral, f), P.T, float(z["ptf_mean"]))
        np.testing.assert_array_equal(v2, var)
        assert it2 == it
    es, m0, _, _ = E.expected_shortfall(P, var, float(z["ptf_mean"]))
    assert np.isfinite(es[~np.isnan(var)]).all()
    qv, qe, qm, margin = Q.quantiles(P, (0.01, 0.05), float(z["ptf_mean"]))
    assert qv.shape == (P.T, 2) and np.nanmin(margin) >= 1e-7


# ------------------------------------------------------------------ package densities
@pytest.mark.parametrize("d", [2, 3])
def test_package_density_equals_the_checker(d):
    from copula_var import copulas
    rng = np.random.default_rng(11)
    u = rng.uniform(1e-9, 1 - 1e-9, size=(300, d))
    # the extreme points: float64 sums of terms up to ~3 x 750 in magnitude (a_i and B_i cancel
    # against S), each rounded to 1.1e-16 relative: 1e-12 absolute on log c
    ux = _points(d, 2)
    ux = ux[np.min(ux, axis=1) >= 2.0 ** -54]     # (float64 cannot hold a = u^16 at u = 1e-300; no floor on the host)
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    for th in (0.25, 4.0, 32.0):
        np.testing.assert_allclose(copulas.frank(u, th), np.exp(f64(A.log_density(u, "frank", th))), rtol=1e-13)
        np.testing.assert_allclose(copulas.frank_log_density(ux, th), f64(A.log_density(ux, "frank", th)),
                                   rtol=0, atol=1e-12)
    for th in (1.0, 1.6, 7.0, 16.0):
        for surv in (False, True):
            kind = "joe_survival" if surv else "joe"
            np.testing.assert_allclose(copulas.joe(u, th, survival=surv), np.exp(f64(A.log_density(u, kind, th))),
                                       rtol=1e-13)
            np.testing.assert_allclose(copulas.joe_log_density(ux, th, survival=surv), f64(A.log_density(ux, kind, th)),
                                       rtol=0, atol=1e-12)
    dead = np.array([[0.0] + [0.5] * (d - 1)])
    assert np.isnan(copulas.frank(dead, 2.0)).all() and np.isnan(copulas.joe(dead, 2.0, survival=True)).all()
    with pytest.raises(ValueError):
        copulas.frank(np.full((3, 4), 0.5), 2.0)
    with pytest.raises(ValueError):
        copulas.joe(np.full((3, 4), 0.5), 2.0)


# ------------------------------------------------------------------ factory rows, names
def test_factory_rows():
    from copula_var.utils.calc_var_class import DEVICE_COPULAS, check_device_adapter
    from copula_var.utils.factory import ValueAtRiskCalculationFactory as F
    from copula_var.utils.model_estimation.copula.archimedean_estimation import (FrankCopulaVaR, JoeCopulaVaR,
                                                                                JoeSurvivalCopulaVaR)
    u = np.array([[0.3, 0.6]])
    for est in ("msm", "garch", "mean_reverting"):
        for name, cls in (("frank", FrankCopulaVaR), ("joe", JoeCopulaVaR), ("joe_survival", JoeSurvivalCopulaVaR)):
            a = F.create_var_calculator(copula_type=name, estimation_type=est)
            assert type(a) is cls and a.copula_kind == name and name in DEVICE_COPULAS
            check_device_adapter(a)
            assert a.copula_integrations_params({"theta": 2.5}) == 2.5
            want = np.exp(np.asarray(A.log_density(u, name, 2.0), dtype=np.float64))
            np.testing.assert_allclose(a.copula_density(u, 2.0), want, rtol=1e-13)
    for est in ("msm", "garch", "mean_reverting"):                 # Clayton stays rejected
        with pytest.raises(ValueError, match="Unsupported estimation type"):
            F.create_var_calculator(copula_type="clayton", estimation_type=est)

    class Clayton:
        model_kind, copula_kind = "garch", "clayton"
    with pytest.raises(ValueError, match="clayton"):
        check_device_adapter(Clayton())


def test_engine_names():
    from copula_var import _native as N
    from copula_var.engine import SORTED_ONLY, auto_strategy
    assert (N.COPULA_KIND["frank"], N.COPULA_KIND["joe"], N.COPULA_KIND["joe_survival"]) == (5, 6, 7)
    assert "clayton" not in N.COPULA_KIND
    for kind in A.KINDS:
        assert kind in SORTED_ONLY
        for model in ("msm", "garch", "ukf"):
            assert auto_strategy(model, 2, 64, kind, [2.0]) == "sorted"
            assert auto_strategy(model, 2, 1024, kind, [2.0]) == "sorted"
            assert auto_strategy(model, 3, 128, kind, [2.0]) == "sorted"
        with pytest.raises(ValueError, match="255"):
            auto_strategy("msm", 3, 256, kind, [2.0])
    assert auto_strategy("msm", 2, 64, "student", [6.0, 0.5]) == "compact"      # unchanged


def test_synthetic_config_packs_theta():
    from copula_var import synthetic
    for kind in A.KINDS:
        c = synthetic.baseline_configs()[3].with_(copula=kind, theta=2.5)
        assert c.copula_params() == 2.5


def test_cli_accepts_the_new_kinds():
    import inspect

    from copula_var import main
    src = inspect.getsource(main)
    for kind in A.KINDS:
        assert f'"{kind}"' in src


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


def _create(copula, params, strategy=None, dim=2):
    from copula_var import _native as N
    lib = N.lib()
    st, keep = _static(N, copula, params, N.STRATEGY_SORTED if strategy is None else strategy, dim)
    h = C.c_void_p()
    rc = lib.cvq_plan_create(C.byref(st), 0, C.byref(h))
    assert not h.value
    return rc, (lib.cvq_last_error() or b"").decode()


def test_abi_version_and_unknown_kinds():
    from copula_var import _native as N
    assert N.lib().cvq_version() == 10900
    for kind in (8, 9, -1):
        rc, msg = _create(kind, [2.0])
        assert rc == N.CVQ_ERR_INVALID and "unknown copula kind" in msg


@pytest.mark.parametrize("dim", [2, 3])
def test_abi_validation_frank(dim):
    from copula_var import _native as N
    for theta in (float("nan"), 0.0):
        rc, msg = _create(5, [theta], dim=dim)
        assert rc == N.CVQ_ERR_INVALID, (theta, rc, msg)
    rc, msg = _create(5, [-2.0], dim=dim)
    assert rc == N.CVQ_ERR_UNSUPPORTED, (rc, msg)
    rc, msg = _create(5, [32.5], dim=dim)
    assert rc == N.CVQ_ERR_UNSUPPORTED and "32" in msg
    rc, msg = _create(5, [2.0, 0.5], dim=dim)
    assert rc == N.CVQ_ERR_INVALID and "parameter" in msg
    for strategy in (N.STRATEGY_PREFIX, N.STRATEGY_DIRECT, N.STRATEGY_COMPACT, N.STRATEGY_SWEEP):
        rc, msg = _create(5, [2.0], strategy, dim=2)
        assert rc == N.CVQ_ERR_UNSUPPORTED and "SORTED" in msg, (strategy, rc, msg)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("copula", [6, 7])
def test_abi_validation_joe(copula, dim):
    from copula_var import _native as N
    for theta in (float("nan"), 0.5):
        rc, msg = _create(copula, [theta], dim=dim)
        assert rc == N.CVQ_ERR_INVALID, (theta, rc, msg)
    rc, msg = _create(copula, [17.0], dim=dim)
    assert rc == N.CVQ_ERR_UNSUPPORTED and "16" in msg
    rc, msg = _create(copula, [2.0, 0.5], dim=dim)
    assert rc == N.CVQ_ERR_INVALID and "parameter" in msg
    for strategy in (N.STRATEGY_PREFIX, N.STRATEGY_DIRECT, N.STRATEGY_COMPACT, N.STRATEGY_SWEEP):
        rc, msg = _create(copula, [2.0], strategy, dim=2)
        assert rc == N.CVQ_ERR_UNSUPPORTED and "SORTED" in msg, (strategy, rc, msg)


# ------------------------------------------------------------------ samplers, fits
def _sample_frank(rng, n, theta, d=2):
    """Marshall-Olkin: V ~ logarithmic(1 - e^-theta), U_i = -log(1 - (1 - e^-theta) e^(-E_i / V)) / theta."""
    V = rng.logseries(-np.expm1(-theta), size=n).astype(np.float64)
    E = rng.exponential(size=(n, d))
    return -np.log1p(np.expm1(-theta) * np.exp(-E / V[:, None])) / theta


def _sample_joe(rng, n, theta, d=2):
    """Marshall-Olkin: V ~ Sibuya(1 / theta) (P(V > k) = prod_{j <= k} (1 - alpha / j), by inversion),
    U_i = 1 - (1 - e^(-E_i / V))^(1 / theta)."""
    alpha = 1.0 / theta
    w = rng.uniform(size=n)
    V = np.ones(n)
    surv = np.full(n, 1.0 - alpha)                    # P(V > 1)
    k = 1
    todo = w < surv
    while todo.any() and k < 10 ** 6:
        k += 1
        V[todo] = k
        surv = surv * (1.0 - alpha / k)
        todo = todo & (w < surv)
    E = rng.exponential(size=(n, d))
    return 1.0 - (-np.expm1(-E / V[:, None])) ** alpha


def _optimizer(kind, u, dens, rotate=False):
    from copula_var.optim.copula_fit import FrankCopulaOptimizer, JoeCopulaOptimizer
    if kind == "frank":
        return FrankCopulaOptimizer(1.0 - u if rotate else u, dens)
    return JoeCopulaOptimizer(1.0 - u if rotate else u, dens, survival=rotate)


def _standard_error(opt, th):
    h = 1e-3 * max(1.0, th)
    f = lambda x: opt.negative_log_likelihood([x])
    return 1.0 / np.sqrt((f(th + h) - 2 * f(th) + f(th - h)) / (h * h))


@pytest.mark.parametrize("kind,theta,d,seed", [("frank", 6.0, 2, 2024), ("joe", 2.2, 2, 2025), ("frank", 4.0, 3, 9),
                                               ("joe", 1.8, 3, 10)])
def test_fit_recovers_theta(kind, theta, d, seed):
    """theta from a seeded sample within 4 standard errors (numerical second derivative of the NLL
    at the optimum), the optimum below the NLL on a 200-point grid of the bounds, and the NLL the
    IFM one."""
    rng = np.random.default_rng(seed)
    sampler = _sample_frank if kind == "frank" else _sample_joe
    u = np.clip(sampler(rng, 1500, theta, d), 1e-12, 1 - 1e-12)
    dens = rng.uniform(0.5, 1.5, size=u.shape)
    opt = _optimizer(kind, u, dens)
    res = opt.optimize()
    assert set(res) == {"theta", "nll", "optimized_params"}
    lo, hi = type(opt).BOUNDS
    se = _standard_error(opt, res["theta"])
    print("theta", res["theta"], "se", se)
    assert lo <= res["theta"] <= hi and abs(res["theta"] - theta) <= 4 * se
    for th in np.linspace(lo, hi, 200):
        assert res["nll"] <= opt.negative_log_likelihood([th]) + 1e-9, th
    want = -(np.sum(np.log(dens)) + float(np.sum(A.log_density(u, kind, res["theta"]))))
    assert abs(res["nll"] - want) <= 1e-9 * abs(want)


def test_survival_fit_of_the_rotated_sample_is_the_plain_fit():
    rng = np.random.default_rng(2025)
    u = np.clip(_sample_joe(rng, 1500, 2.2), 1e-12, 1 - 1e-12)
    dens = rng.uniform(0.5, 1.5, size=u.shape)
    plain = _optimizer("joe", u, dens).optimize()
    rot = _optimizer("joe", u, dens, rotate=True).optimize()
    assert abs(rot["theta"] - plain["theta"]) < 1e-6
    assert abs(rot["nll"] - plain["nll"]) < 1e-6 * abs(plain["nll"])
    # Frank is its own rotation
    uf = np.clip(_sample_frank(rng, 1500, 6.0), 1e-12, 1 - 1e-12)
    a, b = _optimizer("frank", uf, dens).optimize(), _optimizer("frank", uf, dens, rotate=True).optimize()
    assert abs(a["theta"] - b["theta"]) < 1e-6 and abs(a["nll"] - b["nll"]) < 1e-6 * abs(a["nll"])


def _saturated_sample():
    """tests/test_gumbel_cpu.py's in-sample GARCH marginals that hold a value of exactly 0."""
    from copula_var import insample
    r = load_golden("cfg1")["returns"][:1135]
    params = [[0.08095905, 0.12499614, 0.125, 0.12499534, 0.08595985],
              [0.07765225, 0.12499498, 0.12499999, 0.124997, 0.08265021]]
    md = [insample.garch_marginals_densities(r[:, d], (3, 1), np.array(params[d])) for d in range(2)]
    return np.column_stack([m for m, _ in md]), np.column_stack([d for _, d in md])


@pytest.mark.parametrize("kind,rotate", [("frank", False), ("joe", False), ("joe", True)])
def test_fit_with_a_marginal_at_the_boundary(kind, rotate):
    """A marginal of exactly 0 or 1 is clamped one rounding step of 1 inside (2^-53): the fit stays finite."""
    u, dens = _saturated_sample()
    assert (u == 0.0).sum() == 1
    opt = _optimizer(kind, u, dens, rotate=rotate)
    res = opt.optimize()
    lo, hi = type(opt).BOUNDS
    assert lo <= res["theta"] <= hi and np.isfinite(res["nll"]) and res["nll"] < 1e10
    for th in np.linspace(lo, hi, 200):
        assert res["nll"] <= opt.negative_log_likelihood([th]) + 1e-9, th
    edge = 2.0 ** -53
    name = "frank" if kind == "frank" else ("joe_survival" if rotate else "joe")
    uu = np.clip(1.0 - u if rotate else u, edge, 1 - edge)
    want = -(np.sum(np.log(dens)) + float(np.sum(A.log_density(uu, name, res["theta"]))))
    assert abs(res["nll"] - want) <= 1e-9 * abs(want)


def test_fit_rejects_nan_marginals_and_wrong_dims():
    from copula_var.optim.copula_fit import FrankCopulaOptimizer, JoeCopulaOptimizer
    rng = np.random.default_rng(1)
    u = rng.uniform(0.05, 0.95, size=(50, 2))
    bad = u.copy()
    bad[3, 1] = np.nan
    for cls in (FrankCopulaOptimizer, JoeCopulaOptimizer):
        with pytest.raises(ValueError, match="not finite"):
            cls(bad, np.ones_like(u)).optimize()
        with pytest.raises(ValueError):
            cls(np.full((10, 4), 0.5), np.ones((10, 4)))


@pytest.mark.parametrize("kind", A.KINDS)
def test_rolling_copula_params(kind):
    from copula_var import dynamic
    assert kind in dynamic.COPULAS and "clayton" not in dynamic.COPULAS
    rng = np.random.default_rng(4)
    sampler = _sample_frank if kind == "frank" else _sample_joe
    theta = 5.0 if kind == "frank" else 2.0
    u = np.clip(sampler(rng, 460, theta), 1e-9, 1 - 1e-9)
    if kind == "joe_survival":
        u = 1.0 - u
    pdf = np.ones_like(u)
    params, info = dynamic.rolling_copula_params(kind, u[:400], pdf[:400], u[400:], pdf[400:], window=400, every=30)
    assert params.shape == (60, 1) and list(info["refits"]) == [0, 30] and not list(info["failed"])
    assert np.all(np.abs(params[:, 0] - theta) < (2.0 if kind == "frank" else 0.6))
    with pytest.raises(ValueError, match="copula must be one of"):
        dynamic.rolling_copula_params("clayton", u[:400], pdf[:400], u[400:], pdf[400:], window=400)
