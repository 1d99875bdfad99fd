"""Per-date-record quantiles without a GPU: host-side validation of cvq_dynamic_quantiles, the numpy
checker (tests/dynamic_reference.py) and its decision margins on the GPU tests' inputs
(tests/dynamic_cases.py), and copula_var/dynamic.py -- drifting weights, out-of-sample PITs and
rolling copula fits on host likelihoods -- and the CLI flags."""
import ctypes as C

import numpy as np
import pytest
from scipy.stats import norm, t as student_t

import dynamic_cases as DC
import dynamic_reference as R
import es_reference as E
import quantile_reference as Q
from conftest import load_golden

MARGIN = 1e-7                     # 1000 x the slab bar of 1e-10: a condition of the GPU tests' exact equality
# the smallest margin of each case at R.LEVELS, as first measured on the CPU: a drift of the inputs shows
FLOOR = {"cfg2_n64": 5.5e-5, "garch_student_n64": 5.2e-4, "cfg5_n64": 5.8e-4, "msm_gauss_n64": 3.8e-4,
         "msm_plackett_n64": 3.9e-5, "cfg2_n64_gumbel_survival": 6.9e-4, "cfg5_n64_gumbel": 1.3e-4,
         "cfg4_k4_n16": 9.7e-4, "garch3d_student_n16": 4.0e-3, "2d_n70": 1.0e-3, "2d_n130": 5.4e-5,
         "3d_n17": 3.4e-3}


def _tppf(u, nu):
    return student_t.ppf(u, nu)


# ------------------------------------------------------------------ the entry point on the host
def test_entry_point_validates_on_the_host():
    """Every check that needs no plan (the per-date checks read the plan's dim and batch:
    tests/test_dynamic_gpu.py)."""
    from copula_var import _native as N
    lib = N.lib()
    assert lib.cvq_version() >= 10800
    out = np.full(8, -1.0)
    a = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-6, 0.0)
    lv = np.array([0.05])
    assert lib.cvq_dynamic_quantiles(None, C.byref(a), None, None, None, N.ptr(lv), 1, N.ptr(out), None, None,
                                     N.MEM_HOST) == N.CVQ_ERR_INVALID
    assert b"NULL" in lib.cvq_last_error() and np.all(out == -1.0)
    b = C.c_int64()
    assert lib.cvq_dynamic_scratch(None, 1, C.byref(b)) == N.CVQ_ERR_INVALID
    assert hasattr(N.lib(), "cvq_dynamic_scratch")


# ------------------------------------------------------------------ the checker
@pytest.mark.parametrize("case", ["cfg2_n64", "cfg4_k4_n16"])
def test_checker_at_the_plans_own_record_is_the_quantile_checker(case):
    """Every date at the golden's own parameters, weights and one mean: the one-date Problems
    reproduce quantile_reference.quantiles on the batch."""
    z = load_golden(case)
    P = E.problem_of(z, slice(0, 3))
    ptf = float(z["ptf_mean"])
    dates = [R.one_date(P, t, P.copula_params, P.w) for t in range(P.T)]
    got = R.dynamic_quantiles(dates, R.LEVELS, np.full(P.T, ptf))
    ref = Q.quantiles(P, R.LEVELS, ptf)
    for a, b in zip(got, ref):
        assert a.shape == (3, 3) and np.array_equal(a, b, equal_nan=True)


def test_case_dates_carry_their_own_records():
    P, cp, w, pm, dates = DC.problem("cfg2_n64")
    assert len(dates) == P.T == 6 and cp.shape == (6, 2) and w.shape == (6, 2)
    assert np.all(cp[:, 0] == 6.0) and np.array_equal(cp[:, 1], R.RHO2)
    for t, Pt in enumerate(dates):
        assert Pt.T == 1 and np.array_equal(Pt.w, w[t]) and Pt.nu == 6.0 and Pt.R[0, 1] == R.RHO2[t]
        assert np.array_equal(Pt.fbs[0], P.fbs[t]) and np.array_equal(Pt.pi[0], P.pi[t])
    assert np.array_equal(pm, 0.01 * np.arange(1, 7))
    _, cp, _, _, dates = DC.problem("cfg5_n64_gumbel")
    assert [d.theta for d in dates] == list(R.GUMBEL) and not dates[0].survival
    _, cp, w, _, dates = DC.problem("3d_n17")
    assert len(dates) == 3 and np.array_equal(cp[:, 1:], R.RHO3[:3]) and np.array_equal(w, R.W3[:3])
    assert np.array_equal(DC.problem("2d_n130")[1][:, 0], R.PLACKETT[:4])


@pytest.mark.parametrize("name", list(DC.CASES) + list(DC.EDGES))
def test_checker_margin(name):
    """The premise of the GPU tests' exact comparison: no evaluated F within 1e-7 of a level, and no
    level outside the bracket."""
    var, es, _, margin = DC.reference(name)
    P = DC.problem(name)[0]
    print(name, "margin", margin.min(), "per level", margin.min(axis=0))
    assert var.shape == (P.T, len(DC.levels(name)))
    assert margin.min() >= MARGIN
    assert margin.min() >= FLOOR[name]
    assert not np.isnan(var).any() and not np.isnan(es).any()


# ------------------------------------------------------------------ drift_weights
def test_drift_weights_three_steps_by_hand():
    from copula_var.dynamic import drift_weights, from_tickers, to_tickers
    r = np.array([[1.0, -2.0], [0.5, 0.25], [-3.0, 4.0], [9.0, 9.0]])
    w0 = np.array([0.25, 0.75])                       # constructor convention: ticker 0 carries 0.75, ticker 1 0.25
    w = drift_weights(r, w0)
    assert w.shape == (4, 2) and np.array_equal(w[0], w0)
    np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    a = np.array([0.75, 0.25])                        # by ticker
    for t in range(3):
        a = a * np.exp(r[t] / 100.0)
        a = a / a.sum()
        np.testing.assert_allclose(w[t + 1], [a[1], a[0]], rtol=1e-15)
    # step 1 in closed form: ticker 0 gains 1 %, ticker 1 loses 2 %
    g0, g1 = 0.75 * np.exp(0.01), 0.25 * np.exp(-0.02)
    np.testing.assert_allclose(w[1], [g1 / (g0 + g1), g0 / (g0 + g1)], rtol=1e-15)
    assert np.array_equal(drift_weights(np.vstack((r[:3], [[-50.0, 50.0]])), w0), w)   # the last row is not read
    assert np.array_equal(drift_weights(np.zeros((5, 2)), w0), np.tile(w0, (5, 1)))    # no returns, no drift
    # three assets: each entry drifts with the ticker it weighs (Q10: ticker c carries w[c + 1], the last w[0])
    w3 = np.array([0.2, 0.3, 0.5])
    assert np.array_equal(to_tickers(w3), [0.3, 0.5, 0.2]) and np.array_equal(from_tickers(to_tickers(w3)), w3)
    r3 = np.array([[0.0, 0.0, 10.0], [0.0, 0.0, 0.0]])
    got = drift_weights(r3, w3)[1]
    s = 0.3 + 0.5 + 0.2 * np.exp(0.1)
    np.testing.assert_allclose(got, [0.2 * np.exp(0.1) / s, 0.3 / s, 0.5 / s], rtol=1e-15)
    with pytest.raises(ValueError):
        drift_weights(r, [0.5, 0.6])
    with pytest.raises(ValueError):
        drift_weights(r, [0.2, 0.3, 0.5])


def test_drift_weights_has_no_look_ahead():
    from copula_var.dynamic import drift_weights
    rng = np.random.default_rng(5)
    r = rng.normal(0.0, 1.5, size=(30, 3))
    w0 = np.array([0.5, 0.25, 0.25])
    w = drift_weights(r, w0)
    r2 = r.copy()
    r2[12:] = rng.normal(0.0, 5.0, size=(18, 3))
    assert np.array_equal(drift_weights(r2, w0)[:13], w[:13])      # row t reads the rows before t


# ------------------------------------------------------------------ oos_pits
def test_oos_pits():
    from copula_var.conditional import _msm_cdf
    from copula_var.dynamic import oos_pits
    rng = np.random.default_rng(7)
    sig = rng.uniform(0.5, 2.0, size=(9, 2))
    r = rng.normal(0.0, 1.0, size=(9, 2))
    for per in (sig, [sig]):
        u, pdf = oos_pits("garch", per, None, r)
        np.testing.assert_allclose(u, norm.cdf(r / sig), rtol=1e-14)
        np.testing.assert_allclose(pdf, norm.pdf(r / sig) / sig, rtol=1e-14)
    z = load_golden("cfg2_n64")
    fbs, uvs = z["forecasts_by_states"][:9], z["unique_vol_states"]
    u, pdf = oos_pits("msm", (fbs, z["forecasts"][:9]), uvs, r)
    for c in range(2):
        np.testing.assert_allclose(u[:, c], _msm_cdf(fbs[:, c, :], uvs[c], r[:, c]), rtol=1e-14)
        want = np.sum(fbs[:, c, :] * norm.pdf(r[:, c, None] / uvs[c][None, :]) / uvs[c][None, :], axis=1)
        np.testing.assert_allclose(pdf[:, c], want, rtol=1e-13)
    assert np.all((u > 0) & (u < 1)) and np.all(pdf > 0)
    with pytest.raises(ValueError):
        oos_pits("garch", sig, None, r[:-1])
    with pytest.raises(ValueError):
        oos_pits("arch", sig, None, r)


# ------------------------------------------------------------------ rolling_copula_params
@pytest.fixture(scope="module")
def sample():
    """160 in-sample and 60 out-of-sample rows of one Student sample (nu 5, rho 0.5)."""
    from oracle.copula_fit import student_sample
    u, d = student_sample(220, 2, 5.0, 0.5, seed=41)
    return u[:160], d[:160], u[160:], d[160:]


KW = {"student": dict(tppf=_tppf), "gaussian": dict(ndtri=norm.ppf), "plackett": {}, "gumbel": {},
      "gumbel_survival": {}}
STATIC = {"student": np.array([5.0, 0.4]), "gaussian": None, "plackett": None, "gumbel": None,
          "gumbel_survival": None}


@pytest.mark.parametrize("copula", ["student", "gaussian", "plackett", "gumbel_survival"])
def test_rolling_first_fit_is_the_static_fit_and_parameters_hold(copula, sample):
    from copula_var.dynamic import fit_copula, rolling_copula_params
    from copula_var.optim import copula_fit as F
    um, dm, uo, do = sample
    path, info = rolling_copula_params(copula, um, dm, uo, do, window=10_000, every=25, static_params=STATIC[copula],
                                       **KW[copula])
    assert path.shape == (60, 2 if copula == "student" else 1)
    assert info["refits"] == [0, 25, 50] and info["failed"] == [] and np.all(np.isfinite(info["nll"]))
    # held between refits
    for lo, hi in ((0, 25), (25, 50), (50, 60)):
        assert np.all(path[lo:hi] == path[lo])
    assert not np.array_equal(path[0], path[25]) and not np.array_equal(path[25], path[50])
    # the fit at t = 0 with window >= the in-sample length: the same optimiser's static fit on those rows
    if copula == "student":
        static, _ = fit_copula("student", um, dm, nu=5.0, tppf=_tppf)
        assert path[0, 0] == 5.0 and np.all(path[:, 0] == 5.0)
    elif copula == "gaussian":
        res = F.GaussianCopulaOptimizer(um, dm, ndtri=norm.ppf).optimize()
        static = res["optimized_params"]
    elif copula == "plackett":
        static = [F.PlackettCopulaOptimizer(um, dm).optimize()["theta"]]
    else:
        static = [F.GumbelCopulaOptimizer(um, dm, survival=True).optimize()["theta"]]
    assert np.array_equal(path[0], np.asarray(static, dtype=np.float64))
    # later fits see [in-sample, then the out-of-sample rows before the date]
    later, _ = fit_copula(copula, np.vstack((um, uo[:25])), np.vstack((dm, do[:25])), start=path[0],
                          nu=5.0 if copula == "student" else None, **KW[copula])
    assert np.array_equal(path[25], later)


@pytest.mark.parametrize("copula", ["student", "gaussian"])
def test_rolling_has_no_look_ahead(copula, sample):
    from copula_var.dynamic import rolling_copula_params
    um, dm, uo, do = sample
    kw = dict(window=120, every=10, static_params=STATIC[copula], **KW[copula])
    path, _ = rolling_copula_params(copula, um, dm, uo, do, **kw)
    t0 = 30
    rng = np.random.default_rng(3)
    uo2, do2 = uo.copy(), do.copy()
    uo2[t0:] = rng.uniform(0.05, 0.95, size=uo2[t0:].shape)       # rows >= t0 replaced
    do2[t0:] = rng.uniform(0.5, 1.5, size=do2[t0:].shape)
    path2, _ = rolling_copula_params(copula, um, dm, uo2, do2, **kw)
    assert np.array_equal(path2[:t0 + 1], path[:t0 + 1])          # dates <= t0: bit for bit
    assert not np.array_equal(path2[t0 + 10:], path[t0 + 10:])    # and the later refits do see them
    # the window: the fit at t reads rows [n_in + t - window, n_in + t) only
    um2, dm2 = um.copy(), dm.copy()
    um2[:40] = rng.uniform(0.05, 0.95, size=(40, 2))              # in-sample rows out of every window
    path3, _ = rolling_copula_params(copula, um2, dm, uo, do, **kw)
    assert np.array_equal(path3, path)


def test_rolling_failed_fit_keeps_the_previous_parameters(sample):
    from copula_var.dynamic import fit_copula, rolling_copula_params
    um, dm, uo, do = sample
    calls = []

    def flaky(copula, u, pdf, start=None, **kw):
        calls.append((u.shape[0], None if start is None else np.array(start)))
        if len(calls) == 2:
            raise ValueError("no finite likelihood")
        if len(calls) == 4:
            return np.array([float("nan")]), 1.0
        if len(calls) == 5:
            return np.array([2.0]), 1e10
        return fit_copula(copula, u, pdf, start=start, **kw)

    path, info = rolling_copula_params("gumbel", um, dm, uo, do, window=100, every=10, fit=flaky)
    assert info["refits"] == [0, 10, 20, 30, 40, 50] and info["failed"] == [10, 30, 40]
    assert np.all(path[10:20] == path[0]) and np.all(path[30:50] == path[20]) and path[20, 0] != path[0, 0]
    assert np.isnan(info["nll"][1]) and np.isfinite(info["nll"][2])
    assert [c[0] for c in calls] == [100] * 6                     # the last `window` rows each time
    assert calls[0][1] is None and np.array_equal(calls[2][1], path[0])    # warm start from the last good fit
    assert np.array_equal(calls[5][1], path[20])
    # a first fit that fails: the static parameters stand in; without them there is nothing to keep
    always = lambda *a, **k: (_ for _ in ()).throw(ValueError("x"))
    path, info = rolling_copula_params("gumbel", um, dm, uo[:5], do[:5], window=50, every=2, static_params=[3.0],
                                       fit=always)
    assert np.all(path == 3.0) and info["failed"] == [0, 2, 4]
    with pytest.raises(ValueError, match="first"):
        rolling_copula_params("gumbel", um, dm, uo[:5], do[:5], window=50, every=2, fit=always)
    with pytest.raises(ValueError, match="nu"):
        rolling_copula_params("student", um, dm, uo, do, window=50)
    with pytest.raises(ValueError):
        rolling_copula_params("clayton", um, dm, uo, do, window=50)
    with pytest.raises(ValueError):
        rolling_copula_params("gumbel", um, dm[:-1], uo, do, window=50)


# ------------------------------------------------------------------ CLI
def test_main_dynamic_flags_parse():
    from copula_var.main import build_parser, main
    base = ["--prices", "p.csv", "--tickers", "A", "B", "--start", "2009-04-15"]
    a = build_parser().parse_args(base)
    assert a.rolling_copula is None and a.refit_every == 21 and a.drift_weights is False
    a = build_parser().parse_args(base + ["--rolling-copula", "250", "--refit-every", "5", "--drift-weights"])
    assert a.rolling_copula == 250 and a.refit_every == 5 and a.drift_weights is True
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--rolling-copula", "x"])


def test_main_dynamic_flags_need_exact_levels(tmp_path):
    from copula_var import main as M, synthetic
    z = load_golden("garch_student_n64")
    csv = tmp_path / "returns.csv"
    frame = synthetic.returns_frame(z["returns"])
    frame.to_csv(csv)
    base = ["--prices", str(csv), "--returns", "--tickers", *frame.columns, "--start", str(frame.index[0].date())]
    for extra in (["--rolling-copula", "60"], ["--drift-weights"], ["--refit-every", "5", "--exact-levels", "0.05"],
                  ["--rolling-copula", "1", "--exact-levels", "0.05"]):
        with pytest.raises(SystemExit) as e:
            M.main(base + extra)
        assert isinstance(e.value.code, str) and "--" in e.value.code
