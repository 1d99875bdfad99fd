"""The score-driven copula without a GPU: the float64 restatement (tests/gas_reference.py, hand-derived
scores) against the 50-digit fixture (tests/golden/gas_copula.kat, scores by numerical differentiation),
the fixture's freshness, the tie to the project's own densities, the optimiser's control flow on a CPU
likelihood, the no-look-ahead property of gas_copula_params, the driver's flag checks and the C ABI's
host-side validation.

Bars.  The device is held to 1e-12 (likelihood: of sum |l_t|; path: relative).  The recursion feeds
rounding back through alpha s_t, so the fixture's candidate rows are chosen such that a plain float64
evaluation stays within CPU_BAR = 1e-13 of the truth on both measures; this module asserts it.
Student: the restatement takes the fixture's quantiles -- scipy's stdtrit is good to about 1e-11
only, which is the quantile routine's error and not the recursion's (printed below for the record).
"""
import importlib.util
import os

import numpy as np
import pytest

import gas_cases as GC
import gas_reference as GR
from conftest import load_golden

CASES = GC.cases()
IDS = [GC.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def kat():
    return GC.load_kat()


def _ratios(got, truth):
    th, lc, ll, sc = truth
    e_th = np.max(np.abs(got["theta"].astype(GR.LD) - th) / np.abs(th))
    e_lc = np.max(np.abs(got["logc"].astype(GR.LD) - lc) / np.maximum(np.abs(lc), sc[:, None] / lc.shape[1]))
    e_ll = np.max(np.abs(got["ll"].astype(GR.LD) - ll) / sc)
    return float(e_th), float(e_lc), float(e_ll)


# ------------------------------------------------------------------ restatement against the fixture
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float64_restatement_holds_the_cpu_bar(kat, case):
    kind, dim, nu = case
    u, prm = GC.series(case), GC.param_rows(case)
    assert str(kat[GC.key(case, "sha")]) == GC.case_digest(u, prm), "the fixture was generated from other inputs"
    assert np.min(u) < 1e-9 and 1.0 - np.max(u) < 1e-9
    assert prm[0, 1] == 0.0 and prm[1, 2] == 0.97
    for n in GC.NS:
        z = kat[GC.key(case, "z")][:n] if kind == "student" else None
        got = GR.run(kind, u[:n], prm, nu, z=z)
        e_th, e_lc, e_ll = _ratios(got, GC.truth(kat, case, n))
        print(f"MEASURED {GC.case_id(case)} N={n} float64 restatement: theta {e_th:.2e}  logc {e_lc:.2e}  ll {e_ll:.2e}")
        assert np.all(np.isfinite(got["theta"])) and np.all(np.isfinite(got["ll"]))
        assert e_th <= GC.CPU_BAR and e_ll <= GC.CPU_BAR, (GC.case_id(case), n, e_th, e_ll)
        if kind == "student":
            own = GR.run(kind, u[:n], prm, nu)
            print(f"MEASURED {GC.case_id(case)} N={n} with scipy's stdtrit: ll {_ratios(own, GC.truth(kat, case, n))[2]:.2e}")
    # the clamp row sits at +40 from the first update on and stays finite
    full = GR.run(kind, u, prm, nu, z=kat[GC.key(case, "z")] if kind == "student" else None)
    hi = GR.link(kind, np.array([GR.F_CLAMP]))[0][0]
    assert np.all(full["theta"][3, 1:] == hi) and np.isfinite(full["ll"][3])


def test_longdouble_restatement_is_closer_still(kat):
    extended = np.finfo(GR.LD).eps < np.finfo(np.float64).eps
    case = ("gumbel_survival", 3, None)
    got = GR.run(case[0], GC.series(case), GC.param_rows(case), dtype=GR.LD)
    e_th, _, e_ll = _ratios(got, GC.truth(kat, case, GC.N_MAX))
    bar = 4e-16 if extended else GC.CPU_BAR           # the fixture is stored as float64 roundings
    assert e_th <= bar and e_ll <= bar


def _gen():
    spec = importlib.util.spec_from_file_location("gen_gas_kat", os.path.join(GC.HERE, "kat", "gen_gas_kat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_fresh(kat):
    """The generator, re-run in memory, reproduces the committed file (every case; it takes seconds)."""
    pytest.importorskip("mpmath")
    gen = _gen()
    for case in CASES:
        rows = gen.case_rows(case)
        for k, a in rows.items():
            assert np.array_equal(np.asarray(a), kat[GC.key(case, k)]), (GC.case_id(case), k)
    assert len(kat) == sum(6 if c[0] in GR.ELLIPTICAL else 5 for c in CASES)


# ------------------------------------------------------------------ the model is the project's densities
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_alpha_zero_is_the_static_log_density(case):
    """alpha = 0: theta_t = link(f_bar) for every t and LL = sum log c(u; theta) by copula_var.copulas (the
    elliptical kinds from scipy's quantiles on both sides)."""
    from scipy import special
    from copula_var import copulas
    kind, dim, nu = case
    u, row = GC.series(case), GC.param_rows(case)[:1]
    got = GR.run(kind, u, row, nu)
    th = float(got["theta"][0, 0])
    assert np.all(np.abs(got["theta"][0] - th) <= 1e-14 * abs(th))
    corr = np.array([[1.0, th], [th, 1.0]])
    with np.errstate(all="ignore"):
        if kind == "gaussian":
            want = np.log(copulas.gaussian_from_quantiles(special.ndtri(u), corr))
        elif kind == "student":
            want = np.log(copulas.student_from_quantiles(special.stdtrit(nu, u), nu, corr))
        elif kind == "plackett":
            want = np.log(copulas.plackett(u, th))
        elif GR.FAMILY[kind] == "gumbel":
            want = copulas.gumbel_log_density(u, th, survival=kind in GR.ROTATED)
        elif kind == "frank":
            want = copulas.frank_log_density(u, th)
        else:
            want = copulas.joe_log_density(u, th, survival=kind in GR.ROTATED)
    # both sides are float64 evaluations of one formula in two arrangements: 1e-10 of the larger terms
    np.testing.assert_allclose(got["logc"][0], want, rtol=1e-10, atol=1e-10)
    assert abs(float(got["ll"][0]) - float(np.sum(want))) <= 1e-10 * float(np.sum(np.abs(want)))


def test_failure_rows_are_nan_and_leave_their_neighbours_alone():
    case = ("frank", 3, None)
    u, good = GC.series(case), GC.param_rows(case)
    rows = np.vstack((good[:2], [[0.1, 0.05, 1.0]], good[2:3], [[np.nan, 0.1, 0.5]], [[0.1, 0.05, -1.5]], good[3:]))
    got = GR.run("frank", u, rows)
    alone = GR.run("frank", u, good)
    keep = [0, 1, 3, 6]
    assert np.array_equal(got["ll"][keep], alone["ll"]) and np.array_equal(got["theta"][keep], alone["theta"])
    assert np.all(np.isnan(got["ll"][[2, 4, 5]])) and np.all(np.isnan(got["theta"][[2, 4, 5]]))


# ------------------------------------------------------------------ optimiser on a CPU likelihood
def swinging_gaussian(n=600, seed=20240611):
    """u (n, 2) from a Gaussian copula whose rho_t swings between 0.1 and 0.8 (period 200 rows)."""
    from scipy import special
    rng = np.random.default_rng(seed)
    rho = 0.45 + 0.35 * np.sin(2 * np.pi * np.arange(n) / 200.0)
    e = rng.standard_normal((n, 2))
    z = np.column_stack((e[:, 0], rho * e[:, 0] + np.sqrt(1 - rho * rho) * e[:, 1]))
    return special.ndtr(z), rho


class CountingLoglik:
    def __init__(self, fn):
        self.fn, self.calls, self.rows = fn, 0, []

    def __call__(self, rows):
        self.calls += 1
        self.rows.append(np.array(rows))
        return self.fn(rows)


def gaussian_static_rho(u):
    from scipy import special
    from copula_var.optim.copula_fit import GaussianCopulaOptimizer
    return float(GaussianCopulaOptimizer(u, np.ones_like(u), ndtri=special.ndtri).optimize()["corr_matrix"][0, 1])


@pytest.fixture(scope="module")
def swing_fit():
    from copula_var.optim.copula_fit import GasCopulaOptimizer
    u, rho = swinging_gaussian()
    dens = np.full_like(u, 0.7)
    ll = CountingLoglik(GR.loglik("gaussian", u))
    opt = GasCopulaOptimizer(u, dens, "gaussian", static_theta=gaussian_static_rho(u), loglik=ll)
    grid_probe = CountingLoglik(GR.loglik("gaussian", u))
    return u, rho, dens, opt, opt.optimize(), ll, grid_probe


def test_optimizer_beats_the_static_fit_on_a_swinging_correlation(swing_fit):
    u, rho, dens, opt, res, ll, _ = swing_fit
    print(f"MEASURED swinging Gaussian: nll {res['nll']:.4f}  static_nll {res['static_nll']:.4f}  "
          f"(omega, alpha, beta) = ({res['omega']:.5f}, {res['alpha']:.5f}, {res['beta']:.5f})  "
          f"launches {res['launches']}  evaluations {res['evaluations']}")
    assert res["nll"] < res["static_nll"] - 5.0
    assert res["nll"] <= res["static_nll"]
    assert 0.0 <= res["alpha"] <= 4.0 and 0.0 <= res["beta"] <= 0.999
    # the likelihoods include the marginal densities' term, as the static optimisers' do
    own = -(np.sum(np.log(dens)) + GR.loglik("gaussian", u)(np.array([[res["omega"], res["alpha"], res["beta"]]]))[0])
    assert res["nll"] == pytest.approx(own, rel=1e-14)
    # the filtered path follows the swing
    path = GR.run("gaussian", u, [[res["omega"], res["alpha"], res["beta"]]])["theta"][0, :-1]
    assert np.corrcoef(path[100:], rho[100:])[0, 1] > 0.6
    assert set(res) >= {"omega", "alpha", "beta", "nll", "static_nll", "launches", "evaluations"}
    assert res["launches"] == ll.calls and res["evaluations"] == sum(len(r) for r in ll.rows)


def test_optimizer_grid_is_one_launch_and_steps_are_seven_rows(swing_fit):
    u, rho, dens, opt, res, ll, _ = swing_fit
    assert ll.rows[0].shape == (16, 3)                              # the whole grid in the first launch
    betas, alphas = sorted(set(ll.rows[0][:, 2])), sorted(set(ll.rows[0][:, 1]))
    assert betas == [0.0, 0.5, 0.9, 0.97] and alphas == [0.0, 0.02, 0.1, 0.4]
    fbar = res["f_bar"]
    assert np.allclose(ll.rows[0][:, 0], fbar * (1 - ll.rows[0][:, 2]), rtol=0, atol=1e-15)
    assert all(r.shape in ((7, 3), (1, 3)) for r in ll.rows[1:])
    assert sum(r.shape == (1, 3) for r in ll.rows[1:]) == 3         # one closing evaluation per refined start


def test_optimizer_never_launches_penalty_rows():
    from copula_var.optim.copula_fit import GasCopulaOptimizer
    u, _ = swinging_gaussian(120)
    ll = CountingLoglik(GR.loglik("gaussian", u))
    opt = GasCopulaOptimizer(u, np.ones_like(u), "gaussian", static_theta=0.4, loglik=ll)
    rows = np.array([[0.1, 0.05, 0.5], [0.1, 0.05, 1.0], [np.nan, 0.0, 0.1], [0.1, np.inf, 0.1], [0.1, 0.05, -1.0],
                     [0.2, 0.0, 0.9]])
    v = opt.negative_log_likelihoods(rows)
    assert ll.calls == 1 and ll.rows[0].shape == (2, 3) and np.array_equal(ll.rows[0], rows[[0, 5]])
    assert np.all(v[[1, 2, 3, 4]] == 1e10) and np.all(v[[0, 5]] < 1e10)
    assert opt.launches == 1 and opt.evaluations == 2
    v = opt.negative_log_likelihoods(rows[1:5])                     # nothing to launch at all
    assert ll.calls == 1 and np.all(v == 1e10)
    nan_ll = GasCopulaOptimizer(u, np.ones_like(u), "gaussian", static_theta=0.4, loglik=lambda r: np.full(len(r), np.nan))
    assert np.all(nan_ll.negative_log_likelihoods(rows[:1]) == 1e10)
    with pytest.raises(ValueError, match="not finite at any grid start"):
        nan_ll.optimize()


def test_optimizer_rejects_what_the_kernels_do_not_build():
    from copula_var.optim.copula_fit import GasCopulaOptimizer
    u3 = np.full((10, 3), 0.5)
    for kind in ("gaussian", "student", "plackett"):
        with pytest.raises(ValueError, match="not built for 3"):
            GasCopulaOptimizer(u3, u3, kind, nu=6.0)
    with pytest.raises(ValueError, match="needs nu"):
        GasCopulaOptimizer(u3[:, :2], u3[:, :2], "student")
    with pytest.raises(ValueError, match="copula must be one of"):
        GasCopulaOptimizer(u3, u3, "clayton")


def test_optimizer_clamps_saturated_marginals():
    from copula_var.optim.copula_fit import GasCopulaOptimizer
    u, _ = swinging_gaussian(60)
    u[3, 0], u[9, 1] = 0.0, 1.0
    ll = CountingLoglik(GR.loglik("gumbel", np.clip(u, 2.0 ** -53, 1.0 - 2.0 ** -53)))
    opt = GasCopulaOptimizer(u, np.ones_like(u), "gumbel", static_theta=1.5, loglik=ll)
    assert opt._u[3, 0] == 2.0 ** -53 and opt._u[9, 1] == 1.0 - 2.0 ** -53
    assert np.all(opt.negative_log_likelihoods([[0.1, 0.02, 0.5]]) < 1e10)


# ------------------------------------------------------------------ gas_copula_params
def _cpu_path(copula, nu):
    def path(u, p):
        r = GR.run(copula, u, [p], nu)
        return r["theta"][0], r["logc"][0]
    return path


@pytest.mark.parametrize("copula,dim,nu", [("student", 2, 6.0), ("gumbel_survival", 3, None), ("frank", 2, None)])
def test_gas_copula_params_packing_and_no_look_ahead(copula, dim, nu):
    from copula_var.dynamic import gas_copula_params
    case = (copula, dim, nu)
    u = GC.series(case)
    um, uo = u[:30], u[30:]
    static = np.array([nu, 0.4]) if copula == "student" else np.array([2.0])
    fit = {"omega": 0.02, "alpha": 0.05, "beta": 0.9}
    base, info = gas_copula_params(copula, um, uo, static, fit=fit, path=_cpu_path(copula, nu))
    T = uo.shape[0]
    assert base.shape == (T, 2 if copula == "student" else 1) and info["fit"] is fit
    assert info["in_sample_path"].shape == (30,)
    if copula == "student":
        assert np.all(base[:, 0] == nu)
    whole = GR.run(copula, u, [[0.02, 0.05, 0.9]], nu)["theta"][0]
    assert np.array_equal(base[:, -1], whole[30:30 + T]) and np.array_equal(info["in_sample_path"], whole[:30])
    for j in (0, 7, T - 1):
        moved = uo.copy()
        moved[j] = 0.5 * (moved[j] + 0.5)
        got, _ = gas_copula_params(copula, um, moved, static, fit=fit, path=_cpu_path(copula, nu))
        assert np.array_equal(got[:j + 1], base[:j + 1]), j            # rows <= j: bit-identical
        if j < T - 1:
            assert not np.array_equal(got[j + 1:], base[j + 1:])


def test_gas_copula_params_fits_on_the_in_sample_rows_only():
    from copula_var.dynamic import gas_copula_params
    u, _ = swinging_gaussian(260)
    seen = {}

    def fit(copula, um, dens, nu, static_theta, device):
        seen.update(u=um.copy(), static=static_theta, nu=nu)
        return {"omega": 0.05, "alpha": 0.1, "beta": 0.8}

    out, info = gas_copula_params("gaussian", u[:200], u[200:], np.array([0.45]), fit=fit, path=_cpu_path("gaussian", None))
    assert np.array_equal(seen["u"], u[:200]) and seen["static"] == 0.45 and seen["nu"] is None
    assert out.shape == (60, 1) and np.all(np.abs(out) < 0.99)
    with pytest.raises(ValueError, match="built for 2 assets"):
        gas_copula_params("gaussian", np.full((5, 3), 0.5), np.full((2, 3), 0.5), np.array([0.1, 0.1, 0.1]), fit=fit)
    with pytest.raises(ValueError, match="copula must be one of"):
        gas_copula_params("clayton", u[:200], u[200:], np.array([2.0]), fit=fit)


def test_link_helpers_agree_with_the_restatement():
    from copula_var.optim.copula_fit import gas_link, gas_link_inverse
    f = np.array([-40.0, -3.0, -0.2, 0.0, 0.7, 5.0, 40.0])
    for kind in GR.FAMILY:
        np.testing.assert_allclose(gas_link(kind, f), GR.link(kind, f)[0], rtol=1e-13, atol=1e-15)
        for th in gas_link(kind, f[1:-1]):
            assert gas_link(kind, gas_link_inverse(kind, th)) == pytest.approx(th, rel=1e-9)
        lo, hi = GR.THETA_RANGE[GR.FAMILY[kind]]
        assert lo <= gas_link(kind, -40.0) and gas_link(kind, 40.0) <= hi


# ------------------------------------------------------------------ driver
def test_main_gas_flag_validation(tmp_path):
    from copula_var import main as M, synthetic
    from copula_var.main import build_parser
    base = ["--prices", "p.csv", "--tickers", "A", "B", "--start", "2009-04-15"]
    assert build_parser().parse_args(base).gas_copula is False
    assert build_parser().parse_args(base + ["--gas-copula"]).gas_copula is True
    z = load_golden("garch_student_n64")
    csv = tmp_path / "returns.csv"
    frame = synthetic.returns_frame(z["returns"])
    frame.to_csv(csv)
    base = ["--prices", str(csv), "--returns", "--tickers", *frame.columns, "--start", str(frame.index[0].date())]
    for extra, word in ((["--gas-copula"], "--exact-levels"),
                        (["--gas-copula", "--rolling-copula", "60", "--exact-levels", "0.05"], "choose one")):
        with pytest.raises(SystemExit) as e:
            M.main(base + extra)
        assert isinstance(e.value.code, str) and word in e.value.code


# ------------------------------------------------------------------ C ABI, host-side validation
def test_abi_validates_on_the_host():
    from copula_var import _native as N
    lib = N.lib()
    u = np.ascontiguousarray(GC.series(("frank", 3, None)))
    u2 = np.ascontiguousarray(u[:, :2])
    prm = np.array([[0.1, 0.05, 0.9]])
    out = np.full(64, 7.0)

    def ll(copula, survival, dim, nu, params=prm, B=1, uu=u2, n=None, o=out):
        n = uu.shape[0] if n is None else n
        return lib.cvq_gas_loglik(0, copula, survival, dim, nu, None if params is None else N.ptr(params), B,
                                  None if uu is None else N.ptr(uu), n, None if o is None else N.ptr(o), N.MEM_HOST)

    def path(copula, survival, dim, nu, params=prm, uu=u2, n=None, th=out):
        n = uu.shape[0] if n is None else n
        return lib.cvq_gas_path(0, copula, survival, dim, nu, None if params is None else N.ptr(params),
                                None if uu is None else N.ptr(uu), n, None if th is None else N.ptr(th), None, N.MEM_HOST)

    inv, uns = N.CVQ_ERR_INVALID, N.CVQ_ERR_UNSUPPORTED
    assert ll(N.FRANK, 0, 2, 0.0, params=None) == inv and ll(N.FRANK, 0, 2, 0.0, uu=None, n=4) == inv
    assert ll(N.FRANK, 0, 2, 0.0, o=None) == inv and path(N.FRANK, 0, 2, 0.0, th=None) == inv
    assert ll(N.FRANK, 0, 2, 0.0, B=0) == inv and ll(N.FRANK, 0, 2, 0.0, n=0) == inv and path(N.FRANK, 0, 2, 0.0, n=0) == inv
    assert ll(N.FRANK, 0, 1, 0.0) == inv and ll(N.FRANK, 0, 4, 0.0) == inv and path(N.JOE, 0, 4, 0.0) == inv
    for nu in (0.0, -2.0, np.nan, np.inf):
        assert ll(N.STUDENT, 0, 2, nu) == inv and path(N.STUDENT, 0, 2, nu) == inv
    assert ll(N.FRANK, 1, 2, 0.0) == inv                                  # no rotation of Frank
    for bad, row in ((0.0, 5), (1.0, 0), (np.nan, 47), (-0.2, 11), (1.5, 3)):
        ub = u2.copy()
        ub[row, 1] = bad
        assert ll(N.GUMBEL, 0, 2, 0.0, uu=ub) == inv
        assert f"at row {row}" in lib.cvq_last_error().decode()
        assert path(N.JOE_SURVIVAL, 0, 2, 0.0, uu=ub) == inv and f"at row {row}" in lib.cvq_last_error().decode()
    for kind in (N.GAUSSIAN, N.STUDENT, N.PLACKETT):
        assert ll(kind, 0, 3, 6.0, uu=u) == uns and path(kind, 0, 3, 6.0, uu=u) == uns
    assert ll(8, 0, 2, 0.0) == uns and ll(-1, 0, 2, 0.0) == uns and path(99, 0, 2, 0.0) == uns
    assert lib.cvq_last_error()
    assert np.all(out == 7.0)                                             # nothing was written


def test_engine_rejects_bad_names_and_shapes():
    from copula_var import engine
    u = GC.series(("frank", 2, None))
    with pytest.raises(ValueError, match="copula must be one of"):
        engine.gas_loglik(u, "clayton", [[0.1, 0.1, 0.5]])
    with pytest.raises(ValueError, match="needs nu"):
        engine.gas_path(u, "student", [0.1, 0.1, 0.5])
    with pytest.raises(ValueError, match="omega, alpha, beta"):
        engine.gas_loglik(u, "frank", [[0.1, 0.1]])
    with pytest.raises(ValueError, match=r"\(N, dim\)"):
        engine.gas_loglik(u[:, 0], "frank", [[0.1, 0.1, 0.5]])
    with pytest.raises(ValueError, match="at row 2"):
        bad = u.copy()
        bad[2, 0] = 1.0
        engine.gas_loglik(bad, "frank", [[0.1, 0.1, 0.5]])
