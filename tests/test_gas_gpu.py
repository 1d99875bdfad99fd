"""The score-driven copula kernels (csrc/cvq_gas_kernels.h: k_gas_prep, k_gas_loglik, k_gas_path) on the
MI355X against the 50-digit fixture tests/golden/gas_copula.kat -- every kind and dimension, N in
{1, 2, 48} -- the batch / staging invariances, the failure lanes, one end-to-end hand-over to
cvq_dynamic_quantiles per kind, and the optimiser on the device.

Bars (the project's LL_BAR of test_insample_kernels_gpu.py).  Likelihood: |device - truth| <=
1e-12 * sum |l_t|.  Path: rtol 1e-12 on theta_t.  The fixture's rows are chosen so that a plain float64
evaluation holds 1e-13 on both (tests/test_gas_cpu.py asserts that), which leaves the device a decade.

Measured max ratios, from one run of this module on an MI355X (gfx950), beside the float64
restatement's on the same inputs (test_gas_cpu.py, on a CPU; Student from the fixture's quantiles):
                                   device ll   device theta   restatement ll   restatement theta
    gaussian2                      1.6e-15     6.5e-16        1.6e-15          6.5e-16
    student2_nu6                   2.2e-15     6.2e-16        4.1e-15          3.7e-16
    student2_nu5.364               3.1e-15     5.8e-16        3.1e-15          5.8e-16
    plackett2                      4.2e-15     6.7e-15        2.5e-15          4.7e-15
    gumbel2                        2.4e-15     2.0e-15        2.4e-15          1.8e-15
    gumbel3                        7.5e-16     1.5e-15        7.5e-16          1.2e-15
    gumbel_survival2               9.5e-16     1.3e-15        9.5e-16          1.5e-15
    gumbel_survival3               2.1e-15     1.5e-15        1.5e-15          1.6e-15
    frank2                         1.5e-15     1.2e-15        1.5e-15          1.5e-15
    frank3                         2.1e-15     7.2e-16        2.9e-15          8.8e-16
    joe2                           1.9e-15     1.4e-15        1.8e-15          1.2e-15
    joe3                           1.3e-15     1.0e-15        1.3e-15          1.0e-15
    joe_survival2                  8.6e-16     9.1e-16        8.6e-16          1.1e-15
    joe_survival3                  1.9e-15     9.5e-16        1.9e-15          1.2e-15
The bars are the project's, not these figures: one run does not license a tighter one.
"""
import ctypes as C

import numpy as np
import pytest

import gas_cases as GC
import gas_reference as GR
from conftest import load_golden

pytestmark = pytest.mark.gpu

CASES = GC.cases()
IDS = [GC.case_id(c) for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@pytest.fixture(scope="module")
def kat():
    return GC.load_kat()


# ------------------------------------------------------------------ against the fixture
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_loglik_and_path_against_the_fixture(kat, case):
    from copula_var import engine
    kind, dim, nu = case
    u, prm = GC.series(case), GC.param_rows(case)
    assert str(kat[GC.key(case, "sha")]) == GC.case_digest(u, prm)
    worst_ll = worst_th = 0.0
    for n in GC.NS:
        th, lc, ll, sc = GC.truth(kat, case, n)
        got = engine.gas_loglik(u[:n], kind, prm, nu=nu)
        r_ll = np.abs(got.astype(GR.LD) - ll) / sc
        worst_ll = max(worst_ll, float(np.max(r_ll)))
        assert np.all(np.isfinite(got))                                     # the clamp row included
        paths = [engine.gas_path(u[:n], kind, row, nu=nu) for row in prm]
        theta = np.array([p[0] for p in paths])
        logc = np.array([p[1] for p in paths])
        r_th = np.abs(theta.astype(GR.LD) - th) / np.abs(th)
        worst_th = max(worst_th, float(np.max(r_th)))
        print(f"MEASURED {GC.case_id(case)} N={n}: ll {float(np.max(r_ll)):.2e}  theta {float(np.max(r_th)):.2e}")
        assert np.all(r_ll <= GC.LL_BAR), (GC.case_id(case), n, [float(x) for x in r_ll])
        assert np.all(r_th <= GC.PATH_BAR), (GC.case_id(case), n, float(np.max(r_th)))
        # the path's own log densities sum, in row order, to the batched likelihood: same arithmetic
        assert np.array_equal(np.array([np.add.accumulate(row)[-1] for row in logc]), got)
        assert np.all(np.abs(logc.astype(GR.LD) - lc) <= GC.LL_BAR * np.maximum(np.abs(lc), sc[:, None]))
    hi = GR.link(kind, np.array([GR.F_CLAMP]))[0][0]
    assert np.all(np.abs(theta[3, 1:] - hi) <= 4e-16 * abs(hi))              # the clamp row sits at f = +40
    print(f"MEASURED {GC.case_id(case)} worst: ll {worst_ll:.2e}  theta {worst_th:.2e}")


def test_survival_flag_is_the_survival_kind():
    from copula_var import engine
    for base, dim in (("gumbel", 3), ("joe", 2)):
        case = (base + "_survival", dim, None)
        u, prm = GC.series(case), GC.param_rows(case)
        a = engine.gas_loglik(u, base + "_survival", prm)
        b = engine.gas_loglik(u, base, prm, survival=True)
        c = engine.gas_loglik(u, base, prm)
        assert np.array_equal(a, b) and not np.array_equal(a, c)


# ------------------------------------------------------------------ batches, staging, failure lanes
BATCH_CASES = [("student", 2, 5.364), ("frank", 3, None), ("gumbel_survival", 2, None)]


def _batch_rows(case, B):
    """B candidates around the case's own rows (seeded), with a NaN row and a |beta| >= 1 row inside."""
    rng = np.random.default_rng(1000 + B)
    base = GC.param_rows(case)[:3]
    rows = base[rng.integers(0, 3, B)] * (1.0 + 0.05 * rng.standard_normal((B, 3)))
    rows[:, 2] = np.clip(rows[:, 2], 0.0, 0.98)
    rows[:, 1] = np.abs(rows[:, 1])
    bad = []
    if B >= 3:
        rows[B // 2] = [np.nan, 0.05, 0.5]
        rows[B - 2] = [0.1, 0.05, 1.0]
        bad = [B // 2, B - 2]
    return rows, bad


@pytest.mark.parametrize("case", BATCH_CASES, ids=[GC.case_id(c) for c in BATCH_CASES])
def test_batches_are_bit_equal_to_single_rows_and_failures_stay_in_their_lane(case):
    from copula_var import engine
    kind, dim, nu = case
    u = GC.series(case)
    for B in (1, 65, 257):
        rows, bad = _batch_rows(case, B)
        got = engine.gas_loglik(u, kind, rows, nu=nu)
        good = [b for b in range(B) if b not in bad]
        assert np.all(np.isnan(got[bad])) and np.all(np.isfinite(got[good]))
        # B = 1 launches of the rows at the wave / block edges, the failures' neighbours and a sample
        pick = sorted(set([0, 63, 64, 255, 256, B - 1, B // 2 - 1, B // 2 + 1, B - 3] + list(range(0, B, 37))) & set(good))
        for b in pick:
            one = engine.gas_loglik(u, kind, rows[b:b + 1], nu=nu)
            assert one[0] == got[b], (B, b)
        for b in bad:
            theta, logc = engine.gas_path(u, kind, rows[b], nu=nu)
            assert np.all(np.isnan(theta)) and np.all(np.isnan(logc))


def test_a_row_that_is_not_finite_ends_the_candidate_there():
    """Device memory is not validated on the host: a margin at exactly 1 in row 10 makes l_10 NaN.  The
    likelihood is NaN; theta is the healthy series' up to theta_10 (which depends on rows 0 .. 9 only) and NaN
    after it; logc is NaN from row 10 on."""
    import torch
    from copula_var import _native as N, engine
    case = ("joe", 3, None)
    u, prm = GC.series(case), GC.param_rows(case)
    want_th, want_lc = engine.gas_path(u, "joe", prm[2])
    bad = u.copy()
    bad[10, 1] = 1.0
    dev = torch.device("cuda:0")
    du = torch.from_numpy(bad).to(dev)
    n = u.shape[0]
    out = torch.zeros(len(prm), dtype=torch.float64, device=dev)
    th = torch.zeros(n + 1, dtype=torch.float64, device=dev)
    lc = torch.zeros(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rr, r2 = np.ascontiguousarray(prm), np.ascontiguousarray(prm[2])
    N.check(N.lib().cvq_gas_loglik(0, N.JOE, 0, 3, 0.0, N.ptr(rr), len(prm), C.c_void_p(du.data_ptr()), n,
                                   C.c_void_p(out.data_ptr()), N.MEM_DEVICE), "cvq_gas_loglik")
    N.check(N.lib().cvq_gas_path(0, N.JOE, 0, 3, 0.0, N.ptr(r2), C.c_void_p(du.data_ptr()), n,
                                 C.c_void_p(th.data_ptr()), C.c_void_p(lc.data_ptr()), N.MEM_DEVICE), "cvq_gas_path")
    th, lc = th.cpu().numpy(), lc.cpu().numpy()
    assert np.all(np.isnan(out.cpu().numpy()))
    assert np.array_equal(th[:11], want_th[:11]) and np.all(np.isnan(th[11:]))
    assert np.array_equal(lc[:10], want_lc[:10]) and np.all(np.isnan(lc[10:]))
    with pytest.raises(ValueError, match="at row 10"):               # host memory: refused before any device work
        engine.gas_loglik(bad, "joe", prm)


@pytest.mark.parametrize("case", BATCH_CASES, ids=[GC.case_id(c) for c in BATCH_CASES])
def test_device_memory_gives_the_same_bits_as_host_staging(case):
    import torch
    from copula_var import _native as N, engine
    kind, dim, nu = case
    u, (rows, _) = GC.series(case), _batch_rows(case, 65)
    want = engine.gas_loglik(u, kind, rows, nu=nu)
    want_th, want_lc = engine.gas_path(u, kind, rows[0], nu=nu)
    dev = torch.device("cuda:0")
    du = torch.from_numpy(u).to(dev)
    out = torch.full((65,), 7.0, dtype=torch.float64, device=dev)
    th = torch.zeros(u.shape[0] + 1, dtype=torch.float64, device=dev)
    lc = torch.zeros(u.shape[0], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rr = np.ascontiguousarray(rows)
    nuv = 0.0 if nu is None else nu
    N.check(N.lib().cvq_gas_loglik(0, N.COPULA_KIND[kind], 0, dim, nuv, N.ptr(rr), 65, C.c_void_p(du.data_ptr()),
                                   u.shape[0], C.c_void_p(out.data_ptr()), N.MEM_DEVICE), "cvq_gas_loglik")
    r0 = np.ascontiguousarray(rows[0])
    N.check(N.lib().cvq_gas_path(0, N.COPULA_KIND[kind], 0, dim, nuv, N.ptr(r0), C.c_void_p(du.data_ptr()), u.shape[0],
                                 C.c_void_p(th.data_ptr()), C.c_void_p(lc.data_ptr()), N.MEM_DEVICE), "cvq_gas_path")
    assert np.array_equal(out.cpu().numpy(), want, equal_nan=True)
    assert np.array_equal(th.cpu().numpy(), want_th) and np.array_equal(lc.cpu().numpy(), want_lc)
    # a NULL logc_out is allowed
    N.check(N.lib().cvq_gas_path(0, N.COPULA_KIND[kind], 0, dim, nuv, N.ptr(r0), C.c_void_p(du.data_ptr()), u.shape[0],
                                 C.c_void_p(th.data_ptr()), None, N.MEM_DEVICE), "cvq_gas_path")
    assert np.array_equal(th.cpu().numpy(), want_th)


# ------------------------------------------------------------------ hand-over to the per-date solve
STATIC = {"gaussian": [0.3], "student": [4.5, 0.3], "plackett": [3.0], "gumbel": [1.6], "gumbel_survival": [1.6],
          "frank": [3.0], "joe": [1.7], "joe_survival": [1.7]}


@pytest.mark.parametrize("kind", list(STATIC))
def test_dynamic_quantiles_accepts_the_path(kind):
    """garch_student_n64's grid and sigma forecasts, T = 8: the gas_copula_params rows go through
    cvq_dynamic_quantiles' per-date validation for every kind, and the quantiles come back finite."""
    from copula_var.dynamic import gas_copula_params, oos_pits
    from copula_var.engine import QuadraturePlan
    z = load_golden("garch_student_n64")
    T, n_in = 8, int(z["n_in"])
    static = np.array(STATIC[kind])
    rc = z["returns"] - z["returns"][:n_in].mean(axis=0)
    u_oos, _ = oos_pits("garch", z["sigma_forecasts"][:T], None, rc[n_in:n_in + T])
    case = (kind, 2, 6.0 if kind == "student" else None)
    um = GC.series(case)                                             # 48 in-sample rows, edge rows included
    fit = {"omega": GR.link_inverse(kind, static[-1]) * 0.1, "alpha": 0.05, "beta": 0.9}
    path, info = gas_copula_params(kind, um, u_oos, static, fit=fit)
    assert path.shape == (T, static.size) and np.all(np.isfinite(path))
    lo, hi = GR.THETA_RANGE[GR.FAMILY[kind]]
    assert np.all((path[:, -1] >= lo) & (path[:, -1] <= hi)) and len(np.unique(path[:, -1])) == T
    p = QuadraturePlan("garch", kind, 2, z["x_values"], z["step"], z["densities"], z["combos"], z["weights"], static)
    try:
        p.set_dates([z["sigma_forecasts"][:T]])
        var, es, m0 = p.dynamic_quantiles((0.05,), copula_params=path)
        base = p.dynamic_quantiles((0.05,))
    finally:
        p.close()
    assert var.shape == (T, 1) and np.all(np.isfinite(var)) and np.all(np.isfinite(es))
    # the path reached the solve (the quantile itself is a grid level and may coincide; its tail moments do not)
    assert not (np.array_equal(var, base[0]) and np.array_equal(es, base[1]) and np.array_equal(m0, base[2]))


# ------------------------------------------------------------------ optimiser on the device
def test_optimizer_on_the_device_agrees_with_the_cpu_likelihood():
    """The same fit with the device likelihood and with the float64 restatement as `loglik`.

    Tolerance, measured and not guessed: two CPU fits whose likelihoods differ by the LL bar -- the second
    one's loglik is the first's times (1 + 1e-12 sign), sign alternating over the rows of a launch, a
    perturbation of the size the kernel is allowed -- end d_cpu apart in (omega, alpha, beta); the device
    fit must end within 100 d_cpu of the first.  Both figures are printed."""
    from test_gas_cpu import gaussian_static_rho, swinging_gaussian
    from copula_var.optim.copula_fit import GasCopulaOptimizer
    u, _ = swinging_gaussian()
    dens = np.full_like(u, 0.7)
    rho = gaussian_static_rho(u)
    cpu_ll = GR.loglik("gaussian", u)

    def bent(rows):
        ll = cpu_ll(rows)
        return ll * (1.0 + GC.LL_BAR * np.where(np.arange(len(ll)) % 2 == 0, 1.0, -1.0))

    x = lambda r: np.array([r["omega"], r["alpha"], r["beta"]])      # noqa: E731
    a = GasCopulaOptimizer(u, dens, "gaussian", static_theta=rho, loglik=cpu_ll).optimize()
    b = GasCopulaOptimizer(u, dens, "gaussian", static_theta=rho, loglik=bent).optimize()
    d = GasCopulaOptimizer(u, dens, "gaussian", static_theta=rho).optimize()
    d_cpu = float(np.max(np.abs(x(a) - x(b))))
    d_dev = float(np.max(np.abs(x(a) - x(d))))
    print(f"MEASURED optimiser: cpu {x(a)}  device {x(d)}  |device - cpu| {d_dev:.3e}  |cpu - bent cpu| {d_cpu:.3e}  "
          f"nll cpu {a['nll']:.6f} device {d['nll']:.6f} static {d['static_nll']:.6f}  launches {d['launches']}")
    assert d["nll"] < d["static_nll"] - 5.0 and d["launches"] >= 1
    assert d_dev <= 100.0 * d_cpu
    assert abs(d["nll"] - a["nll"]) <= 1e-9 * abs(a["nll"])
