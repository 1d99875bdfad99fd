"""Per-date-record quantiles on the device (cvq_dynamic_quantiles) against plans built per date
(the definition), against the numpy checker tests/dynamic_reference.py, and through every layer:
plan, device mode, driver, CLI.  Inputs and checker results: tests/dynamic_cases.py.

The comparison with the checker is tests/test_portfolio_gpu.py's: margin >= 1e-7 asserted first
(tests/test_dynamic_cpu.py holds the figures), then var with np.array_equal, m0 at the slab bar
(rtol 1e-10, atol 1e-15) and |es - ref| <= 3e-10 (|m1 / m0| + |ptf_mean|).  Against a plan built
with the date's parameters and weights, and between calls, everything is np.array_equal.
What the margin-1e-7 comparison cannot see (1e-8 of relative error in F, the narrow passes) is held by tests/test_quantile_probes_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import dynamic_cases as DC
import dynamic_reference as R
import portfolio_cases as PC
from conftest import load_golden

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
ES_RTOL = 3e-10
MARGIN = 1e-7
LEVELS = R.LEVELS
ALL = list(DC.CASES) + list(DC.EDGES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


def _compare(got, ref, ptf):
    """Device (var, es, m0) against the checker's (var, es, m0, margin), each (T, L); ptf (T,)."""
    var, es, m0 = got
    rvar, res, rm0, margin = ref
    ptf = np.asarray(ptf, dtype=np.float64)[:, None]
    bar = ES_RTOL * (np.abs(res - ptf) + np.abs(ptf))
    print("margin", margin.min(), "m0 rel", np.max(np.abs(m0 - rm0) / np.maximum(np.abs(rm0), 1e-300)),
          "es err / bar", np.nanmax(np.abs(es - res) / bar, initial=0.0))
    assert var.shape == rvar.shape and es.shape == res.shape and m0.shape == rm0.shape
    assert margin.min() >= MARGIN                     # the premise of the exact comparison
    assert np.array_equal(np.isnan(var), np.isnan(rvar)) and np.array_equal(np.isnan(es), np.isnan(res))
    assert np.array_equal(var, rvar, equal_nan=True)
    np.testing.assert_allclose(m0, rm0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    ok = ~np.isnan(res)
    assert np.all(np.abs(es - res)[ok] <= bar[ok])


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _sel(res, idx):
    return [np.ascontiguousarray(a[idx]) for a in res]


@functools.lru_cache(maxsize=None)
def _batch(name):
    """The device's result on a case at its levels: computed once, shared, read-only."""
    P, cp, w, pm, _ = DC.problem(name)
    p = DC.plan_of(P)
    try:
        return p.dynamic_quantiles(DC.levels(name), cp, w, pm)
    finally:
        p.close()


# ------------------------------------------------------------------ 1. per-date plans
@pytest.mark.parametrize("name", ALL)
def test_bit_identical_to_per_date_plans(name):
    """[t] is cvq_quantiles on a fresh plan built with date t's parameters and weights, fed date t
    alone, at ptf_mean_t[t], bit for bit (var, es and m0)."""
    _, _, _, pm, dates = DC.problem(name)
    got = _batch(name)
    assert DC.reference(name)[3].min() >= MARGIN
    for t, Pt in enumerate(dates):
        p = DC.plan_of(Pt)
        try:
            one = p.quantiles(DC.levels(name), float(pm[t]))
        finally:
            p.close()
        assert _same(one, [g[t:t + 1] for g in got]), (name, t)


# ------------------------------------------------------------------ 2. checker parity
@pytest.mark.parametrize("name", list(DC.CASES))
def test_checker_parity(name):
    _compare(_batch(name), DC.reference(name), DC.problem(name)[3])
    assert not np.isnan(_batch(name)[0]).any()


# ------------------------------------------------------------------ 3. degenerate forms
@pytest.mark.parametrize("name", ["cfg2_n64", "msm_plackett_n64", "cfg5_n64_gumbel", "cfg4_k4_n16"])
def test_degenerate_forms(name):
    P, cp, w, pm, _ = DC.problem(name)
    p = DC.plan_of(P)
    try:
        plain = p.quantiles(LEVELS, 0.25)
        assert _same(p.dynamic_quantiles(LEVELS, ptf_mean=0.25), plain)             # all three None
        own = np.tile(np.asarray(P.copula_params, dtype=np.float64).reshape(-1), (P.T, 1))
        assert _same(p.dynamic_quantiles(LEVELS, own, None, 0.25), plain)           # the plan's own parameters
        assert _same(p.dynamic_quantiles(LEVELS, own, np.tile(P.w, (P.T, 1)), np.full(P.T, 0.25)), plain)
        got = p.dynamic_quantiles(LEVELS, None, w, pm)                              # weights only
        port = p.portfolio_quantiles(w, LEVELS, pm)
        t = np.arange(P.T)
        assert _same(got, [a[t, t, :] for a in port])
    finally:
        p.close()


# ------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("name", ["cfg2_n64", "garch3d_student_n16"])
def test_independent_of_the_batch(name):
    z = load_golden(DC.CASES[name][0])
    P, cp, w, pm, _ = DC.problem(name)
    got = _batch(name)
    p = DC.plan_of(P)

    def dates(idx):
        p.set_dates((P.fbs[idx], P.pi[idx]) if P.model == "msm" else [P.sigma[idx]])

    try:
        before, _ = p.calc_var(float(z["ptf_mean"]))                # the solve on these dates
        assert _same(p.dynamic_quantiles(LEVELS, cp, w, pm), got)   # two runs
        for l in range(len(LEVELS)):                                # L = 1 against L = 3
            assert _same(p.dynamic_quantiles(LEVELS[l:l + 1], cp, w, pm), [g[:, l:l + 1] for g in got])
        after, _ = p.calc_var(float(z["ptf_mean"]))                 # the solve state is intact
        assert np.array_equal(before, after, equal_nan=True)
        perm = np.roll(np.arange(P.T)[::-1], 1)                     # the dates with their records, permuted
        dates(perm)
        assert _same(p.dynamic_quantiles(LEVELS, cp[perm], w[perm], pm[perm]), _sel(got, perm))
        for t in (0, P.T - 1, 2):                                   # T = 1
            dates(slice(t, t + 1))
            assert _same(p.dynamic_quantiles(LEVELS, cp[t:t + 1], w[t:t + 1], pm[t:t + 1]), _sel(got, slice(t, t + 1)))
        p.enable_timing(("quantiles",))                             # timed under kind 6
        p.dynamic_quantiles(LEVELS, cp[t:t + 1], w[t:t + 1], pm[t:t + 1])
        ms, launches = p.kernel_time("quantiles")
        assert launches >= 1 and ms > 0.0
    finally:
        p.close()


@pytest.mark.parametrize("strategy", ["compact", "sorted", "sweep", "direct", "prefix"])
def test_every_strategy(strategy):
    P, cp, w, pm, _ = DC.problem("cfg2_n64")
    p = DC.plan_of(P, strategy)
    try:
        assert p.strategy == strategy
        assert _same(p.dynamic_quantiles(LEVELS, cp, w, pm), _batch("cfg2_n64"))
        assert p._wide is None                        # no sibling: the plan itself, whatever v_cap
    finally:
        p.close()


# ------------------------------------------------------------------ 5. chunk and wave edges
@pytest.mark.parametrize("name", list(DC.EDGES))
def test_chunk_and_wave_edges(name):
    """2-D n = 70: 2 chunks of 64 rows, the second with 6 live rows; n = 130 (Plackett): 3 chunks,
    the last with 2 rows; 3-D n = 17: 289 rows, a second 256-row chunk of 33."""
    got = _batch(name)
    _compare(got, DC.reference(name), DC.problem(name)[3])
    assert not np.isnan(got[0]).any()


# ------------------------------------------------------------------ 6. validation
SENTINEL = -12345.0


def _refused(p, T, code, text, t=None, *, cp=None, w=None, pm=None, levels=LEVELS, **consts):
    """One refused call: its status, its message (with the offending date) and untouched outputs."""
    from copula_var import _native as N
    from copula_var import engine
    args = engine.solve_args(0.0, **consts)
    lv = N.f64(levels)
    out = [np.full((T, max(lv.size, 1)), SENTINEL) for _ in range(3)]
    arr = [None if a is None else N.f64(a) for a in (cp, w, pm)]
    rc = N.lib().cvq_dynamic_quantiles(p._h if p is not None else None, C.byref(args),
                                       *[N.ptr(a) if a is not None else None for a in arr], N.ptr(lv), lv.size,
                                       N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]), N.MEM_HOST)
    msg = (N.lib().cvq_last_error() or b"").decode()
    print(rc, msg)
    assert rc == code and text in msg, (rc, msg)
    if t is not None:
        assert msg.endswith(f"at date {t}"), msg
    assert all(np.all(o == SENTINEL) for o in out)


def test_validation_student():
    from copula_var import _native as N
    P, cp, w, pm, _ = DC.problem("cfg2_n64")
    T, inv, uns = P.T, N.CVQ_ERR_INVALID, N.CVQ_ERR_UNSUPPORTED
    p = DC.plan_of(P)
    try:
        def mod(a, t, k, v):
            b = np.array(a, dtype=np.float64)
            b[t, k] = v
            return b

        for bad in (float("nan"), float("inf")):
            _refused(p, T, inv, "finite", 3, cp=mod(cp, 3, 1, bad), w=w, pm=pm)
            _refused(p, T, inv, "finite", 4, cp=cp, w=mod(w, 4, 1, bad), pm=pm)
            _refused(p, T, inv, "finite", 5, cp=cp, w=w, pm=mod(pm[:, None], 5, 0, bad)[:, 0])
        _refused(p, T, inv, "correlation", 2, cp=mod(cp, 2, 1, 1.0))
        _refused(p, T, inv, "correlation", 1, cp=mod(mod(cp, 1, 1, -1.5), 4, 1, 2.0))   # the first offender
        _refused(p, T, inv, "nu", 0, cp=mod(cp, 0, 0, 0.0))
        _refused(p, T, inv, "nu", 3, cp=mod(cp, 3, 0, -2.0))
        _refused(p, T, uns, "nu", 5, cp=mod(cp, 5, 0, cp[5, 0] + 0.5))                  # not the plan's nu
        for bad in (0.0, -0.5):
            _refused(p, T, uns, "> 0", 2, w=mod(w, 2, 0, bad))
        # a bad record and a bad weight on different dates: the earlier date is named
        _refused(p, T, uns, "> 0", 1, cp=mod(cp, 4, 1, 1.0), w=mod(w, 1, 0, 0.0))
        # the checks that read no per-date value
        for L in (0, 9):
            _refused(p, T, inv, "n_levels", levels=[0.05] * L)
        for bad in (0.0, -1.0, float("nan")):
            _refused(p, T, inv, "level", levels=[0.05, bad])
        _refused(p, T, inv, "max_var", min_var=0.0, max_var=0.0)
        _refused(p, T, uns, "62", tolerance=1e-300)
        _refused(None, T, inv, "NULL")
        from copula_var import engine
        a = engine.solve_args(0.0)
        lv, out = N.f64(LEVELS), np.full((T, 3), SENTINEL)
        for args, levels, var in ((None, N.ptr(lv), N.ptr(out)), (C.byref(a), None, N.ptr(out)),
                                  (C.byref(a), N.ptr(lv), None)):
            assert N.lib().cvq_dynamic_quantiles(p._h, args, None, None, None, levels, 3, var, None, None,
                                                 N.MEM_HOST) == inv
            assert b"NULL" in N.lib().cvq_last_error() and np.all(out == SENTINEL)
        # the engine's own shape checks, and the library's message through ValueError
        with pytest.raises(ValueError, match="shape"):
            p.dynamic_quantiles(LEVELS, cp[:-1])
        with pytest.raises(ValueError, match="shape"):
            p.dynamic_quantiles(LEVELS, None, R.W3)
        with pytest.raises(ValueError, match="at date 2"):
            p.dynamic_quantiles(LEVELS, mod(cp, 2, 1, 1.0))
        assert _same(p.dynamic_quantiles(LEVELS, cp, w, pm), _batch("cfg2_n64"))        # and the plan still works
    finally:
        p.close()


def test_validation_other_kinds():
    from copula_var import _native as N
    from copula_var.engine import QuadraturePlan
    inv, uns = N.CVQ_ERR_INVALID, N.CVQ_ERR_UNSUPPORTED
    P, cp, w, pm, _ = DC.problem("cfg5_n64_gumbel")
    p = DC.plan_of(P)
    try:
        th = cp.copy()
        th[3, 0] = 0.99
        _refused(p, P.T, inv, "theta", 3, cp=th)
        th[2, 0] = 16.5
        _refused(p, P.T, uns, "theta", 2, cp=th)
        th[1, 0] = float("nan")
        _refused(p, P.T, inv, "finite", 1, cp=th)
    finally:
        p.close()
    P, cp, w, pm, _ = DC.problem("cfg4_k4_n16")                     # 3-D Gaussian
    p = DC.plan_of(P)
    try:
        bad = cp.copy()
        bad[2] = (0.9, -0.9, 0.9)                                    # every |rho| < 1, not positive definite
        _refused(p, P.T, inv, "positive definite", 2, cp=bad)
        bad[1] = (0.2, 1.0, 0.2)
        _refused(p, P.T, inv, "correlation", 1, cp=bad)
    finally:
        p.close()
    # before cvq_set_dates
    p = QuadraturePlan(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w, P.copula_params,
                       vol_states=P.uvs)
    try:
        _refused(p, P.T, N.CVQ_ERR_STATE, "cvq_set_dates")
        b = C.c_int64()
        assert N.lib().cvq_dynamic_scratch(p._h, 3, C.byref(b)) == N.CVQ_ERR_STATE
    finally:
        p.close()


# ------------------------------------------------------------------ 7. device mode
def test_device_mode_on_a_torch_stream():
    import torch
    from copula_var import engine
    P, cp, w, pm, _ = DC.problem("cfg2_n64")
    host = _batch("cfg2_n64")
    p = DC.plan_of(P)
    try:
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        args = engine.solve_args(0.25)
        shape = (P.T, len(LEVELS))
        with torch.cuda.stream(stream):
            out = torch.empty((3,) + shape, dtype=torch.float64, device=dev)
            only = torch.empty(shape, dtype=torch.float64, device=dev)
            rev = torch.empty((3,) + shape, dtype=torch.float64, device=dev)
            plain = torch.empty((3,) + shape, dtype=torch.float64, device=dev)
            p.set_stream(stream.cuda_stream)
            p.dynamic_quantiles_device(args, LEVELS, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                       copula_params=cp.copy(), weights=w.copy(), ptf_mean=pm.copy())
            p.dynamic_quantiles_device(args, LEVELS, only.data_ptr(), copula_params=cp, weights=w, ptf_mean=pm)
            # no host synchronisation before the next calls: their records go through other staging
            # buffers (or the same, once its upload is done) and overwrite the device records in
            # stream order; the host arrays of the calls above are gone by now
            p.dynamic_quantiles_device(args, LEVELS, rev[0].data_ptr(), rev[1].data_ptr(), rev[2].data_ptr(),
                                       copula_params=cp[::-1].copy(), weights=w.copy(), ptf_mean=pm.copy())
            p.dynamic_quantiles_device(args, LEVELS, plain[0].data_ptr(), plain[1].data_ptr(), plain[2].data_ptr())
        stream.synchronize()
        want_rev = p.dynamic_quantiles(LEVELS, cp[::-1].copy(), w, pm)
        want_plain = p.quantiles(LEVELS, 0.25)                     # all three None: args.ptf_mean
        for k in range(3):
            assert np.array_equal(out[k].cpu().numpy(), host[k])
            assert np.array_equal(rev[k].cpu().numpy(), want_rev[k])
            assert np.array_equal(plain[k].cpu().numpy(), want_plain[k])
        assert np.array_equal(only.cpu().numpy(), host[0])
        # scratch grows with T and L
        s61, s63 = p.dynamic_scratch(1), p.dynamic_scratch(3)
        p.set_dates((P.fbs[:3], P.pi[:3]))
        s33 = p.dynamic_scratch(3)
        assert 0 < s61 < s63 and 0 < s33 < s63 and s63 == 2 * s33
        with pytest.raises(ValueError, match="n_levels"):
            p.dynamic_scratch(9)
    finally:
        p.close()


# ------------------------------------------------------------------ 8. driver and CLI
def _driver(z):
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    tickers, start, kw = inject(z)
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=str(z["copula"]),
                                                               estimation_type=str(z["model"]))
    return ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=int(z["num_points"]),
                                  weights=z["weights"], copula_params=z["copula_params"], **kw)


def test_driver_calc_dynamic_quantiles():
    z = load_golden("cfg2_n64")
    P, cp, w, _, dates = DC.problem("cfg2_n64")
    v = _driver(z)
    try:
        T = v.plan.T
        cpt, wt = np.tile(z["copula_params"], (T, 1)), np.tile(z["weights"], (T, 1))
        cpt[:P.T], wt[:P.T] = cp, w
        var, es = v.calc_dynamic_quantiles(LEVELS, copula_params=cpt, weights=wt)
        m0 = v.last_tail_mass
        qvar, qes = v.calc_quantiles(LEVELS)
        same = v.calc_dynamic_quantiles(LEVELS)
        means = np.array([v.mean_returns[t] for t in v.tickers])
    finally:
        v.close()
    assert var.shape == es.shape == m0.shape == (T, len(LEVELS))
    assert np.array_equal(same[0], qvar, equal_nan=True) and np.array_equal(same[1], qes, equal_nan=True)
    assert np.array_equal(var[P.T:], qvar[P.T:], equal_nan=True)   # the untouched dates
    pm = np.array([np.sum(means * wp) for wp in w])                # the loader's formula per date
    _compare([a[:P.T] for a in (var, es, m0)], R.dynamic_quantiles(dates, LEVELS, pm), pm)


def test_cli_rolling_copula_and_drift_weights(tmp_path, capsys, monkeypatch):
    import pandas as pd
    from copula_var import main as M, synthetic
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from driver_util import inject
    z = load_golden("garch_student_n64")
    tickers, start, _ = inject(z)                                  # fitted GARCH parameters from the cache
    csv, out = tmp_path / "returns.csv", tmp_path / "var.csv"
    synthetic.returns_frame(z["returns"]).to_csv(csv)
    seen = []                                                      # the driver call the CLI makes
    inner = ValueAtRiskCalcualtion.calc_dynamic_quantiles

    def record(self, levels=(0.05,), copula_params=None, weights=None):
        r = inner(self, levels, copula_params, weights)
        seen.append((tuple(levels), np.array(copula_params), np.array(weights), r, self.plan, self.mean_returns))
        again = self.plan.dynamic_quantiles(levels, copula_params, weights, self.dynamic_ptf_mean(weights))
        seen.append(again)
        return r

    monkeypatch.setattr(ValueAtRiskCalcualtion, "calc_dynamic_quantiles", record)
    # the golden's copula parameters instead of the static IFM fit (seconds, and not this test's subject)
    monkeypatch.setattr(ValueAtRiskCalcualtion, "calc_copula_params", lambda self: z["copula_params"])
    T = len(z["returns"]) - int(z["n_in"])
    rc = M.main(["--prices", str(csv), "--returns", "--tickers", *tickers, "--start", start, "--n-in",
                 str(int(z["n_in"])), "--copula", "student", "--estimation", "garch", "--num-points", "64",
                 "--rolling-copula", "60", "--refit-every", str(max(T // 2, 1)), "--drift-weights",
                 "--exact-levels", "0.025", "0.05", "--out", str(out)])
    assert rc == 0
    (levels, cpt, wt, (var, es), _, _), again = seen
    assert levels == (0.025, 0.05) and cpt.shape == (var.shape[0], 2) and wt.shape == (var.shape[0], 2)
    assert np.all(cpt[:, 0] == z["copula_params"][0])              # the plan's nu on every date
    assert len(np.unique(cpt[:, 1])) == 2                          # two refits, held in between
    assert np.allclose(wt.sum(axis=1), 1.0) and np.array_equal(wt[0], z["weights"]) and len(np.unique(wt[:, 0])) > 1
    f = pd.read_csv(out, index_col=0, float_precision="round_trip")
    assert len(f) == var.shape[0]
    for i, lv in enumerate(("0.025", "0.05")):
        assert np.array_equal(f[f"dvar_garch_{lv}"].to_numpy(), again[0][:, i], equal_nan=True)
        assert np.array_equal(f[f"des_garch_{lv}"].to_numpy(), again[1][:, i], equal_nan=True)
        assert np.array_equal(f[f"dvar_garch_{lv}"].to_numpy(), var[:, i], equal_nan=True)
    for k in range(2):
        assert np.array_equal(f[f"dparam_garch_{k}"].to_numpy(), cpt[:, k])
    assert "rolling copula" in capsys.readouterr().err
