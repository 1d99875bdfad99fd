"""The predictive distribution on the device (cvq_distribution) against the numpy checker
tests/distribution_reference.py, through every layer: plan, device chaining, backtest, driver.

Tolerances are the project's slab bar (tests/test_tail_moments_gpu.py): mass rtol 1e-10,
atol 1e-15; m1 |got - ref| <= 1e-10 * m1_abs + 1e-15 (for a one-signed bin the same rtol); a
ratio of two masses (PIT, CDF) rtol 3e-10, as ES_RTOL.  A sum of bins against one slab: 2e-10
(each side at the 1e-10 bar)."""
import functools
import os
import re

import numpy as np
import pytest

import archimedean_reference as A
import distribution_reference as D
import es_reference as E
import gumbel_reference as G
from conftest import GOLDEN, GOLDEN_CASES, load_golden

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
RATIO_RTOL = 3e-10
SMALL = [c for c in GOLDEN_CASES if c not in ("cfg2_n256", "cfg3_n128")]
INF = float("inf")
LADDER = np.array([-100.0, -7.5, -3.0, -2.0, -1.0, 0.0, 0.5, 2.0, INF])
STRATEGIES = ["compact", "sorted", "sweep", "direct", "prefix"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@functools.lru_cache(maxsize=None)
def _ref(case):
    """(golden arrays, oracle Problem, bin_moments of LADDER): computed once per case."""
    z = load_golden(case)
    P = E.problem_of(z)
    return z, P, D.bin_moments(P, LADDER)


def _plan_of(P, strategy="auto", sl=slice(None)):
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w, P.copula_params,
                       vol_states=P.uvs if P.model == "msm" else None, strategy=strategy)
    p.set_dates((P.fbs[sl], P.pi[sl]) if P.model == "msm" else [P.sigma[sl]])
    return p


def _check(got, ref, what=""):
    """Device (mass, m1) against the checker's (m0, m1, m1_abs) at the slab bar."""
    m0, m1, m1a = ref
    print(what, "mass rel", np.max(np.abs(got[0] - m0) / np.maximum(np.abs(m0), 1e-300)),
          "m1 rel", np.max(np.abs(got[1] - m1) / np.maximum(m1a, 1e-300)))
    assert got[0].shape == m0.shape and got[1].shape == m1.shape
    np.testing.assert_allclose(got[0], m0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    assert np.all(np.abs(got[1] - m1) <= 1e-10 * m1a + 1e-15)


def _check_total(p, P, got):
    """The bins of LADDER tile (-100, +inf]: their sum is that slab's tail moments."""
    b = np.tile((-100.0, INF), (P.T, 1))
    t0, t1 = p.tail_moments(b)
    m1a = E.tail_moments(P, b)[2]
    print("sum of bins rel", np.max(np.abs(got[0].sum(axis=1) - t0) / t0))
    np.testing.assert_allclose(got[0].sum(axis=1), t0, rtol=2e-10, atol=SLAB_ATOL)
    assert np.all(np.abs(got[1].sum(axis=1) - t1) <= 2e-10 * m1a + 1e-15)


# ------------------------------------------------------------------ 1. every small golden
@pytest.mark.parametrize("case", SMALL)
def test_small_goldens(case):
    z, P, ref = _ref(case)
    p = _plan_of(P)
    try:
        assert p.T == P.T
        got = p.distribution(LADDER)
        _check(got, ref, case)
        _check_total(p, P, got)
    finally:
        p.close()
    assert np.all(ref[0][:, 2:6] > 0.0)              # the ladder's inner bins hold mass: the test sees nodes


# ------------------------------------------------------------------ 2. Gumbel and product-form instances
@pytest.mark.parametrize("case,kind,theta", [("cfg2_n64", "gumbel_survival", 2.0), ("cfg5_n64", "frank", 6.0),
                                             ("cfg4_k4_n16", "joe_survival", 2.0)])
def test_log_b_kinds(case, kind, theta):
    z = load_golden(case)
    sl = slice(0, 6 if int(z["dim"]) == 2 else 4)
    P = (G if kind.startswith("gumbel") else A).problem_of(z, kind, theta, sl)
    p = _plan_of(P)
    try:
        assert p.strategy == "sorted"
        got = p.distribution(LADDER)
        _check(got, D.bin_moments(P, LADDER), kind)
        _check_total(p, P, got)
    finally:
        p.close()


# ------------------------------------------------------------------ 3. geometry
def _fullbatch_problem(cfg, n, T=6):
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


def test_2d_n80_partial_chunk():
    """80 rows: one full chunk of 64 and one of 16 (rows do not fill the last chunk)."""
    z, P = _fullbatch_problem(2, 80, T=4)
    p = _plan_of(P)
    try:
        got = p.distribution(LADDER)
        _check(got, D.bin_moments(P, LADDER), "n80")
        _check_total(p, P, got)
    finally:
        p.close()


@pytest.mark.parametrize("copula,params", [("student", [5.0, 0.5, 0.4, 0.3]), ("gaussian", [0.5, 0.4, 0.3])])
def test_3d_garch_n18(copula, params):
    """324 rows: one full chunk of 256 and one of 68 (a partial chunk and a partial wave).  Then
    the first date alone: bit-identical to the batch's first row."""
    from oracle import forecast as F
    from oracle.quadrature import Problem
    z = load_golden("garch3d_student_n16")
    n, T = 18, 3
    x, step = F.x_grid(n, "garch")
    sig = z["sigma_forecasts"][:T]
    P = Problem("garch", copula, 3, x, step, np.ones((3, 1, n)), np.zeros((1, 3)), z["weights"], np.array(params),
                sig)
    p = _plan_of(P)
    try:
        got = p.distribution(LADDER)
        _check(got, D.bin_moments(P, LADDER), copula)
        _check_total(p, P, got)
        p.set_dates([sig[:1]])
        one = p.distribution(LADDER)
        assert np.array_equal(one[0], got[0][:1]) and np.array_equal(one[1], got[1][:1])
    finally:
        p.close()


# ------------------------------------------------------------------ 4. per-date edges
def test_per_date_edges():
    z, P, _ = _ref("cfg2_n64")
    nan = float("nan")
    edges = LADDER[None, :] + 0.013 * np.arange(P.T)[:, None]       # a different ladder on each date
    edges[1, 3] = nan                                               # a NaN edge: bins 2 and 3 empty
    edges[2, 3], edges[2, 4] = -1.0, -2.0                           # a descending pair: bin 3 empty
    edges[3, 5] = edges[3, 4]                                       # a repeated edge: bin 4 empty
    edges[4, 0], edges[4, 1] = -INF, -3.2                           # -inf as the first edge
    edges[5] = [0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 4.5, INF]       # every bin wholly above 0
    edges[6] = [INF, -INF, -2.0, -2.0, nan, 0.0, INF, INF, -INF]    # (inf, -inf] and (inf, inf]: empty
    ref = D.bin_moments(P, edges)
    p = _plan_of(P)
    try:
        got = p.distribution(edges)
        again = p.distribution(edges[:, :3])                        # two bins per date: the PIT's shape
    finally:
        p.close()
    _check(got, ref, "per-date")
    for t, b in ((1, 2), (1, 3), (2, 3), (3, 4), (6, 0), (6, 2), (6, 3), (6, 4), (6, 6), (6, 7)):
        assert got[0][t, b] == 0.0 and got[1][t, b] == 0.0, (t, b)  # exactly (0, 0)
        assert ref[0][t, b] == 0.0
    assert np.all(got[0][5] > 0.0) and np.all(got[1][5] > 0.0)
    assert got[0][6, 1] > 0.0 and got[0][6, 5] > 0.0                # (-inf, -2] and (0, inf]
    assert got[0][4, 0] > 0.0                                       # (-inf, -3.2]
    assert np.array_equal(again[0], got[0][:, :2]) and np.array_equal(again[1], got[1][:, :2])


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("case", ["cfg2_n64", "cfg4_k4_n16"])
def test_bins_and_dates_are_independent(case):
    z, P, _ = _ref(case)
    ladder = np.concatenate(([-100.0], np.linspace(-6.0, 3.0, 63), [INF]))      # 64 ascending bins
    order = np.random.default_rng(5).permutation(64)
    p = _plan_of(P)
    try:
        full = p.distribution(ladder)
        again = p.distribution(ladder)
        singles = [p.distribution(ladder[b:b + 2]) for b in range(64)]
        # the same bins in a permuted order: two 64-bin calls whose even bins are 32 of the ladder's
        # bins each, in the permutation's order (the odd bins in between run from one member's upper
        # edge to the next one's lower edge: descending or overlapping, whatever comes)
        scattered = []
        for sel in (order[:32], order[32:]):
            pairs = np.empty(65)
            pairs[0:64:2], pairs[1:64:2], pairs[64] = ladder[sel], ladder[sel + 1], INF
            scattered.append(p.distribution(pairs))
        lo = 1 if P.T == 4 else 5
        sl = slice(lo, lo + 3)
        p.set_dates((P.fbs[sl], P.pi[sl]))
        part = p.distribution(ladder)
    finally:
        p.close()
    _check(full, D.bin_moments(P, ladder), case)
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])          # two runs
    for b in range(64):                                                                    # 64 one-bin calls
        assert np.array_equal(singles[b][0][:, 0], full[0][:, b]), b
        assert np.array_equal(singles[b][1][:, 0], full[1][:, b]), b
    for got, sel in zip(scattered, (order[:32], order[32:])):                              # permuted order
        assert np.array_equal(got[0][:, 0:64:2], full[0][:, sel])
        assert np.array_equal(got[1][:, 0:64:2], full[1][:, sel])
    assert np.array_equal(part[0], full[0][sl]) and np.array_equal(part[1], full[1][sl])   # a 3-date slice


# ------------------------------------------------------------------ 6. every strategy
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_every_strategy(strategy):
    z, P, ref = _ref("cfg2_n64")
    p = _plan_of(P, strategy)
    try:
        assert p.strategy == strategy
        got = p.distribution(LADDER)                  # reaches +inf: no v_cap limit, the plan itself
        assert p._wide is None
        var, _ = p.calc_var(float(z["ptf_mean"]))     # the call left the solve state intact
        later = p.distribution(LADDER)
    finally:
        p.close()
    _check(got, ref, strategy)
    assert np.array_equal(var, z["var"])
    assert np.array_equal(later[0], got[0]) and np.array_equal(later[1], got[1])


# ------------------------------------------------------------------ 7. device mode
def test_device_mode_chained_behind_solve():
    import torch
    from copula_var import engine
    z, P, ref = _ref("cfg2_n64")
    ptf = float(z["ptf_mean"])
    B = LADDER.size - 1
    per = LADDER[None, :] - 0.02 * np.arange(P.T)[:, None]
    p = _plan_of(P)
    try:
        host = p.distribution(LADDER)
        host_per = p.distribution(per)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        args = engine.solve_args(ptf)
        with torch.cuda.stream(stream):
            var = torch.empty(P.T, dtype=torch.float64, device=dev)
            mass, m1, mass_only, pmass, pm1 = (torch.full((P.T, B), -1.0, dtype=torch.float64, device=dev)
                                               for _ in range(5))
            d_edges = torch.tensor(per, dtype=torch.float64, device=dev)
            p.set_stream(stream.cuda_stream)
            p.solve_device(args, var.data_ptr(), check=False)
            p.distribution_device(LADDER, B, mass.data_ptr(), m1.data_ptr())
            p.distribution_device(LADDER, B, mass_only.data_ptr())             # m1_out NULL
            p.distribution_device(d_edges.data_ptr(), B, pmass.data_ptr(), pm1.data_ptr())
        stream.synchronize()
        with pytest.raises(ValueError):
            p.distribution_device(LADDER[:-1], B, mass.data_ptr())
    finally:
        p.close()
    _check(host, ref, "host")
    assert np.array_equal(var.cpu().numpy(), z["var"])
    assert np.array_equal(mass.cpu().numpy(), host[0]) and np.array_equal(m1.cpu().numpy(), host[1])
    assert np.array_equal(mass_only.cpu().numpy(), host[0])
    assert np.array_equal(pmass.cpu().numpy(), host_per[0]) and np.array_equal(pm1.cpu().numpy(), host_per[1])


def test_timed_under_tail_moments():
    z, P, _ = _ref("cfg2_n64")
    p = _plan_of(P)
    try:
        p.enable_timing(("moments",))
        p.distribution(LADDER)
        ms, launches = p.kernel_time("moments")
    finally:
        p.close()
    assert launches == 1 and ms > 0.0


# ------------------------------------------------------------------ 8. PIT and predictive CDF
def _realised(z, T):
    n_in = int(z["n_in"])
    return z["returns"][n_in:n_in + T].mean(axis=1)


@pytest.mark.parametrize("case", ["cfg2_n64", "cfg1"])
def test_pit_and_predictive_cdf(case):
    from copula_var import backtest as B
    z, P, _ = _ref(case)
    ptf = float(z["ptf_mean"])
    r = _realised(z, P.T)
    assert r.shape == (P.T,)
    shifts = (-1.0, -0.4, 0.0, 0.4, 1.0)
    th = np.array([-3.0, -2.0, -1.0, 0.0, 1.0])
    p = _plan_of(P)
    try:
        us = [B.pit(p, r + s, ptf) for s in shifts]
        rn = r.copy()
        rn[2] = np.nan
        un = B.pit(p, rn, ptf)
        F, total = B.predictive_cdf(p, th, ptf)
    finally:
        p.close()
    ref = D.pit(P, r, ptf)
    print("pit rel", np.max(np.abs(us[2] - ref) / ref), "range", us[2].min(), us[2].max())
    np.testing.assert_allclose(us[2], ref, rtol=RATIO_RTOL, atol=0.0)
    np.testing.assert_allclose(us[0], D.pit(P, r - 1.0, ptf), rtol=RATIO_RTOL, atol=0.0)
    for u in us:
        assert np.all((u >= 0.0) & (u <= 1.0))
    assert np.all(np.diff(np.array(us), axis=0) >= 0.0)           # non-decreasing in the realised return
    assert 0.0 < us[2].min() and us[2].max() < 1.0 and np.ptp(us[2]) > 0.1
    assert np.isnan(un[2]) and np.array_equal(np.delete(un, 2), np.delete(us[2], 2))
    m0 = D.bin_moments(P, np.concatenate(([-100.0], th - ptf, [INF])))[0]
    tot = m0.sum(axis=1)
    print("cdf rel", np.max(np.abs(F - np.cumsum(m0[:, :-1], axis=1) / tot[:, None]) / F))
    np.testing.assert_allclose(F, np.cumsum(m0[:, :-1], axis=1) / tot[:, None], rtol=RATIO_RTOL, atol=0.0)
    np.testing.assert_allclose(total, tot, rtol=2e-10, atol=0.0)
    assert np.all(F[:, -1] <= 1.0) and np.all(np.diff(F, axis=1) >= 0.0) and np.all(F[:, 0] >= 0.0)


# ------------------------------------------------------------------ 9. driver
def test_cli_backtest(tmp_path, capsys, monkeypatch):
    import pandas as pd
    from copula_var import main as M, synthetic
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    z = load_golden("garch_student_n64")
    tickers, start, kw = inject(z)                                 # fitted GARCH parameters from the cache
    csv, out, plain = tmp_path / "returns.csv", tmp_path / "bt.csv", tmp_path / "plain.csv"
    synthetic.returns_frame(z["returns"]).to_csv(csv)
    # the golden's copula parameters instead of the static IFM fit (seconds, and not this test's subject)
    monkeypatch.setattr(ValueAtRiskCalcualtion, "calc_copula_params", lambda self: z["copula_params"])
    base = ["--prices", str(csv), "--returns", "--tickers", *tickers, "--start", start, "--n-in",
            str(int(z["n_in"])), "--copula", "student", "--estimation", "garch", "--num-points", "64", "--es",
            "--exact-levels", "0.05", "0.25"]
    assert M.main(base + ["--backtest", "--out", str(out)]) == 0
    err = capsys.readouterr().err
    assert M.main(base + ["--out", str(plain)]) == 0
    assert "backtest" not in capsys.readouterr().err
    f = pd.read_csv(out, index_col=0, float_precision="round_trip")
    realised, var = f["portfolio_return"].to_numpy(), f["var_garch"].to_numpy()
    tables = re.findall(r"backtest garch/student (.*?): alpha ([0-9.]+), (\d+) dates \((\d+) dropped\), hits (\d+) ", err)
    assert [t[0] for t in tables] == ["VaR", "exact VaR at 0.05", "exact VaR at 0.25"]
    assert int(tables[0][4]) == int(np.sum(realised < var)) and int(tables[0][2]) == len(f)
    for t, col in zip(tables[1:], ("qvar_garch_0.05", "qvar_garch_0.25")):
        assert int(t[4]) == int(np.sum(realised < f[col].to_numpy())) and float(t[1]) == float(col.split("_")[-1])
    assert int(tables[2][4]) >= int(tables[1][4])                  # more hits at the wider level
    for name in ("Kupiec", "Christoffersen", "pinball", "Z2", "Berkowitz"):
        assert err.count(name) == 3, name
    assert np.array_equal(f["hit_garch"].to_numpy(), (realised < var).astype(float))
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type="student", estimation_type="garch")
    v = ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=64, weights=z["weights"], **kw)
    try:
        u = v.calc_pit(realised)
        table = v.backtest(realised, 0.05, var=var)
        mass, m1 = v.calc_distribution([-100.0 + v.ptf_mean, -2.0, np.inf])
        b = np.tile((-100.0, -2.0 - v.ptf_mean), (len(f), 1))
        t0, t1 = v.plan.tail_moments(b)
    finally:
        v.close()
    assert np.array_equal(f["pit_garch"].to_numpy(), u) and np.all((u > 0.0) & (u < 1.0))
    assert table["hits"] == int(tables[0][4]) and "z2" not in table and table["berkowitz"]["n"] == len(f)
    np.testing.assert_allclose(mass[:, 0], t0, rtol=2e-10, atol=0.0)
    np.testing.assert_allclose(m1[:, 0], t1, rtol=2e-10, atol=0.0)
    # without the flag: the columns of before, byte for byte
    g = pd.read_csv(plain, index_col=0, float_precision="round_trip")
    assert list(g.columns) == ["var_garch", "garch_es", "qvar_garch_0.05", "qes_garch_0.05", "qvar_garch_0.25",
                               "qes_garch_0.25", "portfolio_return"]
    assert list(f.columns) == list(g.columns)[:-1] + ["pit_garch", "hit_garch", "portfolio_return"]
    lines_bt, lines_plain = open(out).read().splitlines(), open(plain).read().splitlines()
    keep = [0] + [1 + list(f.columns).index(c) for c in g.columns]
    assert [",".join(np.array(l.split(","))[keep]) for l in lines_bt] == lines_plain
