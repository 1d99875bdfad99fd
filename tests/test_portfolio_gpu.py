"""Batched-weights quantiles on the device (cvq_portfolio_quantiles) against the numpy checker
tests/portfolio_reference.py and against single-portfolio plans, through every layer: plan, device
chaining, driver, CLI.  Inputs and checker results: tests/portfolio_cases.py.

The comparison with the checker is tests/test_quantiles_gpu.py's: margin >= 1e-7 asserted first
(tests/test_portfolio_cpu.py holds the figures), then var with np.array_equal, m0 at the slab bar
(rtol 1e-10, atol 1e-15) and |es - ref| <= 3e-10 (|m1 / m0| + |ptf_mean|).  Against a plan built
with the candidate's weights, and between calls, everything is np.array_equal.
What the margin-1e-7 comparison cannot see (1e-8 of relative error in F, the narrow passes) is held by tests/test_quantile_probes_gpu.py."""
import functools

import numpy as np
import pytest

import portfolio_cases as PC
import portfolio_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
ES_RTOL = 3e-10
MARGIN = 1e-7
LEVELS = R.LEVELS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


def _compare(got, ref, ptf):
    """Device (var, es, m0) against the checker's (var, es, m0, margin), each (T, P, L); ptf (P,)."""
    var, es, m0 = got
    rvar, res, rm0, margin = ref
    ptf = np.asarray(ptf, dtype=np.float64)[None, :, None]
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


def _run(name, levels=LEVELS, strategy="auto", **kw):
    """The batch on a plan at the case's own weights."""
    P, w = PC.problem(name)
    p = PC.plan_of(P, strategy)
    try:
        return p.portfolio_quantiles(w, levels, R.means(len(w)), **kw)
    finally:
        p.close()


@functools.lru_cache(maxsize=None)
def _batch(name):
    """The device's result on a case at LEVELS: computed once, shared, read-only."""
    return _run(name)


# ------------------------------------------------------------------ 1. checker parity
@pytest.mark.parametrize("name", list(PC.PARITY))
def test_checker_parity(name):
    _, w = PC.problem(name)
    _compare(_batch(name), PC.reference(name), R.means(len(w)))


# ------------------------------------------------------------------ 2. single-portfolio plans
def _single_plans(P, w, pm, levels=LEVELS):
    """quantiles on a fresh plan per weight vector with its ptf_mean; None where cvq_plan_create
    refuses the vector."""
    out = []
    for wp, m in zip(w, pm):
        try:
            p = PC.plan_of(P, weights=wp)
        except ValueError as e:
            print("plan refused", wp, e)
            out.append(None)
            continue
        try:
            out.append(p.quantiles(levels, float(m)))
        finally:
            p.close()
    return out


@pytest.mark.parametrize("name", ["cfg2_n64", "cfg4_k4_n16"])
def test_bit_identical_to_single_portfolio_plans(name):
    """[:, p, :] is cvq_quantiles on a plan created with weights[p] and ptf_mean[p], bit for bit.
    A vector cvq_plan_create refuses has no such plan: it is held to the checker alone
    (test_checker_parity covers every vector), and at least the plain ones must be accepted."""
    P, w = PC.problem(name)
    got = _batch(name)
    singles = _single_plans(P, w, R.means(len(w)))
    assert sum(s is not None for s in singles) >= 5
    for p, s in enumerate(singles):
        if s is not None:
            assert _same(s, [g[:, p, :] for g in got]), (name, p, w[p])


# ------------------------------------------------------------------ 3. independence
def test_independent_of_the_batch():
    from copula_var import engine
    P, w = PC.problem("cfg2_n64")
    pm = R.means(len(w))
    got = _batch("cfg2_n64")
    p = PC.plan_of(P)
    try:
        for k in (0, 3, 7):                                        # P = 1
            assert _same(p.portfolio_quantiles(w[k:k + 1], LEVELS, pm[k:k + 1]), [g[:, k:k + 1] for g in got])
        assert _same(p.portfolio_quantiles(w[::-1], LEVELS, pm[::-1]), [g[:, ::-1] for g in got])      # reversed
        dup = [0, 3, 3, 1, 3]                                      # a duplicated vector
        assert _same(p.portfolio_quantiles(w[dup], LEVELS, pm[dup]), [g[:, dup] for g in got])
        again = p.portfolio_quantiles(w, LEVELS, pm)               # two runs
        assert _same(again, got)
        for l in range(len(LEVELS)):                               # L = 1 against L = 3
            assert _same(p.portfolio_quantiles(w, LEVELS[l:l + 1], pm), [g[:, :, l:l + 1] for g in got])
        # 70 vectors: two calls (64 + 6) inside portfolio_quantiles
        idx = np.arange(70) % len(w)
        assert p._portfolio_step(len(LEVELS)) == 64
        assert _same(p.portfolio_quantiles(w[idx], LEVELS, pm[idx]), [g[:, idx] for g in got])
        # and with the scratch budget below a 64-candidate call's need: 32 + 32 + 6
        budget = engine.PORTFOLIO_SCRATCH_BUDGET
        engine.PORTFOLIO_SCRATCH_BUDGET = p.portfolio_scratch(32, len(LEVELS))
        try:
            assert p.portfolio_scratch(64, len(LEVELS)) > engine.PORTFOLIO_SCRATCH_BUDGET
            assert p._portfolio_step(len(LEVELS)) == 32
            assert _same(p.portfolio_quantiles(w[idx], LEVELS, pm[idx]), [g[:, idx] for g in got])
        finally:
            engine.PORTFOLIO_SCRATCH_BUDGET = budget
        p.set_dates((P.fbs[:1], P.pi[:1]))                         # T = 1 against the batch's first date
        assert _same(p.portfolio_quantiles(w, LEVELS, pm), [g[:1] for g in got])
        p.set_dates((P.fbs[2:5], P.pi[2:5]))                       # the other dates
        assert _same(p.portfolio_quantiles(w, LEVELS, pm), [g[2:5] for g in got])
    finally:
        p.close()


def test_scalar_ptf_mean_and_the_plans_own_weights():
    """A scalar ptf_mean serves every candidate; the plan's own weights in the batch reproduce
    quantiles."""
    P, w = PC.problem("cfg2_n64")
    p = PC.plan_of(P)
    try:
        got = p.portfolio_quantiles(np.vstack((w[3], P.w)), LEVELS, 0.25)
        assert _same(p.quantiles(LEVELS, 0.25), [g[:, 1, :] for g in got])
    finally:
        p.close()


# ------------------------------------------------------------------ 4. chunk and wave edges
@pytest.mark.parametrize("name", list(PC.EDGES))
def test_chunk_and_wave_edges(name):
    """2-D n = 70: 2 chunks of 64 rows, the second with 6 live rows; n = 130 (Plackett): 3 chunks,
    the last with 2 rows; 3-D n = 17: 289 rows, a second 256-row chunk of 33."""
    P, w = PC.problem(name)
    got = _batch(name)
    _compare(got, PC.reference(name), R.means(len(w)))
    assert not np.isnan(got[0]).any()


def test_tile_with_empty_last_slots():
    """The 3-D opening pass serves two portfolios per workgroup: P = 1, 2, 3, 5, 6 (and a batch
    from an odd offset) leave a tile's last slot empty or not, each against the single-portfolio
    plans' results on the shape with a partial last chunk."""
    P, w = PC.problem("3d_n17")
    pm = R.means(len(w))
    singles = _single_plans(P, w, pm)
    assert all(s is not None for s in singles)
    p = PC.plan_of(P)
    try:
        for sl in (slice(0, 1), slice(0, 2), slice(0, 3), slice(0, 5), slice(0, 6), slice(1, 4)):
            got = p.portfolio_quantiles(w[sl], LEVELS, pm[sl])
            for k, s in enumerate(singles[sl]):
                assert _same(s, [g[:, k, :] for g in got]), (sl, k)
        p.enable_timing(("quantiles",))               # timed under kind 6
        p.portfolio_quantiles(w, LEVELS, pm)
        ms, launches = p.kernel_time("quantiles")
        assert launches >= 1 and ms > 0.0
    finally:
        p.close()


# ------------------------------------------------------------------ 5. every strategy
@pytest.mark.parametrize("strategy", ["compact", "sorted", "sweep", "direct", "prefix"])
def test_every_strategy(strategy):
    import es_reference as E
    z = load_golden("cfg2_n64")
    P, w = E.problem_of(z), R.W2                      # every date of the golden: calc_var couples them (Q2/Q4)
    p = PC.plan_of(P, strategy)
    try:
        assert p.strategy == strategy
        got = p.portfolio_quantiles(w, LEVELS, R.means(len(w)))
        assert p._wide is None                        # no sibling: the plan itself, whatever v_cap
        var, _ = p.calc_var(float(z["ptf_mean"]))     # the solve state is intact
        assert np.array_equal(var, z["var"])
    finally:
        p.close()
    T = PC.problem("cfg2_n64")[0].T                   # identical across strategies (and date batches)
    assert _same([g[:T] for g in got], _batch("cfg2_n64"))


# ------------------------------------------------------------------ 6. Gumbel
def test_survival_gumbel():
    _, w = PC.problem("gumbel")
    _compare(_batch("gumbel"), PC.reference("gumbel"), R.means(len(w)))


# ------------------------------------------------------------------ 7. outside the bracket
def test_level_outside_the_bracket():
    """msm_plackett_n64 at 0.2: NaN and finite dates mixed across the candidates; the NaN pattern
    and m0 = F(max_var) are the checker's."""
    _, w = PC.problem("outside")
    got = _run("outside", (0.05, PC.OUTSIDE_LEVEL))
    _compare(got, PC.reference("outside"), R.means(len(w)))
    nan = np.isnan(got[0][:, :, 1])
    assert nan.any() and not nan.all() and nan.any(axis=0).sum() >= 2 and (~nan).any(axis=0).sum() >= 2
    assert np.all(got[2][:, :, 1][nan] < PC.OUTSIDE_LEVEL) and not np.isnan(got[0][:, :, 0]).any()


# ------------------------------------------------------------------ 8. device chain
def test_device_chain_on_a_torch_stream():
    import torch
    from copula_var import engine
    P, w = PC.problem("cfg2_n64")
    pm = R.means(len(w))
    host = _batch("cfg2_n64")
    p = PC.plan_of(P)
    try:
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        args = engine.solve_args(float("nan"))        # args.ptf_mean is not read
        shape = (P.T, len(w), len(LEVELS))
        with torch.cuda.stream(stream):
            out = torch.empty((3,) + shape, dtype=torch.float64, device=dev)
            only = torch.empty(shape, dtype=torch.float64, device=dev)
            rev = torch.empty((3,) + shape, dtype=torch.float64, device=dev)
            p.set_stream(stream.cuda_stream)
            p.portfolio_quantiles_device(args, w, pm, LEVELS, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
            p.portfolio_quantiles_device(args, w, pm, LEVELS, only.data_ptr())        # es / m0 not asked for
            # no host synchronisation before the next call: it rewrites the weight records the
            # calls above read, in stream order
            p.portfolio_quantiles_device(args, w[::-1].copy(), pm[::-1].copy(), LEVELS, rev[0].data_ptr(),
                                         rev[1].data_ptr(), rev[2].data_ptr())
        stream.synchronize()
        for k in range(3):
            assert np.array_equal(out[k].cpu().numpy(), host[k])
            assert np.array_equal(rev[k].cpu().numpy(), host[k][:, ::-1])
        assert np.array_equal(only.cpu().numpy(), host[0])
    finally:
        p.close()


def test_weights_validated():
    """The two checks that read the plan's dim: a non-finite weight, weights[p][0] <= 0."""
    P, w = PC.problem("cfg2_n64")
    p = PC.plan_of(P)
    try:
        for bad in (float("nan"), float("inf")):
            ww = w.copy()
            ww[5, 1] = bad
            with pytest.raises(ValueError, match="finite"):
                p.portfolio_quantiles(ww, LEVELS)
        for bad in (0.0, -0.5):
            ww = w.copy()
            ww[2, 0] = bad
            with pytest.raises(ValueError, match="> 0"):
                p.portfolio_quantiles(ww, LEVELS)
        with pytest.raises(ValueError, match="shape"):
            p.portfolio_quantiles(R.W3, LEVELS)
        with pytest.raises(ValueError, match="ptf_mean"):
            p.portfolio_quantiles(w, LEVELS, np.full(len(w), np.nan))
    finally:
        p.close()


# ------------------------------------------------------------------ 9. driver and CLI
def _driver(z):
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    tickers, start, kw = inject(z)
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=str(z["copula"]),
                                                               estimation_type=str(z["model"]))
    return ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=int(z["num_points"]),
                                  weights=z["weights"], copula_params=z["copula_params"], **kw)


@pytest.mark.parametrize("case,cand", [("cfg2_n64", R.W2), ("cfg4_k4_n16", R.W3)])
def test_driver_calc_portfolio_quantiles(case, cand):
    from copula_var.portfolios import min_es
    z = load_golden(case)
    v = _driver(z)
    try:
        w = np.vstack((cand, z["weights"]))                        # the constructor's own weights last
        var, es = v.calc_portfolio_quantiles(w, LEVELS)
        m0 = v.last_tail_mass
        qvar, qes = v.calc_quantiles(LEVELS)
        qm0 = v.last_tail_mass
        one, _ = v.calc_portfolio_quantiles(w[:2])
        means = np.array([v.mean_returns[t] for t in v.tickers])
    finally:
        v.close()
    T = qvar.shape[0]
    assert var.shape == es.shape == m0.shape == (T, len(w), len(LEVELS))
    assert np.array_equal(var[:, -1], qvar) and np.array_equal(es[:, -1], qes) and np.array_equal(m0[:, -1], qm0)
    assert one.shape == (T, 2, 1) and np.array_equal(one[:, :, 0], var[:, :2, 2])
    # ptf_mean[p] as the loader forms the constructor's: var - ptf_mean is the same solve at any mean
    P = PC.problem(case)[0]
    ref = R.portfolio_quantiles(P, w[:3], LEVELS, [np.sum(means * wp) for wp in w[:3]])
    _compare([a[:P.T, :3] for a in (var, es, m0)], ref, [np.sum(means * wp) for wp in w[:3]])
    idx, best = min_es(es)
    assert np.array_equal(best, np.nanmax(es, axis=1))


def test_cli_weight_grid(tmp_path, capsys, monkeypatch):
    import pandas as pd
    from copula_var import main as M, synthetic
    from copula_var.portfolios import min_es, weight_lattice
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from driver_util import inject
    z = load_golden("garch_student_n64")
    tickers, start, _ = inject(z)                                  # fitted GARCH parameters from the cache
    csv, out = tmp_path / "returns.csv", tmp_path / "var.csv"
    synthetic.returns_frame(z["returns"]).to_csv(csv)
    seen = []                                                      # the driver call the CLI makes
    inner = ValueAtRiskCalcualtion.calc_portfolio_quantiles

    def record(self, weights, levels=(0.05,)):
        r = inner(self, weights, levels)
        seen.append((np.array(weights), tuple(levels), r[1]))
        return r

    monkeypatch.setattr(ValueAtRiskCalcualtion, "calc_portfolio_quantiles", record)
    # the golden's copula parameters instead of the IFM fit (seconds, and not this test's subject)
    monkeypatch.setattr(ValueAtRiskCalcualtion, "calc_copula_params", lambda self: z["copula_params"])
    rc = M.main(["--prices", str(csv), "--returns", "--tickers", *tickers, "--start", start, "--n-in",
                 str(int(z["n_in"])), "--copula", "student", "--estimation", "garch", "--num-points", "64",
                 "--weight-grid", "4", "--exact-levels", "0.025", "0.05", "--out", str(out)])
    assert rc == 0
    err = capsys.readouterr().err
    assert err.count("candidate") == 4 and "mean ES" in err
    (cand, levels, es), = seen
    assert np.array_equal(cand, weight_lattice(2, 4)) and levels == (0.025, 0.05)
    assert es.shape[1:] == (4, 2) and not np.isnan(es).all()
    idx, best = min_es(es)
    f = pd.read_csv(out, index_col=0, float_precision="round_trip")
    assert len(f) == es.shape[0]
    for i, lv in enumerate(("0.025", "0.05")):
        cols = [f"wbest_garch_{t}_{lv}" for t in tickers] + [f"wbest_es_garch_{lv}"]
        assert all(c in f.columns for c in cols), list(f.columns)
        # wbest_es is the maximum of the per-candidate ES; the weights are that candidate's, per
        # ticker through the Q10 axis mapping (ticker 0 carries weights[1], the last weights[0])
        assert np.array_equal(f[cols[-1]].to_numpy(), np.nanmax(es[:, :, i], axis=1))
        assert np.array_equal(f[cols[-1]].to_numpy(), best[:, i])
        assert np.array_equal(f[cols[0]].to_numpy(), cand[idx[:, i], 1])
        assert np.array_equal(f[cols[1]].to_numpy(), cand[idx[:, i], 0])
