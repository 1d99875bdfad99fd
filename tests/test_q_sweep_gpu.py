"""Every MSM kernel family at every number of unique volatility states per asset, q = 1 ... 8, against the
longdouble / mpmath truths of tests/golden/q_sweep.kat -- the sibling of test_node_slabs_gpu.py and
test_node_ext_gpu.py, whose tier table and bars it shares.  The ten families are compiled once per q and
selected by a host `switch (S.q)` (case 1 ... 7, default = 8); COMPACT's and the quadrature core's node loops
pad the states above q up to kQUnroll = 8.  No mpmath, no reference module and no reference project here:
q_sweep_cases.py, node_cases.py and the fixture only.

Cases (q_sweep_cases.cases(), 95, MSM throughout; 2-D n = 24, 3-D n = 12, T = 3 dates, node_cases' slabs):
Student nu = 6, Gaussian, survival Gumbel theta = 4, Frank theta = 6, survival Joe theta = 2 in 2-D and 3-D and
Plackett theta = 1.5 in 2-D at every q; the fitted Student nu = 5.364 at q = 4 and 8; dates whose pi_t is not
rank 1 at q = 8.  Per case every strategy that accepts the shape runs (the only refusals: the 2-D-only
strategies in 3-D, and every strategy but SORTED for the Gumbel and product-form kinds), and on every plan:

  a  compute_integral on the four slabs                       k_direct (DIRECT, COMPACT), k_mass (PREFIX), SORTED, SWEEP
  b  tail_moments, axis_moments, quantiles' m0 of one level   k_moments, k_attrib, k_quant_pass
     no slab reaches; dynamic_quantiles the same way with     k_dyn_pass
     NULL records and with the alternative middle date
  c  distribution on the ladder q_sweep_cases.LADDER (bins    k_dist_pass, k_dyn_dist_pass
     0, 1, 3, 5 are the slabs: mass and m1; the descending
     bin exactly (0, 0)); dynamic_distribution with NULL
     records (array_equal) and with the alternative date
  d  conditional_quantiles' m0 and p_event on axis 0's        k_cond_pass, k_port_pass
     stress event; portfolio_quantiles' m0 for the plan's
     own weights (= quantiles' m0 bit for bit) and for
     node_cases.PORT_UNEQUAL
  e  calc_var (Student nu = 6 and Gaussian): the oracle's     every strategy's solve kernel
     VaR and iteration count, np.array_equal

(e) is the weak check: at these sizes the VaR sits on a grid step, so it mainly proves that every q's solve
instance launches and agrees; its premise (decisions unchanged under a 1 +- 1e-7 scaling of every integral, and
no level whose F is a rounding residue of a true 0: hence q_sweep_cases.OBJ_VAR[3] = 1.0) is asserted in
tests/test_q_sweep_cpu.py.  The numerically strong checks are (a) to (d).

Bars, all from the project, none from a run:
  Student, Gaussian, Plackett   test_node_slabs_gpu.bar_of(family, ...) with its TIERS: families prefix, direct,
                                sorted, moments, cond, port, and dist and dyn (the precise tier)
  survival Gumbel               node_cases.gumbel_bar of the fixture's ebound arrays (test_node_ext_gpu.py's recipe):
                                SORTED's record path fast, everything else precise
  Frank, survival Joe           the project's stated slab bar, 1e-10 * scale + 1e-15 (SLAB_RTOL / SLAB_ATOL of
                                tests/test_archimedean_gpu.py; DESIGN's 4e-11 exp2_node7 class on the fast
                                path); no tighter product-form bar has been derived
The date under the alternative parameters is held to the same bar as the plan's own dates.

Measured on one MI355X, worst |device - ref| in units of the bar over q = 1 ... 8 and both dimensions, with the
q and dimension at which it occurs (the `MEASURED` lines of a run, kept per (family, kind, q, dim) in
profiles/q_sweep/measured.txt).  prefix ... sweep: that strategy's compute_integral; moments, attrib, quantile:
tail_moments, axis_moments, quantiles' m0; dyn / dyn-alt: dynamic_quantiles' m0 with NULL records / with the
alternative date; dist: distribution; dyndist-alt: dynamic_distribution on the alternative date; cond, port:
conditional_quantiles, portfolio_quantiles:

  family      student          student-fitted   gaussian         plackett         gumbel_survival  frank            joe_survival
  prefix      0.003 (q8 3d)    0.016 (q8 3d)    0.002 (q1 3d)    0.000 (q8 2d)    -                -                -
  direct      0.034 (q7 2d)    0.036 (q4 2d)    0.002 (q1 2d)    0.000 (q8 2d)    -                -                -
  compact     0.034 (q7 2d)    0.036 (q4 2d)    0.002 (q1 2d)    0.000 (q8 2d)    -                -                -
  sorted      0.003 (q8 3d)    0.853 (q8 2d)    0.965 (q6 2d)    0.000 (q8 2d)    0.953 (q6 2d)    0.392 (q1 2d)    0.399 (q2 2d)
  sweep       0.002 (q5 2d)    0.853 (q8 2d)    0.965 (q6 2d)    0.000 (q8 2d)    -                -                -
  moments     0.035 (q7 2d)    0.036 (q4 2d)    0.002 (q1 3d)    0.001 (q5 2d)    0.018 (q8 2d)    0.000 (q8 3d)    0.000 (q8 3d)
  attrib      0.036 (q7 2d)    0.037 (q4 2d)    0.002 (q1 3d)    0.001 (q8 2d)    0.018 (q8 2d)    0.000 (q8 3d)    0.000 (q8 3d)
  quantile    0.035 (q7 2d)    0.036 (q4 2d)    0.002 (q1 3d)    0.000 (q8 2d)    0.018 (q8 2d)    0.000 (q8 3d)    0.000 (q8 3d)
  dyn         0.035 (q7 2d)    0.036 (q4 2d)    0.002 (q1 3d)    0.000 (q8 2d)    0.018 (q8 2d)    0.000 (q8 3d)    0.000 (q8 3d)
  dyn-alt     0.035 (q7 2d)    0.036 (q4 2d)    0.002 (q1 3d)    0.000 (q8 2d)    0.018 (q8 2d)    0.000 (q8 3d)    0.000 (q8 3d)
  dist        0.035 (q7 2d)    0.036 (q4 2d)    0.002 (q1 3d)    0.001 (q5 2d)    0.018 (q8 2d)    0.000 (q8 3d)    0.000 (q8 3d)
  dyndist-alt 0.034 (q3 3d)    0.020 (q8 3d)    0.002 (q1 2d)    0.000 (q8 2d)    0.013 (q7 3d)    0.000 (q8 3d)    0.000 (q8 3d)
  cond        0.035 (q7 2d)    0.036 (q4 2d)    0.002 (q7 2d)    0.000 (q8 2d)    0.022 (q8 2d)    0.000 (q8 3d)    0.000 (q8 3d)
  port        0.042 (q2 3d)    0.040 (q4 3d)    0.002 (q8 3d)    0.000 (q8 2d)    0.018 (q8 2d)    0.000 (q8 3d)    0.000 (q8 3d)

The families above one half are the fast tier's: exp2_node7's own 4.045e-11 of the 4.05e-11 in the bar, as at q = 3
(test_node_slabs_gpu.py's header).  Every precise-tier family stays under 0.05 of its bar at every q.
"""
import collections

import numpy as np
import pytest

import node_cases as NC
import q_sweep_cases as QC
from test_node_slabs_gpu import FAMILY, REFUSAL, STRATEGIES, TIERS, _plan, bar_of

pytestmark = pytest.mark.gpu

CASES = QC.cases()
# cvq_plan_create (cvq_plan.hip): "the Gumbel copulas run on the SORTED strategy (CVQ_STRATEGY_SORTED) only", "the
# Frank copula runs on ..." and "the Joe copulas run on ..."
SORTED_REFUSAL = "on the SORTED strategy (CVQ_STRATEGY_SORTED) only"
SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15       # tests/test_archimedean_gpu.py: the product-form kinds' bar
NO_LEVEL = [1.0e6]                        # a level no slab reaches: var is NaN and m0 = F(max_var)
LADDER = np.array(QC.LADDER)

MEASURED = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@pytest.fixture(scope="module")
def z():
    return QC.load_kat()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(MEASURED):
        print("MEASURED %-12s %-24s q%d %dd max %.3f of bar" % (key + (MEASURED[key],)))


def _hold(label, key, dev, ref, scale, bar, extra=0.0):
    """|dev - ref| <= bar * scale + extra everywhere (bar: a number or an array of dev's shape); the worst
    ratio is recorded under key (test_node_ext_gpu.py's)."""
    dev, ref, scale = np.asarray(dev), np.asarray(ref), np.asarray(scale)
    assert dev.shape == ref.shape == scale.shape, (label, dev.shape, ref.shape, scale.shape)
    assert np.all(np.isfinite(dev)), (label, dev)
    err, tol = np.abs(dev - ref), np.asarray(bar) * scale + extra
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.max(np.where(tol > 0.0, err / tol, np.where(err == 0.0, 0.0, np.inf))))
    MEASURED[key] = max(MEASURED[key], ratio)
    assert ratio <= 1.0, f"{label}: |device - ref| = {ratio:.3f} of the bar {np.max(bar):.3e} * scale"


def kind_of(case):
    copula, _, params = case[:3]
    return "student-fitted" if copula == "student" and params[0] != np.floor(params[0]) else copula


def bar_for(case, family, ebound=None):
    """(bar, absolute extra) of `family` on a case; ebound: the fixture's bound for the sums in question
    (the Gumbel kind's bars are per case, slab and date)."""
    copula, dim, params, _, variant = case
    if copula in QC.PRODUCT_KINDS:
        return SLAB_RTOL, SLAB_ATOL
    if copula in QC.GUMBEL_KINDS:
        fam = family if family != "sorted" or variant != "nr1" else "sorted-generic"
        tier = TIERS[(fam, "gumbel", False)]
        # rank-1 dates take SORTED's record path (node_fast), the others node_value; every row core: node_value
        assert tier == ("fast" if fam == "sorted" else "precise")
        return NC.gumbel_bar(ebound, tier), 0.0
    return bar_of(family, copula, dim, params)[0], 0.0


def _expected(case):
    if case[0] in QC.SORTED_ONLY:
        return ["sorted"]
    return list(STRATEGIES) if case[1] == 2 else ["prefix", "sorted"]


def _run_plan(z, i, p, strategy):
    case = CASES[i]
    copula, dim, params, q, variant = case
    T, slabs, kind = QC.T, NC.slabs(dim), kind_of(case)
    gumbel = copula in QC.GUMBEL_KINDS
    n = NC.N_OF[dim]
    cp, w = QC.records(case)
    own = np.array([t for t in range(T) if t != QC.ALT_DATE])
    axis, (lo, hi) = QC.stress_event(p._x)
    W = np.array([np.full(dim, 1.0 / dim), NC.PORT_UNEQUAL[dim]])
    key = lambda fam: (fam, kind, q, dim)
    eb = lambda name, idx: z[name][idx] if gumbel else None
    cid = QC.case_id(case)

    def spliced(plain, alt):
        """(T,) rows: the plan's own truth on dates 0 and 2, the alternative's on the middle date."""
        out = np.array(plain, dtype=np.float64, copy=True)
        out[QC.ALT_DATE] = alt
        return out

    for s, (a, b) in enumerate(slabs):
        bounds = np.tile((a, b), (T, 1))
        tag = f"{cid} {strategy} slab ({a}, {b}]"
        m0r, sc = z["m0"][i, s], z["scale"][i, s]
        # ---- a: the strategy's own slab
        fam_s = strategy if gumbel or copula in QC.PRODUCT_KINDS else FAMILY[strategy]
        fast = gumbel and variant != "nr1"
        bar, atol = bar_for(case, fam_s, eb("ebound_fast" if fast else "ebound", (i, s)))
        # PREFIX: a difference of running row sums (test_node_slabs_gpu.py)
        extra = 2 * n * 2.0 ** -53 * z["scale_below"][i, s] if strategy == "prefix" else 0.0
        _hold(tag + " compute_integral", key(strategy), p.compute_integral(bounds), m0r, sc, bar, atol + extra)
        # ---- b: the row cores
        bar_m, atol = bar_for(case, "moments", eb("ebound", (i, s)))
        bar_1 = bar_for(case, "moments", eb("ebound1", (i, s)))[0]
        bar_x = bar_for(case, "moments", z["eboundx"][i, s][:, :dim] if gumbel else None)[0]
        m0, m1 = p.tail_moments(bounds)
        _hold(tag + " tail_moments m0", key("moments"), m0, m0r, sc, bar_m, atol)
        _hold(tag + " tail_moments m1", key("moments"), m1, z["m1"][i, s], z["scale1"][i, s], bar_1, atol)
        a0, mx = p.axis_moments(bounds)
        _hold(tag + " axis_moments m0", key("attrib"), a0, m0r, sc, bar_m, atol)
        _hold(tag + " axis_moments mx", key("attrib"), mx, z["mx"][i, s][:, :dim], z["scalex"][i, s][:, :dim], bar_x, atol)
        probe = dict(min_var=(max(a, -7.5) + b) / 2, max_var=b, lower=a)
        var, _, q0 = p.quantiles(NO_LEVEL, **probe)
        assert np.all(np.isnan(var))
        _hold(tag + " quantiles m0", key("quantile"), q0[:, 0], m0r, sc, bar_m, atol)
        bar_d, atol = bar_for(case, "dyn", eb("ebound", (i, s)))
        var, _, d0 = p.dynamic_quantiles(NO_LEVEL, **probe)
        assert np.all(np.isnan(var))
        _hold(tag + " dynamic_quantiles m0, NULL records", key("dyn"), d0[:, 0], m0r, sc, bar_d, atol)
        var, _, d1 = p.dynamic_quantiles(NO_LEVEL, cp, w, **probe)
        assert np.all(np.isnan(var))
        bar_a = spliced(np.broadcast_to(bar_d, (T,)), bar_for(case, "dyn", eb("alt_ebound", (i, s)))[0])
        _hold(tag + " dynamic_quantiles m0, alternative middle date", key("dyn-alt"), d1[:, 0],
              spliced(m0r, z["alt_m0"][i, s]), spliced(sc, z["alt_scale"][i, s]), bar_a, atol)
        # ---- d: the conditional and batched-weights passes
        bar_c, atol = bar_for(case, "cond", eb("ebound_event", (i, s)))
        covar, _, c0, pe = p.conditional_quantiles(axis, np.tile((lo, hi), (T, 1)), NO_LEVEL, **probe)
        assert np.all(np.isnan(covar))
        _hold(tag + " stress event m0", key("cond"), c0[:, 0], z["m0_event"][i, s], z["scale_event"][i, s], bar_c,
              atol + NC.MIN_NORMAL)
        if s == 0:                                              # lower = -100: the event over the whole box
            _hold(tag + " stress event p_event", key("cond"), pe, z["p_event"][i], z["scale_pevent"][i],
                  bar_for(case, "cond", eb("ebound_pevent", (i,)))[0], atol + NC.MIN_NORMAL)
        bar_p, atol = bar_for(case, "port", eb("ebound_port", (i, s)))
        var, _, p0 = p.portfolio_quantiles(W, NO_LEVEL, **probe)
        assert np.all(np.isnan(var)) and p0.shape == (T, 2, 1)
        assert np.array_equal(p0[:, 0, :], q0), f"{tag}: candidate 0 is the plan's own weight vector"
        _hold(tag + " candidate m0", key("port"), p0[:, 1, 0], z["m0_port"][i, s], z["scale_port"][i, s], bar_p,
              atol + NC.MIN_NORMAL)
    # ---- c: the distribution passes, one call each
    mass, m1 = p.distribution(LADDER)
    dn = p.dynamic_distribution(LADDER)
    da = p.dynamic_distribution(LADDER, cp, w)
    tag = f"{cid} {strategy} ladder"
    assert mass.shape == m1.shape == (T, LADDER.size - 1)
    for s, bn in enumerate(QC.BIN_OF_SLAB):       # the truths first: a wrong kernel is named by its own numbers
        tag = f"{cid} {strategy} ladder bin {bn}"
        bar_m, atol = bar_for(case, "dist", eb("ebound", (i, s)))
        bar_1 = bar_for(case, "dist", eb("ebound1", (i, s)))[0]
        _hold(tag + " distribution mass", key("dist"), mass[:, bn], z["m0"][i, s], z["scale"][i, s], bar_m, atol)
        _hold(tag + " distribution m1", key("dist"), m1[:, bn], z["m1"][i, s], z["scale1"][i, s], bar_1, atol)
        t = QC.ALT_DATE
        bar_m = bar_for(case, "dist", eb("alt_ebound", (i, s)))[0]
        bar_1 = bar_for(case, "dist", eb("alt_ebound1", (i, s)))[0]
        _hold(tag + " dynamic_distribution mass, alternative date", key("dyndist-alt"), da[0][t, bn], z["alt_m0"][i, s],
              z["alt_scale"][i, s], bar_m, atol)
        _hold(tag + " dynamic_distribution m1, alternative date", key("dyndist-alt"), da[1][t, bn], z["alt_m1"][i, s],
              z["alt_scale1"][i, s], bar_1, atol)
    tag = f"{cid} {strategy} ladder"
    assert np.array_equal(dn[0], mass) and np.array_equal(dn[1], m1), tag + ": NULL records are the static call"
    assert np.array_equal(da[0][own], mass[own]) and np.array_equal(da[1][own], m1[own]), \
        tag + ": the dates that keep the plan's values"
    for res in (mass, m1, da[0], da[1]):
        assert np.all(res[:, QC.DESCENDING_BIN] == 0.0), tag + ": a descending bin is exactly (0, 0)"
        assert np.all(np.isfinite(res[:, QC.FREE_BIN]))
    # ---- e: the solve
    if QC.solve_case(case):
        var, it = p.calc_var(0.0, obj_var=QC.OBJ_VAR[dim])
        assert it == int(z["solve_it"][i]) and it > 0, (cid, strategy, it, int(z["solve_it"][i]))
        assert np.array_equal(var, z["solve_var"][i], equal_nan=True), (cid, strategy, var, z["solve_var"][i])
    else:
        assert int(z["solve_it"][i]) == -1


@pytest.mark.parametrize("i", range(len(CASES)), ids=[QC.case_id(c) for c in CASES])
def test_q_sweep_against_reference(z, i):
    case = CASES[i]
    copula, dim, params, q, variant = case
    kw = QC.problem_inputs(case, z)
    assert kw["densities"].shape[1] == q and kw["combos"].shape == (q ** dim, dim)
    ran = []
    for strategy in STRATEGIES:
        try:
            p = _plan(kw, "msm", strategy)
        except ValueError as err:
            documented = [REFUSAL[strategy]] if dim == 3 and strategy in REFUSAL else []
            if copula in QC.SORTED_ONLY and strategy != "sorted":
                documented.append(SORTED_REFUSAL)
            assert any(m in str(err) for m in documented), (strategy, str(err))
            continue
        ran.append(strategy)
        try:
            assert p.strategy == strategy and p._static.q == q
            _run_plan(z, i, p, strategy)
        finally:
            p.close()
    assert ran == _expected(case)


def test_q_sweep_tiers():
    """Every bar this module applies exists and sits where the header says."""
    for case in CASES:
        copula, dim, params = case[:3]
        if copula in QC.PRODUCT_KINDS:
            assert bar_for(case, "sorted") == (SLAB_RTOL, SLAB_ATOL) == (1e-10, 1e-15)
        elif copula in QC.GUMBEL_KINDS:
            for fam in ("moments", "dyn", "dist", "cond", "port"):
                assert TIERS[(fam, "gumbel", False)] == "precise"
            assert bar_for(case, "sorted", 0.0)[0] == (1e-12 if case[4] == "nr1" else 1e-12 + NC.EXP7_BAR)
        else:
            for fam in ("dyn", "dist", "cond", "port"):
                assert bar_of(fam, copula, dim, params) == bar_of("moments", copula, dim, params)
                assert bar_of(fam, copula, dim, params)[1] == "precise"
            for fam in ("prefix", "direct", "sorted"):
                assert 1e-12 <= bar_of(fam, copula, dim, params)[0] < 1e-10
    assert not QC.missing_q(CASES)
