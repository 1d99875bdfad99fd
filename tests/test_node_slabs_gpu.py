"""Slab sums of every strategy and of the three moment kernels against the longdouble / mpmath
reference (tests/node_reference.py) stored in tests/golden/node_kat.kat -- not against the float64
oracle, whose own error (scipy's stdtrit, up to 7.6e-11 of sum |mass| at these cases) is what the
1e-10 oracle-parity bar elsewhere has to cover.  No mpmath and no reference project here.

Shapes: 2-D n = 24, 3-D n = 12, T = 3 dates, the slabs (-100, -3], (-3, -2], (-0.5, 0] and the narrow
(-2.55, -2.5] (2 to 4 nodes); the case matrix is tests/node_cases.py's (82 cases: GARCH and MSM for
every copula parameter, UKF once).  Per case and strategy that accepts the shape:

  compute_integral (cvq_slab)            m0                |device - ref| <= bar * sum |mass|
  tail_moments (cvq_slab_moments)        m0, m1            m1: bar * sum |level * mass|
  axis_moments (cvq_slab_axis_moments)   m0, mx[c]         mx: bar * sum |x_c * mass|
  quantiles (cvq_quantiles)              m0 of one level above F(max_var): m0 = F(max_var) = the slab

Bars, from what the code documents for the instance (TIERS below), never from a run:
  precise tier  1e-12 + (2 nu + 3) 7e-14 for Student (first order in the documented quantile
                accuracy), 1e-12 for Gaussian and Plackett
  fast tier     the precise bar + 4.05e-11 (exp2_node7's own polynomial error, 4.045e-11:
                tests/test_node_reference_cpu.py) + |node_ex| 5e-13 (log_node_fast, Student)
  PREFIX        a slab is a difference of two running row sums, so its bar also carries 2 n 2^-53 of
                sum |mass| over everything at or below the slab's upper bound (CPU-derived: n sequential
                additions per prefix).  Against the slab's own sum |mass| alone it is off by up to 2e-2
                on the narrow slab of the near-singular 3-D Gaussian: by design, and harmless to F(v).

Measured on one MI355X, worst |device - ref| in units of the bar (the `MEASURED` lines of a run):

  kernels                    Student integer nu   Student fitted nu    Gaussian         Plackett
  PREFIX slab                0.026                0.033                0.059            0.023
  DIRECT / COMPACT slab      0.434                0.301                0.060            0.023
  SORTED slab                0.090                0.924 (fast)         0.962 (fast)     0.081
  SWEEP slab                 0.039                0.924 (fast)         0.958 (fast)     0.081
  moments / attribution /
  quantile row cores         0.435                0.290                0.127            0.027
"""
import collections

import numpy as np
import pytest

import node_cases as NC

pytestmark = pytest.mark.gpu

CASES = NC.cases()
STRATEGIES = ("prefix", "direct", "compact", "sorted", "sweep")
# cvq_plan_create (cvq_plan.hip): "the SWEEP strategy is built for dim == 2", "the DIRECT and COMPACT
# strategies are built for dim == 2"; nothing else may refuse these shapes
REFUSAL = {"direct": "built for dim == 2", "compact": "built for dim == 2", "sweep": "built for dim == 2"}
QUANTILE_BAR, EXP7_BAR, LOGFAST_ABS = 7e-14, 4.05e-11, 5e-13

# (entry point's kernel family, copula, general power?) -> tier, with the lines that say so
TIERS = {
    # PREFIX slabs: k_mass / node_value -- pow_node (integer: squarings + fast_rcp; fitted nu: log_node /
    # exp_node, 1.4e-14) and the library exp: cvq_quad_kernels.h:227-229
    ("prefix", "student", False): "precise", ("prefix", "student", True): "precise",
    ("prefix", "gaussian", False): "precise", ("prefix", "plackett", False): "precise",
    # DIRECT and COMPACT slabs both run k_direct (cvq_plan.hip launch_slab: "COMPACT: slabs of arbitrary
    # bounds run k_direct"): pow_node_t, cvq_direct_kernels.h:20-41 and :155 (integer: rcp + one Newton
    # step, ~1e-15; PM == 0: pow_node); Gaussian / Plackett: node_value, cvq_quad_kernels.h:229.
    # COMPACT's own fast power (cvq_compact_kernels.h:350-356) runs in its solve only, not in a slab: the
    # "compact-solve" rows below, held by the obj_var probes of tests/test_solve_probes_gpu.py.
    ("direct", "student", False): "precise", ("direct", "student", True): "precise",
    ("direct", "gaussian", False): "precise", ("direct", "plackett", False): "precise",
    # the solve kernels (tests/test_solve_probes_gpu.py; DIRECT's and PREFIX's solves run their slabs' node code:
    # cvq_direct_kernels.h k_direct's solve loop, cvq_quad_kernels.h k_solve_prefix over k_mass's table).
    # k_compact's solve: fast_f, cvq_compact_kernels.h:343-373 -- nu = 6 (PM 8) rcp + one Newton step then two
    # squarings (:346-350); other integer nu pow_node_t (:356); fitted nu and node_m > 128
    # exp2_node7(ex log2(e) log_node_fast(b)) (:352-355); Gaussian exp2_node7 of the folded row constants
    # (:358-361, fast_row_consts :309-313); Plackett rcp + two Newton steps (:363-371); dates deferred to its
    # generic kernel: node_value (:377-394)
    ("compact-solve", "student", False): "precise", ("compact-solve", "student", True): "fast",
    ("compact-solve", "gaussian", False): "fast", ("compact-solve", "plackett", False): "precise",
    # k_sorted's solve loop (:937-973), block tail (:1012), one-wave tail (:1077) and SWEEP's passes (:815) sum
    # the same node_fast / node_generic lambdas (:554, :599) as its slab (:746): the sorted tier
    ("sorted-solve", "student", False): "precise", ("sorted-solve", "student", True): "fast",
    ("sorted-solve", "gaussian", False): "fast", ("sorted-solve", "plackett", False): "precise",
    # SORTED and SWEEP slabs: node_fast, cvq_sorted_kernels.h:554-577 -- Gaussian exp2_node7
    # (:130-133, 4.0e-11); Student pow_fast (:135-160): fitted nu exp2_node7(ex log2(e) log_node_fast(b)),
    # integer nu squarings + rcp + one Newton step (~1e-15); Plackett: rcp + Newton (:560-565)
    ("sorted", "student", False): "precise", ("sorted", "student", True): "fast",
    ("sorted", "gaussian", False): "fast", ("sorted", "plackett", False): "precise",
    # the moment, attribution and quantile kernels: node_value (cvq_moments_kernels.h:144 and the
    # two kernels built on it), cvq_quad_kernels.h:227-229 -- whatever the plan's strategy
    ("moments", "student", False): "precise", ("moments", "student", True): "precise",
    ("moments", "gaussian", False): "precise", ("moments", "plackett", False): "precise",
    # the conditional and batched-weights passes (tests/test_node_ext_gpu.py): their own copies of the slab-row
    # core, make_row / outer_B / node_value at cvq_conditional_kernels.h:170-178 and
    # cvq_portfolio_kernels.h:189-197 -- node_value again, whatever the plan's strategy
    ("cond", "student", False): "precise", ("cond", "student", True): "precise",
    ("cond", "gaussian", False): "precise", ("cond", "plackett", False): "precise",
    ("port", "student", False): "precise", ("port", "student", True): "precise",
    ("port", "gaussian", False): "precise", ("port", "plackett", False): "precise",
    # the predictive distribution and the per-date-record passes (tests/test_q_sweep_gpu.py): their own copies of
    # the slab-row core again -- "dist": k_dist_pass, make_row / outer_B / node_value at
    # cvq_distribution_kernels.h:102-103 and :132, and k_dyn_dist_pass, cvq_dynamic_distribution_kernels.h:110-111
    # and :141; "dyn": k_dyn_pass, cvq_dynamic_kernels.h:183-184 and :191 -- node_value, whatever the plan's
    # strategy and whether the date's parameters are the plan's or a record's
    ("dist", "student", False): "precise", ("dist", "student", True): "precise",
    ("dist", "gaussian", False): "precise", ("dist", "plackett", False): "precise",
    ("dyn", "student", False): "precise", ("dyn", "student", True): "precise",
    ("dyn", "gaussian", False): "precise", ("dyn", "plackett", False): "precise",
    ("dist", "gumbel", False): "precise", ("dyn", "gumbel", False): "precise",
    # the Gumbel kinds (both under "gumbel"; SORTED only, cvq_plan.hip:1348): a SORTED slab of rank-1 dates
    # takes the record path, node_fast at cvq_sorted_kernels.h:578-594 -- log_node / exp_node inside, the outer
    # exponential exp2_node7; dates whose pi_t is not rank 1 take node_generic -> node_value (:599-), as do the
    # moment, attribution, quantile, conditional and batched-weights kernels: cvq_quad_kernels.h:190-204,
    # log_node / exp_node only.  Their bars: tests/gumbel_node_reference.py, stored in node_kat_ext.kat
    ("sorted", "gumbel", False): "fast", ("sorted-generic", "gumbel", False): "precise",
    ("moments", "gumbel", False): "precise", ("cond", "gumbel", False): "precise", ("port", "gumbel", False): "precise",
}
FAMILY = {"prefix": "prefix", "direct": "direct", "compact": "direct", "sorted": "sorted", "sweep": "sorted"}

MEASURED = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@pytest.fixture(scope="module")
def kat():
    return NC.load_kat()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(MEASURED):
        print("MEASURED %-8s %-8s %-9s %-8s max %.3f of bar" % (key + (MEASURED[key],)))


def _node_codes(copula, dim, params):
    """(node_m, node_ex) by the plan's rule (node_cases.plan_codes)."""
    if copula != "student":
        return 0, 0.0
    return NC.plan_codes(params[0], dim)[0], -(float(params[0]) + dim) / 2


def bar_of(family, copula, dim, params):
    node_m, node_ex = _node_codes(copula, dim, params)
    tier = TIERS[(family, copula, node_m < 0)]
    bar = 1e-12 + ((2 * float(params[0]) + 3) * QUANTILE_BAR if copula == "student" else 0.0)
    if tier == "fast":
        bar += EXP7_BAR + abs(node_ex) * LOGFAST_ABS
    return bar, tier, ("general" if node_m < 0 else "integer") if copula == "student" else "-"


def _plan(kw, model, strategy):
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(model, kw["copula"], kw["dim"], kw["x_values"], kw["step"], kw["densities"], kw["combos"],
                       kw["weights"], kw["copula_params"], vol_states=kw["unique_vol_states"], strategy=strategy)
    p.set_dates(kw["per_date"] if model == "msm" else [kw["per_date"]])
    return p


def _hold(label, key, dev, ref, scale, bar, extra=0.0):
    """|dev - ref| <= bar * scale + extra everywhere (scale = 0: the members' x is 0 on that axis, and the
    device's sum must be 0 too); the worst ratio is recorded under key."""
    dev, ref, scale = np.asarray(dev), np.asarray(ref), np.asarray(scale)
    assert np.all(np.isfinite(dev)), (label, dev)
    err, tol = np.abs(dev - ref), bar * scale + extra
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.max(np.where(tol > 0.0, err / tol, np.where(err == 0.0, 0.0, np.inf))))
    MEASURED[key] = max(MEASURED[key], ratio)
    assert ratio <= 1.0, f"{label}: |device - ref| = {ratio:.3f} of the bar {bar:.3e} * scale"


def _run_case(kat, i, model=None):
    case = CASES[i]
    ref_model, copula, dim, params = case
    model = model or ref_model
    kw = NC.problem_inputs(case, kat)
    slabs = NC.slabs(dim)
    T = NC.T
    ran = []
    for strategy in STRATEGIES:
        try:
            p = _plan(kw, model, strategy)
        except ValueError as e:
            assert dim == 3 and strategy in REFUSAL and REFUSAL[strategy] in str(e), (strategy, str(e))
            continue
        assert dim == 2 or strategy in ("prefix", "sorted")
        ran.append(strategy)
        try:
            assert p.strategy == strategy
            bar_s, tier_s, cls = bar_of(FAMILY[strategy], copula, dim, params)
            bar_m, tier_m, _ = bar_of("moments", copula, dim, params)
            for s, (a, b) in enumerate(slabs):
                bounds = np.tile((a, b), (T, 1))
                tag = f"{NC.case_id(case)} {strategy} slab ({a}, {b}]"
                m0r, sc = kat["m0"][i, s], kat["scale"][i, s]
                # PREFIX forms a slab as a difference of running row sums (cvq_quad_kernels.h SolveTeam::slab:
                # pref(kb) - pref(ka)): it rounds against everything at or below the slab's upper bound, n
                # sequential additions per prefix, two prefixes
                extra = 2 * kw["x_values"].size * 2.0 ** -53 * kat["scale_below"][i, s] if strategy == "prefix" else 0.0
                _hold(tag + " compute_integral", (strategy, copula, cls, tier_s), p.compute_integral(bounds), m0r, sc,
                      bar_s, extra)
                key = ("moments", copula, cls, tier_m)
                m0, m1 = p.tail_moments(bounds)
                _hold(tag + " tail_moments m0", key, m0, m0r, sc, bar_m)
                _hold(tag + " tail_moments m1", key, m1, kat["m1"][i, s], kat["scale1"][i, s], bar_m)
                a0, mx = p.axis_moments(bounds)
                _hold(tag + " axis_moments m0", key, a0, m0r, sc, bar_m)
                _hold(tag + " axis_moments mx", key, mx, kat["mx"][i, s][:, :dim], kat["scalex"][i, s][:, :dim], bar_m)
                # one level no slab reaches: var is NaN and m0 = F(max_var), the mass of (lower, max_var]
                var, _, q0 = p.quantiles([1.0e6], min_var=(max(a, -7.5) + b) / 2, max_var=b, lower=a)
                assert np.all(np.isnan(var))
                _hold(tag + " quantiles m0", key, q0[:, 0], m0r, sc, bar_m)
        finally:
            p.close()
    assert ran == (list(STRATEGIES) if dim == 2 else ["prefix", "sorted"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=[NC.case_id(c) for c in CASES])
def test_slabs_against_reference(kat, i):
    _run_case(kat, i)


def test_ukf_once(kat):
    """The UKF model kind runs GARCH's kernels on the same sigma rows: the GARCH case's reference."""
    i = [NC.case_id(c) for c in CASES].index("garch-student-2d-6_0.5")
    _run_case(kat, i, model="mean_reverting")


def test_tier_table_is_complete():
    for case in CASES:
        for fam in ("prefix", "direct", "sorted", "moments"):
            bar, tier, _ = bar_of(fam, *case[1:])
            assert tier in ("precise", "fast") and 1e-12 <= bar < 1e-10
    assert bar_of("sorted", "student", 2, (5.364, 0.5))[1] == "fast"
    assert bar_of("sorted", "student", 2, (127.0, 0.5))[1] == "fast"        # node_m = 129 > 128: the general power
    assert bar_of("sorted", "student", 2, (126.0, 0.5))[1] == "precise"
    assert bar_of("direct", "student", 2, (5.364, 0.5))[1] == "precise"
    # the solve kernels' families (tests/test_solve_probes_gpu.py): COMPACT's solve has its own fast power and
    # Gaussian exponential, which its slab (k_direct) has not; SORTED's solve sits in its slab's tier
    for copula, params in (("student", (6.0, 0.5)), ("student", (5.364, 0.5)), ("student", (127.0, 0.5)),
                           ("gaussian", (0.5,)), ("plackett", (1.5,))):
        assert bar_of("sorted-solve", copula, 2, params) == bar_of("sorted", copula, 2, params)
        assert bar_of("compact-solve", copula, 2, params) == bar_of("sorted", copula, 2, params)
    assert bar_of("compact-solve", "student", 2, (7.0, 0.5))[1] == "precise"
    # the conditional and batched-weights passes sit in the moments tier for every copula; the Gumbel kinds
    # have SORTED instances only (their bars come from the second fixture: tests/test_node_ext_gpu.py)
    for copula, general in (("student", False), ("student", True), ("gaussian", False), ("plackett", False),
                            ("gumbel", False)):
        assert TIERS[("cond", copula, general)] == TIERS[("port", copula, general)] == TIERS[("moments", copula, general)]
        # so do the distribution and per-date-record passes (tests/test_q_sweep_gpu.py)
        assert TIERS[("dist", copula, general)] == TIERS[("dyn", copula, general)] == TIERS[("moments", copula, general)]
    for case in CASES:
        for fam in ("dist", "dyn", "cond", "port"):
            assert bar_of(fam, *case[1:]) == bar_of("moments", *case[1:])
    assert TIERS[("sorted", "gumbel", False)] == "fast" and TIERS[("sorted-generic", "gumbel", False)] == "precise"
    assert not any(fam in ("prefix", "direct") and copula == "gumbel" for fam, copula, _ in TIERS)
    assert all(t in ("precise", "fast") for t in TIERS.values())
