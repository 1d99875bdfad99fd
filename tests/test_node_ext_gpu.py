"""The Gumbel kinds, the chunk-edge shapes, and the conditional (k_cond_pass) and batched-weights
(k_port_pass) passes against the longdouble / mpmath truths of tests/golden/node_kat_ext.kat -- the
sibling of test_node_slabs_gpu.py, whose tier table and bars it shares.  No mpmath, no reference module
and no reference project here: node_cases.py and the two fixtures only.

1. Extension cases (node_cases.ext_cases(): Gumbel and survival Gumbel, GARCH and MSM, 2-D n = 24 and 3-D
   n = 12 at theta in {1, 1 + 2^-30, 1.5, 4, 16}; theta = 4 at the chunk edges 2-D n = 70 and 3-D n = 17 and
   on MSM dates whose pi_t is not rank 1; Plackett theta = 1.5 at 2-D n = 70 and n = 17), per strategy that
   accepts the kind (Gumbel: SORTED only, the others must refuse with the documented message):
   compute_integral, tail_moments, axis_moments and the quantiles m0 probe, as in test_node_slabs_gpu.py.
   Gumbel bars, derived in tests/gumbel_node_reference.py from the device's formulas and stored per case,
   slab and date, never taken from a run:
     precise tier   1e-12 + ebound              (k_moments / k_attrib / k_quant_pass; SORTED's generic path)
     fast tier      1e-12 + ebound_fast + 4.05e-11   (SORTED's record path: the outer exp2_node7)
2. Every case of node_cases.all_cases() (the 82 base cases and the extension cases): per slab
     conditional_quantiles   per axis a stress event (-inf, x[n//3]] and a band (x[n//4], x[3n//4]]: m0 of one
                             level no slab reaches = the mass of slab & event, p_event = the event's mass over
                             the box; the event (-inf, +inf) gives quantiles' m0 bit for bit; an event without
                             a node gives exactly 0
     portfolio_quantiles     three candidates (the plan's own weights, an unequal vector, one with a zero or
                             negative secondary weight): candidate 0 = quantiles' m0 bit for bit, the others
                             against the same masses under their own membership
   at the moments-tier bar of the case, applied to the sum |mass| of the members in question (plus one
   smallest normal float64: an intersection of corner nodes can lie under the normal range).

Measured on one MI355X, worst |device - ref| in units of the bar (the `MEASURED` lines of a run):

  kernels                               Gumbel        survival Gumbel   Plackett (edge shapes)
  SORTED slab, record path (fast)       0.944         0.963             0.002 (precise)
  SORTED slab, generic path (precise)   0.035         0.010             -
  moments / attribution / quantile      0.081         0.038             0.002
  other strategies' slabs               refused       refused           0.002

                                        Student       Gaussian          Plackett     Gumbel     survival Gumbel
  k_cond_pass m0 (slab & event)         0.433         0.506             0.028        0.119      0.043
  k_cond_pass p_event                   0.052         0.010             0.389        0.013      0.010
  k_port_pass m0 (candidates 1, 2)      0.432         0.243             0.039        0.112      0.045

The fast tier's 0.94-0.96 is exp2_node7's own polynomial error (4.045e-11 of the 4.05e-11 in the bar); the
precise tier sits far under its bar because the bar grants log_node and exp_node their documented 1.4e-14
at every use and they are closer than that.
"""
import collections

import numpy as np
import pytest

import node_cases as NC
from test_node_slabs_gpu import FAMILY, REFUSAL, STRATEGIES, TIERS, _plan, bar_of

pytestmark = pytest.mark.gpu

EXT, ALL = NC.ext_cases(), NC.all_cases()
FIRST = len(ALL) - len(EXT)
# cvq_plan_create (cvq_plan.hip): "the Gumbel copulas run on the SORTED strategy (CVQ_STRATEGY_SORTED) only"
GUMBEL_REFUSAL = "the Gumbel copulas run on the SORTED strategy"
NO_LEVEL = [1.0e6]                        # a level no slab reaches: var is NaN and m0 = F(max_var)

MEASURED = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@pytest.fixture(scope="module")
def z():
    out = NC.load_kat()
    out.update(NC.load_ext())
    return out


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(MEASURED):
        print("MEASURED %-14s %-16s %-8s max %.3f of bar" % (key + (MEASURED[key],)))


def _hold(label, key, dev, ref, scale, bar, extra=0.0):
    """|dev - ref| <= bar * scale + extra everywhere (bar: a number or an array of dev's shape); the worst
    ratio is recorded under key."""
    dev, ref, scale = np.asarray(dev), np.asarray(ref), np.asarray(scale)
    assert dev.shape == ref.shape == scale.shape, (label, dev.shape, ref.shape, scale.shape)
    assert np.all(np.isfinite(dev)), (label, dev)
    err, tol = np.abs(dev - ref), np.asarray(bar) * scale + extra
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.max(np.where(tol > 0.0, err / tol, np.where(err == 0.0, 0.0, np.inf))))
    MEASURED[key] = max(MEASURED[key], ratio)
    assert ratio <= 1.0, f"{label}: |device - ref| = {ratio:.3f} of the bar {np.max(bar):.3e} * scale"


def _tier(family, copula):
    return TIERS[(family, "gumbel" if copula in NC.GUMBEL_KINDS else copula, False)]


def _moments_bar(z, i, name, idx):
    """The moments-tier bar of all_cases()[i]: the case's own (bar_of) or, for a Gumbel kind, 1e-12 + the
    stored bound z[name][idx]."""
    case = ALL[i]
    if case[1] in NC.GUMBEL_KINDS:
        assert _tier("moments", case[1]) == "precise"
        return NC.gumbel_bar(z[name][idx], "precise")
    return bar_of("moments", *case[1:4])[0]


# ------------------------------------------------------------------ 1. the extension cases' slabs
def _run_ext_case(z, e, model=None):
    case = EXT[e]
    ref_model, copula, dim, params, n, variant = case
    model = model or ref_model
    gumbel = copula in NC.GUMBEL_KINDS
    kw = NC.ext_problem_inputs(case, z)
    assert kw["x_values"].size == n
    slabs, T = NC.slabs(dim), NC.T
    ran = []
    for strategy in STRATEGIES:
        try:
            p = _plan(kw, model, strategy)
        except ValueError as err:
            # (in 3-D the 2-D-only strategies refuse the shape before the kind is looked at)
            documented = (GUMBEL_REFUSAL, REFUSAL[strategy]) if dim == 3 and strategy in REFUSAL else (GUMBEL_REFUSAL,)
            assert gumbel and strategy != "sorted" and any(m in str(err) for m in documented), (strategy, str(err))
            continue
        ran.append(strategy)
        try:
            assert p.strategy == strategy
            if gumbel:
                # rank-1 dates take SORTED's record path (node_fast), the others node_value
                tier_s = _tier("sorted", copula) if variant != "nr1" else _tier("sorted-generic", copula)
                assert tier_s == ("precise" if variant == "nr1" else "fast")
                fam = "sorted" if variant != "nr1" else "sorted-generic"
            else:
                bar_s, tier_s, _ = bar_of(FAMILY[strategy], copula, dim, params)
                fam = strategy
            for s, (a, b) in enumerate(slabs):
                bounds = np.tile((a, b), (T, 1))
                tag = f"{NC.ext_case_id(case)} {strategy} slab ({a}, {b}]"
                m0r, sc = z["ext_m0"][e, s], z["ext_scale"][e, s]
                if gumbel:
                    bar_s = NC.gumbel_bar(z["ext_ebound_fast" if tier_s == "fast" else "ext_ebound"][e, s], tier_s)
                    bar_m = NC.gumbel_bar(z["ext_ebound"][e, s], "precise")
                    bar_1 = NC.gumbel_bar(z["ext_ebound1"][e, s], "precise")
                    bar_x = NC.gumbel_bar(z["ext_eboundx"][e, s][:, :dim], "precise")
                else:
                    bar_m = bar_1 = bar_x = bar_of("moments", copula, dim, params)[0]
                # PREFIX: a difference of running row sums (test_node_slabs_gpu.py)
                extra = 2 * n * 2.0 ** -53 * z["ext_scale_below"][e, s] if strategy == "prefix" else 0.0
                _hold(tag + " compute_integral", (fam, copula, tier_s), p.compute_integral(bounds), m0r, sc, bar_s, extra)
                key = ("moments", copula, _tier("moments", copula))
                m0, m1 = p.tail_moments(bounds)
                _hold(tag + " tail_moments m0", key, m0, m0r, sc, bar_m)
                _hold(tag + " tail_moments m1", key, m1, z["ext_m1"][e, s], z["ext_scale1"][e, s], bar_1)
                a0, mx = p.axis_moments(bounds)
                _hold(tag + " axis_moments m0", key, a0, m0r, sc, bar_m)
                _hold(tag + " axis_moments mx", key, mx, z["ext_mx"][e, s][:, :dim], z["ext_scalex"][e, s][:, :dim], bar_x)
                var, _, q0 = p.quantiles(NO_LEVEL, min_var=(max(a, -7.5) + b) / 2, max_var=b, lower=a)
                assert np.all(np.isnan(var))
                _hold(tag + " quantiles m0", key, q0[:, 0], m0r, sc, bar_m)
        finally:
            p.close()
    assert ran == (["sorted"] if gumbel else list(STRATEGIES))


@pytest.mark.parametrize("e", range(len(EXT)), ids=[NC.ext_case_id(c) for c in EXT])
def test_ext_slabs_against_reference(z, e):
    _run_ext_case(z, e)


def test_ukf_once(z):
    """The UKF model kind runs GARCH's kernels on the same sigma rows: the GARCH case's reference."""
    _run_ext_case(z, [NC.ext_case_id(c) for c in EXT].index("garch-gumbel-2d-4-n24"), model="mean_reverting")


# ------------------------------------------------------------------ 2. k_cond_pass and k_port_pass, every case
@pytest.mark.parametrize("i", range(len(ALL)), ids=[NC.ext_case_id(c) for c in ALL])
def test_conditional_and_portfolio_against_reference(z, i):
    case = ALL[i]
    model, copula, dim, params, n, variant = case
    kw = NC.ext_problem_inputs(case, z)
    x = kw["x_values"]
    T = NC.T
    kind = "gumbel" if copula in NC.GUMBEL_KINDS else copula
    assert TIERS[("cond", kind, False)] == TIERS[("port", kind, False)] == "precise"
    W = np.ascontiguousarray(z["port_w"][i][:, :dim])
    p = _plan(kw, model, "sorted" if copula in NC.GUMBEL_KINDS else "auto")
    try:
        for s, (a, b) in enumerate(NC.slabs(dim)):
            probe = dict(min_var=(max(a, -7.5) + b) / 2, max_var=b, lower=a)
            tag = f"{NC.ext_case_id(case)} slab ({a}, {b}]"
            _, _, q0 = p.quantiles(NO_LEVEL, **probe)
            for k, (c, name, (lo, hi)) in enumerate(NC.events(x, dim)):
                ev = k % 2
                covar, _, m0, pe = p.conditional_quantiles(c, np.tile((lo, hi), (T, 1)), NO_LEVEL, **probe)
                assert np.all(np.isnan(covar))
                idx = (i, s, c, ev)
                _hold(f"{tag} axis {c} {name} m0", ("cond m0", copula, "precise"), m0[:, 0], z["m0_event"][idx],
                      z["scale_event"][idx], _moments_bar(z, i, "ebound_event", idx), NC.MIN_NORMAL)
                if s == 0:                                      # lower = -100: the event over the whole box
                    idx = (i, c, ev)
                    _hold(f"{tag} axis {c} {name} p_event", ("cond p_event", copula, "precise"), pe, z["p_event"][idx],
                          z["scale_pevent"][idx], _moments_bar(z, i, "ebound_pevent", idx), NC.MIN_NORMAL)
            for c in range(dim):
                # an event between no two grid points, below the grid
                _, _, m0, pe = p.conditional_quantiles(c, np.tile((x[0] - 2.0, x[0] - 1.0), (T, 1)), NO_LEVEL, **probe)
                assert np.all(m0 == 0.0) and np.all(pe == 0.0), f"{tag}: an event without a node on axis {c}"
            var, _, m0 = p.portfolio_quantiles(W, NO_LEVEL, **probe)
            assert np.all(np.isnan(var)) and m0.shape == (T, 3, 1)
            assert np.array_equal(m0[:, 0, :], q0), f"{tag}: candidate 0 is the plan's own weight vector"
            for c in (1, 2):
                idx = (i, s, c)
                _hold(f"{tag} candidate {W[c].tolist()} m0", ("port m0", copula, "precise"), m0[:, c, 0], z["m0_port"][idx],
                      z["scale_port"][idx], _moments_bar(z, i, "ebound_port", idx), NC.MIN_NORMAL)
    finally:
        p.close()


@pytest.mark.parametrize("dim", (2, 3))
def test_full_event_reproduces_quantiles_m0(z, dim):
    """The event (-inf, +inf) on any axis is no event: m0 equal to quantiles' m0 bit for bit, every case
    and slab of the dimension.

    3-D chunks are not split among waves, so k_cond_pass adds a row's node values in k_quant_pass' order by
    itself.  A 2-D chunk's column range is split among its four waves; k_cond_pass' opening pass carries a
    tenth cut, +inf (its sum is p_event), which used to stretch that range to the row's end and so move
    every wave's share: 494 of the 2016 values here then differed from quantiles', by at most 4.1e-16
    relative.  The opening pass now splits k_quant_pass' own range first and the columns only the +inf cut
    reaches after it (cvq_conditional_kernels.h)."""
    worst, where, n_diff, n_all = 0.0, None, 0, 0
    T = NC.T
    for i, case in enumerate(ALL):
        if case[2] != dim:
            continue
        kw = NC.ext_problem_inputs(case, z)
        p = _plan(kw, case[0], "sorted" if case[1] in NC.GUMBEL_KINDS else "auto")
        try:
            for a, b in NC.slabs(dim):
                probe = dict(min_var=(max(a, -7.5) + b) / 2, max_var=b, lower=a)
                _, _, q0 = p.quantiles(NO_LEVEL, **probe)
                for c in range(dim):
                    _, _, m0, _ = p.conditional_quantiles(c, np.tile((-NC.INF, NC.INF), (T, 1)), NO_LEVEL, **probe)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        rel = np.where(q0 != 0.0, np.abs(m0 - q0) / np.abs(q0), np.where(m0 == q0, 0.0, np.inf))
                    n_all += m0.size
                    n_diff += int(np.sum(m0 != q0))
                    if rel.max() > worst:
                        worst, where = float(rel.max()), f"{NC.ext_case_id(case)} slab ({a}, {b}] axis {c}"
        finally:
            p.close()
    print(f"MEASURED full event vs quantiles m0, {dim}-D: {n_diff} of {n_all} values differ, worst relative "
          f"difference {worst:.2e} ({where})")
    assert n_diff == 0, f"{n_diff} of {n_all} values differ, worst relative difference {worst:.2e} at {where}"


def test_ext_tier_table_is_complete(z):
    for fam in ("sorted", "sorted-generic", "moments", "cond", "port"):
        assert ("prefix", "gumbel", False) not in TIERS and (fam, "gumbel", False) in TIERS
    assert _tier("sorted", "gumbel_survival") == "fast" and _tier("sorted-generic", "gumbel") == "precise"
    gum = [e for e, c in enumerate(EXT) if c[1] in NC.GUMBEL_KINDS]
    for e in gum:
        assert np.all(z["ext_ebound"][e] > 0.0) and np.all(z["ext_ebound_fast"][e] > 0.0)
        assert 1e-12 < NC.gumbel_bar(z["ext_ebound"][e], "precise").max() < 1e-11
        assert NC.EXP7_BAR < NC.gumbel_bar(z["ext_ebound_fast"][e], "fast").max() < 5e-11
    for name in ("ebound_event", "ebound_pevent", "ebound_port"):
        assert NC.gumbel_bar(z[name], "precise").max() < 1e-11
        assert not np.any(z[name][:FIRST]) and not np.any(z[name][[FIRST + e for e in range(len(EXT)) if e not in gum]])
