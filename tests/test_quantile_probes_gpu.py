"""The exact-quantile searches -- cvq_quantiles, cvq_conditional_quantiles, cvq_portfolio_quantiles and
cvq_dynamic_quantiles -- against the longdouble truth of their whole decision path, by level probes
(tests/quantile_probe_reference.py states the method; tests/golden/quantile_probes.kat holds the probes).

The row cores' opening pass is held by tests/test_node_slabs_gpu.py and tests/test_node_ext_gpu.py; the narrow
passes (C = 7 and C = 2: each lane walks jm = ka + 1 + k and loads the clamped column), the update kernels (the
chain F(lo) + increment and M1(lo) + increment across up to 9 passes, the at +- half descent, quant_sum over row
chunks, the bracket test, the target alpha p_E) were held to the float64 checker where margin >= 1e-7 alone, which
survives 1e-8 of relative error in F.  Here each probe is one level alpha' = F_true(target) +- bar M: the returned
var, (lo + hi) / 2 of dyadic midpoints, must equal the truth path's bit for bit (NaN included), which it does only
if the device's own F at the target is within bar M of the truth.  Per probe also
  |m0 - truth| <= bar sum |mass|
  |es - truth| <= (bar sum |level mass| + |m1 / m0| bar sum |mass|) / |m0| + 4 2^-53 (|m1 / m0| + |ptf_mean|)
                  (first order in the two sums, plus the division and the add)
  conditional: |p_event - truth| <= bar sum_E |mass|
  outside the bracket: var and es NaN, m0 = F(max_var) at the bar.

One test per plan (copula, model, shape); its cases (quantile_probe_cases.probe_cases(): argument sets, events on
every axis, three candidate weight vectors in one call, per-date weights and parameters) run on that plan, probes
packed eight to a call, each level judged on its target date's row.  A case's first call carries NO_LEVEL and a
tiny level between live probes (finished workgroups beside live ones); its first three probes are repeated at
L = 1 and L = 3 and must give the same bits.  `quantiles` runs on every strategy that accepts the shape for the
first plan of each copula (the kernels do not depend on it), on SORTED elsewhere.

Each probe is also run at 1/4 and 1/16 of its offset: reported only (the `MEASURED` lines), never asserted.
Measured on one MI355X: every probe of every call and copula agrees at the bar, at 1/4 and at 1/16 of it; worst
|device - truth| in units of the bar:

  call    Student integer nu            Student fitted nu / nu = 127   Gaussian   Plackett   Gumbel
  quant   m0 0.082  es 0.004            m0 0.025  es 0.001             m0 0.006   m0 0.001   m0 0.205  es 0.003
  cond    m0 0.082  es 0.004  p_E 0.014 -                              m0 0.006   -          -
  port    m0 0.082  es 0.004            -                              m0 0.006   -          m0 0.205  es 0.001
  dyn     m0 0.082  es 0.003            -                              m0 0.003   -          -
"""
import collections

import numpy as np
import pytest

import node_cases as NC
import quantile_probe_cases as QC
import solve_probe_cases as SC

pytestmark = pytest.mark.gpu

CASES = QC.probe_cases()
GROUPS = list(dict.fromkeys(QC.group_key(c) for c in CASES))
FRACTIONS = (1.0, 0.25, 0.0625)
TINY = 1.0e-300
# (call, copula class) -> worst |device - truth| in units of the bar, per quantity
WORST = collections.defaultdict(lambda: dict(m0=0.0, es=0.0, p_event=0.0))
# (call, copula class) -> fraction -> [probes run, probes that agree]
AGREE = collections.defaultdict(lambda: {f: [0, 0] for f in FRACTIONS})


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@pytest.fixture(scope="module")
def kat():
    return NC.load_kat()


@pytest.fixture(scope="module")
def probes():
    return QC.load_probes()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        w = WORST[key]
        print("MEASURED %-6s %-16s worst / bar: m0 %.3f  es %.3f  p_event %.3f   agree (%s)" % (
            key + (w["m0"], w["es"], w["p_event"],
                   ", ".join("%g: %d/%d" % (f, AGREE[key][f][1], AGREE[key][f][0]) for f in FRACTIONS))))


def _copula_class(case):
    copula, dim, params = case[2], case[3], case[4]
    if copula != "student":
        return "gumbel" if copula in NC.GUMBEL_KINDS else copula
    return "student-" + ("general" if NC.plan_codes(params[0], dim)[0] < 0 else "integer")


def _plan(key, kw, strategy):
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(key[0], kw["copula"], kw["dim"], kw["x_values"], kw["step"], kw["densities"], kw["combos"],
                       kw["weights"], kw["copula_params"], vol_states=kw["unique_vol_states"], strategy=strategy)
    assert p.strategy == strategy
    p.set_dates(kw["per_date"] if key[0] == "msm" else [kw["per_date"]])
    return p


def _calls(n):
    """[[level slots]]: probe indices eight to a call; the first call carries NO_LEVEL and a tiny level (-1, -2)
    between live probes."""
    first = list(range(min(n, QC.MAX_LEVELS - 2)))
    first[1:1] = [-1]
    first[min(3, len(first)):min(3, len(first))] = [-2]
    rest = list(range(QC.MAX_LEVELS - 2, n))
    return [first] + [rest[i:i + QC.MAX_LEVELS] for i in range(0, len(rest), QC.MAX_LEVELS)]


def _levels(rec, slots, frac, unit=None):
    """The call's levels: alpha' itself, or the target's level plus `frac` of the offset (unit[t]: the offset's
    size in units of the level, 1 / p_E for the conditional call)."""
    out = []
    for i in slots:
        if i < 0:
            out.append(QC.NO_LEVEL if i == -1 else TINY)
            continue
        off = float(rec["offset"][i]) * float(rec["sign"][i]) * (1.0 if unit is None else float(unit[int(rec["date"][i])]))
        a = float(rec["alpha"][i])
        base = a - off
        if abs(base) < 1e-6 * a:                       # (a target whose F is 0: the level is the offset alone)
            base = 0.0
        out.append(a if frac == 1.0 else base + off * frac)
    return out


def _run(call, rec, n_out=3, unit=None):
    """Every probe of `rec` through `call(levels) -> arrays (T, L) (or (T,) for p_event)`: per fraction the probes'
    own (var, es, m0[, p_event]) rows, picked on each probe's date."""
    n = rec["alpha"].size
    got = np.full((len(FRACTIONS), n, n_out), np.nan)
    for f, frac in enumerate(FRACTIONS):
        for slots in _calls(n):
            res = call(_levels(rec, slots, frac, unit))
            for l, i in enumerate(slots):
                t = int(rec["date"][i]) if i >= 0 else 0
                if i == -1:
                    assert np.all(np.isnan(res[0][:, l])) and np.all(np.isnan(res[1][:, l]))
                if i < 0:
                    continue
                got[f, i, :3] = [res[k][t, l] for k in range(3)]
                if n_out == 4:
                    got[f, i, 3] = res[3][t]
    # idx % L and idx / L: the first three probes alone and three to a call
    head = list(range(min(3, n)))
    if head:
        three = call(_levels(rec, head, 1.0))
        for l, i in enumerate(head):
            one = call(_levels(rec, [i], 1.0))
            t = int(rec["date"][i])
            for k in range(3):
                assert np.array_equal([one[k][t, 0], three[k][t, l]], [got[0, i, k]] * 2, equal_nan=True), (i, k)
    return got


def _judge(case, a_of, rec, got, bar_t, key, pe=None, tag=""):
    """The assertions of the module docstring on one case's probes; returns the failures' descriptions."""
    K = QC.bisection_steps(a_of(0))
    m0_t, es_t = QC.joined(rec["m0_hi"], rec["m0_lo"]), QC.joined(rec["es_hi"], rec["es_lo"])
    failures = []
    for i in range(rec["alpha"].size):
        t = int(rec["date"][i])
        a = a_of(t)
        bar = float(bar_t[t])
        want = QC.var_from_bits(a, int(rec["nan"][i]), int(rec["bits"][i]), K)
        for f, frac in enumerate(FRACTIONS):
            same = np.array_equal([got[f, i, 0]], [want], equal_nan=True)
            AGREE[key][frac][0] += 1
            AGREE[key][frac][1] += int(same)
        var, es, m0 = got[0, i, :3]
        what = "%s%s date %d %s level %d sign %+d alpha' %.17g offset %.3e" % (
            tag, QC.probe_case_id(case), t, QC.KINDS[int(rec["kind"][i])], int(rec["level"][i]), int(rec["sign"][i]),
            float(rec["alpha"][i]), float(rec["offset"][i]))
        if not np.array_equal([var], [want], equal_nan=True):
            failures.append("%s: var %.17g, truth %.17g" % (what, var, want))
            continue
        tol0 = bar * float(rec["scale0"][i])
        e0 = abs(float(np.longdouble(m0) - m0_t[i]))
        r0 = e0 / tol0 if tol0 > 0 else (0.0 if e0 == 0.0 else np.inf)
        WORST[key]["m0"] = max(WORST[key]["m0"], r0)
        if not r0 <= 1.0:
            failures.append("%s: m0 %.17g off the truth %.17g by %.3f of the bar" % (what, m0, float(m0_t[i]), r0))
        if np.isnan(float(es_t[i])):
            if not np.isnan(es):
                failures.append("%s: es %.17g where the truth has none" % (what, es))
        else:
            ratio = abs(float(es_t[i]) - a["ptf_mean"])                  # |m1 / m0|
            tol = ((bar * float(rec["scale1"][i]) + ratio * bar * float(rec["scale0"][i])) / abs(float(m0_t[i]))
                   + 4 * QC.U53 * (ratio + abs(a["ptf_mean"])))
            re = abs(float(np.longdouble(es) - es_t[i])) / tol
            WORST[key]["es"] = max(WORST[key]["es"], re)
            if not re <= 1.0:
                failures.append("%s: es %.17g off the truth %.17g by %.3f of the bar" % (what, es, float(es_t[i]), re))
        if pe is not None:
            pe_t, tol_e = pe
            rp = abs(float(np.longdouble(got[0, i, 3]) - pe_t[t])) / tol_e[t]
            WORST[key]["p_event"] = max(WORST[key]["p_event"], rp)
            if not rp <= 1.0:
                failures.append("%s: p_event %.17g off the truth by %.3f of the bar" % (what, got[0, i, 3], rp))
    return failures


def _kwargs(a):
    return dict(min_var=a["min_var"], max_var=a["max_var"], lower=a["lower"], tolerance=a["tolerance"])


@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=[QC.group_id(g) for g in GROUPS])
def test_quantile_probes(kat, probes, gi):
    key = GROUPS[gi]
    mine = [ci for ci, c in enumerate(CASES) if QC.group_key(c) == key]
    kw = QC.problem_inputs(CASES[mine[0]], kat)
    dim, copula = key[2], key[1]
    first_of_copula = gi == min(g for g, k in enumerate(GROUPS) if k[1] == copula)
    strategies = [s for s in SC.STRATEGIES if SC.accepts(s, dim, copula)] if first_of_copula else ["sorted"]
    failures = []
    for strategy in strategies:
        p = _plan(key, kw, strategy)
        try:
            port = {}
            for ci in mine:
                case = CASES[ci]
                if strategy != strategies[-1] and not (case[0] == "quant" and case[7] == "default"):
                    continue                                   # the other strategies: `quantiles`, default arguments
                rec = QC.probes_of(probes, ci)
                a_of = lambda t, case=case: QC.args_of(case, kw, t)
                a = a_of(0)
                fam = (case[0], _copula_class(case))
                tag = strategy + " "
                if case[0] == "quant":
                    got = _run(lambda lv: p.quantiles(lv, a["ptf_mean"], **_kwargs(a)), rec)
                    failures += _judge(case, a_of, rec, got, probes["bar"][ci], fam, tag=tag)
                elif case[0] == "cond":
                    ax, _, (lo, hi) = QC.event_of(case, kw)
                    cond = np.tile((lo, hi), (QC.T, 1))
                    pe_t = QC.joined(probes["pe_hi"][ci], probes["pe_lo"][ci])
                    got = _run(lambda lv: p.conditional_quantiles(ax, cond, lv, a["ptf_mean"], **_kwargs(a)), rec, n_out=4,
                               unit=1.0 / probes["pe_hi"][ci])
                    failures += _judge(case, a_of, rec, got, probes["bar"][ci], fam,
                                       pe=(pe_t, probes["bar"][ci] * probes["scale_e"][ci]), tag=tag)
                elif case[0] == "port":
                    port[case[8][0]] = (ci, case, rec)
                else:
                    cp, W = QC.dyn_params(case), QC.port_weights(dim)
                    got = _run(lambda lv: p.dynamic_quantiles(lv, copula_params=cp, weights=W, ptf_mean=np.array(QC.DYN_MEANS),
                                                              **_kwargs(a)), rec)
                    failures += _judge(case, a_of, rec, got, probes["bar"][ci], fam, tag=tag)
                    # no per-date array: `quantiles` bit for bit
                    lv = _levels(rec, _calls(rec["alpha"].size)[0], 1.0)
                    for x, y in zip(p.dynamic_quantiles(lv, **_kwargs(a)), p.quantiles(lv, **_kwargs(a))):
                        assert np.array_equal(x, y, equal_nan=True)
            if port:
                # the three candidates in one call (P = 3: in 3-D a tile of two and a half-empty one), every
                # candidate judged on its own probes
                assert sorted(port) == [0, 1, 2]
                W = QC.port_weights(dim)
                for k, (ci, case, rec) in sorted(port.items()):
                    a = QC.args_of(case, kw)
                    call = lambda lv, k=k: tuple(r[:, k, :] for r in p.portfolio_quantiles(W, lv, a["ptf_mean"], **_kwargs(a)))
                    got = _run(call, rec)
                    failures += _judge(case, lambda t, case=case: QC.args_of(case, kw, t), rec, got, probes["bar"][ci],
                                       (case[0], _copula_class(case)), tag=strategy + " ")
                    if k == 0:                             # candidate 0 carries the plan's own weights
                        lv = _levels(rec, _calls(rec["alpha"].size)[0], 1.0)
                        for x, y in zip(p.portfolio_quantiles(W, lv, a["ptf_mean"], **_kwargs(a)),
                                        p.quantiles(lv, a["ptf_mean"], **_kwargs(a))):
                            assert np.array_equal(x[:, 0, :], y, equal_nan=True)
        finally:
            p.close()
    assert not failures, "%d probes off the truth:\n%s" % (len(failures), "\n".join(failures[:12]))
