"""Every strategy's solve path against the longdouble truth of the whole decision chain, by obj_var probes
(tests/solve_probe_reference.py states the method; tests/golden/solve_probes.kat holds the probes).

The slabs of every strategy are held to the reference by tests/test_node_slabs_gpu.py; the solves -- k_compact's
fast_f / range_sum / fpair schedule / team_sum1 / block tail / generic kernel, k_sorted's solve loop and tails,
SWEEP's passes, k_direct's and k_solve_prefix's level loops -- were held by VaR parity with the float64 oracle
alone, which survives 1e-8 of relative node noise.  Here each probe is one cvq_solve_local with
obj_var = F_true(target) +- bar M: the target date's K + 1 snapshot mids must equal the truth path bit for bit,
which they do only if the device's own F at the target is within bar M of the truth.

One test per (case, n, argument set) of solve_probe_cases.probe_cases(); per strategy that accepts the shape
the probes of its tier (precise, prefix, fast: solve_probe_cases.bar_and_tier, the TIERS rows "compact-solve"
and "sorted-solve" of tests/test_node_slabs_gpu.py).  Shapes: 2-D n = 24 (one level, then COMPACT's block
tail), 128 (the GARCH grid: two levels through kcut), 320 (two rows per thread; with tolerance 0.6 a plan
without cell tables, whose levels run level_sums and, in bracket 0, end in the one-wave tail); min_var = -7.3
for the lane-0 walk; MSM batches whose middle date is not rank 1 (the generic
kernels); 3-D n = 12 and 40 (SORTED and PREFIX).  GARCH's generic path (non-finite table entries) lies
outside NodeProblem's regular regime and stays with the oracle-parity tests.

Each probe is also solved at 1/4 and 1/16 of its offset: reported only (the `MEASURED` lines: the smallest
of the three multiples of the bar at which every probe of the family and copula still agrees), never asserted.
Measured on one MI355X:

  kernel family    Student integer nu   Student fitted nu / nu = 127   Gaussian            Plackett   Gumbel
  prefix           1/16                 1/16                           1/16                1/16       -
  direct           1/16                 1/16                           1/16                1/16       -
  compact-solve    1/16                 1/4  (1/16: 734 of 758)        1  (1/4: 1139/1142) 1/16       -
  sorted-solve     1/16                 1/4  (1/16: 1468 of 1516)      1  (1/4: 2601/2605) 1/16       1  (1/4: 289 / 290)
  (sorted-solve: SORTED and SWEEP.)  The fast paths sit at exp2_node7's own 4.045e-11, as their slabs do.
"""
import collections

import numpy as np
import pytest
import torch

import node_cases as NC
import solve_probe_cases as SC

pytestmark = pytest.mark.gpu

CASES = SC.probe_cases()
FRACTIONS = (1.0, 0.25, 0.0625)
# (kernel family, copula class) -> fraction -> [probes run, probes that agree]
MEASURED = collections.defaultdict(lambda: {f: [0, 0] for f in FRACTIONS})


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@pytest.fixture(scope="module")
def kat():
    return NC.load_kat()


@pytest.fixture(scope="module")
def probes():
    return SC.load_probes()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(MEASURED):
        ok = [f for f in FRACTIONS if MEASURED[key][f][0] and MEASURED[key][f][0] == MEASURED[key][f][1]]
        print("MEASURED %-13s %-16s agrees down to %s of the bar  (%s)" % (
            key + ("%.4g" % min(ok) if ok else "none",
                   ", ".join("%g: %d/%d" % (f, MEASURED[key][f][1], MEASURED[key][f][0]) for f in FRACTIONS))))


def _copula_class(case):
    copula, dim, params = case[1], case[2], case[3]
    if copula != "student":
        return copula
    return "student-" + ("general" if NC.plan_codes(params[0], dim)[0] < 0 else "integer")


def _run_strategy(case, kw, strategy, rec, K):
    """Solve every probe of `rec` (and its fractions) on one plan; returns the (fraction, probe) -> mids array."""
    from copula_var import engine
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(case[0], kw["copula"], kw["dim"], kw["x_values"], kw["step"], kw["densities"], kw["combos"],
                       kw["weights"], kw["copula_params"], vol_states=kw["unique_vol_states"], strategy=strategy)
    try:
        assert p.strategy == strategy
        p.set_stream(torch.cuda.current_stream().cuda_stream)      # order with the torch buffers
        p.set_dates(kw["per_date"] if case[0] == "msm" else [kw["per_date"]])
        n = rec["obj"].size
        stride = K + 1
        snaps = torch.full((len(FRACTIONS), n, SC.T, stride), float("nan"), dtype=torch.float64, device="cuda")
        hdr = torch.zeros((len(FRACTIONS), n, 2), dtype=torch.int64, device="cuda")
        for f, frac in enumerate(FRACTIONS):
            for i in range(n):
                off = float(rec["offset"][i]) * float(rec["sign"][i])
                obj = float(rec["obj"][i]) if frac == 1.0 else (float(rec["obj"][i]) - off) + off * frac
                args = engine.solve_args(0.0, **SC.solve_kwargs(case[6], obj))
                assert QuadraturePlan.snap_stride(args) == stride
                p.solve_local(args, hdr[f, i].data_ptr(), snaps[f, i].data_ptr())
        torch.cuda.synchronize()
        # the rank header of every solve (cvq_common.h Header: int32 iters, int32 error, uint64 nonzero): every
        # date converged within the K levels the snapshots hold
        words = hdr.cpu().numpy().view(np.int32).reshape(len(FRACTIONS), n, 4)
        assert not np.any(words[..., 1]), (strategy, "a solve reported a date that did not converge")
        assert np.all((words[..., 0] >= 0) & (words[..., 0] <= K)), (strategy, int(words[..., 0].min()), int(words[..., 0].max()))
        return snaps.cpu().numpy()
    finally:
        p.close()


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[SC.probe_case_id(c) for c in CASES])
def test_solve_probes(kat, probes, ci):
    case = CASES[ci]
    kw = SC.problem_inputs(case, kat)
    rec_all = SC.probes_of(probes, ci)
    K = int(probes["K"][ci])
    a = SC.solve_kwargs(case[6])
    assert SC.snap_K(a) == K
    ran, failures = [], []
    for strategy in SC.STRATEGIES:
        if not SC.accepts(strategy, case[2], case[1]):
            continue
        ran.append(strategy)
        _, tier = SC.bar_and_tier(case, strategy)
        sel = np.flatnonzero(rec_all["tier"] == tier)
        assert sel.size, (strategy, tier)
        rec = {k: v[sel] for k, v in rec_all.items()}
        got = _run_strategy(case, kw, strategy, rec, K)
        key = (SC.family_of(strategy, case[2]), _copula_class(case))
        for i in range(sel.size):
            want = SC.mids_from_bits(a, int(rec["bracket"][i]), int(rec["bits"][i]), K)
            t = int(rec["date"][i])
            for f, frac in enumerate(FRACTIONS):
                same = np.array_equal(got[f, i, t], want)
                MEASURED[key][frac][0] += 1
                MEASURED[key][frac][1] += int(same)
                if frac == 1.0 and not same:
                    k = int(np.argmax(got[f, i, t] != want))
                    failures.append("%s date %d %s level %d sign %+d obj' %.17g offset %.3e: first differing mid at "
                                    "level %d (device %.17g, truth %.17g)"
                                    % (strategy, t, SC.KINDS[int(rec["kind"][i])], int(rec["level"][i]), int(rec["sign"][i]),
                                       float(rec["obj"][i]), float(rec["offset"][i]), k, got[f, i, t][k], want[k]))
    assert ran, case
    assert not failures, "%d probes off the truth path:\n%s" % (len(failures), "\n".join(failures[:12]))
