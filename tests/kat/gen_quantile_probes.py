"""Writes tests/golden/quantile_probes.kat (an .npz container; tests/quantile_probe_cases.py PROBE_PATH), the
fixture of the exact-quantile level probes; node_kat.kat is read, never written.  Run from the repository
root on a CPU machine with mpmath:

    python tests/kat/gen_quantile_probes.py

Contents (C = len(quantile_probe_cases.probe_cases()), T = 3 dates, a case's probes are the rows
case_start[i] .. case_start[i + 1]):
  sha_case    (C,)   SHA-256 of every case's inputs (quantile_probe_cases.case_digest)
  K           (C,)   the decisions of the case's arguments
  base        (C, T, 5)  the base levels whose truth paths give the date's targets
  candidates, ambiguous  (C, T)  candidate probes of the date and how many of them were dropped as ambiguous
  bar         (C, T)  the relative bar of F (the Gumbel kinds' depends on the date)
  pe_hi, pe_lo, scale_e  (C, T)  conditional: the event's mass over the box and its sum |mass| (else 1, 0, 0)
  per probe   date, kind (min, max, level), level, sign, nan (the level lies outside the bracket), bits (the K
              decisions, bit k set: lo moves up), alpha (alpha'), offset (float32: it sizes nothing but a report),
              count (the target's plateau key), and the closing truths m0, es as hi / lo pairs (lo relative,
              float32: node_cases.truth's form) with their scales sum |mass| and sum |level mass|
tests/test_quantile_probes_cpu.py regenerates every case and requires equality."""
import copy
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "copula-msm-and-copula-garch-var_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import node_cases as NC                  # noqa: E402
import quantile_probe_cases as QC        # noqa: E402
import quantile_probe_reference as QR    # noqa: E402
import solve_probe_cases as SC           # noqa: E402
import solve_probe_reference as SR       # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_solve_probes", SC.GEN_PATH)
SOLVE = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SOLVE)

LD = np.longdouble
MAX_VARIANTS = len(QC.FRACTIONS) // QC.BASES_PER_DATE


def build_problem(case, kat, ztabs):
    """The longdouble reference problem of a case's plan (gen_solve_probes.build_problem: the mpmath quantile
    tables of a shape are computed once)."""
    return SOLVE.build_problem(QC.base_of(case), kat, ztabs)


def date_problem(case, P, t, kw):
    """The problem whose masses, membership and levels are date t's truth: P itself, P under a candidate's or
    the date's weights, or (per-date parameters) one built with the date's copula parameters and weights on
    P's quantile tables, which depend on the u tables and nu alone."""
    w = np.asarray(QC.weights_of(case, t, kw), dtype=np.float64)
    if case[0] == "dyn":
        cp = QC.dyn_params(case)[t]
        args = (kw["model"], kw["copula"], kw["dim"], kw["x_values"], kw["step"], kw["densities"], kw["combos"], w, cp,
                kw["per_date"], kw["unique_vol_states"])
        return type(P)(*args, z=P.quantile_tables())
    if np.array_equal(w, P.w):
        return P
    Pw = copy.copy(P)
    Pw.w = w
    return Pw


def date_truth(case, P, t, kw, geos, mass=None):
    """DateTruth of date t; mass: other flat masses in the longdouble ones' place (the CPU restatement)."""
    import conditional_reference as CR
    Pt = date_problem(case, P, t, kw)
    key = tuple(Pt.w.tolist())
    if key not in geos:
        geos[key] = SR.Geometry(Pt)
    a = QC.args_of(case, kw, t)
    ev = None
    if case[0] == "cond":
        ax, _, (lo, hi) = QC.event_of(case, kw)
        ev = CR.event_mask(Pt, ax, lo, hi)
    gumbel = case[2] in NC.GUMBEL_KINDS
    m = Pt.mass_ld(t) if mass is None else np.reshape(mass, (Pt.n,) * Pt.dim)
    meas = QR.Measure(geos[key], m, Pt.levels_ld(), a["lower"], event=ev,
                      ebound=Pt.ebound_nodes(t) if gumbel else None)
    return QR.DateTruth(meas, a, QC.bisection_steps(a), lambda e: QC.bar_of(case, e), conditional=case[0] == "cond"), Pt


def case_probes(case, P, kat):
    """dict of a case's fixture rows."""
    kw = QC.problem_inputs(case, kat)
    limit, edge_limit = QC.TARGETS["argset" if case[7] != "default" else case[0]]
    recs, geos = [], {}
    base = np.zeros((QC.T, QC.BASES_PER_DATE))
    cand, amb = np.zeros(QC.T, dtype=np.int32), np.zeros(QC.T, dtype=np.int32)
    bars, pe_hi, pe_lo, scale_e = np.zeros(QC.T), np.ones(QC.T), np.zeros(QC.T, dtype=np.float32), np.zeros(QC.T)
    for t in range(QC.T):
        D, _ = date_truth(case, P, t, kw, geos)
        for variant in range(MAX_VARIANTS):
            fr = QC.FRACTIONS[variant * QC.BASES_PER_DATE:(variant + 1) * QC.BASES_PER_DATE]
            targets, bases = QR.candidate_targets(D, fr, limit, edge_limit)
            mine, cand[t], amb[t] = [], 0, 0
            for target in targets:
                for sign in (+1, -1):
                    rec, why = QR.make_probe(D, target, sign)
                    if why == "small":
                        continue
                    cand[t] += 1
                    if rec is None:
                        amb[t] += 1
                        continue
                    rec["date"] = t
                    mine.append(rec)
            if cand[t] > 0 and amb[t] <= QC.AMBIGUOUS_CAP * cand[t]:
                break
        base[t] = bases
        bars[t] = D.bar
        if D.cond:
            pe_hi[t] = np.float64(D.pE)
            pe_lo[t] = float((D.pE - LD(pe_hi[t])) / LD(pe_hi[t]))
            scale_e[t] = float(D.scaleE)
        recs += mine
    assert np.sum(cand) > 0 and np.all(amb <= QC.AMBIGUOUS_CAP * cand), (QC.probe_case_id(case), amb, cand)
    out = {k: np.array([r[k] for r in recs], dtype=dt) for k, dt in QC.PER_PROBE}
    out.update(base=base, candidates=cand, ambiguous=amb, bar=bars, pe_hi=pe_hi, pe_lo=pe_lo, scale_e=scale_e,
               K=np.int32(QC.bisection_steps(QC.args_of(case, kw))))
    return out


def main():
    kat = NC.load_kat()
    cases = QC.probe_cases()
    ztabs, made, rows, sha, start = {}, {}, [], [], [0]
    for i, case in enumerate(cases):
        g = QC.group_key(case)
        if g not in made:
            made[g] = build_problem(case, kat, ztabs)
        r = case_probes(case, made[g], kat)
        rows.append(r)
        sha.append(QC.case_digest(case, kat))
        start.append(start[-1] + r["date"].size)
        print(i, QC.probe_case_id(case), "K", int(r["K"]), "probes", r["date"].size, "ambiguous / candidates",
              r["ambiguous"].tolist(), r["candidates"].tolist(), "bar", r["bar"].tolist(), flush=True)
    out = {k: np.concatenate([r[k] for r in rows]) for k, _ in QC.PER_PROBE}
    for k in QC.PER_CASE:
        out[k] = np.array([r[k] for r in rows])
    out["sha_case"] = np.array(sha)
    out["case_start"] = np.array(start, dtype=np.int32)
    with open(QC.PROBE_PATH, "wb") as f:            # (a file object: savez appends no ".npz")
        np.savez_compressed(f, **out)
    print("wrote", QC.PROBE_PATH, os.path.getsize(QC.PROBE_PATH), "bytes")


if __name__ == "__main__":
    main()
