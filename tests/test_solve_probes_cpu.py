"""CPU checks of the solve-path probes (tests/golden/solve_probes.kat; the method: tests/solve_probe_reference.py).

  * the fixture belongs to today's inputs (digests) and every case regenerates to equal rows;
  * the float64 restatement of the chain (NodeProblem.ftype = np.float64; the Gumbel kinds: device_mass) follows
    every probe's path: a device that computes what the code documents passes;
  * three mutations of those float64 masses each break at least one probe of every case -- half the rows
    x (1 + 30 bar) (per tier, with the tier's own bar), one row x (1 + 1e-9) (but for the one case of ROW_UNSEEN, where
    that is under every probe's offset), one node dropped from a tail cell: errors of the size VaR parity with the oracle does not see (1e-8 decision margin);
  * at most 25% of a (case, date)'s candidate probes were dropped as ambiguous; the bars are bar_of's
    (tests/test_node_slabs_gpu.py) and stay under 1e-11 (precise, prefix) and 5e-11 (fast) -- but for nu = 127,
    whose documented quantile term (2 nu + 3) 7e-14 and log_node_fast term |node_ex| 5e-13 alone exceed those
    caps: there the tier table's own 1e-10 holds;
  * the probes reach every path the GPU module is there for (test_probes_reach_every_path).
"""
import importlib.util
import os

import numpy as np
import pytest

import node_cases as NC
import solve_probe_cases as SC
import solve_probe_reference as SR

_spec = importlib.util.spec_from_file_location("gen_solve_probes", SC.GEN_PATH)
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)

CASES = SC.probe_cases()
IDS = [SC.probe_case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def kat():
    return NC.load_kat()


@pytest.fixture(scope="module")
def probes():
    return SC.load_probes()


@pytest.fixture(scope="module")
def problems(kat):
    """ci -> the case's reference problem; the mpmath quantile tables of a shape are computed once."""
    ztabs, made = {}, {}

    def get(ci):
        if ci not in made:
            made[ci] = GEN.build_problem(CASES[ci], kat, ztabs)
        return made[ci]
    return get


def _mass64(P, t):
    """The float64 restatement of date t's node masses."""
    if P.copula in NC.GUMBEL_KINDS:
        return np.ravel(P.device_mass(t)).astype(np.float64)
    P.ftype = np.float64
    try:
        return np.ravel(P.mass_ld(t)).astype(np.float64)
    finally:
        P.ftype = np.longdouble


def _records(rec):
    n = rec["obj"].size
    return [{k: v[i] for k, v in rec.items()} for i in range(n)]


def test_fixture_belongs_to_these_inputs(kat, probes):
    assert probes["sha_case"].size == len(CASES) and probes["case_start"].size == len(CASES) + 1
    for ci, case in enumerate(CASES):
        assert str(probes["sha_case"][ci]) == SC.case_digest(case, kat), IDS[ci]
        assert int(probes["K"][ci]) == SC.snap_K(SC.solve_kwargs(case[6]))
    assert os.path.getsize(SC.PROBE_PATH) < 275 * 1024


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_fixture_regenerates(probes, problems, ci):
    r = GEN.case_probes(CASES[ci], problems(ci))
    rec = SC.probes_of(probes, ci)
    for k, _ in GEN.PER_PROBE:
        assert np.array_equal(r[k], rec[k]), (IDS[ci], k)
    for k in ("base_obj", "candidates", "ambiguous", "bar"):
        assert np.array_equal(r[k], probes[k][ci]), (IDS[ci], k)


def test_ambiguity_and_bar_caps(probes):
    import test_node_slabs_gpu as SL
    assert np.all(probes["candidates"] > 0)
    assert np.all(probes["ambiguous"] <= SC.AMBIGUOUS_CAP * probes["candidates"])
    for ci, case in enumerate(CASES):
        rec = SC.probes_of(probes, ci)
        tiers = {}
        for s in SC.STRATEGIES:
            if SC.accepts(s, case[2], case[1]):
                bar, tier = SC.bar_and_tier(case, s)
                tiers.setdefault(tier, bar)
        assert set(np.unique(rec["tier"])) == set(tiers), IDS[ci]
        for tier, bar in tiers.items():
            got = float(probes["bar"][ci, tier])
            if case[1] in NC.GUMBEL_KINDS:
                # 1e-12 + exp2_node7's 4.05e-11 + the device formulas' first-order bound, |mass|-weighted
                assert got > NC.EXP7_BAR + 1e-12 and got - NC.EXP7_BAR - 1e-12 < 5e-12, (IDS[ci], got)
            else:
                assert got == bar, (IDS[ci], tier, got, bar)
            cap = SC.FAST_CAP if tier == 2 else SC.PRECISE_CAP
            if case[1] == "student" and case[3][0] == 127.0:
                nu = 127.0
                documented = (2 * nu + 3) * SL.QUANTILE_BAR + (abs(-(nu + 2) / 2) * SL.LOGFAST_ABS if tier == 2 else 0.0)
                assert got - documented < cap and got < 1e-10, (IDS[ci], tier, got)
            else:
                assert got < cap, (IDS[ci], tier, got)
        # the offset is bar M (PREFIX: plus its running-sum term), M <= 3 sum |mass|: never above the bar times
        # a handful of probability masses
        assert np.all(rec["offset"] > 0)


ROW_UNSEEN = {"msm-student-2d-127_0.5-n128"}


def _tail_depth(geo, case):
    d, cnt = SC.build_cell_counts(geo.count, SC.solve_kwargs(case[6]))
    return d, cnt


def _cell_of(a, bracket, bits, depth):
    lo, hi = SC.brackets(a)[bracket]
    for k in range(depth):
        mid = (lo + hi) / 2
        if (int(bits) >> k) & 1:
            lo = mid
        else:
            hi = mid
    return lo, hi


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_float64_chain_passes_and_mutations_fail(probes, problems, ci):
    case, P = CASES[ci], problems(ci)
    a = SC.solve_kwargs(case[6])
    geo = SR.Geometry(P)
    rec = SC.probes_of(probes, ci)
    recs = _records(rec)
    rows = P.n ** (P.dim - 1)                                  # nodes per axis-0 row
    depth, _ = _tail_depth(geo, case)
    D = depth if depth >= 1 else min(2, SC.snap_K(a))
    clean_fail, fails, seen_row = [], {"half": {}, "row": 0, "node": 0}, False
    for t in range(SC.T):
        mine = [r for r in recs if int(r["date"]) == t]
        assert mine, (IDS[ci], t)
        m = _mass64(P, t)
        chain = SR.Chain(geo, m, a)
        clean_fail += [r for r in mine if not SR.follows(chain, r)]
        row_of = np.arange(m.size) // rows
        # (a) half the rows x (1 + 30 bar), per tier with its own bar
        for tier in np.unique(rec["tier"]):
            bar = float(probes["bar"][ci, tier])
            mut = SR.Chain(geo, np.where(row_of % 2 == 0, m * (1 + 30 * bar), m), a)
            fails["half"][tier] = fails["half"].get(tier, 0) + sum(
                not SR.follows(mut, r) for r in mine if int(r["tier"]) == tier)
        # (b) one row x (1 + 1e-9): the row that carries the most mass at or below the first guess (every F holds r0)
        idx = geo.idx(a["lower"], a["first_guess"])
        r_star = int(np.argmax(np.bincount(row_of[idx], weights=np.abs(m[idx]), minlength=P.n)))
        mut = SR.Chain(geo, np.where(row_of == r_star, m * (1 + 1e-9), m), a)
        fails["row"] += sum(not SR.follows(mut, r) for r in mine)
        for r in mine:
            if int(r["sign"]) > 0 and not seen_row:
                kind, b = int(r["kind"]), int(r["bracket"])
                v = (a["first_guess"] if kind == 0 else a["second_guess"][0 if b in (0, 1) else 1] if kind == 1
                     else SC.mids_from_bits(a, b, int(r["bits"]), SC.snap_K(a))[int(r["level"])])
                below = geo.idx(a["lower"], v)
                seen_row = 1e-9 * float(np.sum(np.abs(m[below][row_of[below] == r_star]))) >= 2 * float(r["offset"])
        # (c) one node dropped from the tail cell of the date's first level probe: the cell's median node by mass
        # (a date whose paths have no plateau of their own that deep, the coarse set: its deepest target's own cell)
        lvl = [r for r in mine if int(r["kind"]) == 2 and int(r["level"]) >= D]
        if not lvl:
            lvl = sorted((r for r in mine if int(r["kind"]) == 2), key=lambda r: -int(r["level"]))[:1]
            assert lvl and SC.snap_K(a) <= 5, (IDS[ci], t, "no target at or below the tail's first level")
        cell = geo.idx(*_cell_of(a, int(lvl[0]["bracket"]), int(lvl[0]["bits"]), min(D, int(lvl[0]["level"]))))
        assert cell.size
        drop = cell[np.argsort(np.abs(m[cell]), kind="stable")[cell.size // 2]]
        m2 = m.copy()
        m2[drop] = 0.0
        mut = SR.Chain(geo, m2, a)
        fails["node"] += sum(not SR.follows(mut, r) for r in mine)
    assert not clean_fail, "%s: the clean float64 chain leaves %d of %d probes' paths" % (IDS[ci], len(clean_fail), len(recs))
    assert all(v >= 1 for v in fails["half"].values()), (IDS[ci], fails)
    assert fails["node"] >= 1, (IDS[ci], fails)
    # the one-row mutation moves F at a target by 1e-9 of that row's mass at or below the target's level: a case
    # must see it wherever that is at least two offsets at some probe above its target (sign +).  It is less at
    # every probe of ROW_UNSEEN only: there the tightest bar is (2 nu + 3) 7e-14 = 1.9e-11 and the row holds under
    # 2% of any probe's M
    if seen_row or IDS[ci] not in ROW_UNSEEN:
        assert seen_row and fails["row"] >= 1, (IDS[ci], fails, seen_row)


def _slice_of(case):
    model, copula, dim, params = case[:4]
    m = "msm" if model == "msm" else "gar"
    if copula == "student":
        return "st_%s_%d" % (m, 8 if NC.plan_codes(params[0], dim)[0] == 8 else 0)
    return {"gaussian": "ga_", "plackett": "pl_"}[copula] + m


def test_probes_reach_every_path(kat, probes):
    """Derived from the restated host rules (solve_probe_cases.build_cell_counts, dyadic_walk_ok), not from a run.

    Block-tail targets are classed by the tie group (nodes of equal v*) of the cell at which the probe's
    crossing lies: the target's plateau ends g groups into the cell; a probe below the plateau (sign -) crosses at
    group g, one above it (sign +) at group g + 1.  The two patterns in which every remaining mid decides
    the same way need a node threshold within q = 2^-K of the bracket's width of a cell edge (the decision that
    chose the cell already separates obj' from F at the edge).  The grids have them: their points at exactly
    -5, -2.5, -1, 1, 2.5, 5 and dyadic steps put thresholds on dyadic mids (every mid of the tail then moves
    the lower end up: all tail bits set) and, on the MSM grid at n = 320, an ulp over them (none does: no tail
    bit set).  solve_probe_reference.edge_paths makes such mids targets of their own."""
    from oracle.quadrature import Problem
    seen_slices, generic, tail_pos = set(), set(), set()
    brackets, kinds, signs = set(), set(), set()
    levels_2d128 = set()
    rpt2 = nondyadic = notable = deep3d = onewave = False
    all_up = none_up = 0
    for ci, case in enumerate(CASES):
        rec = SC.probes_of(probes, ci)
        a = SC.solve_kwargs(case[6])
        kw = SC.problem_inputs(case, kat)
        G = Problem(kw["model"], "gaussian", kw["dim"], kw["x_values"], kw["step"], kw["densities"], kw["combos"],
                    kw["weights"], np.zeros(1 if case[2] == 2 else 3), kw["per_date"], kw["unique_vol_states"])
        geo = SR.Geometry(G)                               # (membership needs the grid and the weights only)
        brackets |= set(int(b) for b in rec["bracket"])
        kinds |= set(SC.KINDS[int(k)] for k in rec["kind"])
        signs |= set(int(s) for s in rec["sign"])
        assert set(int(b) for b in rec["bracket"]) == {0, 1, 2, 3}, IDS[ci]
        assert set(int(d) for d in rec["date"]) == {0, 1, 2}, IDS[ci]
        depth, cnt = _tail_depth(geo, case)
        if case[2] == 3:
            # SORTED's block tail takes a cell of at most NT kSortBlk <= 1024 * 8 nodes after the first level
            # (cvq_sorted_kernels.h): both halves of bracket 2 at n = 40 still hold more, so every path into it
            # runs two tabulated levels first
            if case[4] == 40:
                deep3d = deep3d or (min(cnt[1][2]) > 1024 * 8 and bool(np.any((rec["bracket"] == 2) & (rec["level"] >= 2))))
            continue
        seen_slices.add(_slice_of(case))
        if case[5] == "nr1":
            assert {0, 1, 2} == set(int(d) for d in rec["date"])       # deferred (middle) and fast dates in one batch
            generic.add(case[1])
        if case[4] > SC.COMPACT_NT:
            rpt2 = rpt2 or rec["obj"].size > 0
        if case[6] == "nondyadic":
            assert not SC.dyadic_walk_ok(a)
            nondyadic = True
        else:
            assert SC.dyadic_walk_ok(a)
        if case[6] == "coarse":
            assert depth == -1 and SC.snap_K(a) <= 5 and case[4] == SC.N_RPT2
            notable = True
            # without cell tables k_compact counts the bracket's nodes on the device and hands a bracket of at
            # most kTailCap = 64 * 4 nodes to its one-wave tail, if a level is left (cvq_compact_kernels.h:836-837)
            for i in range(rec["obj"].size):
                for k in range(SC.snap_K(a)):
                    if geo.count(*_cell_of(a, int(rec["bracket"][i]), int(rec["bits"][i]), k)) <= 64 * 4:
                        onewave = True
            continue
        # (the MSM grid is denser in its outer parts: one level fewer before its cells fit the tail)
        assert depth == {"garch": {24: 1, 128: 2, 320: 5}, "msm": {24: 1, 128: 1, 320: 4}}[case[0]][case[4]], (IDS[ci], depth)
        if case[4] == 128 and case[0] == "garch":
            levels_2d128 |= set(int(v) for v in rec["level"][rec["kind"] == 2])
        # level targets whose K - depth tail decisions all go one way (COMPACT's block tail; the lane-0 walk too)
        full = (1 << (SC.snap_K(a) - depth)) - 1
        tb = (rec["bits"][rec["kind"] == 2].astype(np.int64) >> depth) & full
        assert np.any(tb == full), IDS[ci]
        all_up += int(np.sum(tb == full))
        none_up += int(np.sum(tb == 0))
        if case[6] != "default":
            continue
        # tail targets: the crossing's tie group within the depth-`depth` cell
        x, w = kw["x_values"], kw["weights"]
        vs = SR.vstar(x, w[0], w[1])[:, 1:]                 # (j = 0 is no member of any slab: Q9)
        for i in np.flatnonzero((rec["kind"] == 2) & (rec["level"] >= depth)):
            lo, hi = _cell_of(a, int(rec["bracket"][i]), int(rec["bits"][i]), depth)
            cell = np.sort(vs[(vs > lo) & (vs <= hi)])
            assert cell.size == geo.count(lo, hi) <= SC.TAIL_CAP
            groups = np.unique(cell)
            below = int(rec["count"][i]) - geo.count(a["lower"], lo)      # the plateau's nodes inside the cell
            g = int(np.searchsorted(np.cumsum([np.sum(cell == v) for v in groups]), below, side="right"))
            cross = g if int(rec["sign"][i]) < 0 else g + 1
            if 1 <= cross <= groups.size:
                tail_pos.add("first" if cross == 1 else ("last" if cross == groups.size else "interior"))
    assert seen_slices == {"st_msm_8", "st_msm_0", "st_gar_8", "st_gar_0", "ga_msm", "ga_gar", "pl_msm", "pl_gar"}
    assert generic == {"student", "plackett"}
    assert brackets == {0, 1, 2, 3} and kinds == set(SC.KINDS) and signs == {-1, 1}
    assert {0, 1} <= levels_2d128 and max(levels_2d128) >= 2          # both kcut levels, then the tail
    assert tail_pos == {"first", "interior", "last"}, tail_pos
    assert all_up >= 1 and none_up >= 1, (all_up, none_up)
    assert rpt2 and nondyadic and notable and deep3d and onewave
