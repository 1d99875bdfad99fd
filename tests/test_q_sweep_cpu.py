"""The q sweep's fixture (tests/golden/q_sweep.kat) and case matrix (tests/q_sweep_cases.py) on the CPU, next
to test_node_reference_ext_cpu.py:

  * the fixture is what tests/kat/gen_q_sweep.py writes: every case's input digest matches q_sweep_cases, the
    MSM inputs of every q and a sample of cases (every kind, q = 1 and q = 8, both dimensions, the nr1 variant)
    regenerate bit-equal; q = 3 is node_kat.kat's own inputs, and the q = 3 truths are node_kat.kat's;
  * the matrix holds every q in 1 ... 8 for every kind and dimension it lists;
  * the float64 checker of every case agrees with the stored truths at the bar it is documented to meet: the
    oracle Problem 1e-10 of sum |mass| (scipy's stdtrit: test_node_slabs_gpu.py's header), the Gumbel and
    product-form checkers 1e-13 (test_node_reference_ext_cpu.py's CHECKER_BAR);
  * the solve premise of tests/test_q_sweep_gpu.py's check (e): on every Student nu = 6 and Gaussian case the
    oracle's calc_var (at q_sweep_cases.OBJ_VAR[dim]) runs a genuine bisection, is the fixture's, keeps its VaR
    and iteration count when every integral is scaled by 1 +- 1e-7, and at no level decides the Q4 break on a
    rounding residue of a true 0 -- which the default target 0.05 does in 3-D, asserted too;
  * what the GPU module relies on: every slab keeps a member and a positive scale, under the candidate weights
    and on the alternative date too; the stress event cuts the wide slabs; the alternative date differs from
    the plan's own; the Gumbel bars stay under 1e-11 (precise) and 5e-11 (fast).
"""
import importlib.util

import numpy as np
import pytest

import node_cases as NC
import q_sweep_cases as QC

_spec = importlib.util.spec_from_file_location("gen_q_sweep", QC.GEN_PATH)
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)

CASES = QC.cases()
IDS = [QC.case_id(c) for c in CASES]
ORACLE_BAR, CHECKER_BAR = 1e-10, 1e-13
MARGIN = 1e-7


@pytest.fixture(scope="module")
def z():
    return QC.load_kat()


# ------------------------------------------------------------------ the matrix
def test_matrix_holds_every_q():
    assert QC.QS == (1, 2, 3, 4, 5, 6, 7, 8)
    assert not QC.missing_q(CASES)
    listed = {("student", 2), ("student", 3), ("gaussian", 2), ("gaussian", 3), ("plackett", 2), ("gumbel_survival", 2),
              ("gumbel_survival", 3), ("frank", 2), ("frank", 3), ("joe_survival", 2), ("joe_survival", 3)}
    assert {(c, d) for c, d, _ in QC.full_sweeps()} == listed
    for copula, dim in listed:
        for q in QC.QS:
            assert any(c[0] == copula and c[1] == dim and c[3] == q and c[4] == "" for c in CASES), (copula, dim, q)
    # a trimmed matrix is noticed
    assert QC.missing_q([c for c in CASES if c[3] != 6]) and QC.missing_q(CASES[1:])
    # the fitted nu (the general power) at q = 4 and the default branch; the nr1 variant at the kQUnroll edge
    for dim in (2, 3):
        assert {c[3] for c in CASES if c[0] == "student" and c[2][0] == QC.FITTED_NU and c[1] == dim} == {4, 8}
    assert [c[:2] + c[3:] for c in CASES if c[4] == "nr1"] == [("student", 2, 8, "nr1"), ("gumbel_survival", 3, 8, "nr1"),
                                                             ("frank", 2, 8, "nr1")]
    assert len(CASES) == 95 and len(set(IDS)) == 95
    assert NC.plan_codes(6.0, 2)[0] == 8 and NC.plan_codes(QC.FITTED_NU, 2)[0] < 0      # k_direct's PM = 8 and PM = 0


# ------------------------------------------------------------------ fixture <-> generator
def test_digests_match_fixture(z):
    assert z["sha_case"].shape == (len(CASES),)
    for i, case in enumerate(CASES):
        assert QC.case_digest(case, z) == str(z["sha_case"][i]), IDS[i]
    assert len(set(z["sha_case"].tolist())) == len(CASES)
    import os
    assert os.path.getsize(QC.KAT_PATH) < 300 * 1024


def test_msm_inputs_regenerate(z):
    kat = NC.load_kat()
    for dim in (2, 3):
        for q in QC.QS:
            k = QC.msm_key(dim, q)
            fbs, pi, uvs = GEN.msm_inputs(dim, q)
            assert np.array_equal(fbs, z[k + "_fbs"]) and np.array_equal(pi, z[k + "_pi"]) and np.array_equal(uvs, z[k + "_uvs"])
            assert uvs.shape == (dim, q) and np.all(np.diff(uvs, axis=1) > 0.0)
            assert np.all(np.abs(pi.sum(axis=1) - 1.0) <= 1e-12) and np.all(pi > 0.0)
        for s in ("_fbs", "_pi", "_uvs"):
            assert np.array_equal(z[QC.msm_key(dim, 3) + s], kat["msm%d" % dim + s]), "q = 3 is node_kat.kat's own"
        # q = 1: one state, every date's probability vector is 1
        k = QC.msm_key(dim, 1)
        assert np.all(z[k + "_fbs"] == 1.0) and np.all(z[k + "_pi"] == 1.0)
    # (the unique-state map rounds a state to a multiple of 1e-6: within an ulp or two of cfg 2 / cfg 4's sigma)
    assert np.all(np.abs(z["msm2_q1_uvs"] - 1.2) <= 1e-15) and np.all(np.abs(z["msm3_q1_uvs"] - 1.2) <= 1e-15)


def test_q3_truths_are_the_base_fixture_s(z):
    """The q = 3 Student, Gaussian and Plackett cases are cases of node_cases.cases(): the same truths."""
    kat = NC.load_kat()
    base = [NC.case_id(c) for c in NC.cases()]
    n = 0
    for i, case in enumerate(CASES):
        copula, dim, params, q, variant = case
        if q == 3 and variant == "" and copula in ("student", "gaussian", "plackett"):
            j = base.index(NC.case_id(("msm", copula, dim, params)))
            for k in ("m0", "m1", "scale", "scale1", "mx", "scalex", "scale_below"):
                assert np.array_equal(z[k][i], kat[k][j]), (IDS[i], k)
            n += 1
    assert n == 5


SAMPLE_IDS = ("student-2d-6_0.5-q1", "student-3d-5.364_0.5_0.4_0.3-q8", "gaussian-3d-0.5_0.4_0.3-q1", "gaussian-2d-0.5-q5",
              "plackett-2d-1.5-q8", "gumbel_survival-2d-4-q1", "gumbel_survival-3d-4-q8-nr1", "frank-3d-6-q8",
              "joe_survival-2d-2-q1", "joe_survival-3d-2-q8", "student-2d-6_0.5-q8-nr1")
SAMPLE = [IDS.index(s) for s in SAMPLE_IDS]


def test_sample_covers_the_matrix():
    got = [CASES[i] for i in SAMPLE]
    assert {c[0] for c in got} == {c[0] for c in CASES}
    assert {(c[1], c[3]) for c in got} >= {(2, 1), (3, 1), (2, 8), (3, 8)}
    assert any(c[0] == "student" and c[2][0] == QC.FITTED_NU for c in got) and any(c[4] == "nr1" for c in got)


@pytest.mark.parametrize("i", SAMPLE, ids=SAMPLE_IDS)
def test_sample_regenerates(z, i):
    rows = GEN.case_rows(CASES[i], z)
    assert {"m0", "m1", "scale", "scale1", "scale_below", "count", "mx", "scalex", "ebound", "ebound1", "ebound_fast",
            "eboundx", "m0_event", "scale_event", "p_event", "m0_port", "scale_port", "alt_m0", "alt_m1", "alt_scale",
            "alt_scale1", "solve_var", "solve_it"} <= set(rows)
    for k, a in rows.items():
        assert a.dtype == z[k].dtype and np.array_equal(a, z[k][i], equal_nan=True), k
    assert set(rows) | {"sha_case"} == {k for k in z if not k.startswith("msm")}


# ------------------------------------------------------------------ every case
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_checker_against_truths_and_populated(z, i):
    case = CASES[i]
    copula, dim, params, q, variant = case
    P = GEN.oracle_problem(case, z)
    sl = NC.slabs(dim)
    oracle = np.array([[P.slab(t, a, b) for t in range(P.T)] for a, b in sl])
    gap = float(np.max(np.abs(oracle - z["m0"][i]) / z["scale"][i]))
    print(f"MEASURED {IDS[i]} checker gap {gap:.2e} of scale, narrow slab members {z['count'][i, 3].tolist()}")
    assert gap <= (ORACLE_BAR if copula in ("student", "gaussian", "plackett") else CHECKER_BAR)
    # what the GPU module relies on
    assert np.all(z["scale"][i] > 0.0) and np.all(z["count"][i] >= 1) and np.all(z["scale_below"][i] >= z["scale"][i])
    assert np.all(z["count"][i][:3] > z["count"][i][3]), "the narrow slab holds fewer nodes than the others"
    assert np.all(z["count_port"][i] >= 1) and np.all(z["scale_port"][i] > 0.0)
    assert np.all(z["alt_count"][i] >= 1) and np.all(z["alt_scale"][i] > 0.0) and np.all(z["alt_scale1"][i] > 0.0)
    assert not np.any(z["alt_m0"][i] == z["m0"][i][:, QC.ALT_DATE]), "the alternative date is another measure"
    ce = z["count_event"][i]
    assert np.all(z["p_event"][i] > 0.0) and np.all(ce <= z["count"][i])
    assert np.all(ce[:2] >= 1) and np.any(ce[:3] < z["count"][i][:3]), "the stress event cuts the wide slabs"
    assert np.all(z["m0_event"][i][ce == 0] == 0.0) and np.all(z["scale_event"][i][ce == 0] == 0.0)
    if copula in QC.GUMBEL_KINDS:
        for k in ("ebound", "ebound1", "ebound_port", "alt_ebound", "alt_ebound1", "ebound_pevent"):
            assert np.all(z[k][i] > 0.0) and NC.gumbel_bar(z[k][i], "precise").max() < 1e-11, k
        assert NC.gumbel_bar(z["eboundx"][i], "precise").max() < 1e-11 and np.all(z["ebound_event"][i][ce > 0] > 0.0)
        assert NC.EXP7_BAR < NC.gumbel_bar(z["ebound_fast"][i], "fast").max() < 5e-11
    else:
        for k in ("ebound", "ebound1", "ebound_fast", "eboundx", "ebound_event", "ebound_pevent", "ebound_port",
                  "alt_ebound", "alt_ebound1"):
            assert not np.any(z[k][i]), k


SOLVE = [i for i, c in enumerate(CASES) if QC.solve_case(c)]


def test_solve_cases():
    got = [CASES[i] for i in SOLVE]
    assert len(SOLVE) == 33 and all(c[0] in ("student", "gaussian") for c in got)
    for copula in ("student", "gaussian"):
        for dim in (2, 3):
            assert {c[3] for c in got if c[0] == copula and c[1] == dim and c[4] == ""} == set(QC.QS)


def _solve(P, obj_var, factor=1.0):
    """(var, iterations, broke, zero margin): the oracle's calc_var on integrals scaled by factor; the margin is
    the least, over the bisection levels, of max over dates |F| / (|prev| + |slab|) -- how far the Q4 rule
    (break when every date's F is exactly 0) is from firing."""
    from oracle.quadrature import calc_var
    trace = {}
    var, it, broke = calc_var(lambda bounds: P.compute_integral(bounds) * factor, P.T, 0.0, obj_var=obj_var, trace=trace)
    zero = min((float(np.max(np.abs(rc) / (np.abs(prev) + np.abs(slab)))) for prev, slab, rc in trace.get("steps", [])),
               default=0.0)
    return var, it, broke, zero


@pytest.mark.parametrize("i", SOLVE, ids=[IDS[i] for i in SOLVE])
def test_solve_premise(z, i):
    """Check (e) of the GPU module compares VaR and iteration count with np.array_equal; its premise: the
    oracle's decisions do not change when every integral it sees is scaled by 1 +- 1e-7 (1000 x the slab bar),
    and no level's F is a rounding residue of a true 0 (q_sweep_cases' header)."""
    P = GEN.oracle_problem(CASES[i], z)
    obj = QC.OBJ_VAR[CASES[i][1]]
    var, it, broke, zero = _solve(P, obj)
    print(f"MEASURED {IDS[i]} VaR {var.tolist()} after {it} iterations, zero margin {zero:.1e}")
    assert not broke and it >= 19 and np.all(np.isfinite(var)), "a genuine bisection"
    assert it == int(z["solve_it"][i]) and np.array_equal(var, z["solve_var"][i])
    assert zero >= MARGIN, "premise: a level's F within 1e-7 of zero on every date"
    for f in (1.0 - MARGIN, 1.0 + MARGIN):
        v, n, b, _ = _solve(P, obj, f)
        assert n == it and not b and np.array_equal(v, var), ("premise: decision margin below 1e-7", f)


def test_default_target_is_degenerate_in_3d(z):
    """Why OBJ_VAR[3] is not the default 0.05: there the first midpoint of the 3-D cases (q <= 7 under Student,
    q <= 4 under Gaussian; the first four are asserted) lies under the grid, and what decides the Q4 break is a
    rounding residue."""
    assert QC.OBJ_VAR == {2: 0.05, 3: 1.0}
    for i in SOLVE:
        if CASES[i][1] == 3 and CASES[i][3] <= 4:
            assert _solve(GEN.oracle_problem(CASES[i], z), 0.05)[3] < 1e-12, IDS[i]


def test_no_solve_truth_elsewhere(z):
    rest = [i for i in range(len(CASES)) if i not in SOLVE]
    assert np.all(z["solve_it"][rest] == -1) and np.all(np.isnan(z["solve_var"][rest]))
