"""The node reference (tests/node_reference.py) and its fixture (tests/golden/node_kat.kat), on the CPU:

  * the fixture is what tests/kat/gen_node_kat.py writes: the points' digests match and a fixed sample
    of every part, regenerated with mpmath, is equal to the stored values;
  * the longdouble slab reference agrees with the float64 oracle within the project's slab bar, 1e-10
    of sum |mass| (measured: up to 7.6e-11, scipy's stdtrit, DESIGN.md §5 -- the gap that bar hides;
    (2 nu + 3) 1e-11 for nu >= 125, where the oracle's own quantile error passes 1e-10: 2.9e-10 measured),
    and with the same arithmetic in float64 on the exact quantiles within 1e-13 (measured 4.9e-14);
  * the reference is well conditioned at every case: moving every u by one ulp moves no slab by more
    than 1e-15 of sum |mass| (measured: up to 9.8e-16; the sigma rows are chosen per case for it,
    node_cases.sigma_rows), or 5e-14 at the stiff copula parameters where none can (node_cases.stiff:
    up to 1.8e-14), so a last-bit difference between the device's erf and the host's stays under 5% of
    the GPU modules' tightest bar;
  * the degree-7 exponentials' documented error is their polynomials' own, recomputed with mpmath;
  * the case matrix reaches every (node_m class, uni_m class) branch of plan creation, computed with a
    Python restatement of the plan rule (cvq_common.h half_power_code).
"""
import importlib.util
import os

import numpy as np
import pytest

import node_cases as NC
import node_reference as NR

_spec = importlib.util.spec_from_file_location("gen_node_kat", NC.GEN_PATH)
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)

CASES = NC.cases()
ORACLE_BAR, CONDITION_BAR = 1e-10, 1e-15
# nu >= 125: the oracle's own quantile error (scipy's stdtrit, 1e-11) times the node
# power's first-order amplification (2 nu + 3) passes 1e-10; the float64 run on exact quantiles shows
# that nothing else separates the two
STDTRIT_ERR = 1e-11
FLOAT64_BAR = 1e-13
# stiff cases (node_cases.stiff): no sigma rows on offer reach 1e-15 (test_stiff_cases_stay_stiff).  What the
# figure protects is the GPU bars: the device's u differs from the host's by at most the last bit of erf, so
# it moves a slab by at most this figure.  The budget given to it there is a twentieth of the tightest GPU
# bar (1e-12) -- a choice, not a derivation: it leaves 95% of every bar to the kernels
STIFF_CONDITION_BAR = 0.05 * 1e-12


@pytest.fixture(scope="module")
def kat():
    return NC.load_kat()


def _problem(kat, case):
    key = NC.ztab_key(case)
    return GEN.build_problem(case, kat, None if key is None else NC.truth(kat, key))


# ------------------------------------------------------------------ fixture <-> generator
def test_points_match_fixture(kat):
    pts = {"exp": NC.exp_points(), "exp2": NC.exp2_points(), "log": NC.log_points(), "logdense": NC.logdense_points(),
           "rcp": NC.rcp_points(), "root6": NC.root_points(), "tppf": NC.tppf_points(),
           "pow": np.concatenate((NC.POW_B, NC.POW_NEG_EX, NC.POW_POS_EX,
                                  [b for m in range(2, 129) for b in NC.overflow_b(m)]))}
    for name, x in pts.items():
        assert NC.digest(x) == str(kat["sha_" + name]), name
        if name not in ("pow", "tppf"):
            assert kat[name + "_hi"].shape == x.shape
            assert x.size >= 1500 or name == "logdense", (name, x.size)    # a few thousand points per helper
    assert kat["tppf_hi"].shape == (len(NC.NUS_KAT), pts["tppf"].size) and kat["tppf_hi"].size >= 3000
    assert kat["pow_neg_hi"].shape == (len(NC.POW_NEG_EX), NC.POW_B.size) and kat["pow_neg_hi"].size >= 2000
    assert os.path.getsize(NC.KAT_PATH) < 512 * 1024


def _same(kat, name, idx, vals):
    hi, lo = GEN.pack(vals)
    assert np.array_equal(hi, kat[name + "_hi"][idx], equal_nan=True), name
    assert np.array_equal(lo, kat[name + "_lo"][idx], equal_nan=True), name


def test_primitive_sample_regenerates(kat):
    for name, x, f in (("exp", NC.exp_points(), GEN.prim_exp), ("exp2", NC.exp2_points(), GEN.prim_exp2),
                       ("log", NC.log_points(), GEN.prim_log), ("logdense", NC.logdense_points(), GEN.prim_log),
                       ("rcp", NC.rcp_points(), GEN.prim_rcp), ("root6", NC.root_points(), GEN.prim_root6)):
        idx = np.unique(np.concatenate((np.arange(0, x.size, 37), [x.size - 1])))
        _same(kat, name, idx, f(x[idx]))
    for name, exs, rows in (("pow_neg", NC.POW_NEG_EX, (0, 1, 8, 9, 127, 128, 129, 130, 131)),
                            ("pow_pos", NC.POW_POS_EX, (0, 7, 16, 17, 18))):
        for r in rows:
            _same(kat, name, r, GEN.prim_pow(NC.POW_B, [exs[r]])[0])
    trip = GEN.prim_pow_trip()
    _same(kat, "pow_trip", np.arange(len(trip)), trip)
    u = NC.tppf_points()
    idx = np.unique(np.concatenate((np.arange(0, u.size, 17), np.arange(u.size - 6, u.size))))
    for i, nu in enumerate(NC.NUS_KAT):
        _same(kat, "tppf", (i, idx), GEN.prim_tppf(u[idx], nu))


def test_t_ppf_against_closed_forms():
    """nu = 1: t = -cot(pi u); nu = 2: t = (2u - 1) / sqrt(2 u (1 - u)) -- the root-finder itself."""
    import mpmath as mp
    for u in (1e-300, 1e-17, 0.01, 0.05, 0.3, 0.499999, 0.7, 1 - 2.0 ** -53):
        um = mp.mpf(u)
        t1 = NR.t_ppf(u, 1.0)
        assert abs(t1 / (-mp.cot(mp.pi * um)) - 1) < mp.mpf(10) ** -40 if u < 0.5 else \
            abs(t1 / mp.cot(mp.pi * (1 - um)) - 1) < mp.mpf(10) ** -40
        t2 = NR.t_ppf(u, 2.0)
        assert abs(t2 / ((2 * um - 1) / mp.sqrt(2 * um * (1 - um))) - 1) < mp.mpf(10) ** -30


SAMPLE = [i for i, c in enumerate(CASES) if NC.case_id(c) in (
    "garch-student-2d-5.364_0.5", "garch-student-3d-126_0.9_0.9_0.85", "garch-gaussian-2d-0.99",
    "garch-plackett-2d-1.00000000093", "msm-student-2d-1_0.5", "msm-student-3d-5_0.5_0.4_0.3",
    "msm-gaussian-3d-0.9_0.9_0.85", "msm-plackett-2d-50")]


def test_sample_ids_exist():
    assert len(SAMPLE) == 8


@pytest.mark.parametrize("i", SAMPLE, ids=[NC.case_id(CASES[i]) for i in SAMPLE])
def test_slab_sample_regenerates(kat, i):
    """From scratch: mpmath quantiles of the oracle's u tables, then the longdouble sums."""
    case = CASES[i]
    if case[0] == "msm" and case[2] == 2 and case[1] == "student":      # the stored MSM inputs are the oracle's
        fbs, pi, uvs = GEN.msm_inputs(2)
        assert np.array_equal(fbs, kat["msm2_fbs"]) and np.array_equal(pi, kat["msm2_pi"])
        assert np.array_equal(uvs, kat["msm2_uvs"])
    P = GEN.build_problem(case, kat, None)
    key = NC.ztab_key(case)
    if key is not None:
        zt = P.quantile_tables()
        hi = zt.astype(np.float64)
        assert np.array_equal(hi, kat[key + "_hi"])
        lo = ((zt - hi.astype(np.longdouble)).astype(np.float64) / np.where(hi != 0, hi, 1.0)).astype(np.float32)
        assert np.array_equal(lo, kat[key + "_lo"])
        P._z = NC.truth(kat, key)
    m0, m1, sc, sc1, mx, scx, cnt, scb = GEN.slab_rows(P, case[2])
    assert np.all(scb >= sc)
    for name, v in (("m0", m0), ("m1", m1), ("scale", sc), ("scale1", sc1), ("mx", mx), ("scalex", scx),
                    ("scale_below", scb)):
        assert np.array_equal(v, kat[name][i]), name
    assert np.all((cnt[3] >= 1) & (cnt[3] <= 8)), "the narrow slab holds a handful of nodes"
    assert np.all(cnt[:3] > cnt[3])


# ------------------------------------------------------------------ every case
@pytest.mark.parametrize("i", range(len(CASES)), ids=[NC.case_id(c) for c in CASES])
def test_reference_against_oracle_and_conditioning(kat, i):
    case = CASES[i]
    P = _problem(kat, case)
    sl = NC.slabs(case[2])
    r = P.slab_moments(sl)
    assert np.array_equal(r["m0"], kat["m0"][i]) and np.array_equal(r["scale"], kat["scale"][i])
    assert np.array_equal(r["mx"], kat["mx"][i][..., :case[2]]) and np.array_equal(r["m1"], kat["m1"][i])
    assert np.all(r["scale"] > 0.0) and np.all(r["count"] >= 1)
    oracle = np.array([[P.slab(t, a, b) for t in range(P.T)] for a, b in sl])
    gap = float(np.max(np.abs(oracle - r["m0"]) / r["scale"]))
    cond = P.conditioning(sl)
    P.ftype = np.float64                      # the same arithmetic in float64 on the rounded mpmath quantiles
    f64 = P.slab_moments(sl)
    P.ftype = NR.LD
    own = float(np.max(np.abs(f64["m0"] - r["m0"]) / r["scale"]))
    print(f"MEASURED {NC.case_id(case)} oracle gap {gap:.2e} of scale, one-ulp conditioning {cond:.2e} of scale, "
          f"float64 arithmetic on exact quantiles {own:.2e} of scale")
    nu = case[3][0] if case[1] == "student" else 0.0
    assert own <= FLOAT64_BAR + (2 * nu + 3) * 2.0 ** -52
    assert gap <= (ORACLE_BAR if nu < 125.0 else (2 * nu + 3) * STDTRIT_ERR)
    assert cond <= (STIFF_CONDITION_BAR if NC.stiff(*case) else CONDITION_BAR)


STIFF_GARCH = [i for i, c in enumerate(CASES) if c[0] == "garch" and NC.stiff(*c)]


@pytest.mark.parametrize("i", STIFF_GARCH, ids=[NC.case_id(CASES[i]) for i in STIFF_GARCH])
def test_stiff_cases_stay_stiff(kat, i, monkeypatch):
    """The looser conditioning bar is not a matter of the sigma rows: under every candidate row set the
    figure stays above 1e-15 (and the rows in use are among the candidates)."""
    case = CASES[i]
    dim = case[2]
    figures = []
    for rows in NC.SIGMA_CANDIDATES[dim]:
        monkeypatch.setattr(NC, "sigma_rows", lambda *a, rows=rows: rows)
        figures.append(GEN.build_problem(case, kat, None).conditioning(NC.slabs(dim)))
    monkeypatch.undo()
    print(f"MEASURED {NC.case_id(case)} conditioning per candidate row set", ["%.2e" % f for f in figures])
    assert any(NC.sigma_rows(*case[1:]) is rows for rows in NC.SIGMA_CANDIDATES[dim])
    assert min(figures) > CONDITION_BAR


# ------------------------------------------------------------------ coverage of the plan's branches
def test_case_matrix_reaches_every_power_class():
    by_dim = {2: set(), 3: set()}
    codes = {2: set(), 3: set()}
    for model, copula, dim, params in CASES:
        if copula == "student":
            by_dim[dim].add(NR.code_class(params[0], dim))
            codes[dim].add(NR.plan_codes(params[0], dim))
    # 2-D: odd / even node power with the other parity's univariate power; both general (fitted nu);
    # DIRECT's node_m 8 and 9; an integer node power with a general univariate one (nu = 16, 30, 126)
    assert {("odd", "even"), ("even", "odd"), ("general", "general"), ("d8", "odd"), ("d9", "even"),
            ("even", "general")} <= by_dim[2]
    assert {("even", "even"), ("odd", "odd"), ("general", "general"), ("even", "general")} <= by_dim[3]
    for dim in (2, 3):
        node = {c[0] for c in codes[dim]}
        assert 128 in node and -1 in node                       # the 128 limit met exactly ...
    assert NR.plan_codes(127.0, 2)[0] == -1 and NR.plan_codes(126.0, 2)[0] == 128     # ... and passed by one,
    assert NR.plan_codes(126.0, 3)[0] == -1 and NR.plan_codes(125.0, 3)[0] == 128     # differently in 2-D and 3-D
    uni = {c[1] for d in codes for c in codes[d]}
    assert 16 in uni and NR.plan_codes(16.0, 2) == (18, -1)     # the 16 limit met (nu = 15) and passed (nu = 16)
    assert (9, 7) in codes[3]                                   # SORTED's 3-D nu = 6 instance (PM = DIM + 6)
    for model in ("garch", "msm"):
        for copula in ("student", "gaussian", "plackett"):
            assert any(c[0] == model and c[1] == copula for c in CASES)


def test_plan_rule_restated():
    assert NR.half_power_code(8.0, 128.0) == 8 and NR.half_power_code(7.364, 128.0) == -1
    assert NR.half_power_code(128.0, 128.0) == 128 and NR.half_power_code(129.0, 128.0) == -1
    assert NR.half_power_code(16.0, 16.0) == 16 and NR.half_power_code(17.0, 16.0) == -1
    assert NR.half_power_code(0.0, 16.0) == 0


# ------------------------------------------------------------------ the polynomials' own error
def _poly_of(fn):
    """Horner coefficients of a cvq_special.h exponential, highest degree first, from its source."""
    import re
    src = open(os.path.join(os.path.dirname(NC.GEN_PATH), "..", "..", "copula-msm-and-copula-garch-var_amd",
                            "csrc", "cvq_special.h")).read()
    body = src[src.index("double %s(double x) {" % fn):]
    body = body[:body.index("return")]
    first = re.search(r"double p = ([0-9.e+-]+);", body).group(1)
    return [float(first)] + [float(c) for c in re.findall(r"p = fma\(p, [rt], ([0-9.e+-]+)\);", body)]


@pytest.mark.parametrize("fn,degree,claim,base2", [("exp_node", 9, 1.4e-14, False), ("exp_node7", 7, 4.05e-11, False),
                                                    ("exp2_node7", 7, 4.05e-11, True)])
def test_exponentials_documented_error_is_the_polynomials(fn, degree, claim, base2):
    """max |p(r) / exp(r) - 1| over the reduced interval, in exact arithmetic on the float64
    coefficients: the figure the comments carry and the GPU modules use as the bar."""
    import mpmath as mp
    c = _poly_of(fn)
    assert len(c) == degree + 1
    half = mp.mpf(1) / 2 if base2 else mp.log(2) / 2
    worst = mp.mpf(0)
    for i in range(2001):
        r = -half + 2 * half * i / 2000
        p = mp.mpf(c[0])
        for a in c[1:]:
            p = p * r + mp.mpf(a)
        worst = max(worst, abs(p / (mp.power(2, r) if base2 else mp.exp(r)) - 1))
    print(f"MEASURED {fn} polynomial error {mp.nstr(worst, 5)} (documented {claim})")
    assert 0.9 * claim <= worst <= claim
