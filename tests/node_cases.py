"""Inputs of the node known-answer tests, shared by tests/kat/gen_node_kat.py (which adds the
mpmath truths), tests/test_node_reference_cpu.py and the two GPU modules: the primitives' points
and the slab case matrix.  Everything here is built from exact float64 arithmetic (linspace,
ldexp, nextafter), so every machine regenerates the same inputs; the fixture carries their SHA-256
and the tests compare it.  No mpmath here: the GPU tests read only this module and the fixture."""
import hashlib
import os

import numpy as np

# the fixture: binary test vectors, which this repository keeps under tests/golden/ and nowhere else; it is
# an .npz container but not a golden case, and conftest lists every *.npz there as one: hence its extension
KAT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_kat.kat")
GEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat", "gen_node_kat.py")
LN2 = 0.6931471805599453
INF, NAN = float("inf"), float("nan")
TINY = 2.0 ** -1074                       # one subnormal ulp
MIN_NORMAL = 2.0 ** -1022


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def load_kat():
    return dict(np.load(KAT_PATH, allow_pickle=False))


def truth(z, name):
    """longdouble truths of primitive `name`: hi + hi * lo_rel (lo kept relative, float32)."""
    hi = z[name + "_hi"].astype(np.longdouble)
    with np.errstate(invalid="ignore"):
        return hi + np.where(np.isfinite(hi), hi * z[name + "_lo"].astype(np.longdouble), 0.0)


def _around(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate((np.nextafter(v, -INF), v, np.nextafter(v, INF)))


def _spread(e_lo, e_hi, e_step, n_mant):
    m = np.linspace(1.0, 2.0, n_mant, endpoint=False)
    e = np.arange(e_lo, e_hi + 1, e_step)
    return np.ldexp(m[None, :], e[:, None]).ravel()


# ------------------------------------------------------------------ primitives' points
def exp_points():
    """exp_node / exp_node7: dense over [-745, 709]; both sides of the reduction boundaries
    (k +- 1/2) ln2; the subnormal-result range; x < -1075 (exactly 0); NaN."""
    k = np.arange(-1074, 1024, 37).astype(np.float64)
    return np.concatenate((np.linspace(-745.0, 709.0, 1455), _around((k + 0.5) * LN2), _around((k - 0.5) * LN2),
                           np.linspace(-745.13, -708.4, 200), _around([0.0]), [709.78],
                           [-1075.5, -1076.0, -1100.0, -2000.0, -1.0e5, -1.0e8, NAN]))


def exp2_points():
    """exp2_node7: the same in base 2; exact integers; half-integers +- 1 ulp."""
    k = np.arange(-1074, 1024, 7).astype(np.float64)
    h = np.arange(-1074, 1023, 29).astype(np.float64) + 0.5
    return np.concatenate((np.linspace(-1074.0, 1023.9, 1400), k, _around(h), np.linspace(-1074.9, -1021.0, 150),
                           [-1075.6, -1076.0, -1100.0, -2000.0, -1.0e6, NAN]))


SQRT_HALF = 0.7071067811865476


def log_points():
    """log_node: [1e-300, 1e300]; 1 +- {1 ulp, 1e-12, 1e-8, 1e-4}; both sides of the sqrt(1/2) fold
    at several exponents; powers of two; the smallest normal and subnormals."""
    near1 = [np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)] + [1.0 + s * d for d in (1e-12, 1e-8, 1e-4)
                                                                 for s in (-1.0, 1.0)] + [1.0]
    fold = np.concatenate([np.ldexp(_around([SQRT_HALF]), e) for e in (-1000, -500, -1, 0, 1, 2, 3, 500, 1000)])
    return np.concatenate((_spread(-996, 996, 8, 6), near1, fold, np.ldexp(1.0, np.arange(-1022, 1024, 31)),
                           [MIN_NORMAL, np.nextafter(MIN_NORMAL, 1.0), TINY, 3 * TINY, 2.0 ** -1060 * 1.5,
                            np.nextafter(MIN_NORMAL, 0.0), 1.0e-300, 1.0e300]))


def logdense_points():
    """log_node_fast's working range, dense: the node power's base b in [1, 2^21) (log_node_fast is
    also run on every log_points() b >= 1, its stated domain)."""
    return _spread(0, 20, 1, 64)


def rcp_points():
    """fast_rcp: r > 0 across the exponent range (the last three give subnormal results)."""
    return np.concatenate((_spread(-1022, 1021, 17, 16), [1.0, 3.0, 1.0e300, 2.0 ** 1022 * 1.5, 2.0 ** 1023,
                                                           2.0 ** 1023 * 1.75]))


def root_points():
    """root_nu<6>: p in (0, 1]; p = 2^(6k), 2^(6k +- 1); subnormal p."""
    k = np.arange(-170, 1)
    sixes = np.concatenate([np.ldexp(1.0, 6 * k + d) for d in (-1, 0, 1)])
    sixes = sixes[(sixes > 0.0) & (sixes <= 1.0)]
    return np.concatenate((_spread(-1021, -1, 11, 12), sixes, [1.0, np.nextafter(1.0, 0.0), 0.5, 0.05, TINY, 3 * TINY,
                                                              2.0 ** -1060 * 1.5, np.nextafter(MIN_NORMAL, 0.0)]))


# the node power's bases: [1, 1e6]
POW_B = np.array([1.0, np.nextafter(1.0, 2.0), 1.0001, 1.0625, 1.3, 1.5, 2.0, 2.75, 3.3, 5.0, 10.0, 31.7, 97.3, 1.0e3,
                  12345.678, 1.0e5, 1.0e6])
EX_NONINT = (-3.682, -64.5, -3.182)       # nu = 5.364: node (2-D) and uni exponents; nu = 127, 2-D: node_m = 129 > 128
POW_NEG_EX = tuple(-m / 2.0 for m in range(129)) + EX_NONINT
POW_POS_EX = tuple(m / 2.0 for m in range(18)) + (3.182,)
OVERFLOW_R = 1.0e300                      # pow_node / pow_half_neg: b^(m/2) >= 1e300 -> 0


def overflow_b(m):
    """(below, above): bases on both sides of the first b with b^(m/2) >= 1e300 (m >= 2), 1e-6 apart
    in relative terms -- far outside the squarings' rounding, so the rule's outcome is certain."""
    b = 10.0 ** (600.0 / m)
    return b * (1.0 - 1.0e-6), b * (1.0 + 1.0e-6)


NUS_KAT = (1.0, 2.0, 2.5, 3.0, 5.364, 6.0, 15.0, 16.0, 30.0, 126.0)
P_SPLIT = 0.05                            # cvq_plan.hip build_timage


def tppf_points():
    """stdtrit_tab_bf / stdtrit_tab_int<6>: u in [1e-300, 1 - 2^-53], dense around p_split on both
    sides, 0.5 +- ulp; then 0, 1 and out-of-range inputs (the last five)."""
    tail = np.ldexp(np.array([1.0, 1.37, 1.81])[None, :], np.arange(-996, -4, 16)[:, None]).ravel()
    split = np.concatenate([[P_SPLIT + s * d for d in (1e-15, 1e-12, 1e-9, 1e-6, 1e-3) for s in (-1.0, 1.0)],
                            _around([P_SPLIT]), np.linspace(0.04, 0.06, 41)])
    lower = np.concatenate(([1.0e-300, 1.0e-100, 1.0e-17], tail, split, np.linspace(0.06, 0.5, 45), _around([0.5])))
    lower = lower[(lower > 0.0) & (lower < 1.0)]
    upper = np.concatenate((1.0 - split, 1.0 - np.ldexp(1.0, -np.arange(2, 54, 3)), np.linspace(0.5, 1.0, 23)[1:-1],
                            [1.0 - 2.0 ** -53]))
    return np.concatenate((lower, upper, [0.0, 1.0, -0.1, 1.5, NAN]))


# ------------------------------------------------------------------ plan rule (cvq_common.h half_power_code)
def half_power_code(m, limit):
    m = float(m)
    return int(m) if (m == np.floor(m) and m <= limit) else -1


def plan_codes(nu, dim):
    """(node_m, uni_m) as cvq_plan_create sets them for a Student copula."""
    nu = float(nu)
    node_ex = -(nu + dim) / 2
    return half_power_code(-2.0 * node_ex, 128.0), half_power_code(nu + 1, 16.0)


def code_class(nu, dim):
    """The branch a (nu, dim) takes: node power class x univariate power class, plus DIRECT's
    specialisations (node_m 8 and 9, cvq_plan.hip launch_direct_c) and the nu = 6 table path."""
    nm, um = plan_codes(nu, dim)
    node = "general" if nm < 0 else ("d%d" % nm if dim == 2 and nm in (8, 9) else ("odd" if nm & 1 else "even"))
    uni = "general" if um < 0 else ("odd" if um & 1 else "even")
    return node, uni


# ------------------------------------------------------------------ slab cases
# GARCH / UKF sigma forecasts, one row per date.  |x| / sigma reaches 8 in the first set; a float64 u is
# then within 6e-16 of 1 and one ulp of it is a sixth of the tail.  Where the copula puts mass on
# such nodes (negative dependence: u -> 1 against v -> 0 lies inside the slabs) or has a pole near
# them (the reference's Plackett form, quirk Q11: 1 + (theta - 1)(1 - u - v) -> 0), milder rows are
# chosen so that the reference alone meets the conditioning bar of tests/test_node_reference_cpu.py.
SIGMA_2D = np.array([[1.0, 1.3], [0.7, 0.9], [2.0, 0.625]])
SIGMA_3D = np.array([[1.0, 1.3, 0.8], [0.7, 0.9, 1.1], [2.0, 0.625, 1.0]])
SIGMA_2D_MILD = np.array([[1.0, 1.3], [1.25, 1.6], [2.0, 1.7]])
SIGMA_2D_EQUAL = np.array([[1.0, 1.0], [1.5, 1.5], [2.0, 2.0]])


def sigma_rows(copula, dim, params):
    if dim == 3:
        return SIGMA_3D
    if copula == "plackett":
        return SIGMA_2D_EQUAL if params[0] >= 6.0 else (SIGMA_2D_MILD if params[0] < 1.0 else SIGMA_2D)
    return SIGMA_2D_MILD if params[-1] == -0.9 else SIGMA_2D


SIGMA_CANDIDATES = {2: (SIGMA_2D, SIGMA_2D_MILD, SIGMA_2D_EQUAL, np.array([[1.1, 1.2], [1.4, 1.3], [1.9, 2.1]]),
                        np.array([[0.9, 1.0], [1.2, 1.1], [1.6, 1.5]]), np.array([[1.0, 2.0], [2.0, 1.0], [1.5, 2.5]])),
                    3: (SIGMA_3D, np.array([[1.0, 1.3, 1.1], [1.25, 1.6, 1.4], [2.0, 1.7, 1.2]]),
                        np.array([[1.0, 1.0, 1.0], [1.5, 1.5, 1.5], [2.0, 2.0, 2.0]]))}


def stiff(model, copula, dim, params):
    """Cases whose one-ulp conditioning figure stays above 1e-15 of the slab's sum |mass| for every
    marginal input on offer: Gaussian rho = -0.9, the near-singular 3-D matrix under a Gaussian or
    nu >= 125 copula, Plackett theta = 50 (its pole, quirk Q11) -- for GARCH under every row set of
    SIGMA_CANDIDATES (tests/test_node_reference_cpu.py asserts it), for MSM, whose marginal inputs
    are the filter's and not chosen, also Plackett theta = 6."""
    if copula == "plackett":
        return params[0] >= (6.0 if model == "msm" else 50.0)
    near_singular = dim == 3 and tuple(params[-3:]) == R3["near_singular"]
    if copula == "gaussian":
        return near_singular or (dim == 2 and params[0] == -0.9)
    return near_singular and params[0] >= 125.0


N_OF = {2: 24, 3: 12}
T = 3
NARROW = (-2.55, -2.5)                    # 2 to 4 member nodes on all four grids (asserted in the CPU module)
R3 = {"mild": (0.5, 0.4, 0.3), "near_singular": (0.9, 0.9, 0.85)}
# (nu = 7: node_m = 9, DIRECT's second specialisation in 2-D)
NU_2D = (1.0, 2.0, 2.5, 3.0, 5.364, 6.0, 7.0, 14.0, 15.0, 16.0, 30.0, 126.0, 127.0)
NU_3D = (1.0, 5.0, 6.0, 5.364, 125.0, 126.0)
NU_2D_OTHER_RHO = (5.364, 6.0)
RHO_2D = (0.5, -0.9, 0.99)
THETA = (0.2, 1.0, 1.0 + 2.0 ** -30, 1.5, 6.0, 50.0)


def slabs(dim):
    return ((-100.0, -3.0), (-3.0, -2.0), (-0.5, 0.0), NARROW)


def copula_cases():
    """[(copula, dim, params)]: the copula side of the matrix, the same for GARCH and MSM."""
    out = [("student", 2, (nu, 0.5)) for nu in NU_2D]
    out += [("student", 2, (nu, rho)) for rho in RHO_2D[1:] for nu in NU_2D_OTHER_RHO]
    out += [("student", 3, (nu,) + R3[k]) for k in R3 for nu in NU_3D]
    out += [("gaussian", 2, (rho,)) for rho in (0.0, 0.5, -0.9, 0.99)]
    out += [("gaussian", 3, R3[k]) for k in R3]
    out += [("plackett", 2, (th,)) for th in THETA]
    return out


def cases():
    """[(model, copula, dim, params)], GARCH then MSM; a case's index is its row in the fixture."""
    return [(m,) + c for m in ("garch", "msm") for c in copula_cases()]


def case_id(case):
    model, copula, dim, params = case
    return "%s-%s-%dd-%s" % (model, copula, dim, "_".join("%.12g" % p for p in params))


def ztab_key(case):
    """The quantile table a case reads: it depends on the model's u tables and, for Student, nu only."""
    model, copula, dim, params = case
    if copula == "plackett":
        return None
    rows = "mild" if model != "msm" and sigma_rows(copula, dim, params) is SIGMA_2D_MILD else ""
    return "zt_%s%s_%dd_%s" % (model, rows, dim, ("t%g" % params[0]).replace(".", "p") if copula == "student" else "n")


def problem_inputs(case, z):
    """Problem(...) arguments of a case; z: the fixture (MSM's filter outputs), or a dict holding
    msm<dim>_fbs / _pi / _uvs."""
    from oracle import forecast as F
    model, copula, dim, params = case
    n = N_OF[dim]
    w = np.full(dim, 1.0 / dim)
    cp = float(params[0]) if copula == "plackett" else np.array(params, dtype=np.float64)
    if model == "msm":
        x, step = F.x_grid(n, "msm")
        uvs = z["msm%d_uvs" % dim]
        dens = F.msm_densities(uvs, x)
        combos = F.vol_combinations(dim, uvs.shape[1])
        return dict(model="msm", copula=copula, dim=dim, x_values=x, step=step, densities=dens, combos=combos,
                    weights=w, copula_params=cp, per_date=(z["msm%d_fbs" % dim], z["msm%d_pi" % dim]),
                    unique_vol_states=uvs)
    x, step = F.x_grid(n, "garch")
    return dict(model=model, copula=copula, dim=dim, x_values=x, step=step, densities=np.ones((dim, 1, n)),
                combos=np.zeros((1, dim)), weights=w, copula_params=cp,
                per_date=sigma_rows(copula, dim, params), unique_vol_states=None)


# ------------------------------------------------------------------ extension: Gumbel kinds, chunk edges, events, candidates
# A second fixture (tests/kat/gen_node_kat_ext.py writes it) holds the truths of the cases below and, for
# them and for every case of cases(), the truths of the conditional and batched-weight passes.  It is kept
# apart from node_kat.kat, whose bytes and case indices do not move.
EXT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_kat_ext.kat")
EXT_GEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat", "gen_node_kat_ext.py")
GUMBEL_KINDS = ("gumbel", "gumbel_survival")
# 1: c == 1; 1 + 2^-30: the cancellation in theta - 1; 16: the plan's cap
GUMBEL_THETA = (1.0, 1.0 + 2.0 ** -30, 1.5, 4.0, 16.0)
# chunk edges of the row cores: 2-D n = 70 is two 64-row chunks, 6 live rows in the second; 3-D n = 17 is
# 289 rows, one 256-row chunk plus 33
N_EDGE = {2: 70, 3: 17}
NR1_FACTOR = 1.0 + 2.0 ** -20             # one entry of pi_t scaled by it, then renormalised: pi_t is not rank 1


EXP7_BAR = 4.05e-11                       # exp2_node7's own polynomial error (tests/test_node_reference_cpu.py)


def gumbel_bar(ebound, tier):
    """The bar of a Gumbel slab sum, as a share of its sum |mass|: 1e-12 plus the device formulas' first-order
    bound (tests/gumbel_node_reference.py; the fixture's ebound, or ebound_fast on SORTED's record path, whose
    outer exp2_node7 adds its own error)."""
    return 1e-12 + np.asarray(ebound, dtype=np.float64) + (EXP7_BAR if tier == "fast" else 0.0)


def load_ext():
    return dict(np.load(EXT_PATH, allow_pickle=False))


def ext_cases():
    """[(model, copula, dim, params, n, variant)]: a case's index is its row in the extension
    fixture's slab truths.  variant "nr1": MSM dates whose pi_t is not rank 1 (SORTED then runs
    node_value, the generic path)."""
    out = []
    for m in ("garch", "msm"):
        for kind in GUMBEL_KINDS:
            for dim in (2, 3):
                out += [(m, kind, dim, (th,), N_OF[dim], "") for th in GUMBEL_THETA]
    for kind in GUMBEL_KINDS:
        out += [("msm", kind, dim, (4.0,), N_OF[dim], "nr1") for dim in (2, 3)]
    for m in ("garch", "msm"):
        for kind in GUMBEL_KINDS:
            out += [(m, kind, dim, (4.0,), N_EDGE[dim], "") for dim in (2, 3)]
        # Plackett is 2-D only: the two edge sizes, both as 2-D grids
        out += [(m, "plackett", 2, (1.5,), n, "") for n in (N_EDGE[2], N_EDGE[3])]
    return out


def all_cases():
    """cases() in the six-field form, then ext_cases(): a case's index is its row in the extension
    fixture's event and candidate truths."""
    return [c + (N_OF[c[2]], "") for c in cases()] + ext_cases()


def ext_case_id(case):
    model, copula, dim, params, n, variant = case
    return case_id(case[:4]) + "-n%d" % n + ("-" + variant if variant else "")


def gumbel_stiff(model, copula, dim, params):
    """Gumbel cases whose one-ulp conditioning figure stays above 1e-15 of the slab's sum |mass|: three
    axes at theta >= 4 (x_i^theta carries an ulp of u_i theta-fold on each axis) -- for GARCH under every
    row set of SIGMA_CANDIDATES (tests/test_node_reference_ext_cpu.py asserts it) -- and, for MSM, whose
    marginal inputs are the filter's and not chosen, also the 2-D survival kind at the cap theta = 16
    (GARCH meets 1e-15 there on the equal rows, gumbel_sigma_rows)."""
    if copula not in GUMBEL_KINDS:
        return False
    return (dim == 3 and params[0] >= 4.0) or (model == "msm" and copula == "gumbel_survival" and params[0] >= 16.0)


def gumbel_sigma_rows(copula, dim, params):
    if dim == 3:
        return SIGMA_3D
    return SIGMA_2D_EQUAL if copula == "gumbel_survival" and params[0] >= 16.0 else SIGMA_2D


def msm_key(dim, n):
    """Fixture prefix of the MSM filter outputs of a shape: node_kat.kat's for the base shapes."""
    return "msm%d" % dim if n == N_OF[dim] else "msm%d_n%d" % (dim, n)


def not_rank1(pi):
    """pi (T, Q) with entry 0 of every date scaled by NR1_FACTOR and the row renormalised, in float64
    steps whose order is fixed (a sequential sum), so every machine gets the same bits."""
    out = np.array(pi, dtype=np.float64, copy=True)
    out[:, 0] = out[:, 0] * NR1_FACTOR
    for t in range(out.shape[0]):
        s = 0.0
        for v in out[t]:
            s = s + float(v)
        out[t] = out[t] / s
    return out


def ext_problem_inputs(case, z):
    """Problem(...) arguments of a six-field case; z: a dict holding the MSM filter outputs the case
    reads (msm_key: both fixtures merged)."""
    from oracle import forecast as F
    model, copula, dim, params, n, variant = case
    w = np.full(dim, 1.0 / dim)
    cp = float(params[0]) if copula == "plackett" else np.array(params, dtype=np.float64)
    if model == "msm":
        x, step = F.x_grid(n, "msm")
        k = msm_key(dim, n)
        uvs, pi = z[k + "_uvs"], z[k + "_pi"]
        if variant == "nr1":
            pi = not_rank1(pi)
        return dict(model="msm", copula=copula, dim=dim, x_values=x, step=step, densities=F.msm_densities(uvs, x),
                    combos=F.vol_combinations(dim, uvs.shape[1]), weights=w, copula_params=cp,
                    per_date=(z[k + "_fbs"], pi), unique_vol_states=uvs)
    assert variant == ""
    x, step = F.x_grid(n, "garch")
    rows = gumbel_sigma_rows(copula, dim, params) if copula in GUMBEL_KINDS else sigma_rows(copula, dim, params)
    return dict(model=model, copula=copula, dim=dim, x_values=x, step=step, densities=np.ones((dim, 1, n)),
                combos=np.zeros((1, dim)), weights=w, copula_params=cp, per_date=rows, unique_vol_states=None)


def events(x, dim):
    """[(axis, name, (lo, hi))] in grid units: per axis a stress event (-inf, x[n // 3]] and a band
    (x[n // 4], x[3 n // 4]]."""
    n = x.size
    out = []
    for c in range(dim):
        out += [(c, "stress", (-INF, float(x[n // 3]))), (c, "band", (float(x[n // 4]), float(x[3 * n // 4])))]
    return out


def case_digest(case, z):
    """SHA-256 of everything a six-field case's truths are computed from: the copula parameters, the
    grid, the per-date inputs, the slabs, the events and the candidate weight vectors on offer."""
    kw = ext_problem_inputs(case, z)
    dim = case[2]
    per = kw["per_date"] if case[0] == "msm" else (kw["per_date"],)
    parts = [np.ravel(np.asarray(case[3], dtype=np.float64)), kw["x_values"], np.ravel(kw["step"]), kw["weights"],
             np.ravel(kw["densities"])] + [np.ravel(a) for a in per]
    if case[0] == "msm":
        parts.append(np.ravel(kw["unique_vol_states"]))
    parts += [np.ravel(slabs(dim)), np.ravel([b for _, _, b in events(kw["x_values"], dim)]),
              np.ravel(PORT_UNEQUAL[dim]), np.ravel(PORT_SIGNED[dim])]
    return digest(np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]))


# candidate weight vectors of the batched-weights pass: the plan's own, an unequal one, and one with a
# zero or negative secondary weight -- the first of the alternatives under which every slab keeps a member
# node on every date (the generator decides and stores the vectors; a zero weight leaves one axis' grid
# to meet the narrow slab alone)
PORT_UNEQUAL = {2: (0.7, 0.3), 3: (0.5, 0.3, 0.2)}
PORT_SIGNED = {2: ((1.0, 0.0), (0.8, -0.2)), 3: ((0.6, 0.0, 0.4), (0.7, 0.5, -0.2))}
