"""Inputs of the solve-path probes, shared by tests/kat/gen_solve_probes.py (which adds the longdouble
truths), tests/test_solve_probes_cpu.py and tests/test_solve_probes_gpu.py: the case matrix, the solve
argument sets, the bars and the fixture's layout.  No mpmath here: the GPU module reads only this
module, tests/node_cases.py and the two fixtures.

A probe is one solve with obj_var = F_true(target) + sign * offset: the device's K + 1 snapshot mids of the
target date then say on which side of the truth its own F at the target lies (tests/solve_probe_reference.py).
The fixture holds, per probe, obj', the offset, the bracket and the K decisions as a bit word; the expected
mids are rebuilt from those in float64 (mids_from_bits), as the device forms them."""
import os

import numpy as np

import node_cases as NC

PROBE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_probes.kat")
GEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat", "gen_solve_probes.py")
T = NC.T
STRATEGIES = ("compact", "sorted", "sweep", "direct", "prefix")
AMBIGUOUS_CAP = 0.25
PRECISE_CAP, FAST_CAP = 1e-11, 5e-11
STIFF_EXTRA = 5e-14
TIER_NAMES = ("precise", "prefix", "fast")
KINDS = ("r0", "F", "level")

# solve argument sets (engine.solve_args keywords)
ARGSETS = {
    "default": {},
    # min_var = -7.3: bracket 0 is (-7.3, -3.5], whose width is no power of two -- dyadic_walk_ok is false and
    # k_compact's block tail takes the lane-0 walk (and K carries the non-dyadic margin of 2)
    "nondyadic": {"min_var": -7.3},
    # K = 3: build_cell_counts stops at depth min(16, K) = 3 without reaching its cap at n = 320 (the GARCH grid
    # needs depth 5, the MSM grid 4), so the plan carries no cell tables
    "coarse": {"tolerance": 0.6},
}
ARG_DEFAULTS = dict(obj_var=0.05, first_guess=-3.0, second_guess=(-3.5, -2.0), min_var=-7.5, max_var=0.0,
                    lower=-100.0, tolerance=1e-6)


def solve_kwargs(argset, obj_var=None):
    kw = dict(ARG_DEFAULTS)
    kw.update(ARGSETS[argset])
    if obj_var is not None:
        kw["obj_var"] = float(obj_var)
    return kw


# ------------------------------------------------------------------ case matrix
COPULAS_2D = (("student", (6.0, 0.5)), ("student", (7.0, 0.5)), ("student", (5.364, 0.5)), ("student", (127.0, 0.5)),
              ("gaussian", (0.5,)), ("gaussian", (-0.9,)), ("plackett", (1.5,)), ("plackett", (0.2,)))
COPULAS_3D = (("student", (6.0,) + NC.R3["mild"]), ("gaussian", NC.R3["mild"]), ("gumbel", (4.0,)))
N_2D, N_RPT2, N_3D = (24, 128), 320, (12, 40)
# targets per date (the issue's cap is 32; fewer where a case runs long or the fixture grows)
TARGETS = {24: 16, 128: 16, 320: 16, 12: 16, 40: 16}


def probe_cases():
    """[(model, copula, dim, params, n, variant, argset)]; a case's index is its row in the fixture.
    variant "nr1": the middle date's pi_t is not rank 1 (COMPACT defers it to its generic kernel, SORTED
    runs node_value on it), the other two dates stay on the fast path."""
    out = []
    for m in ("garch", "msm"):
        for n in N_2D:
            out += [(m, c, 2, p, n, "", "default") for c, p in COPULAS_2D]
    for n in N_2D:
        out += [("msm", "student", 2, (6.0, 0.5), n, "nr1", "default"), ("msm", "plackett", 2, (1.5,), n, "nr1", "default")]
    out += [("garch", "student", 2, (6.0, 0.5), N_RPT2, "", a) for a in ("default", "coarse")]
    out += [("msm", "gaussian", 2, (0.5,), N_RPT2, "", a) for a in ("default", "coarse")]
    for m in ("garch", "msm"):
        out += [(m, "student", 2, (6.0, 0.5), 24, "", "nondyadic"), (m, "gaussian", 2, (0.5,), 24, "", "nondyadic")]
    for m in ("garch", "msm"):
        for n in N_3D:
            out += [(m, c, 3, p, n, "", "default") for c, p in COPULAS_3D]
    return out


def probe_case_id(case):
    model, copula, dim, params, n, variant, argset = case
    return NC.case_id(case[:4]) + "-n%d" % n + ("-" + variant if variant else "") + ("-" + argset if argset != "default" else "")


def not_rank1_middle(pi):
    """NC.not_rank1 on the middle date only."""
    out = np.array(pi, dtype=np.float64, copy=True)
    mid = out.shape[0] // 2
    out[mid] = NC.not_rank1(out[mid:mid + 1])[0]
    return out


def problem_inputs(case, z):
    """Problem(...) arguments of a probe case; z: node_kat.kat (the MSM filter outputs, which do not depend
    on n)."""
    from oracle import forecast as F
    model, copula, dim, params, n, variant, _ = case
    w = np.full(dim, 1.0 / dim)
    cp = float(params[0]) if copula == "plackett" else np.array(params, dtype=np.float64)
    if model == "msm":
        x, step = F.x_grid(n, "msm")
        uvs, pi = z["msm%d_uvs" % dim], z["msm%d_pi" % dim]
        if variant == "nr1":
            pi = not_rank1_middle(pi)
        return dict(model="msm", copula=copula, dim=dim, x_values=x, step=step, densities=F.msm_densities(uvs, x),
                    combos=F.vol_combinations(dim, uvs.shape[1]), weights=w, copula_params=cp,
                    per_date=(z["msm%d_fbs" % dim], pi), unique_vol_states=uvs)
    assert variant == ""
    x, step = F.x_grid(n, "garch")
    rows = NC.gumbel_sigma_rows(copula, dim, params) if copula in NC.GUMBEL_KINDS else NC.sigma_rows(copula, dim, params)
    return dict(model=model, copula=copula, dim=dim, x_values=x, step=step, densities=np.ones((dim, 1, n)),
                combos=np.zeros((1, dim)), weights=w, copula_params=cp, per_date=rows, unique_vol_states=None)


def case_digest(case, z):
    """SHA-256 of everything a probe case's truths are computed from."""
    kw = problem_inputs(case, z)
    per = kw["per_date"] if case[0] == "msm" else (kw["per_date"],)
    a = solve_kwargs(case[6])
    parts = [np.ravel(np.asarray(case[3], dtype=np.float64)), kw["x_values"], np.ravel(kw["step"]), kw["weights"],
             np.ravel(kw["densities"])] + [np.ravel(x) for x in per]
    if case[0] == "msm":
        parts.append(np.ravel(kw["unique_vol_states"]))
    parts.append(np.array([a["first_guess"], a["second_guess"][0], a["second_guess"][1], a["min_var"], a["max_var"],
                           a["lower"], a["tolerance"]]))
    parts.append(np.asarray(BASE_OBJS, dtype=np.float64))
    return NC.digest(np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]))


# base obj_var values on offer, in order of preference; the generator takes, per date, the first of them
# whose truth paths together put the date into as many brackets as any choice can (and every case's dates
# into all four)
BASE_OBJS = (0.05, 0.2, 0.03, 0.004, 0.0015, 0.1, 0.4, 0.01, 0.0005, 0.7, 1e-4, 2e-5, 3e-6, 1e-7, 1e-9,
             # (Gaussian rho = -0.9: the equal-weight portfolio has almost no mass below the first guess)
             1e-11, 1e-13, 1e-15, 1e-18, 1e-22, 1e-26, 1e-30, 1e-35, 1e-40,
             # (3-D MSM: quirk Q6 keeps the axis-0 Delta factor on one plane only, so F runs far above 1)
             1.5, 3.0, 5.0, 8.0, 12.0, 17.0)
BASES_PER_DATE = 5


# ------------------------------------------------------------------ bars
def family_of(strategy, dim):
    """The TIERS family (tests/test_node_slabs_gpu.py) of a strategy's solve kernel."""
    return {"compact": "compact-solve", "sorted": "sorted-solve", "sweep": "sorted-solve", "direct": "direct",
            "prefix": "prefix"}[strategy]


def accepts(strategy, dim, copula):
    """cvq_plan_create: DIRECT, COMPACT and SWEEP are built for dim == 2; the Gumbel kinds have SORTED
    instances only."""
    if copula in NC.GUMBEL_KINDS:
        return strategy == "sorted"
    return dim == 2 or strategy in ("sorted", "prefix")


def bar_and_tier(case, strategy, gumbel_ebound=0.0):
    """(bar, tier index into TIER_NAMES) of a strategy's solve on a case: bar_of / TIERS of
    tests/test_node_slabs_gpu.py, the stiff cases' 5e-14 on top.  PREFIX is its own tier: its probes' offset
    also carries the running row sums' 2 n 2^-53 sum |mass| term."""
    import test_node_slabs_gpu as SL
    model, copula, dim, params = case[:4]
    if copula in NC.GUMBEL_KINDS:
        # rank-1 dates: SORTED's record path (node_fast), the fast Gumbel bar of node_cases.gumbel_bar
        return float(NC.gumbel_bar(gumbel_ebound, "fast")), 2
    bar, tier, _ = SL.bar_of(family_of(strategy, dim), copula, dim, params)
    if NC.stiff(model, copula, dim, params):
        bar += STIFF_EXTRA
    if strategy == "prefix":
        return bar, 1
    return bar, (2 if tier == "fast" else 0)


# ------------------------------------------------------------------ the solve's host-side rules, restated
def halvings(w, tol):
    k = 0
    while w > tol and k < 1000:
        w = w / 2
        k += 1
    return k


def _dyadic(v):
    for k in range(41):
        s = np.ldexp(v, k)
        if s == np.floor(s) and abs(s) < 9.0e15:
            return k
    return None


def brackets(a):
    """k_compact's bracket order (cvq_plan.hip): (vmin, sg0], (sg0, fg], (sg1, vmax], (fg, sg1]."""
    sg0, sg1 = a["second_guess"]
    return ((a["min_var"], sg0), (sg0, a["first_guess"]), (sg1, a["max_var"]), (a["first_guess"], sg1))


def snap_K(a):
    """cvq_snap_stride - 1 (cvq_plan.hip bisect_budget): the most halvings any bracket needs, plus 2 where a
    bracket's mids are not all exact dyadic points."""
    K, exact = 0, True
    for lo, hi in brackets(a):
        k = halvings(hi - lo, a["tolerance"])
        K = max(K, k)
        e0, e1 = _dyadic(lo), _dyadic(hi)
        if e0 is None or e1 is None:
            exact = False
            continue
        mag = max(abs(lo), abs(hi))
        if max(e0, e1) + k + int(np.ceil(np.log2(mag + 1.0))) + 1 > 52:
            exact = False
    return K if exact else K + 2


def dyadic_bracket_ok(lo, hi, K):
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo) or K < 1 or K > 52:
        return False
    W = hi - lo
    if W + lo != hi or hi - W != lo:
        return False
    if np.frexp(W)[0] != 0.5:
        return False
    q = np.ldexp(W, -K)
    if not (q > 0.0) or q < 2.0 ** -1022:
        return False
    N = lo / q
    return bool(N == np.floor(N) and abs(N) + np.ldexp(1.0, K) < np.ldexp(1.0, 53))


def dyadic_walk_ok(a):
    K = snap_K(a)
    return all(dyadic_bracket_ok(lo, hi, K) for lo, hi in brackets(a))


COMPACT_NT, BLK_PER_THREAD, COMPACT_MAX_DEPTH = 256, 12, 16       # cvq_compact_launch.h, cvq_compact_kernels.h, cvq_plan.hip
TAIL_CAP = COMPACT_NT * BLK_PER_THREAD


def build_cell_counts(count, a, cap=TAIL_CAP):
    """cvq_plan.hip build_cell_counts: (depth, cnt) with cnt[d][b][k] the nodes of depth-d cell k of bracket b,
    for d up to the first depth >= 1 at which every cell holds <= cap nodes; depth = -1 where none does within
    min(16, K).  count(lo, hi): the member nodes of (lo, hi] (the oracle's inner_mask)."""
    K = snap_K(a)
    cells = [[(lo, hi)] for lo, hi in brackets(a)]
    cnt = []
    for d in range(min(COMPACT_MAX_DEPTH, max(K, 0)) + 1):
        c = [[count(lo, hi) for lo, hi in row] for row in cells]
        cnt.append(c)
        if d >= 1 and all(v <= cap for row in c for v in row):
            return d, cnt
        cells = [[h for lo, hi in row for h in ((lo, (lo + hi) / 2), ((lo + hi) / 2, hi))] for row in cells]
    return -1, cnt


# ------------------------------------------------------------------ fixture
def load_probes():
    return dict(np.load(PROBE_PATH, allow_pickle=False))


def mids_from_bits(a, bracket, bits, K):
    """The K + 1 snapshot mids of a path: sn[k] = (lo + hi) / 2 before decision k, sn[K] the final one; bit k
    set: F(mid_k) < obj', the bracket's lower end moves up."""
    lo, hi = brackets(a)[bracket]
    out = np.empty(K + 1)
    for k in range(K):
        mid = (lo + hi) / 2
        out[k] = mid
        if (int(bits) >> k) & 1:
            lo = mid
        else:
            hi = mid
    out[K] = (lo + hi) / 2
    return out


def probes_of(z, ci):
    """Record arrays of case ci's probes (a slice of every per-probe array)."""
    s, e = int(z["case_start"][ci]), int(z["case_start"][ci + 1])
    return {k: z[k][s:e] for k in ("date", "tier", "kind", "level", "sign", "bracket", "bits", "obj", "offset", "count")}
