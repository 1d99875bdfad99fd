"""Inputs of the exact-quantile level probes, shared by tests/kat/gen_quantile_probes.py (which adds the
longdouble truths), tests/test_quantile_probes_cpu.py and tests/test_quantile_probes_gpu.py: the case matrix,
the argument sets, the bars, the host rules restated and the fixture's layout.  No mpmath here: the GPU module
reads only this module, tests/solve_probe_cases.py, tests/node_cases.py and the fixtures.

A probe is one level alpha' = F_true(target) + sign * offset handed to cvq_quantiles (or its conditional,
batched-weights or per-date sibling): the returned var is (lo + hi) / 2 of dyadic midpoints and so encodes the
bracket test and all K decisions, which say on which side of the truth the device's own F at the target lies
(tests/quantile_probe_reference.py).  The fixture holds, per probe, alpha', the offset, a NaN flag and the K
decisions as a bit word; the expected var is rebuilt from those in float64 (var_from_bits)."""
import hashlib
import os

import numpy as np

import node_cases as NC
import solve_probe_cases as SC

PROBE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantile_probes.kat")
GEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat", "gen_quantile_probes.py")
T = NC.T
AMBIGUOUS_CAP = SC.AMBIGUOUS_CAP
PRECISE_CAP = SC.PRECISE_CAP
STIFF_EXTRA = SC.STIFF_EXTRA
KINDS = ("min", "max", "level")
CALLS = ("quant", "cond", "port", "dyn")
FAMILY = {"quant": "moments", "cond": "cond", "port": "port", "dyn": "moments"}
MAX_LEVELS = 8                               # CVQ_MAX_LEVELS
NO_LEVEL = 1.0e6                             # a level above every F(max_var)
U53 = 2.0 ** -53

# base levels, as fractions of the date's own F_true(max_var) (3-D F runs above 1 under quirk Q6); the first five
# are the first choice, the generator moves on by five where a date's ambiguous share would pass the cap
FRACTIONS = (0.05, 0.01, 0.2, 0.001, 0.5, 0.1, 0.02, 0.35, 0.003, 0.7, 0.15, 0.03, 0.0003, 0.6, 0.07)
BASES_PER_DATE = 5

# argument sets: keywords of QuadraturePlan.quantiles (ptf_mean among them); max_var None: the grid's top under
# the weights plus 1 (top_of), above every row's last threshold
ARGSETS = {
    "default": {},                                        # K = 23: the last pass takes 2 steps
    "k24": {"tolerance": 5e-7},                           # K = 24: 3 steps
    "k25": {"tolerance": 2.5e-7},                         # K = 25: 1 step
    "k3": {"tolerance": 1.0},                             # K = 3: the opening decisions, then the closing pass
    "k2": {"tolerance": 2.0},                             # K = 2
    "nondyadic": {"min_var": -7.3, "ptf_mean": 3.7e-4},   # non-dyadic mids; the closing cut's rounding
    "inside": {"lower": -4.0, "min_var": -3.5},           # the opening pass starts inside the grid: ka > 0
    "top": {"max_var": None, "ptf_mean": 3.7e-4},         # narrow-pass lanes run past the last column
}
ARG_DEFAULTS = dict(ptf_mean=0.0, min_var=-7.5, max_var=0.0, lower=-100.0, tolerance=1e-6)
DYN_MEANS = (0.01, 0.02, 0.03)               # dynamic_reference.means(3)

COPULAS_2D = (("student", (6.0, 0.5)), ("student", (5.364, 0.5)), ("student", (127.0, 0.5)), ("gaussian", (0.5,)),
              ("gaussian", (-0.9,)), ("plackett", (1.5,)), ("gumbel", (4.0,)), ("gumbel_survival", (4.0,)))
COPULAS_3D = (("student", (6.0,) + NC.R3["mild"]), ("gaussian", NC.R3["mild"]), ("gumbel", (4.0,)))
WIDE = {2: (("student", (6.0, 0.5)), ("gaussian", (0.5,))), 3: (("student", (6.0,) + NC.R3["mild"]), ("gaussian", NC.R3["mild"]))}
SUB = {2: (("student", (6.0, 0.5)), ("gaussian", (0.5,)), ("gumbel", (4.0,))),
       3: (("student", (6.0,) + NC.R3["mild"]), ("gaussian", NC.R3["mild"]), ("gumbel", (4.0,)))}
N_SMALL, N_EDGE, N_WIDE = {2: 24, 3: 12}, {2: 70, 3: 17}, {2: 128, 3: 40}
# targets per date: (thinned level targets and the two bracket targets, edge targets on top)
TARGETS = {"quant": (8, 3), "argset": (5, 2), "cond": (4, 1), "port": (4, 1), "dyn": (5, 2)}


def probe_cases():
    """[(call, model, copula, dim, params, n, variant, argset, sub)]; a case's index is its row in the fixture.
    sub: cond (axis, event: 0 stress, 1 band, of node_cases.events), port (the candidate's index,), else ()."""
    out = []
    for m in ("garch", "msm"):
        for dim, cops in ((2, COPULAS_2D), (3, COPULAS_3D)):
            for n in (N_SMALL[dim], N_EDGE[dim]):
                out += [("quant", m, c, dim, p, n, "", "default", ()) for c, p in cops]
            out += [("quant", m, c, dim, p, N_WIDE[dim], "", "default", ()) for c, p in WIDE[dim]]
    out.append(("quant", "msm", "student", 2, (6.0, 0.5), 24, "nr1", "default", ()))
    for m in ("garch", "msm"):
        for dim in (2, 3):
            for c, p in WIDE[dim]:
                out += [("quant", m, c, dim, p, N_SMALL[dim], "", a, ()) for a in ARGSETS if a != "default"]
    for m in ("garch", "msm"):
        for dim in (2, 3):
            for n in (N_SMALL[dim], N_EDGE[dim]):
                for c, p in WIDE[dim]:
                    out += [("cond", m, c, dim, p, n, "", "default", (ax, e)) for ax in range(dim) for e in (0, 1)]
    for m in ("garch", "msm"):
        for dim, ns in ((2, (24,)), (3, (12, 17))):
            for n in ns:
                for c, p in SUB[dim]:
                    out += [("port", m, c, dim, p, n, "", "default", (k,)) for k in range(3)]
    for m in ("garch", "msm"):
        for dim in (2, 3):
            out += [("dyn", m, c, dim, p, N_SMALL[dim], "", "default", ()) for c, p in WIDE[dim]]
    return out


def base_of(case):
    """The solve_probe_cases case (model, copula, dim, params, n, variant, "default") a case's inputs are built from."""
    return case[1:7] + ("default",)


def group_key(case):
    """Cases that share a device plan."""
    return case[1:7]


def probe_case_id(case):
    call, model, copula, dim, params, n, variant, argset, sub = case
    s = "%s-%s-n%d" % (call, NC.case_id(case[1:5]), n) + ("-" + variant if variant else "")
    s += ("-" + argset if argset != "default" else "")
    return s + ("".join("-%d" % v for v in sub))


def group_id(key):
    return NC.case_id(key[:4]) + "-n%d" % key[4] + ("-" + key[5] if key[5] else "")


def problem_inputs(case, z):
    return SC.problem_inputs(base_of(case), z)


def port_weights(dim):
    """(3, dim): the plan's own weights, the unequal vector and the one with a negative secondary weight."""
    return np.array([tuple(np.full(dim, 1.0 / dim)), NC.PORT_UNEQUAL[dim], NC.PORT_SIGNED[dim][1]])


def dyn_params(case):
    """(T, n_copula_params): dynamic_reference's per-date paths (tests/dynamic_cases.py param_path)."""
    import dynamic_reference as R
    copula, dim, params = case[2], case[3], case[4]
    rho = R.RHO2[:T, None] if dim == 2 else R.RHO3[:T]
    return np.column_stack((np.full(T, float(params[0])), rho)) if copula == "student" else rho.copy()


def weights_of(case, t, kw):
    """The weights date t's membership and levels run under."""
    if case[0] == "port":
        return port_weights(case[3])[case[8][0]]
    if case[0] == "dyn":
        return port_weights(case[3])[t]
    return kw["weights"]


def top_of(x, w):
    """The grid's top under the weights plus 1."""
    return float(np.sum(np.abs(np.asarray(w, dtype=np.float64))) * np.max(x)) + 1.0


def args_of(case, kw, t=0):
    """min_var, max_var, lower, tolerance, ptf_mean of a case (date t: the per-date call has a mean per date)."""
    a = dict(ARG_DEFAULTS)
    a.update(ARGSETS[case[7]])
    if a["max_var"] is None:
        a["max_var"] = top_of(kw["x_values"], kw["weights"])
    if case[0] == "dyn":
        a["ptf_mean"] = DYN_MEANS[t]
    return a


def event_of(case, kw):
    """(axis, name, (lo, hi)) of a conditional case."""
    ax, e = case[8]
    ev = NC.events(kw["x_values"], case[3])[2 * ax + e]
    assert ev[0] == ax
    return ev


def bisection_steps(a):
    import quantile_reference as Q
    return Q.bisection_steps(a["min_var"], a["max_var"], a["tolerance"])


def case_digest(case, z):
    """SHA-256 of everything a case's truths are computed from."""
    kw = problem_inputs(case, z)
    parts = [SC.case_digest(base_of(case), z).encode(), repr(case).encode(), np.asarray(FRACTIONS).tobytes(),
             repr(TARGETS).encode()]
    for t in range(T):
        a = args_of(case, kw, t)
        parts.append(np.array([a[k] for k in sorted(a)], dtype=np.float64).tobytes())
        parts.append(np.asarray(weights_of(case, t, kw), dtype=np.float64).tobytes())
    if case[0] == "cond":
        parts.append(np.array(event_of(case, kw)[2], dtype=np.float64).tobytes())
    if case[0] == "dyn":
        parts.append(np.ascontiguousarray(dyn_params(case)).tobytes())
    return hashlib.sha256(b"|".join(parts)).hexdigest()


# ------------------------------------------------------------------ bars
def bar_of(case, ebound=0.0):
    """The relative bar of a case's F: bar_of / TIERS of tests/test_node_slabs_gpu.py (the rows "moments", "cond"
    and "port": node_value for every copula, the precise tier), the stiff cases' 5e-14 on top; the Gumbel kinds
    1e-12 plus the device formulas' first-order bound weighted over the sum's set (node_cases.gumbel_bar).
    The chain F(lo) + increment adds at most 12 roundings per F (9 passes, the chunk sums), each at most
    2^-53 sum |mass|, 1.3e-15 together: inside the 1e-12, no term of their own."""
    import test_node_slabs_gpu as SL
    call, model, copula, dim, params = case[:5]
    if copula in NC.GUMBEL_KINDS:
        assert SL.TIERS[(FAMILY[call], "gumbel", False)] == "precise"
        return float(NC.gumbel_bar(ebound, "precise")) + (STIFF_EXTRA if NC.gumbel_stiff(model, copula, dim, params) else 0.0)
    bar, tier, _ = SL.bar_of(FAMILY[call], copula, dim, params)
    assert tier == "precise"
    return bar + (STIFF_EXTRA if NC.stiff(model, copula, dim, params) else 0.0)


# ------------------------------------------------------------------ the host rules, restated
def chunk_rows(dim):
    """cvq_moments_kernels.h moments_chunk_rows: 64 rows in 2-D (the four waves split the columns), 256 in 3-D."""
    return 64 if dim == 2 else 256


def chunk_layout(dim, n):
    """(full chunks, rows of the partial last chunk)."""
    rows = n ** (dim - 1)
    return rows // chunk_rows(dim), rows % chunk_rows(dim)


def schedule(K):
    """cvq_quantile.hip launch_quantiles: the steps of the opening pass and of every C = 7 pass."""
    out, left, first = [], K, True
    while first or left > 0:
        s = min(left, 3)
        out.append(s)
        left -= s
        first = False
    return out


def quant_cuts(lo, hi):
    """cvq_quantile_kernels.h quant_cuts."""
    c = [0.0] * 7
    c[3] = (lo + hi) / 2
    c[1] = (lo + c[3]) / 2
    c[5] = (c[3] + hi) / 2
    c[0] = (lo + c[1]) / 2
    c[2] = (c[1] + c[3]) / 2
    c[4] = (c[3] + c[5]) / 2
    c[6] = (c[5] + hi) / 2
    return c


def walk(a, bits, K):
    """k_quant_update's descent of a path: [(pass, cut index, moved up?, lo, hi of the pass)] per decision, and
    the final (lo, hi)."""
    lo, hi = float(a["min_var"]), float(a["max_var"])
    out, k = [], 0
    for p, steps in enumerate(schedule(K)):
        plo, phi = lo, hi
        cuts = quant_cuts(lo, hi)
        at, half = 3, 2
        for _ in range(steps):
            up = bool((int(bits) >> k) & 1)
            out.append((p, at, up, plo, phi))
            if up:
                lo = cuts[at]
                at += half
            else:
                hi = cuts[at]
                at -= half
            half >>= 1
            k += 1
    return out, (lo, hi)


def var_from_bits(a, nan, bits, K):
    """The var a path returns: NaN outside the bracket, else (lo + hi) / 2 + ptf_mean after K decisions (bit k set:
    F(mid_k) < alpha', lo moves up), formed in float64 as k_quant_update forms it."""
    if nan:
        return float("nan")
    lo, hi = float(a["min_var"]), float(a["max_var"])
    for k in range(K):
        mid = (lo + hi) / 2
        if (int(bits) >> k) & 1:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2 + a["ptf_mean"]


# ------------------------------------------------------------------ fixture
PER_PROBE = (("date", np.uint8), ("kind", np.uint8), ("level", np.int8), ("sign", np.int8), ("nan", np.uint8),
             ("bits", np.uint32), ("alpha", np.float64), ("offset", np.float32), ("count", np.int32),
             ("m0_hi", np.float64), ("m0_lo", np.float32), ("es_hi", np.float64), ("es_lo", np.float32),
             ("scale0", np.float64), ("scale1", np.float64))
PER_CASE = ("K", "base", "candidates", "ambiguous", "bar", "pe_hi", "pe_lo", "scale_e")


def load_probes():
    return dict(np.load(PROBE_PATH, allow_pickle=False))


def probes_of(z, ci):
    s, e = int(z["case_start"][ci]), int(z["case_start"][ci + 1])
    return {k: z[k][s:e] for k, _ in PER_PROBE}


def joined(hi, lo):
    """hi + hi * lo (lo kept relative, float32), as node_cases.truth."""
    hi = np.asarray(hi, dtype=np.longdouble)
    with np.errstate(invalid="ignore"):
        return hi + np.where(np.isfinite(hi), hi * np.asarray(lo, dtype=np.longdouble), 0.0)
