"""Inputs of the q sweep: every MSM kernel family at every number of unique volatility states per asset,
q = 1 ... 8 (the host dispatches `switch (S.q)` with case 1 ... 7 and default = 8; COMPACT's and the
quadrature core's node loops pad the states above q up to kQUnroll = 8), next to tests/node_cases.py, whose
shapes, slabs, events and candidate weights these are.  tests/kat/gen_q_sweep.py adds the longdouble /
mpmath truths (tests/golden/q_sweep.kat); tests/test_q_sweep_cpu.py and tests/test_q_sweep_gpu.py read this
module, node_cases and the fixtures.  No mpmath here.

MSM inputs.  q = 2 ... 8: tests/kat/gen_node_kat.py msm_inputs' recipe (cfg 2 in 2-D, cfg 4 in 3-D, T = 3
dates, 2-D n = 24, 3-D n = 12) at k = q - 1 volatility components, which have k + 1 distinct products; q = 3
is node_kat.kat's own (the generator asserts equality).  q = 1: the same recipe at k = 2 with every asset's
m_0 set to 1, the production route tests/test_forecast_kernels_gpu.py::test_single_unique_vol documents
(all four states carry the asset's sigma, and the unique-state map sends them to one): a genuine one-state
filter output on the cfg 2 / cfg 4 parameters, fbs = pi = 1 on every date.

The solve target.  Check (e) of tests/test_q_sweep_gpu.py compares calc_var's VaR and iteration count with the
oracle's bit for bit, which is sound only where no decision of the oracle hangs on rounding.  In 2-D the
default obj_var = 0.05 is such a target.  In 3-D it is not (q <= 7 under Student, q <= 4 under Gaussian): the
3-D Delta-weights are not normalised (quirk Q6: the box holds a mass of about 11.9), so F(-3.5) > 0.05, the bracket is
(-7.5, -3.5] and its first midpoint -5.5 lies under the lowest grid level -5.  The true F(-5.5) is 0; what the
reference's bookkeeping (prev - slab) leaves of it is a rounding residue of 1e-16, and the Q4 rule -- break
when every date's F is exactly 0 -- then fires or not by the order of a sum (on the device it fired on 3 of 32
(case, strategy) pairs where the oracle's own residues did not vanish; with q = 1, where the three dates are
identical, the oracle itself breaks at iteration 0 under Student).  A common 1 +- 1e-7 scaling of every integral
does not see this, residues scale with the rest.  So the 3-D solves take OBJ_VAR[3] = 1.0, whose bracket lies
among populated levels, and tests/test_q_sweep_cpu.py asserts a second premise next to the scaling one: at
every bisection level some date's F is at least 1e-7 of |prev| + |slab| away from 0.

A case is (copula, dim, params, q, variant); the model is MSM throughout (GARCH and UKF have one instance
per family and no q).  variant "nr1": node_cases.not_rank1 dates, on which SORTED runs its generic node
path and COMPACT defers the dates to its generic kernel, at q = 8, the kQUnroll edge."""
import os

import numpy as np

import node_cases as NC

KAT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "q_sweep.kat")
GEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat", "gen_q_sweep.py")
QS = (1, 2, 3, 4, 5, 6, 7, 8)
T = NC.T
GUMBEL_KINDS = NC.GUMBEL_KINDS
PRODUCT_KINDS = ("frank", "joe", "joe_survival")          # tests/archimedean_reference.py KINDS
SORTED_ONLY = GUMBEL_KINDS + PRODUCT_KINDS
FITTED_NU = 5.364
OBJ_VAR = {2: 0.05, 3: 1.0}               # the header: the solve target

# (copula, {dim: params}, the q it runs at).  Student nu = 6: k_direct's PM = 8 (2-D), the integer power;
# the fitted nu: PM = 0, the general power; survival Gumbel: the kLogB tables; Frank, survival Joe: the
# product form
SWEEP = (
    ("student", {2: (6.0, 0.5), 3: (6.0,) + NC.R3["mild"]}, QS),
    ("student", {2: (FITTED_NU, 0.5), 3: (FITTED_NU,) + NC.R3["mild"]}, (4, 8)),
    ("gaussian", {2: (0.5,), 3: NC.R3["mild"]}, QS),
    ("plackett", {2: (1.5,)}, QS),
    ("gumbel_survival", {2: (4.0,), 3: (4.0,)}, QS),
    ("frank", {2: (6.0,), 3: (6.0,)}, QS),
    ("joe_survival", {2: (2.0,), 3: (2.0,)}, QS),
)
NR1 = (("student", 2, (6.0, 0.5)), ("gumbel_survival", 3, (4.0,)), ("frank", 2, (6.0,)))
NR1_Q = 8

# the alternative middle date: another parameter set inside the kind's documented range (Student keeps
# the plan's nu: cvq_dynamic_quantiles, "copula_params[t, 0] must repeat nu"), and node_cases.PORT_UNEQUAL as
# the drifted weights
ALT_RHO = {2: (0.3,), 3: (0.3, 0.5, 0.2)}
ALT_THETA = {"plackett": 2.5, "gumbel_survival": 2.5, "frank": 3.0, "joe_survival": 3.0}
ALT_DATE = 1

# the distribution ladder: bins 0, 1, 3 and 5 are node_cases.slabs' four slabs, bin 2 descends (exactly
# (0, 0)), bin 4 is the rest between the narrow slab and (-0.5, 0]
LADDER = (-100.0, -3.0, -2.0, -2.55, -2.5, -0.5, 0.0)
BIN_OF_SLAB = (0, 1, 5, 3)
DESCENDING_BIN, FREE_BIN = 2, 4
for _s, (_a, _b) in enumerate(NC.slabs(2)):
    assert (LADDER[BIN_OF_SLAB[_s]], LADDER[BIN_OF_SLAB[_s] + 1]) == (_a, _b)
assert LADDER[DESCENDING_BIN + 1] < LADDER[DESCENDING_BIN] and NC.slabs(2) == NC.slabs(3)


def cases():
    """[(copula, dim, params, q, variant)]; a case's index is its row in the fixture."""
    out = []
    for copula, by_dim, qs in SWEEP:
        for dim in sorted(by_dim):
            out += [(copula, dim, by_dim[dim], q, "") for q in qs]
    out += [(copula, dim, params, NR1_Q, "nr1") for copula, dim, params in NR1]
    return out


def case_id(case):
    copula, dim, params, q, variant = case
    return "%s-%dd-%s-q%d%s" % (copula, dim, "_".join("%.12g" % p for p in params), q, "-" + variant if variant else "")


def full_sweeps():
    """[(copula, dim, params)] that must run at every q of QS."""
    return [(copula, dim, by_dim[dim]) for copula, by_dim, qs in SWEEP if qs == QS for dim in sorted(by_dim)]


def missing_q(case_list):
    """[(copula, dim, params, q)] of full_sweeps() that case_list does not hold (variant "")."""
    have = {c[:4] for c in case_list if c[4] == ""}
    return [s + (q,) for s in full_sweeps() for q in QS if s + (q,) not in have]


# every kind and dimension the matrix lists holds every q in 1 ... 8: a later trim cannot reopen the gap
# silently (tests/test_q_sweep_cpu.py states the same)
assert not missing_q(cases()), missing_q(cases())
assert {(c, d) for c, d, _ in full_sweeps()} == {(c, d) for c, by_dim, _ in SWEEP for d in by_dim}


def msm_key(dim, q):
    return "msm%d_q%d" % (dim, q)


def solve_case(case):
    """The cases whose solve is held to the oracle's calc_var: Student nu = 6 and Gaussian."""
    return case[0] == "gaussian" or (case[0] == "student" and case[2][0] == 6.0)


def plan_params(copula, params):
    return float(params[0]) if copula == "plackett" else np.array(params, dtype=np.float64)


def alt_params(case):
    copula, dim, params = case[:3]
    if copula == "student":
        return (params[0],) + ALT_RHO[dim]
    if copula == "gaussian":
        return ALT_RHO[dim]
    return (ALT_THETA[copula],)


def records(case):
    """(copula_params (T, n_params), weights (T, dim)) of the per-date record call: the plan's own values on
    dates 0 and 2, the alternative on date ALT_DATE."""
    copula, dim, params = case[:3]
    cp = np.tile(np.array(params, dtype=np.float64), (T, 1))
    w = np.full((T, dim), 1.0 / dim)
    cp[ALT_DATE], w[ALT_DATE] = alt_params(case), NC.PORT_UNEQUAL[dim]
    return cp, w


def problem_inputs(case, z, alt=False):
    """Problem(...) arguments of a case; z: the fixture (its msm<dim>_q<q>_fbs / _pi / _uvs).  alt: the
    alternative middle date alone (T = 1) under its own parameters and weights."""
    from oracle import forecast as F
    copula, dim, params, q, variant = case
    k = msm_key(dim, q)
    fbs, pi, uvs = z[k + "_fbs"], z[k + "_pi"], z[k + "_uvs"]
    assert uvs.shape == (dim, q) and fbs.shape == (T, dim, q) and pi.shape == (T, q ** dim)
    if variant == "nr1":
        pi = NC.not_rank1(pi)
    w = np.full(dim, 1.0 / dim)
    if alt:
        params, w = alt_params(case), np.array(NC.PORT_UNEQUAL[dim])
        fbs, pi = fbs[ALT_DATE:ALT_DATE + 1], pi[ALT_DATE:ALT_DATE + 1]
    x, step = F.x_grid(NC.N_OF[dim], "msm")
    return dict(model="msm", copula=copula, dim=dim, x_values=x, step=step, densities=F.msm_densities(uvs, x),
                combos=F.vol_combinations(dim, q), weights=w, copula_params=plan_params(copula, params),
                per_date=(fbs, pi), unique_vol_states=uvs)


def stress_event(x):
    """Axis 0's stress event of node_cases.events: (axis, (lo, hi))."""
    c, name, bounds = NC.events(x, 2)[0]
    assert c == 0 and name == "stress"
    return c, bounds


def case_digest(case, z):
    """SHA-256 of everything a case's truths are computed from."""
    kw, ka = problem_inputs(case, z), problem_inputs(case, z, alt=True)
    dim = case[1]
    parts = [np.ravel(np.asarray(case[2], dtype=np.float64)), [float(case[3])], kw["x_values"], np.ravel(kw["step"]),
             kw["weights"], np.ravel(kw["densities"]), np.ravel(kw["per_date"][0]), np.ravel(kw["per_date"][1]),
             np.ravel(kw["unique_vol_states"]), np.ravel(NC.slabs(dim)), np.ravel(stress_event(kw["x_values"])[1]),
             np.ravel(NC.PORT_UNEQUAL[dim]), np.ravel(alt_params(case)), ka["weights"], np.ravel(ka["per_date"][1]),
             np.ravel(LADDER)]
    return NC.digest(np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]))


def load_kat():
    return dict(np.load(KAT_PATH, allow_pickle=False))
