"""Inputs of the per-date-record quantile tests, shared by tests/test_dynamic_cpu.py (which asserts
the checker's decision margins on them) and tests/test_dynamic_gpu.py (which compares the device
against the checker bit for bit under that premise).  Each case: a base oracle Problem on a few
dates (the device plan's own parameters and weights), the per-date parameter and weight paths, the
one-date Problems the definition speaks of, and the checker's result, computed once per process."""
import functools

import numpy as np

import dynamic_reference as R
import es_reference as E
import gumbel_reference as G
import portfolio_cases as PC
from conftest import load_golden

# case -> (golden, copula the golden must hold, Gumbel kind or None).  2-D cases: 6 dates, 3-D: 4.
CASES = {"cfg2_n64": ("cfg2_n64", "student", None),
         "garch_student_n64": ("garch_student_n64", "student", None),
         "cfg5_n64": ("cfg5_n64", "student", None),
         "msm_gauss_n64": ("msm_gauss_n64", "gaussian", None),
         "msm_plackett_n64": ("msm_plackett_n64", "plackett", None),
         "cfg2_n64_gumbel_survival": ("cfg2_n64", "student", "gumbel_survival"),
         "cfg5_n64_gumbel": ("cfg5_n64", "student", "gumbel"),
         "cfg4_k4_n16": ("cfg4_k4_n16", "gaussian", None),
         "garch3d_student_n16": ("garch3d_student_n16", "student", None)}
# chunk and wave edges, as tests/portfolio_cases.py builds them: 2-D n = 70 (2 chunks of 64 rows, the
# second with 6 live rows), n = 130 (3 chunks, the last with 2 rows), 3-D n = 17 (289 rows: a second
# 256-row chunk of 33).  A level whose CPU margin fell under the 1e-7 bar would be left out here;
# none does (the smallest, n = 130 at 0.05, is 5.4e-5: tests/test_dynamic_cpu.py asserts them).
EDGES = {"2d_n70": R.LEVELS, "2d_n130": R.LEVELS, "3d_n17": R.LEVELS}


def param_path(copula, dim, T, nu=None):
    """(T, n_copula_params) in cvq_static.copula_params' packing."""
    if copula in G.KINDS:
        return R.GUMBEL[:T, None].copy()
    if copula == "plackett":
        return R.PLACKETT[:T, None].copy()
    rho = R.RHO2[:T, None] if dim == 2 else R.RHO3[:T]
    return np.column_stack((np.full(T, float(nu)), rho)) if copula == "student" else rho.copy()


def _base(name):
    if name in CASES:
        golden, copula, kind = CASES[name]
        z = load_golden(golden)
        assert str(z["copula"]) == copula, (name, str(z["copula"]))
        T = 6 if int(z["dim"]) == 2 else 4
        if kind is not None:
            return G.problem_of(z, kind, R.GUMBEL[2], slice(0, T))
        return E.problem_of(z, slice(0, T))
    return PC.problem(name)[0]


@functools.lru_cache(maxsize=None)
def problem(name):
    """(base Problem, copula_params_t (T, ncp), weights_t (T, dim), ptf_mean_t (T,), one-date
    Problems).  Treat as read-only."""
    P = _base(name)
    nu = float(np.asarray(P.copula_params).reshape(-1)[0]) if P.copula == "student" else None
    cp = param_path(P.copula, P.dim, P.T, nu)
    w = (R.W2 if P.dim == 2 else R.W3)[:P.T].copy()
    if name in CASES and CASES[name][2] is None:
        # the definition's own route: the golden's arrays with date t's parameters and weights
        z = dict(load_golden(CASES[name][0]))
        dates = []
        for t in range(P.T):
            z["copula_params"], z["weights"] = cp[t], w[t]
            dates.append(E.problem_of(z, slice(t, t + 1)))
    elif name in CASES:
        z = dict(load_golden(CASES[name][0]))
        dates = []
        for t in range(P.T):
            z["weights"] = w[t]
            dates.append(G.problem_of(z, CASES[name][2], cp[t, 0], slice(t, t + 1)))
    else:
        dates = [R.one_date(P, t, cp[t], w[t]) for t in range(P.T)]
    return P, cp, w, R.means(P.T), tuple(dates)


def levels(name):
    return EDGES.get(name, R.LEVELS)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The checker's (var, es, m0, margin), each (T, L), at the case's levels.  Computed once; treat
    as read-only."""
    _, _, _, pm, dates = problem(name)
    return R.dynamic_quantiles(dates, levels(name), pm)


plan_of = PC.plan_of
