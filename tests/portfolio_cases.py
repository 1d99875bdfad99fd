"""Inputs of the batched-weights quantile tests, shared by tests/test_portfolio_cpu.py (which asserts
the checker's decision margins on them) and tests/test_portfolio_gpu.py (which compares the device
against the checker bit for bit under that premise).  Each case: an oracle Problem on a few dates,
the candidate weights, and the checker's result, computed once per process."""
import functools
import os

import numpy as np

import es_reference as E
import gumbel_reference as G
import portfolio_reference as R
from conftest import GOLDEN, load_golden

# golden case -> (candidates, dates): 2-D cases take W2 on 6 dates, 3-D cases W3 on 4
PARITY = {"cfg2_n64": (R.W2, 6), "cfg5_n64": (R.W2, 6), "msm_plackett_n64": (R.W2, 6),
          "garch_student_n64": (R.W2, 6), "cfg4_k4_n16": (R.W3, 4), "garch3d_student_n16": (R.W3, 4)}
# chunk and wave edges, as tests/test_quantiles_gpu.py builds them.  n = 130 leaves out
# (0.125, 0.875): its margin there is 5.8e-7, too close to the 1e-7 bar (the rest are >= 5.7e-6).
EDGES = {"2d_n70": R.W2, "2d_n130": R.W2[:-1], "3d_n17": R.W3}
GUMBEL = ("cfg2_n64", "gumbel_survival", 1.6)         # tests/test_gumbel_gpu.py's first case
OUTSIDE_LEVEL = 0.2                                   # msm_plackett_n64: F(max_var) straddles it


def _fullbatch_problem(cfg, n, T):
    from oracle import forecast as F
    from oracle.quadrature import Problem
    z = dict(np.load(os.path.join(GOLDEN, f"fullbatch_cfg{cfg}.npz"), allow_pickle=False))
    model = str(z["model"])
    x, step = F.x_grid(n, model)
    if model == "msm":
        uvs = z["unique_vol_states"]
        dens = F.msm_densities(uvs, x)
        per = (z["forecasts_by_states"][:T], z["forecasts"][:T])
        combos = z["combos"]
    else:
        uvs = None
        dens = np.ones((2, 1, n))
        per = z["sigma_forecasts"][:T]
        combos = np.zeros((1, 2))
    return Problem(model, str(z["copula"]), 2, x, step, dens, combos, z["weights"], z["copula_params"], per, uvs)


def _3d_n17():
    from oracle import forecast as F
    from oracle.quadrature import Problem
    z = load_golden("garch3d_student_n16")
    n, T = 17, 3
    x, step = F.x_grid(n, "garch")
    return Problem("garch", "student", 3, x, step, np.ones((3, 1, n)), np.zeros((1, 3)), z["weights"],
                   np.array([5.0, 0.5, 0.4, 0.3]), z["sigma_forecasts"][:T])


@functools.lru_cache(maxsize=None)
def problem(name):
    """(oracle Problem, candidate weights) of a case."""
    if name in PARITY:
        w, T = PARITY[name]
        return E.problem_of(load_golden(name), slice(0, T)), w
    if name == "2d_n70":
        return _fullbatch_problem(5, 70, 4), EDGES[name]
    if name == "2d_n130":
        return _fullbatch_problem(3, 130, 4), EDGES[name]
    if name == "3d_n17":
        return _3d_n17(), EDGES[name]
    if name == "gumbel":
        case, kind, theta = GUMBEL
        return G.problem_of(load_golden(case), kind, theta, slice(0, 6)), R.W2[:4]
    if name == "outside":
        return E.problem_of(load_golden("msm_plackett_n64")), R.W2
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The checker's (var, es, m0, margin), each (T, P, L), at R.LEVELS (case "outside": at
    (0.05, OUTSIDE_LEVEL)) and ptf_mean = R.means(P).  Computed once; treat as read-only."""
    P, w = problem(name)
    levels = (0.05, OUTSIDE_LEVEL) if name == "outside" else R.LEVELS
    return R.portfolio_quantiles(P, w, levels, R.means(len(w)))


def plan_of(P, strategy="auto", weights=None):
    """A device plan on P's inputs (weights: another vector than P's own)."""
    from copula_var.engine import QuadraturePlan
    p = QuadraturePlan(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w if weights is None else weights,
                       P.copula_params, vol_states=P.uvs if P.model == "msm" else None, strategy=strategy)
    p.set_dates((P.fbs, P.pi) if P.model == "msm" else [P.sigma])
    return p
