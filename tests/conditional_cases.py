"""The inputs on which the GPU tests compare the conditional quantiles with the checker exactly
(tests/test_conditional_gpu.py), in one place so that tests/test_conditional_cpu.py can assert
their premise (margin >= 1e-7) without a GPU.  An input is (Problem, copula params, ptf_mean, axis,
cond [T][2]); the checker's result is computed once per input and never modified."""
import functools
import os

import numpy as np

import conditional_reference as CR
import es_reference as E
from conftest import GOLDEN, GOLDEN_CASES, load_golden

LEVELS = (0.01, 0.05, 0.5)
STRESS = 0.05
BAND = (0.25, 0.75)
SMALL = [c for c in GOLDEN_CASES if c not in ("cfg2_n256", "cfg3_n128")]


# ------------------------------------------------------------------ problems
@functools.lru_cache(maxsize=None)
def problem(name):
    """(Problem, copula params, ptf_mean) by name: a golden case, or one of the built shapes."""
    from oracle import forecast as F
    from oracle.quadrature import Problem
    if name in GOLDEN_CASES:
        z = load_golden(name)
        return E.problem_of(z), z["copula_params"], float(z["ptf_mean"])
    if name.startswith("fullbatch"):                 # "fullbatch<cfg>_n<n>": the reference's grid at n
        cfg, n = (int(v) for v in name[len("fullbatch"):].split("_n"))   # points, first 4 dates
        z = dict(np.load(os.path.join(GOLDEN, f"fullbatch_cfg{cfg}.npz"), allow_pickle=False))
        model, T = str(z["model"]), 4
        x, step = F.x_grid(n, model)
        if model == "msm":
            uvs = z["unique_vol_states"]
            dens, combos = F.msm_densities(uvs, x), z["combos"]
            per = (z["forecasts_by_states"][:T], z["forecasts"][:T])
        else:
            uvs, dens, combos, per = None, np.ones((2, 1, n)), np.zeros((1, 2)), z["sigma_forecasts"][:T]
        P = Problem(model, str(z["copula"]), 2, x, step, dens, combos, z["weights"], z["copula_params"], per, uvs)
        return P, z["copula_params"], float(z["ptf_mean"])
    if name == "garch3d_n17":                        # 289 rows: a second 256-row chunk of 33
        z = load_golden("garch3d_student_n16")
        n, T = 17, 3
        x, step = F.x_grid(n, "garch")
        cp = np.array([5.0, 0.5, 0.4, 0.3])
        P = Problem("garch", "student", 3, x, step, np.ones((3, 1, n)), np.zeros((1, 3)), z["weights"], cp,
                    z["sigma_forecasts"][:T])
        return P, cp, 0.0
    z = load_golden("cfg2_n64")
    per = (z["forecasts_by_states"], z["forecasts"])
    if name == "cfg2_gumbel_survival":
        import gumbel_reference as G
        P = G.problem_of(z, "gumbel_survival", 2.0)
        return P, P.copula_params, float(z["ptf_mean"])
    w, cp = {"cfg2_weights": (np.array([0.3, 0.7]), z["copula_params"]),
             "cfg2_nu": (z["weights"], np.array([5.364, 0.5]))}[name]
    P = Problem("msm", "student", 2, z["x_values"], z["step"], z["densities"], z["combos"], w, cp, per,
                z["unique_vol_states"])
    return P, cp, float(z["ptf_mean"])


def dates(P, sl):
    """The same Problem on a slice of its dates."""
    per = (P.fbs[sl], P.pi[sl]) if P.model == "msm" else P.sigma[sl]
    return type(P)(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w, P.copula_params, per,
                   P.uvs if P.model == "msm" else None)


# ------------------------------------------------------------------ events
def event(P, axis, kind):
    """cond (T, 2) of an event on `axis`: "stress" = asset at or below its 5 % quantile, "band" =
    between its quartiles (both from the checker's marginal_quantile), "grid" = (x[10], x[25]],
    bounds exactly on grid values, "full" = (-inf, +inf]; "driver_stress" / "driver_band": the
    first two as ValueAtRiskCalcualtion.calc_covar forms them, from copula_var.conditional."""
    if kind.startswith("driver_"):
        from copula_var.conditional import marginal_quantile
        per, vs = ((P.fbs, P.pi), P.uvs) if P.model == "msm" else (P.sigma, None)
        lo, hi = (0.0, STRESS) if kind == "driver_stress" else BAND
        return np.column_stack((marginal_quantile(P.model, per, vs, axis, lo),
                                marginal_quantile(P.model, per, vs, axis, hi)))
    if kind == "stress":
        return np.column_stack((np.full(P.T, -np.inf), CR.marginal_quantile(P, axis, STRESS)))
    if kind == "band":
        return np.column_stack((CR.marginal_quantile(P, axis, BAND[0]), CR.marginal_quantile(P, axis, BAND[1])))
    if kind == "grid":
        return np.column_stack((np.full(P.T, P.x[10]), np.full(P.T, P.x[25])))
    assert kind == "full"
    return np.column_stack((np.full(P.T, -np.inf), np.full(P.T, np.inf)))


def _axes(name):
    return range(3 if name in ("cfg4_k4_n16", "cfg4_k6_n16", "garch3d_student_n16", "garch3d_n17") else 2)


# every (problem, axis, event) the GPU tests compare exactly
EXACT = ([(c, a, "stress") for c in SMALL for a in _axes(c)]
         + [(c, a, "band") for c in ("cfg2_n64", "cfg5_n64", "garch3d_student_n16") for a in _axes(c)]
         + [("fullbatch5_n70", a, k) for a in range(2) for k in ("stress", "band")]
         + [("fullbatch3_n130", a, "stress") for a in range(2)]
         + [("garch3d_n17", a, "stress") for a in range(3)]
         + [("cfg2_n64", a, k) for a in range(2) for k in ("grid", "full")]
         + [(c, a, "stress") for c in ("cfg2_weights", "cfg2_nu", "cfg2_gumbel_survival") for a in range(2)]
         + [(c, 0, k) for c in ("cfg2_n64", "garch_student_n64") for k in ("driver_stress", "driver_band")])


@functools.lru_cache(maxsize=None)
def reference(name, axis, kind):
    """(P, copula params, ptf_mean, cond, checker's (covar, coes, m0, p_event, margin)) at LEVELS."""
    P, cp, ptf = problem(name)
    cond = event(P, axis, kind)
    ref = CR.conditional_quantiles(P, axis, cond[:, 0], cond[:, 1], LEVELS, ptf)
    for a in (cond,) + ref:
        a.setflags(write=False)
    return P, cp, ptf, cond, ref
