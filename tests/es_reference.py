"""Checker for the tail moments and the Expected Shortfall: a numpy restatement on the
oracle's own terms (oracle.quadrature.Problem: inner_mask = the reference's membership
rule, mass = integrand x Delta).  The reference has no ES; this is the definition the
device entry points (cvq_slab_moments, cvq_expected_shortfall) are held to.

  level(node) = w[0] x[i_inner] + sum_{c < dim-1} w[c+1] x[i_c]   (as inner_mask weighs the axes)
  m0 = sum_mask mass   (bit for bit Problem.compute_integral's value)
  m1 = sum_mask level * mass,   m1_abs = sum_mask |level * mass|
  es = m1 / m0 + ptf_mean over (lower, var - ptf_mean]; NaN where var is NaN or m0 == 0.
"""
import numpy as np


def problem_of(z, sl=slice(None)):
    """oracle Problem of a golden case's arrays (optionally a slice of its dates)."""
    from oracle.quadrature import Problem
    model = str(z["model"])
    per = (z["forecasts_by_states"][sl], z["forecasts"][sl]) if model == "msm" else z["sigma_forecasts"][sl]
    return Problem(model, str(z["copula"]), int(z["dim"]), z["x_values"], z["step"], z["densities"],
                   z["combos"], z["weights"], z["copula_params"], per, z.get("unique_vol_states"))


def levels(P):
    """Portfolio level of every node of the box, shape (n,) * dim."""
    x, w, d = P.x, P.w, P.dim
    lev = (w[0] * x).reshape([1] * (d - 1) + [P.n])
    for c in range(d - 1):
        lev = lev + (w[c + 1] * x).reshape([P.n if a == c else 1 for a in range(d)])
    return lev


def tail_moments(P, bounds):
    """(m0, m1, m1_abs), each (T,), of the slabs (bounds[t, 0], bounds[t, 1]]."""
    bounds = np.asarray(bounds, dtype=np.float64)
    lev = levels(P)
    m0, m1, m1a = np.zeros(P.T), np.zeros(P.T), np.zeros(P.T)
    for t in range(P.T):
        mask = P.inner_mask(bounds[t, 0], bounds[t, 1])
        mass = P.mass(t)
        lm = np.broadcast_to(lev, mass.shape)[mask] * mass[mask]
        m0[t] = float(np.sum(mass[mask]))
        m1[t] = float(np.sum(lm))
        m1a[t] = float(np.sum(np.abs(lm)))
    return m0, m1, m1a


def expected_shortfall(P, var, ptf_mean, lower=-100.0):
    """(es, m0, m1, m1_abs) for a solved VaR vector (ptf_mean included, as calc_var returns it)."""
    var = np.asarray(var, dtype=np.float64)
    b = np.column_stack((np.full(P.T, float(lower)), var - ptf_mean))
    m0, m1, m1a = tail_moments(P, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        es = np.where(np.isnan(var) | (m0 == 0.0), np.nan, m1 / m0 + ptf_mean)
    return es, m0, m1, m1a
