"""Checker for the per-axis moments and the risk contributions: a numpy restatement on the
oracle's own terms (oracle.quadrature.Problem: inner_mask = the reference's membership rule,
mass = integrand x Delta), next to tests/es_reference.py.  The reference has no attribution;
this is the definition the device entry points (cvq_slab_axis_moments, cvq_es_contributions)
are held to.

  m0     = sum_mask mass                       (es_reference's m0 bit for bit)
  mx[c]  = sum_mask x[i_c] * mass              for grid axis c = asset c in input order
  mx_abs = sum_mask |x[i_c] * mass|            (x changes sign: the error scale of mx)
  wa[c]  = the weight inner_mask gives axis c: wa[dim-1] = w[0], wa[c] = w[c+1] (Q10)
  contrib[c] = wa[c] * mx[c] / m0 over (lower, var - ptf_mean]; the row is NaN where var is
               NaN or m0 == 0.  sum_c contrib[c] = es - ptf_mean.
"""
import numpy as np

import es_reference as E


def axis_weights(P):
    """wa (dim,): the weight of axis c in es_reference.levels."""
    w = np.asarray(P.w, dtype=np.float64)
    return np.concatenate((w[1:P.dim], w[:1]))


def axis_moments(P, bounds):
    """(m0 (T,), mx (T, dim), mx_abs (T, dim)) of the slabs (bounds[t, 0], bounds[t, 1]]."""
    bounds = np.asarray(bounds, dtype=np.float64)
    d = P.dim
    m0, mx, mxa = np.zeros(P.T), np.zeros((P.T, d)), np.zeros((P.T, d))
    for t in range(P.T):
        mask = P.inner_mask(bounds[t, 0], bounds[t, 1])
        mass = P.mass(t)
        m0[t] = float(np.sum(mass[mask]))
        for c in range(d):
            xc = np.broadcast_to(P.x.reshape([P.n if a == c else 1 for a in range(d)]), mass.shape)
            xm = xc[mask] * mass[mask]
            mx[t, c] = float(np.sum(xm))
            mxa[t, c] = float(np.sum(np.abs(xm)))
    return m0, mx, mxa


def contributions_of(P, m0, mx, valid):
    """wa[c] * mx[c] / m0 per row; NaN rows where not valid or m0 == 0."""
    ok = np.asarray(valid, dtype=bool) & (m0 != 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok[:, None], axis_weights(P) * mx / m0[:, None], np.nan)


def es_contributions(P, var, ptf_mean, lower=-100.0):
    """(contrib (T, dim), m0, mx, mx_abs) for a solved VaR vector (ptf_mean included)."""
    var = np.asarray(var, dtype=np.float64)
    b = np.column_stack((np.full(P.T, float(lower)), var - ptf_mean))
    m0, mx, mxa = axis_moments(P, b)
    return contributions_of(P, m0, mx, ~np.isnan(var)), m0, mx, mxa


def var_contributions(P, var, ptf_mean, band):
    """(contrib (T, dim), band_mean (T,), m0, mx, mx_abs) over (var - ptf_mean - band, var - ptf_mean];
    band_mean = m1 / m0 of that band from es_reference's own m1."""
    var = np.asarray(var, dtype=np.float64)
    top = var - ptf_mean
    b = np.column_stack((top - band, top))
    m0, mx, mxa = axis_moments(P, b)
    _, m1, _ = E.tail_moments(P, b)
    ok = ~np.isnan(var) & (m0 != 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(ok, m1 / m0, np.nan)
    return contributions_of(P, m0, mx, ~np.isnan(var)), mean, m0, mx, mxa
