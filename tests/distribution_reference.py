"""Checker for the predictive distribution (cvq_distribution): per date, the tail moments of
every bin (e[b], e[b+1]] of a level ladder, on the oracle's own terms (es_reference.levels,
Problem.inner_mask = the reference's membership rule, Problem.mass = integrand x Delta).

The mass of a date is taken once and masked per bin.  Each bin stands alone: a NaN edge gives
an empty mask, and so does e[b+1] <= e[b]; +-inf edges go through inner_mask's own arithmetic
(+inf: every node of a row is at or below it; -inf: the lower edge clamps to the box, Q9).
"""
import numpy as np

import es_reference as E


def bin_moments(P, edges):
    """(m0, m1, m1_abs), each (T, B): the moments of the bins of `edges` -- (B + 1,) shared by
    every date or (T, B + 1) per date."""
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim == 1:
        e = np.broadcast_to(e, (P.T, e.size))
    assert e.shape[0] == P.T and e.shape[1] >= 2
    B = e.shape[1] - 1
    lev = E.levels(P)
    m0, m1, m1a = np.zeros((P.T, B)), np.zeros((P.T, B)), np.zeros((P.T, B))
    for t in range(P.T):
        mass = P.mass(t)                                   # once per date
        lm = np.broadcast_to(lev, mass.shape) * mass
        for b in range(B):
            with np.errstate(invalid="ignore"):
                mask = P.inner_mask(e[t, b], e[t, b + 1])
            m0[t, b] = float(np.sum(mass[mask]))
            m1[t, b] = float(np.sum(lm[mask]))
            m1a[t, b] = float(np.sum(np.abs(lm[mask])))
    return m0, m1, m1a


def pit(P, realised, ptf_mean=0.0, lower=-100.0):
    """u (T,) = F_t(r_t) / F_t(+inf) from bin_moments over [lower, r_t - ptf_mean, +inf]."""
    r = np.asarray(realised, dtype=np.float64)
    edges = np.column_stack((np.full(P.T, float(lower)), r - ptf_mean, np.full(P.T, np.inf)))
    m0 = bin_moments(P, edges)[0]
    tot = m0[:, 0] + m0[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.isnan(r) | (tot == 0.0), np.nan, m0[:, 0] / tot)
