"""Checker for the conditional quantiles (cvq_conditional_quantiles: CoVaR / CoES): a numpy
restatement of the definition on the oracle's own terms (oracle.quadrature.Problem: mass,
inner_mask) and on tests/es_reference.py's levels.  It serves any object with that interface,
tests/gumbel_reference.py's Problem included.

Per date t, conditioning axis c (asset c, input order) and bounds (s_lo[t], s_hi[t]] in grid units:

  E_t     = { node : x[i_c] > s_lo[t] and x[i_c] <= s_hi[t] }      (a NaN bound, or s_hi <= s_lo: empty)
  F_E(v)  = sum of mass[ inner_mask(lower, v) & E_t ]
  p_E[t]  = F_E(+inf)
  target  = alpha * p_E[t]                                           (one FP64 product)
  K = ceil(log2((max_var - min_var) / tolerance))
  not (F_E(min_var) < target <= F_E(max_var)):  covar = coes = NaN, m0 = F_E(max_var)
  else K times: mid = (lo + hi) / 2; lo = mid if F_E(mid) < target else hi = mid
  covar = (lo + hi) / 2 + ptf_mean;  m0 = F_E(covar - ptf_mean)
  coes  = M1_E / m0 + ptf_mean, M1_E the level-weighted sum over the same nodes (NaN when m0 == 0)

margin[t, l] = min over every evaluated point (lo, hi and each mid) of |F_E - target| / target: how
far the closest decision was from flipping (inf where target == 0: nothing to decide).  With
margin >= 1e-7 the device's decisions are the checker's, so its covar must be equal bit for bit
(tests/quantile_reference.py).

marginal_quantile / marginal_cdf: a scipy restatement of copula_var.conditional.marginal_quantile.
"""
import numpy as np
from scipy import optimize, stats

import es_reference as E
from quantile_reference import bisection_steps


def event_mask(P, axis, s_lo, s_hi):
    """The event on grid axis `axis`, broadcastable against the box (n,) * dim."""
    x = P.x
    with np.errstate(invalid="ignore"):
        e = (x > s_lo) & (x <= s_hi)
    return e.reshape([P.n if a == axis else 1 for a in range(P.dim)])


def conditional_quantiles(P, axis, s_lo, s_hi, levels, ptf_mean, min_var=-7.5, max_var=0.0, lower=-100.0,
                          tolerance=1e-6):
    """(covar, coes, m0, p_event, margin): the first three and margin (T, L), p_event (T,)."""
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    s_lo = np.broadcast_to(np.asarray(s_lo, dtype=np.float64), (P.T,))
    s_hi = np.broadcast_to(np.asarray(s_hi, dtype=np.float64), (P.T,))
    if not 0 <= int(axis) < P.dim:
        raise ValueError("axis outside [0, dim)")
    K = bisection_steps(min_var, max_var, tolerance)
    T, L = P.T, levels.size
    lev = E.levels(P)
    covar = np.full((T, L), np.nan)
    coes = np.full((T, L), np.nan)
    m0 = np.empty((T, L))
    margin = np.empty((T, L))
    p_event = np.empty(T)
    for t in range(T):
        mass = P.mass(t)
        ev = np.broadcast_to(event_mask(P, int(axis), s_lo[t], s_hi[t]), mass.shape)
        seen = {}                                     # the levels share their first mids

        def F(v):
            if v not in seen:
                seen[v] = float(np.sum(mass[P.inner_mask(lower, v) & ev]))
            return seen[v]

        p_event[t] = F(np.inf)
        for l, alpha in enumerate(levels):
            target = alpha * p_event[t]
            lo, hi = float(min_var), float(max_var)
            f_lo, f_hi = F(lo), F(hi)
            near = min(abs(f_lo - target), abs(f_hi - target))
            if not (f_lo < target <= f_hi):
                m0[t, l] = f_hi
                margin[t, l] = near / target if target != 0.0 else np.inf
                continue
            for _ in range(K):
                mid = (lo + hi) / 2
                f = F(mid)
                near = min(near, abs(f - target))
                if f < target:
                    lo = mid
                else:
                    hi = mid
            margin[t, l] = near / target
            covar[t, l] = (lo + hi) / 2 + ptf_mean
            member = P.inner_mask(lower, covar[t, l] - ptf_mean) & ev
            m0[t, l] = float(np.sum(mass[member]))
            if m0[t, l] != 0.0:
                m1 = float(np.sum(np.broadcast_to(lev, mass.shape)[member] * mass[member]))
                coes[t, l] = m1 / m0[t, l] + ptf_mean
    return covar, coes, m0, p_event, margin


def conditional_mass(P, axis, s_lo, s_hi, v, lower=-100.0):
    """F_E(v) per date, (T,)."""
    s_lo = np.broadcast_to(np.asarray(s_lo, dtype=np.float64), (P.T,))
    s_hi = np.broadcast_to(np.asarray(s_hi, dtype=np.float64), (P.T,))
    out = np.empty(P.T)
    for t in range(P.T):
        mass = P.mass(t)
        ev = np.broadcast_to(event_mask(P, int(axis), s_lo[t], s_hi[t]), mass.shape)
        out[t] = float(np.sum(mass[P.inner_mask(lower, v) & ev]))
    return out


# ------------------------------------------------------------------ the asset's own marginal
def marginal_cdf(P, asset, s):
    """CDF of asset `asset`'s forecast marginal at the grid coordinates s (T,), per date."""
    s = np.asarray(s, dtype=np.float64)
    if P.model == "msm":
        return np.sum(P.fbs[:, asset, :] * stats.norm.cdf(s[:, None] / P.uvs[asset][None, :]), axis=1)
    return stats.norm.cdf(s / P.sigma[:, asset])


def marginal_quantile(P, asset, q):
    """(T,) the q-quantile of asset `asset`'s forecast marginal in grid units (scipy: norm.ppf for
    the sigma models, brentq on the mixture CDF for MSM)."""
    if q == 0.0:
        return np.full(P.T, -np.inf)
    if q == 1.0:
        return np.full(P.T, np.inf)
    z = float(stats.norm.ppf(q))
    if P.model != "msm":
        return P.sigma[:, asset] * z
    u = P.uvs[asset]
    a, b = min(u.min() * z, u.max() * z), max(u.min() * z, u.max() * z)
    span = max(b - a, 1e-9)
    out = np.empty(P.T)
    for t in range(P.T):
        w = P.fbs[t, asset, :]
        out[t] = optimize.brentq(lambda s: float(np.sum(w * stats.norm.cdf(s / u))) - q, a - span, b + span,
                                 xtol=1e-15, rtol=4 * np.finfo(float).eps, maxiter=500)
    return out
