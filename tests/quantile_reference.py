"""Checker for the exact quantile solve (cvq_quantiles): a numpy restatement of its definition on
the oracle's own terms (oracle.quadrature.Problem) and on tests/es_reference.py.

Per date t and level alpha > 0, with F(v) = Problem.slab(t, lower, v) (the mass of (lower, v]
under the reference's membership rule and node masses):

  lo, hi = min_var, max_var;  K = ceil(log2((max_var - min_var) / tolerance))
  not (F(lo) < alpha <= F(hi)):  var = es = NaN, m0 = F(hi)
  else K times: mid = (lo + hi) / 2; lo = mid if F(mid) < alpha else hi = mid
  var = (lo + hi) / 2 + ptf_mean;  es, m0 = es_reference.expected_shortfall of that var

margin[t, l] = min over every evaluated point (lo, hi and each mid) of |F - alpha| / alpha: how
far the closest decision was from flipping.  The device sums the same masses in another order
(relative error ~1e-13, bar 1e-10); with margin >= 1e-7 its decisions are the checker's, so its
var must be equal bit for bit.
"""
import math

import numpy as np

import es_reference as E


def bisection_steps(min_var=-7.5, max_var=0.0, tolerance=1e-6):
    return max(0, int(math.ceil(math.log2((max_var - min_var) / tolerance))))


def quantiles(P, levels, ptf_mean, min_var=-7.5, max_var=0.0, lower=-100.0, tolerance=1e-6):
    """(var, es, m0, margin), each (T, L)."""
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    K = bisection_steps(min_var, max_var, tolerance)
    T, L = P.T, levels.size
    var = np.full((T, L), np.nan)
    m0 = np.empty((T, L))
    margin = np.empty((T, L))
    for t in range(T):
        seen = {}                                     # the levels share their first mids

        def F(v):
            if v not in seen:
                seen[v] = P.slab(t, lower, v)
            return seen[v]

        for l, alpha in enumerate(levels):
            lo, hi = float(min_var), float(max_var)
            f_lo, f_hi = F(lo), F(hi)
            near = min(abs(f_lo - alpha), abs(f_hi - alpha))
            if not (f_lo < alpha <= f_hi):
                m0[t, l] = f_hi
                margin[t, l] = near / alpha
                continue
            for _ in range(K):
                mid = (lo + hi) / 2
                f = F(mid)
                near = min(near, abs(f - alpha))
                if f < alpha:
                    lo = mid
                else:
                    hi = mid
            var[t, l] = (lo + hi) / 2 + ptf_mean
            margin[t, l] = near / alpha
    es = np.full((T, L), np.nan)
    for l in range(L):
        e, m, _, _ = E.expected_shortfall(P, var[:, l], ptf_mean, lower)
        ok = ~np.isnan(var[:, l])
        es[ok, l] = e[ok]
        m0[ok, l] = m[ok]
    return var, es, m0, margin
