"""Checker for the batched-weights quantiles (cvq_portfolio_quantiles): tests/quantile_reference.py
on oracle Problems that differ only in their weight vector, stacked to (T, P, L).

The measure does not depend on the weights (only inner_mask and the level do), so the copies
share the base Problem's node-mass cache; everything else is quantile_reference.quantiles."""
import copy

import numpy as np

import quantile_reference as Q

# Candidate sets of the tests (the constructor's own convention, quirk Q10).  W2: a power-of-two w0
# (the reciprocal path), the division path, a zero and a negative weight.
W2 = np.array([(0.5, 0.5), (0.25, 0.75), (0.75, 0.25), (0.3, 0.7), (0.6, 0.4), (1.0, 0.0), (0.8, -0.2),
               (0.125, 0.875)])
W3 = np.array([(1 / 3, 1 / 3, 1 / 3), (0.5, 0.25, 0.25), (0.25, 0.5, 0.25), (0.2, 0.3, 0.5), (0.6, 0.4, 0.0),
               (0.7, 0.5, -0.2)])
LEVELS = (0.01, 0.025, 0.05)


def means(P):
    """ptf_mean[p] = 0.01 (p + 1): distinct per candidate, so that a swapped index shows."""
    return 0.01 * (np.arange(P) + 1.0)


def with_weights(P, w):
    """A Problem that differs from P only in its weights (the node masses are shared)."""
    Pw = copy.copy(P)
    Pw.w = np.asarray(w, dtype=np.float64)
    assert Pw.w.shape == (P.dim,)
    return Pw


def portfolio_quantiles(P, weights, levels, ptf_mean, **kw):
    """(var, es, m0, margin), each (T, P, L): quantile_reference.quantiles per weight vector."""
    weights = np.asarray(weights, dtype=np.float64)
    pm = np.broadcast_to(np.asarray(ptf_mean, dtype=np.float64), (weights.shape[0],))
    per = [Q.quantiles(with_weights(P, w), levels, float(m), **kw) for w, m in zip(weights, pm)]
    return tuple(np.stack([r[k] for r in per], axis=1) for k in range(4))
