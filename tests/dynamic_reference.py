"""Checker for the per-date-record quantiles (cvq_dynamic_quantiles): per date t,
tests/quantile_reference.py on a one-date oracle Problem that carries that date's copula
parameters, weights and mean -- the definition itself (a plan that differs only in those, given
date t alone), on the oracle's terms."""
import numpy as np

import quantile_reference as Q

LEVELS = (0.01, 0.025, 0.05)

# Per-date weights of the tests (the constructor's convention, quirk Q10): a power-of-two w0 (the
# reciprocal path), the division path, a negative weight.
W2 = np.array([(0.5, 0.5), (0.25, 0.75), (0.3, 0.7), (0.6, 0.4), (0.8, -0.2), (0.5, 0.5)])
W3 = np.array([(1 / 3, 1 / 3, 1 / 3), (0.5, 0.25, 0.25), (0.2, 0.3, 0.5), (0.7, 0.5, -0.2)])
# Per-date parameter paths
RHO2 = np.array([0.1, 0.3, 0.5, 0.7, -0.4, 0.9])
PLACKETT = np.array([0.5, 1.5, 3.0, 6.0, 12.0, 25.0])
GUMBEL = np.array([1.0, 1.3, 1.6, 2.5, 5.0, 16.0])
RHO3 = np.array([(0.5, 0.4, 0.3), (0.1, 0.2, 0.3), (0.8, 0.6, 0.7), (-0.3, 0.2, 0.1)])


def means(T):
    """ptf_mean_t[t] = 0.01 (t + 1): distinct per date, so that a swapped index shows."""
    return 0.01 * (np.arange(T) + 1.0)


def one_date(P, t, copula_params, weights):
    """The oracle Problem of P's date t alone under other copula parameters and weights (P's own
    class: a GumbelProblem stays one)."""
    per = (P.fbs[t:t + 1], P.pi[t:t + 1]) if P.model == "msm" else P.sigma[t:t + 1]
    return type(P)(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, np.asarray(weights, dtype=np.float64),
                   np.asarray(copula_params, dtype=np.float64), per, P.uvs if P.model == "msm" else None)


def dynamic_quantiles(problems, levels, ptf_mean_t, **kw):
    """(var, es, m0, margin), each (T, L): quantile_reference.quantiles on each date's one-date
    Problem (problems[t]) at ptf_mean_t[t]."""
    per = [Q.quantiles(P, levels, float(m), **kw) for P, m in zip(problems, ptf_mean_t)]
    assert all(r[0].shape[0] == 1 for r in per)
    return tuple(np.concatenate([r[k] for r in per], axis=0) for k in range(4))
