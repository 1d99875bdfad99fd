"""Stress events for the conditional quantiles (CoVaR / CoES): quantiles of one asset's forecast
marginal, in grid units.  numpy / scipy only, importable without a GPU.

The event of QuadraturePlan.conditional_quantiles is an interval of grid coordinates on the
conditioning asset's axis.  The usual events are stated as probabilities of that asset's own
forecast distribution ("asset i at or below its 5 % quantile", "asset i between its quartiles");
marginal_quantile turns such a probability into the grid coordinate, per date:

  GARCH / UKF   x_i ~ N(0, sigma_t,i^2):                    s = sigma_t,i * ndtri(q)
  MSM           x_i ~ sum_s fbs[t, i, s] N(0, uvs[i, s]^2): the root of
                sum_s fbs[t, i, s] * Phi(s / uvs[i, s]) = q, by bisection to convergence.
"""
from __future__ import annotations

import numpy as np
from scipy import special


def _msm_cdf(fbs_a: np.ndarray, uvs_a: np.ndarray, s: np.ndarray) -> np.ndarray:
    return np.sum(fbs_a * special.ndtr(s[:, None] / uvs_a[None, :]), axis=1)


def marginal_quantile(model: str, per_date, vol_states, asset: int, q: float) -> np.ndarray:
    """(T,) the q-quantile of asset `asset`'s forecast marginal in grid units.  model: "msm"
    (per_date = (forecasts_by_states (T, dim, q), forecasts), vol_states (dim, q)) or a sigma
    model, "garch" / "mean_reverting" / "ukf" (per_date = sigma forecasts (T, dim), bare or in the
    reference's one-element list).  q = 0 gives
    -inf and q = 1 gives +inf on every date."""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError("q must be in [0, 1]")
    if model == "msm":
        fbs = np.asarray(per_date[0], dtype=np.float64)
        T, dim = fbs.shape[0], fbs.shape[1]
    else:
        # the reference wraps the sigma forecasts in a one-element list (QuadraturePlan.set_dates)
        sigma = np.asarray(per_date[0] if isinstance(per_date, (list, tuple)) else per_date, dtype=np.float64)
        T, dim = sigma.shape[0], sigma.shape[1]
    asset = int(asset)
    if not 0 <= asset < dim:
        raise ValueError(f"asset must be in [0, {dim})")
    if q == 0.0:
        return np.full(T, -np.inf)
    if q == 1.0:
        return np.full(T, np.inf)
    z = float(special.ndtri(q))
    if model != "msm":
        return sigma[:, asset] * z
    fbs_a = fbs[:, asset, :]
    uvs_a = np.asarray(vol_states, dtype=np.float64)[asset]
    # the mixture's quantile lies between its narrowest and widest component's
    lo = np.full(T, min(uvs_a.min() * z, uvs_a.max() * z))
    hi = np.full(T, max(uvs_a.min() * z, uvs_a.max() * z))
    while True:
        mid = (lo + hi) / 2
        if np.all((mid <= lo) | (mid >= hi)):          # no double left strictly between them
            return mid
        below = _msm_cdf(fbs_a, uvs_a, mid) < q
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
