"""Backtests of the VaR / ES forecasts against realised returns (no reference counterpart: the
reference plots its VaR series next to the returns and stops there).

Two device-backed pieces, both on QuadraturePlan.distribution (cvq_distribution: the mass of the
nested-grid measure in many level bins per date in one sweep), or on
QuadraturePlan.dynamic_distribution where the forecast has per-date copula parameters, weights or
means (the model behind dynamic_quantiles):

  predictive_cdf  -- F_t at K thresholds per date;
  pit             -- u_t = F_t(r_t) / F_t(+inf), the probability integral transform of a
                     realised return.

The measure is not normalised, so both divide by the date's total mass,
the sum of the ladder's bins up to +inf.

The statistics are plain numpy / scipy on the host, each a small dict:

  hits, kupiec_pof, christoffersen  -- unconditional and conditional coverage of the VaR hits;
  acerbi_szekely_z2                 -- the ES test statistic Z2 (statistic only);
  berkowitz                         -- the density-forecast LR test on the PITs;
  pinball                           -- the mean quantile score;
  backtest_table                    -- all of them in one dict.
"""
from __future__ import annotations

import numpy as np
from scipy import stats
from scipy.special import xlogy

PIT_CLIP = 1e-12          # berkowitz: u is clipped to [PIT_CLIP, 1 - PIT_CLIP] before norm.ppf


# ------------------------------------------------------------------ device-backed pieces
def _per_date(plan, ptf_mean, copula_params, weights):
    """(dynamic, mean): whether the call goes to plan.dynamic_distribution (per-date parameters,
    weights or means), and the mean as given (scalar) or as a checked (T,) vector."""
    m = np.asarray(ptf_mean, dtype=np.float64)
    if m.ndim == 0:
        return copula_params is not None or weights is not None, ptf_mean
    if m.shape != (plan.T,):
        raise ValueError(f"ptf_mean must be a scalar or have shape ({plan.T},)")
    return True, m


def predictive_cdf(plan, thresholds, ptf_mean=0.0, lower: float = -100.0, copula_params=None, weights=None):
    """(F (T, K), total (T,)): the normalised predictive CDF of the portfolio return at K
    ascending thresholds (returns, ptf_mean included) -- shared by every date (K,) or per date
    (T, K).  The ladder is [lower, thresholds - ptf_mean ..., +inf]; F is the running sum of the
    bin masses divided by `total`, the sum of all K + 1 bins.  F is NaN where total == 0.
    copula_params (T, n_copula_params) / weights (T, dim) / a (T,) ptf_mean: the forecast of
    plan.dynamic_quantiles, every date under its own parameters, weights and mean
    (plan.dynamic_distribution); with both None and a scalar mean the plan's static model
    (plan.distribution)."""
    th = np.asarray(thresholds, dtype=np.float64)
    if th.ndim not in (1, 2) or th.shape[-1] < 1:
        raise ValueError("thresholds must have shape (K,) or (T, K) with K >= 1")
    dynamic, mean = _per_date(plan, ptf_mean, copula_params, weights)
    if np.ndim(mean) == 1:                            # a ladder per date, each centred on its own mean
        th = np.broadcast_to(th, (plan.T, th.shape[-1])) - mean[:, None]
    else:
        th = th - mean
    lead = th.shape[:-1]
    edges = np.concatenate((np.full(lead + (1,), float(lower)), th, np.full(lead + (1,), np.inf)), axis=-1)
    if dynamic:
        mass, _ = plan.dynamic_distribution(edges, copula_params=copula_params, weights=weights)
    else:
        mass, _ = plan.distribution(edges)
    total = mass.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        F = np.where(total[:, None] != 0.0, np.cumsum(mass[:, :-1], axis=1) / total[:, None], np.nan)
    return F, total


def pit(plan, realised, ptf_mean=0.0, lower: float = -100.0, copula_params=None, weights=None) -> np.ndarray:
    """u (T,): the probability integral transform of each date's realised portfolio return
    (ptf_mean included) under that date's forecast, u = bin0 / (bin0 + bin1) over the per-date
    ladder [lower, realised[t] - ptf_mean, +inf].  NaN where the return is NaN or the total
    mass is 0.  copula_params / weights / a (T,) ptf_mean as in predictive_cdf: the PIT under the
    per-date model that plan.dynamic_quantiles forecasts with."""
    r = np.asarray(realised, dtype=np.float64)
    if r.shape != (plan.T,):
        raise ValueError(f"realised must have shape ({plan.T},)")
    dynamic, mean = _per_date(plan, ptf_mean, copula_params, weights)
    edges = np.column_stack((np.full(r.size, float(lower)), r - mean, np.full(r.size, np.inf)))
    if dynamic:
        mass, _ = plan.dynamic_distribution(edges, copula_params=copula_params, weights=weights)
    else:
        mass, _ = plan.distribution(edges)
    total = mass[:, 0] + mass[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.isnan(r) | (total == 0.0), np.nan, mass[:, 0] / total)


# ------------------------------------------------------------------ hit sequence
def hits(realised, var) -> dict:
    """The VaR violations realised < var (strict).  Dates with a NaN on either side are dropped
    and counted: {"hit": bool array of the kept dates, "keep": mask over all dates, "n", "x",
    "dropped"}."""
    r, v = np.asarray(realised, dtype=np.float64), np.asarray(var, dtype=np.float64)
    if r.shape != v.shape or r.ndim != 1:
        raise ValueError("realised and var must be vectors of one length")
    keep = ~(np.isnan(r) | np.isnan(v))
    h = r[keep] < v[keep]
    return {"hit": h, "keep": keep, "n": int(h.size), "x": int(h.sum()), "dropped": int((~keep).sum())}


def _hit_array(h) -> np.ndarray:
    return np.asarray(h["hit"] if isinstance(h, dict) else h, dtype=bool)


def _check_alpha(alpha: float) -> float:
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must be in (0, 1)")
    return alpha


def _lr_pof(n: int, x: int, alpha: float) -> float:
    if n == 0:
        return float("nan")
    return float(-2.0 * (xlogy(n - x, 1.0 - alpha) + xlogy(x, alpha) - xlogy(n - x, 1.0 - x / n) - xlogy(x, x / n)))


def kupiec_pof(h, alpha: float) -> dict:
    """Kupiec's proportion-of-failures test of unconditional coverage:
    LR = -2[(n-x) ln(1-alpha) + x ln alpha - (n-x) ln(1-x/n) - x ln(x/n)] with 0 ln 0 = 0,
    chi2(1) under the null."""
    h, alpha = _hit_array(h), _check_alpha(alpha)
    n, x = int(h.size), int(h.sum())
    lr = _lr_pof(n, x, alpha)
    return {"statistic": lr, "p_value": float(stats.chi2.sf(lr, 1)), "n": n, "x": x,
            "hit_rate": x / n if n else float("nan")}


def christoffersen(h, alpha: float) -> dict:
    """Christoffersen's independence and conditional-coverage tests from the transition counts
    n_ij (i = yesterday's hit, j = today's): LR_ind = -2[ln L(pi) - ln L(pi01, pi11)] with
    0 ln 0 = 0, chi2(1); LR_cc = LR_pof + LR_ind, chi2(2)."""
    h, alpha = _hit_array(h), _check_alpha(alpha)
    a, b = h[:-1], h[1:]
    n00, n01 = int(np.sum(~a & ~b)), int(np.sum(~a & b))
    n10, n11 = int(np.sum(a & ~b)), int(np.sum(a & b))
    m = n00 + n01 + n10 + n11
    pi = (n01 + n11) / m if m else 0.0
    pi01 = n01 / (n00 + n01) if n00 + n01 else 0.0        # an empty row contributes 0 ln 0 = 0 whatever pi is
    pi11 = n11 / (n10 + n11) if n10 + n11 else 0.0
    l0 = xlogy(n00 + n10, 1.0 - pi) + xlogy(n01 + n11, pi)
    l1 = xlogy(n00, 1.0 - pi01) + xlogy(n01, pi01) + xlogy(n10, 1.0 - pi11) + xlogy(n11, pi11)
    lr_ind = float(-2.0 * (l0 - l1)) if m else float("nan")
    lr_pof = _lr_pof(int(h.size), int(h.sum()), alpha)
    lr_cc = lr_pof + lr_ind
    return {"lr_ind": lr_ind, "p_ind": float(stats.chi2.sf(lr_ind, 1)), "lr_pof": lr_pof, "lr_cc": lr_cc,
            "p_cc": float(stats.chi2.sf(lr_cc, 2)), "statistic": lr_cc, "p_value": float(stats.chi2.sf(lr_cc, 2)),
            "n00": n00, "n01": n01, "n10": n10, "n11": n11}


# ------------------------------------------------------------------ ES, density, score
def acerbi_szekely_z2(realised, var, es, alpha: float) -> dict:
    """Acerbi-Szekely's second ES statistic, Z2 = 1 - (1 / (n alpha)) sum_t r_t hit_t / es_t with
    returns and es signed as calc_es returns them (both negative in the tail).  Expectation 0
    under a correct forecast; negative: the risk is understated.  Statistic only (its p-value
    needs simulation from the forecast).  Dates with a NaN in any of the three are dropped."""
    r, v, e = (np.asarray(z, dtype=np.float64) for z in (realised, var, es))
    alpha = _check_alpha(alpha)
    if not (r.shape == v.shape == e.shape) or r.ndim != 1:
        raise ValueError("realised, var and es must be vectors of one length")
    keep = ~(np.isnan(r) | np.isnan(v) | np.isnan(e))
    r, v, e = r[keep], v[keep], e[keep]
    h = r < v
    n = int(r.size)
    z2 = 1.0 - float(np.sum(r[h] / e[h])) / (n * alpha) if n else float("nan")
    return {"statistic": z2, "n": n, "x": int(h.sum()), "dropped": int((~keep).sum())}


def berkowitz(pit_values) -> dict:
    """Berkowitz's LR test of the density forecasts: z = norm.ppf(clip(u, 1e-12, 1 - 1e-12)), a
    Gaussian AR(1) z_t - mu = rho (z_{t-1} - mu) + eps_t fitted by conditional least squares on
    z[1:] given z[:-1], LR = -2[L(mu=0, sigma=1, rho=0) - L(mu^, sigma^, rho^)] on the same
    conditional likelihood, chi2(3).  NaN PITs are dropped and counted (the series is joined
    over them)."""
    u = np.asarray(pit_values, dtype=np.float64).ravel()
    keep = ~np.isnan(u)
    z = stats.norm.ppf(np.clip(u[keep], PIT_CLIP, 1.0 - PIT_CLIP))
    out = {"n": int(z.size), "dropped": int((~keep).sum())}
    if z.size < 4:
        out.update(statistic=float("nan"), p_value=float("nan"), mu=float("nan"), sigma=float("nan"),
                   rho=float("nan"))
        return out
    y, x = z[1:], z[:-1]
    xc = x - x.mean()
    sxx = float(np.sum(xc * xc))
    rho = float(np.sum(xc * (y - y.mean())) / sxx) if sxx > 0.0 else 0.0
    c = float(y.mean() - rho * x.mean())
    resid = y - c - rho * x
    s2 = float(np.mean(resid * resid))
    m = y.size
    l1 = -0.5 * m * (np.log(2.0 * np.pi * s2) + 1.0)
    l0 = -0.5 * m * np.log(2.0 * np.pi) - 0.5 * float(np.sum(y * y))
    lr = float(-2.0 * (l0 - l1))
    out.update(statistic=lr, p_value=float(stats.chi2.sf(lr, 3)), mu=c / (1.0 - rho) if rho != 1.0 else float("nan"),
               sigma=float(np.sqrt(s2)), rho=rho)
    return out


def pinball(realised, var, alpha: float) -> dict:
    """The mean quantile (pinball) score of the VaR as an alpha-quantile forecast,
    mean (alpha - 1{r < var}) (r - var); lower is better.  NaN dates are dropped."""
    alpha = _check_alpha(alpha)
    k = hits(realised, var)
    r = np.asarray(realised, dtype=np.float64)[k["keep"]]
    v = np.asarray(var, dtype=np.float64)[k["keep"]]
    score = float(np.mean((alpha - k["hit"]) * (r - v))) if k["n"] else float("nan")
    return {"statistic": score, "n": k["n"], "dropped": k["dropped"]}


def backtest_table(realised, var, es=None, pit=None, alpha: float = 0.05) -> dict:
    """Every test above for one VaR series: counts, Kupiec, Christoffersen, the pinball score, Z2
    when `es` is given and Berkowitz when `pit` is given."""
    k = hits(realised, var)
    table = {"alpha": _check_alpha(alpha), "n": k["n"], "hits": k["x"], "dropped": k["dropped"],
             "hit_rate": k["x"] / k["n"] if k["n"] else float("nan"),
             "kupiec": kupiec_pof(k, alpha), "christoffersen": christoffersen(k, alpha),
             "pinball": pinball(realised, var, alpha)}
    if es is not None:
        table["z2"] = acerbi_szekely_z2(realised, var, es, alpha)
    if pit is not None:
        table["berkowitz"] = berkowitz(pit)
    return table


def format_table(table: dict, title: str = "") -> str:
    """A backtest_table as the lines the driver prints."""
    ku, ch = table["kupiec"], table["christoffersen"]
    lines = [f"backtest {title}".rstrip() + f": alpha {table['alpha']:g}, {table['n']} dates "
             f"({table['dropped']} dropped), hits {table['hits']} (rate {table['hit_rate']:.4f})",
             f"  Kupiec POF       LR {ku['statistic']:.4f}  p {ku['p_value']:.4f}",
             f"  Christoffersen   LR_ind {ch['lr_ind']:.4f}  p {ch['p_ind']:.4f}   LR_cc {ch['lr_cc']:.4f}  "
             f"p {ch['p_cc']:.4f}   (n00 {ch['n00']} n01 {ch['n01']} n10 {ch['n10']} n11 {ch['n11']})",
             f"  pinball score    {table['pinball']['statistic']:.6f}"]
    if "z2" in table:
        lines.append(f"  Acerbi-Szekely   Z2 {table['z2']['statistic']:.4f}")
    if "berkowitz" in table:
        bk = table["berkowitz"]
        lines.append(f"  Berkowitz        LR {bk['statistic']:.4f}  p {bk['p_value']:.4f}   (mu {bk['mu']:.4f} "
                     f"sigma {bk['sigma']:.4f} rho {bk['rho']:.4f}, {bk['n']} PITs, {bk['dropped']} dropped)")
    return "\n".join(lines)
