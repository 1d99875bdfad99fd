"""Per-date inputs of QuadraturePlan.dynamic_quantiles: buy-and-hold weights that drift with the
realised returns, the out-of-sample probability integral transforms of the forecast marginals,
copula parameters refitted on a rolling window, and the path of a score-driven copula recursion
fitted once (gas_copula_params; its likelihoods and its filter are the kernels of csrc/cvq_gas.hip).
Otherwise numpy / scipy only (the Student and Gaussian fits take their quantiles from the device
unless a host function is passed, as the optimisers of optim/copula_fit.py do).

Nothing here looks ahead: the weights and the parameters of out-of-sample date t are functions of
the rows before t alone.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np
from scipy import special
from scipy.optimize import minimize

SIGMA_MODELS = ("garch", "mean_reverting", "ukf")
COPULAS = ("gaussian", "student", "plackett", "gumbel", "gumbel_survival", "frank", "joe", "joe_survival")


# ---------------------------------------------------------------------- weights
def to_tickers(w: np.ndarray) -> np.ndarray:
    """Constructor-convention weights (..., dim) -> the weight each ticker carries (quirk Q10,
    QuadraturePlan.axis_weights: ticker c carries w[c + 1], the last ticker w[0])."""
    w = np.asarray(w, dtype=np.float64)
    return np.concatenate((w[..., 1:], w[..., :1]), axis=-1)


def from_tickers(a: np.ndarray) -> np.ndarray:
    """The inverse of to_tickers."""
    a = np.asarray(a, dtype=np.float64)
    return np.concatenate((a[..., -1:], a[..., :-1]), axis=-1)


def drift_weights(returns, w0) -> np.ndarray:
    """(T, dim) buy-and-hold weights for T dates: row 0 is w0 and
        a[t + 1, c]  proportional to  a[t, c] * exp(r[t, c] / 100),   renormalised to sum 1,
    where a[t, c] is the weight ticker c carries on date t and r = returns (T, dim) holds the
    tickers' log returns x 100 (the loader's unit), column c = ticker c.  Row t uses the returns
    of the dates before t only (the last row of `returns` is not read).  w0 and the result are in
    the constructor's weight convention, as --weights reaches the driver: ticker c carries
    weights[c + 1] and the last ticker weights[0] (quirk Q10, QuadraturePlan.axis_weights), so
    each entry drifts with the return of the ticker it weighs.  w0 must sum to 1."""
    r = np.asarray(returns, dtype=np.float64)
    w0 = np.asarray(w0, dtype=np.float64)
    if r.ndim != 2 or w0.shape != (r.shape[1],):
        raise ValueError("returns must be (T, dim) and w0 (dim,)")
    if not np.isclose(np.sum(w0), 1.0):
        raise ValueError("w0 must sum to 1")
    a = np.empty_like(r)
    if r.shape[0] == 0:
        return a
    a[0] = to_tickers(w0)
    for t in range(r.shape[0] - 1):
        g = a[t] * np.exp(r[t] / 100.0)
        a[t + 1] = g / np.sum(g)
    out = from_tickers(a)
    out[0] = w0                                            # the caller's own bits on the first date
    return out


# ---------------------------------------------------------------------- out-of-sample PITs
def oos_pits(model: str, per_date, vol_states, returns_c) -> Tuple[np.ndarray, np.ndarray]:
    """(u, pdf), each (T, dim): every asset's forecast-marginal CDF and density at the realised
    centred return of its date.  model "msm": per_date = (forecasts_by_states (T, dim, q),
    forecasts), vol_states (dim, q), u = sum_s f_t[s] Phi(r / sigma_s); a sigma model ("garch",
    "mean_reverting" / "ukf"): per_date = sigma forecasts (T, dim), bare or in the reference's
    one-element list, u = Phi(r / sigma_t).  returns_c (T, dim)."""
    r = np.asarray(returns_c, dtype=np.float64)
    if model == "msm":
        fbs = np.asarray(per_date[0], dtype=np.float64)
        uvs = np.asarray(vol_states, dtype=np.float64)
        if r.shape != fbs.shape[:2]:
            raise ValueError(f"returns_c must have shape {fbs.shape[:2]}")
        z = r[:, :, None] / uvs[None, :, :]
        u = np.sum(fbs * special.ndtr(z), axis=2)
        pdf = np.sum(fbs * np.exp(-0.5 * z * z) / (np.sqrt(2.0 * np.pi) * uvs[None, :, :]), axis=2)
        return u, pdf
    if model not in SIGMA_MODELS:
        raise ValueError(f"model must be 'msm' or one of {SIGMA_MODELS}")
    sigma = np.asarray(per_date[0] if isinstance(per_date, (list, tuple)) else per_date, dtype=np.float64)
    if r.shape != sigma.shape:
        raise ValueError(f"returns_c must have shape {sigma.shape}")
    z = r / sigma
    return special.ndtr(z), np.exp(-0.5 * z * z) / (np.sqrt(2.0 * np.pi) * sigma)


# ---------------------------------------------------------------------- rolling copula fits
def _triu(corr) -> np.ndarray:
    corr = np.asarray(corr, dtype=np.float64)
    return corr[np.triu_indices_from(corr, k=1)]


def fit_copula(copula: str, u, pdf, start=None, nu: Optional[float] = None, tppf: Optional[Callable] = None,
               ndtri: Optional[Callable] = None, device: int = 0) -> Tuple[np.ndarray, float]:
    """One IFM fit by the optimisers of optim/copula_fit.py on rows u / pdf (N, dim): (parameters
    in cvq_static.copula_params' packing, negative log-likelihood).  start=None: the optimiser's
    own starting points (the static fit); else the previous parameters, same packing.  Student:
    the correlations at the fixed nu (the optimiser's first stage at that nu alone)."""
    from .optim import copula_fit as F
    if copula == "gaussian":
        opt = F.GaussianCopulaOptimizer(u, pdf, device=device, ndtri=ndtri)
        res = opt.optimize(initial_corr=None if start is None else np.asarray(start, dtype=np.float64))
        return _triu(res["corr_matrix"]), float(res["nll"])
    if copula == "student":
        if nu is None:
            raise ValueError("the Student fit needs the plan's nu")
        opt = F.StudentCopulaOptimizer(u, pdf, nu_values=np.array([nu]), device=device, tppf=tppf)
        n_corr = opt.dim * (opt.dim - 1) // 2
        x0 = np.full(n_corr, 0.5) if start is None else np.asarray(start, dtype=np.float64)[1:]
        fun = lambda c: opt.negative_log_likelihood(np.hstack(([nu], c)))
        res = minimize(fun=fun, x0=x0, method="L-BFGS-B", bounds=[(-0.99, 0.99)] * n_corr, tol=opt.tol,
                       options={"maxiter": opt.max_iter})
        return np.hstack(([nu], res.x)), float(fun(res.x))
    if copula == "plackett":
        opt = F.PlackettCopulaOptimizer(u, pdf)
        res = opt.optimize(theta_range=None if start is None else [float(np.asarray(start).reshape(-1)[0])])
        if res["theta"] is None:
            raise ValueError("Plackett copula fit: no finite likelihood")
        return np.array([float(res["theta"])]), float(res["nll"])
    if copula in ("gumbel", "gumbel_survival"):
        opt = F.GumbelCopulaOptimizer(u, pdf, survival=copula == "gumbel_survival")
        res = opt.optimize(theta_range=None if start is None else (float(np.asarray(start).reshape(-1)[0]),))
        return np.array([float(res["theta"])]), float(res["nll"])
    if copula == "frank":
        opt = F.FrankCopulaOptimizer(u, pdf)
        res = opt.optimize(theta_range=None if start is None else (float(np.asarray(start).reshape(-1)[0]),))
        return np.array([float(res["theta"])]), float(res["nll"])
    if copula in ("joe", "joe_survival"):
        opt = F.JoeCopulaOptimizer(u, pdf, survival=copula == "joe_survival")
        res = opt.optimize(theta_range=None if start is None else (float(np.asarray(start).reshape(-1)[0]),))
        return np.array([float(res["theta"])]), float(res["nll"])
    raise ValueError(f"copula must be one of {COPULAS}")


def rolling_copula_params(copula: str, in_sample_marginals, in_sample_densities, oos_u, oos_pdf, window: int,
                          every: int = 21, static_params=None, tppf: Optional[Callable] = None,
                          ndtri: Optional[Callable] = None, device: int = 0, fit: Optional[Callable] = None
                          ) -> Tuple[np.ndarray, dict]:
    """(params (T, n_copula_params), info): the copula parameters of every out-of-sample date, in
    cvq_static.copula_params' packing, refitted on a rolling window.

    For each refit date t = 0, every, 2 every, ... the fit runs on the last `window` rows of
    [in-sample rows, then out-of-sample rows s < t] -- no row >= t ever enters it -- and its
    parameters hold until the next refit.  The first fit starts from the optimiser's own starting
    points (with window >= the in-sample length it is the static fit), each later one from the
    previous parameters.  static_params (the static fit, same packing) gives the Student nu, which
    stays fixed -- the plan's quantile tables hang on it -- and stands in where the first fit
    fails; a later failed fit (an exception, or a non-finite likelihood or parameter) keeps the
    previous parameters.  info: "refits" (the refit dates), "failed" (those whose fit failed),
    "nll" (per refit date, NaN where failed).  fit: the single-fit function (fit_copula's
    signature), for tests."""
    if copula not in COPULAS:
        raise ValueError(f"copula must be one of {COPULAS}")
    um, dm = np.asarray(in_sample_marginals, dtype=np.float64), np.asarray(in_sample_densities, dtype=np.float64)
    uo, do = np.asarray(oos_u, dtype=np.float64), np.asarray(oos_pdf, dtype=np.float64)
    if um.shape != dm.shape or uo.shape != do.shape or um.ndim != 2 or uo.ndim != 2 or um.shape[1] != uo.shape[1]:
        raise ValueError("marginals and densities must be (N, dim) in-sample and (T, dim) out-of-sample")
    window, every = int(window), int(every)
    if window < 2 or every < 1:
        raise ValueError("window must be >= 2 and every >= 1")
    static = None if static_params is None else np.atleast_1d(np.asarray(static_params, dtype=np.float64))
    nu = None
    if copula == "student":
        if static is None:
            raise ValueError("the Student copula needs static_params: its nu stays the plan's")
        nu = float(static[0])
    fit = fit or fit_copula
    T = uo.shape[0]
    rows_u, rows_d = np.vstack((um, uo)), np.vstack((dm, do))
    n_in = um.shape[0]
    prev, out = None, []
    info = {"refits": [], "failed": [], "nll": []}
    for t in range(T):
        if t % every == 0:
            end = n_in + t                                 # rows before out-of-sample date t
            lo = max(0, end - window)
            info["refits"].append(t)
            try:
                got, nll = fit(copula, rows_u[lo:end].copy(), rows_d[lo:end].copy(), start=prev, nu=nu, tppf=tppf,
                               ndtri=ndtri, device=device)
                got = np.atleast_1d(np.asarray(got, dtype=np.float64))
                ok = np.isfinite(nll) and nll < 1e10 and np.all(np.isfinite(got))
            except (ValueError, FloatingPointError, np.linalg.LinAlgError):
                got, nll, ok = None, np.nan, False
            if ok:
                prev = got
            else:
                info["failed"].append(t)
                nll = np.nan
                if prev is None:
                    if static is None:
                        raise ValueError("the first rolling copula fit failed and there are no static_params to keep")
                    prev = static.copy()
            info["nll"].append(float(nll))
        out.append(prev)
    n_par = len(out[0]) if out else (0 if static is None else static.size)
    return np.array(out, dtype=np.float64).reshape(T, n_par), info


# ---------------------------------------------------------------------- score-driven copula path
def gas_copula_params(copula: str, in_sample_marginals, oos_u, static_params, fit=None, device: int = 0,
                      in_sample_densities=None, path: Optional[Callable] = None) -> Tuple[np.ndarray, dict]:
    """(params (T, n_copula_params), info): the copula parameters of every out-of-sample date, in
    cvq_static.copula_params' packing (Student: [nu, rho_t]), from the score-driven recursion of
    optim.copula_fit.GasCopulaOptimizer (DESIGN.md §4 "Score-driven copula").

    The three recursion parameters are fitted once, on the in-sample rows only; the filter then runs
    once over [in-sample rows, then out-of-sample rows] and rows n_in ... n_in + T - 1 of its path are
    returned: the parameter of out-of-sample date t is a function of the rows before it alone.
    static_params (the static fit, same packing) gives the Student nu -- fixed, the plan's -- and the
    level the search starts from.  Marginals are clamped to [2^-53, 1 - 2^-53] as the optimiser does.
    fit: None (GasCopulaOptimizer on the device), a dict with "omega", "alpha", "beta" (a fit made
    elsewhere), or a function (copula, u_in, densities, nu, static_theta, device) -> such a dict.
    path: the filter, (u, params) -> (theta (N + 1,), logc (N,)); default engine.gas_path.
    in_sample_densities only shifts the reported likelihoods (default: ones).
    info: "fit" (the fit dict) and "in_sample_path" (theta_0 ... theta_{n_in - 1})."""
    from .optim import copula_fit as F
    if copula not in COPULAS:
        raise ValueError(f"copula must be one of {COPULAS}")
    um, uo = np.asarray(in_sample_marginals, dtype=np.float64), np.asarray(oos_u, dtype=np.float64)
    if um.ndim != 2 or uo.ndim != 2 or um.shape[1] != uo.shape[1]:
        raise ValueError("marginals must be (N, dim) in-sample and (T, dim) out-of-sample")
    static = np.atleast_1d(np.asarray(static_params, dtype=np.float64))
    if um.shape[1] != 2 and copula in ("gaussian", "student", "plackett"):
        raise ValueError(f"the score-driven {copula} copula is built for 2 assets")
    nu = float(static[0]) if copula == "student" else None
    dens = np.ones_like(um) if in_sample_densities is None else np.asarray(in_sample_densities, dtype=np.float64)
    if fit is None:
        fit = F.GasCopulaOptimizer(um, dens, copula, nu=nu, static_theta=static[-1], device=device).optimize()
    elif callable(fit):
        fit = fit(copula, um, dens, nu, float(static[-1]), device)
    prm = np.array([fit["omega"], fit["alpha"], fit["beta"]], dtype=np.float64)
    edge = F.GasCopulaOptimizer.EDGE
    rows = np.clip(np.vstack((um, uo)), edge, 1.0 - edge)
    if path is None:
        from . import engine
        path = lambda u, p: engine.gas_path(u, copula, p, nu=nu, device=device)      # noqa: E731
    theta, _ = path(rows, prm)
    n_in, T = um.shape[0], uo.shape[0]
    th = np.asarray(theta, dtype=np.float64)[n_in:n_in + T]
    out = np.column_stack((np.full(T, nu), th)) if copula == "student" else th.reshape(T, 1)
    return np.ascontiguousarray(out), {"fit": fit, "in_sample_path": np.asarray(theta, dtype=np.float64)[:n_in]}
