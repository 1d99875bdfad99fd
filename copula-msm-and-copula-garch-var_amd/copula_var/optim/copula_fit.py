"""Copula fits by inference for margins (copulas/{student,gaussian,plackett}/opti.py)
with the quantile transforms on the device.

The reference's Student objective (student/opti.py:34-64 -> inference_for_margins.py:38-55
-> student.py:49-174) spends most of its time in a scalar ``scipy.stats.t.ppf`` loop
over the N x dim marginals (student.py:96-102).  Here one device
launch (cvq_special "tppf", the VaR path's stdtrit) returns all N x dim quantiles
of a candidate nu; Gaussian uses the device ``ndtri`` the same way.  The densities
and the log-sums follow the reference's formulas (copula_var.copulas).  The
optimiser control flow (L-BFGS-B sweeps, bounds, starting points, result dicts)
is the reference's, on scipy.optimize.minimize.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
from scipy.linalg import cholesky
from scipy.optimize import minimize

from .. import _native as N
from ..copulas import (frank_log_density, gaussian_from_quantiles, gumbel_log_density, joe_log_density, plackett,
                       student_from_quantiles)


def construct_correlation_matrix(dim, corr_params):
    """student/opti.py:66-85 == gaussian/opti.py:58-77 (lower triangle, row by row)."""
    corr_matrix = np.eye(dim)
    idx = 0
    for i in range(dim):
        for j in range(i):
            corr_matrix[i, j] = corr_params[idx]
            corr_matrix[j, i] = corr_params[idx]
            idx += 1
    return corr_matrix


def _invalid(corr_matrix) -> bool:
    """1e10 guard of student/opti.py:44-52, gaussian/opti.py:37-45."""
    if np.isnan(corr_matrix).any() or np.isinf(corr_matrix).any():
        return True
    try:
        cholesky(corr_matrix)
    except np.linalg.LinAlgError:
        return True
    return False


class _IFM:
    def __init__(self, marginals, densities, tol, max_iter, device):
        self.marginals = np.array(marginals, dtype=np.float64)
        self.densities = np.array(densities, dtype=np.float64)
        if len(self.marginals) != len(self.densities):               # inference_for_margins.py verify_sizes
            raise ValueError("Marginals and densities must have the same length.")
        self.N = self.marginals.shape[0]
        self.dim = self.marginals.shape[1]
        self.tol = tol
        self.max_iter = max_iter
        self.device = device
        self._log_dens = np.sum(np.sum(np.log(self.densities)))
        self.launches = 0

    def construct_correlation_matrix(self, corr_params):
        return construct_correlation_matrix(self.dim, corr_params)


class StudentCopulaOptimizer(_IFM):
    """student/opti.py:Optimizer (same constructor, objective and two-stage optimize)
    with the quantiles of each candidate nu from one device launch.

    tppf(u, nu) -> Student-t quantiles of u (any shape); default the device kernel.
    Tests pass scipy's t.ppf to replay the reference on the CPU.
    """

    def __init__(self, marginals, densities, nu_values=np.linspace(2.1, 30, 10), tol=1e-9, max_iter=5000,
                 device: int = 0, tppf: Optional[Callable] = None, verbose: bool = False):
        super().__init__(marginals, densities, tol, max_iter, device)
        self.nu_values = nu_values
        self.verbose = verbose
        self._tppf = tppf or (lambda u, nu: N.special("tppf", u, nu=nu, device=self.device))

    def negative_log_likelihood(self, params):
        """student/opti.py:34-64 -> inference_for_margins.py:38-55."""
        params = np.asarray(params, dtype=np.float64).ravel()
        nu = float(params[0])
        corr_matrix = self.construct_correlation_matrix(params[1:])
        if _invalid(corr_matrix):
            return 1e10
        z = np.asarray(self._tppf(self.marginals, nu), dtype=np.float64)   # student.py:96-102, one launch
        self.launches += 1
        with np.errstate(divide="ignore", invalid="ignore"):
            total = self._log_dens + np.sum(np.log(student_from_quantiles(z, nu, corr_matrix)))
        return -total

    def optimize(self, initial_corr=None, method="L-BFGS-B"):
        """student/opti.py:87-184: correlations by `method` for each nu in nu_values
        (bounds (-0.99, 0.99)), then nu from 10 (bounds (2.01, 50)) with the best ones."""
        best_nll, best_corr_params = np.inf, None
        n_corr = (self.dim * (self.dim - 1)) // 2
        if initial_corr is None:
            initial_corr = np.full(n_corr, 0.5)
        corr_bounds = [(-0.99, 0.99)] * n_corr
        nu_bounds = [(2.01, 50)]
        for nu in self.nu_values:
            res_corr = minimize(fun=lambda c: self.negative_log_likelihood(np.hstack(([nu], c))), x0=initial_corr,
                                method=method, bounds=corr_bounds, tol=self.tol, options={"maxiter": self.max_iter})
            nll_corr = self.negative_log_likelihood(np.hstack(([nu], res_corr.x)))
            if self.verbose:
                print(f"Negative Log-Likelihood for nu={nu}: {nll_corr}")
            if nll_corr < best_nll:
                best_nll, best_corr_params = nll_corr, res_corr.x
        if best_corr_params is None:
            # the reference goes on with None and fails in np.hstack / construct_correlation_matrix
            raise ValueError("Student copula fit: the negative log-likelihood is NaN for every nu "
                             "(a marginal at exactly 0 or 1 has an infinite t quantile, student.py:133-172)")
        res_nu = minimize(fun=lambda v: self.negative_log_likelihood(np.hstack((v, best_corr_params))), x0=[10],
                          method=method, bounds=nu_bounds, tol=self.tol, options={"maxiter": self.max_iter})
        optimized_nu = np.array([res_nu.x[0]])
        final_nll = self.negative_log_likelihood(np.hstack((optimized_nu, best_corr_params)))
        return {"nu": optimized_nu, "corr_matrix": self.construct_correlation_matrix(best_corr_params),
                "nll": final_nll, "optimized_params": np.hstack((optimized_nu, best_corr_params))}


Optimizer = StudentCopulaOptimizer          # the reference's class name (copulas/student/opti.py:8)


class GaussianCopulaOptimizer(_IFM):
    """gaussian/opti.py:GaussianCopulaOptimizer; the norm.ppf quantiles (gaussian.py:43-44)
    are computed once on the device -- they do not depend on the correlations."""

    def __init__(self, marginals, densities, tol=1e-9, max_iter=5000, device: int = 0,
                 ndtri: Optional[Callable] = None):
        super().__init__(marginals, densities, tol, max_iter, device)
        self._ndtri = ndtri or (lambda u: N.special("ndtri", u, device=self.device))
        self._z = None

    def negative_log_likelihood(self, corr_params):
        """gaussian/opti.py:30-56 -> inference_for_margins.py:34-53 (copula pdf floored at 1e-10)."""
        corr_matrix = self.construct_correlation_matrix(np.asarray(corr_params, dtype=np.float64).ravel())
        if _invalid(corr_matrix):
            return 1e10
        if self._z is None:
            self._z = np.asarray(self._ndtri(self.marginals), dtype=np.float64)
            self.launches += 1
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            copula_pdf = np.maximum(gaussian_from_quantiles(self._z, corr_matrix), 1e-10)
            total = self._log_dens + np.sum(np.log(copula_pdf))
        return -total

    def optimize(self, initial_corr=None, method="L-BFGS-B"):
        """gaussian/opti.py:79-128."""
        n_corr = (self.dim * (self.dim - 1)) // 2
        if initial_corr is None:
            initial_corr = np.full(n_corr, 0.5)
        res_corr = minimize(fun=self.negative_log_likelihood, x0=initial_corr, method=method,
                            bounds=[(-0.99, 0.99)] * n_corr, tol=self.tol, options={"maxiter": self.max_iter})
        optimized_corr_params = res_corr.x
        final_nll = self.negative_log_likelihood(optimized_corr_params)
        return {"corr_matrix": self.construct_correlation_matrix(optimized_corr_params), "nll": final_nll,
                "optimized_params": optimized_corr_params}


class PlackettCopulaOptimizer(_IFM):
    """plackett/opti.py:PlackettCopulaOptimizer (closed-form density, Q11 formula; no
    quantile transform, so nothing to put on the device)."""

    def __init__(self, marginals, densities, tol=1e-9, max_iter=5000):
        super().__init__(marginals, densities, tol, max_iter, device=0)
        if self.dim != 2:                                              # plackett inference_for_margins.py:29-30
            raise ValueError("Plackett copula is only defined for 2-dimensional marginals.")
        self._log_dens = np.sum(np.log(self.densities))

    def negative_log_likelihood(self, theta):
        """plackett/opti.py:28-42 -> inference_for_margins.py:32-49."""
        with np.errstate(divide="ignore", invalid="ignore"):
            total = self._log_dens + np.sum(np.log(plackett(self.marginals, theta)))
        return -total

    def optimize(self, theta_range=None, method="L-BFGS-B"):
        """plackett/opti.py:44-97: one L-BFGS-B run per starting theta (bounds (0.1, None))."""
        if theta_range is None:
            theta_range = np.linspace(0.5, 50, 10)
        best_nll, best_theta = np.inf, None
        for initial_theta in theta_range:
            res = minimize(fun=self.negative_log_likelihood, x0=[initial_theta], method=method,
                           bounds=[(0.1, None)], tol=self.tol, options={"maxiter": self.max_iter})
            if res.fun < best_nll:
                best_nll, best_theta = res.fun, res.x[0]
        return {"theta": best_theta, "nll": best_nll, "optimized_params": best_theta}


class GumbelCopulaOptimizer(_IFM):
    """IFM fit of the Gumbel (survival=True: survival Gumbel) copula parameter theta by its
    closed-form log-density (copulas.gumbel_log_density), as PlackettCopulaOptimizer: there is
    no quantile transform, so nothing to put on the device.  dim 2 or 3.

    A marginal model's CDF saturates in double precision: an in-sample residual far in a tail
    comes back as exactly 0 or 1 (a poorly fitted GARCH does this on a handful of days), where
    the Gumbel density is 0 or infinite and the likelihood undefined.  Such a value stands for
    one within a rounding step of the boundary, so the marginals are clamped to
    [EDGE, 1 - EDGE], EDGE = 2^-53 (1 - 2^-53 is the largest double below 1; the same step at
    both ends keeps the fit symmetric under the rotation u -> 1 - u).  Such a row is kept, not
    dropped, and it weighs heavily: at u = 2^-53 the Gumbel x = -log u is 36.7 (survival, at
    1 - 2^-53, likewise), entering the likelihood as x^theta, so one saturated observation pulls
    theta towards independence unless its partner is extreme too.  That is the honest reading of
    an observation the marginal model calls all but impossible; a caller who prefers to discard
    such rows filters them before constructing the optimiser.  A NaN marginal or a density <= 0
    still fails the fit."""

    BOUNDS = (1.0001, 16.0)            # theta = 1 is independence; the device plan takes theta <= 16
    EDGE = 2.0 ** -53

    def __init__(self, marginals, densities, survival=False, tol=1e-9, max_iter=5000):
        super().__init__(marginals, densities, tol, max_iter, device=0)
        if self.dim not in (2, 3):
            raise ValueError("the Gumbel copula is implemented for 2 or 3 marginals")
        self.survival = bool(survival)
        self._u = np.clip(self.marginals, self.EDGE, 1.0 - self.EDGE)      # NaN stays NaN

    def negative_log_likelihood(self, theta):
        th = float(np.asarray(theta, dtype=np.float64).reshape(-1)[0])
        total = self._log_dens + np.sum(gumbel_log_density(self._u, th, self.survival))
        return -total if np.isfinite(total) else 1e10

    def optimize(self, theta_range=None, method="L-BFGS-B"):
        """One L-BFGS-B run per starting theta inside BOUNDS; the best NLL wins."""
        if theta_range is None:
            theta_range = (1.2, 2.0, 4.0, 9.0)
        best_nll, best_theta = np.inf, None
        for initial_theta in theta_range:
            res = minimize(fun=self.negative_log_likelihood, x0=[float(initial_theta)], method=method,
                           bounds=[self.BOUNDS], tol=self.tol, options={"maxiter": self.max_iter})
            nll = self.negative_log_likelihood(res.x)
            if nll < best_nll:
                best_nll, best_theta = nll, float(res.x[0])
        if best_theta is None or best_nll >= 1e10:
            raise ValueError("Gumbel copula fit: the negative log-likelihood is not finite at any start "
                             "(a NaN marginal, or a marginal density that is not positive)")
        return {"theta": best_theta, "nll": best_nll, "optimized_params": best_theta}


class _OneParameterIFM(_IFM):
    """IFM fit of a one-parameter copula by its closed-form log-density and a bounded 1-D search, as
    GumbelCopulaOptimizer (whose note on saturated marginals applies unchanged: they are clamped
    to [EDGE, 1 - EDGE], EDGE = 2^-53, and the row is kept)."""

    NAME = ""
    BOUNDS = (0.0, 1.0)
    STARTS = ()
    EDGE = 2.0 ** -53

    def __init__(self, marginals, densities, tol=1e-9, max_iter=5000):
        super().__init__(marginals, densities, tol, max_iter, device=0)
        if self.dim not in (2, 3):
            raise ValueError(f"the {self.NAME} copula is implemented for 2 or 3 marginals")
        self._u = np.clip(self.marginals, self.EDGE, 1.0 - self.EDGE)      # NaN stays NaN

    def _log_density(self, th):
        raise NotImplementedError

    def negative_log_likelihood(self, theta):
        th = float(np.asarray(theta, dtype=np.float64).reshape(-1)[0])
        total = self._log_dens + np.sum(self._log_density(th))
        return -total if np.isfinite(total) else 1e10

    def optimize(self, theta_range=None, method="L-BFGS-B"):
        """One L-BFGS-B run per starting theta inside BOUNDS; the best NLL wins."""
        if theta_range is None:
            theta_range = self.STARTS
        best_nll, best_theta = np.inf, None
        for initial_theta in theta_range:
            x0 = min(max(float(initial_theta), self.BOUNDS[0]), self.BOUNDS[1])
            res = minimize(fun=self.negative_log_likelihood, x0=[x0], method=method,
                           bounds=[self.BOUNDS], tol=self.tol, options={"maxiter": self.max_iter})
            nll = self.negative_log_likelihood(res.x)
            if nll < best_nll:
                best_nll, best_theta = nll, float(res.x[0])
        if best_theta is None or best_nll >= 1e10:
            raise ValueError(f"{self.NAME} copula fit: the negative log-likelihood is not finite at any start "
                             "(a NaN marginal, or a marginal density that is not positive)")
        return {"theta": best_theta, "nll": best_nll, "optimized_params": best_theta}


class FrankCopulaOptimizer(_OneParameterIFM):
    """IFM fit of the Frank copula's theta (copulas.frank_log_density); dim 2 or 3."""

    NAME = "Frank"
    BOUNDS = (1e-3, 32.0)              # theta -> 0 is independence; the device plan takes theta <= 32
    STARTS = (0.5, 2.0, 6.0, 15.0)

    def _log_density(self, th):
        return frank_log_density(self._u, th)


class JoeCopulaOptimizer(_OneParameterIFM):
    """IFM fit of the Joe (survival=True: survival Joe) copula's theta (copulas.joe_log_density);
    dim 2 or 3."""

    NAME = "Joe"
    BOUNDS = (1.0001, 16.0)            # theta = 1 is independence; the device plan takes theta <= 16
    STARTS = (1.2, 2.0, 4.0, 9.0)

    def __init__(self, marginals, densities, survival=False, tol=1e-9, max_iter=5000):
        super().__init__(marginals, densities, tol, max_iter)
        self.survival = bool(survival)

    def _log_density(self, th):
        return joe_log_density(self._u, th, self.survival)


# ---------------------------------------------------------------------- score-driven copula
GAS_FAMILY = {"gaussian": "gaussian", "student": "student", "plackett": "plackett", "gumbel": "gumbel",
              "gumbel_survival": "gumbel", "frank": "frank", "joe": "joe", "joe_survival": "joe"}
GAS_RANGE = {"gaussian": (-0.99, 0.99), "student": (-0.99, 0.99), "plackett": (0.1, 1000.0),
             "gumbel": (1.0001, 16.0), "joe": (1.0001, 16.0), "frank": (1e-3, 32.0)}


def gas_link(copula, f):
    """The bounded sigmoid link of cvq_gas_loglik / cvq_gas_path (include/cvq.h), float64."""
    fam = GAS_FAMILY[copula]
    sg = 1.0 / (1.0 + np.exp(-np.asarray(f, dtype=np.float64)))
    if fam in ("gaussian", "student"):
        return 0.99 * (2.0 * sg - 1.0)
    if fam == "plackett":
        return 0.1 * 10.0 ** (4.0 * sg)
    lo, hi = GAS_RANGE[fam]
    return lo + (hi - lo) * sg


def gas_link_inverse(copula, theta):
    """f with gas_link(copula, f) = theta; theta is first moved inside the link's open range."""
    fam = GAS_FAMILY[copula]
    lo, hi = GAS_RANGE[fam]
    th = float(theta)
    if fam in ("gaussian", "student"):
        sg = (th / 0.99 + 1.0) / 2.0
    elif fam == "plackett":
        sg = np.log10(max(th, lo) / 0.1) / 4.0
    else:
        sg = (th - lo) / (hi - lo)
    sg = min(max(float(sg), 1e-9), 1.0 - 1e-9)
    return float(np.log(sg) - np.log1p(-sg))


class GasCopulaOptimizer(_IFM):
    """Fit of the score-driven copula recursion (DESIGN.md §4 "Score-driven copula"; cvq_gas_loglik):
    the three parameters (omega, alpha, beta) of
        f_{t+1} = clamp(omega + beta f_t + alpha s_t, -40, 40),   theta_t = link(f_t),
    by maximum likelihood on the in-sample marginals, every likelihood on the device and every
    optimiser step one launch.

    copula: a name of _native.COPULA_KIND; nu: the Student degrees of freedom (fixed: the plan's).
    static_theta: the static fit's parameter (rho or theta); None runs the existing static optimiser
    (copula_var.dynamic.fit_copula).  loglik(rows (B, 3)) -> LL (B,): default the device kernel; tests
    pass a CPU restatement, as GarchOptimizer allows.  The marginals are clamped to
    [2^-53, 1 - 2^-53], as the Archimedean optimisers do (GumbelCopulaOptimizer's note).

    optimize(): the 4 x 4 grid beta in BETAS, alpha in ALPHAS, omega = f_bar (1 - beta) with
    f_bar = link^-1(static theta) in ONE launch; the best N_REFINE starts refined by L-BFGS-B
    (alpha in [0, 4], beta in [0, 0.999], omega free) whose objective and central-difference gradient
    come from one 7-row launch per step.  Rows with |beta| >= 1, non-finite rows and NaN
    likelihoods score 1e10; the first two kinds are never launched.  The grid holds alpha = 0,
    beta = 0 -- the static model -- so nll <= static_nll."""

    EDGE = 2.0 ** -53
    BETAS = (0.0, 0.5, 0.9, 0.97)
    ALPHAS = (0.0, 0.02, 0.1, 0.4)
    BOUNDS = ((None, None), (0.0, 4.0), (0.0, 0.999))
    N_REFINE = 3
    STEP = 1e-5

    def __init__(self, marginals, densities, copula, nu=None, static_theta=None, device: int = 0,
                 loglik: Optional[Callable] = None, tol=1e-9, max_iter=200):
        super().__init__(marginals, densities, tol, max_iter, device)
        if copula not in GAS_FAMILY:
            raise ValueError(f"copula must be one of {sorted(GAS_FAMILY)}")
        fam = GAS_FAMILY[copula]
        if self.dim not in (2, 3) or (self.dim == 3 and fam in ("gaussian", "student", "plackett")):
            raise ValueError(f"the score-driven {copula} copula is not built for {self.dim} marginals")
        if fam == "student" and nu is None:
            raise ValueError("the score-driven Student copula needs nu (it stays fixed)")
        self.copula, self.nu = copula, None if nu is None else float(nu)
        self._u = np.clip(self.marginals, self.EDGE, 1.0 - self.EDGE)      # NaN stays NaN
        self.static_theta = static_theta
        self._loglik = loglik or self._device_loglik
        self.evaluations = 0

    def _device_loglik(self, rows):
        from .. import engine
        return engine.gas_loglik(self._u, self.copula, rows, nu=self.nu, device=self.device)

    def negative_log_likelihoods(self, rows) -> np.ndarray:
        """rows (B, 3) -> NLL (B,), the sum of the log marginal densities included; one launch for
        the rows that can be launched, 1e10 for the others and for NaN likelihoods."""
        rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
        out = np.full(rows.shape[0], 1e10)
        good = np.all(np.isfinite(rows), axis=1) & (np.abs(rows[:, 2]) < 1.0)
        if np.any(good):
            ll = np.asarray(self._loglik(np.ascontiguousarray(rows[good])), dtype=np.float64)
            self.launches += 1
            self.evaluations += int(np.sum(good))
            nll = -(self._log_dens + ll)
            out[good] = np.where(np.isfinite(nll), nll, 1e10)
        return out

    def _static_theta(self):
        if self.static_theta is not None:
            return float(np.asarray(self.static_theta, dtype=np.float64).reshape(-1)[-1])
        from ..dynamic import fit_copula
        got, _ = fit_copula(self.copula, self._u, self.densities, nu=self.nu, device=self.device)
        return float(np.asarray(got).reshape(-1)[-1])

    def _value_and_gradient(self, x):
        x = np.asarray(x, dtype=np.float64)
        h = self.STEP * (1.0 + np.abs(x))
        rows = np.tile(x, (7, 1))
        for i in range(3):
            rows[1 + 2 * i, i] += h[i]
            rows[2 + 2 * i, i] -= h[i]
        v = self.negative_log_likelihoods(rows)
        # the spacing actually taken (x + h - (x - h) in floating point)
        g = np.array([(v[1 + 2 * i] - v[2 + 2 * i]) / (rows[1 + 2 * i, i] - rows[2 + 2 * i, i]) for i in range(3)])
        if not np.all(v < 1e10):
            g = np.zeros(3)
        return float(v[0]), g

    def optimize(self):
        fbar = gas_link_inverse(self.copula, self._static_theta())
        grid = np.array([[fbar * (1.0 - b), a, b] for b in self.BETAS for a in self.ALPHAS])
        nll = self.negative_log_likelihoods(grid)                           # one launch
        static_nll = float(nll[0])                                          # beta = 0, alpha = 0
        if not np.any(nll < 1e10):
            raise ValueError("score-driven copula fit: the likelihood is not finite at any grid start "
                             "(a NaN marginal, or a marginal density that is not positive)")
        best_x, best_nll = grid[int(np.argmin(nll))].copy(), float(np.min(nll))
        for j in np.argsort(nll, kind="stable")[:self.N_REFINE]:
            if not nll[j] < 1e10:
                continue
            res = minimize(self._value_and_gradient, grid[j], jac=True, method="L-BFGS-B", bounds=list(self.BOUNDS),
                           tol=self.tol, options={"maxiter": self.max_iter})
            val = float(self.negative_log_likelihoods(res.x[None, :])[0])
            if val < best_nll:
                best_x, best_nll = np.asarray(res.x, dtype=np.float64).copy(), val
        return {"omega": float(best_x[0]), "alpha": float(best_x[1]), "beta": float(best_x[2]), "nll": best_nll,
                "static_nll": static_nll, "static_theta": float(gas_link(self.copula, fbar)), "f_bar": fbar,
                "launches": self.launches, "evaluations": self.evaluations,
                "optimized_params": best_x}
