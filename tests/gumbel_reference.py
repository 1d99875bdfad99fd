"""Checker for the Gumbel and survival-Gumbel copulas: the definition the device is held to.

There is no reference implementation of these kinds.  GumbelProblem is oracle.quadrature.Problem
with only mass(t) overridden; axis_cdf, delta_weights (Q5 / Q6), inner_mask (Q9 / Q10),
compute_integral and oracle.quadrature.calc_var (Q1-Q4) are inherited unchanged, and the object
works where tests/es_reference.py and tests/quantile_reference.py take a Problem.

Per axis i, u_i the marginal CDF table (axis_cdf, erf form), theta >= 1, d = dim:
  l_i = log u_i            (Gumbel)
  l_i = log1p(-u_i)        (survival Gumbel: the rotated margin 1 - u_i)
  x_i = -l_i
Per node:
  log S = logaddexp_i(theta log x_i),  log A = log S / theta,  A = exp(log A)
  log c = -A - sum l_i + (theta - 1) sum log x_i + (1 - d theta) log A + log poly_d(A)
  poly_2(A) = A + (theta - 1),  poly_3(A) = A^2 + 3 (theta - 1) A + (theta - 1)(2 theta - 1)
  GARCH / UKF: mass = exp(log c + sum log pdf_i) W;  MSM: mass = exp(log c) W;  W = delta_weights(t)
Dead-entry rule (both models): a node contributes exactly 0 if any u_i is not strictly inside
(0, 1), is NaN, or if the value is not finite; the mass is never NaN and never +-inf.
"""
import numpy as np

from oracle.quadrature import Problem

KINDS = ("gumbel", "gumbel_survival")


def log_density(u, theta, survival=False):
    """log c(u) for u of shape (..., d), d = 2 or 3; NaN where a u_i is not strictly inside (0, 1)."""
    u = np.asarray(u, dtype=np.float64)
    d = u.shape[-1]
    th = float(theta)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ell = np.log1p(-u) if survival else np.log(u)
        x = -ell
        lx = np.log(x)
        logS = np.logaddexp.reduce(th * lx, axis=-1)
        logA = logS / th
        A = np.exp(logA)
        if d == 2:
            poly = A + (th - 1)
        else:
            poly = A * A + 3 * (th - 1) * A + (th - 1) * (2 * th - 1)
        lc = -A - np.sum(ell, axis=-1) + (th - 1) * np.sum(lx, axis=-1) + (1 - d * th) * logA + np.log(poly)
    live = np.all((u > 0.0) & (u < 1.0), axis=-1)
    return np.where(live, lc, np.nan)


def density(u, theta, survival=False):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(log_density(u, theta, survival))


def cdf(u, theta):
    """C(u) = exp(-(sum_i (-log u_i)^theta)^(1/theta)) (the Gumbel copula itself, for the self-test)."""
    u = np.asarray(u, dtype=np.float64)
    return np.exp(-np.sum((-np.log(u)) ** float(theta), axis=-1) ** (1.0 / float(theta)))


class GumbelProblem(Problem):
    """Problem(model, "gumbel" | "gumbel_survival", ..., copula_params=[theta], ...)."""

    @property
    def theta(self):
        return float(np.asarray(self.copula_params, dtype=np.float64).reshape(-1)[0])

    @property
    def survival(self):
        return self.copula == "gumbel_survival"

    def mass(self, t):
        if t in self._mass:
            return self._mass[t]
        assert self.copula in KINDS, self.copula
        u, pdf = self.axis_cdf(t)
        U = np.stack(np.broadcast_arrays(*self._broadcast(u)), axis=-1)          # (n,) * dim + (dim,)
        logv = log_density(U, self.theta, self.survival)
        if self.model != "msm":
            with np.errstate(divide="ignore"):
                lp = np.log(pdf)
            for c, L in enumerate(self._broadcast(lp)):
                logv = logv + L
        with np.errstate(over="ignore", invalid="ignore"):
            m = np.exp(logv) * self.delta_weights(t)
        m = np.where(np.isfinite(m), m, 0.0)                                     # dead rule
        self._mass[t] = m
        return m

    def dead_entries(self, t):
        """Table entries (axis, index) whose u is not strictly inside (0, 1)."""
        u, _ = self.axis_cdf(t)
        return ~((u > 0.0) & (u < 1.0))


def problem_of(z, kind, theta, sl=slice(None)):
    """GumbelProblem on a golden case's arrays (its copula swapped), optionally a slice of its dates."""
    model = str(z["model"])
    per = (z["forecasts_by_states"][sl], z["forecasts"][sl]) if model == "msm" else z["sigma_forecasts"][sl]
    return GumbelProblem(model, kind, int(z["dim"]), z["x_values"], z["step"], z["densities"], z["combos"],
                         z["weights"], np.array([float(theta)]), per, z.get("unique_vol_states"))


def scaled(compute_integral, factor):
    """compute_integral with every value scaled: the decision-margin probe of the exact-VaR premise."""
    return lambda bounds: compute_integral(bounds) * factor


def corner_problem(kind, theta=16.0, n=32, T=2):
    """A consistent 2-D MSM problem whose lower grid edge has 0 < u_i < 1e-19 on both axes.  The erf
    form of the normal CDF is 0 or at least 2^-54 = 5.6e-17, so a mixture CDF gets that small only
    through a small state probability: vol states (0.3, 0.6), the wide state forecast with
    probability ~1e-6, give u < 1e-20 at the two lowest grid points of each axis.  Under the survival kind
    x_i = -log1p(-u_i) = u_i there and x_i^16 < 1e-300, below the device tables' floor
    (kGumbelFloor)."""
    from oracle import forecast as F
    x, step = F.x_grid(n, "msm")
    uvs = np.array([[0.3, 0.6], [0.3, 0.6]])
    dens = F.msm_densities(uvs, x)
    combos = np.array([[a, b] for a in range(2) for b in range(2)])
    rng = np.random.default_rng(16)
    f1 = rng.uniform(0.5e-6, 2e-6, size=(T, 2, 1))                                 # the wide state
    fbs = np.concatenate([1.0 - f1, f1], axis=2)                                   # (T, dim, q)
    pi = (fbs[:, 0, :, None] * fbs[:, 1, None, :]).reshape(T, 4)
    return GumbelProblem("msm", kind, 2, x, step, dens, combos, np.array([0.5, 0.5]), np.array([float(theta)]),
                         (fbs, pi), uvs)
