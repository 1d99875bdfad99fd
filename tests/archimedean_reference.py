"""Checker for the Frank, Joe and survival-Joe copulas: the definition the device is held to.

There is no reference implementation of these kinds.  ArchimedeanProblem is
oracle.quadrature.Problem with only mass(t) overridden, as tests/gumbel_reference.GumbelProblem:
axis_cdf, delta_weights (Q5 / Q6), inner_mask (Q9 / Q10), compute_integral and
oracle.quadrature.calc_var (Q1-Q4) are inherited unchanged, and the object works wherever
es_reference, quantile_reference, attribution_reference, conditional_reference,
portfolio_reference and dynamic_reference take a Problem.

All arithmetic between the float64 marginal CDF tables and the float64 node masses is longdouble,
in the stable "product form".  log1mexp(x) = log(1 - e^-x), x > 0: log1p(-exp(-x)) above log 2,
log(-expm1(-x)) below.  Per axis entry (u the marginal CDF value):
  Frank (theta > 0), g = -expm1(-theta), X = e^-theta expm1(theta (1 - u)) / g:
      a = -log1p(-X) if X <= 1/2 else log1mexp(theta) - log1mexp(theta u)
      B = log theta - theta u + a - log1mexp(theta) [+ log pdf]
  Joe (theta >= 1), l = log1p(-u); survival Joe l = log u:
      a = -log1mexp(-theta l)
      B = log theta + (theta - 1) l + a [+ log pdf]
Per node, d = dim, S = sum a_i:
  E = expm1(-S), om = q0 - p0 E, y = p0 (1 + E) / om
  log(c prod pdf) = sum B_i + log p0 - log theta - S + (kappa - 1) log om + log(1 + y (c2 + c3 y))
  Frank: p0 = g, q0 = e^-theta, kappa = 0, (c2, c3) = (1, 0) | (3, 2)
  Joe:   p0 = 1, q0 = 0, kappa = 1 / theta, k = 1 - 1 / theta, (c2, c3) = (k, 0) | (3 k, k (1 + k))
Dead rule (both models): a node contributes exactly 0 if any u_i is NaN or not strictly inside
(0, 1), or if the value is not finite.
"""
import numpy as np

from oracle.quadrature import Problem

KINDS = ("frank", "joe", "joe_survival")
LD = np.longdouble
LOG2 = np.log(LD(2))


def log1mexp(x):
    x = np.asarray(x, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(x > LOG2, np.log1p(-np.exp(-x)), np.log(-np.expm1(-x)))


def constants(kind, theta, d):
    """(p0, q0, kappa, c2, c3, log p0 - log theta) in longdouble."""
    th = LD(theta)
    if kind == "frank":
        c2, c3 = (LD(1), LD(0)) if d == 2 else (LD(3), LD(2))
        return -np.expm1(-th), np.exp(-th), LD(0), c2, c3, log1mexp(th) - np.log(th)
    k = 1 - 1 / th
    c2, c3 = (k, LD(0)) if d == 2 else (3 * k, k * (1 + k))
    return LD(1), LD(0), 1 / th, c2, c3, -np.log(th)


def axis_terms(kind, theta, u):
    """(a, B without the pdf term) per entry of u, longdouble; meaningless where u is dead."""
    th = LD(theta)
    u = np.asarray(u, dtype=np.float64).astype(LD)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind == "frank":
            g = -np.expm1(-th)
            X = np.exp(-th) * np.expm1(th * (1 - u)) / g
            a = np.where(X <= LD(0.5), -np.log1p(-X), log1mexp(th) - log1mexp(th * u))
            B = np.log(th) - th * u + a - log1mexp(th)
        else:
            ell = np.log(u) if kind == "joe_survival" else np.log1p(-u)
            a = -log1mexp(-th * ell)
            B = np.log(th) + (th - 1) * ell + a
    return a, B


def node_log(kind, theta, d, S, sumB):
    """log(c prod pdf) from S = sum a_i and sum B_i (longdouble arrays)."""
    p0, q0, kappa, c2, c3, lc = constants(kind, theta, d)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        E = np.expm1(-S)
        om = q0 - p0 * E
        y = p0 * (1 + E) / om
        return sumB + lc - S + (kappa - 1) * np.log(om) + np.log(1 + y * (c2 + c3 * y))


def log_density(u, kind, theta):
    """log c(u), longdouble, for u of shape (..., d), d = 2 or 3; NaN where a u_i is dead."""
    u = np.asarray(u, dtype=np.float64)
    d = u.shape[-1]
    a, B = axis_terms(kind, theta, u)
    lc = node_log(kind, theta, d, np.sum(a, axis=-1), np.sum(B, axis=-1))
    live = np.all((u > 0.0) & (u < 1.0), axis=-1)
    return np.where(live, lc, LD("nan"))


class ArchimedeanProblem(Problem):
    """Problem(model, "frank" | "joe" | "joe_survival", ..., copula_params=[theta], ...)."""

    def __init__(self, model, copula, dim, x_values, step, densities, combos, weights, copula_params, per_date,
                 unique_vol_states=None):
        assert copula in KINDS, copula
        # the base class unpacks a correlation matrix from the parameters of a kind it does not
        # know; one parameter reads as Plackett's theta
        super().__init__(model, "plackett", dim, x_values, step, densities, combos, weights, copula_params,
                         per_date, unique_vol_states)
        self.copula = copula

    @property
    def theta(self):
        return float(np.asarray(self.copula_params, dtype=np.float64).reshape(-1)[0])

    def mass(self, t):
        if t in self._mass:
            return self._mass[t]
        u, pdf = self.axis_cdf(t)
        a, B = axis_terms(self.copula, self.theta, u)
        if self.model != "msm":
            with np.errstate(divide="ignore"):
                B = B + np.log(pdf.astype(LD))
        S, sumB = 0, 0
        with np.errstate(invalid="ignore"):                                      # dead entries: inf - inf
            for c in range(self.dim):
                S = S + self._broadcast(a)[c]
                sumB = sumB + self._broadcast(B)[c]
        logv = node_log(self.copula, self.theta, self.dim, S, sumB)
        live = (u > 0.0) & (u < 1.0)
        ok = True
        for L in self._broadcast(live):
            ok = ok & L
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            m = (np.exp(logv) * self.delta_weights(t).astype(LD)).astype(np.float64)
        m = np.where(ok & np.isfinite(m), m, 0.0)                                # dead rule
        self._mass[t] = m
        return m

    def dead_entries(self, t):
        u, _ = self.axis_cdf(t)
        return ~((u > 0.0) & (u < 1.0))


def problem_of(z, kind, theta, sl=slice(None)):
    """ArchimedeanProblem on a golden case's arrays (its copula swapped), optionally a slice of its dates."""
    model = str(z["model"])
    per = (z["forecasts_by_states"][sl], z["forecasts"][sl]) if model == "msm" else z["sigma_forecasts"][sl]
    return ArchimedeanProblem(model, kind, int(z["dim"]), z["x_values"], z["step"], z["densities"], z["combos"],
                              z["weights"], np.array([float(theta)]), per, z.get("unique_vol_states"))


def scaled(compute_integral, factor):
    """compute_integral with every value scaled: the decision-margin probe of the exact-VaR premise."""
    return lambda bounds: compute_integral(bounds) * factor


# Table 1: (golden case, kind, theta)
TABLE1 = (
    ("cfg2_n64", "frank", 6.0), ("cfg2_n64", "joe_survival", 2.0), ("cfg2_n64", "joe", 3.0),
    ("garch_student_n64", "frank", 12.0), ("garch_student_n64", "joe_survival", 2.2),
    ("cfg5_n64", "frank", 32.0), ("cfg5_n64", "frank", 0.25), ("cfg5_n64", "joe", 16.0),
    ("cfg5_n64", "joe_survival", 16.0), ("cfg5_n64", "joe_survival", 1.3),
    ("cfg4_k4_n16", "frank", 5.0), ("cfg4_k4_n16", "joe_survival", 1.8),
    ("garch3d_student_n16", "joe", 2.5), ("garch3d_student_n16", "joe_survival", 16.0),
    ("garch3d_student_n16", "frank", 32.0),
    ("q1_lowvol", "joe_survival", 8.0),
    ("cfg1", "frank", 4.0),
    ("ukf_plackett_n64", "joe_survival", 6.0),
)


def corner_problem(kind, theta, n=32, T=2):
    """tests/gumbel_reference.corner_problem's inputs under one of these kinds: a consistent 2-D MSM
    problem whose lower grid edge has 0 < u_i < 1e-19 on both axes.  Under survival Joe at theta = 16
    a = -log1mexp(-theta log u) ~ u^theta < 1e-300 there, below the device tables' floor."""
    from gumbel_reference import corner_problem as gumbel_corner
    g = gumbel_corner("gumbel_survival", theta=2.0, n=n, T=T)
    return ArchimedeanProblem("msm", kind, 2, g.x, g.step, g.dens, g.combos, g.w, np.array([float(theta)]),
                              (g.fbs, g.pi), g.uvs)
