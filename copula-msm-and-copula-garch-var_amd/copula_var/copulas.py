"""Pointwise copula densities c(u) for the adapters' ``copula_density`` API.

The VaR path never calls these: the device quadrature evaluates the copula
inside its kernels.  They exist so code written against the reference's
adapters (``StudentCopulaVaR.copula_density(cdf=, nu=, corr_matrix=)`` etc.)
keeps working.  The quantile transforms (t.ppf / norm.ppf, the expensive part,
student.py:100-102, gaussian.py:43-44) run on the GPU through cvq_special; the
closed-form density around them is a few numpy array expressions.

Semantics follow the reference, including its edge behaviour: Student density
0 when a quantile is non-finite, so c = 0/0 = NaN at u in {0, 1}
(student.py:133-141, 164-172); Gaussian has no guard (gaussian.py:105-113);
Plackett uses the reference's non-standard formula (Q11, plackett.py:66-69).
The Gumbel family has no reference counterpart.
"""
from __future__ import annotations

import math

import numpy as np

from . import _native as N


def student(cdf, nu, corr_matrix):
    """copulas/student/student.py:49-174."""
    u = np.asarray(cdf, dtype=np.float64)
    return student_from_quantiles(N.special("tppf", u, nu=float(nu)), nu, corr_matrix)


def student_from_quantiles(z, nu, corr_matrix):
    """student.py:66-79 after the t.ppf step: the multivariate t pdf of the
    quantiles z (P, d) over the product of the univariate t pdfs."""
    P, d = z.shape
    Ri, det = np.linalg.inv(corr_matrix), np.linalg.det(corr_matrix)
    term1 = math.gamma((nu + d) / 2) / (math.gamma(nu / 2) * ((nu * np.pi) ** (d / 2)) * np.sqrt(det))
    g = math.gamma((nu + 1) / 2) / (np.sqrt(nu * np.pi) * math.gamma(nu / 2))
    fin_row = np.all(np.isfinite(z), axis=1)
    zz = np.where(np.isfinite(z), z, 0.0)
    qf = np.einsum("pi,ij,pj->p", zz, Ri, zz)
    mv = np.where(fin_row, term1 * (1 + qf / nu) ** (-(nu + d) / 2), 0.0)
    uni = np.where(np.isfinite(z), g * (1 + zz ** 2 / nu) ** (-(nu + 1) / 2), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return mv / np.prod(uni, axis=1)


def gaussian(cdf, corr_matrix):
    """copulas/gaussian/gaussian.py:43-117."""
    u = np.asarray(cdf, dtype=np.float64)
    return gaussian_from_quantiles(N.special("ndtri", u), corr_matrix)


def gaussian_from_quantiles(z, corr_matrix):
    """gaussian.py:52-61 after the norm.ppf step."""
    P, d = z.shape
    Ri, det = np.linalg.inv(corr_matrix), np.linalg.det(corr_matrix)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        qf = np.einsum("pi,ij,pj->p", z, Ri, z)
        mv = (1 / np.sqrt((2 * np.pi) ** d * det)) * np.exp(-0.5 * qf)
        uni = (1 / np.sqrt(2 * np.pi)) * np.exp(-0.5 * z ** 2)
        return mv / np.prod(uni, axis=1)


def plackett(cdf, theta):
    """copulas/plackett/plackett.py:35-71 (Q11 formula, columns 0 and 1)."""
    c = np.asarray(cdf, dtype=np.float64)
    u, v = c[:, 0], c[:, 1]
    th = float(np.asarray(theta).reshape(-1)[0])
    num = th * (1 + (th - 1) * (u + v - 2 * u * v))
    den = ((1 + (th - 1) * (u + v)) * (1 + (th - 1) * (1 - u - v))) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / den


def gumbel_log_density(cdf, theta, survival=False):
    """log c(u) of the exchangeable Gumbel copula C(u) = exp(-(sum_i (-log u_i)^theta)^(1/theta)),
    theta >= 1, columns = assets (2 or 3); survival: the 180-degree rotation c(1 - u).
    With x_i = -log u_i, S = sum x_i^theta, A = S^(1/theta), d = dim:
        log c = -A + sum x_i + (theta - 1) sum log x_i + (1 - d theta) log A + log poly_d(A)
        poly_2(A) = A + (theta - 1),  poly_3(A) = A^2 + 3 (theta - 1) A + (theta - 1)(2 theta - 1).
    NaN where a u_i is not strictly inside (0, 1)."""
    u = np.asarray(cdf, dtype=np.float64)
    P, d = u.shape
    if d not in (2, 3):
        raise ValueError("the Gumbel copula is implemented for 2 or 3 marginals")
    th = float(np.asarray(theta).reshape(-1)[0])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ell = np.log1p(-u) if survival else np.log(u)
        ok = np.all((u > 0.0) & (u < 1.0), axis=1)
        x = -ell
        lx = np.log(x)
        logS = np.logaddexp.reduce(th * lx, axis=1)
        logA = logS / th
        A = np.exp(logA)
        poly = A + (th - 1) if d == 2 else A * A + 3 * (th - 1) * A + (th - 1) * (2 * th - 1)
        lc = -A - np.sum(ell, axis=1) + (th - 1) * np.sum(lx, axis=1) + (1 - d * th) * logA + np.log(poly)
    return np.where(ok, lc, np.nan)


def gumbel(cdf, theta, survival=False):
    """Pointwise Gumbel (survival=True: survival Gumbel) copula density, (P, d) -> (P,)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(gumbel_log_density(cdf, theta, survival))


def _log1mexp(x):
    """log(1 - e^-x) for x > 0: log1p(-exp(-x)) above log 2, log(-expm1(-x)) below."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(x > np.log(2.0), np.log1p(-np.exp(-x)), np.log(-np.expm1(-x)))


def _product_form_log_density(a, B, p0, q0, kappa, c2, c3, lc):
    """log c of a product-form Archimedean copula from the per-margin generator values a (P, d) and
    log factors B (P, d): S = sum a, om = q0 - p0 expm1(-S) = 1 - p0 e^-S (a sum of
    two non-negative terms), p = p0 e^-S,
        log c = sum B + lc - S + (kappa - d) log om + log poly_d,
        poly_2 = om + c2 p,  poly_3 = om^2 + p (c2 om + c3 p)."""
    d = a.shape[1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        S = np.sum(a, axis=1)
        om = q0 - p0 * np.expm1(-S)
        p = p0 * np.exp(-S)
        poly = om + c2 * p if d == 2 else om * om + p * (c2 * om + c3 * p)
        return np.sum(B, axis=1) + lc - S + (kappa - d) * np.log(om) + np.log(poly)


def frank_log_density(cdf, theta):
    """log c(u) of the exchangeable Frank copula
        C(u) = -log(1 - prod_i (1 - e^(-theta u_i)) / (1 - e^-theta)^(d-1)) / theta,  theta > 0,
    columns = assets (2 or 3).  Per margin, with g = 1 - e^-theta and X = e^-theta expm1(theta (1 - u)) / g:
        a = -log((1 - e^(-theta u)) / g) = -log1p(-X)  (X <= 1/2) | log1mexp(theta) - log1mexp(theta u)
        B = log theta - theta u + a - log1mexp(theta)
    then the product form with p0 = g, q0 = e^-theta, kappa = 0, (c2, c3) = (1, 0) | (3, 2).
    NaN where a u_i is not strictly inside (0, 1)."""
    u = np.asarray(cdf, dtype=np.float64)
    P, d = u.shape
    if d not in (2, 3):
        raise ValueError("the Frank copula is implemented for 2 or 3 marginals")
    th = float(np.asarray(theta).reshape(-1)[0])
    if not th > 0.0:
        raise ValueError("the Frank copula is implemented for theta > 0")
    g, lg = -np.expm1(-th), float(_log1mexp(th))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.all((u > 0.0) & (u < 1.0), axis=1)
        X = np.exp(-th) * np.expm1(th * (1.0 - u)) / g
        a = np.where(X <= 0.5, -np.log1p(-X), lg - _log1mexp(th * u))
        B = np.log(th) - th * u + a - lg
        c2, c3 = (1.0, 0.0) if d == 2 else (3.0, 2.0)
        lc = _product_form_log_density(a, B, g, np.exp(-th), 0.0, c2, c3, lg - np.log(th))
    return np.where(ok, lc, np.nan)


def frank(cdf, theta):
    """Pointwise Frank copula density, (P, d) -> (P,)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(frank_log_density(cdf, theta))


def joe_log_density(cdf, theta, survival=False):
    """log c(u) of the exchangeable Joe copula C(u) = 1 - (1 - prod_i (1 - (1 - u_i)^theta))^(1/theta),
    theta >= 1, columns = assets (2 or 3); survival: the 180-degree rotation c(1 - u).  Per margin,
    with l = log1p(-u) (survival: log u):
        a = -log1mexp(-theta l),  B = log theta + (theta - 1) l + a
    then the product form with p0 = 1, q0 = 0, kappa = 1 / theta, k = 1 - kappa,
    (c2, c3) = (k, 0) | (3 k, k (1 + k)).  NaN where a u_i is not strictly inside (0, 1)."""
    u = np.asarray(cdf, dtype=np.float64)
    P, d = u.shape
    if d not in (2, 3):
        raise ValueError("the Joe copula is implemented for 2 or 3 marginals")
    th = float(np.asarray(theta).reshape(-1)[0])
    if not th >= 1.0:
        raise ValueError("the Joe copula is implemented for theta >= 1")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.all((u > 0.0) & (u < 1.0), axis=1)
        ell = np.log(u) if survival else np.log1p(-u)
        a = -_log1mexp(-th * ell)
        B = np.log(th) + (th - 1.0) * ell + a
        kap = 1.0 / th
        k = 1.0 - kap
        c2, c3 = (k, 0.0) if d == 2 else (3.0 * k, k * (1.0 + k))
        lc = _product_form_log_density(a, B, 1.0, 0.0, kap, c2, c3, -np.log(th))
    return np.where(ok, lc, np.nan)


def joe(cdf, theta, survival=False):
    """Pointwise Joe (survival=True: survival Joe) copula density, (P, d) -> (P,)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(joe_log_density(cdf, theta, survival))
