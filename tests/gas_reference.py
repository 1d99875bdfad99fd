"""numpy restatement of the score-driven copula recursion (csrc/cvq_gas_kernels.h),
generic over float64 / longdouble and vectorised over the candidates:

    f_0 = omega / (1 - beta),  theta_t = link(f_t),  l_t = log c(u_t; theta_t),
    s_t = (d log c / d theta)(u_t; theta_t) link'(f_t),  f_{t+1} = clamp(omega + beta f_t + alpha s_t, -40, 40).

The scores are derived by hand, family by family (the kernels differentiate by forward-mode dual
numbers, the fixture by mpmath's numerical derivative of the log density: three routes).  The
densities are those of copula_var.copulas in log form.  Quantiles: float64 takes scipy's ndtri /
stdtrit unless `z` is passed (the fixture's, for longdouble runs).
"""
import numpy as np

LD = np.longdouble
F_CLAMP = 40.0
LN10 = 2.302585092994045684017991454684364207601
ELLIPTICAL = ("gaussian", "student")
FAMILY = {"gaussian": "gaussian", "student": "student", "plackett": "plackett", "gumbel": "gumbel",
          "gumbel_survival": "gumbel", "frank": "frank", "joe": "joe", "joe_survival": "joe"}
ROTATED = ("gumbel_survival", "joe_survival")
THETA_RANGE = {"gaussian": (-0.99, 0.99), "student": (-0.99, 0.99), "plackett": (0.1, 1000.0),
               "gumbel": (1.0001, 16.0), "joe": (1.0001, 16.0), "frank": (1e-3, 32.0)}


def link(copula, f):
    """(theta, d theta / d f) of the family's bounded sigmoid link."""
    fam = FAMILY[copula]
    dt = f.dtype.type
    e = np.exp(-f)
    if fam in ELLIPTICAL:
        return dt(0.99) * (-np.expm1(-f) / (1 + e)), dt(0.99) * 2 * e / ((1 + e) * (1 + e))
    sg = 1 / (1 + e)
    dsg = e * sg * sg
    if fam == "plackett":
        th = dt(0.1) * np.exp(4 * dt(LN10) * sg)
        return th, th * (4 * dt(LN10)) * dsg
    lo, hi = THETA_RANGE[fam]
    return dt(lo) + (dt(hi) - dt(lo)) * sg, (dt(hi) - dt(lo)) * dsg


def link_inverse(copula, theta):
    """f with link(f) = theta (float64; theta strictly inside the link's range)."""
    fam = FAMILY[copula]
    lo, hi = THETA_RANGE[fam]
    if fam in ELLIPTICAL:
        sg = (theta / 0.99 + 1.0) / 2.0
    elif fam == "plackett":
        sg = np.log10(theta / 0.1) / 4.0
    else:
        sg = (theta - lo) / (hi - lo)
    sg = min(max(float(sg), 1e-12), 1.0 - 1e-12)
    return float(np.log(sg) - np.log1p(-sg))


def _log1mexp(y):
    with np.errstate(all="ignore"):
        return np.where(y > np.log(y.dtype.type(2)), np.log1p(-np.exp(-y)), np.log(-np.expm1(-y)))


def prepare(copula, u, nu=None, dtype=np.float64, z=None):
    """Everything of the rows that does not depend on f (k_gas_prep's job), as a dict of (N, ...) arrays."""
    fam = FAMILY[copula]
    u = np.asarray(u, dtype=np.float64)
    ud = u.astype(dtype)
    rot = copula in ROTATED
    with np.errstate(all="ignore"):
        if fam in ELLIPTICAL:
            if z is None:
                from scipy import special
                z = special.ndtri(u) if fam == "gaussian" else special.stdtrit(float(nu), u)
            z = np.asarray(z).astype(dtype)
            w = {"A": z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1], "P": z[:, 0] * z[:, 1]}
            if fam == "student":
                from math import lgamma
                v = dtype(nu)
                cst = dtype(lgamma(0.5 * (nu + 2.0)) + lgamma(0.5 * nu) - 2.0 * lgamma(0.5 * (nu + 1.0)))   # (float64 constant)
                w["base"] = cst + (v + 1) / 2 * (np.log1p(z[:, 0] * z[:, 0] / v) + np.log1p(z[:, 1] * z[:, 1] / v))
            return w
        if fam == "plackett":
            a, b = ud[:, 0], ud[:, 1]
            return {"s": a + b - 2 * a * b, "p": a + b, "m": 1 - a - b}
        if fam == "gumbel":
            ell = np.log1p(-ud) if rot else np.log(ud)
            lx = np.log(-ell)
            return {"lx": lx, "sumell": np.sum(ell, axis=1), "sumlx": np.sum(lx, axis=1)}
        if fam == "frank":
            return {"u": ud}
        return {"l": np.log(ud) if rot else np.log1p(-ud)}


def _product_form(d, a, da, sB, dsB, p0, dp0, q0, dq0, kap, dkap, c2, dc2, c3, dc3, lc, dlc):
    S, dS = sum(a), sum(da)
    E, ex = np.expm1(-S), np.exp(-S)
    om = q0 - p0 * E
    dom = dq0 - dp0 * E + p0 * ex * dS
    p = p0 * ex
    dp = dp0 * ex - p * dS
    if d == 2:
        poly, dpoly = om + c2 * p, dom + dc2 * p + c2 * dp
    else:
        inner = c2 * om + c3 * p
        poly = om * om + p * inner
        dpoly = 2 * om * dom + dp * inner + p * (dc2 * om + c2 * dom + dc3 * p + c3 * dp)
    ell = sB + lc - S + (kap - d) * np.log(om) + np.log(poly)
    return ell, dsB + dlc - dS + dkap * np.log(om) + (kap - d) * dom / om + dpoly / poly


def logc_score(copula, dim, th, w, t, nu=None):
    """(log c, d log c / d theta) of row t at the candidates' theta (B,)."""
    fam = FAMILY[copula]
    dt = th.dtype.type
    if fam == "gaussian":
        A, P = w["A"][t], w["P"][t]
        om = 1 - th * th
        N2 = th * th * A - 2 * th * P
        return -np.log(om) / 2 - N2 / (2 * om), th / om - ((th * A - P) * om + th * N2) / (om * om)
    if fam == "student":
        A, P, v = w["A"][t], w["P"][t], dt(nu)
        om = 1 - th * th
        num = A - 2 * th * P
        q = num / om
        dq = (-2 * P * om + 2 * th * num) / (om * om)
        return w["base"][t] - np.log(om) / 2 - (v + 2) / 2 * np.log1p(q / v), th / om - (v + 2) / 2 * dq / (v + q)
    if fam == "plackett":
        s, p, m = w["s"][t], w["p"][t], w["m"][t]
        t1 = th - 1
        n1, a, b = 1 + t1 * s, 1 + t1 * p, 1 + t1 * m
        return np.log(th * n1) - np.log((a * b) * (a * b)), 1 / th + s / n1 - 2 * p / a - 2 * m / b
    if fam == "gumbel":
        lx = w["lx"][t]                                            # (dim,)
        tt = th[:, None] * lx[None, :]
        mx = np.max(tt, axis=1)
        e = np.exp(tt - mx[:, None])
        se = np.sum(e, axis=1)
        logS = mx + np.log(se)
        dlogS = np.sum(e * lx[None, :], axis=1) / se
        logA = logS / th
        dlogA = (dlogS - logA) / th
        A = np.exp(logA)
        dA = A * dlogA
        t1 = th - 1
        if dim == 2:
            poly, dpoly = A + t1, dA + 1
        else:
            poly = A * A + 3 * t1 * A + t1 * (2 * th - 1)
            dpoly = 2 * A * dA + 3 * A + 3 * t1 * dA + (2 * th - 1) + 2 * t1
        ell = -A - w["sumell"][t] + t1 * w["sumlx"][t] + (1 - dim * th) * logA + np.log(poly)
        return ell, -dA + w["sumlx"][t] - dim * logA + (1 - dim * th) * dlogA + dpoly / poly
    zero, one = th * 0, th * 0 + 1
    if fam == "frank":
        u = w["u"][t]
        g, dg = -np.expm1(-th), np.exp(-th)
        lg, dlg = _log1mexp(th), 1 / np.expm1(th)
        eth, lth = np.exp(-th), np.log(th)
        a, da, sB, dsB = [], [], zero, zero
        for i in range(dim):
            X = eth * np.expm1(th * (1 - u[i])) / g
            with np.errstate(all="ignore"):
                ai = np.where(X <= 0.5, -np.log1p(-X), lg - _log1mexp(th * u[i]))
            dai = dlg - u[i] / np.expm1(th * u[i])
            a.append(ai)
            da.append(dai)
            sB = sB + (lth - th * u[i] + ai - lg)
            dsB = dsB + (1 / th - u[i] + dai - dlg)
        c2, c3 = (one, zero) if dim == 2 else (3 * one, 2 * one)
        return _product_form(dim, a, da, sB, dsB, g, dg, eth, -eth, zero, zero, c2, zero, c3, zero, lg - lth, dlg - 1 / th)
    lj = w["l"][t]
    lth = np.log(th)
    a, da, sB, dsB = [], [], zero, zero
    for i in range(dim):
        y = -th * lj[i]
        ai = -_log1mexp(y)
        dai = lj[i] / np.expm1(y)
        a.append(ai)
        da.append(dai)
        sB = sB + (lth + (th - 1) * lj[i] + ai)
        dsB = dsB + (1 / th + lj[i] + dai)
    kap, dkap = 1 / th, -1 / (th * th)
    k, dk = 1 - kap, 1 / (th * th)
    if dim == 2:
        c2, dc2, c3, dc3 = k, dk, zero, zero
    else:
        c2, dc2, c3, dc3 = 3 * k, 3 * dk, k * (1 + k), dk * (1 + 2 * k)
    return _product_form(dim, a, da, sB, dsB, one, zero, zero, zero, kap, dkap, c2, dc2, c3, dc3, -lth, -1 / th)


def run(copula, u, params, nu=None, dtype=np.float64, z=None):
    """params (B, 3) -> dict: theta (B, N + 1), logc (B, N), ll (B,), scale (B,) = sum |l_t|.  The
    kernels' NaN rule: a candidate whose l, s or next f stops being finite at row t has ll NaN, logc
    NaN from row t and theta NaN from row t + 1; |beta| >= 1 or a non-finite parameter: all NaN."""
    u = np.asarray(u, dtype=np.float64)
    N, dim = u.shape
    prm = np.atleast_2d(np.asarray(params, dtype=np.float64))
    B = prm.shape[0]
    w = prepare(copula, u, nu, dtype, z)
    om, al, be = (prm[:, j].astype(dtype) for j in range(3))
    with np.errstate(all="ignore"):
        ok = np.all(np.isfinite(prm), axis=1) & (np.abs(prm[:, 2]) < 1.0)
        f = om / (1 - be)
        ok &= np.isfinite(f)
        theta, logc = np.full((B, N + 1), np.nan, dtype=dtype), np.full((B, N), np.nan, dtype=dtype)
        ll, scale = np.zeros(B, dtype=dtype), np.zeros(B, dtype=dtype)
        for t in range(N):
            th, dth = link(copula, f)
            ell, dell = logc_score(copula, dim, th, w, t, nu)
            s = dell * dth
            fn = om + be * f + al * s
            theta[ok, t] = th[ok]
            ok &= np.isfinite(ell) & np.isfinite(s) & np.isfinite(fn)
            logc[ok, t] = ell[ok]
            ll = ll + ell
            scale = scale + np.abs(ell)
            f = np.clip(fn, -dtype(F_CLAMP), dtype(F_CLAMP))
        theta[ok, N] = link(copula, f)[0][ok]
    ll = np.where(ok, ll, np.nan)
    return {"theta": theta, "logc": logc, "ll": ll, "scale": np.where(ok, scale, np.nan)}


def loglik(copula, u, nu=None):
    """rows (B, 3) -> LL (B,): the `loglik` callable GasCopulaOptimizer takes in place of the device."""
    return lambda rows: run(copula, u, rows, nu)["ll"].astype(np.float64)
