"""Writes tests/golden/gas_copula.kat (an .npz container; tests/gas_cases.py KAT_PATH): the truths of
the score-driven copula recursion at 50 significant digits (mpmath).  Run from the repository root
on a CPU machine with mpmath:

    python tests/kat/gen_gas_kat.py

Per case (gas_cases.cases(); R = len(param_rows), N = gas_cases.N_MAX), keyed "<case id>_<name>":
  theta (R, N + 1), logc (R, N)   the path and the per-row log densities of the full series
  ll, scale (R, len(NS))          sum l_t and sum |l_t| of each prefix length in gas_cases.NS
  z (N, 2)                        Gaussian / Student cases: the exact quantiles of u (for longdouble reruns)
  sha                             SHA-256 of the case's u and candidate rows
all float64 roundings of the 50-digit values.

Independence.  The densities are restated here from the docstring formulas of copula_var/copulas.py
in their plain form (log1p / expm1 only where 50 digits would otherwise lose the value), the
quantiles are solved from the distribution functions, and the score is mpmath's numerical derivative (mp.diff) of f -> log c(u; link(f)): no hand derivation
and none of the kernels' or gas_reference's arithmetic enters.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE),):
    if p not in sys.path:
        sys.path.insert(0, p)

import gas_cases as GC                   # noqa: E402

mp.mp.dps = 50
ONE = mp.mpf(1)


def sigma(f):
    return ONE / (ONE + mp.exp(-f))


def link(copula, f):
    fam = GC.GR.FAMILY[copula]
    if fam in ("gaussian", "student"):
        return mp.mpf("0.99") * (2 * sigma(f) - ONE)
    if fam == "plackett":
        return mp.mpf("0.1") * mp.power(10, 4 * sigma(f))
    if fam == "frank":
        return mp.mpf("1e-3") + (32 - mp.mpf("1e-3")) * sigma(f)
    return mp.mpf("1.0001") + (16 - mp.mpf("1.0001")) * sigma(f)


def norm_ppf(u):
    return mp.sqrt(2) * mp.erfinv(2 * u - ONE)


def t_cdf_lower(t, nu):
    """F(t) for t <= 0."""
    return mp.betainc(nu / 2, ONE / 2, 0, nu / (nu + t * t), regularized=True) / 2


def t_ppf(u, nu):
    from scipy import special
    if u > mp.mpf("0.5"):
        return -t_ppf(ONE - u, nu)
    if u == mp.mpf("0.5"):
        return mp.mpf(0)
    guess = mp.mpf(float(special.stdtrit(float(nu), float(u))))
    return mp.findroot(lambda t: mp.log(t_cdf_lower(t, nu)) - mp.log(u), guess, tol=mp.mpf(10) ** -45)


def quantiles(case, u):
    kind, dim, nu = case
    if kind == "gaussian":
        return [[norm_ppf(mp.mpf(float(v))) for v in row] for row in u]
    return [[t_ppf(mp.mpf(float(v)), mp.mpf(nu)) for v in row] for row in u]


def _product_form(a, B, p0, q0, kappa, c2, c3, lc):
    d = len(a)
    S = sum(a)
    om = q0 - p0 * mp.expm1(-S)
    p = p0 * mp.exp(-S)
    poly = om + c2 * p if d == 2 else om * om + p * (c2 * om + c3 * p)
    return sum(B) + lc - S + (kappa - d) * mp.log(om) + mp.log(poly)


def log_density(case, row, zrow, th):
    """log c(u; theta): copulas.py's docstring formulas, plainly."""
    kind, dim, nu = case
    fam = GC.GR.FAMILY[kind]
    u = [mp.mpf(float(v)) for v in row]
    if kind in GC.GR.ROTATED:
        u = [ONE - v for v in u]
    if fam == "gaussian":
        x, y = zrow
        det = ONE - th * th
        qf = (x * x + y * y - 2 * th * x * y) / det
        mv = mp.exp(-qf / 2) / mp.sqrt((2 * mp.pi) ** 2 * det)
        uni = [mp.exp(-v * v / 2) / mp.sqrt(2 * mp.pi) for v in (x, y)]
        return mp.log(mv / (uni[0] * uni[1]))
    if fam == "student":
        x, y = zrow
        nu = mp.mpf(nu)
        det = ONE - th * th
        qf = (x * x + y * y - 2 * th * x * y) / det
        term1 = mp.gamma((nu + 2) / 2) / (mp.gamma(nu / 2) * (nu * mp.pi) * mp.sqrt(det))
        g = mp.gamma((nu + 1) / 2) / (mp.sqrt(nu * mp.pi) * mp.gamma(nu / 2))
        mv = term1 * (1 + qf / nu) ** (-(nu + 2) / 2)
        uni = [g * (1 + v * v / nu) ** (-(nu + 1) / 2) for v in (x, y)]
        return mp.log(mv / (uni[0] * uni[1]))
    if fam == "plackett":
        a, b = u
        num = th * (1 + (th - 1) * (a + b - 2 * a * b))
        den = ((1 + (th - 1) * (a + b)) * (1 + (th - 1) * (1 - a - b))) ** 2
        return mp.log(num / den)
    if fam == "gumbel":
        x = [-mp.log(v) for v in u]
        S = sum(v ** th for v in x)
        A = S ** (ONE / th)
        poly = A + (th - 1) if dim == 2 else A * A + 3 * (th - 1) * A + (th - 1) * (2 * th - 1)
        return -A + sum(x) + (th - 1) * sum(mp.log(v) for v in x) + (1 - dim * th) * mp.log(A) + mp.log(poly)
    if fam == "frank":
        g = ONE - mp.exp(-th)
        a = [-mp.log((ONE - mp.exp(-th * v)) / g) for v in u]
        B = [mp.log(th) - th * v + ai - mp.log(g) for v, ai in zip(u, a)]
        c2, c3 = (1, 0) if dim == 2 else (3, 2)
        return _product_form(a, B, g, mp.exp(-th), 0, c2, c3, mp.log(g) - mp.log(th))
    a = [-mp.log1p(-(ONE - v) ** th) for v in u]        # (1 - v)^theta can be below 1e-50
    B = [mp.log(th) + (th - 1) * mp.log(ONE - v) + ai for v, ai in zip(u, a)]
    kap = ONE / th
    k = ONE - kap
    c2, c3 = (k, 0) if dim == 2 else (3 * k, k * (1 + k))
    return _product_form(a, B, ONE, mp.mpf(0), kap, c2, c3, -mp.log(th))


def case_rows(case, n_max=GC.N_MAX, rows=None):
    """The fixture arrays of one case over its first n_max rows (rows: the candidate indices; None = all)."""
    kind, dim, nu = case
    u = GC.series(case)[:n_max]
    prm = GC.param_rows(case)
    sel = range(len(prm)) if rows is None else rows
    z = quantiles(case, u) if kind in GC.GR.ELLIPTICAL else [None] * len(u)
    theta = np.zeros((len(prm), n_max + 1))
    logc = np.zeros((len(prm), n_max))
    ns = [n for n in GC.NS if n <= n_max]
    ll, scale = np.zeros((len(prm), len(GC.NS))), np.zeros((len(prm), len(GC.NS)))
    for r in sel:
        om, al, be = (mp.mpf(float(v)) for v in prm[r])
        f = om / (ONE - be)
        acc, sc = mp.mpf(0), mp.mpf(0)
        for t in range(n_max):
            fun = lambda x: log_density(case, u[t], z[t], link(kind, x))       # noqa: E731
            theta[r, t] = float(link(kind, f))
            ell = fun(f)
            s = mp.diff(fun, f)
            logc[r, t] = float(ell)
            acc += ell
            sc += abs(ell)
            if t + 1 in ns:
                ll[r, GC.NS.index(t + 1)], scale[r, GC.NS.index(t + 1)] = float(acc), float(sc)
            f = om + be * f + al * s
            f = max(min(f, mp.mpf(40)), mp.mpf(-40))
        theta[r, n_max] = float(link(kind, f))
    out = {"theta": theta, "logc": logc, "ll": ll, "scale": scale, "sha": np.array(GC.case_digest(u, prm))}
    if kind in GC.GR.ELLIPTICAL:
        out["z"] = np.array([[float(v) for v in row] for row in z])
    return out


def main():
    out = {}
    for case in GC.cases():
        for k, a in case_rows(case).items():
            out[GC.key(case, k)] = a
        print(GC.case_id(case), "ll", out[GC.key(case, "ll")][:, -1].tolist(), flush=True)
    with open(GC.KAT_PATH, "wb") as f:              # (a file object: savez appends no ".npz")
        np.savez_compressed(f, **out)
    print("wrote", GC.KAT_PATH, os.path.getsize(GC.KAT_PATH), "bytes")


if __name__ == "__main__":
    main()
