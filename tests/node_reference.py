"""High-precision restatement of the quadrature node arithmetic (csrc/cvq_special.h and the node
values built from it), next to insample_reference.py / forecast_reference.py.

Primitives: mpmath at 50 digits -- exp, log, powers, reciprocals, roots and the two quantiles
(t.ppf by Newton root-finding on the regularised incomplete beta from scipy's 1e-11 start, ndtri
via erfinv).  A truth is kept as a float64 pair hi + lo (hi = the rounded truth, lo = the rest).

Slabs: NodeProblem subclasses oracle.quadrature.Problem.  The membership mask, the Delta-weights
and the float64 u tables stay the oracle's: they are the reference's own float64 decisions.  The
quantiles are mpmath's on that float64 u; the copula constants come from mpmath's gamma and an
mpmath inverse of the correlation matrix; the marginal densities, the quadratic form, the powers
and the sums run in np.longdouble (64-bit mantissa).  Per date and slab:

  m0       = sum_mask mass                 scale  = sum_mask |mass|
  m1       = sum_mask level * mass         scale1 = sum_mask |level * mass|   (es_reference.levels)
  mx[c]    = sum_mask x[i_c] * mass        scalex[c] = sum_mask |x[i_c] * mass|   (attribution_reference)

Regular regime only, asserted: every u strictly inside (0, 1), |x| / sigma <= 8 (no node under- or
overflows in float64) and every mass finite.  The NaN / dead-entry / nan_to_num behaviours (Q15, dead
records) stay with the oracle-parity tests.
"""
import mpmath as mp
import numpy as np

from node_cases import code_class, half_power_code, plan_codes  # noqa: F401  (the plan rule's one Python copy)
from oracle.quadrature import Problem

mp.mp.dps = 50
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble must carry a 64-bit mantissa"


# ------------------------------------------------------------------ hi + lo pairs
def split(v):
    """mpf -> (hi, lo) float64 with hi + lo = v to ~2^-106."""
    v = mp.mpf(v)
    hi = float(v)
    if not np.isfinite(hi) or hi == 0.0:
        return hi, 0.0
    return hi, float(v - mp.mpf(hi))


def split_all(vals):
    p = np.array([split(v) for v in vals], dtype=np.float64).reshape(-1, 2)
    return p[:, 0].copy(), p[:, 1].copy()


def join(hi, lo):
    return np.asarray(hi, dtype=LD) + np.asarray(lo, dtype=LD)


# ------------------------------------------------------------------ quantiles
def _t_cdf_pdf(t, nu):
    """(F(t), pdf(t)) of Student-t for t < 0, mpmath."""
    t2 = t * t
    if t2 > nu:                         # x = nu / (nu + t^2) < 1/2: F = I_x(nu/2, 1/2) / 2
        F = mp.betainc(nu / 2, mp.mpf(1) / 2, 0, nu / (nu + t2), regularized=True) / 2
    else:                               # F = (1 - I_y(1/2, nu/2)) / 2, y = t^2 / (nu + t^2)
        F = (1 - mp.betainc(mp.mpf(1) / 2, nu / 2, 0, t2 / (nu + t2), regularized=True)) / 2
    ln_k = mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(nu * mp.pi) / 2
    return F, mp.exp(ln_k - (nu + 1) / 2 * mp.log1p(t2 / nu))


def t_ppf(u, nu):
    """t.ppf(u, nu) for a float64 u in (0, 1), as an mpf good to > 40 digits."""
    from scipy import special
    u = float(u)
    assert 0.0 < u < 1.0
    if u == 0.5:
        return mp.mpf(0)
    upper = u > 0.5
    pp = mp.mpf(1.0 - u if upper else u)            # 1 - u is exact in float64 for u > 1/2
    nu_m = mp.mpf(float(nu))
    t = mp.mpf(float(special.stdtrit(float(nu), float(pp))))
    if not (t < 0) or not mp.isfinite(t):           # far tail: F ~ C |t|^-nu
        ln_k = mp.loggamma((nu_m + 1) / 2) - mp.loggamma(nu_m / 2) - mp.log(nu_m * mp.pi) / 2
        t = -mp.exp((ln_k + (nu_m - 1) / 2 * mp.log(nu_m) - mp.log(pp)) / nu_m)
    lp = mp.log(pp)
    for _ in range(60):                             # Newton on log F = log pp: in t at the centre, in log|t|
        F, pdf = _t_cdf_pdf(t, nu_m)                # in the tail (log F is nearly linear in it there, so a
        g = mp.log(F) - lp                          # start decades off, as scipy's for nu = 1, still lands)
        if t * t > nu_m:
            tn = t * mp.exp(-g * F / (pdf * t))
        else:
            tn = t - g * F / pdf
        if not (tn < 0):
            tn = t / 2
        dt, t = tn - t, tn
        if abs(dt) <= abs(t) * mp.mpf(10) ** -44:
            break
    else:
        raise AssertionError(f"t_ppf did not converge at u = {u!r}, nu = {nu!r}")
    return -t if upper else t


def ndtri(u):
    """norm.ppf(u) for a float64 u in (0, 1), mpf."""
    u = float(u)
    assert 0.0 < u < 1.0
    with mp.workdps(80):                            # 2u - 1 cancels up to ~16 digits for u ~ 1e-16
        return +(mp.sqrt(2) * mp.erfinv(2 * mp.mpf(u) - 1))


# ------------------------------------------------------------------ slabs
class NodeProblem(Problem):
    """oracle Problem with the node values restated in longdouble from mpmath quantiles.

    z: the quantile tables (T, dim, n) as longdouble (a fixture's), or None to compute them
    with mpmath from the oracle's float64 u (Plackett has none)."""

    def __init__(self, *a, z=None, **kw):
        super().__init__(*a, **kw)
        self._z = None if z is None else np.asarray(z, dtype=LD)
        self.ftype = LD
        self._u = [self.axis_cdf(t)[0] for t in range(self.T)]
        for u in self._u:
            assert np.all((u > 0.0) & (u < 1.0)), "regular regime: every u strictly inside (0, 1)"
        if self.model != "msm":         # (MSM multiplies no marginal density in: u inside (0, 1) is its regime)
            assert np.max(np.abs(self.x)) / np.min(self.sigma) <= 8.0, "regular regime: |x| / sigma <= 8"
        if self.copula != "plackett":
            d = self.dim
            Rm = mp.matrix(d, d)
            for i in range(d):
                for j in range(d):
                    Rm[i, j] = mp.mpf(float(self.R[i, j]))
            Ri, det = Rm ** -1, mp.det(Rm)
            self.Ri_ld = np.array([[join(*split(Ri[i, j])) for j in range(d)] for i in range(d)], dtype=LD)
            if self.copula == "student":
                nu = mp.mpf(float(self.nu))
                t1 = mp.gamma((nu + d) / 2) / (mp.gamma(nu / 2) * (nu * mp.pi) ** (mp.mpf(d) / 2) * mp.sqrt(det))
                g = mp.gamma((nu + 1) / 2) / (mp.sqrt(nu * mp.pi) * mp.gamma(nu / 2))
                self.g_ld = join(*split(g))
            else:
                t1 = 1 / mp.sqrt((2 * mp.pi) ** d * det)
            self.term1_ld = join(*split(t1))

    def quantile_tables(self):
        """(T, dim, n) longdouble quantiles of the float64 u tables (mpmath unless given)."""
        if self._z is None:
            assert self.copula != "plackett"
            f = (lambda u: t_ppf(u, self.nu)) if self.copula == "student" else ndtri
            cache = {}
            out = np.empty((self.T, self.dim, self.n), dtype=LD)
            for t in range(self.T):
                for c in range(self.dim):
                    for i in range(self.n):
                        u = float(self._u[t][c, i])
                        if u not in cache:
                            cache[u] = join(*split(f(u)))
                        out[t, c, i] = cache[u]
            self._z = out
        return self._z

    def quantile_slope(self, t):
        """dz/du (dim, n) at the tables' points, longdouble: 1 / pdf(z)."""
        z = self.quantile_tables()[t]
        if self.copula == "student":
            nu = LD(self.nu)
            pdf = self.g_ld * (1 + z * z / nu) ** (-(nu + 1) / 2)
        else:
            pdf = np.exp(-z * z / 2) / np.sqrt(2 * LD(np.pi))
        return 1 / pdf

    def mass_ld(self, t, ulp_shift=0):
        """Integrand x Delta on every node of date t, longdouble.  ulp_shift = +-1: every u moved by
        one ulp, to first order (z + dz/du ulp(u); Plackett: u itself).  self.ftype = np.float64 runs the
        same arithmetic in float64 (the quantiles rounded): what separates the oracle from this reference
        then is the oracle's quantile alone."""
        LD = self.ftype
        d, n = self.dim, self.n
        u = self._u[t]
        du = ulp_shift * np.spacing(u).astype(LD) if ulp_shift else None
        if self.copula == "plackett":
            uu = u.astype(LD) + (du if ulp_shift else 0)
            U, V = self._broadcast(uu)[:2]
            th = LD(self.nu)
            num = th * (1 + (th - 1) * (U + V - 2 * U * V))
            den = ((1 + (th - 1) * (U + V)) * (1 + (th - 1) * (1 - U - V))) ** 2
            c = num / den
        else:
            z = self.quantile_tables()[t]
            if ulp_shift:
                z = z + self.quantile_slope(t) * du
            z = z.astype(LD)
            Z = self._broadcast(z)
            Ri = self.Ri_ld.astype(LD)
            qf = sum(Z[i] * Ri[i, j] * Z[j] for i in range(d) for j in range(d))
            if self.copula == "student":
                nu = LD(self.nu)
                mv = LD(self.term1_ld) * (1 + qf / nu) ** (-(nu + d) / 2)
                uni = LD(self.g_ld) * (1 + z * z / nu) ** (-(nu + 1) / 2)
            else:
                mv = LD(self.term1_ld) * np.exp(-qf / 2)
                uni = np.exp(-z * z / 2) / np.sqrt(2 * LD(np.pi))
            Un = self._broadcast(uni)
            prod = Un[0]
            for k in range(1, d):
                prod = prod * Un[k]
            c = mv / prod
        W = self.delta_weights(t).astype(LD)
        if self.model == "msm":
            m = c * W
        else:
            s = self.sigma[t].astype(LD)
            xs = self.x.astype(LD)[None, :] / s[:, None]
            pdf = np.exp(-xs * xs / 2) / (np.sqrt(2 * LD(np.pi)) * s[:, None])
            P = self._broadcast(pdf)
            dp = P[0]
            for k in range(1, d):
                dp = dp * P[k]
            m = c * dp * W
        assert np.all(np.isfinite(m)), "regular regime: every node mass finite"
        return m

    def levels_ld(self):
        x, w, d = self.x.astype(LD), self.w.astype(LD), self.dim
        lev = (w[0] * x).reshape([1] * (d - 1) + [self.n])
        for c in range(d - 1):
            lev = lev + (w[c + 1] * x).reshape([self.n if a == c else 1 for a in range(d)])
        return lev

    def slab_moments(self, slabs, ulp_shift=0):
        """dict of float64 arrays over (slab, date): m0, m1, scale, scale1 (S, T), mx, scalex
        (S, T, dim), count (S, T) = member nodes, scale_below (S, T) = sum |mass| over every node whose level
        is <= the slab's upper bound (what a difference of prefix sums rounds against)."""
        S, T, d = len(slabs), self.T, self.dim
        out = dict(m0=np.zeros((S, T)), m1=np.zeros((S, T)), scale=np.zeros((S, T)), scale1=np.zeros((S, T)),
                   mx=np.zeros((S, T, d)), scalex=np.zeros((S, T, d)), count=np.zeros((S, T), dtype=np.int64),
                   scale_below=np.zeros((S, T)))
        lev = self.levels_ld()
        for t in range(T):
            mass = self.mass_ld(t, ulp_shift)
            levb = np.broadcast_to(lev, mass.shape)
            for s, (a, b) in enumerate(slabs):
                mask = self.inner_mask(a, b)
                mm = mass[mask]
                out["count"][s, t] = mm.size
                out["scale_below"][s, t] = float(np.sum(np.abs(mass[(levb <= b) | mask])))
                out["m0"][s, t] = float(np.sum(mm))
                out["scale"][s, t] = float(np.sum(np.abs(mm)))
                lm = levb[mask] * mm
                out["m1"][s, t] = float(np.sum(lm))
                out["scale1"][s, t] = float(np.sum(np.abs(lm)))
                for c in range(d):
                    xc = np.broadcast_to(self.x.astype(LD).reshape([self.n if k == c else 1 for k in range(d)]),
                                         mass.shape)
                    xm = xc[mask] * mm
                    out["mx"][s, t, c] = float(np.sum(xm))
                    out["scalex"][s, t, c] = float(np.sum(np.abs(xm)))
        return out

    def conditioning(self, slabs):
        """max over slabs, dates and both directions of |m0(u +- 1 ulp) - m0| / scale."""
        base = self.slab_moments(slabs)
        worst = 0.0
        for sh in (+1, -1):
            m0 = np.zeros_like(base["m0"], dtype=LD)
            b0 = np.zeros_like(m0)
            for t in range(self.T):
                ms, mb = self.mass_ld(t, sh), self.mass_ld(t)
                for s, (a, b) in enumerate(slabs):
                    mask = self.inner_mask(a, b)
                    m0[s, t], b0[s, t] = np.sum(ms[mask]), np.sum(mb[mask])
            worst = max(worst, float(np.max(np.abs(m0 - b0) / base["scale"])))
        return worst
