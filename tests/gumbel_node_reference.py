"""Longdouble restatement of tests/gumbel_reference.py's mass(t), next to node_reference.py, and the
first-order error bound of the device's own Gumbel formulas that the GPU bars are built from.

GumbelNodeProblem subclasses GumbelProblem.  The membership mask, the Delta-weights and the float64 u
tables stay the oracle's, as in NodeProblem.  Everything downstream of u runs above float64.  A sum of
longdouble logs cannot hold the node to the 1e-17 the mpmath spot check asks for: the exponent adds terms
of size up to several hundred, each rounded at 2^-64 of itself (4e-17 measured at theta = 1 already).  So
the per-axis factors A_i = x_i^theta and F_i = pdf_i x_i^(theta - 1) / u_i -- log / log1p, the powers and
the GARCH / UKF marginal pdf, dim x n values per date -- are formed by mpmath at 50 digits and rounded to
longdouble once (as NodeProblem takes its quantiles from mpmath), and the node
prod F_i exp(-A) S^((1 - d theta) / theta) poly_d(A) W, S = sum A_i, A = S^(1 / theta), the polynomial and
the sums run in np.longdouble; the spot check (mp_mass: the log form of gumbel_reference.py, all in
mpmath) then agrees to 6.7e-18.  The error bound below takes its magnitudes from a plain longdouble
evaluation of the log form (_axis / _node).  Regular regime only, asserted: every u strictly inside (0, 1), |x| / sigma <= 8, every mass finite and no table entry
x^theta under the device's floor (kGumbelFloor).  Dead entries and the floor stay with
tests/test_gumbel_gpu.py / test_gumbel_cpu.py.

The error bound (ebound_nodes), in units of U = 2^-53, first order, per node.  The Gumbel node is
exp(E) poly W, so an absolute error of E is a relative error of the node.  LIB = 2 U is one ulp, the
accuracy the HIP math API documentation states for the double-precision log, log1p and exp of the
device library (taken as stated, not measured here); NODE = 1.4e-14 / U is what cvq_special.h
documents for log_node / exp_node (relative).  |.| of a rounded intermediate costs U times its size.

  table_entry<CVQ_GUMBEL> (cvq_quad_kernels.h:129-139), per axis:
    l  = log u | log1p(-u)                         dl  = LIB |l|
    lx = log(-l)                                   dlx = dl / |l| + LIB |lx| = 2 + 2 |lx|
    A  = exp(theta lx)            relative:        rA  = theta dlx + |theta lx| + LIB
         (theta dlx is the theta |delta log x| carried by A = exp(theta log x); |theta lx| the product's rounding)
    pdf (GARCH / UKF, marginal_u :104-107)         rpdf = 1.5 xs^2 + 5    (xs = x / sigma: 1; xs xs: 3 relative,
         i.e. 1.5 xs^2 absolute in the exponent; exp: LIB; the constant, the product, the division: 3); MSM: pdf = 1
    log(pdf)                                       dlp = rpdf + LIB |log pdf|
    (theta - 1) lx                                 dq  = 2 |(theta - 1) lx| + (theta - 1) dlx
    B  = (log pdf + (theta - 1) lx) - l            dB  = dlp + dq + |log pdf + (theta - 1) lx| + dl + |B|   (stored B)
  node_value<CVQ_GUMBEL> (:190-204):
    S  = sum A_i                  relative:        rS  = max rA_i + (d - 1)
    lA = log_node(S) / theta                       dlA = rS / theta + (NODE + 1) |lA|
    Av = exp_node(lA)             relative:        rAv = dlA + NODE
    poly_d(Av), positive terms    relative:        rp  = (d - 1) rAv + 3
    Bs = sum B_i  (outer_B, r.B + Bc)              dBs = sum dB_i + (d - 1) sum |B_i|
    G  = Bs - Av                                   dG  = dBs + Av rAv + |G|
    E  = fma(1 - d theta, lA, G)                   dE  = 2 |(1 - d theta) lA| + |1 - d theta| dlA + dG + |E|
    v  = exp_node(E) poly W       relative:        dE + NODE + rp + 2
  SORTED's fast record path (cvq_sorted_kernels.h:473-486, :578-594), what differs:
    L_i = log2(e) (B_i + log w_i)                  dL  = dB + LIB |log w_i| + 3 |B_i + log w_i|   (natural units:
         the sum, the constant log2(e) and the product round once each)
    lA = log_node(S) (1 / theta)                   dlA = rS / theta + (NODE + 2) |lA|
    G  = fma(-log2(e), Av, sum L_i)                dG  = sum dL_i + (d - 1) sum |B_i + log w_i| + Av (rAv + 1) + |G|
    E  = fma((1 - d theta) log2(e), lA, G)         dE  = 4 |(1 - d theta) lA| + |1 - d theta| dlA + dG + |E|
    v  = exp2_node7(E log2(e)) poly                dE + rp + 2, and exp2_node7's own 4.05e-11 on top (EXP7_BAR)
The fixture stores the bound weighted by |mass| (|level mass|, |x_c mass|) per case, slab and date.
"""
import numpy as np

from gumbel_reference import GumbelProblem

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble must carry a 64-bit mantissa"
U = 2.0 ** -53
LIB = 2.0                                  # one ulp, in units of U: the device library's log / log1p / exp
NODE = 1.4e-14 / U                         # log_node / exp_node, cvq_special.h
GUMBEL_FLOOR = 1.0e-300                    # kGumbelFloor, cvq_quad_kernels.h:111


def _ld(v):
    """mpf -> the nearest longdouble (through a float64 pair)."""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


class GumbelNodeProblem(GumbelProblem):
    """GumbelProblem with the node masses restated in longdouble from the oracle's float64 u."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._u = [self.axis_cdf(t)[0] for t in range(self.T)]
        self._tab = {}
        for u in self._u:
            assert np.all((u > 0.0) & (u < 1.0)), "regular regime: every u strictly inside (0, 1)"
        if self.model != "msm":
            assert np.max(np.abs(self.x)) / np.min(self.sigma) <= 8.0, "regular regime: |x| / sigma <= 8"
        for t in range(self.T):
            assert np.all(self._axis(t)["A"] >= GUMBEL_FLOOR), "regular regime: no entry under kGumbelFloor"

    # ------------------------------------------------------------------ per-axis tables, longdouble
    def _axis(self, t, ulp_shift=0):
        u64 = self._u[t]
        u = u64.astype(LD)
        if ulp_shift:
            u = u + ulp_shift * np.spacing(u64).astype(LD)
        th = LD(self.theta)
        l = np.log1p(-u) if self.survival else np.log(u)
        lx = np.log(-l)
        if self.model == "msm":
            lp = np.zeros_like(u)
            xs = np.zeros_like(u)
        else:
            s = self.sigma[t].astype(LD)[:, None]
            xs = self.x.astype(LD)[None, :] / s
            lp = -xs * xs / 2 - np.log(np.sqrt(2 * LD(np.pi)) * s)
        return dict(l=l, lx=lx, lp=lp, xs=xs, A=np.exp(th * lx), B=(lp + (th - 1) * lx) - l)

    def _node(self, ax):
        """(lA, Av, poly, E) on the box from the per-axis tables."""
        d, th = self.dim, LD(self.theta)
        tl = self._broadcast(th * ax["lx"])
        logS = tl[0]
        for k in range(1, d):
            logS = np.logaddexp(logS, tl[k])
        lA = logS / th
        Av = np.exp(lA)
        poly = Av + (th - 1) if d == 2 else Av * Av + 3 * (th - 1) * Av + (th - 1) * (2 * th - 1)
        Bs = sum(self._broadcast(ax["B"]))
        return lA, Av, poly, (1 - d * th) * lA + (Bs - Av)

    def _tables(self, t, ulp_shift=0):
        """(A, F) (dim, n) longdouble roundings of mpmath's A_i = x_i^theta and F_i = pdf_i x_i^(theta - 1) / u_i
        (survival: / (1 - u_i); MSM: pdf_i = 1) on the float64 u (+- one ulp).  The node's exponent sums terms
        of size up to several hundred, which no sum of longdouble logs holds to 1e-17; per-axis factors formed
        at 50 digits and multiplied do."""
        import mpmath as mp
        key = (t, ulp_shift)
        if key not in self._tab:
            with mp.workdps(50):
                th = mp.mpf(self.theta)
                A = np.zeros((self.dim, self.n), dtype=LD)
                F = np.zeros((self.dim, self.n), dtype=LD)
                for c in range(self.dim):
                    for i in range(self.n):
                        u64 = float(self._u[t][c, i])
                        u = mp.mpf(u64) + ulp_shift * mp.mpf(float(np.spacing(u64)))
                        x = -(mp.log1p(-u) if self.survival else mp.log(u))
                        f = x ** (th - 1) / ((1 - u) if self.survival else u)
                        if self.model != "msm":
                            s = mp.mpf(float(self.sigma[t, c]))
                            xs = mp.mpf(float(self.x[i])) / s
                            f = f * mp.exp(-xs * xs / 2) / (mp.sqrt(2 * mp.pi) * s)
                        A[c, i], F[c, i] = _ld(x ** th), _ld(f)
            self._tab[key] = (A, F)
        return self._tab[key]

    def mass_ld(self, t, ulp_shift=0):
        """Integrand x Delta on every node of date t (ulp_shift = +-1: every u moved one ulp):
        prod F_i exp(-A) S^((1 - d theta) / theta) poly_d(A) W with S = sum A_i, A = S^(1 / theta), longdouble."""
        import mpmath as mp
        d, th = self.dim, LD(self.theta)
        A, F = self._tables(t, ulp_shift)
        S = sum(self._broadcast(A))
        prod = self._broadcast(F)[0]
        for k in range(1, d):
            prod = prod * self._broadcast(F)[k]
        with mp.workdps(50):
            p = (1 - d * mp.mpf(self.theta)) / mp.mpf(self.theta)
            p_hi = _ld(p)
            p_lo = float(p - mp.mpf(float(p_hi)) - mp.mpf(float(p_hi - LD(float(p_hi)))))
        Av = S ** (1 / th)
        poly = Av + (th - 1) if d == 2 else Av * Av + 3 * (th - 1) * Av + (th - 1) * (2 * th - 1)
        m = prod * np.exp(-Av) * (S ** p_hi * (1 + LD(p_lo) * np.log(S))) * poly * self.delta_weights(t).astype(LD)
        assert np.all(np.isfinite(m)), "regular regime: every node mass finite"
        return m

    # ------------------------------------------------------------------ the device's formulas
    def axis_weights_log(self, t):
        """|log w_c(i)| (dim, n): the per-axis Delta factor whose log SORTED's fast record carries."""
        d = self.dim
        out = np.zeros((d, self.n), dtype=LD)
        for c in range(d):
            if self.model == "msm":
                fax = c if d == 2 else (c + 2) % 3
                w = np.sum(self.fbs[t, fax, :, None] * self.dens[(c - 1) % d] * self.step, axis=0)
            else:
                w = self.dens[(c - 1) % d, 0] * self.step
            out[c] = np.abs(np.log(np.broadcast_to(w, (self.n,)).astype(LD)))
        return out

    def ebound_nodes(self, t, fast=False):
        """The module docstring's bound per node of date t (float64, relative to the node)."""
        d, th = self.dim, LD(self.theta)
        ax = self._axis(t)
        l, lx, lp = np.abs(ax["l"]), np.abs(ax["lx"]), np.abs(ax["lp"])
        dl = LIB * l
        dlx = 2 + LIB * lx
        rA = th * dlx + th * lx + LIB
        dlp = 0 * l if self.model == "msm" else 1.5 * ax["xs"] ** 2 + 5 + LIB * lp
        dq = 2 * (th - 1) * lx + (th - 1) * dlx
        dB = dlp + dq + np.abs(ax["lp"] + (th - 1) * ax["lx"]) + dl + np.abs(ax["B"])
        lA, Av, poly, E = self._node(ax)
        lA_a, coef = np.abs(lA), abs(1 - d * th)
        rS = np.maximum.reduce(np.broadcast_arrays(*self._broadcast(rA))) + (d - 1)
        if not fast:
            dlA = rS / th + (NODE + 1) * lA_a
            rAv = dlA + NODE
            dBs = sum(self._broadcast(dB)) + (d - 1) * sum(self._broadcast(np.abs(ax["B"])))
            dG = dBs + Av * rAv + np.abs(E + coef * lA)          # G = Bs - Av = E - (1 - d theta) lA
            dE = 2 * coef * lA_a + coef * dlA + dG + np.abs(E)
            out = dE + NODE + ((d - 1) * rAv + 3) + 2
        else:
            lw = self.axis_weights_log(t)
            # |B + log w| <= |B| + |log w|
            bw = np.abs(ax["B"]) + lw
            dL = dB + LIB * lw + 3 * bw
            dlA = rS / th + (NODE + 2) * lA_a
            rAv = dlA + NODE
            Ew = np.abs(E) + sum(self._broadcast(lw))            # the record's exponent also carries log W
            dG = sum(self._broadcast(dL)) + (d - 1) * sum(self._broadcast(bw)) + Av * (rAv + 1) + (Ew + coef * lA_a)
            dE = 4 * coef * lA_a + coef * dlA + dG + Ew
            out = dE + ((d - 1) * rAv + 3) + 2
        return (out * U).astype(np.float64)

    def device_mass(self, t):
        """float64 numpy restatement of table_entry / node_value (tests/test_gumbel_cpu.py's
        _device_formula_mass, for both models and dimensions, numpy's log / log1p / exp in the library's
        and the node helpers' place, products and sums in place of the FMAs)."""
        th, d = self.theta, self.dim
        u, pdf = self.axis_cdf(t)
        l = np.log1p(-u) if self.survival else np.log(u)
        lx = np.log(-l)
        A = np.maximum(np.exp(th * lx), GUMBEL_FLOOR)
        B = ((0.0 if pdf is None else np.log(pdf)) + (th - 1.0) * lx) - l
        S = sum(self._broadcast(A))
        Bs = sum(self._broadcast(B))
        lA = np.log(S) / th
        Av = np.exp(lA)
        t1 = th - 1.0
        poly = Av + t1 if d == 2 else Av * (3.0 * t1 + Av) + t1 * (2.0 * th - 1.0)
        v = (np.exp((1.0 - d * th) * lA + (Bs - Av)) * poly) * self.delta_weights(t)
        return np.where(np.isfinite(v), v, 0.0)

    # ------------------------------------------------------------------ slabs (NodeProblem's interface)
    def levels_ld(self):
        x, w, d = self.x.astype(LD), self.w.astype(LD), self.dim
        lev = (w[0] * x).reshape([1] * (d - 1) + [self.n])
        for c in range(d - 1):
            lev = lev + (w[c + 1] * x).reshape([self.n if a == c else 1 for a in range(d)])
        return lev

    def slab_moments(self, slabs, ulp_shift=0):
        """NodeProblem.slab_moments' dict over (slab, date) -- m0, m1, mx, scale, scale1, scalex, count,
        scale_below -- plus ebound, ebound1, eboundx (the bound weighted by |mass|, |level mass|,
        |x_c mass| over the slab's members) and ebound_fast (SORTED's record path, by |mass|)."""
        S, T, d = len(slabs), self.T, self.dim
        out = dict(m0=np.zeros((S, T)), m1=np.zeros((S, T)), scale=np.zeros((S, T)), scale1=np.zeros((S, T)),
                   mx=np.zeros((S, T, d)), scalex=np.zeros((S, T, d)), count=np.zeros((S, T), dtype=np.int64),
                   scale_below=np.zeros((S, T)), ebound=np.zeros((S, T)), ebound1=np.zeros((S, T)),
                   eboundx=np.zeros((S, T, d)), ebound_fast=np.zeros((S, T)))
        lev = self.levels_ld()
        for t in range(T):
            mass = self.mass_ld(t, ulp_shift)
            eb, ebf = self.ebound_nodes(t).astype(LD), self.ebound_nodes(t, fast=True).astype(LD)
            levb = np.broadcast_to(lev, mass.shape)
            for s, (a, b) in enumerate(slabs):
                mask = self.inner_mask(a, b)
                mm, am = mass[mask], np.abs(mass[mask])
                out["count"][s, t] = mm.size
                out["scale_below"][s, t] = float(np.sum(np.abs(mass[(levb <= b) | mask])))
                out["m0"][s, t] = float(np.sum(mm))
                out["scale"][s, t] = float(np.sum(am))
                out["ebound"][s, t] = float(np.sum(am * eb[mask]) / np.sum(am))
                out["ebound_fast"][s, t] = float(np.sum(am * ebf[mask]) / np.sum(am))
                lm = levb[mask] * mm
                out["m1"][s, t] = float(np.sum(lm))
                out["scale1"][s, t] = float(np.sum(np.abs(lm)))
                out["ebound1"][s, t] = float(np.sum(np.abs(lm) * eb[mask]) / np.sum(np.abs(lm)))
                for c in range(d):
                    xc = np.broadcast_to(self.x.astype(LD).reshape([self.n if k == c else 1 for k in range(d)]),
                                         mass.shape)
                    xm = xc[mask] * mm
                    out["mx"][s, t, c] = float(np.sum(xm))
                    sx = np.sum(np.abs(xm))
                    out["scalex"][s, t, c] = float(sx)
                    out["eboundx"][s, t, c] = float(np.sum(np.abs(xm) * eb[mask]) / sx) if sx > 0 else 0.0
        return out

    def conditioning(self, slabs):
        """max over slabs, dates and both directions of |m0(u +- 1 ulp) - m0| / scale."""
        worst = 0.0
        for t in range(self.T):
            mb = self.mass_ld(t)
            for sh in (+1, -1):
                ms = self.mass_ld(t, sh)
                for a, b in slabs:
                    mask = self.inner_mask(a, b)
                    worst = max(worst, float(np.abs(np.sum(ms[mask]) - np.sum(mb[mask])) / np.sum(np.abs(mb[mask]))))
        return worst


def mp_mass(P, t, idx):
    """The mass of date t at the node indices idx (a list of index tuples), mpmath at 50 digits from
    the same float64 u, sigma and Delta-weights."""
    import mpmath as mp
    mp.mp.dps = 50
    d, th = P.dim, mp.mpf(P.theta)
    u = P._u[t]
    W = P.delta_weights(t)
    out = []
    for ix in idx:
        ls, lxs, lps = [], [], mp.mpf(0)
        for c, i in enumerate(ix):
            uc = mp.mpf(float(u[c, i]))
            l = mp.log1p(-uc) if P.survival else mp.log(uc)
            ls.append(l)
            lxs.append(mp.log(-l))
            if P.model != "msm":
                s = mp.mpf(float(P.sigma[t, c]))
                xs = mp.mpf(float(P.x[i])) / s
                lps += -xs * xs / 2 - mp.log(mp.sqrt(2 * mp.pi) * s)
        S = sum(mp.exp(th * v) for v in lxs)
        lA = mp.log(S) / th
        A = mp.exp(lA)
        poly = A + (th - 1) if d == 2 else A * A + 3 * (th - 1) * A + (th - 1) * (2 * th - 1)
        lc = -A - sum(ls) + (th - 1) * sum(lxs) + (1 - d * th) * lA + mp.log(poly)
        out.append(mp.exp(lc + lps) * mp.mpf(float(W[ix])))
    return out
