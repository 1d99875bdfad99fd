"""Longdouble truth of the exact quantile solve's decisions, and the level probes built on it.

For one date this restates tests/quantile_reference.py's definition (conditional_reference.py's with an event)
over mass_ld(t) of a NodeProblem / GumbelNodeProblem, under the oracle's exact float64 membership (inner_mask,
through solve_probe_reference.Geometry):

  F(v)      longdouble sum over the members of (lower, v] (within the event: s_lo < x[i_axis] <= s_hi)
  target    alpha (conditional: alpha p_E, p_E the longdouble mass of the event over the box)
  bracket   F(min_var) < target <= F(max_var), else var = es = NaN and m0 = F(max_var)
  K         bisection_steps(min_var, max_var, tolerance) decisions, mid = (lo + hi) / 2 in float64 exactly as
            quant_cuts forms it; lo = mid if F(mid) < target else hi = mid
  closing   cut = ((lo + hi) / 2 + ptf_mean) - ptf_mean in float64, as k_quant_update writes it; m0 and m1 over
            (lower, cut], es = m1 / m0 + ptf_mean; scales sum |mass| and sum |level mass| of the same set

A call with alpha' = F_true(target) + sign * offset is a comparator on the device's own F at the target: its
var encodes the bracket test and all K decisions.  A target's plateau key is the member count of (lower, target]:
the nodes are ordered by their thresholds, so two points with the same count have the same F in exact
arithmetic (keys are compared, never F values).  A probe is unambiguous when every other evaluated point
(min_var, max_var, every mid of the path under alpha') either has the target's key or an F at least 3 offsets
from the target level: then a device whose F is within one offset of the truth everywhere must return the truth
path's var bit for bit, and one that is off by more than the offset at the target, on the probe's side, cannot.

offset = bar M, M = sum |mass| over (lower, max_var] (within the event).  The chain's own additions (at most 12
per F, each at most 2^-53 M, 1.3e-15 M together) sit inside the bar's 1e-12.  Conditional adds the first-order
term of the target product: alpha' bar sum_E |mass| + 2^-53 alpha' p_E.
"""
import numpy as np

import quantile_probe_cases as QC

LD = np.longdouble
U53 = 2.0 ** -53
NUDGE = 1e-12                                 # far above a threshold's rounding, far below 2^-25 of a bracket


class Measure:
    """One date's member sets and sums: geo (solve_probe_reference.Geometry of the problem whose weights decide
    membership), flat masses of any float type (longdouble: the truth; float64: the CPU restatement the
    mutations are applied to), flat levels, and an optional flat event mask."""

    def __init__(self, geo, mass, levels, lower, event=None, ebound=None):
        self.geo, self.lower = geo, float(lower)
        self.m = np.ravel(mass)
        self.absm = np.abs(self.m)
        self.lev = np.ravel(np.broadcast_to(levels, np.shape(mass)))
        self.ev = None if event is None else np.ravel(np.broadcast_to(event, np.shape(mass)))
        self.eb = None if ebound is None else np.ravel(ebound).astype(LD)
        self._F = {}
        if len(geo._idx) > 400:                   # (the member lists of one date's mids are of no use to the next)
            geo._idx.clear()

    def idx(self, v):
        i = self.geo.idx(self.lower, v)
        return i if self.ev is None else i[self.ev[i]]

    def F(self, v):
        """(F(v), plateau key)."""
        key = float(v)
        if key not in self._F:
            i = self.idx(key)
            self._F[key] = (np.sum(self.m[i]), int(i.size))
        return self._F[key]

    def scale(self, v):
        return np.sum(self.absm[self.idx(v)])

    def ebound(self, v):
        """The Gumbel kinds' first-order bound, |mass|-weighted over the members of (lower, v]."""
        if self.eb is None:
            return 0.0
        i = self.idx(v)
        return float(np.sum(self.absm[i] * self.eb[i]) / np.sum(self.absm[i]))

    def event_mass(self):
        """(p_E, sum_E |mass|): the event over the whole box, conditional_reference's F_E(+inf)."""
        i = self.idx(np.inf)
        return np.sum(self.m[i]), np.sum(self.absm[i])

    def closing(self, cut):
        """(m0, m1, sum |mass|, sum |level mass|) over (lower, cut]."""
        i = self.idx(cut)
        lm = self.lev[i] * self.m[i]
        return np.sum(self.m[i]), np.sum(lm), np.sum(self.absm[i]), np.sum(np.abs(lm))

    def neighbours(self, v):
        """(F of the next plateau below, F of the next plateau above) the plateau of v (None where there is none
        inside (lower, +inf)): the levels w . x of the nodes order them up to a threshold's rounding, so the
        nearest levels on either side, nudged, are points on the neighbouring plateaus."""
        box = self.idx(np.inf)
        lev = self.lev[box].astype(np.float64)
        inside = np.zeros(self.m.size, dtype=bool)
        inside[self.idx(v)] = True
        isin = inside[box]
        below = self.F(np.max(lev[isin]) - NUDGE)[0] if np.any(isin) else None
        above = self.F(np.min(lev[~isin]) + NUDGE)[0] if np.any(~isin) else None
        return below, above


class Path:
    """The definition's run of one date under one target level."""

    def __init__(self, meas, a, K, target):
        lo, hi = float(a["min_var"]), float(a["max_var"])
        f_lo, f_hi = meas.F(lo), meas.F(hi)
        self.points = [(lo, f_lo[0], f_lo[1]), (hi, f_hi[0], f_hi[1])]      # every evaluated (v, F, key)
        self.nan = not (f_lo[0] < target and target <= f_hi[0])
        self.bits, self.mids = 0, []
        if not self.nan:
            for k in range(K):
                mid = (lo + hi) / 2
                f, c = meas.F(mid)
                self.points.append((mid, f, c))
                self.mids.append(mid)
                if f < target:
                    lo = mid
                    self.bits |= 1 << k
                else:
                    hi = mid
        self.var_mid = float("nan") if self.nan else (lo + hi) / 2
        self.top = float(a["max_var"])

    def closing(self, meas, ptf_mean):
        """dict m0, es, scale0, scale1 (longdouble): outside the bracket m0 = F(max_var), es NaN."""
        if self.nan:
            m0 = self.points[1][1]
            return dict(m0=m0, es=LD("nan"), scale0=meas.scale(self.top), scale1=LD(0))
        cut = (self.var_mid + ptf_mean) - ptf_mean
        m0, m1, s0, s1 = meas.closing(cut)
        # (an empty closing set: m0 = 0 and no es, as k_quant_finish leaves it)
        return dict(m0=m0, es=m1 / m0 + LD(ptf_mean) if m0 != 0 else LD("nan"), scale0=s0, scale1=s1)


class DateTruth:
    """A date's measure with its arguments, event mass and bar."""

    def __init__(self, meas, a, K, bar_fn, conditional=False):
        self.meas, self.a, self.K, self.cond = meas, a, K, conditional
        self.M = meas.scale(a["max_var"])
        self.bar = bar_fn(meas.ebound(a["max_var"]))
        if conditional:
            self.pE, self.scaleE = meas.event_mass()
            self.bar_e = bar_fn(meas.ebound(np.inf))
        else:
            self.pE, self.scaleE, self.bar_e = LD(1), LD(0), 0.0

    def target_of(self, alpha):
        return LD(np.float64(alpha)) * self.pE if self.cond else LD(np.float64(alpha))

    def path(self, alpha):
        return Path(self.meas, self.a, self.K, self.target_of(alpha))

    def offset(self, alpha_up):
        off = LD(self.bar) * self.M
        if self.cond:
            off = off + LD(alpha_up) * (LD(self.bar_e) * self.scaleE + LD(U53) * self.pE)
        return off


def candidate_targets(D, fractions, limit, edge_limit, edge_depth=6):
    """[(kind, level, v)]: the two bracket decisions, the mids of the truth paths of the base levels (fractions
    of the date's own F_true(max_var)), deduplicated by plateau key and thinned evenly in level order to `limit`
    in all, and on top at most `edge_limit` edge targets: mids of the first `edge_depth` levels with a node
    threshold within 2^-K of the bracket on either side (the later decisions of a probe there all go one way)."""
    a, meas = D.a, D.meas
    f_top = meas.F(a["max_var"])[0]
    bases = [float(np.float64(LD(f) * f_top / D.pE)) for f in fractions]
    seen, levels = set(), []
    paths = [D.path(b) for b in bases]
    for k in range(D.K):
        for p in paths:
            if not p.nan:
                key = p.points[2 + k][2]
                if key not in seen:
                    seen.add(key)
                    levels.append(("level", k, p.mids[k]))
    m = max(limit - 2, 0)
    if len(levels) > m:
        levels = [levels[i] for i in sorted(set(np.rint(np.linspace(0, len(levels) - 1, m)).astype(int).tolist()))] if m else []
    out = [("min", -1, float(a["min_var"])), ("max", -1, float(a["max_var"]))] + levels
    # edges
    box = meas.idx(np.inf)
    lev = np.sort(meas.lev[box].astype(np.float64))
    q = np.ldexp(float(a["max_var"]) - float(a["min_var"]), -D.K)
    edges, cells = [], [(float(a["min_var"]), float(a["max_var"]))]
    for k in range(min(edge_depth, D.K)):
        nxt = []
        for lo, hi in cells:
            mid = (lo + hi) / 2
            nxt += [(lo, mid), (mid, hi)]
            i0, i1, i2 = np.searchsorted(lev, [mid - q, mid, mid + q], side="right")
            key = meas.F(mid)[1]
            if (i1 > i0 or i2 > i1) and 0 < key and ("e", key) not in seen:
                seen.add(("e", key))
                edges.append(("level", k, mid))
        cells = nxt
    if len(edges) > edge_limit:
        edges = [edges[i] for i in sorted(set(np.rint(np.linspace(0, len(edges) - 1, edge_limit)).astype(int).tolist()))] if edge_limit else []
    return out + edges, bases


def make_probe(D, target, sign):
    """(record | None, reason): None with "small" where the probe is skipped (alpha' <= 0, or the next plateau on
    either side is under 3 offsets away) and with "ambiguous" where another evaluated point comes within 3 offsets."""
    kind, level, v = target
    meas = D.meas
    Ft, count = meas.F(v)
    off = D.offset((Ft + LD(D.bar) * D.M) / D.pE * (1 + LD(1e-9)))
    alpha = np.float64((Ft + sign * off) / D.pE)
    if not (alpha > 0.0 and np.isfinite(alpha)):
        return None, "small"
    below, above = meas.neighbours(v)
    if (below is not None and not Ft - below >= 3 * off) or (above is not None and not above - Ft >= 3 * off):
        return None, "small"
    tgt = D.target_of(alpha)
    p = D.path(alpha)
    hit = False
    for pv, f, c in p.points:
        if c == count:
            hit = True
        elif not abs(f - tgt) >= 3 * off:
            return None, "ambiguous"
    if not hit:
        return None, "ambiguous"                     # the path under alpha' no longer visits the target's plateau
    cl = p.closing(meas, D.a["ptf_mean"])
    rec = dict(kind=QC.KINDS.index(kind), level=level, sign=sign, nan=int(p.nan), bits=p.bits, alpha=float(alpha),
               offset=float(off), count=count)
    for k in ("m0", "es"):
        hi = np.float64(cl[k])
        rec[k + "_hi"] = hi
        rec[k + "_lo"] = float((cl[k] - LD(hi)) / LD(hi)) if np.isfinite(hi) and hi != 0.0 else 0.0
    rec["scale0"], rec["scale1"] = float(cl["scale0"]), float(cl["scale1"])
    return rec, ""


def follows(D, rec):
    """Does D's measure (any mass type) reproduce the probe's decisions?"""
    p = D.path(rec["alpha"])
    return int(p.nan) == int(rec["nan"]) and p.bits == int(rec["bits"])
