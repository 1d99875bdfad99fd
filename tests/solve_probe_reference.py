"""Longdouble truth of the solve's whole decision chain, and the probes built on it.

For one date of a NodeProblem (tests/node_reference.py; the Gumbel kinds: gumbel_node_reference.py) this
restates the reference's chain -- oracle/quadrature.py calc_var with Q1 and Q3, the form every solve kernel
follows (cvq_quad_kernels.h k_solve_prefix states it most plainly) -- with every slab summed in longdouble
over mass_ld(t).  Membership is the oracle's exact float64 inner_mask; mids are (lo + hi) / 2 in float64, as
the device forms them; K is snap_stride - 1 (solve_probe_cases.snap_K).

  (i)   r0 = S(lower, fg]
  (ii)  second slab: (sg0, fg] if r0 >= obj else (fg, sg1];  F = r0 - slab | r0 + slab
  (iii) bracket (k_compact's order): 0 (vmin, sg0] if F > obj and the slab ended at fg; 1 (sg0, fg] if F < obj
        there; 2 (sg1, vmax] if F < obj and it ended at sg1; 3 (fg, sg1] if F > obj there; F == obj: NaN (Q3)
  (iv)  K levels of prev +- S(lo, mid] | S(mid, hi] with the prev_upper rule (adjust_integral, Q1)

A solve with obj_var = F_true(target) + s * offset is a comparator: its decisions say on which side of the truth
the device's own F at the target lies.  The probe's expected result is the whole truth path under that
obj_var, K + 1 mids.  Its plateau key is the number of member nodes of (lower, mid]: the nodes are ordered
by their thresholds v*, so two mids with the same count have the same F in exact arithmetic (the chain's
longdouble values still differ at 1e-20: keys are compared, never F values).  A probe is unambiguous when every
fixed decision other than its target lies at least 2 offset from obj' and every level of the path either has
the target's key or an F at least 3 offset from the target's: then a device whose F is within the offset of
the truth everywhere must reproduce the path bit for bit, and one that is off by more at the target cannot.

offset = bar * M (+ PREFIX's running-sum term), M = |r0| + |second slab| + sum |mass| over the bracket.
"""
import numpy as np

import solve_probe_cases as SC

LD = np.longdouble
U53 = 2.0 ** -53


class Geometry:
    """Member nodes of (a, b] as flat indices into the box: the oracle's inner_mask, cached (it depends on the
    grid and the weights only, not on the date)."""

    def __init__(self, P):
        self.P = P
        self._idx = {}

    def idx(self, a, b):
        key = (float(a), float(b))
        if key not in self._idx:
            m = self.P.inner_mask(key[0], key[1])
            self._idx[key] = np.flatnonzero(np.broadcast_to(m, (self.P.n,) * self.P.dim)).astype(np.int32)
        return self._idx[key]

    def count(self, a, b):
        return int(self.idx(a, b).size)


def vstar(x, w0, w1):
    """cvq_plan.hip vstar_exact on the 2-D box: v*[r, j], the smallest double v with x_j <= (v - x_r w1) / w0."""
    lev = (x * w1)[:, None]
    xj = x[None, :]
    v = xj * w0 + lev
    for _ in range(64):
        v = np.where(xj <= (v - lev) / w0, v, np.nextafter(v, np.inf))
    for _ in range(64):
        d = np.nextafter(v, -np.inf)
        v = np.where(xj <= (d - lev) / w0, d, v)
    ok = (xj <= (v - lev) / w0) & ~(xj <= (np.nextafter(v, -np.inf) - lev) / w0)
    for r, j in np.argwhere(~ok):
        # cancellation near 0 (x_j w0 = -lev_r: v* is about -ulp(lev) / 2, far below the start's ulp): bisection
        # over the ordered doubles, as vstar_exact's
        def o2d(k):                                  # ordered integer -> double: sign * the double with bits |k|
            d = np.array([abs(k)], dtype=np.int64).view(np.float64)[0]
            return d if k >= 0 else -d
        lo_k, hi_k = -0x7FF0000000000000, 0x7FF0000000000000          # -inf: false, +inf: true
        while hi_k - lo_k > 1:
            m = (lo_k + hi_k) // 2
            if x[j] <= (o2d(m) - lev[r, 0]) / w0:
                hi_k = m
            else:
                lo_k = m
        v[r, j] = o2d(hi_k)
    assert np.all(xj <= (v - lev) / w0) and not np.any(xj <= (np.nextafter(v, -np.inf) - lev) / w0)
    return v


class Chain:
    """The chain of one date over one mass array (flat, any float type: longdouble is the truth, float64 the
    CPU restatement the mutations are applied to)."""

    def __init__(self, geo, mass, args):
        self.geo, self.m, self.a = geo, np.ravel(mass), args
        self.absm = np.abs(self.m)
        self.K = SC.snap_K(args)
        self._sum = {}

    def S(self, a, b):
        key = (float(a), float(b))
        if key not in self._sum:
            self._sum[key] = np.sum(self.m[self.geo.idx(a, b)])
        return self._sum[key]

    def Sabs(self, a, b):
        return np.sum(self.absm[self.geo.idx(a, b)])

    def run(self, obj):
        """dict: r0, slab2, F (stage iii), bracket (-1: Q3), mids (K + 1), Fl (K,) the levels' F, count (K,)
        their plateau keys, bits, M."""
        a, K = self.a, self.K
        fg, (sg0, sg1), lower = a["first_guess"], a["second_guess"], a["lower"]
        obj = np.float64(obj)
        r0 = self.S(lower, fg)
        nl = sg0 if r0 >= obj else fg
        nu = sg1 if r0 < obj else fg
        prevU = sg0 if nl == sg0 else fg
        nr = self.S(nl, nu)
        F = r0 + nr if nl == fg else r0 - nr
        br = -1
        if F > obj:
            br = 0
        if F < obj and nu == fg:
            br = 1
        if F < obj and nu == sg1:
            br = 2
        if F > obj and nu == sg1:
            br = 3
        out = dict(r0=r0, slab2=nr, F=F, bracket=br, count_r0=self.geo.count(lower, fg), count_F=self.geo.count(lower, nl if nl != fg else nu))
        if br < 0:
            return out
        lo, hi = SC.brackets(a)[br]
        out["M"] = float(abs(r0) + abs(nr) + self.Sabs(lo, hi))
        out["top"] = max(fg, sg1, hi)
        ustack = not (hi == sg0 or hi == sg1)
        mids, Fl, cnt, bits = np.empty(K + 1), [], [], 0
        prev = F
        for k in range(K):
            mid = (lo + hi) / 2
            mids[k] = mid
            val = self.S(lo, mid) if ustack else self.S(mid, hi)
            slab_lower = lo if ustack else mid
            Fn = prev + val if slab_lower == prevU else prev - val
            Fl.append(Fn)
            cnt.append(self.geo.count(lower, mid))
            ustack = bool(Fn < obj)
            if ustack:
                lo = mid
                bits |= 1 << k
            else:
                hi = mid
            prev, prevU = Fn, mid
        mids[K] = (lo + hi) / 2
        out.update(mids=mids, Fl=Fl, count=cnt, bits=bits)
        return out


def prefix_extra(chain, path, n):
    """PREFIX's own term: a slab is a difference of two running row sums of n sequential additions each, so it
    rounds against everything at or below the highest level the path can touch."""
    return 2 * n * U53 * float(chain.Sabs(chain.a["lower"], path["top"]))


def edge_paths(chain, depth):
    """[(level, path, node just above?)]: truth paths that visit, at a level above the tail (< depth), a mid with a node threshold
    within q = bracket width 2^-K on either side.  Such a mid is an edge of the tail cells below it, and a probe
    on its plateau ends in a block tail whose remaining mids all decide the same way: below a node at or just
    under the edge (sign -) every one moves the lower end up, above a node just over it (sign +) none does --
    the ends of the tail's crossing searches.  The grids put points at exactly -5, -2.5, -1, 1, 2.5 and 5, so
    with equal weights thresholds land on dyadic mids (-2, -1, 0) or an ulp off them."""
    a, geo, out = chain.a, chain.geo, []
    for b, (lo0, hi0) in enumerate(SC.brackets(a)):
        q = np.ldexp(hi0 - lo0, -chain.K)
        cells = [(lo0, hi0)]
        for k in range(depth):
            nxt = []
            for lo, hi in cells:
                m = (lo + hi) / 2
                nxt += [(lo, m), (m, hi)]
                below, above = geo.count(m - q, m), geo.count(m, m + q)
                if below == 0 and above == 0:
                    continue
                p = chain.run(np.float64(chain.S(a["lower"], m)))
                if p["bracket"] == b and p["mids"][k] == m:
                    out.append((k, p, above > 0))
            cells = nxt
    return out


def candidate_targets(chain, base_objs, limit, edge_depth=0, hard_limit=32):
    """[(kind, level, F_target, count, base path)] of one date: the r0 decision, the stage-(iii) decision on
    each F the base paths meet, the tail-cell edges with a node within q (edge_paths: always kept), and the base
    paths' levels, deduplicated by plateau key, the levels thinned evenly (in level order, round-robin over the
    base paths) so that fixed decisions and thinned levels are at most `limit`, and all at most `hard_limit`."""
    paths = [chain.run(o) for o in base_objs]
    paths = [p for p in paths if p["bracket"] >= 0]
    out, seen = [], set()

    def add(kind, level, F, count, p):
        if (kind == "level" and ("level", p["bracket"], count) in seen) or (kind != "level" and (kind, count) in seen):
            return
        seen.add(("level", p["bracket"], count) if kind == "level" else (kind, count))
        out.append((kind, level, F, count, p))

    add("r0", -1, paths[0]["r0"], paths[0]["count_r0"], paths[0])
    for p in paths:
        add("F", -1, p["F"], p["count_F"], p)
    fixed, out = out, []
    # edges with a node just above them first (the rarer kind: thresholds an ulp over a dyadic mid), then the
    # others, thinned evenly to what is left of the hard limit
    ep = edge_paths(chain, edge_depth)
    for k, p, _ in [e for e in ep if e[2]]:
        add("level", k, p["Fl"][k], p["count"][k], p)
    rest = [e for e in ep if not e[2]]
    room = max(hard_limit - limit - len(out), 0)
    if len(rest) > room:
        rest = [rest[i] for i in sorted(set(np.rint(np.linspace(0, len(rest) - 1, room)).astype(int).tolist()))] if room else []
    for k, p, _ in rest:
        add("level", k, p["Fl"][k], p["count"][k], p)
    edges, out = out, []
    for k in range(chain.K):
        for p in paths:
            add("level", k, p["Fl"][k], p["count"][k], p)
    # the levels' share of the limit, spread evenly over every level the paths have a plateau of their own at
    # (shallow levels hold one plateau per path, the deepest few: the block tails' own)
    m = max(limit - len(fixed), 0)
    if len(out) > m:
        out = [out[i] for i in sorted(set(np.rint(np.linspace(0, len(out) - 1, m)).astype(int).tolist()))]
    out = (fixed + out)[:limit] + edges
    return out[:hard_limit], paths


def make_probe(chain, target, sign, bar, n, prefix=False, ebound=None):
    """(record | None, reason): the probe of one target, sign and bar; None where it is ambiguous or skipped.
    ebound(path): an extra relative term of the bar that depends on the path's sets (the Gumbel kinds)."""
    kind, level, Ft, count, base = target

    def offset_of(path):
        b = bar + (ebound(path) if ebound is not None else 0.0)
        return b * path["M"] + (prefix_extra(chain, path, n) if prefix else 0.0), b

    off, _ = offset_of(base)
    if not (Ft >= 3 * off):
        return None, "small"
    trial = chain.run(np.float64(Ft + sign * LD(off)))
    if trial["bracket"] < 0:
        return None, "ambiguous"
    off, b = offset_of(trial)
    if not (Ft >= 3 * off):
        return None, "small"
    obj = np.float64(Ft + sign * LD(off))
    p = chain.run(obj)
    if p["bracket"] < 0 or offset_of(p)[0] != off:
        return None, "ambiguous"
    # fixed decisions: on the target's plateau (then they are the target: exactly one offset away), or
    # at least two offsets from obj'
    hit = False
    for c, v in ((p["count_r0"], p["r0"]), (p["count_F"], p["F"])):
        if c == count:
            hit = True
        elif not abs(v - LD(obj)) >= 2 * off:
            return None, "ambiguous"
    if kind != "level" and not hit:
        return None, "ambiguous"
    for k in range(chain.K):
        if p["count"][k] == count:
            hit = True
        elif not abs(p["Fl"][k] - Ft) >= 3 * off:
            return None, "ambiguous"
    if not hit:
        return None, "ambiguous"                     # the path under obj' no longer visits the target's plateau
    return dict(kind=SC.KINDS.index(kind), level=level, sign=sign, bracket=p["bracket"], bits=p["bits"], obj=float(obj),
                offset=off, count=count, bar=b), ""


def follows(chain, rec):
    """Does `chain` (any mass type) reproduce the probe's path?  The bracket and all K decisions."""
    p = chain.run(rec["obj"])
    return p["bracket"] == int(rec["bracket"]) and p["bits"] == int(rec["bits"])
