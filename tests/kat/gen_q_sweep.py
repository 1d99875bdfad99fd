"""Writes tests/golden/q_sweep.kat (an .npz container; tests/q_sweep_cases.py KAT_PATH), the fixture of the
q sweep: every MSM kernel family at q = 1 ... 8 unique volatility states per asset.  node_kat.kat is read only
to cross-check q = 3; nothing else is written.  Run from the repository root on a CPU machine with mpmath:

    python tests/kat/gen_q_sweep.py

Contents (C = len(q_sweep_cases.cases()), S = 4 slabs, T = 3 dates):
  MSM inputs     msm<dim>_q<q>_fbs / _pi / _uvs, dim 2 and 3, q = 1 ... 8 (q_sweep_cases' header: the recipe)
  sha_case       (C,) SHA-256 of every case's inputs (q_sweep_cases.case_digest)
  slab truths    m0, m1, scale, scale1, scale_below, count (C, S, T); mx, scalex (C, S, T, 3); ebound, ebound1,
                 ebound_fast (C, S, T), eboundx (C, S, T, 3): gen_node_kat_ext.py's slab_rows (the bounds 0
                 outside the Gumbel kind).  From the kind's high-precision checker: node_reference.NodeProblem
                 (Student, Gaussian, Plackett), gumbel_node_reference.GumbelNodeProblem (survival Gumbel),
                 archimedean_reference's product form kept in longdouble up to the sums (Frank, survival Joe)
  event          axis 0's stress event of node_cases.events: m0_event, scale_event, ebound_event, count_event
                 (C, S, T); p_event, scale_pevent, ebound_pevent (C, T) -- gen_node_kat_ext.py's event_rows
  candidate      node_cases.PORT_UNEQUAL[dim]: m0_port, scale_port, ebound_port, count_port (C, S, T)
  alternative    the middle date under q_sweep_cases.alt_params and the candidate as its weights: alt_m0, alt_m1,
                 alt_scale, alt_scale1, alt_ebound, alt_ebound1, alt_count (C, S)
  solve          solve_var (C, T), solve_it (C,): the float64 oracle's calc_var at ptf_mean = 0 and obj_var =
                 q_sweep_cases.OBJ_VAR[dim] on the cases of q_sweep_cases.solve_case (NaN / -1 elsewhere)
Sums and scales are float64 roundings of longdouble sums; the bounds are kept as float32 (they only size a
tolerance).  tests/test_q_sweep_cpu.py regenerates a sample of every part and requires equality."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "copula-msm-and-copula-garch-var_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import node_cases as NC                  # noqa: E402
import q_sweep_cases as QC               # noqa: E402
import node_reference as NR              # noqa: E402
import gumbel_node_reference as GR       # noqa: E402
import archimedean_reference as AR       # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_node_kat_ext", NC.EXT_GEN_PATH)
EXT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(EXT)

LD = np.longdouble
F32 = ("ebound", "ebound1", "ebound_fast", "eboundx", "ebound_event", "ebound_pevent", "ebound_port", "alt_ebound",
       "alt_ebound1")
SLAB_KEYS = ("m0", "m1", "scale", "scale1", "scale_below", "count", "mx", "scalex", "ebound", "ebound1", "ebound_fast",
             "eboundx")


class ProductNodeProblem(AR.ArchimedeanProblem):
    """ArchimedeanProblem whose node masses stay in longdouble up to the slab sums (its own mass(t) rounds
    every node to float64), with NodeProblem's slab interface.  Regular regime only, asserted."""
    levels_ld = NR.NodeProblem.levels_ld
    slab_moments = NR.NodeProblem.slab_moments

    def mass_ld(self, t, ulp_shift=0):
        assert ulp_shift == 0 and self.model == "msm"
        u, _ = self.axis_cdf(t)
        assert np.all((u > 0.0) & (u < 1.0)), "regular regime: every u strictly inside (0, 1)"
        a, B = AR.axis_terms(self.copula, self.theta, u)
        S = sum(self._broadcast(a))
        sumB = sum(self._broadcast(B))
        m = np.exp(AR.node_log(self.copula, self.theta, self.dim, S, sumB)) * self.delta_weights(t).astype(LD)
        assert np.all(np.isfinite(m)), "regular regime: every node mass finite"
        return m


def msm_inputs(dim, q):
    """gen_node_kat.msm_inputs' recipe at k = q - 1 components (q >= 2); q = 1: k = 2 with every m_0 = 1."""
    from copula_var import synthetic
    from oracle import forecast as F
    k = q - 1 if q >= 2 else 2
    c = synthetic.baseline_configs()[2 if dim == 2 else 4].with_(T=NC.T, num_points=NC.N_OF[dim], k=k)
    rets = synthetic.simulate_returns(c)
    _, _, windows = F.insample_split(rets[:c.n_in + NC.T], c.n_in, c.weights)
    params = c.msm_params if q >= 2 else [dict(p, m_0=1.0) for p in c.msm_params]
    m = F.msm_integration_params(windows, params, k, c.num_points)
    assert m["unique_vol_states"].shape == (dim, q), (dim, q, m["unique_vol_states"].shape)
    return m["forecasts_by_states"], m["forecasts"], m["unique_vol_states"]


_ZTABS = {}


def build_problem(case, z, alt=False):
    """The high-precision problem of a case (alt: its alternative middle date alone, T = 1)."""
    copula, dim, params, q, variant = case
    kw = QC.problem_inputs(case, z, alt)
    args = (kw["model"], kw["copula"], kw["dim"], kw["x_values"], kw["step"], kw["densities"], kw["combos"],
            kw["weights"], kw["copula_params"], kw["per_date"], kw["unique_vol_states"])
    if copula in QC.GUMBEL_KINDS:
        return GR.GumbelNodeProblem(*args)
    if copula in QC.PRODUCT_KINDS:
        return ProductNodeProblem(*args)
    if copula == "plackett":
        return NR.NodeProblem(*args)
    # the quantile tables depend on the filter outputs' u and, for Student, nu: neither on the correlations
    # nor on pi_t (the "nr1" variant) nor on the weights
    key = (dim, q, params[0] if copula == "student" else None)
    if key not in _ZTABS:
        base = QC.problem_inputs(case, z)
        P = NR.NodeProblem(base["model"], copula, dim, base["x_values"], base["step"], base["densities"], base["combos"],
                           base["weights"], base["copula_params"], base["per_date"], base["unique_vol_states"])
        _ZTABS[key] = P.quantile_tables()
    zt = _ZTABS[key]
    return NR.NodeProblem(*args, z=zt[QC.ALT_DATE:QC.ALT_DATE + 1] if alt else zt)


def event_rows(P, dim):
    """gen_node_kat_ext.event_rows, axis 0's stress event alone."""
    r = EXT.event_rows(P, dim)
    out = {k: r[k][:, 0, 0, :] for k in ("m0_event", "scale_event", "ebound_event", "count_event")}
    out.update({k: r[k][0, 0, :] for k in ("p_event", "scale_pevent", "ebound_pevent")})
    return out


def port_rows(P, dim):
    """gen_node_kat_ext.port_rows' sums for the one candidate node_cases.PORT_UNEQUAL[dim]."""
    slabs, T = NC.slabs(dim), P.T
    o = dict(m0_port=np.zeros((4, T)), scale_port=np.zeros((4, T)), ebound_port=np.zeros((4, T)),
             count_port=np.zeros((4, T), dtype=np.int16))
    Pw = EXT.with_weights(P, NC.PORT_UNEQUAL[dim])
    for t in range(T):
        mass, eb = P.mass_ld(t), EXT._bounds(P, t)
        for s, (a, b) in enumerate(slabs):
            o["m0_port"][s, t], o["scale_port"][s, t], o["ebound_port"][s, t], o["count_port"][s, t] = \
                EXT._sums(mass, eb, Pw.inner_mask(a, b))
    return o


def alt_rows(case, z):
    P = build_problem(case, z, alt=True)
    assert P.T == 1
    r = EXT.slab_rows(P, case[1])
    return {"alt_" + k: r[k][:, 0] for k in ("m0", "m1", "scale", "scale1", "ebound", "ebound1", "count")}


def oracle_problem(case, z):
    """The float64 checker of a case: oracle.quadrature.Problem, gumbel_reference.GumbelProblem or
    archimedean_reference.ArchimedeanProblem."""
    from oracle.quadrature import Problem
    from gumbel_reference import GumbelProblem
    kw = QC.problem_inputs(case, z)
    cls = GumbelProblem if case[0] in QC.GUMBEL_KINDS else (AR.ArchimedeanProblem if case[0] in QC.PRODUCT_KINDS else Problem)
    return cls(kw["model"], kw["copula"], kw["dim"], kw["x_values"], kw["step"], kw["densities"], kw["combos"],
               kw["weights"], kw["copula_params"], kw["per_date"], kw["unique_vol_states"])


def solve_rows(case, z):
    """(var (T,), iterations) of the oracle's calc_var at ptf_mean = 0 and the dimension's target (NaN, -1
    outside solve_case)."""
    from oracle.quadrature import calc_var
    if not QC.solve_case(case):
        return np.full(NC.T, np.nan), -1
    P = oracle_problem(case, z)
    var, it, _ = calc_var(P.compute_integral, P.T, 0.0, obj_var=QC.OBJ_VAR[case[1]])
    return var, it


def case_rows(case, z):
    """Every per-case array of the fixture but the digest."""
    dim = case[1]
    P = build_problem(case, z)
    rows = dict(EXT.slab_rows(P, dim))
    assert set(rows) == set(SLAB_KEYS)
    rows.update(event_rows(P, dim))
    rows.update(port_rows(P, dim))
    rows.update(alt_rows(case, z))
    var, it = solve_rows(case, z)
    rows.update(solve_var=var, solve_it=np.array(it, dtype=np.int16))
    return {k: cast(k, np.asarray(a)) for k, a in rows.items()}


def cast(name, a):
    return a.astype(np.float32) if name in F32 else (a.astype(np.int16) if "count" in name else a)


def main():
    kat = NC.load_kat()
    out = {}
    for dim in (2, 3):
        for q in QC.QS:
            k = QC.msm_key(dim, q)
            out[k + "_fbs"], out[k + "_pi"], out[k + "_uvs"] = msm_inputs(dim, q)
        for s in ("_fbs", "_pi", "_uvs"):
            assert np.array_equal(out[QC.msm_key(dim, 3) + s], kat["msm%d" % dim + s]), "q = 3 is node_kat.kat's own"
    cases = QC.cases()
    rows, sha = {}, []
    for i, case in enumerate(cases):
        sha.append(QC.case_digest(case, out))
        for k, a in case_rows(case, out).items():
            if k not in rows:
                rows[k] = np.zeros((len(cases),) + a.shape, dtype=a.dtype)
            rows[k][i] = a
        print(i, QC.case_id(case), "narrow slab members", rows["count"][i, 3].tolist(), "alt", int(rows["alt_count"][i, 3]),
              "solve", int(rows["solve_it"][i]), flush=True)
    out.update(rows)
    out["sha_case"] = np.array(sha)
    with open(QC.KAT_PATH, "wb") as f:              # (a file object: savez appends no ".npz")
        np.savez_compressed(f, **out)
    print("wrote", QC.KAT_PATH, os.path.getsize(QC.KAT_PATH), "bytes")


if __name__ == "__main__":
    main()
