"""cvq_dynamic_distribution without a GPU: the symbol is declared, exported and bound, its
host-side argument checks return their codes before any device work, the engine and
copula_var.backtest route and centre their ladders as documented (against stand-in objects that
record what they were handed), the parser takes the new flag combination, and the checker's view of
the shared cases (tests/dynamic_cases.py) is what the GPU tests rely on."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import distribution_reference as D
import dynamic_cases as DC
from conftest import REPO

HEADER = os.path.join(REPO, "include", "cvq.h")
INF = float("inf")
LADDER = np.array([-100.0, -7.5, -3.0, -2.0, -1.0, 0.0, 0.5, 2.0, INF])    # tests/test_distribution_gpu.py's


# ------------------------------------------------------------------ ABI
def test_symbol_is_declared_exported_and_bound():
    from copula_var import _native as N
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"int32_t\s+cvq_dynamic_distribution\s*\(([^)]*)\)", code)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["plan", "copula_params_t", "weights_t", "edges", "n_bins", "per_date", "mass_out", "m1_out", "mem"]
    assert hasattr(C.CDLL(N.LIB_PATH), "cvq_dynamic_distribution")
    assert '"cvq_dynamic_distribution"' in inspect.getsource(N._declare)
    lib = N.lib()
    assert len(lib.cvq_dynamic_distribution.argtypes) == 9 and lib.cvq_dynamic_distribution.restype is C.c_int32
    assert lib.cvq_version() == 10900                # the feature is detected by the symbol, not the version


def test_invalid_arguments_fail_on_the_host():
    """cvq_distribution's checks in its order (arguments first, the plan last), whatever the
    per-date arrays hold, without a device: the message says which check fired."""
    from copula_var import _native as N
    lib = N.lib()
    e, out = np.array([-100.0, -3.0, INF]), np.zeros(8)
    junk = np.full(8, np.nan)                        # per-date values are read after these checks
    err = lambda: (lib.cvq_last_error() or b"").decode()

    def call(plan, edges, nb, per, mass, m1=None, mem=N.MEM_HOST, cp=None, w=None):
        return lib.cvq_dynamic_distribution(plan, N.ptr(cp) if cp is not None else None,
                                            N.ptr(w) if w is not None else None,
                                            N.ptr(edges) if edges is not None else None, nb, per,
                                            N.ptr(mass) if mass is not None else None,
                                            N.ptr(m1) if m1 is not None else None, mem)

    for cp, w in ((None, None), (junk, junk)):
        assert call(None, None, 2, 0, out, cp=cp, w=w) == N.CVQ_ERR_INVALID and "NULL argument" in err()
        assert call(None, e, 2, 0, None, cp=cp, w=w) == N.CVQ_ERR_INVALID and "NULL argument" in err()
        for nb in (0, -1, N.MAX_BINS + 1, 2 ** 31 - 1):
            assert call(None, e, nb, 0, out, cp=cp, w=w) == N.CVQ_ERR_INVALID and "n_bins" in err(), nb
        for per in (-1, 2, 7):
            assert call(None, e, 2, per, out, cp=cp, w=w) == N.CVQ_ERR_INVALID and "per_date" in err(), per
        for mem in (N.MEM_HOST, N.MEM_DEVICE):       # everything else valid: the NULL plan is what is left
            assert call(None, e, 2, 0, out, out, mem, cp, w) == N.CVQ_ERR_INVALID and "plan is NULL" in err()
            assert call(None, e, N.MAX_BINS, 1, out, None, mem, cp, w) == N.CVQ_ERR_INVALID and "plan is NULL" in err()
    assert np.all(out == 0.0)


# ------------------------------------------------------------------ engine
class _StubLib:
    """cvq_dynamic_distribution that records its calls and fills mass = upper edge, m1 = lower edge."""

    def __init__(self, T, ncp, dim):
        self.T, self.ncp, self.dim, self.calls = T, ncp, dim, []

    def _arr(self, p, shape):
        if p is None:
            return None
        return np.array(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=shape))

    def cvq_dynamic_distribution(self, h, cp, w, edges, nb, per_date, mass, m1, mem):
        cols = nb + 1
        e = self._arr(edges, (self.T, cols) if per_date else (cols,))
        self.calls.append((nb, per_date, mem, e, self._arr(cp, (self.T, self.ncp)), self._arr(w, (self.T, self.dim))))
        ee = e if per_date else np.broadcast_to(e, (self.T, cols))
        np.ctypeslib.as_array(C.cast(mass, C.POINTER(C.c_double)), shape=(self.T, nb))[:] = ee[:, 1:]
        np.ctypeslib.as_array(C.cast(m1, C.POINTER(C.c_double)), shape=(self.T, nb))[:] = ee[:, :-1]
        return 0


def _stub_plan(T, ncp, dim):
    from copula_var.engine import QuadraturePlan
    p = object.__new__(QuadraturePlan)               # no device: only the fields dynamic_distribution() reads
    p.T, p._h, p.dim, p._cp = T, None, dim, np.zeros(ncp)
    return p


@pytest.mark.parametrize("B", [1, 64, 65, 150])
def test_engine_splits_more_than_max_bins(monkeypatch, B):
    from copula_var import _native as N
    T = 3
    stub = _StubLib(T, 2, 2)
    monkeypatch.setattr(N, "lib", lambda: stub)
    p = _stub_plan(T, 2, 2)
    cp, w = np.arange(6.0).reshape(3, 2), np.arange(6.0).reshape(3, 2) + 10.0
    shared = np.linspace(-7.0, 2.0, B + 1)
    mass, m1 = p.dynamic_distribution(shared, cp, w)
    assert mass.shape == m1.shape == (T, B)
    assert np.array_equal(mass, np.broadcast_to(shared[1:], (T, B))) and np.array_equal(m1[0], shared[:-1])
    sizes = [c[0] for c in stub.calls]
    assert sizes == [64] * (B // 64) + ([B % 64] if B % 64 else [])
    assert all(c[1] == 0 and c[2] == N.MEM_HOST for c in stub.calls)
    assert all(np.array_equal(c[4], cp) and np.array_equal(c[5], w) for c in stub.calls)   # every call, the same records
    at = 0
    for nb, _, _, e, _, _ in stub.calls:             # neighbouring calls share their boundary edge
        assert np.array_equal(e, shared[at:at + nb + 1])
        at += nb
    stub.calls.clear()
    per = shared[None, :] + np.arange(T)[:, None]    # a ladder of its own per date, nothing else per date
    mass, m1 = p.dynamic_distribution(per)
    assert np.array_equal(mass, per[:, 1:]) and np.array_equal(m1, per[:, :-1])
    assert [c[0] for c in stub.calls] == sizes and all(c[1] == 1 and c[4] is None and c[5] is None for c in stub.calls)


def test_engine_shape_rules(monkeypatch):
    from copula_var import _native as N
    monkeypatch.setattr(N, "lib", lambda: _StubLib(3, 1, 2))
    p = _stub_plan(3, 1, 2)
    for bad in (np.zeros(1), np.zeros((2, 5)), np.zeros((3, 1)), np.zeros((3, 2, 2)), 1.0):
        with pytest.raises(ValueError, match="edges"):
            p.dynamic_distribution(bad)
    e = np.array([-1.0, 0.0, 1.0])
    for bad in (np.zeros(2), np.zeros((3, 2)), np.zeros((4, 1))):
        with pytest.raises(ValueError, match="copula_params"):
            p.dynamic_distribution(e, bad)
    for bad in (np.zeros(3), np.zeros((3, 3)), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="weights"):
            p.dynamic_distribution(e, None, bad)
    p.dynamic_distribution(e, np.zeros(3), np.zeros((3, 2)))       # a (T,) vector for a one-parameter copula
    with pytest.raises(ValueError, match="n_bins"):
        p.dynamic_distribution_device(e, 3, 0)
    with pytest.raises(ValueError, match="weights"):
        p.dynamic_distribution_device(e, 2, 0, weights=np.zeros((3, 3)))


# ------------------------------------------------------------------ backtest routing
class _Plan:
    """Records the call it was handed; two unit masses below and above the middle edge."""
    T = 2

    def __init__(self):
        self.seen = []

    def _mass(self, edges):
        m = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0]])[:, :np.asarray(edges).shape[-1] - 1]
        return m, np.zeros_like(m)

    def distribution(self, edges):
        self.seen.append(("static", np.array(edges), None, None))
        return self._mass(edges)

    def dynamic_distribution(self, edges, copula_params=None, weights=None):
        self.seen.append(("dynamic", np.array(edges), copula_params, weights))
        return self._mass(edges)


def test_backtest_routes_and_centres():
    from copula_var import backtest as B
    cp, w = np.array([[0.1], [0.2]]), np.array([[0.5, 0.5], [0.25, 0.75]])
    r = np.array([-1.0, np.nan])
    # both None and a scalar mean: plan.distribution, the ladders of before
    p = _Plan()
    u = B.pit(p, r, ptf_mean=0.5)
    F, total = B.predictive_cdf(p, [-2.0, 0.0], ptf_mean=0.5, lower=-50.0)
    assert [s[0] for s in p.seen] == ["static", "static"]
    assert np.array_equal(p.seen[0][1][0], [-100.0, -1.5, INF]) and np.isnan(p.seen[0][1][1, 1])
    assert np.array_equal(p.seen[1][1], [-50.0, -2.5, -0.5, INF])
    assert u[0] == 1.0 / 3.0 and np.isnan(u[1])
    assert np.array_equal(total, [4.0, 0.0]) and np.array_equal(F[0], [0.25, 0.75]) and np.all(np.isnan(F[1]))
    # a 0-d array is a scalar mean too
    p = _Plan()
    B.pit(p, r, np.float64(0.5))
    assert p.seen[0][0] == "static"
    # parameters, weights or a (T,) mean: plan.dynamic_distribution with what was given
    for kw in ({"copula_params": cp}, {"weights": w}, {"copula_params": cp, "weights": w}):
        p = _Plan()
        u = B.pit(p, r, 0.5, **kw)
        kind, edges, got_cp, got_w = p.seen[0]
        assert kind == "dynamic" and got_cp is kw.get("copula_params") and got_w is kw.get("weights")
        assert np.array_equal(edges[0], [-100.0, -1.5, INF]) and u[0] == 1.0 / 3.0 and np.isnan(u[1])
        F, total = B.predictive_cdf(p, [-2.0, 0.0], 0.5, -50.0, **kw)
        kind, edges, got_cp, got_w = p.seen[1]
        assert kind == "dynamic" and got_cp is kw.get("copula_params") and got_w is kw.get("weights")
        assert np.array_equal(edges, [-50.0, -2.5, -0.5, INF]) and np.array_equal(F[0], [0.25, 0.75])
    # a per-date mean: each date's ladder is centred on its own
    pm = np.array([0.5, 0.25])
    p = _Plan()
    u = B.pit(p, np.array([-1.0, 2.0]), pm, weights=w)
    F, _ = B.predictive_cdf(p, [-2.0, 0.0], pm, lower=-50.0)
    F2, _ = B.predictive_cdf(p, np.array([[-2.0, 0.0], [-1.0, 1.0]]), pm)
    assert [s[0] for s in p.seen] == ["dynamic"] * 3 and p.seen[1][2] is None and p.seen[1][3] is None
    assert np.array_equal(p.seen[0][1], [[-100.0, -1.5, INF], [-100.0, 1.75, INF]])
    assert np.array_equal(p.seen[1][1], [[-50.0, -2.5, -0.5, INF], [-50.0, -2.25, -0.25, INF]])
    assert np.array_equal(p.seen[2][1], [[-100.0, -2.5, -0.5, INF], [-100.0, -1.25, 0.75, INF]])
    assert u[0] == 1.0 / 3.0 and np.isnan(u[1])      # the second date's total mass is 0
    for bad in (np.zeros(3), np.zeros((2, 1))):
        with pytest.raises(ValueError, match="ptf_mean"):
            B.pit(p, np.zeros(2), bad)
        with pytest.raises(ValueError, match="ptf_mean"):
            B.predictive_cdf(p, [0.0], bad)
    with pytest.raises(ValueError):
        B.pit(p, np.zeros(3), pm)


def test_driver_methods_centre_on_the_dates_means():
    """calc_dynamic_distribution / calc_dynamic_pit / dynamic_backtest on a stand-in run: the per-date
    means are dynamic_ptf_mean's, the plan sees centred ladders and the arrays it was given."""
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion as V
    v = object.__new__(V)
    v.plan, v.dim, v.ptf_mean = _Plan(), 2, 0.125
    v.mean_returns = {"A": 0.5, "B": 0.25}
    w = np.array([[0.5, 0.5], [0.25, 0.75]])
    pm = np.array([0.5 * 0.5 + 0.25 * 0.5, 0.5 * 0.25 + 0.25 * 0.75])
    assert np.array_equal(v.dynamic_ptf_mean(w), pm)
    v.calc_dynamic_distribution([-2.0, 0.0, 1.0], weights=w)
    kind, edges, cp, got_w = v.plan.seen[-1]
    assert kind == "dynamic" and cp is None and np.array_equal(got_w, w)
    assert np.array_equal(edges, np.array([[-2.0, 0.0, 1.0]] * 2) - pm[:, None])
    v.calc_dynamic_distribution([-2.0, 0.0, 1.0], copula_params=[[0.1], [0.2]])
    assert np.array_equal(v.plan.seen[-1][1], np.array([-2.0, 0.0, 1.0]) - 0.125)
    u = v.calc_dynamic_pit(np.array([-1.0, 2.0]), weights=w)
    assert np.array_equal(v.plan.seen[-1][1], [[-100.0, -1.0 - pm[0], INF], [-100.0, 2.0 - pm[1], INF]])
    assert u[0] == 1.0 / 3.0
    assert v.calc_dynamic_pit(np.array([-1.0, 2.0]))[0] == 1.0 / 3.0 and v.plan.seen[-1][0] == "static"
    table = v.dynamic_backtest(np.array([-1.0, 2.0]), 0.05, np.array([-0.5, -0.5]), weights=w)
    assert table["hits"] == 1 and "berkowitz" in table and np.array_equal(v.last_dynamic_pit, u, equal_nan=True)
    with pytest.raises(ValueError, match="weights"):
        v.calc_dynamic_pit(np.zeros(2), weights=np.zeros((2, 3)))


# ------------------------------------------------------------------ parser
def test_parser_takes_backtest_with_the_dynamic_flags():
    from copula_var.main import build_parser
    base = ["--prices", "p.csv", "--tickers", "A", "B", "--start", "2010-01-01"]
    a = build_parser().parse_args(base + ["--backtest", "--rolling-copula", "250", "--refit-every", "5",
                                          "--drift-weights", "--exact-levels", "0.05"])
    assert a.backtest and a.rolling_copula == 250 and a.refit_every == 5 and a.drift_weights
    assert a.exact_levels == [0.05]
    # nothing it accepted before is rejected
    a = build_parser().parse_args(base + ["--backtest"])
    assert a.backtest and a.rolling_copula is None and not a.drift_weights
    a = build_parser().parse_args(base + ["--rolling-copula", "60", "--exact-levels", "0.05", "0.25", "--es",
                                          "--covar", "A", "--weight-grid", "4", "--contributions"])
    assert not a.backtest and a.rolling_copula == 60
    text = build_parser().format_help()
    assert "dpit_<estimation>" in text and "dhit_<estimation>_<level>" in text


# ------------------------------------------------------------------ the cases the GPU tests use
@pytest.mark.parametrize("name", list(DC.CASES) + list(DC.EDGES))
def test_cases_see_nodes_and_the_records_matter(name):
    """On every shared case the ladder's inner bins hold mass on every date, and in some bin the
    per-date result is at least 0.9 (relative to the static plan's value) away from the static
    plan's: a kernel that ignored the records could not pass the GPU comparison."""
    P, cp, w, _, dates = DC.problem(name)
    static = D.bin_moments(P, LADDER)[0]
    dyn = np.concatenate([D.bin_moments(Pt, LADDER)[0] for Pt in dates], axis=0)
    assert dyn.shape == static.shape == (P.T, LADDER.size - 1)
    assert np.all(dyn[:, 2:6] > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(dyn - static) / np.abs(static)
    print(name, "largest relative difference", np.nanmax(rel))
    assert np.nanmax(rel) >= 0.9
