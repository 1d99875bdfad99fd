"""cvq_distribution without a GPU: the symbol is declared, exported and bound, every
CVQ_ERR_INVALID path fails on the host before any device work, and the engine's split of more
than MAX_BINS bins into several calls is held against a stubbed native call."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "cvq.h")


def test_symbol_is_declared_exported_and_bound():
    from copula_var import _native as N
    src = open(HEADER).read()
    assert re.search(r"#define\s+CVQ_MAX_BINS\s+64\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int32_t\s+cvq_distribution\s*\(([^)]*)\)", code)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["plan", "edges", "n_bins", "per_date", "mass_out", "m1_out", "mem"]
    assert hasattr(C.CDLL(N.LIB_PATH), "cvq_distribution")
    assert '"cvq_distribution"' in inspect.getsource(N._declare)
    lib = N.lib()
    assert len(lib.cvq_distribution.argtypes) == 7 and lib.cvq_distribution.restype is C.c_int32
    assert N.MAX_BINS == 64
    assert lib.cvq_version() >= 10900                # the feature is detected by the symbol, not the version


def test_invalid_arguments_fail_on_the_host():
    """Every CVQ_ERR_INVALID path, in the order the entry point checks them (arguments first,
    the plan last), without a device: the message says which check fired."""
    from copula_var import _native as N
    lib = N.lib()
    e, out = np.array([-100.0, -3.0, np.inf]), np.zeros(8)
    err = lambda: (lib.cvq_last_error() or b"").decode()
    call = lambda plan, edges, nb, per, mass, m1=None, mem=N.MEM_HOST: lib.cvq_distribution(
        plan, N.ptr(edges) if edges is not None else None, nb, per, N.ptr(mass) if mass is not None else None,
        N.ptr(m1) if m1 is not None else None, mem)
    assert call(None, None, 2, 0, out) == N.CVQ_ERR_INVALID and "NULL argument" in err()
    assert call(None, e, 2, 0, None) == N.CVQ_ERR_INVALID and "NULL argument" in err()
    for nb in (0, -1, N.MAX_BINS + 1, 2 ** 31 - 1):
        assert call(None, e, nb, 0, out) == N.CVQ_ERR_INVALID and "n_bins" in err(), nb
    for per in (-1, 2, 7):
        assert call(None, e, 2, per, out) == N.CVQ_ERR_INVALID and "per_date" in err(), per
    for mem in (N.MEM_HOST, N.MEM_DEVICE):           # everything else valid: the NULL plan is what is left
        assert call(None, e, 2, 0, out, out, mem) == N.CVQ_ERR_INVALID and "plan is NULL" in err()
        assert call(None, e, N.MAX_BINS, 1, out, None, mem) == N.CVQ_ERR_INVALID and "plan is NULL" in err()


class _StubLib:
    """cvq_distribution that records its calls and fills mass = upper edge, m1 = lower edge."""

    def __init__(self, T):
        self.T, self.calls = T, []

    def cvq_distribution(self, h, edges, nb, per_date, mass, m1, mem):
        cols = nb + 1
        e = np.ctypeslib.as_array(C.cast(edges, C.POINTER(C.c_double)), shape=(self.T * cols if per_date else cols,))
        e = np.array(e).reshape((self.T, cols) if per_date else (cols,))
        self.calls.append((nb, per_date, mem, e))
        ee = e if per_date else np.broadcast_to(e, (self.T, cols))
        np.ctypeslib.as_array(C.cast(mass, C.POINTER(C.c_double)), shape=(self.T, nb))[:] = ee[:, 1:]
        np.ctypeslib.as_array(C.cast(m1, C.POINTER(C.c_double)), shape=(self.T, nb))[:] = ee[:, :-1]
        return 0


def _stub_plan(T):
    from copula_var.engine import QuadraturePlan
    p = object.__new__(QuadraturePlan)               # no device: only the fields distribution() reads
    p.T, p._h = T, None
    return p


@pytest.mark.parametrize("B", [1, 63, 64, 65, 128, 150])
def test_engine_splits_more_than_max_bins(monkeypatch, B):
    from copula_var import _native as N
    T = 3
    stub = _StubLib(T)
    monkeypatch.setattr(N, "lib", lambda: stub)
    p = _stub_plan(T)
    shared = np.linspace(-7.0, 2.0, B + 1)
    mass, m1 = p.distribution(shared)
    assert mass.shape == m1.shape == (T, B)
    assert np.array_equal(mass, np.broadcast_to(shared[1:], (T, B))) and np.array_equal(m1[0], shared[:-1])
    sizes = [c[0] for c in stub.calls]
    assert sizes == [64] * (B // 64) + ([B % 64] if B % 64 else [])
    assert all(c[1] == 0 and c[2] == N.MEM_HOST for c in stub.calls)
    at = 0
    for nb, _, _, e in stub.calls:                   # neighbouring calls share their boundary edge
        assert np.array_equal(e, shared[at:at + nb + 1])
        at += nb
    stub.calls.clear()
    per = shared[None, :] + np.arange(T)[:, None]    # a ladder of its own per date
    mass, m1 = p.distribution(per)
    assert np.array_equal(mass, per[:, 1:]) and np.array_equal(m1, per[:, :-1])
    assert [c[0] for c in stub.calls] == sizes and all(c[1] == 1 for c in stub.calls)
    assert all(c[3].flags["C_CONTIGUOUS"] for c in stub.calls)


def test_engine_rejects_bad_edge_shapes(monkeypatch):
    from copula_var import _native as N
    monkeypatch.setattr(N, "lib", lambda: _StubLib(3))
    p = _stub_plan(3)
    for bad in (np.zeros(1), np.zeros((2, 5)), np.zeros((3, 1)), np.zeros((3, 2, 2)), 1.0):
        with pytest.raises(ValueError):
            p.distribution(bad)


def test_backtest_ladders_through_a_stub(monkeypatch):
    """predictive_cdf and pit build the ladders the definition names and normalise by the total."""
    from copula_var import backtest as B

    class Plan:
        T = 2

        def distribution(self, edges):
            self.edges = np.array(edges)
            m = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0]])[:, :self.edges.shape[-1] - 1]
            return m, np.zeros_like(m)

    p = Plan()
    F, total = B.predictive_cdf(p, [-2.0, 0.0], ptf_mean=0.5, lower=-50.0)
    assert np.array_equal(p.edges, [-50.0, -2.5, -0.5, np.inf])
    assert np.array_equal(total, [4.0, 0.0]) and np.array_equal(F[0], [0.25, 0.75]) and np.all(np.isnan(F[1]))
    u = B.pit(p, np.array([-1.0, np.nan]), ptf_mean=0.5)
    assert np.array_equal(p.edges[0], [-100.0, -1.5, np.inf]) and np.isnan(p.edges[1, 1])
    assert u[0] == 1.0 / 3.0 and np.isnan(u[1])
    with pytest.raises(ValueError):
        B.pit(p, np.zeros(3))
