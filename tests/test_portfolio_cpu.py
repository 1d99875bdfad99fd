"""Batched-weights quantiles without a GPU: host-side validation of cvq_portfolio_quantiles, the
numpy checker (tests/portfolio_reference.py) and its decision margins on the GPU tests' inputs
(tests/portfolio_cases.py), the candidate lattice, the pick, the CLI flag."""
import ctypes as C

import numpy as np
import pytest

import es_reference as E
import portfolio_cases as PC
import portfolio_reference as R
import quantile_reference as Q
from conftest import load_golden

MARGIN = 1e-7                     # 1000 x the slab bar of 1e-10: a condition of the GPU tests' exact equality


def test_entry_point_validates_on_the_host():
    """Every check that needs no plan.  (A non-finite weight and weights[p][0] <= 0 are read
    through the plan's dim: tests/test_portfolio_gpu.py::test_weights_validated.)"""
    from copula_var import _native as N
    lib = N.lib()
    assert lib.cvq_version() >= 10700 and N.MAX_PORTFOLIOS == 64
    out = np.zeros(64 * 8)
    a = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-6, 0.0)
    w0 = np.tile([0.5, 0.5], (65, 1))

    def call(levels=(0.05,), L=1, P=1, args=a, w=w0, pm=None, var=out, plan=None, null_pm=False, null_lv=False):
        lv = np.asarray(levels, dtype=np.float64)
        pm = np.zeros(65) if pm is None else np.asarray(pm, dtype=np.float64)
        return lib.cvq_portfolio_quantiles(
            plan, C.byref(args) if args is not None else None, N.ptr(w) if w is not None else None,
            None if null_pm else N.ptr(pm), P, None if null_lv else N.ptr(lv), L,
            N.ptr(var) if var is not None else None, None, None, N.MEM_HOST)

    assert call() == N.CVQ_ERR_INVALID                             # NULL plan: the last check
    assert b"plan" in lib.cvq_last_error()
    for kw in (dict(args=None), dict(w=None), dict(null_pm=True), dict(null_lv=True), dict(var=None)):
        assert call(**kw) == N.CVQ_ERR_INVALID
        assert b"NULL" in lib.cvq_last_error()
    for P in (0, -1, 65):
        assert call(P=P) == N.CVQ_ERR_INVALID
        assert b"n_portfolios" in lib.cvq_last_error()
    for L in (0, 9):
        assert call([0.05] * 9, L) == N.CVQ_ERR_INVALID
        assert b"n_levels" in lib.cvq_last_error()
    for bad in (0.0, -1.0, float("nan")):
        assert call([0.05, bad], 2) == N.CVQ_ERR_INVALID
        assert b"level" in lib.cvq_last_error()
    flat = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, 0.0, 0.0, -100.0, 1e-6, 0.0)
    assert call(args=flat) == N.CVQ_ERR_INVALID
    assert b"max_var" in lib.cvq_last_error()
    for bad in (float("nan"), float("inf")):
        assert call(P=3, pm=[0.0, 0.0, bad]) == N.CVQ_ERR_INVALID
        assert b"ptf_mean" in lib.cvq_last_error()
    odd = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-6, float("nan"))
    assert call(args=odd) == N.CVQ_ERR_INVALID and b"plan" in lib.cvq_last_error()   # args->ptf_mean is not read
    deep = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-300, 0.0)
    assert call(args=deep) == N.CVQ_ERR_UNSUPPORTED                # K > 62
    b = C.c_int64()
    assert lib.cvq_portfolio_scratch(None, 1, 1, C.byref(b)) == N.CVQ_ERR_INVALID


@pytest.mark.parametrize("case", ["cfg2_n64", "cfg4_k4_n16"])
def test_checker_at_the_plans_own_weights_is_the_quantile_checker(case):
    z = load_golden(case)
    P = E.problem_of(z, slice(0, 3))
    ptf = float(z["ptf_mean"])
    got = R.portfolio_quantiles(P, [P.w], R.LEVELS, [ptf])
    ref = Q.quantiles(P, R.LEVELS, ptf)
    for a, b in zip(got, ref):
        assert a.shape == (3, 1, 3) and np.array_equal(a[:, 0, :], b, equal_nan=True)


def test_checker_copies_differ_only_in_the_weights():
    P, _ = PC.problem("cfg2_n64")
    Pw = R.with_weights(P, (0.3, 0.7))
    assert np.array_equal(P.w, [0.5, 0.5]) and np.array_equal(Pw.w, [0.3, 0.7])
    assert Pw.mass(0) is P.mass(0)                                 # one measure
    assert Pw.slab(0, -100.0, -1.0) != P.slab(0, -100.0, -1.0)


@pytest.mark.parametrize("name", list(PC.PARITY) + list(PC.EDGES) + ["gumbel"])
def test_checker_margin(name):
    """The premise of the GPU tests' exact comparison: no evaluated F within 1e-7 of a level, and no
    level outside the bracket."""
    var, es, _, margin = PC.reference(name)
    _, w = PC.problem(name)
    print(name, "margin", margin.min(), "per candidate", margin.min(axis=(0, 2)))
    assert var.shape[1:] == (len(w), len(R.LEVELS))
    assert margin.min() >= MARGIN
    assert not np.isnan(var).any() and not np.isnan(es).any()
    if name == "3d_n17":
        assert margin.min() >= 2.0e-4
    if name == "2d_n130":
        assert margin.min() >= 5.7e-6


def test_checker_outside_the_bracket():
    var, es, m0, margin = PC.reference("outside")
    nan = np.isnan(var[:, :, 1])
    assert nan.any() and not nan.all()
    assert nan.any(axis=0).sum() >= 2 and (~nan).any(axis=0).sum() >= 2     # mixed across portfolios
    assert np.array_equal(np.isnan(es[:, :, 1]), nan) and not np.isnan(var[:, :, 0]).any()
    assert np.all(m0[:, :, 1][nan] < PC.OUTSIDE_LEVEL)             # m0 = F(max_var) below the level
    assert margin.min() >= MARGIN


def test_weight_lattice():
    from copula_var.portfolios import weight_lattice
    w2, w3 = weight_lattice(2, 4), weight_lattice(3, 4)
    assert w2.shape == (4, 2) and w3.shape == (10, 3)
    assert np.array_equal(w2, [[0.25, 0.75], [0.5, 0.5], [0.75, 0.25], [1.0, 0.0]])
    for dim, steps, count in ((2, 4, 4), (3, 4, 10), (3, 7, 28), (2, 1, 1)):
        w = weight_lattice(dim, steps)
        assert w.shape == (count, dim)
        k = np.round(w * steps)
        assert np.array_equal(k / steps, w) and np.all(k >= 0) and np.all(k[:, 0] >= 1)
        assert np.all(k.sum(axis=1) == steps)
        rows = [tuple(r) for r in k]
        assert rows == sorted(rows) and len(set(rows)) == len(rows)          # lexicographic, no repeats
    assert np.array_equal(w3[0], [0.25, 0.0, 0.75]) and np.array_equal(w3[-1], [1.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        weight_lattice(1, 4)
    with pytest.raises(ValueError):
        weight_lattice(2, 0)


def test_min_es_tie_and_nan_rules():
    from copula_var.portfolios import min_es
    nan = float("nan")
    es = np.array([[[-3.0], [-2.0], [-2.0], [nan]],                # a tie: the first in batch order
                   [[nan], [-5.0], [nan], [-4.0]],                 # NaN candidates never win
                   [[nan], [nan], [nan], [nan]],                   # an all-NaN date
                   [[nan], [-np.inf], [nan], [nan]]])              # the only number there is
    idx, val = min_es(es)
    assert idx.shape == (4, 1) and val.shape == (4, 1)
    assert idx[:, 0].tolist() == [1, 3, -1, 1]
    assert np.array_equal(val[:, 0], [-2.0, -4.0, nan, -np.inf], equal_nan=True)
    two = np.stack((es[:, :, 0], es[:, ::-1, 0]), axis=2)          # levels are independent
    idx2, _ = min_es(two)
    assert idx2[:, 0].tolist() == [1, 3, -1, 1] and idx2[:, 1].tolist() == [1, 0, -1, 2]
    with pytest.raises(ValueError):
        min_es(np.zeros((3, 2)))


def test_main_weight_grid_flag_parses():
    from copula_var.main import build_parser
    base = ["--prices", "p.csv", "--tickers", "A", "B", "--start", "2009-04-15"]
    assert build_parser().parse_args(base).weight_grid is None
    assert build_parser().parse_args(base + ["--weight-grid", "4"]).weight_grid == 4
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--weight-grid", "x"])
