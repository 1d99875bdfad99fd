"""Conditional quantiles (CoVaR / CoES) without a GPU: the numpy checker
(tests/conditional_reference.py) on the goldens, the premise of the GPU tests' exact comparison,
copula_var.conditional.marginal_quantile, host-side validation of cvq_conditional_quantiles, the
sharded exchange on gloo ranks, the CLI flags."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import conditional_cases as CC
import conditional_reference as CR
import es_reference as E
import quantile_reference as Q
from conftest import load_golden

MARGIN = 1e-7                     # tests/test_quantiles_cpu.py's bar: 1000 x the slab bar of 1e-10
INF = float("inf")


# ------------------------------------------------------------------ 1. checker identities
@pytest.mark.parametrize("case,axis", [("cfg2_n64", 0), ("cfg2_n64", 1), ("garch3d_student_n16", 1)])
def test_full_event_is_the_unconditional_quantile(case, axis):
    """Event (-inf, +inf]: covar at level alpha = quantile_reference's var at level alpha p_E[t],
    date by date, bit for bit (and so are coes / m0)."""
    P, _, ptf = CC.problem(case)
    covar, coes, m0, pe, _ = CR.conditional_quantiles(P, axis, -INF, INF, CC.LEVELS, ptf)
    assert not np.isnan(covar[:, :2]).any()
    for t in range(P.T):
        var, es, qm0, _ = Q.quantiles(CC.dates(P, slice(t, t + 1)), np.asarray(CC.LEVELS) * pe[t], ptf)
        assert np.array_equal(covar[t], var[0], equal_nan=True)
        assert np.array_equal(coes[t], es[0], equal_nan=True) and np.array_equal(m0[t], qm0[0])


@pytest.mark.parametrize("case,axis", [("cfg2_n64", 0), ("cfg2_n64", 1), ("cfg4_k4_n16", 0), ("cfg4_k4_n16", 1),
                                       ("cfg4_k4_n16", 2), ("ukf_plackett_n64", 0)])
def test_complementary_events_partition_the_box(case, axis):
    P, _, _ = CC.problem(case)
    s = CR.marginal_quantile(P, axis, 0.3)
    for v in (INF, 0.0, -2.0, -3.25):
        lo, hi = CR.conditional_mass(P, axis, -INF, s, v), CR.conditional_mass(P, axis, s, INF, v)
        whole = np.array([P.slab(t, -100.0, v) for t in range(P.T)])
        np.testing.assert_allclose(lo + hi, whole, rtol=1e-12, atol=0.0)
        assert np.array_equal(whole, CR.conditional_mass(P, axis, -INF, INF, v))


@pytest.mark.parametrize("name,axis,kind", CC.EXACT, ids=lambda v: str(v))
def test_margin_premise_and_coes_below_covar(name, axis, kind):
    """Every input the GPU tests compare exactly: no decision closer than 1e-7 (relative) to its
    target; coes <= covar wherever both are finite."""
    _, _, _, _, (covar, coes, m0, pe, margin) = CC.reference(name, axis, kind)
    print(name, axis, kind, "margin", margin.min(), "p_E", pe.min(), pe.max(), "NaN", int(np.isnan(covar).sum()))
    assert margin.min() >= MARGIN
    ok = np.isfinite(covar) & np.isfinite(coes)
    assert np.all(coes[ok] <= covar[ok])
    assert np.array_equal(np.isnan(covar), np.isnan(coes)) or np.all(m0[np.isnan(coes) & ~np.isnan(covar)] == 0.0)


def test_empty_events():
    """A NaN bound, s_hi <= s_lo and s_hi = -inf: p_E = 0, everything NaN, m0 = 0."""
    P, _, ptf = CC.problem("cfg2_n64")
    P4 = CC.dates(P, slice(0, 4))
    s_lo = np.array([np.nan, -1.0, -INF, -INF])
    s_hi = np.array([0.0, -1.0, -INF, np.nan])
    for axis in range(2):
        covar, coes, m0, pe, margin = CR.conditional_quantiles(P4, axis, s_lo, s_hi, CC.LEVELS, ptf)
        assert np.all(pe == 0.0) and np.all(m0 == 0.0) and np.isnan(covar).all() and np.isnan(coes).all()
        assert np.all(margin == INF)


# ------------------------------------------------------------------ 3. NaN pattern
def test_nan_pattern_of_the_stress_event():
    """The stress event at 0.05 leaves no NaN on any small golden except where the event holds no
    grid node: so a comparison elsewhere cannot pass on NaNs."""
    expect = {("cfg1_hivol", 0): (24, 72), ("cfg1_hivol", 1): (9, 27), ("ukf_plackett_n64", 0): (5, 15)}
    for case in CC.SMALL:
        for axis in CC._axes(case):
            _, _, _, _, (covar, coes, m0, pe, _) = CC.reference(case, axis, "stress")
            empty, nans = expect.get((case, axis), (0, 0))
            assert int((pe == 0.0).sum()) == empty, (case, axis)
            assert int(np.isnan(covar).sum()) == nans and int(np.isnan(coes).sum()) == nans, (case, axis)
            assert np.array_equal(np.isnan(covar), np.repeat((pe == 0.0)[:, None], len(CC.LEVELS), axis=1))
            assert np.all(pe[pe != 0.0] > 1e-3)
    P, _, _ = CC.problem("cfg1_hivol")
    assert P.T == 24


# ------------------------------------------------------------------ 4. marginal_quantile
def _per(P):
    return ((P.fbs, P.pi), P.uvs) if P.model == "msm" else (P.sigma, None)


@pytest.mark.parametrize("case", ["cfg2_n64", "cfg4_k4_n16"])
def test_marginal_quantile_inverts_the_mixture_cdf(case):
    from copula_var.conditional import marginal_quantile
    P, _, _ = CC.problem(case)
    per, vs = _per(P)
    for asset in range(P.dim):
        for q in (0.001, 0.05, 0.25, 0.5, 0.75, 0.99):
            s = marginal_quantile("msm", per, vs, asset, q)
            assert s.shape == (P.T,)
            assert np.max(np.abs(CR.marginal_cdf(P, asset, s) - q)) <= 1e-12
            np.testing.assert_allclose(s, CR.marginal_quantile(P, asset, q), rtol=0, atol=1e-12)
        assert np.all(marginal_quantile("msm", per, vs, asset, 0.0) == -INF)
        assert np.all(marginal_quantile("msm", per, vs, asset, 1.0) == INF)


def test_marginal_quantile_of_a_sigma_model():
    from scipy import special
    from copula_var.conditional import marginal_quantile
    P, _, _ = CC.problem("cfg1")
    for asset in range(2):
        for q in (0.05, 0.25, 0.75):
            assert np.array_equal(marginal_quantile("garch", P.sigma, None, asset, q),
                                  P.sigma[:, asset] * special.ndtri(q))
        assert np.all(marginal_quantile("garch", P.sigma, None, asset, 0.0) == -INF)
        assert np.all(marginal_quantile("garch", P.sigma, None, asset, 1.0) == INF)
    with pytest.raises(ValueError):
        marginal_quantile("garch", P.sigma, None, 2, 0.05)
    with pytest.raises(ValueError):
        marginal_quantile("garch", P.sigma, None, 0, 1.5)


# ------------------------------------------------------------------ 5. host validation
def test_entry_point_validates_on_the_host():
    from copula_var import _native as N
    lib = N.lib()
    assert lib.cvq_version() >= 10600
    out = np.zeros(16)
    cond = np.zeros((8, 2))
    a = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-6, 0.0)

    def call(levels, L, args=a, plan=None, covar=out, axis=0, cd=cond):
        lv = np.asarray(levels, dtype=np.float64)
        return lib.cvq_conditional_quantiles(plan, C.byref(args) if args is not None else None, axis,
                                             N.ptr(cd) if cd is not None else None, N.ptr(lv), L,
                                             N.ptr(covar) if covar is not None else None, None, None, None,
                                             N.MEM_HOST)

    assert call([0.05], 1) == N.CVQ_ERR_INVALID                    # NULL plan
    assert b"plan" in lib.cvq_last_error()
    for axis in (-1, 3, 7):                                        # the dim is unknown without a plan
        assert call([0.05], 1, axis=axis) == N.CVQ_ERR_INVALID
        assert b"axis" in lib.cvq_last_error()
    assert call([0.05], 1, cd=None) == N.CVQ_ERR_INVALID
    assert b"NULL" in lib.cvq_last_error()
    assert call([0.05], 1, args=None) == N.CVQ_ERR_INVALID
    assert call([0.05], 1, covar=None) == N.CVQ_ERR_INVALID
    for L in (0, 9):
        assert call([0.05] * 9, L) == N.CVQ_ERR_INVALID
        assert b"n_levels" in lib.cvq_last_error()
    for bad in (0.0, -1.0, float("nan"), INF):
        assert call([0.05, bad], 2) == N.CVQ_ERR_INVALID
        assert b"level" in lib.cvq_last_error()
    flat = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, 0.0, 0.0, -100.0, 1e-6, 0.0)
    assert call([0.05], 1, args=flat) == N.CVQ_ERR_INVALID
    assert b"max_var" in lib.cvq_last_error()
    deep = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-300, 0.0)
    assert call([0.05], 1, args=deep) == N.CVQ_ERR_UNSUPPORTED     # K > 62


# ------------------------------------------------------------------ 6. sharding on gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SHARD_LEVELS = (0.05, 0.5)


def _sharded_reference(P, ptf):
    s = CR.marginal_quantile(P, 0, 0.05)
    covar, coes, m0, pe, _ = CR.conditional_quantiles(P, 0, -INF, s, SHARD_LEVELS, ptf)
    return np.stack((covar, coes, m0, np.repeat(pe[:, None], len(SHARD_LEVELS), axis=1)), axis=2)


def _worker(rank, world, port, case, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from copula_var.distributed import ShardedVaR, shard
        z = load_golden(case)
        T = int(z["var"].size)
        lo, hi, per = shard(T, rank, world)
        P = E.problem_of(z, slice(lo, hi))
        ptf = float(z["ptf_mean"])

        def cond_local(block):
            block.copy_(torch.from_numpy(_sharded_reference(P, ptf)))

        s = ShardedVaR(T, 3, lambda h, sn: None, lambda b, v: None, torch.device("cpu"), cond_local=cond_local)
        q.put((rank, s.conditional_quantiles(len(SHARD_LEVELS)).numpy().copy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case,world", [("cfg1", 2), ("msm_gauss_n64", 3)])
def test_gloo_sharded_conditional_quantiles_are_bit_identical(case, world):
    """World 2, and world 3 over the uneven T = 10 (blocks of 4, 4, 2): every rank holds the
    unsharded result bit for bit."""
    z = load_golden(case)
    ref = _sharded_reference(E.problem_of(z), float(z["ptf_mean"]))
    assert not np.isnan(ref).any()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert len(out) == world
    for got in out.values():
        assert got.shape == ref.shape and np.array_equal(got, ref)


def test_sharded_conditional_quantiles_need_cond_local():
    from copula_var.distributed import ShardedVaR
    s = ShardedVaR(4, 3, lambda h, sn: None, lambda b, v: None, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="cond_local"):
        s.conditional_quantiles(2)


# ------------------------------------------------------------------ 7. parser
def test_main_covar_flags_parse():
    from copula_var.main import build_parser
    base = ["--prices", "p.csv", "--tickers", "A", "B", "--start", "2009-04-15"]
    a = build_parser().parse_args(base)
    assert a.covar is None and a.covar_stress == 0.05
    a = build_parser().parse_args(base + ["--covar", "B", "--covar-stress", "0.1", "--exact-levels", "0.01", "0.05"])
    assert a.covar == "B" and a.covar_stress == 0.1 and a.exact_levels == [0.01, 0.05]
