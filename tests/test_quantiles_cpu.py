"""Exact quantiles without a GPU: the numpy checker (tests/quantile_reference.py) on the goldens,
host-side validation of cvq_quantiles, the sharded exchange on gloo ranks, the CLI flag."""
import ctypes as C
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import es_reference as E
import quantile_reference as Q
from conftest import golden_kwargs, load_golden

CASES = ["cfg1", "cfg2_n64", "q1_lowvol", "cfg4_k4_n16", "garch3d_student_n16", "msm_plackett_n64", "cfg5_n64",
         "ukf_plackett_n64", "cfg1_hivol", "msm_gauss_n64"]
LEVELS = (0.01, 0.025, 0.05, 0.10)
TOL = 1e-6
MARGIN = 1e-7                     # 1000 x the slab bar of 1e-10: a condition of the GPU tests' exact equality


@functools.lru_cache(maxsize=None)
def _ref(case):
    z = load_golden(case)
    P = E.problem_of(z)
    return z, P, Q.quantiles(P, LEVELS, float(z["ptf_mean"]))


@pytest.mark.parametrize("case", CASES)
def test_checker_finite_monotone_and_bracketing(case):
    z, P, (var, es, m0, margin) = _ref(case)
    ptf = float(z["ptf_mean"])
    assert not np.isnan(var).any() and not np.isnan(es).any() and not np.isnan(m0).any()
    assert np.all(np.diff(var, axis=1) >= 0.0)                     # non-decreasing in the level
    assert np.all(es < var)
    for t in range(P.T):
        for l, alpha in enumerate(LEVELS):
            v = var[t, l] - ptf
            assert P.slab(t, -100.0, v - TOL) < alpha <= P.slab(t, -100.0, v + TOL), (t, alpha)


@pytest.mark.parametrize("case", CASES)
def test_checker_against_the_goldens(case):
    """Where the golden VaR lies at or below -2 the reference's bisection is right: both end within
    tolerance / 2 of the same jump of F."""
    z, P, (var, _, _, _) = _ref(case)
    assert not golden_kwargs(z)                                    # recorded at the default obj_var = 0.05
    g = z["var"]
    right = g - float(z["ptf_mean"]) <= -2.0
    d = np.abs(var[:, 2] - g)
    print(case, "dates the reference has right:", int(right.sum()), "of", g.size,
          "max diff there:", d[right].max() if right.any() else None)
    assert np.all(d[right] <= TOL)
    if case == "q1_lowvol":                                        # Q1 is visible on every date
        assert np.all(d > 1.0)


@pytest.mark.parametrize("case", CASES)
def test_checker_margin(case):
    _, _, (_, _, _, margin) = _ref(case)
    print(case, "margin", margin.min())
    assert margin.min() >= MARGIN


def test_checker_nan_cases():
    z = load_golden("cfg1")
    var, es, m0, _ = Q.quantiles(E.problem_of(z), [0.6], float(z["ptf_mean"]))
    assert np.isnan(var).all() and np.isnan(es).all()
    assert np.all(m0 <= 0.527) and np.all(m0 > 0)                  # m0 = F(max_var)
    z = load_golden("msm_plackett_n64")
    var, es, m0, _ = Q.quantiles(E.problem_of(z), [0.2], float(z["ptf_mean"]))
    nan = np.isnan(var[:, 0])
    assert nan.any() and (~nan).any()
    assert np.array_equal(np.isnan(es[:, 0]), nan)
    assert np.all(m0[nan, 0] < 0.2) and np.all(m0[nan, 0] > 0.18)  # m0 = F(max_var) below the level
    assert np.all(np.isfinite(m0[~nan, 0]))


def test_entry_point_validates_on_the_host():
    from copula_var import _native as N
    lib = N.lib()
    assert lib.cvq_version() >= 10200
    out = np.zeros(16)
    a = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-6, 0.0)

    def call(levels, L, args=a, plan=None, var=out):
        lv = np.asarray(levels, dtype=np.float64)
        return lib.cvq_quantiles(plan, C.byref(args) if args is not None else None, N.ptr(lv), L,
                                 N.ptr(var) if var is not None else None, None, None, N.MEM_HOST)

    assert call([0.05], 1) == N.CVQ_ERR_INVALID                    # NULL plan
    assert b"plan" in lib.cvq_last_error()
    assert call([0.05], 1, args=None) == N.CVQ_ERR_INVALID
    assert call([0.05], 1, var=None) == N.CVQ_ERR_INVALID
    for L in (0, 9):
        assert call([0.05] * 9, L) == N.CVQ_ERR_INVALID
        assert b"n_levels" in lib.cvq_last_error()
    for bad in (0.0, -1.0, float("nan")):
        assert call([0.05, bad], 2) == N.CVQ_ERR_INVALID
        assert b"level" in lib.cvq_last_error()
    flat = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, 0.0, 0.0, -100.0, 1e-6, 0.0)
    assert call([0.05], 1, args=flat) == N.CVQ_ERR_INVALID
    assert b"max_var" in lib.cvq_last_error()
    deep = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-300, 0.0)
    assert call([0.05], 1, args=deep) == N.CVQ_ERR_UNSUPPORTED     # K > 62


# ------------------------------------------------------------------ sharding on gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SHARD_LEVELS = (0.025, 0.05)


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

        def quant_local(block):
            var, es, m0, _ = Q.quantiles(P, SHARD_LEVELS, ptf)
            block.copy_(torch.from_numpy(np.stack((var, es, m0), axis=2)))

        s = ShardedVaR(T, 3, lambda h, sn: None, lambda b, v: None, torch.device("cpu"), quant_local=quant_local)
        q.put((rank, s.quantiles(len(SHARD_LEVELS)).numpy().copy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case,world", [("cfg1", 2), ("msm_gauss_n64", 3)])
def test_gloo_sharded_quantiles_are_bit_identical(case, world):
    """World 2, and world 3 over the uneven T = 10 (blocks of 4, 4, 2: the last block's padding
    never reaches the result): every rank holds the unsharded result bit for bit."""
    z = load_golden(case)
    var, es, m0, _ = Q.quantiles(E.problem_of(z), SHARD_LEVELS, float(z["ptf_mean"]))
    ref = np.stack((var, es, m0), axis=2)
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


def test_sharded_quantiles_need_quant_local():
    from copula_var.distributed import ShardedVaR
    s = ShardedVaR(4, 3, lambda h, sn: None, lambda b, v: None, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="quant_local"):
        s.quantiles(2)


def test_main_exact_levels_flag_parses():
    from copula_var.main import build_parser
    base = ["--prices", "p.csv", "--tickers", "A", "B", "--start", "2009-04-15"]
    assert build_parser().parse_args(base).exact_levels is None
    assert build_parser().parse_args(base + ["--exact-levels", "0.01", "0.05"]).exact_levels == [0.01, 0.05]
