"""Expected Shortfall without a GPU: the numpy checker (tests/es_reference.py) on the goldens,
host-side validation of the new entry points, the sharded ES exchange on gloo ranks, the CLI flag."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import es_reference as E
from conftest import GOLDEN_CASES, load_golden

K = 30                                   # bisection budget of the oracle's sharded restatement
SMALL = [c for c in GOLDEN_CASES if c not in ("cfg2_n256", "cfg3_n128")]


@pytest.mark.parametrize("case", SMALL)
def test_checker_on_goldens(case):
    """m0 is Problem.compute_integral's value bit for bit; the ES lies below the VaR."""
    z = load_golden(case)
    P = E.problem_of(z)
    ptf = float(z["ptf_mean"])
    es, m0, m1, m1a = E.expected_shortfall(P, z["var"], ptf)
    b = np.column_stack((np.full(P.T, -100.0), z["var"] - ptf))
    assert np.array_equal(m0, P.compute_integral(b))
    assert np.all(es < z["var"])
    assert np.all(m1 < 0) and np.array_equal(m1a, -m1)          # bounds <= 0: one sign
    assert np.all(np.abs(m1 / m0) >= 0.5)                        # the ES tolerance's premise


def test_checker_nan_and_empty():
    z = load_golden("cfg2_n64")
    P = E.problem_of(z)
    m0, m1, _ = E.tail_moments(P, np.tile((np.nan, -3.0), (P.T, 1)))
    assert np.all(m0 == 0) and np.all(m1 == 0)
    var = z["var"].copy()
    var[2] = np.nan
    es = E.expected_shortfall(P, var, float(z["ptf_mean"]))[0]
    assert np.array_equal(np.isnan(es), np.isnan(var))


def test_entry_points_validate_on_the_host():
    from copula_var import _native as N
    lib = N.lib()
    assert lib.cvq_version() >= 10100
    buf = np.zeros(4)
    a = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-6, 0.0)
    assert lib.cvq_slab_moments(None, N.ptr(buf), N.ptr(buf), N.ptr(buf), N.MEM_HOST) == N.CVQ_ERR_INVALID
    assert lib.cvq_expected_shortfall(None, C.byref(a), N.ptr(buf), N.ptr(buf), None, N.MEM_HOST) == \
        N.CVQ_ERR_INVALID
    assert lib.cvq_last_error()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, case, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from copula_var.distributed import ShardedVaR, shard
        from oracle import sharded as S
        z = load_golden(case)
        T = int(z["var"].size)
        lo, hi, per = shard(T, rank, world)
        P = E.problem_of(z, slice(lo, hi))
        ptf = float(z["ptf_mean"])

        def local(hdr, snaps):
            it, err, nz, sn = S.local_solve(P, ptf, K)
            hdr[0] = it | (err << 32)
            hdr[1] = nz if nz < (1 << 63) else nz - (1 << 64)
            snaps[: sn.shape[0]] = torch.from_numpy(sn)

        def finalize(blocks, var):
            hdr_all = blocks[:, s.hdr_off: s.hdr_off + 2].contiguous().view(torch.int64)
            snaps_all = blocks[:, : per * (K + 1)].reshape(world * per, K + 1)
            h = hdr_all.numpy().reshape(-1, 2)
            headers = [(int(a) & 0xFFFFFFFF, int(a) >> 32, int(b) & ((1 << 64) - 1)) for a, b in h]
            v, _, err = S.finalize(headers, snaps_all.numpy(), T, K, ptf)
            assert not err
            var.copy_(torch.from_numpy(v))

        def es_local(var_block, es_block):
            es_block.copy_(torch.from_numpy(E.expected_shortfall(P, var_block.numpy(), ptf)[0]))

        s = ShardedVaR(T, K + 1, local, finalize, torch.device("cpu"), es_local=es_local)
        var = s.solve().numpy().copy()
        q.put((rank, (var, s.expected_shortfall().numpy().copy())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case,world", [("cfg1", 2), ("msm_gauss_n64", 3)])
def test_gloo_sharded_es_is_bit_identical(case, world):
    """World 2, and world 3 over the uneven T = 10 (blocks of 4, 4, 2: the last block's padding
    never reaches the result): every rank holds the unsharded ES bit for bit."""
    z = load_golden(case)
    ref = E.expected_shortfall(E.problem_of(z), z["var"], float(z["ptf_mean"]))[0]
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
    for var, es in out.values():
        assert np.array_equal(var, z["var"])
        assert es.shape == ref.shape and np.array_equal(es, ref)


def test_sharded_es_needs_es_local():
    from copula_var.distributed import ShardedVaR
    s = ShardedVaR(4, 3, lambda h, sn: None, lambda b, v: None, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="es_local"):
        s.expected_shortfall()


def test_main_es_flag_parses():
    from copula_var.main import build_parser
    base = ["--prices", "p.csv", "--tickers", "A", "B", "--start", "2009-04-15"]
    assert build_parser().parse_args(base).es is False
    assert build_parser().parse_args(base + ["--es"]).es is True
