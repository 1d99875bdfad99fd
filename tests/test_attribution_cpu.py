"""Risk attribution without a GPU: the numpy checker (tests/attribution_reference.py) on the
goldens and on unequal weights, the library's new symbols and their host-side validation, the
sharded contribution exchange on gloo ranks, the CLI flag, and the premise of the GPU suite's
band test (the share of cfg1 dates whose default band holds no node)."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import attribution_reference as A
import es_reference as E
from conftest import GOLDEN_CASES, load_golden

K = 30                                   # bisection budget of the oracle's sharded restatement
SMALL = [c for c in GOLDEN_CASES if c not in ("cfg2_n256", "cfg3_n128")]
UNEQUAL = {2: (0.7, 0.3), 3: (0.5, 0.3, 0.2)}
BAND = 0.25                              # var_contributions' default band


def _reweighted(z):
    z = dict(z)
    z["weights"] = np.array(UNEQUAL[int(z["dim"])])
    return z


def _check_identities(P, var, ptf):
    """sum_c wa mx = m1 within 1e-13 m1_abs (dim + 1 roundings of terms bounded by m1_abs, plus
    the two sums' own ~1e-15 m1_abs: pairwise summation); m0 bit-equal; rows sum to es - ptf_mean."""
    es, m0e, m1, m1a = E.expected_shortfall(P, var, ptf)
    contrib, m0, mx, mxa = A.es_contributions(P, var, ptf)
    wa = A.axis_weights(P)
    assert np.array_equal(m0, m0e)
    assert np.all(np.abs(mx) <= mxa)
    assert np.all(np.abs(mx @ wa - m1) <= 1e-13 * m1a)
    assert np.all(m0 > 0) and np.isfinite(contrib).all()
    assert np.all(np.abs(contrib.sum(axis=1) - (es - ptf)) <= 1e-13 * np.abs(wa * mxa).sum(axis=1) / m0)
    return contrib


@pytest.mark.parametrize("case", SMALL)
def test_checker_identities_on_goldens(case):
    z = load_golden(case)
    _check_identities(E.problem_of(z), z["var"], float(z["ptf_mean"]))


@pytest.mark.parametrize("case", ["cfg2_n64", "garch_student_n64", "cfg4_k4_n16", "garch3d_student_n16"])
def test_checker_identities_on_unequal_weights(case):
    """Unequal weights tell wa from the weights in input order: the additivity holds with wa and
    fails with the unpermuted weights."""
    z = _reweighted(load_golden(case))
    P = E.problem_of(z)
    ptf = float(z["ptf_mean"])
    var = np.full(P.T, -2.5) + ptf                  # any level: the identities hold on every slab
    _check_identities(P, var, ptf)
    _, _, m1, m1a = E.expected_shortfall(P, var, ptf)
    _, _, mx, _ = A.es_contributions(P, var, ptf)
    assert np.all(np.abs(mx @ P.w - m1) > 1e-6 * m1a)       # weights[k] is not asset k's weight (Q10)
    assert np.array_equal(A.axis_weights(P), np.roll(P.w, -1))


def test_checker_nan_and_empty():
    z = load_golden("cfg2_n64")
    P = E.problem_of(z)
    for row in ((np.nan, -3.0), (-3.0, np.nan), (-2.0, -2.0)):
        m0, mx, mxa = A.axis_moments(P, np.tile(row, (P.T, 1)))
        assert np.all(m0 == 0) and np.all(mx == 0) and np.all(mxa == 0)
    var = z["var"].copy()
    var[2] = np.nan
    ptf = float(z["ptf_mean"])
    contrib = A.es_contributions(P, var, ptf)[0]
    assert np.isnan(contrib[2]).all() and np.isfinite(np.delete(contrib, 2, axis=0)).all()
    contrib = A.es_contributions(P, z["var"], ptf, lower=0.0)[0]      # empty slab: m0 == 0
    assert np.isnan(contrib).all()


def test_band_premise_on_cfg1():
    """The default band on cfg1 (the GPU suite's band test): at most 10 % of the dates may hold no
    mass, and on the others the band's mean level lies inside the band."""
    z = load_golden("cfg1")
    P = E.problem_of(z)
    ptf = float(z["ptf_mean"])
    contrib, mean, m0, _, _ = A.var_contributions(P, z["var"], ptf, BAND)
    empty = m0 == 0.0
    print("cfg1: dates with an empty band", int(empty.sum()), "of", P.T)
    assert empty.mean() <= 0.10
    top = z["var"] - ptf
    assert np.all((top - BAND < mean[~empty]) & (mean[~empty] <= top[~empty]))
    assert np.isnan(contrib[empty]).all() and np.isfinite(contrib[~empty]).all()


def test_library_exports_the_entry_points():
    from copula_var import _native as N
    lib = N.lib()
    assert lib.cvq_version() >= 10400
    assert hasattr(lib, "cvq_slab_axis_moments") and hasattr(lib, "cvq_es_contributions")


def test_entry_points_validate_on_the_host():
    from copula_var import _native as N
    lib = N.lib()
    buf = np.zeros(8)
    a = N.CvqSolveArgs(0.05, -3.0, -3.5, -2.0, -7.5, 0.0, -100.0, 1e-6, 0.0)
    assert lib.cvq_slab_axis_moments(None, N.ptr(buf), N.ptr(buf), N.ptr(buf), N.MEM_HOST) == N.CVQ_ERR_INVALID
    assert lib.cvq_last_error()
    assert lib.cvq_es_contributions(None, C.byref(a), N.ptr(buf), N.ptr(buf), None, N.MEM_HOST) == \
        N.CVQ_ERR_INVALID
    assert lib.cvq_es_contributions(None, None, N.ptr(buf), N.ptr(buf), None, N.MEM_DEVICE) == N.CVQ_ERR_INVALID


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

        def contrib_local(var_block, contrib_block):
            contrib_block.copy_(torch.from_numpy(A.es_contributions(P, var_block.numpy(), ptf)[0]))

        s = ShardedVaR(T, K + 1, local, finalize, torch.device("cpu"), contrib_local=contrib_local, dim=P.dim)
        var = s.solve().numpy().copy()
        q.put((rank, (var, s.es_contributions().numpy().copy())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case,world", [("cfg1", 2), ("msm_gauss_n64", 3)])
def test_gloo_sharded_contributions_are_bit_identical(case, world):
    """World 2, and world 3 over the uneven T = 10 (blocks of 4, 4, 2: the last block's NaN padding
    never reaches the result): every rank holds the unsharded contributions bit for bit."""
    z = load_golden(case)
    ref = A.es_contributions(E.problem_of(z), z["var"], float(z["ptf_mean"]))[0]
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
    for var, contrib in out.values():
        assert np.array_equal(var, z["var"])
        assert contrib.shape == ref.shape and np.array_equal(contrib, ref)


def test_sharded_contributions_need_contrib_local():
    from copula_var.distributed import ShardedVaR
    s = ShardedVaR(4, 3, lambda h, sn: None, lambda b, v: None, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="contrib_local"):
        s.es_contributions()


def test_main_contributions_flag_parses():
    from copula_var.main import build_parser
    base = ["--prices", "p.csv", "--tickers", "A", "B", "--start", "2009-04-15"]
    assert build_parser().parse_args(base).contributions is False
    a = build_parser().parse_args(base + ["--contributions"])
    assert a.contributions is True
