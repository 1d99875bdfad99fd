"""The predictive distribution under per-date copula parameters and weights on the device
(cvq_dynamic_distribution) against plans built per date (the definition: cvq_distribution on a plan
created with date t's parameters and weights), against the numpy checker
tests/distribution_reference.py on the one-date Problems, and through every layer: plan, device
mode, backtest, driver, CLI.  Inputs: tests/dynamic_cases.py; the ladder is
tests/test_distribution_gpu.py's.

Against a per-date plan, and between calls, everything is np.array_equal.  Against the checker the
tolerances are the project's slab bar (tests/test_distribution_gpu.py): mass rtol 1e-10, atol 1e-15;
|m1 - ref| <= 1e-10 * m1_abs + 1e-15; a ratio of two masses (the PIT) rtol 3e-10."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import archimedean_reference as A
import distribution_reference as D
import dynamic_cases as DC
import dynamic_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

SLAB_RTOL, SLAB_ATOL = 1e-10, 1e-15
RATIO_RTOL = 3e-10
INF = float("inf")
NAN = float("nan")
LADDER = np.array([-100.0, -7.5, -3.0, -2.0, -1.0, 0.0, 0.5, 2.0, INF])
LADDER64 = np.concatenate(([-100.0], np.linspace(-6.0, 3.0, 63), [INF]))       # 64 ascending bins: the LDS bound
STRATEGIES = ["compact", "sorted", "sweep", "direct", "prefix"]
ALL = list(DC.CASES) + list(DC.EDGES)
# (golden, kind, theta path): the product-form kinds, thetas inside the supported ranges
# (Frank (0, 32], Joe [1, 16])
ARCHIMEDEAN = {"cfg5_n64_frank": ("cfg5_n64", "frank", (0.5, 2.0, 6.0, 12.0, 20.0, 30.0)),
               "cfg4_k4_n16_joe_survival": ("cfg4_k4_n16", "joe_survival", (1.0, 1.5, 2.0, 6.0))}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(base Problem, copula_params_t, weights_t, ptf_mean_t, one-date Problems); read-only."""
    if name not in ARCHIMEDEAN:
        return DC.problem(name)
    golden, kind, thetas = ARCHIMEDEAN[name]
    z = load_golden(golden)
    T = len(thetas)
    P = A.problem_of(z, kind, thetas[2], slice(0, T))
    cp = np.array(thetas, dtype=np.float64)[:, None]
    w = (R.W2 if P.dim == 2 else R.W3)[:T].copy()
    return P, cp, w, R.means(T), tuple(R.one_date(P, t, cp[t], w[t]) for t in range(T))


@functools.lru_cache(maxsize=None)
def _batch(name):
    """The device's (mass, m1) of a case on LADDER: computed once, shared, read-only."""
    P, cp, w, _, _ = _problem(name)
    p = DC.plan_of(P)
    try:
        return p.dynamic_distribution(LADDER, cp, w)
    finally:
        p.close()


@functools.lru_cache(maxsize=None)
def _reference(name, ladder="LADDER"):
    """bin_moments of every one-date Problem, stacked: (m0, m1, m1_abs), each (T, B)."""
    edges = {"LADDER": LADDER, "LADDER64": LADDER64}[ladder]
    per = [D.bin_moments(Pt, edges) for Pt in _problem(name)[4]]
    return tuple(np.concatenate([r[k] for r in per], axis=0) for k in range(3))


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _rows(res, idx):
    return [np.ascontiguousarray(a[idx]) for a in res]


def _check(got, ref, what=""):
    """Device (mass, m1) against the checker's (m0, m1, m1_abs) at the slab bar."""
    m0, m1, m1a = ref
    print(what, "mass rel", np.max(np.abs(got[0] - m0) / np.maximum(np.abs(m0), 1e-300)),
          "m1 err / m1_abs", np.max(np.abs(got[1] - m1) / np.maximum(m1a, 1e-300)))
    assert got[0].shape == m0.shape and got[1].shape == m1.shape
    np.testing.assert_allclose(got[0], m0, rtol=SLAB_RTOL, atol=SLAB_ATOL)
    assert np.all(np.abs(got[1] - m1) <= 1e-10 * m1a + 1e-15)


def _set_dates(p, P, idx):
    p.set_dates((P.fbs[idx], P.pi[idx]) if P.model == "msm" else [P.sigma[idx]])


def _per_date_plans(dates, edges, per_date_edges=False):
    """cvq_distribution on a fresh plan per date, given that date alone: the definition."""
    rows = []
    for t, Pt in enumerate(dates):
        p = DC.plan_of(Pt)
        try:
            rows.append(p.distribution(edges[t:t + 1] if per_date_edges else edges))
        finally:
            p.close()
    return [np.concatenate([r[k] for r in rows], axis=0) for k in range(2)]


# ------------------------------------------------------------------ 1. per-date plans
@pytest.mark.parametrize("name", ALL + list(ARCHIMEDEAN))
def test_bit_identical_to_per_date_plans(name):
    """[t] is cvq_distribution on a fresh plan built with date t's parameters and weights, fed date
    t alone, bit for bit (mass and m1)."""
    got = _batch(name)
    want = _per_date_plans(_problem(name)[4], LADDER)
    assert _same(got, want), name
    assert np.all(got[0][:, 2:6] > 0.0)               # the ladder's inner bins hold mass: the test sees nodes


# ------------------------------------------------------------------ 2. checker parity
@pytest.mark.parametrize("name", ALL)
def test_checker_parity(name):
    P, cp, w, pm, dates = _problem(name)
    ref = _reference(name)
    assert np.all(ref[0][:, 2:6] > 0.0)
    _check(_batch(name), ref, name)


@pytest.mark.parametrize("name", ["cfg2_n64", "cfg5_n64_gumbel", "garch3d_student_n16", "2d_n130"])
def test_dynamic_pit(name):
    """backtest.pit under per-date parameters, weights and means against the checker's PIT of
    every one-date Problem at that date's mean; a NaN realised return gives a NaN PIT."""
    from copula_var import backtest as B
    P, cp, w, pm, dates = _problem(name)
    r = np.linspace(-1.5, 1.0, P.T) + pm
    ref = np.array([D.pit(Pt, r[t:t + 1], float(pm[t]))[0] for t, Pt in enumerate(dates)])
    rn = r.copy()
    rn[1] = NAN
    th = np.array([-3.0, -2.0, -1.0, 0.0, 1.0])
    p = DC.plan_of(P)
    try:
        u = B.pit(p, r, pm, copula_params=cp, weights=w)
        un = B.pit(p, rn, pm, copula_params=cp, weights=w)
        static = B.pit(p, r, 0.0)
        F, total = B.predictive_cdf(p, th, pm, copula_params=cp, weights=w)
        centred = np.broadcast_to(th, (P.T, th.size)) - pm[:, None]
        mass, _ = p.dynamic_distribution(np.column_stack((np.full(P.T, -100.0), centred, np.full(P.T, INF))), cp, w)
    finally:
        p.close()
    print("pit rel", np.max(np.abs(u - ref) / ref), "range", u.min(), u.max())
    np.testing.assert_allclose(u, ref, rtol=RATIO_RTOL, atol=0.0)
    assert 0.0 < u.min() and u.max() < 1.0
    assert np.isnan(un[1]) and np.array_equal(np.delete(un, 1), np.delete(u, 1))
    assert not np.array_equal(u, static)
    # the CDF at thresholds th is the running sum over each date's ladder th - mean_t
    tot = mass.sum(axis=1)
    assert np.array_equal(total, tot) and np.array_equal(F, np.cumsum(mass[:, :-1], axis=1) / tot[:, None])
    assert np.all(np.diff(F, axis=1) >= 0.0) and np.all((F >= 0.0) & (F <= 1.0))


# ------------------------------------------------------------------ 3. degenerate forms
@pytest.mark.parametrize("name", ["cfg2_n64", "msm_plackett_n64", "cfg5_n64_gumbel", "cfg4_k4_n16"])
def test_degenerate_forms(name):
    P, cp, w, _, _ = _problem(name)
    own = np.tile(np.asarray(P.copula_params, dtype=np.float64).reshape(-1), (P.T, 1))
    p = DC.plan_of(P)
    try:
        plain = p.distribution(LADDER)
        both_none = p.dynamic_distribution(LADDER)
        own_values = p.dynamic_distribution(LADDER, own, np.tile(P.w, (P.T, 1)))
        params_only = p.dynamic_distribution(LADDER, cp, None)
        weights_only = p.dynamic_distribution(LADDER, None, w)
    finally:
        p.close()
    assert _same(both_none, plain)                    # both None: cvq_distribution
    assert _same(own_values, plain)                   # the plan's own values as arrays
    assert _same(params_only, _per_date_plans([R.one_date(P, t, cp[t], P.w) for t in range(P.T)], LADDER))
    assert _same(weights_only, _per_date_plans([R.one_date(P, t, P.copula_params, w[t]) for t in range(P.T)],
                                               LADDER))
    assert not _same(params_only, plain) and not _same(weights_only, plain)


# ------------------------------------------------------------------ 4. chunk and wave edges
@pytest.mark.parametrize("name", list(DC.EDGES))
def test_chunk_and_wave_edges_64_bins(name):
    """2-D n = 70: 2 chunks of 64 rows, the second with 6 live rows; n = 130: 3 chunks, the last
    with 2 rows; 3-D n = 17: 289 rows, a second 256-row chunk of 33.  A 64-bin ladder (the LDS
    bound) against the checker, against 64 one-bin calls and against a permuted order."""
    P, cp, w, _, _ = _problem(name)
    order = np.random.default_rng(5).permutation(64)
    p = DC.plan_of(P)
    try:
        full = p.dynamic_distribution(LADDER64, cp, w)
        singles = [p.dynamic_distribution(LADDER64[b:b + 2], cp, w) for b in range(64)]
        scattered = []
        for sel in (order[:32], order[32:]):          # even bins: 32 of the ladder's bins in the permutation's order
            pairs = np.empty(65)
            pairs[0:64:2], pairs[1:64:2], pairs[64] = LADDER64[sel], LADDER64[sel + 1], INF
            scattered.append(p.dynamic_distribution(pairs, cp, w))
    finally:
        p.close()
    _check(full, _reference(name, "LADDER64"), name)
    for b in range(64):
        assert np.array_equal(singles[b][0][:, 0], full[0][:, b]), b
        assert np.array_equal(singles[b][1][:, 0], full[1][:, b]), b
    for got, sel in zip(scattered, (order[:32], order[32:])):
        assert np.array_equal(got[0][:, 0:64:2], full[0][:, sel])
        assert np.array_equal(got[1][:, 0:64:2], full[1][:, sel])


# ------------------------------------------------------------------ 5. bin grouping
def test_bin_grouping():
    """n = 130 has 3 row chunks.  4 dates: 12 workgroups, one bin per group.  Tiled to 6 dates: 18
    workgroups, 57 groups wanted, so a group serves two bins.  Tiled to 342 dates: 1026 workgroups,
    no grouping.  A date's row is the same in all three."""
    P, cp, w, _, _ = _problem("2d_n130")
    assert P.T == 4
    p = DC.plan_of(P)
    try:
        base = p.dynamic_distribution(LADDER64, cp, w)
        for T in (6, 342):
            idx = np.arange(T) % P.T
            _set_dates(p, P, idx)
            got = p.dynamic_distribution(LADDER64, cp[idx], w[idx])
            assert _same(got, _rows(base, idx)), T
    finally:
        p.close()
    _check(base, _reference("2d_n130", "LADDER64"), "2d_n130")


# ------------------------------------------------------------------ 6. independence
@pytest.mark.parametrize("name", ["cfg2_n64", "garch3d_student_n16"])
def test_independent_of_the_batch(name):
    z = load_golden(DC.CASES[name][0])
    P, cp, w, _, _ = _problem(name)
    got = _batch(name)
    p = DC.plan_of(P)
    try:
        before, _ = p.calc_var(float(z["ptf_mean"]))                # the solve on these dates
        assert _same(p.dynamic_distribution(LADDER, cp, w), got)    # a second run (another plan, another call)
        assert _same(p.dynamic_distribution(LADDER, cp, w), got)
        after, _ = p.calc_var(float(z["ptf_mean"]))                 # the solve state is intact
        assert np.array_equal(before, after, equal_nan=True)
        assert p._wide is None
        perm = np.roll(np.arange(P.T)[::-1], 1)                     # the dates with their records, permuted
        _set_dates(p, P, perm)
        assert _same(p.dynamic_distribution(LADDER, cp[perm], w[perm]), _rows(got, perm))
        for t in (0, P.T - 1, 2):                                   # T = 1
            _set_dates(p, P, slice(t, t + 1))
            assert _same(p.dynamic_distribution(LADDER, cp[t:t + 1], w[t:t + 1]), _rows(got, slice(t, t + 1)))
        p.enable_timing(("moments",))                               # timed under kind 5
        p.dynamic_distribution(LADDER, cp[t:t + 1], w[t:t + 1])
        ms, launches = p.kernel_time("moments")
        assert launches == 1 and ms > 0.0
    finally:
        p.close()


# ------------------------------------------------------------------ 7. per-date ladders
def _per_date_ladder(T):
    edges = LADDER[None, :] + 0.013 * np.arange(T)[:, None]         # a different ladder on each date
    edges[1, 3] = NAN                                               # a NaN edge: bins 2 and 3 empty
    edges[2, 3], edges[2, 4] = -1.0, -2.0                           # a descending pair: bin 3 empty
    edges[3, 5] = edges[3, 4]                                       # a repeated edge: bin 4 empty
    edges[4, 0], edges[4, 1] = -INF, -3.2                           # -inf as the first edge
    edges[5] = [INF, -INF, -2.0, -2.0, NAN, 0.0, INF, INF, -INF]    # (inf, -inf] and (inf, inf]: empty
    return edges


def test_per_date_ladders_host_and_device():
    import torch
    name = "cfg2_n64"
    P, cp, w, _, dates = _problem(name)
    edges = _per_date_ladder(P.T)
    B = edges.shape[1] - 1
    want = _per_date_plans(dates, edges, per_date_edges=True)
    ref = [np.concatenate([D.bin_moments(Pt, edges[t:t + 1])[k] for t, Pt in enumerate(dates)], axis=0)
           for k in range(3)]
    p = DC.plan_of(P)
    try:
        host = p.dynamic_distribution(edges, cp, w)
        two = p.dynamic_distribution(edges[:, :3], cp, w)           # two bins per date: the PIT's shape
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            d_edges = torch.tensor(edges, dtype=torch.float64, device=dev)
            mass, m1 = (torch.full((P.T, B), -1.0, dtype=torch.float64, device=dev) for _ in range(2))
            p.set_stream(stream.cuda_stream)
            p.dynamic_distribution_device(d_edges.data_ptr(), B, mass.data_ptr(), m1.data_ptr(), cp, w)
        stream.synchronize()
    finally:
        p.close()
    assert _same(host, want)
    _check(host, ref, "per-date ladders")
    assert np.array_equal(mass.cpu().numpy(), host[0]) and np.array_equal(m1.cpu().numpy(), host[1])
    for t, b in ((1, 2), (1, 3), (2, 3), (3, 4), (5, 0), (5, 2), (5, 3), (5, 4), (5, 6), (5, 7)):
        assert host[0][t, b] == 0.0 and host[1][t, b] == 0.0, (t, b)    # exactly (0, 0)
    assert host[0][5, 1] > 0.0 and host[0][5, 5] > 0.0              # (-inf, -2] and (0, inf]
    assert host[0][4, 0] > 0.0                                      # (-inf, -3.2]
    assert np.array_equal(two[0], host[0][:, :2]) and np.array_equal(two[1], host[1][:, :2])


# ------------------------------------------------------------------ 8. every strategy
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_every_strategy(strategy):
    P, cp, w, _, _ = _problem("cfg2_n64")
    p = DC.plan_of(P, strategy)
    try:
        assert p.strategy == strategy
        assert _same(p.dynamic_distribution(LADDER, cp, w), _batch("cfg2_n64"))   # reaches +inf: no v_cap limit
        assert p._wide is None                        # no sibling: the plan itself
    finally:
        p.close()


# ------------------------------------------------------------------ 9. validation
SENTINEL = -12345.0


def _refused(p, T, code, text, t=None, *, cp=None, w=None, edges=LADDER, nb=None, per_date=0):
    """One refused call: its status, its message (with the offending date) and untouched outputs."""
    from copula_var import _native as N
    e = N.f64(edges)
    nb = e.shape[-1] - 1 if nb is None else nb
    out = [np.full((T, 64), SENTINEL) for _ in range(2)]
    arr = [None if a is None else N.f64(a) for a in (cp, w)]
    rc = N.lib().cvq_dynamic_distribution(p._h if p is not None else None,
                                          *[N.ptr(a) if a is not None else None for a in arr], N.ptr(e), nb,
                                          per_date, N.ptr(out[0]), N.ptr(out[1]), N.MEM_HOST)
    msg = (N.lib().cvq_last_error() or b"").decode()
    print(rc, msg)
    assert rc == code and text in msg, (rc, msg)
    if t is not None:
        assert msg.endswith(f"at date {t}"), msg
    assert all(np.all(o == SENTINEL) for o in out)


def _mod(a, t, k, v):
    b = np.array(a, dtype=np.float64)
    b[t, k] = v
    return b


def test_validation_student():
    from copula_var import _native as N
    P, cp, w, _, _ = _problem("cfg2_n64")
    T, inv, uns = P.T, N.CVQ_ERR_INVALID, N.CVQ_ERR_UNSUPPORTED
    p = DC.plan_of(P)
    try:
        for bad in (NAN, INF):
            _refused(p, T, inv, "finite", 3, cp=_mod(cp, 3, 1, bad), w=w)
            _refused(p, T, inv, "finite", 4, cp=cp, w=_mod(w, 4, 1, bad))
        _refused(p, T, inv, "correlation", 2, cp=_mod(cp, 2, 1, 1.0))
        _refused(p, T, inv, "correlation", 1, cp=_mod(_mod(cp, 1, 1, -1.5), 4, 1, 2.0))   # the first offender
        _refused(p, T, inv, "nu", 0, cp=_mod(cp, 0, 0, 0.0))
        _refused(p, T, inv, "nu", 3, cp=_mod(cp, 3, 0, -2.0))
        _refused(p, T, uns, "nu", 5, cp=_mod(cp, 5, 0, cp[5, 0] + 0.5))                   # not the plan's nu
        for bad in (0.0, -0.5):
            _refused(p, T, uns, "> 0", 2, w=_mod(w, 2, 0, bad))
        # a bad record and a bad weight on different dates: the earlier date is named
        _refused(p, T, uns, "> 0", 1, cp=_mod(cp, 4, 1, 1.0), w=_mod(w, 1, 0, 0.0))
        # the distribution's own checks come first, whatever the per-date values
        bad_cp = _mod(cp, 0, 1, NAN)
        for nb in (0, 65):
            _refused(p, T, inv, "n_bins", cp=bad_cp, nb=nb)
        _refused(p, T, inv, "per_date", cp=bad_cp, per_date=2)
        _refused(None, T, inv, "plan is NULL", cp=bad_cp)
        out = np.full((T, 8), SENTINEL)
        for edges, mass in ((None, N.ptr(out)), (N.ptr(N.f64(LADDER)), None)):
            assert N.lib().cvq_dynamic_distribution(p._h, N.ptr(N.f64(bad_cp)), None, edges, 8, 0, mass, None,
                                                    N.MEM_HOST) == inv
            assert b"NULL argument" in N.lib().cvq_last_error() and np.all(out == SENTINEL)
        # the engine's own shape checks, and the library's message through ValueError
        with pytest.raises(ValueError, match="shape"):
            p.dynamic_distribution(LADDER, cp[:-1])
        with pytest.raises(ValueError, match="shape"):
            p.dynamic_distribution(LADDER, None, R.W3)
        with pytest.raises(ValueError, match="shape"):
            p.dynamic_distribution(np.zeros((P.T + 1, 3)), cp, w)
        with pytest.raises(ValueError, match="at date 2"):
            p.dynamic_distribution(LADDER, _mod(cp, 2, 1, 1.0))
        assert _same(p.dynamic_distribution(LADDER, cp, w), _batch("cfg2_n64"))           # and the plan still works
    finally:
        p.close()


def test_validation_other_kinds():
    from copula_var import _native as N
    from copula_var.engine import QuadraturePlan
    inv, uns = N.CVQ_ERR_INVALID, N.CVQ_ERR_UNSUPPORTED
    P, cp, w, _, _ = _problem("cfg5_n64_gumbel")
    p = DC.plan_of(P)
    try:
        th = cp.copy()
        th[3, 0] = 0.99
        _refused(p, P.T, inv, "theta", 3, cp=th)
        th[2, 0] = 16.5
        _refused(p, P.T, uns, "theta", 2, cp=th)
        th[1, 0] = NAN
        _refused(p, P.T, inv, "finite", 1, cp=th)
    finally:
        p.close()
    P, cp, w, _, _ = _problem("cfg5_n64_frank")
    p = DC.plan_of(P)
    try:
        _refused(p, P.T, inv, "Frank theta", 4, cp=_mod(cp, 4, 0, 0.0))
        _refused(p, P.T, uns, "Frank theta", 2, cp=_mod(cp, 2, 0, -1.0))
        _refused(p, P.T, uns, "Frank theta", 5, cp=_mod(cp, 5, 0, 32.5))
    finally:
        p.close()
    P, cp, w, _, _ = _problem("cfg4_k4_n16_joe_survival")
    p = DC.plan_of(P)
    try:
        _refused(p, P.T, inv, "Joe theta", 1, cp=_mod(cp, 1, 0, 0.5))
        _refused(p, P.T, uns, "Joe theta", 3, cp=_mod(cp, 3, 0, 16.5))
    finally:
        p.close()
    P, cp, w, _, _ = _problem("cfg4_k4_n16")                        # 3-D Gaussian
    p = DC.plan_of(P)
    try:
        bad = cp.copy()
        bad[2] = (0.9, -0.9, 0.9)                                    # every |rho| < 1, not positive definite
        _refused(p, P.T, inv, "positive definite", 2, cp=bad)
        bad[1] = (0.2, 1.0, 0.2)
        _refused(p, P.T, inv, "correlation", 1, cp=bad)
    finally:
        p.close()
    # before cvq_set_dates
    p = QuadraturePlan(P.model, P.copula, P.dim, P.x, P.step, P.dens, P.combos, P.w, P.copula_params,
                       vol_states=P.uvs)
    try:
        _refused(p, P.T, N.CVQ_ERR_STATE, "cvq_set_dates")
    finally:
        p.close()


# ------------------------------------------------------------------ 10. device mode
def test_device_mode_on_a_torch_stream():
    import torch
    P, cp, w, _, _ = _problem("cfg2_n64")
    host = _batch("cfg2_n64")
    B = LADDER.size - 1
    p = DC.plan_of(P)
    try:
        want_rev = p.dynamic_distribution(LADDER, cp[::-1].copy(), w)
        want_plain = p.distribution(LADDER)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            out, rev, plain = (torch.full((2, P.T, B), -1.0, dtype=torch.float64, device=dev) for _ in range(3))
            only = torch.full((P.T, B), -1.0, dtype=torch.float64, device=dev)
            p.set_stream(stream.cuda_stream)
            p.dynamic_distribution_device(LADDER, B, out[0].data_ptr(), out[1].data_ptr(), copula_params=cp.copy(),
                                          weights=w.copy())
            p.dynamic_distribution_device(LADDER, B, only.data_ptr(), copula_params=cp, weights=w)   # m1_out NULL
            # no host synchronisation before the next calls: their records go through other staging
            # buffers (or the same, once its upload is done) and overwrite the device records in
            # stream order; the host arrays of the calls above are gone by now
            p.dynamic_distribution_device(LADDER, B, rev[0].data_ptr(), rev[1].data_ptr(),
                                          copula_params=cp[::-1].copy(), weights=w.copy())
            p.dynamic_distribution_device(LADDER, B, plain[0].data_ptr(), plain[1].data_ptr())
        stream.synchronize()
        with pytest.raises(ValueError):
            p.dynamic_distribution_device(LADDER[:-1], B, only.data_ptr())
    finally:
        p.close()
    for k in range(2):
        assert np.array_equal(out[k].cpu().numpy(), host[k])
        assert np.array_equal(rev[k].cpu().numpy(), want_rev[k])
        assert np.array_equal(plain[k].cpu().numpy(), want_plain[k])
    assert np.array_equal(only.cpu().numpy(), host[0])


# ------------------------------------------------------------------ 11. driver and CLI
def _driver(z):
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from copula_var.utils.factory import ValueAtRiskCalculationFactory
    from driver_util import inject
    tickers, start, kw = inject(z)
    calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=str(z["copula"]),
                                                               estimation_type=str(z["model"]))
    return ValueAtRiskCalcualtion(tickers, start, int(z["n_in"]), calc, None, num_points=int(z["num_points"]),
                                  weights=z["weights"], copula_params=z["copula_params"], **kw)


def _plan_level_pit(plan, realised, mean, cp, w):
    edges = np.column_stack((np.full(realised.size, -100.0), realised - mean, np.full(realised.size, INF)))
    mass, _ = plan.dynamic_distribution(edges, cp, w)
    return mass[:, 0] / (mass[:, 0] + mass[:, 1])


def test_driver_dynamic_pit_and_distribution():
    z = load_golden("cfg2_n64")
    P, cp, w, _, dates = _problem("cfg2_n64")
    v = _driver(z)
    try:
        T = v.plan.T
        cpt, wt = np.tile(z["copula_params"], (T, 1)), np.tile(z["weights"], (T, 1))
        cpt[:P.T], wt[:P.T] = cp, w
        n_in = int(z["n_in"])
        realised = z["returns"][n_in:n_in + T].mean(axis=1)
        means = np.array([v.mean_returns[t] for t in v.tickers])
        pm = np.array([np.sum(means * wp) for wp in wt])            # the loader's formula per date
        u = v.calc_dynamic_pit(realised, cpt, wt)
        want = _plan_level_pit(v.plan, realised, pm, cpt, wt)
        same, static = v.calc_dynamic_pit(realised), v.calc_pit(realised)
        mass, m1 = v.calc_dynamic_distribution(LADDER, cpt, wt)
        centred = v.plan.dynamic_distribution(LADDER[None, :] - pm[:, None], cpt, wt)
        var, es = v.calc_dynamic_quantiles((0.05,), cpt, wt)
        table = v.dynamic_backtest(realised, 0.05, var[:, 0], es=es[:, 0], copula_params=cpt, weights=wt)
        kept = v.last_dynamic_pit
    finally:
        v.close()
    assert np.array_equal(u, want) and np.all((u > 0.0) & (u < 1.0))
    assert np.array_equal(same, static)               # nothing per date: the static model's PIT
    assert np.array_equal(u[P.T:], static[P.T:]) and not np.array_equal(u[:P.T], static[:P.T])
    assert _same((mass, m1), centred)
    ref = np.array([D.pit(Pt, realised[t:t + 1], float(pm[t]))[0] for t, Pt in enumerate(dates)])
    np.testing.assert_allclose(u[:P.T], ref, rtol=RATIO_RTOL, atol=0.0)
    assert np.array_equal(kept, u) and table["berkowitz"]["n"] == T and "z2" in table
    assert table["hits"] == int(np.sum(realised < var[:, 0]))


def test_cli_dynamic_backtest(tmp_path, capsys, monkeypatch):
    import pandas as pd
    from copula_var import main as M, synthetic
    from copula_var.utils.calc_var_class import ValueAtRiskCalcualtion
    from driver_util import inject
    z = load_golden("garch_student_n64")
    tickers, start, _ = inject(z)                                  # fitted GARCH parameters from the cache
    csv, out, static_out = tmp_path / "returns.csv", tmp_path / "dyn.csv", tmp_path / "static.csv"
    synthetic.returns_frame(z["returns"]).to_csv(csv)
    seen = []                                                      # the driver call the CLI makes
    inner = ValueAtRiskCalcualtion.dynamic_backtest

    def record(self, realised, alpha, var, es=None, copula_params=None, weights=None):
        table = inner(self, realised, alpha, var, es, copula_params, weights)
        want = _plan_level_pit(self.plan, np.asarray(realised, dtype=np.float64), self.dynamic_ptf_mean(weights),
                               copula_params, weights)
        seen.append((alpha, np.array(copula_params), np.array(weights), want, self.calc_pit(realised)))
        return table

    monkeypatch.setattr(ValueAtRiskCalcualtion, "dynamic_backtest", record)
    # the golden's copula parameters instead of the static IFM fit (seconds, and not this test's subject)
    monkeypatch.setattr(ValueAtRiskCalcualtion, "calc_copula_params", lambda self: z["copula_params"])
    T = len(z["returns"]) - int(z["n_in"])
    base = ["--prices", str(csv), "--returns", "--tickers", *tickers, "--start", start, "--n-in",
            str(int(z["n_in"])), "--copula", "student", "--estimation", "garch", "--num-points", "64",
            "--exact-levels", "0.05", "0.25", "--backtest"]
    assert M.main(base + ["--rolling-copula", "60", "--refit-every", str(max(T // 2, 1)), "--drift-weights",
                          "--out", str(out)]) == 0
    err = capsys.readouterr().err
    assert M.main(base + ["--out", str(static_out)]) == 0
    static_err = capsys.readouterr().err
    (alpha, cpt, wt, want, static_pit), = seen                     # one sweep serves every level
    f = pd.read_csv(out, index_col=0, float_precision="round_trip")
    T = len(f)
    assert alpha == 0.05 and cpt.shape == (T, 2) and wt.shape == (T, 2) and len(np.unique(wt[:, 0])) > 1
    g = pd.read_csv(static_out, index_col=0, float_precision="round_trip")
    realised = f["portfolio_return"].to_numpy()
    titles = re.findall(r"backtest garch/student (.*?): alpha ([0-9.]+), (\d+) dates \((\d+) dropped\), hits (\d+) ",
                        err)
    assert [t[0] for t in titles] == ["VaR", "exact VaR at 0.05", "exact VaR at 0.25", "dynamic VaR at 0.05",
                                      "dynamic VaR at 0.25"]
    for t, lv in zip(titles[3:], ("0.05", "0.25")):
        dv = f[f"dvar_garch_{lv}"].to_numpy()
        assert float(t[1]) == float(lv) and int(t[2]) == T and int(t[4]) == int(np.sum(realised < dv))
        assert np.array_equal(f[f"dhit_garch_{lv}"].to_numpy(), (realised < dv).astype(float))
    assert err.count("Berkowitz") == 5 and err.count("Z2") == 4    # Z2: the exact and dynamic tables carry an ES
    assert np.array_equal(f["dpit_garch"].to_numpy(), want) and np.all((want > 0.0) & (want < 1.0))
    assert np.array_equal(f["pit_garch"].to_numpy(), static_pit) and not np.array_equal(want, static_pit)
    # without the dynamic flags: the parent's tables and columns
    assert "dynamic" not in static_err
    assert re.findall(r"backtest garch/student (.*?): alpha", static_err) == \
        ["VaR", "exact VaR at 0.05", "exact VaR at 0.25"]
    assert list(g.columns) == ["var_garch", "qvar_garch_0.05", "qes_garch_0.05", "qvar_garch_0.25", "qes_garch_0.25",
                               "pit_garch", "hit_garch", "portfolio_return"]
    extra = ["dvar_garch_0.05", "des_garch_0.05", "dvar_garch_0.25", "des_garch_0.25", "dparam_garch_0",
             "dparam_garch_1"]
    assert list(f.columns) == list(g.columns)[:5] + extra + ["pit_garch", "hit_garch", "dpit_garch",
                                                              "dhit_garch_0.05", "dhit_garch_0.25", "portfolio_return"]
    for c in g.columns:                               # the shared columns carry the same numbers
        assert np.array_equal(f[c].to_numpy(), g[c].to_numpy(), equal_nan=True), c
