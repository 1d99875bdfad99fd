"""Known-answer tests of the device-only node arithmetic (csrc/cvq_special.h) through cvq_special's
fn codes 4..16, against the 50-digit truths of tests/golden/node_kat.kat (tests/kat/gen_node_kat.py;
the points are tests/node_cases.py's).  No mpmath and no reference project here.

Bars: each helper's own documented claim, plus the 0.5 ulp of a correctly rounded result
(ULP = 2^-52 relative).  Below the normal range: the claim, plus one subnormal ulp for the
denormalising step and half of one for the rounded truth (_tol).  Measured on one MI355X as the
worst error over the helper's points, in units of its bar (the `MEASURED` lines of a run):

  helper                         bar                                  source of the claim                  measured
  exp_node                       1.4e-14 relative                     cvq_special.h exp_node               0.976
  exp_node7, exp2_node7          4.05e-11 relative                    the polynomials' own error, 4.045e-11
                                                                      (test_node_reference_cpu.py); the
                                                                      comments said 4.0e-11 and were corrected  0.999
  log_node                       4 ulp relative                       "< 1 ulp" fdlibm + "~1 ulp" rcp, x 2  0.120
  log_node_fast (b >= 1)         5e-13 absolute                       cvq_special.h log_node_fast          0.973
  fast_rcp, root_nu<6>           2 ulp                                "~1 ulp", x 2                        0.167, 0.193
  integer-m powers               (m + 4) / 2 ulp                      one rounding per multiply + the rcp  0.222 (pow_node),
                                                                                                           0.914 (pow_half_*)
  general powers                 1.4e-14 + |ex log b| ulp             exp_node + the exponent's rounding   0.949
  stdtrit_tab_int<6>             7e-14 relative                       DESIGN.md §5 (against mpmath)        0.082
  stdtrit_tab_bf                 7e-14; its tail just under p_split:  table 4e-14 + exp_node's 1.4e-14 in  0.982 (nu = 1),
                                 max(7e-14, 4e-14 + nu S 1.4e-14)     v = p^(1/nu), amplified (see         0.696 (nu = 30:
                                                                      _quantile_bar)                       1.10e-13 relative)

Two figures the code documented did not hold and were corrected there and in DESIGN.md §5, the code
being as designed: exp_node7 / exp2_node7 reach 4.045e-11 at their interval's ends (not 4.0e-11), and
stdtrit_tab_bf passes 7e-14 just under p_split from nu ~ 13 up (1.10e-13 at nu = 30).  nu = 126 has no
direct tables (fn 16 refuses it, as documented); its plans take stdtrit's refined path, fn 0, held here
to the same 7e-14 plus the absolute floor of Halley on log F (2^-52 F / pdf, within ulps of u = 1/2).
It first measured 1.03e-13 there (u = 0.9555): the Student constants lbeta and ln_k were differences of
double-precision lgammas, each half an ulp of ~195 off, which the complement branch amplifies tenfold at
its branch point.  They are now formed in long double (cvq_plan.hip build_timage); the same source run
on the host gives 1.4e-14 at nu = 126 after the change (1.03e-13 before); the device measures 0.161 of
the bar.
"""
import numpy as np
import pytest

import node_cases as NC

pytestmark = pytest.mark.gpu

LD = np.longdouble
ULP, HALF = 2.0 ** -52, 2.0 ** -53
EXP_BAR, EXP7_BAR, LOGFAST_ABS, QUANTILE_BAR = 1.4e-14, 4.05e-11, 5e-13, 7e-14


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.fail("GPU tests were selected but no HIP device / libcvq.so is available")


@pytest.fixture(scope="module")
def kat():
    return NC.load_kat()


def _special(fn, x, nu=0.0):
    from copula_var import _native as N
    return N.special(fn, x, nu=nu)


def _same_points(kat, name, pts):
    assert NC.digest(pts) == str(kat["sha_" + name]), f"{name}: the points differ from the fixture's (regenerate it)"


def _tol(tr, rel, absolute=0.0):
    """Allowed |device - truth|: (rel + 0.5 ulp) |truth| + absolute.  Under the normal range an ulp is the
    fixed 2^-1074 and the result is denormalised after the helper's last operation: one subnormal ulp for
    that step and half of one for the rounded truth take the place of the relative 0.5 ulp; the helper's
    own relative claim stays (1.4e-14 of 2e-308 is 60 subnormal ulps, so it cannot be dropped)."""
    a = np.abs(tr)
    return np.where(a < NC.MIN_NORMAL, rel * a + LD(1.5 * NC.TINY) + absolute, (rel + HALF) * a + absolute)


def _measure(label, dev, tr, tol):
    """Worst |dev - tr| / tol over finite truths; printed, then returned for the assertion."""
    err = np.abs(dev.astype(LD) - tr)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
        rel = np.where(tr != 0, err / np.abs(tr), 0.0)
    i = int(np.argmax(ratio)) if ratio.size else 0
    print(f"MEASURED {label} max {float(ratio.max(initial=0.0)):.3f} of bar "
          f"(max rel err {float(rel.max(initial=0.0)):.3e}, n = {ratio.size}, worst at index {i})")
    return float(ratio.max(initial=0.0))


def _check(label, dev, tr, tol):
    assert np.all(np.isfinite(dev)), f"{label}: non-finite results {dev[~np.isfinite(dev)][:4]}"
    assert _measure(label, dev, tr, tol) <= 1.0, label


# ------------------------------------------------------------------ exp
@pytest.mark.parametrize("fn,bar", [("exp_node", EXP_BAR), ("exp_node7", EXP7_BAR)])
def test_exp(kat, fn, bar):
    x = NC.exp_points()
    _same_points(kat, "exp", x)
    tr = NC.truth(kat, "exp")
    dev = _special(fn, x)
    nan, zero = np.isnan(x), x < -1075.0
    assert nan.sum() == 1 and zero.sum() >= 6
    assert np.all(np.isnan(dev[nan])), "NaN -> NaN"
    assert np.all(dev[zero] == 0.0) and not np.any(np.signbit(dev[zero])), "x < -1075 -> exactly +0"
    ok = ~nan & ~zero
    sub = ok & (np.abs(tr) < NC.MIN_NORMAL)
    assert sub.sum() >= 150, "the subnormal-result range is covered"
    _check(fn, dev[ok], tr[ok], _tol(tr[ok], bar))


def test_exp2(kat):
    x = NC.exp2_points()
    _same_points(kat, "exp2", x)
    tr = NC.truth(kat, "exp2")
    dev = _special("exp2_node7", x)
    nan, zero = np.isnan(x), x < -1075.5
    assert np.all(np.isnan(dev[nan])) and np.all(dev[zero] == 0.0) and zero.sum() >= 5
    ok = ~nan & ~zero
    assert (ok & (x == np.rint(x))).sum() >= 290, "exact integers are covered"
    _check("exp2_node7", dev[ok], tr[ok], _tol(tr[ok], EXP7_BAR))


# ------------------------------------------------------------------ log
def test_log_node(kat):
    b = NC.log_points()
    _same_points(kat, "log", b)
    tr = NC.truth(kat, "log")
    dev = _special("log_node", b)
    assert (b < NC.MIN_NORMAL).sum() >= 4, "subnormal arguments are covered"
    assert dev[b == 1.0].tolist() == [0.0]
    tol = (4 * ULP + HALF) * np.abs(tr)
    _check("log_node", dev, tr, tol)


def test_log_node_fast(kat):
    b_all = NC.log_points()
    _same_points(kat, "log", b_all)
    keep = b_all >= 1.0
    tr = NC.truth(kat, "log")[keep]
    dev = _special("log_node_fast", b_all[keep])
    _check("log_node_fast", dev, tr, LOGFAST_ABS + HALF * np.abs(tr))
    dense = NC.logdense_points()                     # the node power's base range [1, 2^21)
    _same_points(kat, "logdense", dense)
    tr = NC.truth(kat, "logdense")
    _check("log_node_fast dense [1, 2^21)", _special("log_node_fast", dense), tr, LOGFAST_ABS + HALF * np.abs(tr))
    _check("log_node dense [1, 2^21)", _special("log_node", dense), tr, (4 * ULP + HALF) * np.abs(tr))


# ------------------------------------------------------------------ reciprocal, root
def test_fast_rcp(kat):
    r = NC.rcp_points()
    _same_points(kat, "rcp", r)
    tr = NC.truth(kat, "rcp")
    dev = _special("fast_rcp", r)
    assert (np.abs(tr) < NC.MIN_NORMAL).sum() == 3
    _check("fast_rcp", dev, tr, _tol(tr, 2 * ULP))


def test_root_nu6(kat):
    p = NC.root_points()
    _same_points(kat, "root6", p)
    tr = NC.truth(kat, "root6")
    dev = _special("root_nu6", p, nu=6.0)
    assert (p < NC.MIN_NORMAL).sum() >= 4
    _check("root_nu<6>", dev, tr, _tol(tr, 2 * ULP))


# ------------------------------------------------------------------ powers
def _pow_bar(ex, m, b, tr):
    """Integer code m >= 0: (m + 4) / 2 ulp; m < 0 (general leg): 1.4e-14 + |ex log b| ulp."""
    if m >= 0:
        return _tol(tr, (m + 4) / 2.0 * ULP)
    return _tol(tr, EXP_BAR + np.abs(ex * np.log(b)) * ULP)


def _pow_points(kat):
    _same_points(kat, "pow", np.concatenate((NC.POW_B, NC.POW_NEG_EX, NC.POW_POS_EX,
                                             [b for m in range(2, 129) for b in NC.overflow_b(m)])))
    return NC.truth(kat, "pow_neg"), NC.truth(kat, "pow_pos"), NC.truth(kat, "pow_trip")


def _split_overflow(b, tr):
    """(regular, zeroed) masks of the 1e300 rule: b^(m/2) = 1 / truth against 1e300 with a 1e-6 margin
    (a point inside the margin is in neither)."""
    with np.errstate(divide="ignore"):
        r = 1.0 / tr
    over, under = r > LD(NC.OVERFLOW_R) * (1 + 1e-6), r < LD(NC.OVERFLOW_R) * (1 - 1e-6)
    assert (~(over | under)).sum() <= 1       # (1e6^50 = 1e300 sits on the edge: the squarings' rounding decides it)
    return under, over


def test_pow_node_integer(kat):
    """Every m in 0..128 (ex = -m/2): the squarings, the sqrt leg of odd m, the reciprocal, the 1e300
    overflow rule on both sides of its first b, +inf and NaN."""
    neg, _, trip = _pow_points(kat)
    worst = 0.0
    for m in range(129):
        ex = -m / 2.0
        assert NC.POW_NEG_EX[m] == ex
        extra = list(NC.overflow_b(m)) if m >= 2 else []
        b = np.concatenate((NC.POW_B, extra, [NC.INF, NC.NAN]))
        dev = _special("pow_node", b, nu=ex)
        nb = NC.POW_B.size
        tr = neg[m]
        reg, zero = _split_overflow(NC.POW_B, tr)
        assert np.all(dev[:nb][zero] == 0.0), (m, "b^(m/2) >= 1e300 -> 0")
        tol = _pow_bar(ex, m, NC.POW_B[reg], tr[reg])
        err = np.abs(dev[:nb][reg].astype(LD) - tr[reg])
        assert np.all(err <= tol), (m, NC.POW_B[reg][err > tol])
        worst = max(worst, float(np.max(err / tol)))
        if m >= 2:
            t = trip[m - 2]
            assert abs(LD(dev[nb]) - t) <= _pow_bar(ex, m, extra[0], np.array([t]))[0], (m, "just under the rule")
            assert dev[nb + 1] == 0.0, (m, "just over the rule -> 0")
        if m > 0:
            assert dev[-2] == 0.0 and np.isnan(dev[-1]), (m, "+inf -> 0, NaN -> NaN")
        else:
            assert dev[-2] == 1.0 and dev[-1] == 1.0, "b^0 = 1 for every b, as pow gives it"
    print(f"MEASURED pow_node integer m max {worst:.3f} of bar")


def test_pow_general(kat):
    """The general leg exp_node(ex log_node(b)): pow_node with a non-integer exponent and with
    node_m = 129 > 128, and pow_gen itself (also at an integer exponent)."""
    neg, _, _ = _pow_points(kat)
    b = np.concatenate((NC.POW_B, [NC.INF, NC.NAN]))
    nb = NC.POW_B.size
    for fn, rows in (("pow_node", (129, 130)), ("pow_gen", (129, 130, 131, 8, 1))):
        for row in rows:
            ex = NC.POW_NEG_EX[row]
            dev = _special(fn, b, nu=ex)
            assert dev[-2] == 0.0 and np.isnan(dev[-1]), (fn, ex, "+inf -> 0, NaN -> NaN")
            _check(f"{fn} ex = {ex}", dev[:nb], neg[row], _pow_bar(ex, -1, NC.POW_B, neg[row]))


def test_pow_half(kat):
    """pow_half_neg / pow_half_pos: m = 0..16, m = 17 (the general leg) and a non-integer exponent;
    pow_half_pos_c<7>."""
    neg, pos, _ = _pow_points(kat)
    b = NC.POW_B
    worst = {"pow_half_neg": 0.0, "pow_half_pos": 0.0}
    for m in range(18):
        code = m if m <= 16 else -1
        for fn, ex, tr in (("pow_half_neg", -m / 2.0, neg[m]), ("pow_half_pos", m / 2.0, pos[m])):
            dev = _special(fn, b, nu=ex)
            tol = _pow_bar(ex, code, b, tr)
            err = np.abs(dev.astype(LD) - tr)
            assert np.all(np.isfinite(dev)) and np.all(err <= tol), (fn, m, b[err > tol])
            worst[fn] = max(worst[fn], float(np.max(err / tol)))
    for fn, w in worst.items():
        print(f"MEASURED {fn} m = 0..17 max {w:.3f} of bar")
    assert NC.POW_NEG_EX[131] == -3.182 and NC.POW_POS_EX[18] == 3.182
    _check("pow_half_neg ex = -3.182", _special("pow_half_neg", b, nu=-3.182), neg[131], _pow_bar(-3.182, -1, b, neg[131]))
    _check("pow_half_pos ex = 3.182", _special("pow_half_pos", b, nu=3.182), pos[18], _pow_bar(3.182, -1, b, pos[18]))
    _check("pow_half_pos_c<7>", _special("pow_half_pos_c7", b), pos[7], _pow_bar(3.5, 7, b, pos[7]))
    inf_nan = np.array([NC.INF, NC.NAN])
    d = _special("pow_half_neg", inf_nan, nu=-3.0)
    assert d[0] == 0.0 and np.isnan(d[1])


# ------------------------------------------------------------------ quantiles
NO_DIRECT_TABLES = (126.0,)               # cvq_plan.hip build_timage: the quintic tables fail their 4e-14 host check


TABLE_BAR = 4e-14                         # cvq_special.h TConst: the quintic tables, host-verified


def _quantile_bar(nu, u, tr, tail_from_exp_node):
    """7e-14 relative.  stdtrit_tab_bf's tail (pp < p_split) reads its table at
    v = exp_node(log_node(pp) / nu): exp_node's 1.4e-14 in v is nu times that in p, and t moves by the
    elasticity S = p / (|t| pdf(t)) of it -- 4e-14 + nu S 1.4e-14, which passes 7e-14 from nu ~ 13 up
    just under p_split (computed here from the truth; DESIGN.md §5 carries the corrected figure)."""
    from scipy import stats
    bar = np.full(u.shape, QUANTILE_BAR)
    if tail_from_exp_node:
        pp = np.minimum(u, 1.0 - u)
        t = np.abs(tr.astype(np.float64))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            S = pp / (t * stats.t.pdf(t, nu))
        tail = (pp < NC.P_SPLIT) & np.isfinite(S)
        bar[tail] = np.maximum(QUANTILE_BAR, TABLE_BAR + nu * S[tail] * EXP_BAR)
    return bar


def _check_quantile(label, dev, u, tr, nu, tail_from_exp_node=False, floor=0.0):
    edge = slice(-5, None)
    assert dev[edge][0] == -NC.INF and dev[edge][1] == NC.INF and np.all(np.isnan(dev[edge][2:])), \
        f"{label}: 0 -> -inf, 1 -> +inf, out of range -> NaN"
    dev, u, tr = dev[:-5], u[:-5], tr[:-5]
    assert (u == 0.5).any() and np.all(dev[u == 0.5] == 0.0)
    _check(label, dev, tr, (_quantile_bar(nu, u, tr, tail_from_exp_node) + HALF) * np.abs(tr) + floor)


@pytest.mark.parametrize("i", range(len(NC.NUS_KAT)), ids=["nu%g" % v for v in NC.NUS_KAT])
def test_stdtrit_tab_bf(kat, i):
    """The quantile the solve kernels use for a fitted nu (tail variable from log_node / exp_node)."""
    u = NC.tppf_points()
    _same_points(kat, "tppf", u)
    nu = NC.NUS_KAT[i]
    tr = NC.truth(kat, "tppf")[i]
    if nu in NO_DIRECT_TABLES:
        # the plan builds no direct tables here and fn 16 must say so; its plans take stdtrit's refined
        # path instead (cvq_quad_kernels.h table_entry, TAB = false), fn 0: the same 7e-14.  That path is
        # Halley on g(t) = log F(t) - log p, so it cannot place t finer than g's own rounding allows:
        # log F and log p each round to half an ulp of log(1/2) and their difference is a multiple of
        # that ulp, 2 ulp(log 1/2) = 2^-52 in all, which is F / pdf times that in t -- the absolute floor
        # that matters within a few ulps of u = 1/2, where t itself is of that size
        with pytest.raises(ValueError, match="no direct t.ppf tables"):
            _special("tppf_bf", u, nu=nu)
        from scipy import stats
        floor = 2.0 ** -52 * 0.5 / stats.t.pdf(0.0, nu)
        _check_quantile(f"stdtrit (no direct tables) nu = {nu:g}", _special("tppf", u, nu=nu), u, tr, nu, floor=floor)
        return
    _check_quantile(f"stdtrit_tab_bf nu = {nu:g}", _special("tppf_bf", u, nu=nu), u, tr, nu, tail_from_exp_node=True)


def test_stdtrit_tab_int6(kat):
    u = NC.tppf_points()
    _same_points(kat, "tppf", u)
    i = NC.NUS_KAT.index(6.0)
    _check_quantile("stdtrit_tab_int<6>", _special("tppf6", u, nu=6.0), u, NC.truth(kat, "tppf")[i], 6.0)


# ------------------------------------------------------------------ the ABI's checks
def test_fn_range_and_parameters():
    from copula_var import _native as N
    x, out = np.array([1.5]), np.empty(1)
    call = lambda fn, nu: N.lib().cvq_special(0, fn, nu, N.ptr(x), 1, N.ptr(out), N.MEM_HOST)
    assert call(17, 6.0) == N.CVQ_ERR_INVALID and call(-1, 6.0) == N.CVQ_ERR_INVALID
    assert call(10, 5.0) == N.CVQ_ERR_INVALID            # root_nu<6> is nu = 6
    assert call(11, 0.5) == N.CVQ_ERR_INVALID            # pow_node: ex <= 0
    assert call(14, -0.5) == N.CVQ_ERR_INVALID           # pow_half_pos: ex >= 0
    assert call(16, -1.0) == N.CVQ_ERR_INVALID           # stdtrit_tab_bf: nu > 0
    assert max(N.SPECIAL_FN.values()) == 16 and len(set(N.SPECIAL_FN.values())) == 17
