"""Pins tests/forecast_reference.py (the longdouble yardstick of test_forecast_kernels_gpu.py)
without a GPU:

* against the reference-run goldens (filtered_probs, forecasts_by_states, forecasts of cfg2_n64 and
  cfg4_k6_n16; sigma_forecasts of the UKF and GARCH goldens), rounded to double;
* against the float64 oracle (oracle/forecast.py) on exactly the inputs the GPU module uses, under
  the tiered rule of forecast_reference.check_tiers with the oracle held 10x / 100x tighter than
  the device bars (1e-13 top tier, 1e-12 middle tier): the bars are ones a float64 filter can
  meet.  Measured on the CPU this suite was written on (max over every shared input):
      filtered probabilities, k = 1 .. 7, every shape   top 4.6e-14   middle 1.6e-13   bottom <= 1.1e-202
      fbs / pi of 2 and 3 assets                        top 3.1e-14   middle 1.2e-13
  and every tier is populated on the spiky series at every k >= 3 (asserted);
* scan_middle_class visits every class a window longer than two blocks can fall in over the GPU
  module's scan shapes.  ("none" needs t % 16 + n_in <= 32, so n_in <= 32: the scan filter never
  sees it, cvq_msm_tables runs such windows step by step.  It is pinned on those shapes instead.)
"""
import numpy as np
import pytest

import forecast_reference as F
import insample_reference as R
from conftest import load_golden

ORACLE_TOP, ORACLE_MID = 1e-13, 1e-12


def _oracle_check(name, got, ref):
    m = F.tier_errors(got, ref)
    print(f"MEASURED oracle {name}: top {m['top']:.2e} ({m['n'][0]}), middle {m['mid']:.2e} ({m['n'][1]}), "
          f"bottom max {m['bottom']:.2e} ({m['n'][2]})")
    assert m["top"] <= ORACLE_TOP and m["mid"] <= ORACLE_MID and m["bottom"] <= F.BOTTOM_CAP, (name, m)
    return m


def _windows(x, n_in):
    T = x.shape[0] - n_in + 1
    return x[np.arange(T)[:, None] + np.arange(n_in)[None, :]]


# ------------------------------------------------------------------- reference-run goldens
@pytest.mark.parametrize("case", ["cfg2_n64", "cfg4_k6_n16"])
def test_reference_tables_match_golden(case):
    from copula_var import tables
    from oracle import forecast as O
    z = load_golden(case)
    n_in, k, dim = int(z["n_in"]), int(z["k"]), int(z["dim"])
    mean, _, _ = O.insample_split(z["returns"], n_in, z["weights"])
    rc = (z["returns"] - mean)[:-1]
    names = [str(n) for n in z["model_param_names"]]
    rows = [tuple(float(row[names.index(n)]) for n in ("m_0", "sig", "b", "gamma")) for row in z["model_params"]]
    vsa = np.array([tables.msm_vol_states(k, row[0], row[1]) for row in rows])
    smap, uvs = tables.unique_vol_map(vsa)
    probs = [F.msm_window_probs(rc[:, d], n_in, k, *rows[d]) for d in range(dim)]
    for d in range(dim):
        F.check_tiers(f"{case} filtered_probs[{d}]", z["filtered_probs"][d], probs[d])
    fbs = np.stack([F.collapse(probs[d], smap[d], uvs.shape[1]) for d in range(dim)], axis=1)
    F.check_tiers(f"{case} forecasts_by_states", z["forecasts_by_states"], fbs)
    F.check_tiers(f"{case} forecasts", z["forecasts"], F.combinations(fbs))


def test_combinations_keep_the_q7_order():
    """3 assets: pi[l] = f0[L1] f1[L2] f2[L0], l = (L0 q + L1) q + L2 -- on distinct primes, so a
    swapped axis changes the value."""
    fbs = np.array([[[2.0, 3.0], [5.0, 7.0], [11.0, 13.0]]])
    pi = F.combinations(fbs)[0]
    want = [fbs[0, 0, (l // 2) % 2] * fbs[0, 1, l % 2] * fbs[0, 2, l // 4] for l in range(8)]
    assert [float(v) for v in pi] == want
    pi2 = F.combinations(fbs[:, :2])[0]
    assert [float(v) for v in pi2] == [10.0, 14.0, 15.0, 21.0]


def test_popcount_map_is_the_production_map():
    from copula_var import tables
    for k in range(1, 8):
        for row in F.asset_rows(k, 3):
            smap, uvs = tables.unique_vol_map(tables.msm_vol_states(k, row[0], row[1])[None, :])
            assert uvs.shape[1] == k + 1
            np.testing.assert_array_equal(smap[0], F.popcount_map(k))


@pytest.mark.parametrize("case,windows", [("ukf_plackett_n64", (0, 9)), ("cfg5_n64", (15,))])
def test_reference_ukf_forecast_matches_golden(case, windows):
    from oracle import forecast as O
    z = load_golden(case)
    n_in = int(z["n_in"])
    mean, _, _ = O.insample_split(z["returns"], n_in, z["weights"])
    rc = z["returns"] - mean
    names = [str(n) for n in z["model_param_names"]]
    for d, row in enumerate(z["model_params"]):
        a, l, q = (float(row[names.index(n)]) for n in ("a", "l", "q"))
        for t in windows:
            got = F.ukf_forecast(rc[t:t + n_in, d], a, l, q)
            np.testing.assert_allclose(np.float64(got), z["sigma_forecasts"][t, d], rtol=1e-12, err_msg=f"{d} {t}")


@pytest.mark.parametrize("case", ["cfg1_kwargs", "garch3d_student_n16"])
def test_reference_garch_forecast_matches_sigma_golden(case):
    from oracle import forecast as O
    z = load_golden(case)
    n_in = int(z["n_in"])
    mean, _, _ = O.insample_split(z["returns"], n_in, z["weights"])
    rc = z["returns"] - mean
    names = [str(n) for n in z["model_param_names"]]
    for d, row in enumerate(z["model_params"]):
        omega, alpha, beta = (float(row[names.index(n)]) for n in ("omega", "alpha", "beta"))
        got = [F.garch_forecast_pq(rc[t:t + n_in, d], omega, alpha, beta)[0] for t in range(z["sigma_forecasts"].shape[0])]
        np.testing.assert_allclose(np.asarray(got, dtype=np.float64), z["sigma_forecasts"][:, d], rtol=1e-12)


def test_reference_ukf_forecast_is_the_oracle_on_the_shared_rows():
    """... and fails where the oracle fails: an exact 0.0 return anywhere in the window, the last
    step included."""
    from oracle import forecast as O
    for d, (a, l, q) in enumerate(R.UKF_ROWS[:3]):
        w = R.ukf_returns(64, seed=6600 + d)
        f, _, _, failed = O.ukf_run(w, a, l, q)
        assert not failed.any()
        np.testing.assert_allclose(np.float64(F.ukf_forecast(w, a, l, q)), f[0], rtol=1e-13)
        for at in (0, 20, 63):
            bad = w.copy()
            bad[at] = 0.0
            assert O.ukf_run(bad, a, l, q)[3].all() and F.ukf_forecast(bad, a, l, q) is None
    one = R.ukf_returns(1)
    np.testing.assert_allclose(np.float64(F.ukf_forecast(one, *R.UKF_ROWS[0])), O.ukf_run(one, *R.UKF_ROWS[0])[0][0],
                               rtol=1e-14)


# ---------------------------------------------- the float64 oracle on every shared GPU input
def _filter_cases():
    for k in range(1, 8):
        for kind in F.SERIES_KINDS:
            yield k, kind


@pytest.mark.parametrize("k,kind", list(_filter_cases()))
def test_oracle_filter_inside_the_rule(k, kind):
    """cvq_msm_filter's inputs (FILTER_SHAPES) and cvq_msm_tables' (step-by-step and scan shapes),
    asset by asset: the float64 filter of oracle/forecast.py against the longdouble one."""
    from oracle import forecast as O
    row = F.base_row(k)
    pop = np.zeros(3, dtype=int)
    for n_in, T in F.FILTER_SHAPES:
        N = n_in + T - 1
        x = F.series(kind, N, 3000 + N, row[1])
        ref = F.msm_window_probs(x, n_in, k, *row)
        assert ref.shape == (T, 1 << k)
        np.testing.assert_allclose(np.asarray(ref.sum(axis=1), dtype=np.float64), 1.0, rtol=1e-15)
        m = _oracle_check(f"filter k={k} {kind} ({n_in},{T})", O.msm_filtered_probs(_windows(x, n_in), k, *row), ref)
        pop += m["n"]
    shapes = F.step_shapes(k) + (F.SCAN_SHAPES if 2 <= k <= 6 else ())
    for n_in, T in shapes:
        rc, rows = F.asset_series(kind, n_in, T, k, 3)
        for d in range(3):
            ref = F.asset_window_probs(kind, n_in, T, k, d, rows[d])
            m = _oracle_check(f"tables k={k} {kind} ({n_in},{T}) asset {d}",
                              O.msm_filtered_probs(_windows(rc[:, d], n_in), k, *rows[d]), ref)
            pop += m["n"]
    if kind == "spiky" and k >= 3:                             # k = 1, 2: 2 / 4 states never fall below 1e-200
        assert np.all(pop > 0), f"a tier is empty on the spiky series: {pop}"


@pytest.mark.parametrize("k,n_in,T", [(1, 5, 19), (3, 32, 33), (4, 49, 130), (6, 33, 17), (7, 33, 17)])
def test_oracle_fbs_and_pi_inside_the_rule(k, n_in, T):
    from oracle import forecast as O
    for kind in F.SERIES_KINDS:
        for dim in (2, 3):
            rc, rows = F.asset_series(kind, n_in, T, k, dim)
            fbs, pi = F.tables_reference(kind, n_in, T, k, dim)
            filt = np.array([O.msm_filtered_probs(_windows(rc[:, d], n_in), k, *rows[d]) for d in range(dim)])
            vsa = np.array([O.msm_vol_states(k, rows[d][0], rows[d][1]) for d in range(dim)])
            ofbs, _ = O.sum_forecast_by_state(vsa, filt)
            _oracle_check(f"fbs k={k} {kind} dim={dim}", ofbs, fbs)
            _oracle_check(f"pi k={k} {kind} dim={dim}", O.forecast_combinations(ofbs), pi)


def test_reference_raises_where_the_oracle_does():
    from oracle import forecast as O
    x = F.plain_series(40, 1)
    x[17] = 1e4 * 1.2
    with pytest.raises(FloatingPointError):
        F.msm_window_probs(x, 8, 3, *F.BASE_ROW)
    with pytest.raises(FloatingPointError):
        O.msm_filtered_probs(_windows(x, 8), 3, *F.BASE_ROW)
    F.msm_window_probs(x[18:], 8, 3, *F.BASE_ROW)              # the windows that miss it pass


# ------------------------------------------------------------------ the scan geometry
def test_scan_shapes_visit_every_class():
    seen = set()
    for n_in, T in F.SCAN_SHAPES:
        assert n_in > 2 * F.SCAN_B and T % 16 != 0
        seen |= F.scan_classes(n_in, T)
    kinds = {c for c, _ in seen}
    assert kinds == {"prefix", "suffix", "loose", "several"}, kinds
    assert {n for c, n in seen if c == "several"} >= {2, 3}      # with and without a whole superblock inside
    assert {n for c, n in seen if c == "loose"} >= {1, 2}
    # the wide scan classifies a group of 16 windows by its first one
    wide = {F.scan_middle_class(t, n_in, n_in + T - 1)[0] for n_in, T in F.SCAN_SHAPES for t in range(0, T, 16)}
    assert wide == {"prefix", "suffix", "loose", "several"}, wide
    assert sum((n_in + T - 1) % 16 != 0 for n_in, T in F.SCAN_SHAPES) >= 2
    # "none" only below the scan's threshold: those windows run step by step
    assert all(F.scan_middle_class(t, n_in, n_in + 200)[0] != "none" for n_in in range(33, 120) for t in range(64))
    assert F.scan_middle_class(0, 32, 64) == ("none", 0) and F.scan_middle_class(5, 20, 64) == ("none", 0)
    assert F.scan_middle_class(15, 33, 64) == ("loose", 1)
    assert F.scan_middle_class(112, 49, 400) == ("prefix", 1)               # blocks 8 .. 9 start superblock 1
    assert F.scan_middle_class(80, 49, 400) == ("suffix", 1)                # blocks 6 .. 7 end superblock 0
    assert F.scan_middle_class(16, 33, 49) == ("suffix", 1)                 # block 2 ends the series' partial one
    assert F.scan_middle_class(0, 160, 400) == ("several", 2)               # blocks 1 .. 8
