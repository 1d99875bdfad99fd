"""The Gumbel node reference (tests/gumbel_node_reference.py) and the second fixture
(tests/golden/node_kat_ext.kat), on the CPU, next to test_node_reference_cpu.py:

  * the fixture is what tests/kat/gen_node_kat_ext.py writes: every case's input digest matches
    node_cases, the chunk-edge MSM inputs and a sample of cases regenerate bit-equal;
  * the longdouble Gumbel masses agree with mpmath at 50 digits to 1e-17 relative on a sample of nodes
    that holds the narrow slab's members (measured: up to 6.7e-18);
  * the reference agrees with the float64 checker (tests/gumbel_reference.py) within 1e-13 of sum |mass|
    (measured: up to 5.9e-14; the Plackett chunk-edge rows: the oracle, 1e-10 as elsewhere);
  * one ulp of every u moves no slab by more than 1e-15 of sum |mass|, 5e-14 at the stiff parameters
    (node_cases.gumbel_stiff: measured up to 6.4e-15), and the stiff GARCH cases stay stiff under every
    sigma row set on offer;
  * the bars the GPU module applies (1e-12 + ebound; SORTED's record path + 4.05e-11) stay under 1e-11 and
    5e-11 on every case, and a float64 numpy restatement of the device formulas lies within the precise
    bar of the truth (measured: at most 0.03 of it);
  * every slab of every case keeps a member and a positive scale, the narrow slab fewer members than the
    others; every candidate weight vector keeps a member and a positive scale in every slab, and every slab
    meets each kind of event with members on some axis (test_events_and_candidates_are_populated).
"""
import importlib.util

import numpy as np
import pytest

import node_cases as NC

_spec = importlib.util.spec_from_file_location("gen_node_kat_ext", NC.EXT_GEN_PATH)
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)
GR = GEN.GR

EXT, ALL = NC.ext_cases(), NC.all_cases()
FIRST = len(ALL) - len(EXT)
GUMBEL = [i for i, c in enumerate(EXT) if c[1] in NC.GUMBEL_KINDS]
CONDITION_BAR, STIFF_CONDITION_BAR = 1e-15, 0.05 * 1e-12       # test_node_reference_cpu.py's, for the same reasons
CHECKER_BAR, ORACLE_BAR, MP_BAR = 1e-13, 1e-10, 1e-17


@pytest.fixture(scope="module")
def z():
    out = NC.load_kat()
    out.update(NC.load_ext())
    return out


# ------------------------------------------------------------------ fixture <-> generator
def test_base_fixture_is_not_shadowed():
    assert not (set(NC.load_kat()) & set(NC.load_ext()))
    import os
    assert os.path.getsize(NC.EXT_PATH) < os.path.getsize(NC.KAT_PATH)


def test_digests_match_fixture(z):
    assert ALL[FIRST:] == EXT and ALL[:FIRST] == [c + (NC.N_OF[c[2]], "") for c in NC.cases()]
    assert z["sha_case"].shape == (len(ALL),)
    for i, case in enumerate(ALL):
        assert NC.case_digest(case, z) == str(z["sha_case"][i]), NC.ext_case_id(case)
    assert len({NC.ext_case_id(c) for c in ALL}) == len(ALL)


def test_case_matrix():
    ids = {NC.ext_case_id(c) for c in EXT}
    for m in ("garch", "msm"):
        for kind in NC.GUMBEL_KINDS:
            for dim in (2, 3):
                for th in NC.GUMBEL_THETA:
                    assert (m, kind, dim, (th,), NC.N_OF[dim], "") in EXT
                assert (m, kind, dim, (4.0,), NC.N_EDGE[dim], "") in EXT
            assert m != "msm" or all(("msm", kind, dim, (4.0,), NC.N_OF[dim], "nr1") in EXT for dim in (2, 3))
        assert {"%s-plackett-2d-1.5-n70" % m, "%s-plackett-2d-1.5-n17" % m} <= ids
    assert NC.GUMBEL_THETA == (1.0, 1.0 + 2.0 ** -30, 1.5, 4.0, 16.0)
    # the chunk edges: 64-row chunks in 2-D (6 live rows in the second), 256-row chunks in 3-D (289 = 256 + 33)
    assert NC.N_EDGE[2] - 64 == 6 and NC.N_EDGE[3] ** 2 - 256 == 33


def test_not_rank1_is_not_rank1(z):
    for dim in (2, 3):
        fbs, pi = z["msm%d_fbs" % dim], z["msm%d_pi" % dim]
        q = fbs.shape[2]
        pn = NC.not_rank1(pi)
        assert np.all(np.abs(pn.sum(axis=1) - 1.0) <= 2.0 ** -52) and np.all(pn > 0.0)
        for t in range(pi.shape[0]):
            if dim == 2:
                r1 = (fbs[t, 0][:, None] * fbs[t, 1][None, :]).ravel()
            else:      # pi[L0][L1][L2] = f0[L1] f1[L2] f2[L0] (quirk Q7, cvq_sorted_kernels.h's bitwise check)
                l = np.arange(q ** 3)
                r1 = (fbs[t, 0][(l // q) % q] * fbs[t, 1][l % q]) * fbs[t, 2][l // (q * q)]
            assert np.array_equal(pi[t], r1), "the stored dates are rank 1 bit for bit (SORTED's fast path)"
            assert np.sum(pn[t] != r1) == pi.shape[1], "every entry moved: no factorisation survives"


def test_edge_msm_inputs_regenerate(z):
    shapes = GEN.edge_shapes()
    assert shapes == [(2, 17), (2, 70), (3, 17)]
    for dim, n in shapes[1:]:
        k = NC.msm_key(dim, n)
        fbs, pi, uvs = GEN.msm_inputs(dim, n)
        assert np.array_equal(fbs, z[k + "_fbs"]) and np.array_equal(pi, z[k + "_pi"]) and np.array_equal(uvs, z[k + "_uvs"])


SAMPLE_IDS = ("garch-student-2d-5.364_0.5-n24", "msm-gaussian-3d-0.9_0.9_0.85-n12", "msm-plackett-2d-50-n24",
              "garch-gumbel-2d-1.00000000093-n24", "garch-gumbel_survival-3d-16-n12", "msm-gumbel-3d-4-n12-nr1",
              "msm-gumbel_survival-2d-4-n70", "garch-gumbel-3d-4-n17", "msm-plackett-2d-1.5-n17")
SAMPLE = [i for i, c in enumerate(ALL) if NC.ext_case_id(c) in SAMPLE_IDS]


def test_sample_ids_exist():
    assert len(SAMPLE) == len(SAMPLE_IDS)


@pytest.mark.parametrize("i", SAMPLE, ids=[NC.ext_case_id(ALL[i]) for i in SAMPLE])
def test_sample_regenerates(z, i):
    case = ALL[i]
    P = GEN.build_problem(case, z)
    rows = dict(GEN.event_rows(P, case[2]))
    rows.update(GEN.port_rows(P, case[2]))
    for k, a in rows.items():
        assert np.array_equal(GEN.cast(k, a), z[k][i]), k
    if i >= FIRST:
        for k, a in GEN.slab_rows(P, case[2]).items():
            assert np.array_equal(GEN.cast("ext_" + k, a), z["ext_" + k][i - FIRST]), k
    else:           # the base cases' own truths are node_kat.kat's: the same masses
        r = P.slab_moments(NC.slabs(case[2]))
        assert np.array_equal(r["m0"], z["m0"][i])
        # candidate 0 is the plan's own weight vector: the slab itself
        assert np.array_equal(z["m0_port"][i][:, 0, :], r["m0"])


# ------------------------------------------------------------------ every extension case
@pytest.mark.parametrize("e", GUMBEL, ids=[NC.ext_case_id(EXT[e]) for e in GUMBEL])
def test_mpmath_spot_check(z, e):
    case = EXT[e]
    P = GEN.build_problem(case, z)
    sample = GEN.mp_sample(P, case[2])
    a, b = NC.NARROW
    for t, idx in sample:
        assert {tuple(i) for i in np.argwhere(P.inner_mask(a, b))} <= set(idx)
    gap = GEN.mp_gap(P, case[2], stride=1 if case[4] == NC.N_OF[case[2]] else 5)
    print(f"MEASURED {NC.ext_case_id(case)} longdouble mass against mpmath {gap:.2e} relative")
    assert gap <= MP_BAR and z["mp_gap"][e] <= MP_BAR


@pytest.mark.parametrize("e", range(len(EXT)), ids=[NC.ext_case_id(c) for c in EXT])
def test_reference_against_checker_bars_and_conditioning(z, e):
    case = EXT[e]
    model, copula, dim, params, n, variant = case
    P = GEN.build_problem(case, z)
    sl = NC.slabs(dim)
    r = P.slab_moments(sl)
    assert np.array_equal(r["m0"], z["ext_m0"][e]) and np.array_equal(r["m1"], z["ext_m1"][e])
    assert np.all(r["scale"] > 0.0) and np.all(r["count"] >= 1) and np.array_equal(r["count"], z["ext_count"][e])
    assert np.all(r["count"][:3] > r["count"][3]), "the narrow slab holds fewer nodes than the others"
    assert np.all(r["scale_below"] >= r["scale"])
    oracle = np.array([[P.slab(t, a, b) for t in range(P.T)] for a, b in sl])
    gap = float(np.max(np.abs(oracle - r["m0"]) / r["scale"]))
    cond = P.conditioning(sl)
    gumbel = copula in NC.GUMBEL_KINDS
    print(f"MEASURED {NC.ext_case_id(case)} checker gap {gap:.2e} of scale, one-ulp conditioning {cond:.2e} of scale, "
          f"narrow slab members {r['count'][3].tolist()}")
    assert gap <= (CHECKER_BAR if gumbel else ORACLE_BAR)
    assert cond <= (STIFF_CONDITION_BAR if NC.gumbel_stiff(*case[:4]) else CONDITION_BAR)
    if not gumbel:
        assert not np.any(z["ext_ebound"][e]) and not np.any(z["ext_ebound_fast"][e])
        return
    precise = NC.gumbel_bar(z["ext_ebound"][e], "precise")
    fast = NC.gumbel_bar(z["ext_ebound_fast"][e], "fast")
    worst_x = NC.gumbel_bar(max(float(z["ext_eboundx"][e].max()), float(z["ext_ebound1"][e].max())), "precise")
    dev = np.array([[float(np.sum(P.device_mass(t)[P.inner_mask(a, b)])) for t in range(P.T)] for a, b in sl])
    ratio = float(np.max(np.abs(dev - r["m0"]) / (precise * r["scale"])))
    print(f"MEASURED {NC.ext_case_id(case)} precise bar {precise.max():.2e}, fast bar {fast.max():.2e}, float64 "
          f"restatement of the device formulas {ratio:.3f} of the precise bar")
    assert np.all(z["ext_ebound"][e] > 0.0) and np.all(z["ext_ebound_fast"][e] > 0.0)
    assert precise.max() < 1e-11 and worst_x < 1e-11 and fast.max() < 5e-11
    assert ratio <= 1.0


STIFF_GARCH = [e for e, c in enumerate(EXT) if c[0] == "garch" and c[4] == NC.N_OF[c[2]] and NC.gumbel_stiff(*c[:4])]


def test_stiff_rule():
    assert len(STIFF_GARCH) == 4                                  # 3-D, theta in {4, 16}, both kinds
    assert NC.gumbel_stiff("msm", "gumbel_survival", 2, (16.0,)) and not NC.gumbel_stiff("garch", "gumbel_survival", 2, (16.0,))
    assert not NC.gumbel_stiff("msm", "gumbel", 2, (16.0,)) and not NC.gumbel_stiff("msm", "gumbel", 3, (1.5,))
    assert not any(NC.gumbel_stiff(*c[:4]) for c in ALL[:FIRST])


@pytest.mark.parametrize("e", STIFF_GARCH, ids=[NC.ext_case_id(EXT[e]) for e in STIFF_GARCH])
def test_stiff_cases_stay_stiff(z, e, monkeypatch):
    """The looser conditioning bar is not a matter of the sigma rows: under every candidate row set the
    figure stays above 1e-15 (and the rows in use are among the candidates)."""
    case = EXT[e]
    dim = case[2]
    figures = []
    for rows in NC.SIGMA_CANDIDATES[dim]:
        monkeypatch.setattr(NC, "gumbel_sigma_rows", lambda *a, rows=rows: rows)
        figures.append(GEN.build_problem(case, z).conditioning(NC.slabs(dim)))
    monkeypatch.undo()
    print(f"MEASURED {NC.ext_case_id(case)} conditioning per candidate row set", ["%.2e" % f for f in figures])
    assert any(NC.gumbel_sigma_rows(*case[1:4]) is rows for rows in NC.SIGMA_CANDIDATES[dim])
    assert min(figures) > CONDITION_BAR


# ------------------------------------------------------------------ events and candidates, all 138 cases
def test_events_and_candidates_are_populated(z):
    """What the GPU module relies on: every candidate keeps a member and a positive scale in every slab;
    every event holds mass over the box; each of the three wide slabs meets the band event of some axis and the stress event
    of some axis with members (so an error in either bound of the event's column range shows), and an
    intersection without members has a zero truth and a zero scale."""
    assert z["count_port"].shape == (len(ALL), 4, 3, NC.T)
    assert np.all(z["count_port"] >= 1) and np.all(z["scale_port"] > 0.0)
    for i, case in enumerate(ALL):
        dim = case[2]
        W = z["port_w"][i]
        assert np.array_equal(W[0, :dim], np.full(dim, 1.0 / dim)) and tuple(W[1, :dim]) == NC.PORT_UNEQUAL[dim]
        assert tuple(W[2, :dim]) in NC.PORT_SIGNED[dim] and min(W[2, 1:dim]) <= 0.0 and W[2, 0] > 0.0
        ce = z["count_event"][i][:, :dim]                         # (S, axis, event, T)
        assert np.all(z["scale_pevent"][i][:dim] > 0.0) and np.all(z["p_event"][i][:dim] > 0.0)
        for ev in (0, 1):
            # (the narrow slab's handful of members may all lie outside an event)
            assert np.all(ce[:3, :, ev, :].max(axis=1) >= 1), (NC.ext_case_id(case), ev)
        empty = z["count_event"][i] == 0
        assert np.all(z["m0_event"][i][empty] == 0.0) and np.all(z["scale_event"][i][empty] == 0.0)
        # (a populated intersection's scale can lie under float64's range -- the survival kind at theta = 16,
        # corner nodes of 1e-300 and less: the GPU module allows one smallest normal absolutely)
        assert np.all(z["scale_event"][i][~empty] >= 0.0)
        # an event's part of a slab is no more than the slab (the masses are positive)
        sc = (z["scale"][i] if i < FIRST else z["ext_scale"][i - FIRST])[:, None, None, :]
        assert np.all(z["scale_event"][i] <= sc * (1 + 1e-6))
    # the events do cut the slabs: somewhere an intersection keeps some of the slab's members, not all
    band, whole = z["count_event"][:, :, :, 1, :], z["count_port"][:, :, 0, :][:, :, None, :]
    assert np.any((band > 0) & (band < whole))
