"""Inputs of the score-driven copula tests (tests/golden/gas_copula.kat; tests/kat/gen_gas_kat.py
writes the truths).  No mpmath here.

A case is (copula, dim, nu): one seeded series of N_MAX rows u in (0, 1)^dim and a few candidate
rows (omega, alpha, beta).  The lengths N in NS are prefixes of the same series, so one truth path
serves all three.  Rows EDGE_LO / EDGE_HI of every series sit within 1e-9 of 0 and of 1.
"""
import hashlib
import os

import numpy as np

import gas_reference as GR

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_PATH = os.path.join(HERE, "golden", "gas_copula.kat")

NS = (1, 2, 48)
N_MAX = 48
EDGE_LO, EDGE_HI = 5, 17
STUDENT_NUS = (6.0, 5.364)
LL_BAR, PATH_BAR = 1e-12, 1e-12           # the device's bars (the issue's)
CPU_BAR = 1e-13                           # the float64 restatement's, on both measures

KIND_DIMS = [("gaussian", 2), ("student", 2), ("plackett", 2)] + \
    [(k, d) for k in ("gumbel", "gumbel_survival", "frank", "joe", "joe_survival") for d in (2, 3)]

# a central parameter per family: the candidates' unconditional level f_bar = link^-1(CENTRE)
CENTRE = {"gaussian": 0.45, "student": 0.45, "plackett": 1.4, "gumbel": 1.8, "frank": 4.0, "joe": 1.9}


def cases():
    out = []
    for kind, dim in KIND_DIMS:
        for nu in (STUDENT_NUS if kind == "student" else (None,)):
            out.append((kind, dim, nu))
    return out


def case_id(case):
    kind, dim, nu = case
    return f"{kind}{dim}" + ("" if nu is None else f"_nu{nu:g}")


def series(case):
    """(N_MAX, dim) seeded u: a one-factor Gaussian dependence (loading 0.7) pushed through Phi, then
    the two edge rows.  Every value is strictly inside (0, 1)."""
    from scipy import special
    kind, dim, nu = case
    seed = 7919 + 31 * cases().index(case)
    rng = np.random.default_rng(seed)
    common = rng.standard_normal(N_MAX)
    z = 0.7 * common[:, None] + np.sqrt(1 - 0.49) * rng.standard_normal((N_MAX, dim))
    u = special.ndtr(z)
    u[EDGE_LO] = np.array([7e-10, 3e-10, 9e-10])[:dim]
    u[EDGE_HI] = 1.0 - np.array([5e-10, 2e-10, 8e-10])[:dim]
    assert np.all((u > 0) & (u < 1))
    return np.ascontiguousarray(u)


# The recursion feeds a row's rounding back through alpha s_t.  Plackett's density (the reference's Q11 formula)
# has poles on u + v = 1 + 1 / (theta - 1) once theta > 2, so its scores are large near them: its alphas are
# softened until the float64 restatement holds CPU_BAR (tests/test_gas_cpu.py asserts it for every case).
ALPHA_SCALE = {"plackett": 0.25}


def param_rows(case):
    """(R, 3) candidates (omega, alpha, beta): alpha = 0; beta = 0.97; a lively mid-persistence row; a row
    whose f_0 = 60 sits above the clamp and whose every update is cut back to +40.  (No row sits at -40:
    there the Archimedean kinds are within 1e-16 of independence, log c is a difference of O(1) terms that
    is itself ~1e-4, and no float64 evaluation holds 1e-13 of sum |l_t|.)"""
    fbar = GR.link_inverse(case[0], CENTRE[GR.FAMILY[case[0]]])
    k = ALPHA_SCALE.get(GR.FAMILY[case[0]], 1.0)
    return np.array([
        [fbar * (1 - 0.9), 0.0, 0.9],
        [fbar * (1 - 0.97), 0.03 * k, 0.97],
        [fbar * (1 - 0.5), 0.08 * k, 0.5],
        [30.0, 0.02, 0.5],
    ])


ROW_NAMES = ("alpha0", "beta097", "mid", "clamp_hi")


def case_digest(u, rows):
    return hashlib.sha256(np.ascontiguousarray(u).tobytes() + np.ascontiguousarray(rows).tobytes()).hexdigest()


def load_kat():
    return dict(np.load(KAT_PATH, allow_pickle=False))


def key(case, name):
    return f"{case_id(case)}_{name}"


def truth(kat, case, n):
    """(theta (R, n + 1), logc (R, n), ll (R,), scale (R,)) of the length-n prefix, longdouble."""
    th = kat[key(case, "theta")].astype(GR.LD)[:, :n + 1]
    lc = kat[key(case, "logc")].astype(GR.LD)[:, :n]
    i = NS.index(n)
    return th, lc, kat[key(case, "ll")].astype(GR.LD)[:, i], kat[key(case, "scale")].astype(GR.LD)[:, i]
