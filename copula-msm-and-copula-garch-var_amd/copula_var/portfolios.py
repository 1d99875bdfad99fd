"""Candidate weight vectors for QuadraturePlan.portfolio_quantiles and the pick among their
results (no reference counterpart; pure numpy, no device)."""
from __future__ import annotations

from itertools import product
from typing import Tuple

import numpy as np


def weight_lattice(dim: int, steps: int) -> np.ndarray:
    """(P, dim): every vector k / steps with non-negative integers k summing to `steps` and
    k[0] >= 1 (the engine divides by weights[0], quirk Q10), in lexicographic order of k."""
    dim, steps = int(dim), int(steps)
    if dim < 2 or steps < 1:
        raise ValueError("weight_lattice needs dim >= 2 and steps >= 1")
    rows = [k + (steps - sum(k),) for k in product(range(steps + 1), repeat=dim - 1)
            if k[0] >= 1 and sum(k) <= steps]
    return np.asarray(rows, dtype=np.float64) / steps


def min_es(es) -> Tuple[np.ndarray, np.ndarray]:
    """(index (T, L) int, value (T, L)) of the candidate with the smallest expected loss per date
    and level: es (T, P, L) holds returns, so that is the largest ES.  The first such candidate
    in batch order wins; a NaN candidate never does; where every candidate is NaN the index is
    -1 and the value NaN."""
    e = np.asarray(es, dtype=np.float64)
    if e.ndim != 3:
        raise ValueError("es must have shape (T, P, L)")
    nan = np.isnan(e)
    idx = np.argmax(np.where(nan, -np.inf, e), axis=1)            # argmax: the first maximum
    lost = np.take_along_axis(nan, idx[:, None, :], axis=1)[:, 0, :]     # only -inf candidates beside the NaNs
    idx = np.where(lost, np.argmax(~nan, axis=1), idx)
    val = np.take_along_axis(e, idx[:, None, :], axis=1)[:, 0, :]
    none = nan.all(axis=1)
    return np.where(none, -1, idx), np.where(none, np.nan, val)
