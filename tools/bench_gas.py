#!/usr/bin/env python3
"""Latency of the score-driven copula likelihood (cvq_gas_loglik) and of one full fit.

  * one cvq_gas_loglik call at B = 512 candidates, N = 2000 rows, Student dim 2 (nu = 6) and Frank
    dim 3, with u in device memory (the call is the row preparation, the batched recursion and a device
    synchronise, so a host clock around it is a complete time) and with u in host memory (the staging
    copy included); `--warmup` untimed calls, then `--batches` batches of `--reps` calls, the median and
    the min / max of the per-call batch means;
  * the float64 numpy restatement (tests/gas_reference.py) on the same rows on the host, wall clock;
  * launches, evaluations and wall time of one GasCopulaOptimizer.optimize() on the Student series.

One thread per candidate leaves most of the machine idle at this B (8 wavefronts on a chip that holds
thousands): the figures are latencies of a sequential recursion, not fractions of any roofline.

    python tools/bench_gas.py --out profiles/gas/bench_gas.jsonl
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "copula-msm-and-copula-garch-var_amd"), REPO, os.path.join(REPO, "tests")]

B, N_ROWS = 512, 2000


def series(dim: int, seed: int) -> np.ndarray:
    """(N_ROWS, dim) u from a one-factor Gaussian dependence whose loading swings over time."""
    from scipy import special
    rng = np.random.default_rng(seed)
    load = 0.55 + 0.3 * np.sin(2 * np.pi * np.arange(N_ROWS) / 500.0)
    common = rng.standard_normal(N_ROWS)
    z = load[:, None] * common[:, None] + np.sqrt(1 - load * load)[:, None] * rng.standard_normal((N_ROWS, dim))
    return np.ascontiguousarray(np.clip(special.ndtr(z), 2.0 ** -53, 1 - 2.0 ** -53))


def candidates(copula: str, centre: float, seed: int) -> np.ndarray:
    from copula_var.optim.copula_fit import gas_link_inverse
    rng = np.random.default_rng(seed)
    beta = rng.uniform(0.0, 0.98, B)
    alpha = rng.uniform(0.0, 0.3, B)
    return np.ascontiguousarray(np.column_stack((gas_link_inverse(copula, centre) * (1 - beta), alpha, beta)))


def timed(fn, warmup: int, batches: int, reps: int):
    for _ in range(warmup):
        fn()
    per = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        per.append((time.perf_counter() - t0) / reps * 1e3)
    return {"median_ms": statistics.median(per), "min_ms": min(per), "max_ms": max(per), "batches": batches, "reps": reps}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import gas_reference as GR
    from copula_var import _native as N
    from copula_var import engine
    from copula_var.optim.copula_fit import GasCopulaOptimizer

    N.require_gpu()
    lines = []
    for copula, dim, nu, centre in (("student", 2, 6.0, 0.45), ("frank", 3, None, 4.0)):
        u, rows = series(dim, 11 + dim), candidates(copula, centre, 5 + dim)
        du = torch.from_numpy(u).to("cuda:0")
        dout = torch.zeros(B, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        nuv = 0.0 if nu is None else nu

        def dev_call():
            N.check(N.lib().cvq_gas_loglik(0, N.COPULA_KIND[copula], 0, dim, nuv, N.ptr(rows), B, C.c_void_p(du.data_ptr()),
                                           N_ROWS, C.c_void_p(dout.data_ptr()), N.MEM_DEVICE), "cvq_gas_loglik")

        host = engine.gas_loglik(u, copula, rows, nu=nu)
        dev_call()
        assert np.array_equal(dout.cpu().numpy(), host, equal_nan=True)
        t0 = time.perf_counter()
        ref = GR.run(copula, u, rows, nu)["ll"]
        t_ref = (time.perf_counter() - t0) * 1e3
        fin = np.isfinite(ref) & np.isfinite(host)
        rec = {"what": "cvq_gas_loglik", "copula": copula, "dim": dim, "B": B, "N": N_ROWS,
               "device_mem": timed(dev_call, a.warmup, a.batches, a.reps),
               "host_mem": timed(lambda: engine.gas_loglik(u, copula, rows, nu=nu), a.warmup, a.batches, a.reps),
               "numpy_float64_ms": t_ref, "finite_rows": int(np.sum(fin)),
               "max_rel_diff_to_numpy": float(np.max(np.abs(host[fin] - ref[fin]) / np.abs(ref[fin])))}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        if copula == "student":
            dens = np.ones_like(u)
            opt = GasCopulaOptimizer(u, dens, copula, nu=nu, static_theta=centre)
            t0 = time.perf_counter()
            res = opt.optimize()
            rec = {"what": "GasCopulaOptimizer.optimize", "copula": copula, "dim": dim, "N": N_ROWS,
                   "wall_s": time.perf_counter() - t0, "launches": res["launches"], "evaluations": res["evaluations"],
                   "omega": res["omega"], "alpha": res["alpha"], "beta": res["beta"], "nll": res["nll"],
                   "static_nll": res["static_nll"]}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
