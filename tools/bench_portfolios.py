#!/usr/bin/env python3
"""Device-mode batched-weights quantiles (cvq_portfolio_quantiles) at P = 8 candidates, L = 1 and
L = 3 levels, against the route without it: 8 back-to-back device-mode cvq_quantiles calls on 8
plans built beforehand, one per weight vector (their build time is reported separately), for
BASELINE configs at their full T and a 125-date block of cfg 2.

tools/bench_quantiles.py's method: HIP events around batches of `--reps` back-to-back sequences
on one stream, `--warmup` untimed batches first, the median of `--batches` batches with the
min-max spread; the sequences alternate batch by batch.  Prints one JSON line per (config, T)
and, with --out, writes them to a file.

    python tools/bench_portfolios.py --out profiles/portfolios/bench_portfolios.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "copula-msm-and-copula-garch-var_amd"), REPO]

LEVELS = {1: (0.05,), 3: (0.01, 0.025, 0.05)}
# P = 8 candidates (the constructor's convention, Q10): a power-of-two w0, the division path, a
# zero and a negative weight
WEIGHTS = {2: [(0.5, 0.5), (0.25, 0.75), (0.75, 0.25), (0.3, 0.7), (0.6, 0.4), (1.0, 0.0), (0.8, -0.2),
               (0.125, 0.875)],
           3: [(1 / 3, 1 / 3, 1 / 3), (0.5, 0.25, 0.25), (0.25, 0.5, 0.25), (0.2, 0.3, 0.5), (0.6, 0.4, 0.0),
               (0.7, 0.5, -0.2), (0.25, 0.25, 0.5), (0.4, 0.3, 0.3)]}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="2:full,2:125,3:full,4:full",
                    help="comma list of config:T; 'full' = the config's BASELINE T")
    ap.add_argument("--reps", type=int, default=0, help="sequences per timed batch (0: sized to ~20 ms per batch)")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from copula_var import _native as N
    from copula_var import engine, synthetic

    N.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    lines, built = [], {}
    for shape in a.shapes.split(","):
        cfg_no, tv = shape.split(":")
        cfg_no = int(cfg_no)
        if cfg_no not in built:
            cfg = synthetic.baseline_configs()[cfg_no]
            built[cfg_no] = bench.build_inputs(cfg, cfg.T, 0, 1, 0)
        c, ipt, uvs, ggp, _, per, _, _ = built[cfg_no]
        dens, x, step, combos = ggp
        W = np.array(WEIGHTS[c.dim])
        P = len(W)
        means = 0.01 * (np.arange(P) + 1.0)
        T = per if tv == "full" else min(int(tv), per)
        d_a = torch.tensor(ipt[0], dtype=torch.float64, device=dev).contiguous()
        d_b = torch.tensor(ipt[1], dtype=torch.float64, device=dev).contiguous() if c.model == "msm" else None
        stream = torch.cuda.current_stream().cuda_stream

        def make_plan(w):
            p = engine.QuadraturePlan(c.model, c.copula, c.dim, x, step, dens, combos, w, c.copula_params(),
                                      vol_states=uvs, device=0)
            p.set_stream(stream)
            p.set_dates_device(T, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None)
            return p

        plans = []
        try:
            plan = make_plan(c.weights)
            plans.append(plan)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            singles = [make_plan(w) for w in W]
            torch.cuda.synchronize()
            build_ms = 1e3 * (time.perf_counter() - t0)
            plans += singles
            args = [engine.solve_args(float(m)) for m in means]
            out_b = {L: torch.empty((3, T, P, L), dtype=torch.float64, device=dev) for L in LEVELS}
            out_s = {L: torch.empty((P, 3, T, L), dtype=torch.float64, device=dev) for L in LEVELS}

            def batched(L):
                o = out_b[L]
                return lambda: plan.portfolio_quantiles_device(args[0], W, means, LEVELS[L], o[0].data_ptr(),
                                                               o[1].data_ptr(), o[2].data_ptr())

            def eight(L):
                o = out_s[L]

                def run():
                    for p in range(P):
                        singles[p].quantiles_device(args[p], LEVELS[L], o[p, 0].data_ptr(), o[p, 1].data_ptr(),
                                                    o[p, 2].data_ptr())
                return run

            fns = {}
            for L in LEVELS:                                # the contenders alternate
                fns[f"eight{L}"] = eight(L)
                fns[f"batch{L}"] = batched(L)

            def batch(fn, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / reps          # ms per sequence

            reps = a.reps
            if reps <= 0:                                   # size the batch from one warm sequence each
                for fn in fns.values():
                    batch(fn, 1)
                one = max(batch(fn, 1) for fn in fns.values())
                reps = int(min(200, max(3, 20.0 / max(one, 1e-3))))
            for _ in range(a.warmup):
                for fn in fns.values():
                    batch(fn, reps)
            ts = {k: [] for k in fns}
            for _ in range(a.batches):
                for k, fn in fns.items():
                    ts[k].append(batch(fn, reps))
            med = {k: statistics.median(v) for k, v in ts.items()}
            rec = {"config": cfg_no, "name": c.name, "strategy": plan.strategy, "T": T, "n": c.num_points,
                   "dim": c.dim, "P": P, "reps": reps, "batches": a.batches,
                   "build_8_plans_ms": round(build_ms, 1)}
            for k in fns:
                rec[f"{k}_us"] = round(1e3 * med[k], 2)
                rec[f"{k}_us_min_max"] = [round(1e3 * min(ts[k]), 2), round(1e3 * max(ts[k]), 2)]
            for L in LEVELS:
                rec[f"batch{L}_over_eight{L}"] = round(med[f"batch{L}"] / med[f"eight{L}"], 3)
                # the two routes agree bit for bit (the contract), checked on what was just timed
                same = all(torch.equal(torch.nan_to_num(out_b[L][k][:, p, :], nan=-1.0),
                                       torch.nan_to_num(out_s[L][p, k], nan=-1.0)) for k in range(3) for p in range(P))
                rec[f"identical_L{L}"] = bool(same)
                rec[f"nan_L{L}"] = int(torch.isnan(out_b[L][0]).sum().item())
            rec["scratch_bytes_L3"] = plan.portfolio_scratch(P, 3)
            rec["lib_sha16"] = bench._lib_sha16()
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        finally:
            for p in plans:
                p.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
