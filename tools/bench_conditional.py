#!/usr/bin/env python3
"""Device-mode conditional quantiles (cvq_conditional_quantiles) at L = 1 and L = 3 levels against
the unchanged cvq_quantiles at the same L on the same plan, for BASELINE configs at their full T
and a 125-date block of cfg 2.  The event is the stress event at 0.05 (the conditioning asset at
or below the 5 % quantile of its own forecast marginal), on asset 0 (an outer axis: a row
predicate) and on the inner axis's asset (a column clamp).

tools/bench_quantiles.py's method: HIP events around batches of `--reps` back-to-back calls on
one stream, `--warmup` untimed batches first, the median of `--batches` batches with the min-max
spread; the call sequences alternate batch by batch.  Prints one JSON line per (config, T) and,
with --out, writes them to a file.

    python tools/bench_conditional.py --out profiles/conditional/bench_conditional.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "copula-msm-and-copula-garch-var_amd"), REPO]

LEVELS = {1: (0.05,), 3: (0.01, 0.025, 0.05)}
STRESS = 0.05


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="2:full,5:full,3:full,4:full,2:125",
                    help="comma list of config:T; 'full' = the config's BASELINE T")
    ap.add_argument("--reps", type=int, default=0, help="calls per timed batch (0: sized to ~20 ms per batch)")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from copula_var import _native as N
    from copula_var import engine, synthetic
    from copula_var.conditional import marginal_quantile

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
        plan = engine.QuadraturePlan(c.model, c.copula, c.dim, x, step, dens, combos, c.weights, c.copula_params(),
                                     vol_states=uvs, device=0)
        plan.set_stream(torch.cuda.current_stream().cuda_stream)
        d_a = torch.tensor(ipt[0], dtype=torch.float64, device=dev).contiguous()
        d_b = torch.tensor(ipt[1], dtype=torch.float64, device=dev).contiguous() if c.model == "msm" else None
        try:
            T = per if tv == "full" else min(int(tv), per)
            plan.set_dates_device(T, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None)
            args = engine.solve_args(0.0)
            per_date = (np.asarray(ipt[0])[:T], np.asarray(ipt[1])[:T]) if c.model == "msm" else np.asarray(ipt[0])[:T]
            axes = {"outer": 0, "inner": c.dim - 1}
            cond = {k: torch.tensor(np.column_stack((np.full(T, -np.inf),
                                                     marginal_quantile(c.model, per_date, uvs, ax, STRESS))),
                                    dtype=torch.float64, device=dev).contiguous() for k, ax in axes.items()}
            q = {L: torch.empty((3, T, L), dtype=torch.float64, device=dev) for L in LEVELS}
            co = {(k, L): torch.empty((3, T, L), dtype=torch.float64, device=dev) for k in axes for L in LEVELS}
            pe = {k: torch.empty(T, dtype=torch.float64, device=dev) for k in axes}

            def quant(L):
                o = q[L]
                return lambda: plan.quantiles_device(args, LEVELS[L], o[0].data_ptr(), o[1].data_ptr(),
                                                     o[2].data_ptr())

            def cond_call(k, L):
                o = co[k, L]
                return lambda: plan.conditional_quantiles_device(args, axes[k], cond[k].data_ptr(), LEVELS[L],
                                                                 o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                                 pe[k].data_ptr())

            fns = {}
            for L in LEVELS:                                # the contenders alternate
                fns[f"q{L}"] = quant(L)
                for k in axes:
                    fns[f"c{L}_{k}"] = cond_call(k, L)

            def batch(fn, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / reps          # ms per call

            reps = a.reps
            if reps <= 0:                                   # size the batch from one warm call each
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
                   "dim": c.dim, "reps": reps, "batches": a.batches, "stress": STRESS}
            for k in fns:
                rec[f"{k}_us"] = round(1e3 * med[k], 2)
                rec[f"{k}_us_min_max"] = [round(1e3 * min(ts[k]), 2), round(1e3 * max(ts[k]), 2)]
            for L in LEVELS:
                for k in axes:
                    rec[f"c{L}_{k}_over_q{L}"] = round(med[f"c{L}_{k}"] / med[f"q{L}"], 3)
            for k in axes:
                rec[f"p_event_{k}_min_max"] = [float(pe[k].min().item()), float(pe[k].max().item())]
                rec[f"nan_dates_L1_{k}"] = int(torch.isnan(co[k, 1][0][:, 0]).sum().item())
            rec["lib_sha16"] = bench._lib_sha16()
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        finally:
            plan.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
