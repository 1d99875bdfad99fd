#!/usr/bin/env python3
"""Device-mode exact quantiles (cvq_quantiles) at L = 1 and L = 3 levels against device-mode
cvq_solve + cvq_expected_shortfall on the same plan, for BASELINE configs at their full T and a
125-date block of cfg 2.

HIP events around batches of `--reps` back-to-back calls on one stream, `--warmup` untimed
batches first, the median of `--batches` batches; the three call sequences alternate batch by
batch.  The library's own timing kind 6 (tables, passes and updates of cvq_quantiles) is read
over one extra batch per L.  Prints one JSON line per (config, T) and, with --out, writes them
to a file.

    python tools/bench_quantiles.py --out profiles/quantiles/bench_quantiles.jsonl
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="2:full,5:full,3:full,4:full,2:125",
                    help="comma list of config:T; 'full' = the config's BASELINE T")
    ap.add_argument("--reps", type=int, default=0, help="calls per timed batch (0: sized to ~20 ms per batch)")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

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
        plan = engine.QuadraturePlan(c.model, c.copula, c.dim, x, step, dens, combos, c.weights, c.copula_params(),
                                     vol_states=uvs, device=0)
        plan.set_stream(torch.cuda.current_stream().cuda_stream)
        d_a = torch.tensor(ipt[0], dtype=torch.float64, device=dev).contiguous()
        d_b = torch.tensor(ipt[1], dtype=torch.float64, device=dev).contiguous() if c.model == "msm" else None
        try:
            T = per if tv == "full" else min(int(tv), per)
            plan.set_dates_device(T, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None)
            args = engine.solve_args(0.0)
            var, es, m0 = (torch.empty(T, dtype=torch.float64, device=dev) for _ in range(3))
            q = {L: torch.empty((3, T, L), dtype=torch.float64, device=dev) for L in LEVELS}

            def solve_es():
                plan.solve_device(args, var.data_ptr(), check=False)
                plan.expected_shortfall_device(args, var.data_ptr(), es.data_ptr(), m0.data_ptr())

            def quant(L):
                o = q[L]
                return lambda: plan.quantiles_device(args, LEVELS[L], o[0].data_ptr(), o[1].data_ptr(),
                                                     o[2].data_ptr())

            fns = {"solve_es": solve_es, "q1": quant(1), "q3": quant(3)}

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
            kind6 = {}
            for L in LEVELS:                                # the library's own events around each call
                plan.enable_timing(("quantiles",))
                batch(fns[f"q{L}"], reps)
                ms, n = plan.kernel_time("quantiles")
                kind6[L] = 1e3 * ms / max(n, 1)
                plan.enable_timing(False)
            med = {k: statistics.median(v) for k, v in ts.items()}
            v1 = q[1][0][:, 0]
            rec = {"config": cfg_no, "name": c.name, "strategy": plan.strategy, "T": T, "n": c.num_points,
                   "dim": c.dim, "reps": reps, "batches": a.batches,
                   "solve_es_us": round(1e3 * med["solve_es"], 2),
                   "solve_es_us_min_max": [round(1e3 * min(ts["solve_es"]), 2), round(1e3 * max(ts["solve_es"]), 2)],
                   "quantiles_L1_us": round(1e3 * med["q1"], 2),
                   "quantiles_L1_us_min_max": [round(1e3 * min(ts["q1"]), 2), round(1e3 * max(ts["q1"]), 2)],
                   "quantiles_L3_us": round(1e3 * med["q3"], 2),
                   "quantiles_L3_us_min_max": [round(1e3 * min(ts["q3"]), 2), round(1e3 * max(ts["q3"]), 2)],
                   "quantiles_L1_kind6_us": round(kind6[1], 2), "quantiles_L3_kind6_us": round(kind6[3], 2),
                   "L1_over_solve_es": round(med["q1"] / med["solve_es"], 3),
                   "L3_over_L1": round(med["q3"] / med["q1"], 3),
                   "nan_dates_L1": int(torch.isnan(v1).sum().item()),
                   "dates_off_calc_var_by_0.1": int((torch.abs(v1 - var) > 0.1).sum().item()),
                   "L1_equals_L3_column": bool(torch.equal(torch.nan_to_num(q[1][:, :, 0], nan=7.0),
                                                           torch.nan_to_num(q[3][:, :, 2], nan=7.0))),
                   "lib_sha16": bench._lib_sha16()}
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
