#!/usr/bin/env python3
"""Device-mode tail moments (cvq_slab_moments) against device-mode cvq_slab on the same plan
and bounds (lower, first_guess] = (-100, -3], for BASELINE configs at their full T and at
T = 1 and T = 125.  cvq_slab is the plan's existing slab path and evaluates the same nodes.

HIP events around batches of `--reps` back-to-back calls on one stream, `--warmup` untimed
batches first, the median of `--batches` batches; the two entry points alternate batch by
batch.  Prints one JSON line per (config, T) and, with --out, writes them to a file.

    python tools/bench_moments.py --configs 2,3,4,5 --out profiles/moments/bench_moments.jsonl
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "copula-msm-and-copula-garch-var_amd"), REPO]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="2,3,4,5")
    ap.add_argument("--dates", default="1,125,full", help="comma list of T; 'full' = the config's BASELINE T")
    ap.add_argument("--reps", type=int, default=0, help="calls per timed batch (0: sized to ~20 ms per batch)")
    ap.add_argument("--batches", type=int, default=9)
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
    lines = []
    for cfg_no in (int(v) for v in a.configs.split(",")):
        cfg = synthetic.baseline_configs()[cfg_no]
        c, ipt, uvs, ggp, _, per, _, _ = bench.build_inputs(cfg, cfg.T, 0, 1, 0)
        dens, x, step, combos = ggp
        plan = engine.QuadraturePlan(c.model, c.copula, c.dim, x, step, dens, combos, c.weights, c.copula_params(),
                                     vol_states=uvs, device=0)
        plan.set_stream(torch.cuda.current_stream().cuda_stream)
        d_a = torch.tensor(ipt[0], dtype=torch.float64, device=dev).contiguous()
        d_b = torch.tensor(ipt[1], dtype=torch.float64, device=dev).contiguous() if c.model == "msm" else None
        try:
            for tv in a.dates.split(","):
                T = per if tv == "full" else min(int(tv), per)
                plan.set_dates_device(T, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None)
                bounds = torch.tensor(np.tile((-100.0, -3.0), (T, 1)), dtype=torch.float64, device=dev)
                out, m0, m1 = (torch.empty(T, dtype=torch.float64, device=dev) for _ in range(3))
                h = plan._h

                def slab():
                    N.check(N.lib().cvq_slab(h, C.c_void_p(bounds.data_ptr()), C.c_void_p(out.data_ptr()),
                                             N.MEM_DEVICE), "cvq_slab")

                def moments():
                    plan.tail_moments_device(bounds.data_ptr(), m0.data_ptr(), m1.data_ptr())

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
                    batch(slab, 1), batch(moments, 1)
                    one = max(batch(slab, 1), batch(moments, 1))
                    reps = int(min(200, max(3, 20.0 / max(one, 1e-3))))
                for _ in range(a.warmup):
                    batch(slab, reps), batch(moments, reps)
                ts, tm = [], []
                for _ in range(a.batches):
                    ts.append(batch(slab, reps))
                    tm.append(batch(moments, reps))
                # a date with no mass below the bound has out == m0 == 0: compared absolutely
                rel = float(torch.max(torch.abs(m0 - out) / torch.clamp(torch.abs(out), min=1e-300)).item())
                rec = {"config": cfg_no, "name": c.name, "strategy": plan.strategy, "T": T, "n": c.num_points,
                       "dim": c.dim, "reps": reps, "batches": a.batches,
                       "slab_us": round(1e3 * statistics.median(ts), 2),
                       "slab_us_min_max": [round(1e3 * min(ts), 2), round(1e3 * max(ts), 2)],
                       "moments_us": round(1e3 * statistics.median(tm), 2),
                       "moments_us_min_max": [round(1e3 * min(tm), 2), round(1e3 * max(tm), 2)],
                       "ratio": round(statistics.median(tm) / statistics.median(ts), 3),
                       "m0_vs_slab_max_rel": rel, "lib_sha16": bench._lib_sha16()}
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
