#!/usr/bin/env python3
"""Device-mode time of one cvq_distribution call with a 32-bin ascending ladder over (-100, +inf]
against a loop of 32 cvq_slab_moments calls over the same disjoint bins, same session, on the
BASELINE grids and per-date inputs of bench.py's cfg 2 (2-D 256^2, 1000 dates) and cfg 4
(3-D 128^3, 2000 dates).

Method of tools/bench_archimedean.py: HIP events around batches of `--reps` back-to-back
repetitions on one stream, `--warmup` untimed batches first, `--batches` timed batches per side,
the two sides alternating batch by batch (the side that goes first alternates too); reported are
the median and the min / max of the batches, the ratio loop / sweep of the medians, and whether the
sweep's slowest batch beats the loop's fastest (`sweep_max_below_loop_min`).  The two sides'
results are compared at the slab bar first (`max_rel_mass`, `max_rel_m1`).  `kind5_*`: the
same two sides by the plan's own kind-5 (tail moments) events, one synchronised call at a time.

--only loop / --only sweep time one side alone (the loop side runs on any build that has
cvq_slab_moments, e.g. the parent commit's), for alternating two builds from a shell.

    python tools/bench_distribution.py --out profiles/distribution/bench_distribution.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "copula-msm-and-copula-garch-var_amd"), REPO]

BINS = 32


def ladder() -> np.ndarray:
    """-100, 31 levels from -7.5 to 4.5, +inf: 32 ascending bins that tile (-100, +inf]."""
    return np.concatenate(([-100.0], np.linspace(-7.5, 4.5, BINS - 1), [np.inf]))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="2:full,4:full", help="comma list of config:T; 'full' = the config's BASELINE T")
    ap.add_argument("--only", default="both", choices=["both", "sweep", "loop"])
    ap.add_argument("--reps", type=int, default=0, help="repetitions per timed batch (0: sized to ~50 ms per batch)")
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
    edges = ladder()
    lines = []
    for shape in a.shapes.split(","):
        cfg_no, tv = shape.split(":")
        cfg = synthetic.baseline_configs()[int(cfg_no)]
        c, ipt, uvs, ggp, _, per, _, _ = bench.build_inputs(cfg, cfg.T, 0, 1, 0)
        dens, x, step, combos = ggp
        T = per if tv == "full" else min(int(tv), per)
        d_a = torch.tensor(ipt[0], dtype=torch.float64, device=dev).contiguous()
        d_b = torch.tensor(ipt[1], dtype=torch.float64, device=dev).contiguous() if c.model == "msm" else None
        p = engine.QuadraturePlan(c.model, c.copula, c.dim, x, step, dens, combos, c.weights, c.copula_params(),
                                  vol_states=uvs, device=0)
        try:
            p.set_stream(torch.cuda.current_stream().cuda_stream)
            p.set_dates_device(T, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None)
            mass = torch.zeros((T, BINS), dtype=torch.float64, device=dev)
            m1 = torch.zeros((T, BINS), dtype=torch.float64, device=dev)
            l0 = torch.zeros((BINS, T), dtype=torch.float64, device=dev)
            l1 = torch.zeros((BINS, T), dtype=torch.float64, device=dev)
            bounds = [torch.tensor(np.tile(edges[b:b + 2], (T, 1)), dtype=torch.float64, device=dev)
                      for b in range(BINS)]

            def sweep():
                p.distribution_device(edges, BINS, mass.data_ptr(), m1.data_ptr())

            def loop():
                for b in range(BINS):
                    p.tail_moments_device(bounds[b].data_ptr(), l0[b].data_ptr(), l1[b].data_ptr())

            fns = {k: f for k, f in (("sweep", sweep), ("loop", loop)) if a.only in ("both", k)}

            def batch(fn, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / reps          # ms per repetition

            reps = a.reps
            if reps <= 0:                                   # size the batch from one warm repetition each
                for fn in fns.values():
                    batch(fn, 1)
                one = max(batch(fn, 1) for fn in fns.values())
                reps = int(min(200, max(3, 50.0 / max(one, 1e-3))))
            for _ in range(a.warmup):
                for fn in fns.values():
                    batch(fn, reps)
            ts = {k: [] for k in fns}
            for i in range(a.batches):
                order = list(fns) if i % 2 == 0 else list(fns)[::-1]
                for k in order:
                    ts[k].append(batch(fns[k], reps))
            rec = {"config": int(cfg_no), "name": c.name, "model": c.model, "copula": c.copula, "T": T,
                   "n": c.num_points, "dim": c.dim, "strategy": p.strategy, "bins": BINS, "reps": reps,
                   "batches": a.batches, "lib_sha16": bench._lib_sha16()}
            for k, v in ts.items():
                rec[f"{k}_ms"] = round(statistics.median(v), 4)
                rec[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
                rec[f"{k}_ms_batches"] = [round(t, 4) for t in v]
            if a.only == "both":
                rec["loop_over_sweep"] = round(rec["loop_ms"] / rec["sweep_ms"], 2)
                rec["loop_min_over_sweep_max"] = round(min(ts["loop"]) / max(ts["sweep"]), 2)
                rec["sweep_max_below_loop_min"] = bool(max(ts["sweep"]) < min(ts["loop"]))
                m, w = mass.cpu().numpy(), m1.cpu().numpy()
                r0, r1 = l0.cpu().numpy().T, l1.cpu().numpy().T
                rec["max_rel_mass"] = float(np.max(np.abs(m - r0) / np.maximum(np.abs(r0), 1e-300)))
                rec["max_rel_m1"] = float(np.max(np.abs(w - r1) / np.maximum(np.abs(r1), 1e-300)))
                rec["total_mass_mean"] = float(m.sum(axis=1).mean())
                rec["empty_bins"] = int(np.sum(np.all(m == 0.0, axis=0)))
                torch.cuda.synchronize()
                for k, fn in fns.items():                   # the plan's own kind-5 events, one call at a time
                    vals = []
                    for _ in range(5):
                        p.enable_timing(("moments",))
                        fn()
                        torch.cuda.synchronize()
                        vals.append(p.kernel_time("moments"))
                    p.enable_timing(False)
                    rec[f"kind5_{k}_ms"] = round(statistics.median(v[0] for v in vals), 4)
                    rec[f"kind5_{k}_launches"] = vals[0][1]
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        finally:
            p.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
