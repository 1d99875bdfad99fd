#!/usr/bin/env python3
"""Device-mode solve (cvq_solve) and slab (cvq_slab, (-100, -3]) time of the Frank (theta = 6) and
survival-Joe (theta = 2) copulas on SORTED against the survival-Gumbel (theta = 2) and Plackett
copulas on SORTED, same library, same session, on BASELINE grids and per-date inputs (the copula
swapped): cfg 3 (2-D 512^2, 5000 dates), cfg 2 (256^2, 1000 and 125 dates), cfg 4 (3-D 128^3,
2000 dates; Plackett is 2-D).

Method of tools/bench_gumbel.py: HIP events around batches of `--reps` back-to-back calls on one
stream, `--warmup` untimed batches first, the median (and min / max) of `--batches` batches; the
copulas alternate batch by batch.  Prints one JSON line per (config, T) and, with --out, writes
them to a file.

    python tools/bench_archimedean.py --out profiles/archimedean/bench_archimedean.jsonl
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

NEW = ("frank", "joe_survival")


def copulas_for(dim: int, frank_theta: float, theta: float):
    """name -> (copula kind, packed parameters)."""
    c = {"frank": ("frank", [frank_theta]), "joe_survival": ("joe_survival", [theta]),
         "gumbel_survival": ("gumbel_survival", [theta])}
    if dim == 2:
        c["plackett"] = ("plackett", [3.0])
    return c


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="3:full,2:full,2:125,4:full",
                    help="comma list of config:T; 'full' = the config's BASELINE T")
    ap.add_argument("--theta", type=float, default=2.0, help="survival Joe's and survival Gumbel's theta")
    ap.add_argument("--frank-theta", type=float, default=6.0)
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
        T = per if tv == "full" else min(int(tv), per)
        d_a = torch.tensor(ipt[0], dtype=torch.float64, device=dev).contiguous()
        d_b = torch.tensor(ipt[1], dtype=torch.float64, device=dev).contiguous() if c.model == "msm" else None
        args = engine.solve_args(0.0)
        bounds = torch.tensor(np.column_stack((np.full(T, -100.0), np.full(T, -3.0))), device=dev)
        plans, fns, outs = {}, {}, {}
        try:
            for name, (kind, params) in copulas_for(c.dim, a.frank_theta, a.theta).items():
                p = engine.QuadraturePlan(c.model, kind, c.dim, x, step, dens, combos, c.weights, params,
                                          vol_states=uvs, device=0, strategy="sorted")
                plans[name] = p
                p.set_stream(torch.cuda.current_stream().cuda_stream)
                p.set_dates_device(T, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None)
                var = torch.empty(T, dtype=torch.float64, device=dev)
                slab = torch.empty(T, dtype=torch.float64, device=dev)
                outs[name] = (var, slab)
                fns[name, "solve"] = (lambda p=p, var=var: p.solve_device(args, var.data_ptr(), check=False))
                fns[name, "slab"] = (lambda p=p, slab=slab: N.check(
                    N.lib().cvq_slab(p._h, N.C.c_void_p(bounds.data_ptr()), N.C.c_void_p(slab.data_ptr()),
                                     N.MEM_DEVICE), "cvq_slab"))

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
            rec = {"config": cfg_no, "name": c.name, "model": c.model, "T": T, "n": c.num_points, "dim": c.dim,
                   "theta": a.theta, "frank_theta": a.frank_theta, "reps": reps, "batches": a.batches,
                   "lib_sha16": bench._lib_sha16()}
            for name, p in plans.items():
                its = p.solve_status()
                var, slab = outs[name]
                for what in ("solve", "slab"):
                    v = ts[name, what]
                    rec[f"{name}_{what}_us"] = round(1e3 * statistics.median(v), 2)
                    rec[f"{name}_{what}_us_min_max"] = [round(1e3 * min(v), 2), round(1e3 * max(v), 2)]
                rec[f"{name}_iterations"] = its
                rec[f"{name}_nan_dates"] = int(torch.isnan(var).sum().item())
                rec[f"{name}_mean_var"] = round(float(torch.nanmean(var).item()), 4)
                rec[f"{name}_mean_slab"] = float(slab.mean().item())
            for name in NEW:
                for other in ("gumbel_survival", "plackett"):
                    if other in plans:
                        for what in ("solve", "slab"):
                            rec[f"{name}_{what}_over_{other}"] = round(rec[f"{name}_{what}_us"] /
                                                                       rec[f"{other}_{what}_us"], 3)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        finally:
            for p in plans.values():
                p.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
