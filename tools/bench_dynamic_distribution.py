#!/usr/bin/env python3
"""Device-mode time of cvq_dynamic_distribution with real per-date paths against cvq_distribution
on the same plan and ladder (what the date records cost), on the BASELINE grids and per-date inputs
of bench.py's cfg 2 (2-D 256^2, 1000 dates) and cfg 4 (3-D 128^3, 2000 dates): a 32-bin ascending
ladder shared by every date, and the two-bin per-date ladder of a PIT.  The paths are
tools/bench_dynamic.py's: a smooth parameter path around the plan's, buy-and-hold weights drifting
with the synthetic returns.

Method of tools/bench_distribution.py: HIP events around batches of `--reps` back-to-back calls on
one stream (sized to ~50 ms), `--warmup` untimed batches first, `--batches` timed batches per side,
the sides alternating batch by batch and swapping who goes first; reported are the median and the
min / max of the batches and the ratio dynamic / static of the medians.  `own_*`: the dynamic call
with the plan's own values on every date, compared bit for bit with the static call first.

--route N: also the only route to the same numbers without this entry point, one plan per date
(create, set one date, cvq_distribution, destroy), on the first N dates, host mode and wall clock
on both sides, two rounds in alternating order (`route_*`; the plan-per-date results are compared
bit for bit with the batch's).

    python tools/bench_dynamic_distribution.py --route 64 --out profiles/dynamic_distribution/bench_dynamic_distribution.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "copula-msm-and-copula-garch-var_amd"), REPO, os.path.join(REPO, "tools")]

BINS = 32


def ladder() -> np.ndarray:
    """-100, 31 levels from -7.5 to 4.5, +inf: 32 ascending bins that tile (-100, +inf]."""
    return np.concatenate(([-100.0], np.linspace(-7.5, 4.5, BINS - 1), [np.inf]))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="2,4", help="comma list of BASELINE configs")
    ap.add_argument("--reps", type=int, default=0, help="calls per timed batch (0: sized to ~50 ms per batch)")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route", type=int, default=0, metavar="N", help="also time one plan per date on N dates")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import bench
    from bench_dynamic import param_path
    from copula_var import _native as N
    from copula_var import dynamic, engine, synthetic

    N.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    edges = ladder()
    lines = []
    for cfg_no in (int(v) for v in a.configs.split(",")):
        cfg = synthetic.baseline_configs()[cfg_no]
        c, ipt, uvs, ggp, _, T, _, block = bench.build_inputs(cfg, cfg.T, 0, 1, 0)
        dens, x, step, combos = ggp
        d_a = torch.tensor(ipt[0], dtype=torch.float64, device=dev).contiguous()
        d_b = torch.tensor(ipt[1], dtype=torch.float64, device=dev).contiguous() if c.model == "msm" else None
        base = np.atleast_1d(np.asarray(c.copula_params(), dtype=np.float64))
        w0 = np.asarray(c.weights, dtype=np.float64)
        own = (np.tile(base, (T, 1)), np.tile(w0, (T, 1)))
        path = (param_path(c.copula, base, T), dynamic.drift_weights(block[c.n_in:c.n_in + T], w0))
        # the PIT's per-date ladder: a return inside the bulk, moving from date to date
        pit = np.column_stack((np.full(T, -100.0), -1.0 + np.sin(np.arange(T) / 7.0), np.full(T, np.inf)))
        p = engine.QuadraturePlan(c.model, c.copula, c.dim, x, step, dens, combos, w0, base, vol_states=uvs, device=0)
        try:
            p.set_stream(torch.cuda.current_stream().cuda_stream)
            p.set_dates_device(T, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None)
            d_pit = torch.tensor(pit, dtype=torch.float64, device=dev)
            out = {k: torch.zeros((2, T, BINS), dtype=torch.float64, device=dev)
                   for k in ("static32", "own32", "path32", "static_pit", "path_pit")}

            def static(key, e, nb):
                o = out[key]
                return lambda: p.distribution_device(e, nb, o[0].data_ptr(), o[1].data_ptr())

            def dyn(key, e, nb, rec):
                o = out[key]
                return lambda: p.dynamic_distribution_device(e, nb, o[0].data_ptr(), o[1].data_ptr(),
                                                             copula_params=rec[0], weights=rec[1])

            groups = {"32": {"static32": static("static32", edges, BINS), "own32": dyn("own32", edges, BINS, own),
                             "path32": dyn("path32", edges, BINS, path)},
                      "pit": {"static_pit": static("static_pit", d_pit.data_ptr(), 2),
                              "path_pit": dyn("path_pit", d_pit.data_ptr(), 2, path)}}

            def batch(fn, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / reps          # ms per call

            rec = {"config": cfg_no, "name": c.name, "model": c.model, "copula": c.copula, "T": T,
                   "n": c.num_points, "dim": c.dim, "strategy": p.strategy, "bins": BINS, "batches": a.batches,
                   "lib_sha16": bench._lib_sha16()}
            for gname, fns in groups.items():
                reps = a.reps
                if reps <= 0:                               # size the batch from one warm call each
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
                rec[f"reps_{gname}"] = reps
                for k, v in ts.items():
                    rec[f"{k}_ms"] = round(statistics.median(v), 4)
                    rec[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
                    rec[f"{k}_ms_batches"] = [round(t, 4) for t in v]
            rec["path32_over_static32"] = round(rec["path32_ms"] / rec["static32_ms"], 3)
            rec["own32_over_static32"] = round(rec["own32_ms"] / rec["static32_ms"], 3)
            rec["path_pit_over_static_pit"] = round(rec["path_pit_ms"] / rec["static_pit_ms"], 3)
            torch.cuda.synchronize()
            rec["own32_equals_static32"] = bool(torch.equal(out["own32"], out["static32"]))
            m = out["path32"][0].cpu().numpy()
            rec["path_total_mass_mean"] = float(m.sum(axis=1).mean())
            rec["path_differs_from_static"] = bool(not torch.equal(out["path32"], out["static32"]))

            if a.route > 0:
                Tn = min(a.route, T)
                ha = np.ascontiguousarray(ipt[0][:Tn])
                hb = np.ascontiguousarray(ipt[1][:Tn]) if c.model == "msm" else None
                p.set_dates((ha, hb) if c.model == "msm" else [ha])
                cpn, wn = path[0][:Tn], path[1][:Tn]

                def one_call():
                    return p.dynamic_distribution(edges, cpn, wn)

                def plan_per_date():
                    rows = []
                    for t in range(Tn):
                        q = engine.QuadraturePlan(c.model, c.copula, c.dim, x, step, dens, combos, wn[t], cpn[t],
                                                  vol_states=uvs, device=0)
                        try:
                            q.set_dates((ha[t:t + 1], hb[t:t + 1]) if c.model == "msm" else [ha[t:t + 1]])
                            rows.append(q.distribution(edges))
                        finally:
                            q.close()
                    return [np.concatenate([r[k] for r in rows], axis=0) for k in range(2)]

                def wall(fn):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = fn()
                    return (time.perf_counter() - t0) * 1e3, r

                wall(one_call)                              # warm (the library and the plan's scratch)
                tr = {"route_one_call": [], "route_plan_per_date": []}
                sides = [("route_one_call", one_call), ("route_plan_per_date", plan_per_date)]
                for i in range(2):
                    for k, fn in (sides if i % 2 == 0 else sides[::-1]):
                        ms, res = wall(fn)
                        tr[k].append(ms)
                        if k == "route_one_call":
                            got = res
                        else:
                            want = res
                rec["route_dates"] = Tn
                for k, v in tr.items():
                    rec[f"{k}_ms"] = round(statistics.median(v), 3)
                    rec[f"{k}_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
                rec["route_plan_per_date_over_one_call"] = round(rec["route_plan_per_date_ms"] / rec["route_one_call_ms"], 1)
                rec["route_bit_identical"] = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
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
