#!/usr/bin/env python3
"""Device-mode per-date-record quantiles (cvq_dynamic_quantiles) against device-mode cvq_quantiles
of the same library on the same plan and batch, at L = 1 and L = 3 levels, for BASELINE configs at
their full T.

Two dynamic contenders per level count: `own`, every date's record the plan's own parameters and
weights (the same work as cvq_quantiles: the outputs are compared bit for bit after timing), and
`path`, a smooth parameter path around the plan's with buy-and-hold weights drifting from the
plan's (what a rolling backtest sends).

tools/bench_portfolios.py's method: HIP events around batches of `--reps` back-to-back calls on one
stream sized to ~20 ms, `--warmup` untimed batches first, the median of `--batches` batches with
the min-max spread; the contenders alternate batch by batch.  Prints one JSON line per config
and, with --out, writes them to a file.

    python tools/bench_dynamic.py --out profiles/dynamic/bench_dynamic.jsonl
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


def param_path(copula, base, T):
    """(T, n) parameters around `base` (cvq_static.copula_params' packing): a slow sine, every
    entry inside the entry point's bounds; a Student nu stays put."""
    import numpy as np
    base = np.atleast_1d(np.asarray(base, dtype=np.float64))
    s = np.sin(np.arange(T) / 50.0)[:, None]
    if copula in ("gumbel", "gumbel_survival"):
        return np.clip(1.0 + (base - 1.0) * (1.0 + 0.3 * s), 1.0, 16.0)
    if copula == "plackett":
        return base * (1.0 + 0.3 * s)
    out = np.tile(base, (T, 1))
    k = 1 if copula == "student" else 0
    out[:, k:] = np.clip(base[k:] * (1.0 + 0.2 * s), -0.95, 0.95)       # scaled together: stays positive definite
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="2,3,5,4", help="comma list of BASELINE configs")
    ap.add_argument("--reps", type=int, default=0, help="calls per timed batch (0: sized to ~20 ms per batch)")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from copula_var import _native as N
    from copula_var import dynamic, engine, synthetic

    N.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    lines = []
    for cfg_no in (int(v) for v in a.configs.split(",")):
        cfg = synthetic.baseline_configs()[cfg_no]
        c, ipt, uvs, ggp, _, T, _, block = bench.build_inputs(cfg, cfg.T, 0, 1, 0)
        dens, x, step, combos = ggp
        d_a = torch.tensor(ipt[0], dtype=torch.float64, device=dev).contiguous()
        d_b = torch.tensor(ipt[1], dtype=torch.float64, device=dev).contiguous() if c.model == "msm" else None
        stream = torch.cuda.current_stream().cuda_stream
        base = np.atleast_1d(np.asarray(c.copula_params(), dtype=np.float64))
        w0 = np.asarray(c.weights, dtype=np.float64)
        own = (np.tile(base, (T, 1)), np.tile(w0, (T, 1)), np.full(T, 0.25))
        path = (param_path(c.copula, base, T), dynamic.drift_weights(block[c.n_in:c.n_in + T], w0),
                0.25 + 0.01 * np.sin(np.arange(T) / 30.0))
        plan = engine.QuadraturePlan(c.model, c.copula, c.dim, x, step, dens, combos, w0, base, vol_states=uvs,
                                     device=0)
        try:
            plan.set_stream(stream)
            plan.set_dates_device(T, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None)
            args = engine.solve_args(0.25)
            outs = {k: {L: torch.empty((3, T, L), dtype=torch.float64, device=dev) for L in LEVELS}
                    for k in ("quant", "own", "path")}

            def quant(L):
                o = outs["quant"][L]
                return lambda: plan.quantiles_device(args, LEVELS[L], o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())

            def dyn(kind, rec, L):
                o = outs[kind][L]
                return lambda: plan.dynamic_quantiles_device(args, LEVELS[L], o[0].data_ptr(), o[1].data_ptr(),
                                                             o[2].data_ptr(), copula_params=rec[0], weights=rec[1],
                                                             ptf_mean=rec[2])

            fns = {}
            for L in LEVELS:                                # the contenders alternate
                fns[f"quant{L}"] = quant(L)
                fns[f"own{L}"] = dyn("own", own, L)
                fns[f"path{L}"] = dyn("path", path, L)

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
                   "dim": c.dim, "reps": reps, "batches": a.batches}
            for k in fns:
                rec[f"{k}_us"] = round(1e3 * med[k], 2)
                rec[f"{k}_us_min_max"] = [round(1e3 * min(ts[k]), 2), round(1e3 * max(ts[k]), 2)]
            for L in LEVELS:
                rec[f"own{L}_over_quant{L}"] = round(med[f"own{L}"] / med[f"quant{L}"], 3)
                rec[f"path{L}_over_quant{L}"] = round(med[f"path{L}"] / med[f"quant{L}"], 3)
                rec[f"quant{L}_spread"] = round(max(ts[f"quant{L}"]) / min(ts[f"quant{L}"]), 3)
                # the plan's own records reproduce cvq_quantiles bit for bit, checked on what was just timed
                rec[f"identical_L{L}"] = bool(all(
                    torch.equal(torch.nan_to_num(outs["own"][L][k], nan=-1.0),
                                torch.nan_to_num(outs["quant"][L][k], nan=-1.0)) for k in range(3)))
                rec[f"nan_path_L{L}"] = int(torch.isnan(outs["path"][L][0]).sum().item())
            rec["scratch_bytes_L3"] = plan.dynamic_scratch(3)
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
