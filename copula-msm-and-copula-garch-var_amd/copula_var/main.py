"""Command-line driver mirroring the reference's main.py (main.py:25-75), offline.

    python -m copula_var.main --prices prices.csv --tickers ^GSPC ^IXIC \\
        --start 2009-04-15 --end 2015-10-12 --n-in 1135 --copula student \\
        --estimation garch msm --num-points 100 --k 4 --out var.csv --plot var.png

The reference downloads adjusted closes with yfinance; here they come from a CSV
(date index, one column per ticker), converted to the reference's log returns x 100
and put into the loader's cache under the reference's key (load_data.py:21-24).
Then, per estimation type, the pipeline main.py runs: factory -> ValueAtRiskCalcualtion
(in-sample fit, marginals, copula fit, forecasts) -> calc_var, all on the device.
The VaR series (one column per estimation type) and the equal-weight portfolio
returns go to --out; --plot saves main.py's plot_var_and_returns figure to a file.
--backtest tests each VaR series against those portfolio returns (copula_var.backtest), the
dynamic ones (--rolling-copula, --gas-copula, --drift-weights) under their own per-date predictive distribution.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np
import pandas as pd

from . import backtest, dynamic, portfolios
from .data_loader.load_data import SharedCacheIndexReturns, load_returns_csv
from .utils.calc_var_class import ValueAtRiskCalcualtion
from .utils.factory import ValueAtRiskCalculationFactory


def plot_var_and_returns(series: dict, portfolio_returns, path: str) -> None:
    """main.py:6-21, saved to `path` instead of shown."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.figure(figsize=(10, 6))
    for (name, var), style in zip(series.items(), ["-", "--", "-."]):
        plt.plot(range(len(var)), var, label=f"{name.upper()} VaR", linestyle=style, alpha=0.8)
    plt.plot(range(len(portfolio_returns)), portfolio_returns, label="Portfolio Returns", linestyle=":", alpha=0.8)
    plt.title("VaR and Portfolio Returns Over Time")
    plt.xlabel("Time")
    plt.ylabel("Value")
    plt.legend()
    plt.grid(True)
    plt.savefig(path)
    plt.close()


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--prices", required=True, help="CSV of adjusted closes (date index, one column per ticker)")
    ap.add_argument("--returns", action="store_true", help="the CSV already holds log returns x 100")
    ap.add_argument("--tickers", nargs="+", required=True)
    ap.add_argument("--start", required=True)
    ap.add_argument("--end", default=None)
    ap.add_argument("--n-in", type=int, default=1135, help="in-sample days (main.py:34)")
    ap.add_argument("--copula", default="student",
                    choices=["student", "gaussian", "plackett", "gumbel", "gumbel_survival", "frank", "joe",
                             "joe_survival"])
    ap.add_argument("--estimation", nargs="+", default=["garch", "msm"], choices=["garch", "msm", "mean_reverting"])
    ap.add_argument("--num-points", type=int, default=100)
    ap.add_argument("--k", type=int, default=4, help="MSM components")
    ap.add_argument("--weights", type=float, nargs="+", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="CSV of the VaR series")
    ap.add_argument("--plot", default=None, help="PNG of main.py's VaR / returns plot")
    ap.add_argument("--es", action="store_true",
                    help="also compute the Expected Shortfall below each VaR (an <estimation>_es column in --out)")
    ap.add_argument("--contributions", action="store_true",
                    help="also compute each asset's Euler contribution to the Expected Shortfall (implies --es; "
                         "<estimation>_esc_<ticker> columns in --out, summing to <estimation>_es minus the "
                         "portfolio mean)")
    ap.add_argument("--exact-levels", type=float, nargs="+", default=None, metavar="A",
                    help="also compute the exact quantile (true VaR, without calc_var's reproduced quirks) and its "
                         "Expected Shortfall at these levels: qvar_<estimation>_<level> / qes_<estimation>_<level> "
                         "columns in --out")
    ap.add_argument("--covar", default=None, metavar="TICKER",
                    help="also compute the portfolio's conditional quantile and Expected Shortfall given that this "
                         "ticker is at or below its --covar-stress quantile (CoVaR / CoES), and the difference to the "
                         "quantile given the ticker between its quartiles (Delta-CoVaR), at the levels of "
                         "--exact-levels (default 0.05): covar_<estimation>_<ticker>_<level>, coes_... and "
                         "dcovar_... columns in --out")
    ap.add_argument("--covar-stress", type=float, default=0.05, metavar="Q",
                    help="the stress event's probability under the ticker's own forecast marginal (default 0.05)")
    ap.add_argument("--weight-grid", type=int, default=None, metavar="STEPS",
                    help="also compute the exact quantile and Expected Shortfall of every candidate weight vector "
                         "k / STEPS (non-negative integers summing to STEPS) at the levels of --exact-levels "
                         "(default 0.05) in one batched device call, and the candidate with the smallest expected "
                         "loss per date: wbest_<estimation>_<ticker>_<level> (that candidate's weight on the ticker) "
                         "and wbest_es_<estimation>_<level> columns in --out")
    ap.add_argument("--rolling-copula", type=int, default=None, metavar="WINDOW",
                    help="also compute the exact quantile and Expected Shortfall at the levels of --exact-levels "
                         "under copula parameters refitted on the last WINDOW rows before each refit date "
                         "(in-sample rows, then the realised out-of-sample rows; a Student nu stays fixed): "
                         "dvar_<estimation>_<level> / des_<estimation>_<level> columns in --out, the parameter "
                         "path in dparam_<estimation>_<k>")
    ap.add_argument("--gas-copula", action="store_true",
                    help="as --rolling-copula, but the parameter path comes from a score-driven (GAS) recursion: "
                         "three parameters (omega, alpha, beta) fitted once on the in-sample marginals on the "
                         "device, then filtered through the realised out-of-sample rows; the same dvar / des / "
                         "dparam columns.  Needs --exact-levels; not with --rolling-copula")
    ap.add_argument("--refit-every", type=int, default=21, metavar="STEP",
                    help="out-of-sample dates between two refits of --rolling-copula (default 21)")
    ap.add_argument("--drift-weights", action="store_true",
                    help="the dvar / des columns follow a buy-and-hold portfolio: --weights on the first date, then "
                         "drifting with the realised returns (with or without --rolling-copula)")
    ap.add_argument("--backtest", action="store_true",
                    help="backtest each estimation's VaR against the realised portfolio returns (the plotted "
                         "series): hit counts, Kupiec, Christoffersen, pinball score, Berkowitz on the PITs, "
                         "Acerbi-Szekely's Z2 with --es, and one more table per level of --exact-levels; "
                         "pit_<estimation> / hit_<estimation> columns in --out.  With --rolling-copula or "
                         "--drift-weights: one more table per level for the dvar / des columns, with Berkowitz on "
                         "the PITs of the per-date model that produced them (not the static one); "
                         "dpit_<estimation> / dhit_<estimation>_<level> columns in --out")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)

    df = load_returns_csv(a.prices, prices=not a.returns)[a.tickers]
    SharedCacheIndexReturns.returns_cache[(tuple(a.tickers), a.start, a.end)] = df
    weights = np.array(a.weights if a.weights else [1.0 / len(a.tickers)] * len(a.tickers))
    a.es = a.es or a.contributions
    covar_levels = a.exact_levels or [0.05]
    if a.covar and a.covar not in a.tickers:
        raise SystemExit(f"--covar {a.covar}: not one of --tickers")
    if a.weight_grid is not None and a.weight_grid < 1:
        raise SystemExit("--weight-grid: STEPS must be >= 1")
    dynamic_on = a.rolling_copula is not None or a.drift_weights or a.gas_copula
    if dynamic_on and not a.exact_levels:
        raise SystemExit("--rolling-copula, --gas-copula, --refit-every and --drift-weights need --exact-levels")
    if a.gas_copula and a.rolling_copula is not None:
        raise SystemExit("--gas-copula and --rolling-copula are two producers of one parameter path: choose one")
    if a.gas_copula and len(a.tickers) != 2 and a.copula in ("gaussian", "student", "plackett"):
        raise SystemExit(f"--gas-copula: the score-driven {a.copula} copula is built for 2 assets")
    if a.refit_every != 21 and a.rolling_copula is None:
        raise SystemExit("--refit-every needs --rolling-copula")
    if a.rolling_copula is not None and a.rolling_copula < 2:
        raise SystemExit("--rolling-copula: WINDOW must be >= 2")
    if a.refit_every < 1:
        raise SystemExit("--refit-every: STEP must be >= 1")
    out, runs, es, esc, exact, covar, wbest, dyn = {}, {}, {}, {}, {}, {}, {}, {}
    bt, dbt, dyn_w = {}, {}, {}
    for est in a.estimation:
        calc = ValueAtRiskCalculationFactory.create_var_calculator(copula_type=a.copula, estimation_type=est)
        kw = {"k": a.k} if est == "msm" else {}
        runs[est] = ValueAtRiskCalcualtion(a.tickers, a.start, a.n_in, calc, a.end, num_points=a.num_points,
                                           weights=weights, device=a.device, **kw)
        out[est] = runs[est].calc_var()
        print(f"{est}/{a.copula}: {out[est].size} dates, mean VaR {np.nanmean(out[est]):.4f}", file=sys.stderr)
        if a.es:
            es[est] = runs[est].calc_es(var=out[est])
            print(f"{est}/{a.copula}: mean ES {np.nanmean(es[est]):.4f}", file=sys.stderr)
        if a.contributions:
            esc[est] = runs[est].calc_es_contributions(var=out[est])
            print(f"{est}/{a.copula}: mean ES contributions " +
                  ", ".join(f"{t} {m:.4f}" for t, m in zip(a.tickers, np.nanmean(esc[est], axis=0))), file=sys.stderr)
        if a.exact_levels:
            exact[est] = runs[est].calc_quantiles(a.exact_levels)
            for i, lv in enumerate(a.exact_levels):
                print(f"{est}/{a.copula}: mean exact VaR at {lv:g}: {np.nanmean(exact[est][0][:, i]):.4f}",
                      file=sys.stderr)
        if a.covar:
            covar[est] = runs[est].calc_covar(a.covar, a.covar_stress, covar_levels)
            for i, lv in enumerate(covar_levels):
                print(f"{est}/{a.copula}: mean CoVaR at {lv:g} given {a.covar}: {np.nanmean(covar[est][0][:, i]):.4f}",
                      file=sys.stderr)
        if a.weight_grid:
            cand = portfolios.weight_lattice(len(a.tickers), a.weight_grid)
            p_es = runs[est].calc_portfolio_quantiles(cand, covar_levels)[1]
            pick, best = portfolios.min_es(p_es)
            # the candidate's weight per ticker, through the Q10 axis mapping (QuadraturePlan.axis_weights)
            by_ticker = np.concatenate((cand[:, 1:], cand[:, :1]), axis=1)
            wbest[est] = (np.where(pick[..., None] >= 0, by_ticker[np.maximum(pick, 0)], np.nan), best)
            with np.errstate(all="ignore"):
                mean_es = np.nanmean(p_es, axis=0)
            for p, wv in enumerate(by_ticker):
                print(f"{est}/{a.copula}: candidate " + ", ".join(f"{t} {x:g}" for t, x in zip(a.tickers, wv)) +
                      ": mean ES " + ", ".join(f"{lv:g}: {mean_es[p, i]:.4f}" for i, lv in enumerate(covar_levels)),
                      file=sys.stderr)
        if dynamic_on:
            run = runs[est]
            T = run.plan.T
            path = np.tile(run.copula_params, (T, 1))
            if a.rolling_copula is not None:
                path, info = run.rolling_copula_params(a.rolling_copula, a.refit_every)
                print(f"{est}/{a.copula}: rolling copula, window {a.rolling_copula}: {len(info['refits'])} refits, "
                      f"{len(info['failed'])} failed; parameters from "
                      + ", ".join(f"{v:.4f}" for v in path[0]) + " to " + ", ".join(f"{v:.4f}" for v in path[-1]),
                      file=sys.stderr)
            if a.gas_copula:
                path, info = run.gas_copula_params()
                fit = info["fit"]
                print(f"{est}/{a.copula}: score-driven copula: omega {fit['omega']:.6f}, alpha {fit['alpha']:.6f}, "
                      f"beta {fit['beta']:.6f}; NLL {fit['nll']:.4f} (static {fit['static_nll']:.4f}), "
                      f"{fit['launches']} launches; parameters from "
                      + ", ".join(f"{v:.4f}" for v in path[0]) + " to " + ", ".join(f"{v:.4f}" for v in path[-1]),
                      file=sys.stderr)
            wt = None
            if a.drift_weights:
                wt = dynamic.drift_weights(run.out_sample_data.to_numpy(dtype=np.float64)[:T], weights)
            dyn[est] = run.calc_dynamic_quantiles(a.exact_levels, copula_params=path, weights=wt) + (path,)
            dyn_w[est] = wt
            for i, lv in enumerate(a.exact_levels):
                print(f"{est}/{a.copula}: mean dynamic VaR at {lv:g}: {np.nanmean(dyn[est][0][:, i]):.4f}",
                      file=sys.stderr)
    first = runs[a.estimation[0]]
    portfolio = first.out_sample_data.mean(axis=1).to_numpy()                    # main.py:73
    if a.backtest:
        for est in a.estimation:
            run = runs[est]
            realised = portfolio[:run.plan.T]
            table = run.backtest(realised, 0.05, var=out[est], es=es.get(est))
            bt[est] = (run.last_pit, backtest.hits(realised, out[est]))
            print(backtest.format_table(table, f"{est}/{a.copula} VaR"), file=sys.stderr)
            for i, lv in enumerate(a.exact_levels or []):
                table = backtest.backtest_table(realised, exact[est][0][:, i], es=exact[est][1][:, i],
                                                pit=run.last_pit, alpha=lv)
                print(backtest.format_table(table, f"{est}/{a.copula} exact VaR at {lv:g}"), file=sys.stderr)
            if est in dyn:                          # the per-date model's own PITs, one sweep for every level
                dvar, des, path = dyn[est]
                dhits = []
                for i, lv in enumerate(a.exact_levels):
                    if i == 0:
                        table = run.dynamic_backtest(realised, lv, dvar[:, 0], es=des[:, 0], copula_params=path,
                                                     weights=dyn_w[est])
                    else:
                        table = backtest.backtest_table(realised, dvar[:, i], es=des[:, i],
                                                        pit=run.last_dynamic_pit, alpha=lv)
                    dhits.append(backtest.hits(realised, dvar[:, i]))
                    print(backtest.format_table(table, f"{est}/{a.copula} dynamic VaR at {lv:g}"), file=sys.stderr)
                dbt[est] = (run.last_dynamic_pit, dhits)
    if a.out:
        idx = first.out_sample_data.index[:len(out[a.estimation[0]])]
        cols = {}
        for k, v in out.items():
            cols[f"var_{k}"] = v
            if k in es:
                cols[f"{k}_es"] = es[k]                     # next to its VaR column
            if k in esc:
                for c, ticker in enumerate(a.tickers):
                    cols[f"{k}_esc_{ticker}"] = esc[k][:, c]
            if k in exact:
                for i, lv in enumerate(a.exact_levels):
                    cols[f"qvar_{k}_{lv:g}"] = exact[k][0][:, i]
                    cols[f"qes_{k}_{lv:g}"] = exact[k][1][:, i]
            if k in covar:
                for i, lv in enumerate(covar_levels):
                    for name, arr in zip(("covar", "coes", "dcovar"), covar[k]):
                        cols[f"{name}_{k}_{a.covar}_{lv:g}"] = arr[:, i]
            if k in dyn:
                for i, lv in enumerate(a.exact_levels):
                    cols[f"dvar_{k}_{lv:g}"] = dyn[k][0][:, i]
                    cols[f"des_{k}_{lv:g}"] = dyn[k][1][:, i]
                for j in range(dyn[k][2].shape[1]):
                    cols[f"dparam_{k}_{j}"] = dyn[k][2][:, j]
            if k in bt:
                cols[f"pit_{k}"] = bt[k][0]
                cols[f"hit_{k}"] = np.where(bt[k][1]["keep"], (portfolio[:len(v)] < v).astype(np.float64), np.nan)
            if k in dbt:
                cols[f"dpit_{k}"] = dbt[k][0]
                for i, lv in enumerate(a.exact_levels):
                    dv = dyn[k][0][:, i]
                    cols[f"dhit_{k}_{lv:g}"] = np.where(dbt[k][1][i]["keep"],
                                                        (portfolio[:len(dv)] < dv).astype(np.float64), np.nan)
            if k in wbest:
                for i, lv in enumerate(covar_levels):
                    for c, ticker in enumerate(a.tickers):
                        cols[f"wbest_{k}_{ticker}_{lv:g}"] = wbest[k][0][:, i, c]
                    cols[f"wbest_es_{k}_{lv:g}"] = wbest[k][1][:, i]
        frame = pd.DataFrame(cols, index=idx)
        frame["portfolio_return"] = portfolio[:len(frame)]
        frame.to_csv(a.out)
    if a.plot:
        plot_var_and_returns(out, portfolio, a.plot)
    return 0


if __name__ == "__main__":
    sys.exit(main())
