"""ValueAtRiskCalcualtion -- the reference's VaR driver (utils/calc_var_class.py:8-309)
with the quadrature and the bisection on the GPU.

Same constructor, same pipeline order, same ``calc_var(obj_var, first_guess,
second_guess) -> np.ndarray (T,)`` and ``compute_integral(bounds) -> (T,)``
(the seam SURVEY.md §8b names).  Underneath:

* ``compute_integral`` is one device slab launch (cvq_slab) instead of
  np.unique + nested-grid build + joblib over dates (calc_var_class.py:179-212);
* ``calc_var`` is one device solve (cvq_solve: one k_compact launch for 2 assets,
  one k_sorted launch for 3, each with the finalize fused in) that reproduces
  calc_var + bisection_algorithm (:95-177, :250-309) with quirks Q1-Q4 -- results
  bit-identical to the reference on the golden cases (tests/test_gpu_parity.py,
  tests/test_driver_gpu.py);
* ``bisection_algorithm`` / ``adjust_integral`` keep the reference's host loop
  over device slabs, for callers that drive the bisection themselves.

The in-sample stage runs as the reference's does (model fits, marginals, the IFM
copula fit of calc_copula_params, :77-82) on the device likelihoods.

Keyword-only additions: ``copula_params`` (packed copula parameters that override
the IFM fit), ``device``, ``strategy`` ("auto" = COMPACT for 2-asset MSM, SORTED for
3 assets and for 2-asset GARCH / UKF, engine.auto_strategy; or "direct", "prefix", "sorted", "compact").
"""
from __future__ import annotations

import time

import numpy as np

from ..conditional import marginal_quantile
from ..data_loader.load_data import IndexReturnsRetriever
from ..engine import QuadraturePlan


DEVICE_MODELS = ("msm", "garch", "mean_reverting")
DEVICE_COPULAS = ("student", "gaussian", "plackett", "gumbel", "gumbel_survival", "frank", "joe", "joe_survival")


def check_device_adapter(method) -> None:
    """The device evaluates the integrand itself (integrated_function is not a per-node
    callback here), so an adapter must name a device model and copula: `model_kind` in
    DEVICE_MODELS and `copula_kind` in DEVICE_COPULAS, as the factory's adapters do.  A
    user-written VaRCalculationMethod without them fails here, before any in-sample work."""
    model = getattr(method, "model_kind", None)
    copula = getattr(method, "copula_kind", None)
    bad = []
    if model not in DEVICE_MODELS:
        bad.append(f"model_kind={model!r} (one of {DEVICE_MODELS})")
    if copula not in DEVICE_COPULAS:
        bad.append(f"copula_kind={copula!r} (one of {DEVICE_COPULAS})")
    if bad:
        raise ValueError(
            f"{type(method).__name__} cannot run on the device engine: it needs " + " and ".join(bad)
            + ". The integrand is evaluated inside the HIP quadrature (cvq_slab / cvq_solve), so a "
              "VaRCalculationMethod must be one of the factory's (copula x model) adapters or "
              "declare those two attributes; a Python integrated_function is not called "
              "(INTEGRATION.md, 'Plug-in adapters').")


class ValueAtRiskCalcualtion:
    def __init__(self, tickers, start_date, in_sample_data_num, VaRCalculationMethod, end_date=None,
                 num_points=100, weights=np.array([0.5, 0.5]), *args, copula_params=None, device=0,
                 strategy="auto", **kwargs):
        check_device_adapter(VaRCalculationMethod)
        self.num_points = num_points
        self.tickers = tickers
        self.start_date = start_date
        self.in_sample_data_num = in_sample_data_num
        self.VaRCalculationMethod = VaRCalculationMethod
        self.end_date = end_date
        self.weights = weights
        self.device = int(device)
        if hasattr(VaRCalculationMethod, "set_device"):
            VaRCalculationMethod.set_device(self.device)

        (self.in_sample_dict, self.rolling_windows_dict, self.mean_returns, self.end_date, self.out_sample_data,
         self.out_sample_N, self.dim, self.ptf_mean) = self.get_in_sample_data()

        self.in_sample_params = self.retrieve_param_in_sample(*args, **kwargs)
        self.marginals, self.densities, self.vol_states_array = self.calc_marg_and_densities(*args, **kwargs)
        self.copula_params = np.atleast_1d(np.asarray(
            copula_params if copula_params is not None else self.calc_copula_params(), dtype=np.float64))
        self.integrations_params_t, self.integrations_params_static, self.grids_generations_params = (
            self.integration_params_retrieval())

        self.copula_function = VaRCalculationMethod.copula_density
        self.unpack_copula_params = VaRCalculationMethod.unpack_copula_params
        self.integrated_function = VaRCalculationMethod.integrated_function

        densities, x_values, step_size, combos = self.grids_generations_params
        self.plan = QuadraturePlan(VaRCalculationMethod.model_kind, VaRCalculationMethod.copula_kind, self.dim,
                                   x_values, step_size, densities, combos, self.weights, self.copula_params,
                                   vol_states=self.integrations_params_static, device=self.device,
                                   strategy=strategy)
        self.plan.set_dates(self.integrations_params_t)

    # ----------------------------------------------------------- pipeline (:47-93)
    def get_in_sample_data(self):
        retriever = IndexReturnsRetriever(tickers=self.tickers, start_date=self.start_date,
                                          N=self.in_sample_data_num, weights=self.weights, end_date=self.end_date)
        return retriever.get_insample_data()

    def retrieve_param_in_sample(self, *args, **kwargs):
        return self.VaRCalculationMethod.model_params_insample(self.in_sample_dict, *args, **kwargs)

    def calc_marg_and_densities(self, *args, **kwargs):
        return self.VaRCalculationMethod.calculate_marginals_and_densities_in_sample(
            self.in_sample_dict, self.in_sample_params, *args, **kwargs)

    def calc_copula_params(self):
        best_fit = self.VaRCalculationMethod.copula_or_correl_params_insample(self.marginals, self.densities)
        return self.VaRCalculationMethod.copula_integrations_params(best_fit)

    def integration_params_retrieval(self):
        return self.VaRCalculationMethod.integration_params_retrieval(
            self.dim, self.rolling_windows_dict, self.in_sample_params, self.num_points, self.vol_states_array)

    # ----------------------------------------------------------- VaR (:95-177)
    def calc_var(self, obj_var=0.05, first_guess=-3, second_guess=(-3.5, -2)):
        """Per-date VaR (T,) = solved quantile + ptf_mean, one device solve."""
        start_time = time.time()
        var, self.last_iterations = self.plan.calc_var(self.ptf_mean, obj_var, first_guess, second_guess)
        print(f"calc_var function execution time: {time.time() - start_time:.4f} seconds")
        return var

    def calc_es(self, obj_var=0.05, first_guess=-3, second_guess=(-3.5, -2), var=None):
        """Per-date Expected Shortfall (T,): the mean portfolio return given that it falls at or
        below the VaR, on the VaR's own nested grid (no reference counterpart).  var=None solves
        the VaR first (calc_var with these arguments).  The mass found below each VaR is kept
        in last_tail_mass."""
        if var is None:
            var = self.calc_var(obj_var, first_guess, second_guess)
        es, self.last_tail_mass = self.plan.expected_shortfall(np.asarray(var, dtype=np.float64), self.ptf_mean)
        return es

    def calc_es_contributions(self, var=None, obj_var=0.05, first_guess=-3, second_guess=(-3.5, -2)):
        """Per-asset contributions to the Expected Shortfall (T, dim), column c = tickers[c]: the
        Euler allocation w_c E[x_c | portfolio <= VaR] on the VaR's own nested grid (no reference
        counterpart).  A row sums to calc_es's value minus ptf_mean (the portfolio mean is not
        allocated).  var=None solves the VaR first.  The mass found below each VaR is kept in
        last_tail_mass."""
        if var is None:
            var = self.calc_var(obj_var, first_guess, second_guess)
        contrib, self.last_tail_mass = self.plan.es_contributions(np.asarray(var, dtype=np.float64), self.ptf_mean)
        return contrib

    def calc_var_contributions(self, var=None, band=0.25, obj_var=0.05, first_guess=-3, second_guess=(-3.5, -2)):
        """Per-asset contributions to the VaR (T, dim): w_c E[x_c | portfolio = VaR] estimated
        over the band (VaR - band, VaR] of portfolio levels (DESIGN.md §4 justifies the default
        band from the grid spacing).  A row sums to the band's mean level, kept in
        last_band_mean (T,); the band's mass is kept in last_tail_mass."""
        if var is None:
            var = self.calc_var(obj_var, first_guess, second_guess)
        contrib, self.last_band_mean, self.last_tail_mass = self.plan.var_contributions(
            np.asarray(var, dtype=np.float64), self.ptf_mean, band)
        return contrib

    def calc_quantiles(self, levels=(0.05,)):
        """(var, es), each (T, L): the exact quantile of the nested-grid measure at every level
        (plain bisection, none of calc_var's quirks: where calc_var's result lies above -2 + ptf_mean
        it is not the obj_var quantile) and the Expected Shortfall below it, all
        levels in one device call (no reference counterpart).  calc_var stays the reference's
        number.  The masses found below each quantile are kept in last_tail_mass (T, L)."""
        var, es, self.last_tail_mass = self.plan.quantiles(levels, self.ptf_mean)
        return var, es

    def calc_distribution(self, edges):
        """(mass, m1), each (T, B): the mass and first moment of the nested-grid measure in the bins
        (edges[b], edges[b+1]] of a ladder of portfolio returns (ptf_mean included, as calc_var's
        values are) -- (B + 1,) for every date or (T, B + 1) per date -- all bins in one device
        sweep (no reference counterpart).  m1 is in centred levels, as expected_shortfall's m1.
        The measure is not normalised: divide by the bin sum up to +inf for probabilities."""
        return self.plan.distribution(np.asarray(edges, dtype=np.float64) - self.ptf_mean)

    def calc_pit(self, realised):
        """u (T,): the probability integral transform F_t(r_t) / F_t(+inf) of each date's realised
        portfolio return under that date's forecast (no reference counterpart); NaN where the
        return is NaN."""
        from ..backtest import pit
        return pit(self.plan, realised, self.ptf_mean)

    def backtest(self, realised, alpha=0.05, var=None, es=None):
        """The backtest table (copula_var.backtest.backtest_table) of a VaR series against the
        realised portfolio returns (T,): hit counts, Kupiec, Christoffersen, the pinball score,
        Berkowitz on this run's PITs and, when `es` is given, Acerbi-Szekely's Z2.  var=None solves
        calc_var at obj_var = alpha first.  The PITs are kept in last_pit."""
        from ..backtest import backtest_table
        if var is None:
            var = self.calc_var(alpha)
        self.last_pit = self.calc_pit(realised)
        return backtest_table(realised, var, es=es, pit=self.last_pit, alpha=alpha)

    def calc_portfolio_quantiles(self, weights, levels=(0.05,)):
        """(var, es), each (T, P, L): calc_quantiles for P candidate weight vectors (P, dim) on this
        run's fitted measure, all candidates in one device call per 64 (no reference
        counterpart).  Row p is what calc_quantiles returns from a run constructed with
        weights=weights[p], its portfolio mean included.  The weights follow the constructor's own
        convention, quirk Q10: weights[p, k] is NOT ticker k's weight unless the weights are
        equal -- ticker c carries QuadraturePlan.axis_weights' entry, weights[p, c + 1] for
        c < dim - 1 and weights[p, 0] for the last ticker; weights[p, 0] must be > 0.  The masses
        found below each quantile are kept in last_tail_mass (T, P, L)."""
        w = np.asarray(weights, dtype=np.float64)
        if w.ndim != 2 or w.shape[1] != self.dim:
            raise ValueError(f"weights must have shape (P, {self.dim})")
        means = np.array([self.mean_returns[tk] for tk in self.mean_returns], dtype=np.float64)
        ptf_mean = np.array([np.sum(means * wp) for wp in w])       # load_data.py:128 per candidate
        var, es, self.last_tail_mass = self.plan.portfolio_quantiles(w, levels, ptf_mean)
        return var, es

    def dynamic_ptf_mean(self, weights=None):
        """The portfolio mean of every date: the loader's formula (load_data.py:128) applied to
        that date's weights (T, dim); None: the constructor's own mean on every date."""
        if weights is None:
            return float(self.ptf_mean)
        means = np.array([self.mean_returns[tk] for tk in self.mean_returns], dtype=np.float64)
        return np.array([np.sum(means * wt) for wt in np.asarray(weights, dtype=np.float64)])

    def calc_dynamic_quantiles(self, levels=(0.05,), copula_params=None, weights=None):
        """(var, es), each (T, L): calc_quantiles where every date has copula parameters and weights
        of its own (no reference counterpart) -- a refitted or DCC-style dependence path, a
        buy-and-hold portfolio whose weights drift (copula_var.dynamic builds both).
        copula_params (T, n) in this run's own packing (self.copula_params; a Student nu must stay
        the run's), weights (T, dim) in the constructor's convention (quirk Q10, see
        calc_portfolio_quantiles; weights[t, 0] > 0); None keeps the run's own.  Row t is what
        calc_quantiles returns for date t from a run constructed with those parameters and
        weights, its portfolio mean included.  All dates in one device call.  The masses found
        below each quantile are kept in last_tail_mass (T, L)."""
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.shape != (self.plan.T, self.dim):
                raise ValueError(f"weights must have shape ({self.plan.T}, {self.dim})")
        var, es, self.last_tail_mass = self.plan.dynamic_quantiles(levels, copula_params, weights,
                                                                   self.dynamic_ptf_mean(weights))
        return var, es

    def _dynamic_weights(self, weights):
        if weights is None:
            return None
        weights = np.asarray(weights, dtype=np.float64)
        if weights.shape != (self.plan.T, self.dim):
            raise ValueError(f"weights must have shape ({self.plan.T}, {self.dim})")
        return weights

    def calc_dynamic_distribution(self, edges, copula_params=None, weights=None):
        """(mass, m1), each (T, B): calc_distribution under calc_dynamic_quantiles' per-date copula
        parameters and weights (no reference counterpart).  edges are portfolio returns, the
        date's own mean included (dynamic_ptf_mean of that date's weights), (B + 1,) for every date
        or (T, B + 1) per date.  Row t is what calc_distribution returns for date t from a run
        constructed with those parameters and weights.  All dates in one device sweep."""
        weights = self._dynamic_weights(weights)
        e = np.asarray(edges, dtype=np.float64)
        mean = self.dynamic_ptf_mean(weights)
        if np.ndim(mean) == 1:
            e = np.broadcast_to(e, (self.plan.T, e.shape[-1])) - mean[:, None]
        else:
            e = e - mean
        return self.plan.dynamic_distribution(e, copula_params, weights)

    def calc_dynamic_pit(self, realised, copula_params=None, weights=None):
        """u (T,): calc_pit under calc_dynamic_quantiles' per-date model -- the PIT of each date's
        realised portfolio return under the forecast that produced that date's dynamic VaR (no
        reference counterpart); NaN where the return is NaN."""
        from ..backtest import pit
        weights = self._dynamic_weights(weights)
        return pit(self.plan, realised, self.dynamic_ptf_mean(weights), copula_params=copula_params,
                   weights=weights)

    def dynamic_backtest(self, realised, alpha, var, es=None, copula_params=None, weights=None):
        """The backtest table of a calc_dynamic_quantiles VaR series (T,) at level alpha against
        the realised portfolio returns: `backtest` with Berkowitz on the PITs of the per-date
        model (calc_dynamic_pit with the same copula_params and weights), kept in
        last_dynamic_pit."""
        from ..backtest import backtest_table
        self.last_dynamic_pit = self.calc_dynamic_pit(realised, copula_params, weights)
        return backtest_table(realised, var, es=es, pit=self.last_dynamic_pit, alpha=alpha)

    def oos_pits(self):
        """(u, pdf), each (T, dim): the forecast marginals' CDF and density at the realised centred
        return of every out-of-sample date (copula_var.dynamic.oos_pits on this run's forecasts)."""
        from ..data_loader.load_data import centred_series
        from ..dynamic import oos_pits
        r = centred_series(self.rolling_windows_dict, list(self.tickers))
        T = self.plan.T
        return oos_pits(self.VaRCalculationMethod.model_kind, self.integrations_params_t,
                        self.integrations_params_static, r[self.in_sample_data_num:self.in_sample_data_num + T])

    def rolling_copula_params(self, window, every=21):
        """(params (T, n), info): this run's copula refitted every `every` out-of-sample dates on the
        last `window` rows of [in-sample marginals, then the out-of-sample PITs before the date]
        (copula_var.dynamic.rolling_copula_params); a Student nu stays the run's."""
        from ..dynamic import rolling_copula_params
        u, pdf = self.oos_pits()
        return rolling_copula_params(self.VaRCalculationMethod.copula_kind, self.marginals, self.densities, u, pdf,
                                     window, every, static_params=self.copula_params, device=self.device)

    def gas_copula_params(self, fit=None):
        """(params (T, n), info): this run's copula parameter on every out-of-sample date from the
        score-driven recursion fitted once on the in-sample marginals and filtered through the
        out-of-sample PITs before each date (copula_var.dynamic.gas_copula_params); a Student nu
        stays the run's."""
        from ..dynamic import gas_copula_params
        u, _ = self.oos_pits()
        return gas_copula_params(self.VaRCalculationMethod.copula_kind, self.marginals, u, self.copula_params, fit=fit,
                                 device=self.device, in_sample_densities=self.densities)

    def _asset_index(self, asset) -> int:
        if isinstance(asset, str):
            tickers = list(self.tickers)
            if asset not in tickers:
                raise ValueError(f"{asset!r} is not one of the tickers {tickers}")
            return tickers.index(asset)
        asset = int(asset)
        if not 0 <= asset < self.dim:
            raise ValueError(f"asset must be in [0, {self.dim}) or a ticker")
        return asset

    def calc_covar(self, asset, stress=0.05, levels=(0.05,), benchmark=(0.25, 0.75)):
        """(covar, coes, delta): the portfolio's exact quantile and Expected Shortfall at every
        level, each (T, L), given that `asset` (an index or a ticker) is in distress -- at or below
        the `stress` quantile of its own forecast marginal -- and delta = covar under stress minus
        covar under the benchmark event, the asset between its benchmark[0] and benchmark[1]
        quantiles (Adrian-Brunnermeier's Delta-CoVaR in Girardi-Ergun's "<=" form; no reference
        counterpart).  delta is NaN where either covar is; benchmark=None skips the second call
        and returns delta = None.  The stress call's event mass is kept in last_event_mass (T,)
        and the masses found below each covar in last_tail_mass (T, L)."""
        c = self._asset_index(asset)
        model = self.VaRCalculationMethod.model_kind
        per, vs = self.integrations_params_t, self.integrations_params_static
        T = self.plan.T
        ev = np.column_stack((np.full(T, -np.inf), marginal_quantile(model, per, vs, c, stress)))
        covar, coes, self.last_tail_mass, self.last_event_mass = self.plan.conditional_quantiles(
            c, ev, levels, self.ptf_mean)
        if benchmark is None:
            return covar, coes, None
        band = np.column_stack((marginal_quantile(model, per, vs, c, benchmark[0]),
                                marginal_quantile(model, per, vs, c, benchmark[1])))
        base = self.plan.conditional_quantiles(c, band, levels, self.ptf_mean)[0]
        return covar, coes, covar - base

    def compute_integral(self, bounds):
        """I_t(a, b] for every date t (calc_var_class.py:179-212), one device launch."""
        return self.plan.compute_integral(np.asarray(bounds, dtype=np.float64))

    def adjust_integral(self, new_result, prev_results, bounds, prev_upper):
        """calc_var_class.py:214-248 (exact float equality)."""
        return np.where(bounds[:, 0] == prev_upper, prev_results + new_result, prev_results - new_result)

    def bisection_algorithm(self, obj_var, bisection_bounds, prev_result, upper_stack, prev_upper,
                            tolerance=1e-6):
        """calc_var_class.py:250-309 on the host, each slab integral on the device."""
        lower, upper = bisection_bounds[:, 0].copy(), bisection_bounds[:, 1].copy()
        while np.any(upper - lower > tolerance):
            mid = (lower + upper) / 2
            b = np.where(upper_stack[:, None], np.column_stack((lower, mid)), np.column_stack((mid, upper)))
            result = self.adjust_integral(self.compute_integral(b), prev_result, b, prev_upper)
            if np.all(result == 0):
                break
            upper_stack = result < obj_var
            lower = np.where(~upper_stack, lower, mid)
            upper = np.where(upper_stack, upper, mid)
            prev_result = result
            prev_upper = mid
        return (lower + upper) / 2

    def close(self):
        self.plan.close()
