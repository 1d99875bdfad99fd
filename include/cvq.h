/*
 * cvq.h -- C ABI of the MI355X copula-VaR quadrature engine (libcvq.so).
 *
 * Drop-in boundary for the hot path of Nassim-cha/copula-MSM-and-copula-Garch-VaR
 * (reference @ 2024-11-25).  Each entry point names the reference interface it
 * replaces.  Plain C: no C++ or torch types, int32 status (0 = ok, < 0 = error,
 * text in cvq_last_error(), thread-local), caller-owned buffers.
 *
 * Memory flags: every buffer argument documented "host|device" is interpreted
 * according to the call's `mem` argument (CVQ_MEM_HOST: the library copies it
 * and returns only when the result is back on the host; CVQ_MEM_DEVICE: a
 * pointer into device memory of the plan's device, used in stream order on the
 * plan's stream, no host synchronisation).
 */
#ifndef CVQ_H
#define CVQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ----------------------------------------------------------------- status */
#define CVQ_OK               0
#define CVQ_ERR_INVALID     -1   /* bad argument (reference: ValueError)            */
#define CVQ_ERR_UNSUPPORTED -2   /* e.g. Plackett with dim != 2, dim not in {2,3}   */
#define CVQ_ERR_HIP         -3   /* HIP runtime error                               */
#define CVQ_ERR_OOM         -4   /* device allocation failed                        */
#define CVQ_ERR_STATE       -5   /* call order (e.g. solve before set_dates)        */
#define CVQ_ERR_RANGE       -6   /* a bound above the plan's v_cap                  */
#define CVQ_ERR_NUMERIC     -7   /* MSM normaliser 0 (calc_prob.py:64), UKF Z<1e-10
                                    (estimate.py:219), bisection budget exceeded    */

#define CVQ_MEM_HOST   0
#define CVQ_MEM_DEVICE 1

/* copula kinds: copulas/{gaussian,student,plackett} */
#define CVQ_GAUSSIAN 0
#define CVQ_STUDENT  1
#define CVQ_PLACKETT 2
/* Gumbel family (no reference counterpart): C(u) = exp(-(sum_i (-log u_i)^theta)^(1/theta)),
 * upper-tail dependent, and its 180-degree rotation c(1 - u) (survival Gumbel, lower-tail
 * dependent: the loss tail of a long portfolio).  copula_params = [theta], 1 <= theta <= 16,
 * dim 2 or 3 (exchangeable), CVQ_STRATEGY_SORTED only.  A node contributes exactly 0 where a
 * marginal CDF value is not strictly inside (0, 1) or the value is not finite (both models). */
#define CVQ_GUMBEL          3
#define CVQ_GUMBEL_SURVIVAL 4
/* Product-form Archimedean kinds (no reference counterpart), copula_params = [theta],
 * dim 2 or 3 (exchangeable), CVQ_STRATEGY_SORTED only, Gumbel's dead-node rule:
 *   Frank  C(u) = -log(1 - prod_i (1 - e^(-theta u_i)) / (1 - e^(-theta))^(d-1)) / theta: no tail
 *          dependence (radially symmetric for 2 assets).  0 < theta <= 32; theta = 0 or NaN is CVQ_ERR_INVALID,
 *          theta < 0 (negative dependence) and theta > 32 are CVQ_ERR_UNSUPPORTED.
 *   Joe    C(u) = 1 - (1 - prod_i (1 - (1 - u_i)^theta))^(1/theta): upper-tail dependent, and its
 *          180-degree rotation c(1 - u) (survival Joe, lower-tail dependent).  1 <= theta <= 16,
 *          with Gumbel's codes (theta < 1 or NaN: CVQ_ERR_INVALID; theta > 16: CVQ_ERR_UNSUPPORTED). */
#define CVQ_FRANK        5
#define CVQ_JOE          6
#define CVQ_JOE_SURVIVAL 7
/* model kinds: utils/model_estimation/model/{msm,garch,mean_reverting}_estimation.py */
#define CVQ_MSM   0
#define CVQ_GARCH 1
#define CVQ_UKF   2

/* quadrature strategy (all reproduce the reference) */
#define CVQ_STRATEGY_PREFIX 0    /* materialise per-date row-prefix joint mass, then solve */
#define CVQ_STRATEGY_DIRECT 1    /* evaluate each slab's nodes inside the solve kernel     */
#define CVQ_STRATEGY_COMPACT 2   /* DIRECT control flow, one barrier per level, one-wave tail */
#define CVQ_STRATEGY_SORTED 3    /* reachable nodes sorted by membership threshold: a slab is
                                    one contiguous range (2-D, and 3-D with n <= 255)       */
#define CVQ_STRATEGY_SWEEP 4     /* SORTED's node order, each bisection cell summed in one pass
                                    with prefix sums at its subtree's mids (2-D)            */

typedef struct cvq_plan cvq_plan;

/* Static quadrature inputs = the reference's grids_generations_params
 * (densities, x_values, step_size, vol_combinations) + integrations_params_static
 * (MSM unique_vol_states) + packed copula params + portfolio weights.
 * Replaces: msm_estimation.py:123-137 / garch_estimation.py:133-145 outputs as
 * consumed by calc_integral.py:8-119. */
typedef struct cvq_static {
    int32_t model;              /* CVQ_MSM | CVQ_GARCH | CVQ_UKF                        */
    int32_t copula;             /* CVQ_GAUSSIAN ... CVQ_JOE_SURVIVAL (the copula kinds above)        */
    int32_t dim;                /* assets: 2 or 3                                        */
    int32_t n;                  /* num_points                                            */
    int32_t q;                  /* unique vol states per asset (GARCH/UKF: 1)            */
    int32_t n_combos;           /* q**dim                                                */
    const double*  x_values;    /* [n]         host                                      */
    const double*  step;        /* [n]         host                                      */
    const double*  densities;   /* [dim][q][n] host (GARCH/UKF: ones)                    */
    const int32_t* combos;      /* [n_combos][dim] host, ij-meshgrid order               */
    const double*  weights;     /* [dim]       host, weights[0] > 0                      */
    const double*  vol_states;  /* [dim][q]    host, MSM unique_vol_states; else NULL    */
    const double*  copula_params; /* packed as copula_integrations_params              */
    int32_t n_copula_params;    /* Student 1+d(d-1)/2, Gaussian d(d-1)/2, Plackett 1, Gumbel / Frank / Joe 1 */
    int32_t strategy;           /* CVQ_STRATEGY_*                                        */
    double  v_cap;              /* largest portfolio level any query may use (e.g. 0)    */
} cvq_static;

/* calc_var arguments: utils/calc_var_class.py:95 (obj_var, first_guess,
 * second_guess) + the constants of :111-114 and :257. */
typedef struct cvq_solve_args {
    double obj_var;             /* 0.05   */
    double first_guess;         /* -3     */
    double second_guess_lo;     /* -3.5   */
    double second_guess_hi;     /* -2     */
    double min_var;             /* -7.5   */
    double max_var;             /* 0      */
    double lower;               /* -100   */
    double tolerance;           /* 1e-6   */
    double ptf_mean;            /* load_data.py:113, added at calc_var_class.py:171 */
} cvq_solve_args;

const char* cvq_last_error(void);
int32_t     cvq_version(void);
int32_t     cvq_device_count(int32_t* count);

/* Plan = one device + one stream + device copies of the static tables. */
int32_t cvq_plan_create(const cvq_static* s, int32_t device, cvq_plan** out);
int32_t cvq_plan_destroy(cvq_plan* plan);
/* Run every later launch of the plan on hip_stream (a hipStream_t, e.g.
 * torch.cuda.current_stream().cuda_stream).  NULL is the HIP null stream (torch's
 * default stream), so the plan's work is ordered with the caller's; a new plan
 * runs on a private non-blocking stream until this is called. */
int32_t cvq_plan_set_stream(cvq_plan* plan, void* hip_stream);
/* Reachable quadrature nodes per date (nodes with level <= v_cap in the box). */
int32_t cvq_plan_info(const cvq_plan* plan, int64_t* reach_nodes, int32_t* rows);

/* Per-kernel timing with HIP events recorded on the plan's stream (bench.py's
 * live roofline).  kind: 0 tables, 1 joint-mass/prefix, 2 solve, 3 finalize,
 * 4 slab, 5 tail moments (cvq_slab_moments / cvq_expected_shortfall and the axis moments
 * cvq_slab_axis_moments / cvq_es_contributions: their tables,
 * partial sums and finish together; cvq_distribution and cvq_dynamic_distribution likewise), 6 exact quantiles (cvq_quantiles and its conditional,
 * batched-weights and per-date-record forms: their tables, passes and updates together).
 * cvq_plan_timing(mask) times the kinds whose bit (1 << kind) is
 * set (0 = off, 0x7F = all) and clears previous records. */
int32_t cvq_plan_timing(cvq_plan* plan, int32_t enable);
int32_t cvq_plan_kernel_time(cvq_plan* plan, int32_t kind, double* total_ms, int32_t* launches);
/* Diagnostic build aid: per-date phase timestamps (s_memtime) of the last DIRECT
 * solve, recorded only when the process runs with CVQ_STAMPS=1 (never in a timed
 * run).  host receives count uint64 values, 32 per date. */
int32_t cvq_plan_debug_stamps(cvq_plan* plan, uint64_t* host, int64_t count);
/* Diagnostic: the SORTED plan's node words in solve order (first `count` of its reachable
   nodes; the LDS byte offsets of their records, cvq_sorted_kernels.h sorted_pack) and, when
   fix != NULL, the sorted positions of the six fixed levels of the last solve's arguments. */
int32_t cvq_plan_debug_nodes(cvq_plan* plan, uint32_t* host, int64_t count, int32_t* fix);
/* Diagnostics: the ends of the solve-order segments (positions the solve's range sums start or
 * end at; inside one the node order is free).  Writes min(cap, *count) of them. */
int32_t cvq_plan_debug_cuts(cvq_plan* plan, int32_t* host, int64_t cap, int32_t* count);
/* Measurement aid (bench.py's FP64 roofline basis): with cvq_plan_count_nodes(plan, 1)
 * the following COMPACT / SORTED / SWEEP solves record how many quadrature nodes each
 * date evaluated (the phase-stamp buffer: slower, never in a timed run);
 * cvq_plan_nodes_evaluated returns the last such solve's total over its dates. */
int32_t cvq_plan_count_nodes(cvq_plan* plan, int32_t enable);
int32_t cvq_plan_nodes_evaluated(cvq_plan* plan, int64_t* total);

/* Per-date inputs = integrations_params_t (calc_integral.py:158):
 *   MSM:       a = forecasts_by_states [T][dim][q], b = forecasts [T][n_combos]
 *   GARCH/UKF: a = sigma forecasts [T][dim],        b = NULL
 * CVQ_MEM_HOST: copied.  CVQ_MEM_DEVICE: read in place by the following launches
 * (no copy); the caller keeps a and b alive and unchanged until the next call. */
int32_t cvq_set_dates(cvq_plan* plan, int64_t T, const double* a, const double* b, int32_t mem);

/* COMPACT: the caller asserts that every date of the current cvq_set_dates batch takes
 * the fast node path -- MSM: b[t] is the outer product of the per-asset rows of a[t]
 * bit for bit (compute_forecast_combinations, msm_estimation.py:392-418, and
 * cvq_msm_tables build it so); GARCH / UKF: every marginal table entry is finite.  The
 * solve then skips its deferred-date (generic path) kernel.  A date that violates the
 * assertion fails the solve with CVQ_ERR_NUMERIC.  cvq_set_dates with CVQ_MEM_HOST sets
 * the hint itself when it can prove it; CVQ_MEM_DEVICE clears it.  No reference
 * counterpart (a launch-count optimisation of the device-resident path). */
int32_t cvq_set_fast_hint(cvq_plan* plan, int32_t on);

/* Diagnostic knob: threads per date (one workgroup each) of the SORTED and SWEEP launches.
 * nt = 0 (the default) leaves the width to the rule -- the widest of 256 / 512 / 1024 whose
 * waves the device holds at once for the current number of dates; 256, 384, 512 or 1024
 * forces that instance.  Every width computes bit-identical results.  Any other value:
 * CVQ_ERR_INVALID.  A non-zero width below what the plan's grid needs (2-D with n > 512
 * needs 1024): CVQ_ERR_UNSUPPORTED.  Any plan accepts the call; only the SORTED and SWEEP
 * strategies' solve and slab launches read the setting. */
int32_t cvq_plan_set_sorted_threads(cvq_plan* plan, int32_t nt);
/* The width the next SORTED / SWEEP launch takes for the plan's current dates: the forced
 * value, else the rule's.  CVQ_ERR_STATE before cvq_set_dates. */
int32_t cvq_plan_get_sorted_threads(cvq_plan* plan, int32_t* nt);

/* Drop-in for ValueAtRiskCalcualtion.compute_integral (calc_var_class.py:179-212)
 * == calc_grids_and_integrals_results (calc_integral.py:8-119):
 * out[t] = integral of the joint copula density over the nested grid of
 * (bounds[t][0], bounds[t][1]] for date t.  bounds [T][2], out [T]. */
int32_t cvq_slab(cvq_plan* plan, const double* bounds, double* out, int32_t mem);

/* No reference counterpart.  Tail moments of the slab (bounds[t][0], bounds[t][1]] on the
 * same nested grid, membership rule (create_grids.py:102-108, Q9/Q10) and node masses as
 * cvq_slab:  m0_out[t] = sum of the member nodes' mass (cvq_slab's value to rounding),
 * m1_out[t] = sum of level x mass, level = w[0] x[i_inner] + sum_c w[c + 1] x[i_c].
 * Any bounds are valid (no v_cap limit, on every strategy); a NaN bound gives 0, 0.
 * Each date is a fixed-order sum over its own row chunks: results are bit-identical
 * between runs and do not depend on the other dates of the batch.  bounds [T][2],
 * m0_out / m1_out [T], all host|device. */
int32_t cvq_slab_moments(cvq_plan* plan, const double* bounds, double* m0_out, double* m1_out,
                         int32_t mem);

/* No reference counterpart.  Expected Shortfall (CVaR) of a solved VaR vector: with
 * (m0, m1) the tail moments of (args->lower, var[t] - args->ptf_mean],
 *   es_out[t] = m1 / m0 + args->ptf_mean,
 * the mean portfolio return given that it falls at or below the VaR, normalised by the
 * mass m0 actually found there (not by obj_var: quirks Q1/Q2 do not always leave the
 * bisection at the obj_var quantile).  NaN where var[t] is NaN (Q3) or m0 == 0.
 * m0_out [T] receives m0 (may be NULL).  Only lower and ptf_mean of args are read.
 * var / es_out / m0_out host|device; CVQ_MEM_DEVICE chains behind a device-mode
 * cvq_solve on the plan's stream without a host synchronisation. */
int32_t cvq_expected_shortfall(cvq_plan* plan, const cvq_solve_args* args, const double* var,
                               double* es_out, double* m0_out, int32_t mem);

/* No reference counterpart.  Per-axis first moments of the slab (bounds[t][0], bounds[t][1]],
 * cvq_slab_moments' membership and node masses:  m0_out[t] = sum of the member nodes' mass
 * (cvq_slab_moments' m0 bit for bit), mx_out[t][c] = sum of x[i_c] x mass for grid axis c.
 * Axis c carries asset c's marginal (input order).  The membership rule weighs axis c with
 *   wa[dim - 1] = w[0],  wa[c] = w[c + 1] for c < dim - 1     (Q10),
 * so sum_c wa[c] mx[c] = cvq_slab_moments' m1 to rounding.  Any bounds are valid (no v_cap
 * limit, on every strategy); a NaN bound gives 0 everywhere.  Fixed-order sums: bit-identical
 * between runs and independent of the other dates of the batch; the plan's solve state is
 * untouched.  bounds [T][2], m0_out [T], mx_out [T][dim], all host|device. */
int32_t cvq_slab_axis_moments(cvq_plan* plan, const double* bounds, double* m0_out, double* mx_out,
                              int32_t mem);

/* No reference counterpart.  Euler allocation of the Expected Shortfall of a solved VaR vector:
 * with (m0, mx) the axis moments of (args->lower, var[t] - args->ptf_mean],
 *   contrib_out[t][c] = wa[c] mx[c] / m0  =  wa[c] E[x_c | portfolio <= VaR],
 * which sum over c to cvq_expected_shortfall's es_out[t] - args->ptf_mean (ptf_mean is one
 * scalar of the portfolio and is not allocated).  The whole row is NaN where var[t] is NaN
 * (Q3) or m0 == 0.  m0_out [T] receives m0 (may be NULL).  Only lower and ptf_mean of args are
 * read.  var / contrib_out [T][dim] / m0_out host|device; CVQ_MEM_DEVICE chains behind
 * device-mode cvq_solve / cvq_expected_shortfall on the plan's stream without a host
 * synchronisation. */
int32_t cvq_es_contributions(cvq_plan* plan, const cvq_solve_args* args, const double* var,
                             double* contrib_out, double* m0_out, int32_t mem);

/* No reference counterpart.  Exact quantiles of the nested-grid measure at up to CVQ_MAX_LEVELS
 * levels per date: the true VaR that cvq_solve's reproduced quirk Q1 misses wherever the
 * quantile lies in (-2, 0], and the Expected Shortfall below it.  With
 *   F(v) = cvq_slab_moments' m0 of (args->lower, v],
 *   K = ceil(log2((max_var - min_var) / tolerance))   (23 by default; > 62: CVQ_ERR_UNSUPPORTED),
 * per date t and level alpha = levels[l]:
 *   not (F(min_var) < alpha <= F(max_var)):  var = es = NaN, m0 = F(max_var);
 *   else K steps from (lo, hi) = (min_var, max_var): mid = (lo + hi) / 2, lo = mid if
 *   F(mid) < alpha else hi = mid (the reference's own update rule, without Q1-Q4);
 *   var = (lo + hi) / 2 + ptf_mean; es, m0 = cvq_expected_shortfall's of that var.
 * F is not normalised (quirks Q5/Q6 are the measure's): any finite alpha > 0 is a level.
 * The node evaluation is shared: the marginal tables are built once per call, the opening
 * pass (min_var, max_var and the first three steps' seven mids, all level-independent) serves
 * every level, and each later pass takes three bisection steps (seven cut points) in one sweep
 * over the nodes of its bracket.  Dates are independent (no Q2/Q4 coupling); each date is a
 * fixed-order sum: results are bit-identical between runs, across batches and across the
 * number of levels asked for.  Runs on every strategy with no v_cap limit, on scratch of its
 * own: the plan's solve state is untouched.  Reads only min_var, max_var, lower, tolerance and
 * ptf_mean of args.  levels: host [n_levels] whatever `mem` says; var_out / es_out / m0_out
 * [T][n_levels] host|device, the last two may be NULL.  CVQ_ERR_INVALID: NULL argument,
 * n_levels outside 1..CVQ_MAX_LEVELS, a level <= 0 or NaN, max_var <= min_var. */
#define CVQ_MAX_LEVELS 8
int32_t cvq_quantiles(cvq_plan* plan, const cvq_solve_args* args, const double* levels, int32_t n_levels,
                      double* var_out, double* es_out, double* m0_out, int32_t mem);

/* No reference counterpart.  The predictive distribution of the portfolio return: per date, the
 * mass and first moment of the nested-grid measure in up to CVQ_MAX_BINS level bins in one
 * sweep -- the value-to-level direction that cvq_quantiles lacks (a PIT is two bins, a CDF at K
 * thresholds K + 1).  Bin b of date t is the slab (e[b], e[b+1]] under cvq_slab_moments'
 * membership rule and node masses:
 *   mass_out[t][b] = that slab's m0,  m1_out[t][b] = its m1  (cvq_slab_moments' values to
 *   rounding: the summation order differs).
 * per_date == 0: edges is host [n_bins + 1] whatever `mem` says and serves every date;
 * per_date == 1: edges is [T][n_bins + 1], host|device.  mass_out / m1_out [T][n_bins]
 * host|device; m1_out may be NULL.
 * Each bin stands alone: edges need not ascend; a bin with a NaN edge or with e[b+1] <= e[b] is
 * exactly (0, 0); +-inf edges are valid (every node, or none, lies at or below them).  The measure
 * is not normalised (quirks Q5/Q6): the total mass is the bin (lower, +inf].
 * A bin's two numbers depend on its own two edges and its date's inputs alone -- not on the other
 * bins of the call, their number or order, nor on the other dates -- and are bit-identical between
 * runs (fixed-order sums, no atomics).  The marginal tables are built once per call and the row
 * setup once per row; with an ascending ladder every quadrature node is evaluated once.
 * Runs on every strategy with no v_cap limit, on lazily sized scratch of its own: the plan's
 * solve state is untouched.  CVQ_MEM_DEVICE is stream-ordered without a host synchronisation.
 * Timed under kind 5 (tail moments).
 *   CVQ_ERR_INVALID: NULL plan, edges or mass_out; n_bins outside 1..CVQ_MAX_BINS; per_date not
 *     0 or 1.
 *   CVQ_ERR_STATE: called before cvq_set_dates.
 *   CVQ_ERR_UNSUPPORTED: a grid outside cvq_quantiles' limits (n <= 1024, q <= 8, dim 2 or 3,
 *     Plackett 2-D only).
 * All of them are found on the host before any device work. */
#define CVQ_MAX_BINS 64
int32_t cvq_distribution(cvq_plan* plan, const double* edges, int32_t n_bins, int32_t per_date,
                         double* mass_out, double* m1_out, int32_t mem);

/* No reference counterpart.  Conditional quantiles of the nested-grid measure: CoVaR / CoES of
 * the portfolio given an event on one grid axis (Adrian-Brunnermeier; the "<=" form of
 * Girardi-Ergun).  Axis c in [0, dim) carries asset c's marginal (input order, as in
 * cvq_slab_axis_moments).  Per date t the event is a predicate on grid nodes,
 *   E_t = { node : x[i_axis] > cond[t][0] and x[i_axis] <= cond[t][1] }   (plain FP64 compares;
 *   +-inf bounds are allowed; a NaN bound or cond[t][1] <= cond[t][0] is the empty event),
 * and with cvq_quantiles' membership and node masses
 *   F_E(v) = mass of the nodes of (args->lower, v] that lie in E_t,   p_E[t] = F_E(+inf).
 * The measure is not normalised and the event sits on grid nodes, so p_E is not the nominal
 * stress probability: it is returned (pe_out) and it is the normaliser.  Per level
 * alpha = levels[l] the target is alpha * p_E[t] (one FP64 product), and with
 * K = ceil(log2((max_var - min_var) / tolerance)):
 *   not (F_E(min_var) < alpha p_E <= F_E(max_var)):  covar = coes = NaN, m0 = F_E(max_var)
 *     (this covers p_E == 0);
 *   else K steps from (lo, hi) = (min_var, max_var): mid = (lo + hi) / 2, lo = mid if
 *   F_E(mid) < alpha p_E else hi = mid (cvq_quantiles' rule);
 *   covar = (lo + hi) / 2 + ptf_mean;  m0 = F_E(covar - ptf_mean);
 *   coes = M1_E / m0 + ptf_mean with M1_E the level-weighted sum over the same nodes (NaN when
 *   m0 == 0).
 * Dates are independent (no Q2/Q4 coupling); each date is a fixed-order sum: results are
 * bit-identical between runs, across batches and across the number of levels asked for.  Runs
 * on every strategy with no v_cap limit, on scratch of its own: the plan's solve state is
 * untouched.  Reads only min_var, max_var, lower, tolerance and ptf_mean of args.  levels: host
 * [n_levels] whatever `mem` says; cond [T][2], covar_out / coes_out / m0_out [T][n_levels] and
 * pe_out [T] host|device, the last three may be NULL.  CVQ_MEM_DEVICE is stream-ordered without
 * a host synchronisation.  Timed under kind 6.  CVQ_ERR_INVALID: NULL argument, axis outside
 * [0, dim), n_levels outside 1..CVQ_MAX_LEVELS, a level <= 0 or NaN, max_var <= min_var. */
int32_t cvq_conditional_quantiles(cvq_plan* plan, const cvq_solve_args* args, int32_t axis, const double* cond,
                                  const double* levels, int32_t n_levels, double* covar_out, double* coes_out,
                                  double* m0_out, double* pe_out, int32_t mem);

/* No reference counterpart.  cvq_quantiles for a batch of portfolio weights on one plan: the
 * exact quantile, Expected Shortfall and mass of the same nested-grid measure for
 * n_portfolios weight vectors x n_levels levels per date.  Nothing of the measure depends on the
 * weights (only the membership of a node and its level do), so the marginal tables are built once
 * per call and one launch sequence serves every portfolio.  For portfolio p,
 *   var / es / m0 [t][p][:] is what cvq_quantiles returns on a plan that differs only in
 *   cvq_static.weights = weights[p] and args->ptf_mean = ptf_mean[p],
 * bit for bit, cvq_plan_create's reciprocal rule included (weights[p][0] a power of two with a
 * normal reciprocal: multiply by it; else divide).  weights follow cvq_static.weights' convention
 * (Q10: weights[p][0] scales the inner, last-integrated axis); weights[p][0] <= 0 is
 * CVQ_ERR_UNSUPPORTED as in cvq_plan_create, the other weights may be zero or negative.
 * A portfolio's result does not depend on the other portfolios of the call, their number or order,
 * the number of levels or the other dates, and is bit-identical between runs (fixed-order sums;
 * no atomics).  K, the bracket rule, the NaN convention outside the bracket and everything else
 * are cvq_quantiles': runs on every strategy with no v_cap limit, on lazily sized scratch of its
 * own (cvq_portfolio_scratch; a failed allocation is CVQ_ERR_OOM); the plan's solve state is
 * untouched.  Reads only min_var, max_var, lower and tolerance of args (args->ptf_mean is not
 * read).  weights host [n_portfolios][dim], ptf_mean host [n_portfolios], levels host [n_levels]
 * whatever `mem` says; var_out / es_out / m0_out [T][n_portfolios][n_levels] host|device, the
 * last two may be NULL.  CVQ_MEM_DEVICE is stream-ordered without a host synchronisation.  Timed
 * under kind 6.  CVQ_ERR_INVALID (before any device work): NULL argument, n_portfolios outside
 * 1..CVQ_MAX_PORTFOLIOS, n_levels outside 1..CVQ_MAX_LEVELS, a level <= 0 or NaN,
 * max_var <= min_var, a non-finite weight or ptf_mean.  K > 62: CVQ_ERR_UNSUPPORTED. */
#define CVQ_MAX_PORTFOLIOS 64
int32_t cvq_portfolio_quantiles(cvq_plan* plan, const cvq_solve_args* args, const double* weights,
                                const double* ptf_mean, int32_t n_portfolios, const double* levels,
                                int32_t n_levels, double* var_out, double* es_out, double* m0_out, int32_t mem);

/* Bytes of device scratch one cvq_portfolio_quantiles call of this shape takes on the plan's
 * current batch (a caller splitting a long candidate list sizes its calls with it). */
int32_t cvq_portfolio_scratch(const cvq_plan* plan, int32_t n_portfolios, int32_t n_levels, int64_t* bytes);

/* No reference counterpart.  cvq_quantiles under per-date copula parameters, weights and means on
 * one plan: the exact quantile, Expected Shortfall and mass of a rolling backtest whose dependence
 * is re-estimated (or follows a DCC-style path) and whose weights drift from date to date.
 *   var / es / m0 [t][:] is what cvq_quantiles returns, bit for bit, on a plan that differs from
 *   this one only in cvq_static.copula_params = copula_params_t[t], cvq_static.weights =
 *   weights_t[t] and args->ptf_mean = ptf_mean_t[t], and that is given date t alone,
 * cvq_plan_create's reciprocal rule included (weights_t[t][0] a power of two with a normal
 * reciprocal: multiply by it; else divide).  copula_params_t follows cvq_static.copula_params'
 * packing, [T][n_copula_params] with the plan's n_copula_params; weights_t [T][dim] follows
 * cvq_static.weights' convention (Q10); ptf_mean_t [T].  A NULL array means the plan's own value
 * (args->ptf_mean for the means) on every date; with all three NULL the call is cvq_quantiles, bit
 * for bit, and args->ptf_mean is read only when ptf_mean_t is NULL.  Fixed per plan: the copula
 * kind (with the Gumbel / Joe survival flag) and the Student nu (the t quantile tables and the integer-power
 * paths hang on nu; copula_params_t[t][0] must repeat the plan's).
 * A date's result depends on its own record and inputs alone: not on the other dates, their
 * order or the number of levels, and it is bit-identical between runs (fixed-order sums; no
 * atomics).  K, the bracket rule, the NaN convention outside the bracket and everything else are
 * cvq_quantiles': runs on every strategy with no v_cap limit, on lazily sized scratch of its own
 * (cvq_dynamic_scratch; a failed allocation is CVQ_ERR_OOM); the plan's solve state is untouched.
 * The three per-date arrays and levels are host memory whatever `mem` says and need not outlive
 * the call; var_out / es_out / m0_out [T][n_levels] host|device, the last two may be NULL.
 * CVQ_MEM_DEVICE is stream-ordered without a host synchronisation.  Timed under kind 6.
 * Everything is validated before any device work; a failure on a per-date value names the first
 * offending date ("at date <t>") in cvq_last_error() and leaves the outputs unwritten:
 *   CVQ_ERR_INVALID: NULL plan, args, levels or var_out; n_levels outside 1..CVQ_MAX_LEVELS; a
 *     level <= 0 or NaN; max_var <= min_var; a non-finite parameter, weight or mean; Gumbel
 *     or Joe theta < 1; Frank theta = 0; Student nu <= 0; Gaussian / Student: a correlation with |rho| >= 1, or a matrix
 *     whose cofactor determinant is not > 0 -- stricter than cvq_plan_create, which takes any
 *     correlation values without this check;
 *   CVQ_ERR_UNSUPPORTED: Gumbel or Joe theta > 16; Frank theta < 0 or > 32; weights_t[t][0] <= 0; a Student
 *     copula_params_t[t][0] other than the plan's nu; K > 62;
 *   CVQ_ERR_STATE: called before cvq_set_dates. */
int32_t cvq_dynamic_quantiles(cvq_plan* plan, const cvq_solve_args* args, const double* copula_params_t,
                              const double* weights_t, const double* ptf_mean_t, const double* levels,
                              int32_t n_levels, double* var_out, double* es_out, double* m0_out, int32_t mem);

/* Bytes of device scratch one cvq_dynamic_quantiles call of n_levels levels takes on the plan's
 * current batch (the date records included). */
int32_t cvq_dynamic_scratch(const cvq_plan* plan, int32_t n_levels, int64_t* bytes);

/* No reference counterpart.  cvq_distribution under per-date copula parameters and weights on one
 * plan: the predictive distribution of the forecast that cvq_dynamic_quantiles produces (a rolling
 * refit on a drifting book), so that forecast can be backtested (PIT, coverage, scoring).
 *   mass_out[t][:] and m1_out[t][:] are what cvq_distribution returns, bit for bit, on a plan that
 *   differs from this one only in cvq_static.copula_params = copula_params_t[t] and
 *   cvq_static.weights = weights_t[t], given date t alone or date t in any batch,
 * cvq_plan_create's reciprocal rule for weights[0] included.  copula_params_t
 * [T][n_copula_params] and weights_t [T][dim] follow cvq_dynamic_quantiles' conventions: host
 * memory whatever `mem` says, not needed after the call; a NULL array means the plan's own value
 * on every date, and with both NULL the call is cvq_distribution, bit for bit.  Fixed per plan:
 * the copula kind (with the survival / family code) and the Student nu.
 * edges, n_bins, per_date, mass_out, m1_out and mem are cvq_distribution's: edges host
 * [n_bins + 1] serving every date (per_date == 0), or [T][n_bins + 1] host|device (per_date == 1).
 * Edges are centred levels: there is no mean argument, a caller with a per-date mean subtracts it
 * from each date's ladder.  Every property of cvq_distribution carries over: each bin stands
 * alone, a NaN, repeated or descending pair of edges is exactly (0, 0), +-inf edges are valid, a
 * bin depends on its own two edges and its date's inputs and record alone, results are
 * bit-identical between runs (fixed-order sums, no atomics).  Runs on every strategy with no
 * v_cap limit, on lazily sized scratch of its own; the plan's solve state is untouched.
 * CVQ_MEM_DEVICE is stream-ordered without a host synchronisation.  Timed under kind 5.
 * cvq_distribution's argument checks come first, in its order and with its codes; then the
 * per-date values by cvq_dynamic_quantiles' rules, codes and "at date <t>" wording (one helper
 * serves both entry points).  All of it happens on the host before any device work; a failure
 * leaves the outputs unwritten. */
int32_t cvq_dynamic_distribution(cvq_plan* plan, const double* copula_params_t, const double* weights_t,
                                 const double* edges, int32_t n_bins, int32_t per_date,
                                 double* mass_out, double* m1_out, int32_t mem);

/* Drop-in for ValueAtRiskCalcualtion.calc_var (calc_var_class.py:95-177 +
 * bisection_algorithm :250-309), quirks Q1-Q4 reproduced.  var_out [T];
 * iters_out = bisection iterations the reference would run (may be NULL). */
int32_t cvq_solve(cvq_plan* plan, const cvq_solve_args* args, double* var_out,
                  int32_t* iters_out, int32_t mem);

/* Status of the plan's last device-mode solve or finalize (cvq_solve with
 * CVQ_MEM_DEVICE and iters_out == NULL, cvq_solve_finalize): synchronises the
 * plan's stream and returns CVQ_ERR_NUMERIC if a date did not converge within the
 * bisection budget K (only possible for non-dyadic guesses, whose K carries a
 * 2-iteration margin); iters_out = bisection iterations the reference runs (Q2/Q4).
 * Device mode never synchronises by itself: call this to check.  cvq_solve with a
 * non-NULL iters_out checks and widens K itself. */
int32_t cvq_solve_status(cvq_plan* plan, int32_t* iters_out);

/* Sharded solve, for one process per GPU (date blocks).
 * Phase 1 (local):  per-date bisection snapshots + a 16-byte header
 *   d_header: 16 bytes device, d_snaps: [T_local][cvq_snap_stride(args)] device.
 * Exchange: the caller all-gathers headers and snaps (RCCL) -- or, packed, one buffer.
 * Phase 2: finalise every date from the gathered blocks; d_var [T_total] device. */
int32_t cvq_snap_stride(const cvq_solve_args* args, int32_t* stride);
int32_t cvq_solve_local(cvq_plan* plan, const cvq_solve_args* args, void* d_header, double* d_snaps);
int32_t cvq_solve_finalize(cvq_plan* plan, const cvq_solve_args* args, const void* d_headers,
                           int32_t n_ranks, const double* d_snaps, int64_t dates_per_rank,
                           int64_t T_total, double* d_var);
/* Packed variant for ONE all-gather per solve: each rank's block is its snapshots
 * [dates_per_rank][stride] followed by its 16-byte header at header_offset (doubles;
 * cvq_solve_local's d_snaps = block, d_header = block + header_offset), block length
 * len doubles (even, so blocks stay 16-byte aligned).  d_blocks = [n_ranks][len],
 * 16-byte aligned. */
int32_t cvq_packed_block_len(const cvq_solve_args* args, int64_t dates_per_rank, int64_t* len,
                             int64_t* header_offset);
int32_t cvq_solve_finalize_packed(cvq_plan* plan, const cvq_solve_args* args, const double* d_blocks,
                                  int32_t n_ranks, int64_t dates_per_rank, int64_t T_total,
                                  double* d_var);

/* ------------------------------------------------ per-date forecast stage */
/* MSM forecasts_array (msm_estimation.py:140-202 -> calc_marginals.py:33-38 ->
 * calc_prob.py:8-69): filtered state probabilities at the end of each rolling
 * window.  returns_c: centred returns [n_in + T - 1] of ONE asset; out [T][2**k]. */
int32_t cvq_msm_filter(int32_t device, int32_t k, double m0, double sigma, double b, double gamma,
                       const double* returns_c, int64_t n_in, int64_t T, double* out, int32_t mem);
/* Device-resident MSM forecast stage for all assets in one pass (no host round trip):
 * forecasts_array (msm_estimation.py:140-202 -> calc_prob.py:8-69, filtered
 * probabilities at each window's end, Q12) + sum_forecast_by_state (:205-248, Q14)
 * + compute_forecast_combinations (:392-418, Q7), i.e. integrations_params_t ready for
 * cvq_set_dates(..., CVQ_MEM_DEVICE).  Stream-ordered on `stream` (NULL = null stream),
 * no synchronisation.  params (host) [dim][4] = (m0, sigma, b, gamma); state_map (host)
 * [dim][2**k] = index of state s's 1e-6-rounded vol among the asset's q unique vols;
 * returns_c (device) [dim][n_in + T - 1] centred returns; scratch (device) of
 * cvq_msm_tables_scratch doubles; fbs_out (device) [T][dim][q]; pi_out (device)
 * [T][q**dim].  cvq_msm_tables_status synchronises and reports a zero Bayes
 * normaliser (calc_prob.py:64-65) of the last cvq_msm_tables run on that scratch as
 * CVQ_ERR_NUMERIC. */
int32_t cvq_msm_tables_scratch(int32_t dim, int32_t k, int64_t n_in, int64_t T, int64_t* doubles);
int32_t cvq_msm_tables(int32_t device, void* stream, int32_t dim, int32_t k, const double* params,
                       const int32_t* state_map, int32_t q, const double* returns_c, int64_t n_in,
                       int64_t T, double* scratch, double* fbs_out, double* pi_out);
int32_t cvq_msm_tables_status(double* scratch, int32_t dim, int32_t k, int64_t n_in, int64_t T, void* stream);
/* In-sample MSM marginals and densities of ONE asset's return series (calc_marginals.py:7-30,
 * used by MsmEstimation.calculate_marginals_and_densities_in_sample, msm_estimation.py:90-104):
 * marg_out / dens_out [N - 1] = sum over states of the filtered probabilities of step i
 * (calc_prob.py:51-69) times norm.cdf / norm.pdf of return i - 1 (calc_prob.py:110-132).
 * CVQ_ERR_NUMERIC on a zero Bayes normaliser (calc_prob.py:64-65). */
int32_t cvq_msm_marginals(int32_t device, int32_t k, double m0, double sigma, double b, double gamma,
                          const double* returns, int64_t N, double* marg_out, double* dens_out, int32_t mem);
/* GARCH(1,1) compute_forecast (garch_estimation.py:190-231 -> garch/forecast.py:5-19).
 * out [T] = sigma forecast per window. */
int32_t cvq_garch_forecast(int32_t device, double omega, double alpha, double beta,
                           const double* returns_c, int64_t n_in, int64_t T, double* out, int32_t mem);
/* GARCH(p, q) compute_forecast, 1 <= p, q <= 4 (garch/forecast.py:5-19):
 * params (host) [1 + p + q] = (omega, alpha_1..p, beta_1..q); out [T]. */
int32_t cvq_garch_forecast_pq(int32_t device, int32_t p, int32_t q, const double* params, const double* returns_c,
                              int64_t n_in, int64_t T, double* out, int32_t mem);
/* UKF compute_forecast (mean_reverting_estimation.py:192-232 -> forecast.py:5-12 ->
 * estimate.py:230-281); Q19 semantics.  out [T]. */
int32_t cvq_ukf_forecast(int32_t device, double a, double l, double q,
                         const double* returns_c, int64_t n_in, int64_t T, double* out, int32_t mem);

/* Device-resident GARCH / UKF forecast stage for all assets (no host round trip):
 * Garch/MeanRevertingEstimation.integration_params_retrieval's sigma forecasts
 * (garch_estimation.py:133-145 -> :190-231 -> garch/forecast.py:5-19;
 * mean_reverting_estimation.py:135-147 -> :192-232 -> kalman_mean_reverting/forecast.py:5-12),
 * written as integrations_params_t [T][dim] for cvq_set_dates(..., CVQ_MEM_DEVICE).
 * Stream-ordered on `stream`, no synchronisation.  model CVQ_GARCH: orders (host)
 * [dim][2] = (p, q) per asset, 1 <= p, q <= 4 (NULL = all (1, 1)), params (host) the
 * assets' (omega, alpha_1..p, beta_1..q) rows back to back; CVQ_UKF: params (host)
 * [dim][3] = (a, l, q), orders ignored.  returns_c (device) [dim][n_in + T - 1];
 * d_err (device) one int32; sig_out (device) [T][dim].  cvq_sigma_tables_status
 * synchronises and reports a UKF failure (Z < 1e-10 / NaN, estimate.py:219-220,
 * :270-271; NaN sigma) as CVQ_ERR_NUMERIC. */
int32_t cvq_sigma_tables(int32_t device, void* stream, int32_t model, int32_t dim, const int32_t* orders,
                         const double* params, const double* returns_c, int64_t n_in, int64_t T,
                         int32_t* d_err, double* sig_out);
int32_t cvq_sigma_tables_status(const int32_t* d_err, void* stream);

/* --------------------------------------- batched in-sample likelihoods */
/* One log-likelihood per parameter candidate over the same return series
 * (optimiser inner loops).  params: MSM [B][4] = (m0, sigma, b, gamma);
 * GARCH [B][3] = (omega, alpha, beta); UKF [B][3] = (a, l, q).  out [B].
 * MSM: calc_prob.py:36-47; GARCH: garch/estimation.py:91-125; UKF: estimate.py:276. */
int32_t cvq_msm_loglik(int32_t device, int32_t k, const double* params, int64_t B,
                       const double* returns, int64_t N, double* out, int32_t mem);
int32_t cvq_garch_loglik(int32_t device, const double* params, int64_t B,
                         const double* returns, int64_t N, double* out, int32_t mem);
int32_t cvq_ukf_loglik(int32_t device, const double* params, int64_t B,
                       const double* returns, int64_t N, double* out, int32_t mem);
/* GARCH(p, q), 1 <= p, q <= 4, for the (p, q) search of GarchOptimizer.optimize
 * (garch/opti.py:89-137): params [B][1 + p + q] = (omega, alpha_1..p, beta_1..q);
 * garch/estimation.py:91-125 incl. the max(p, q) chopped prefix. */
/* UKF E-step of VolOptimizer (kalman_mean_reverting/optimize.py:28-32 ->
 * estimate.py:7-51, 230-281): per candidate (a, l, q) [B][3] the log-likelihood
 * ll_out [B] (-1e10 on the Z / NaN failure) and the filtered state path
 * states_out [N][B] (time-major; NaN column on failure).  returns: one series [N]
 * shared by all candidates (per_candidate = 0) or one per candidate [B][N]
 * (per_candidate = 1: several assets' EM chains in one launch). */
int32_t cvq_ukf_filter(int32_t device, const double* params, int64_t B, const double* returns, int32_t per_candidate,
                       int64_t N, double* ll_out, double* states_out, int32_t mem);
int32_t cvq_garch_loglik_pq(int32_t device, int32_t p, int32_t q, const double* params, int64_t B,
                            const double* returns, int64_t N, double* out, int32_t mem);

/* ------------------------------------- score-driven time-varying copula */
/* No reference counterpart.  The observation-driven (GAS; Creal, Koopman and Lucas 2013) dependence
 * recursion that produces the per-date copula parameters cvq_dynamic_quantiles and
 * cvq_dynamic_distribution take (DESIGN.md §4 "Score-driven copula").  For rows u_t in (0,1)^dim,
 * t = 0 .. N-1, and a candidate (omega, alpha, beta):
 *     f_0 = omega / (1 - beta),   theta_t = link(f_t),   l_t = log c(u_t; theta_t),
 *     s_t = d l_t / d f (analytic, unit scaling),   f_{t+1} = clamp(omega + beta f_t + alpha s_t, -40, 40).
 * Links, sigma(f) = 1 / (1 + e^-f), inside the ranges the plans accept:
 *     Gaussian, Student (nu fixed)   rho   = 0.99 (2 sigma(f) - 1)                  dim 2
 *     Plackett                       theta = 0.1 * 10^(4 sigma(f))                  dim 2
 *     Gumbel, Joe and rotations      theta = 1.0001 + (16 - 1.0001) sigma(f)        dim 2, 3
 *     Frank                          theta = 1e-3 + (32 - 1e-3) sigma(f)            dim 2, 3
 * copula: the CVQ_* kinds above.  The rotation follows cvq_static: CVQ_GUMBEL_SURVIVAL and
 * CVQ_JOE_SURVIVAL are kinds of their own; `survival` != 0 with CVQ_GUMBEL / CVQ_JOE selects the same
 * rotation (it is ignored with the two _SURVIVAL codes and CVQ_ERR_INVALID with any other kind).
 * nu: the Student degrees of freedom (read for CVQ_STUDENT only).
 * cvq_gas_loglik: ll_out[b] = sum_t l_t of candidate row b, one launch for all B rows; a row's
 *   result does not depend on B or on the other rows (fixed-order sum, no atomics).
 * cvq_gas_path: theta_out[0 .. N] (theta_t depends on the rows before t only; theta_N is the
 *   one-step-ahead forecast) and, unless NULL, logc_out[t] = l_t.
 * A candidate with |beta| >= 1 or a non-finite parameter, or whose f, s or l stops being finite at
 * some row, is not an error: its ll is NaN; its logc is NaN from that row and its theta from the
 * next one on.  params is host memory; u [N][dim] and the outputs are host|device per `mem`
 * (the call returns after the device has finished in both modes).
 * Validated on the host before any device work, outputs unwritten on failure:
 *   CVQ_ERR_INVALID: a NULL pointer (logc_out may be NULL); B < 1 or N < 1; dim outside 2..3; Student
 *     nu <= 0 or not finite; with host u, a value not strictly inside (0, 1) or NaN -- the message
 *     names the first such row ("at row <i>");
 *   CVQ_ERR_UNSUPPORTED: Gaussian, Student or Plackett with dim 3 (a correlation-matrix recursion is
 *     not built); an unknown kind. */
int32_t cvq_gas_loglik(int32_t device, int32_t copula, int32_t survival, int32_t dim, double nu,
                       const double* params /*[B][3] = (omega, alpha, beta)*/, int64_t B,
                       const double* u /*[N][dim]*/, int64_t N, double* ll_out /*[B]*/, int32_t mem);
int32_t cvq_gas_path(int32_t device, int32_t copula, int32_t survival, int32_t dim, double nu,
                     const double* params /*[3]*/, const double* u, int64_t N,
                     double* theta_out /*[N+1]*/, double* logc_out /*[N] or NULL*/, int32_t mem);

/* Special functions on the device (known-answer tests against scipy):
 * fn 0 = t.ppf(u, nu) (student.py:102), 1 = norm.ppf (gaussian.py:44),
 * 2 = erf (utils/utils.py:20), 3 = t.ppf as the solve kernels' tables evaluate it for
 * nu = 6 (integer-nu root, nu must be 6).
 *
 * fn 4..16: the device-only node arithmetic of csrc/cvq_special.h, one code per helper
 * (known-answer tests against a 50-digit reference, tests/test_node_kat_gpu.py).  `nu`
 * carries the helper's one parameter:
 *    4 log_node(x)          5 log_node_fast(x)     6 exp_node(x)       7 exp_node7(x)
 *    8 exp2_node7(x)        9 fast_rcp(x)         10 root_nu<6>(x)     (nu must be 6)
 *   11 pow_node(x, m, ex)      nu = ex <= 0, m = the plan's node_m rule on -2 ex (limit 128)
 *   12 pow_gen(x, ex)          nu = ex
 *   13 pow_half_neg(x, m, ex)  nu = ex <= 0, m = the plan's uni_m rule on -2 ex (limit 16)
 *   14 pow_half_pos(x, m, ex)  nu = ex >= 0, m = the same rule on 2 ex
 *   15 pow_half_pos_c<7>(x)
 *   16 stdtrit_tab_bf(x)       nu = nu; CVQ_ERR_UNSUPPORTED where the plan builds no direct
 *                              tables for this nu (as fn 3)
 * Slab tier only (they live in kernel headers that k_special's translation unit cannot
 * include without the solve kernels; tests/test_node_slabs_gpu.py holds them through the
 * slab sums): pow_node_t (cvq_direct_kernels.h: DIRECT and COMPACT slabs, which both run
 * k_direct) and pow_fast incl. SORTED's exp2_node7(ex log2(e) log_node_fast(b)) power
 * (cvq_sorted_kernels.h: SORTED and SWEEP slabs).  Not reached by either tier:
 * COMPACT's own copy of that fast power (cvq_compact_kernels.h), which runs in its solve
 * only.  It, and every strategy's solve path with it (level loops, block tails, generic
 * kernels), is held to the same longdouble reference by obj_var probes of cvq_solve_local
 * (tests/test_solve_probes_gpu.py; DESIGN.md §5 "Solve-path probes"). */
int32_t cvq_special(int32_t device, int32_t fn, double nu, const double* x, int64_t n,
                    double* out, int32_t mem);

#ifdef __cplusplus
}
#endif
#endif /* CVQ_H */
