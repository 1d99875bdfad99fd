// cvq_conditional_kernels.h -- conditional quantiles (cvq_conditional_quantiles): CoVaR / CoES of
// the portfolio given an event on one grid axis.  No reference counterpart.  Per date t the event
// is a predicate on grid nodes, E_t = { node : s_lo[t] < x[i_c] <= s_hi[t] } for the conditioning
// axis c, and the measure is cvq_quantiles' F restricted to it:
//   F_E(v) = mass of (lower, v] within E_t,   p_E = F_E(+inf),   target = alpha p_E.
// Membership, node values and Delta weights are the slab paths' own.
//
// k_cond_pass is k_quant_pass (same mapping, same partial layout, same fixed-order reduction)
// with the event applied before any range is formed:
//   outer axis (c < DIM - 1): a row predicate on x[i0] / x[i1]; a row outside the event takes
//     the empty range (ka = n, kb = 0), so a chunk without an event row skips its node loop and
//     writes zero partials;
//   inner axis (c == DIM - 1): the event is the column range (ea, eb], two count_le searches of
//     the LDS grid copy per lane with wave-uniform operands (the bounds are per date); every
//     row's (ka, kb[i]] is clamped to it before kbmax, jlo / jhi and the SKEW trip count.
// A NaN bound compares false with every node: the empty event.
//
// Schedule: cvq_quantiles' own, 9 node passes and 19 launches at K = 23: tables -> opening pass
// (C = 10: k_quant_pass' nine cuts from `lower`, then +inf, whose sum is p_E; level-independent)
// -> k_cond_update (p_E, bracket test on alpha p_E, first three decisions) -> ceil((K - 3) / 3)
// passes of C = 7 with their updates -> closing pass (C = 2) -> k_cond_finish.  The tenth cut
// makes the opening pass sweep an event row to its end instead of to max_var; a pass of its own
// for p_E swept the same nodes a second time (measured slower on every shape).
#pragma once
// cvq_quantile_kernels.h defines its two plain (non-template) kernels in every unit that
// includes it.  This unit takes its helpers (quant_cuts, quant_sum) and constants only, so its
// copies of those two kernels get names of their own and cvq_quantile.hip keeps the originals.
#define k_quant_update k_quant_update_conditional_unit
#define k_quant_finish k_quant_finish_conditional_unit
#include "cvq_quantile_kernels.h"
#undef k_quant_update
#undef k_quant_finish

namespace cvq {

constexpr int kCondState = kQuantState + 1;    // + p_E of the date
constexpr int kCondOpenCuts = kQuantOpenCuts + 1;   // the opening pass: k_quant_pass' nine cuts, then +inf for p_E

// The opening pass's lower edge and cuts (the same for every date and level).
struct CondUniform {
    double a;
    double c[kCondOpenCuts];
};

__device__ __forceinline__ bool cond_member(double xv, double s_lo, double s_hi) { return xv > s_lo && xv <= s_hi; }

// st == nullptr: the opening pass, U's edge and first C cuts for every date (one level).
template <int COP, bool MSM, int DIM, int QT, int C>
__global__ __launch_bounds__(kMomNT) void k_cond_pass(StaticDev S, const double* __restrict__ tA,
                                                      const double* __restrict__ tB, const double* __restrict__ pi,
                                                      const double* __restrict__ st, const double* __restrict__ cuts,
                                                      CondUniform U, int axis, const double* __restrict__ cond,
                                                      double* __restrict__ part) {
    constexpr int CS = moments_colsplit(DIM);
    constexpr bool SKEW = C != kCondOpenCuts;    // narrow passes: each lane walks its own columns
    __shared__ double sx[kMomMaxN];
    __shared__ double red[kMomWaves][2 * C];
    const int n = S.n, q = QT;
    for (int j = threadIdx.x; j < n; j += kMomNT) sx[j] = S.x[j];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long t = blockIdx.x;
    const size_t tl = (size_t)t * gridDim.z + blockIdx.z;
    const int r = (int)blockIdx.y * moments_chunk_rows(DIM) + (wave / CS) * 64 + lane;
    const bool live = r < S.nrows;
    double a, c[C];
    if (st) {
        a = st[tl * kCondState];
#pragma unroll
        for (int i = 0; i < C; ++i) c[i] = cuts[tl * kQuantCuts + i];
    } else {
        a = U.a;
#pragma unroll
        for (int i = 0; i < C; ++i) c[i] = U.c[i < kCondOpenCuts ? i : 0];
    }
    const double s_lo = cond[2 * t], s_hi = cond[2 * t + 1];     // wave-uniform

    const double* At = tA + t * S.dim * n;
    const double* Bt = tB + t * S.dim * n;
    const double* pit = pi + t * S.Q;
    const int inner = DIM - 1;
    const double* Ac = At + inner * n;           // inner-axis tables (wave-uniform reads)
    const double* Bc = Bt + inner * n;
    const double* Fc = S.F + (size_t)inner * q * n;

    const int rr_ = live ? r : 0;
    const int i0 = (DIM == 2) ? rr_ : rr_ / n;
    const int i1 = (DIM == 2) ? 0 : rr_ % n;

    // ---- the event: a row predicate (outer axis) or the column range (ea, eb] (inner axis)
    bool in_event = live;
    int ea = 0, eb = n - 1;
    if (axis == inner) {
        if (s_lo == s_lo && s_hi == s_hi) {
            ea = count_le(sx, s_lo, 0, n - 1);   // columns j > ea have x[j] > s_lo (column 0 is never a member)
            eb = count_le(sx, s_hi, 0, n - 1);   // columns j <= eb have x[j] <= s_hi
        } else {
            in_event = false;
        }
    } else {
        in_event = live && cond_member(sx[(DIM == 3 && axis == 1) ? i1 : i0], s_lo, s_hi);
    }

    // ---- membership, k_quant_pass' rule per cut, clamped to the event: columns (ka, kb[i]]
    const double lev = row_level(S, sx, rr_);
    int ka = n, kb[C], kbmax = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) kb[i] = 0;
    if (in_event && a == a) {
        ka = max(count_le(sx, inner_coord(S, a, lev), 0, n - 1), ea);
#pragma unroll
        for (int i = 0; i < C; ++i) {
            if (c[i] == c[i]) kb[i] = min(count_le(sx, inner_coord(S, c[i], lev), 0, n - 1), eb);
            kbmax = max(kbmax, kb[i]);
        }
    }
    // k's range, as k_quant_pass: the column itself over the chunk's union range (opening pass),
    // or the offset from each lane's own ka + 1 over the longest row's length (SKEW)
    int jlo = kbmax > ka ? (SKEW ? 0 : ka + 1) : n, jhi = kbmax > ka ? (SKEW ? kbmax - ka - 1 : kbmax) : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        jlo = min(jlo, __shfl_xor(jlo, o, 64));
        jhi = max(jhi, __shfl_xor(jhi, o, 64));
    }
    jlo = __builtin_amdgcn_readfirstlane(jlo);
    jhi = __builtin_amdgcn_readfirstlane(jhi);
    // This wave's share of the chunk's range.  The split opening pass (2-D) takes k_quant_pass' own
    // range first -- the union over the cuts below +inf, [jlo9, jhi9], split among the waves as there --
    // and then the columns only the +inf cut reaches, below and above it, split the same way: a cut
    // below +inf then sums the columns k_quant_pass sums, per wave and in its order, so the event
    // (-inf, +inf) gives cvq_quantiles' F bit for bit, as the unsplit 3-D pass does by itself.
    constexpr bool SPLIT3 = CS > 1 && !SKEW;
    constexpr int NSEG = SPLIT3 ? 3 : 1;
    int seg_lo[NSEG], seg_hi[NSEG];
    seg_lo[0] = jlo;
    seg_hi[0] = jhi;
    if constexpr (SPLIT3) {
        int kb9 = 0;
#pragma unroll
        for (int i = 0; i < C - 1; ++i) kb9 = max(kb9, kb[i]);
        int jlo9 = kb9 > ka ? ka + 1 : n, jhi9 = kb9 > ka ? kb9 : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            jlo9 = min(jlo9, __shfl_xor(jlo9, o, 64));
            jhi9 = max(jhi9, __shfl_xor(jhi9, o, 64));
        }
        jlo9 = __builtin_amdgcn_readfirstlane(jlo9);
        jhi9 = __builtin_amdgcn_readfirstlane(jhi9);
        if (jhi9 >= jlo9) {                       // (then jlo <= jlo9 and jhi9 <= jhi: kbmax >= kb9 on every lane)
            seg_lo[0] = jlo9;  seg_hi[0] = jhi9;
            seg_lo[1] = jlo;   seg_hi[1] = jlo9 - 1;
            seg_lo[2] = jhi9 + 1;  seg_hi[2] = jhi;
        } else {
            seg_lo[1] = seg_lo[2] = n;
            seg_hi[1] = seg_hi[2] = -1;
        }
    }
#pragma unroll
    for (int g = 0; g < NSEG; ++g) {
        if (CS > 1 && seg_hi[g] >= seg_lo[g]) {
            const int per = (seg_hi[g] - seg_lo[g] + CS) / CS;
            const int lo = seg_lo[g] + (wave % CS) * per;
            seg_hi[g] = min(seg_hi[g], lo + per - 1);
            seg_lo[g] = lo;
        }
    }

    double m0[C], m1[C];
#pragma unroll
    for (int i = 0; i < C; ++i) m0[i] = m1[i] = 0.0;
    bool any = false;
#pragma unroll
    for (int g = 0; g < NSEG; ++g) any = any || seg_hi[g] >= seg_lo[g];
    if (any) {
        // ---- row weights G[b] (outer axes contracted with pi_t), as k_moments
        double G[QT];
        if (DIM == 2) {
#pragma unroll
            for (int bb = 0; bb < QT; ++bb) {
                double g = 0.0;
#pragma unroll
                for (int aa = 0; aa < QT; ++aa) g = fma(pit[aa * q + bb], S.F[(size_t)aa * n + i0], g);
                G[bb] = g;
            }
        } else {
            double f0[QT], f1[QT];
#pragma unroll
            for (int aa = 0; aa < QT; ++aa) {
                f0[aa] = (i1 == 0) ? S.F[(size_t)aa * n + i0] : 1.0;     // Q6: axis-0 factor only at i1 == 0
                f1[aa] = S.F[((size_t)q + aa) * n + i1];
            }
#pragma unroll
            for (int cc = 0; cc < QT; ++cc) {
                double g = 0.0;
#pragma unroll
                for (int bb = 0; bb < QT; ++bb) {
                    double h = 0.0;
#pragma unroll
                    for (int aa = 0; aa < QT; ++aa) h = fma(pit[(aa * q + bb) * q + cc], f0[aa], h);
                    g = fma(h, f1[bb], g);
                }
                G[cc] = g;
            }
        }
        RowCtx ctx;
        if (DIM == 2) ctx = make_row<COP, DIM>(S, At[i0], 0.0, Bt[i0]);
        else ctx = make_row<COP, DIM>(S, At[i0], At[n + i1], outer_B<COP>(Bt[i0], Bt[n + i1]));   // prod over axes in order
        for (int g = 0; g < NSEG; ++g) {
        const int kl = g == 0 ? seg_lo[0] : g == 1 ? seg_lo[NSEG > 1 ? 1 : 0] : seg_lo[NSEG > 2 ? 2 : 0];
        const int kh = g == 0 ? seg_hi[0] : g == 1 ? seg_hi[NSEG > 1 ? 1 : 0] : seg_hi[NSEG > 2 ? 2 : 0];
        for (int k = kl; k <= kh; ++k) {          // wave-uniform trip count
            const int jm = SKEW ? ka + 1 + k : k;               // the column whose membership is tested
            const int j = SKEW ? min(jm, n - 1) : k;            // the column loaded (in the grid)
            double W = 0.0;
#pragma unroll
            for (int bb = 0; bb < QT; ++bb) W = fma(G[bb], Fc[(size_t)bb * n + j], W);
            const double v = node_value<COP, MSM, DIM>(S, ctx, Ac[j], Bc[j], W);
            const double lv = (lev + S.w0 * sx[j]) * v;
            if (jm > ka) {
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    if (jm <= kb[i]) {
                        m0[i] += v;
                        m1[i] += lv;
                    }
                }
            }
        }
        }
    }
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const double s0 = wave_sum(m0[i]), s1 = wave_sum(m1[i]);
        if (lane == 0) { red[wave][2 * i] = s0; red[wave][2 * i + 1] = s1; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * C) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kMomWaves; ++w) s += red[w][threadIdx.x];
        part[(tl * gridDim.y + blockIdx.y) * (2 * C) + threadIdx.x] = s;
    }
}

// k_quant_update with the per-date target alpha p_E (one FP64 product).  open: the opening pass's
// partials are [T][1][chunks][10][2]; its last cut (+inf) summed in index order is p_E, kept in the
// state (and written to pe_out by the date's first level) before the bracket test
// F_E(min_var) < alpha p_E <= F_E(max_var); p_E == 0 fails it.
__global__ __launch_bounds__(256) void k_cond_update(long long T, int L, int chunks, QuantLevels lv, bool open,
                                                     CondUniform U, int steps, bool last, double ptf_mean,
                                                     const double* __restrict__ part, double* __restrict__ st,
                                                     double* __restrict__ cuts, double* __restrict__ var_out,
                                                     double* __restrict__ pe_out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * L) return;
    double* s = st + (size_t)idx * kCondState;
    double* c = cuts + (size_t)idx * kQuantCuts;
    const int C = open ? kCondOpenCuts : kQuantCuts, first = open ? 1 : 0;
    const double* p = part + (size_t)(open ? idx / L : idx) * chunks * 2 * C;
    double lo, hi, f_lo, m_lo, pe;
    bool ok;
    if (open) {
        double pm;
        quant_sum(p, chunks, C, C - 1, &pe, &pm);     // the +inf cut: the event's mass over the whole box
        s[6] = pe;
        if (pe_out && idx % L == 0) pe_out[idx / L] = pe;
    } else {
        pe = s[6];
    }
    const double alpha = lv.alpha[idx % L] * pe;
    if (open) {
        double f_hi, m_hi;
        quant_sum(p, chunks, C, 0, &f_lo, &m_lo);
        quant_sum(p, chunks, C, C - 2, &f_hi, &m_hi);
        ok = f_lo < alpha && alpha <= f_hi;
        const double nan = __builtin_nan("");
        lo = ok ? U.c[0] : nan;
        hi = ok ? U.c[C - 2] : nan;
        s[4] = ok ? 1.0 : 0.0;
        s[5] = f_hi;
    } else {
        lo = s[0], hi = s[1], f_lo = s[2], m_lo = s[3];
        ok = s[4] != 0.0;
    }
    if (ok) {
        const double f0 = open ? 0.0 : f_lo, m0 = open ? 0.0 : m_lo;     // the pass summed from `lower` / from lo
        int at = 3;
        for (int k = 0, half = 2; k < steps; ++k, half >>= 1) {
            double d0, d1;
            quant_sum(p, chunks, C, first + at, &d0, &d1);
            const double mid = open ? U.c[first + at] : c[at];
            const double f_mid = f0 + d0;
            if (f_mid < alpha) {
                lo = mid;
                f_lo = f_mid;
                m_lo = m0 + d1;
                at += half;
            } else {
                hi = mid;
                at -= half;
            }
        }
    }
    s[0] = lo;
    s[1] = hi;
    s[2] = f_lo;
    s[3] = m_lo;
    if (!last) {
        quant_cuts(lo, hi, c);
        return;
    }
    const double var = (lo + hi) / 2 + ptf_mean;      // NaN outside the bracket
    var_out[idx] = var;
    c[0] = c[1] = var - ptf_mean;                     // the closing pass's upper edge
}

// After the closing pass (part [T][L][chunks][2][2] over (lo, covar - ptf_mean] within the event):
// m0 = F_E(covar - ptf_mean) and coes = M1_E / m0 + ptf_mean; outside the bracket coes = NaN and
// m0 = F_E(max_var).
__global__ __launch_bounds__(256) void k_cond_finish(long long T, int L, int chunks, double ptf_mean,
                                                     const double* __restrict__ part, const double* __restrict__ st,
                                                     double* __restrict__ es_out, double* __restrict__ m0_out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * L) return;
    const double* s = st + (size_t)idx * kCondState;
    double m0 = s[5], es = __builtin_nan("");
    if (s[4] != 0.0) {
        double d0, d1;
        quant_sum(part + (size_t)idx * chunks * 4, chunks, 2, 0, &d0, &d1);
        m0 = s[2] + d0;
        const double m1 = s[3] + d1;
        if (m0 != 0.0) es = m1 / m0 + ptf_mean;
    }
    if (es_out) es_out[idx] = es;
    if (m0_out) m0_out[idx] = m0;
}

}  // namespace cvq
