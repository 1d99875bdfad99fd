// cvq_dynamic_kernels.h -- exact quantiles under per-date copula parameters and weights
// (cvq_dynamic_quantiles): cvq_quantiles' bisection of F(v) = mass of the slab (lower, v] where
// every date carries a record of its own.  No reference counterpart.
//
// The copula parameters reach the generic node path through a few plan constants only: theta
// (Plackett's and Gumbel's node value, Gumbel's table entries), term1 and the inverse correlation
// Ri[9] (Gaussian / Student: make_row and node_value).  The weights reach it through row_level,
// inner_coord and the level factor of the first moment.  So a workgroup, which serves one date,
// takes that date's record
//   theta, term1, Ri[9], w0, w1, w2, w0_inv, pad          (16 doubles = 128 bytes)
// from a device array [T][16] into a local StaticDev copy (wave-uniform loads), on which the slab
// paths' own helpers run unchanged: the same expressions in the same order as a plan created with
// that date's parameters and weights, bit for bit.  The copula kind, the Gumbel survival flag and
// the Student nu (with tk, g_uni, node_m, uni_m: the quantile tables hang on them) stay the plan's.
//
// k_dyn_pass is k_quant_pass (same mapping, same partial layout per (date, level), same
// fixed-order reduction) on that copy; grid z = 1 in the opening pass (its nine cuts depend on
// neither level nor record), levels in the narrow passes.  No atomics, no waiting between
// workgroups: a date's result depends on its own record and inputs alone.
#pragma once
// cvq_quantile_kernels.h defines its two plain (non-template) kernels in every unit that
// includes it.  This unit takes its helpers (quant_cuts, quant_sum), constants and structs only,
// so its copies of those two kernels get names of their own and cvq_quantile.hip keeps the
// originals.
#define k_quant_update k_quant_update_dynamic_unit
#define k_quant_finish k_quant_finish_dynamic_unit
#include "cvq_quantile_kernels.h"
#undef k_quant_update
#undef k_quant_finish

namespace cvq {

constexpr int kDynRec = 16;                    // doubles per date record
// offsets into a record
constexpr int kDynTheta = 0, kDynTerm1 = 1, kDynRi = 2, kDynW = 11, kDynW0Inv = 14;

// The date's record onto a copy of the plan's constants.
__device__ __forceinline__ void dyn_overlay(StaticDev& S, const double* __restrict__ rec) {
    S.theta = rec[kDynTheta];
    S.term1 = rec[kDynTerm1];
#pragma unroll
    for (int i = 0; i < 9; ++i) S.Ri[i] = rec[kDynRi + i];
    S.w0 = rec[kDynW];
    S.w1 = rec[kDynW + 1];
    S.w2 = rec[kDynW + 2];
    S.w0_inv = rec[kDynW0Inv];
}

// k_moments_tables with the date's theta (Gumbel: A = x^theta, B's (theta - 1) log x; Frank / Joe:
// prod_entry's generator value and log factor); the other
// kinds' tables do not depend on the varying parameters and never read the records.
template <int COP, bool MSM, bool TAB>
__global__ __launch_bounds__(256) void k_dyn_tables(StaticDev S0, long long T, const double* __restrict__ a,
                                                    const double* __restrict__ rec, double* __restrict__ tA,
                                                    double* __restrict__ tB) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * S0.dim * S0.n) return;
    const int i = (int)(idx % S0.n);
    const long long td = idx / S0.n;
    const int d = (int)(td % S0.dim);
    double A, B;
    if constexpr (kLogB<COP>) {
        StaticDev S = S0;
        S.theta = rec[(td / S0.dim) * kDynRec + kDynTheta];
        table_entry<COP, MSM, TAB>(S, a, td, d, i, &A, &B);
    } else {
        table_entry<COP, MSM, TAB>(S0, a, td, d, i, &A, &B);
    }
    tA[idx] = A;
    tB[idx] = B;
}

// st == nullptr: the opening pass, U's edge and first C cuts for every date (one level).
template <int COP, bool MSM, int DIM, int QT, int C>
__global__ __launch_bounds__(kMomNT) void k_dyn_pass(StaticDev S0, const double* __restrict__ tA,
                                                     const double* __restrict__ tB, const double* __restrict__ pi,
                                                     const double* __restrict__ rec, const double* __restrict__ st,
                                                     const double* __restrict__ cuts, QuantUniform U,
                                                     double* __restrict__ part) {
    constexpr int CS = moments_colsplit(DIM);
    constexpr bool SKEW = C != kQuantOpenCuts;   // narrow passes: each lane walks its own columns
    __shared__ double sx[kMomMaxN];
    __shared__ double red[kMomWaves][2 * C];
    const long long t = blockIdx.x;
    StaticDev S = S0;                            // the plan's constants under the date's record
    dyn_overlay(S, rec + t * kDynRec);
    const int n = S.n, q = QT;
    for (int j = threadIdx.x; j < n; j += kMomNT) sx[j] = S.x[j];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t tl = (size_t)t * gridDim.z + blockIdx.z;
    const int r = (int)blockIdx.y * moments_chunk_rows(DIM) + (wave / CS) * 64 + lane;
    const bool live = r < S.nrows;
    double a, c[C];
    if (st) {
        a = st[tl * kQuantState];
#pragma unroll
        for (int i = 0; i < C; ++i) c[i] = cuts[tl * kQuantCuts + i];
    } else {
        a = U.a;
#pragma unroll
        for (int i = 0; i < C; ++i) c[i] = U.c[i < kQuantOpenCuts ? i : 0];
    }

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

    // ---- membership, k_quant_pass' rule per cut on the date's weights: columns (ka, kb[i]]
    const double lev = row_level(S, sx, rr_);
    int ka = n, kb[C], kbmax = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) kb[i] = 0;
    if (live && a == a) {
        ka = count_le(sx, inner_coord(S, a, lev), 0, n - 1);
#pragma unroll
        for (int i = 0; i < C; ++i) {
            if (c[i] == c[i]) kb[i] = count_le(sx, inner_coord(S, c[i], lev), 0, n - 1);
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
    // this wave's share of the chunk's range
    int j0 = jlo, j1 = jhi;
    if (CS > 1 && jhi >= jlo) {
        const int per = (jhi - jlo + CS) / CS;
        j0 = jlo + (wave % CS) * per;
        j1 = min(jhi, j0 + per - 1);
    }

    double m0[C], m1[C];
#pragma unroll
    for (int i = 0; i < C; ++i) m0[i] = m1[i] = 0.0;
    if (j1 >= j0) {
        // ---- row weights G[b] (outer axes contracted with pi_t), as k_moments: record-free
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
        for (int k = j0; k <= j1; ++k) {          // wave-uniform trip count
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

// k_quant_update per (date, level) with the date's own ptf_mean[t].
__global__ __launch_bounds__(256) void k_dyn_update(long long T, int L, int chunks, QuantLevels lv, bool open,
                                                    QuantUniform U, int steps, bool last,
                                                    const double* __restrict__ ptf_mean,
                                                    const double* __restrict__ part, double* __restrict__ st,
                                                    double* __restrict__ cuts, double* __restrict__ var_out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * L) return;
    const double alpha = lv.alpha[idx % L];
    double* s = st + (size_t)idx * kQuantState;
    double* c = cuts + (size_t)idx * kQuantCuts;
    const int C = open ? kQuantOpenCuts : kQuantCuts, first = open ? 1 : 0;
    const double* p = part + (size_t)(open ? idx / L : idx) * chunks * 2 * C;
    double lo, hi, f_lo, m_lo;
    bool ok;
    if (open) {
        double f_hi, m_hi;
        quant_sum(p, chunks, C, 0, &f_lo, &m_lo);
        quant_sum(p, chunks, C, C - 1, &f_hi, &m_hi);
        ok = f_lo < alpha && alpha <= f_hi;
        const double nan = __builtin_nan("");
        lo = ok ? U.c[0] : nan;
        hi = ok ? U.c[C - 1] : nan;
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
    const double mean = ptf_mean[idx / L];
    const double var = (lo + hi) / 2 + mean;          // NaN outside the bracket
    var_out[idx] = var;
    c[0] = c[1] = var - mean;                         // the closing pass's upper edge
}

// k_quant_finish per (date, level) with the date's own ptf_mean[t].
__global__ __launch_bounds__(256) void k_dyn_finish(long long T, int L, int chunks,
                                                    const double* __restrict__ ptf_mean,
                                                    const double* __restrict__ part, const double* __restrict__ st,
                                                    double* __restrict__ es_out, double* __restrict__ m0_out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * L) return;
    const double* s = st + (size_t)idx * kQuantState;
    double m0 = s[5], es = __builtin_nan("");
    if (s[4] != 0.0) {
        double d0, d1;
        quant_sum(part + (size_t)idx * chunks * 4, chunks, 2, 0, &d0, &d1);
        m0 = s[2] + d0;
        const double m1 = s[3] + d1;
        if (m0 != 0.0) es = m1 / m0 + ptf_mean[idx / L];
    }
    if (es_out) es_out[idx] = es;
    if (m0_out) m0_out[idx] = m0;
}

}  // namespace cvq
