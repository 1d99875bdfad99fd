// cvq_dynamic_distribution_kernels.h -- the predictive distribution under per-date copula
// parameters and weights (cvq_dynamic_distribution): cvq_distribution's bin sweep where every date
// carries the 128-byte record of cvq_dynamic_quantiles.  No reference counterpart.
//
// k_dyn_dist_pass is k_dist_pass (same grid of dates x row chunks x bin groups, same chunk and wave
// mapping, same LDS, same per-bin SKEW walk, same fixed-order reduction, same
// part[t][chunk][bin][2] layout) on a local StaticDev copy that carries the date's record
//   theta, term1, Ri[9], w0, w1, w2, w0_inv, pad          (16 doubles)
// applied by dyn_overlay as k_dyn_pass applies it: the slab paths' own helpers run unchanged on
// the copy, the same expressions in the same order as a plan created with that date's parameters
// and weights, bit for bit.  The tables of the kinds whose entries depend on theta (kLogB) come
// from k_dyn_tables; k_dist_finish sums a date's chunks.  The copula kind, the survival / family
// code and the Student nu stay the plan's.
//
// The record loads are wave-uniform (the address depends on blockIdx.x alone), so the 15 values
// live in scalar registers beside the kernel arguments they replace: the copy costs no vector
// registers.  No atomics, no waiting between workgroups; LDS as k_dist_pass: 12 808 bytes.
#pragma once
// The two parent headers define plain (non-template) kernels in every unit that includes them.
// This unit launches k_dist_finish and none of the others, so its copies get names of their own
// and cvq_distribution.hip / cvq_dynamic.hip / cvq_quantile.hip keep theirs.  The quantile header
// comes first: cvq_dynamic_kernels.h's own renaming of it is then a no-op (#pragma once).
#define k_quant_update k_quant_update_dyndist_unit
#define k_quant_finish k_quant_finish_dyndist_unit
#include "cvq_quantile_kernels.h"
#undef k_quant_update
#undef k_quant_finish
#define k_dyn_update k_dyn_update_dyndist_unit
#define k_dyn_finish k_dyn_finish_dyndist_unit
#include "cvq_dynamic_kernels.h"
#undef k_dyn_update
#undef k_dyn_finish
#define k_dist_finish k_dist_finish_dyndist_unit
#include "cvq_distribution_kernels.h"
#undef k_dist_finish

namespace cvq {

// rec: device [T][kDynRec].  edges != nullptr: the date's own ladder edges[t][nb + 1]; else U's.
// Workgroup z serves bins [z * per_group, min(nb, (z + 1) * per_group)).
template <int COP, bool MSM, int DIM, int QT>
__global__ __launch_bounds__(kMomNT) void k_dyn_dist_pass(StaticDev S0, const double* __restrict__ tA,
                                                          const double* __restrict__ tB,
                                                          const double* __restrict__ pi,
                                                          const double* __restrict__ rec,
                                                          const double* __restrict__ edges, DistEdges U, int nb,
                                                          int per_group, double* __restrict__ part) {
    constexpr int CS = moments_colsplit(DIM);
    __shared__ double sx[kMomMaxN];
    __shared__ double se[kDistMaxBins + 1];
    __shared__ double red[kMomWaves][2 * kDistMaxBins];
    const long long t = blockIdx.x;
    StaticDev S = S0;                            // the plan's constants under the date's record
    dyn_overlay(S, rec + t * kDynRec);
    const int n = S.n, q = QT;
    const int b0 = (int)blockIdx.z * per_group, b1 = min(nb, b0 + per_group);
    for (int j = threadIdx.x; j < n; j += kMomNT) sx[j] = S.x[j];
    for (int j = b0 + (int)threadIdx.x; j <= b1; j += kMomNT)
        se[j - b0] = edges ? edges[(size_t)t * (nb + 1) + j] : U.e[j];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = (int)blockIdx.y * moments_chunk_rows(DIM) + (wave / CS) * 64 + lane;
    const bool live = r < S.nrows;

    const double* At = tA + t * S.dim * n;
    const double* Bt = tB + t * S.dim * n;
    const double* pit = pi + t * S.Q;
    const int inner = DIM - 1;
    const double* Ac = At + inner * n;           // inner-axis tables
    const double* Bc = Bt + inner * n;
    const double* Fc = S.F + (size_t)inner * q * n;

    const int rr_ = live ? r : 0;
    const int i0 = (DIM == 2) ? rr_ : rr_ / n;
    const int i1 = (DIM == 2) ? 0 : rr_ % n;
    const double lev = row_level(S, sx, rr_);    // the date's weights

    // ---- row weights G[b] (outer axes contracted with pi_t), as k_moments: record-free, once
    // per row, whatever the number of bins
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
    RowCtx ctx;                                   // the date's theta / Ri / term1
    if (DIM == 2) ctx = make_row<COP, DIM>(S, At[i0], 0.0, Bt[i0]);
    else ctx = make_row<COP, DIM>(S, At[i0], At[n + i1], outer_B<COP>(Bt[i0], Bt[n + i1]));   // prod over axes in order

    for (int b = b0; b < b1; ++b) {               // wave-uniform
        const double a = se[b - b0], c = se[b - b0 + 1];
        double m0 = 0.0, m1 = 0.0;
        if (c > a) {                              // a NaN edge, a repeated or a descending pair: exactly (0, 0)
            // ---- membership, k_moments' rule on the date's weights: columns (ka, kb]; column 0 is
            // never a member (Q9)
            int ka = 0, len = 0;
            if (live) {
                ka = count_le(sx, inner_coord(S, a, lev), 0, n - 1);
                len = max(count_le(sx, inner_coord(S, c, lev), 0, n - 1) - ka, 0);
            }
            int kmax = len;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o, 64));
            kmax = __builtin_amdgcn_readfirstlane(kmax);
            // this wave's share of the longest row's length (the four waves of a 2-D chunk hold
            // the same rows, so kmax is the same in all of them)
            int k0 = 0, k1 = kmax;
            if (CS > 1) {
                const int per = (kmax + CS - 1) / CS;
                k0 = (wave % CS) * per;
                k1 = min(kmax, k0 + per);
            }
            for (int k = k0; k < k1; ++k) {       // wave-uniform trip count
                const int j = min(ka + 1 + k, n - 1);               // the column loaded (in the grid)
                double W = 0.0;
#pragma unroll
                for (int bb = 0; bb < QT; ++bb) W = fma(G[bb], Fc[(size_t)bb * n + j], W);
                const double v = node_value<COP, MSM, DIM>(S, ctx, Ac[j], Bc[j], W);
                const double lv = (lev + S.w0 * sx[j]) * v;
                if (k < len) {
                    m0 += v;
                    m1 += lv;
                }
            }
            m0 = wave_sum(m0);
            m1 = wave_sum(m1);
        }
        if (lane == 0) {
            red[wave][2 * (b - b0)] = m0;
            red[wave][2 * (b - b0) + 1] = m1;
        }
    }
    __syncthreads();
    double* dst = part + (((size_t)t * gridDim.y + blockIdx.y) * nb + b0) * 2;
    for (int i = threadIdx.x; i < 2 * (b1 - b0); i += kMomNT) {
        double s = red[0][i];
#pragma unroll
        for (int w = 1; w < kMomWaves; ++w) s += red[w][i];
        dst[i] = s;
    }
}

}  // namespace cvq
