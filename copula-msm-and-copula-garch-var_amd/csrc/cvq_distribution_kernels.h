// cvq_distribution_kernels.h -- the predictive distribution of the portfolio return
// (cvq_distribution): per date, (m0, m1) of up to CVQ_MAX_BINS slabs (e[b], e[b+1]] in one sweep.
// No reference counterpart; membership, node values and Delta weights are the slab paths' own,
// a bin's pair is cvq_slab_moments' of that slab to rounding.
//
// k_dist_pass is k_moments' row setup shared by the bins of a call: grid (dates x row chunks x
// bin groups), 256 threads = 4 waves, lane = row, k_moments' chunks (2-D: 64 rows shared by the
// four waves, 3-D: 256 rows, one wave per 64).  Once per row: the grid copy and the date's edges
// in LDS, row_level, the row weights G[] and make_row.  Then a wave-uniform loop over the bins;
// per bin each lane walks its own columns (ka_b, kb_b] from count_le (k_quant_pass' SKEW form:
// k counts from the lane's ka_b + 1, the trip count is the longest row's length, per-lane column
// operands at neighbouring addresses; in 2-D the four waves take a quarter of that range each).
// With an ascending ladder the bins' column ranges are disjoint: every node is evaluated once.
// Per bin a wave_sum pair goes to LDS; after the loop the waves' pairs are summed in wave order
// and written to part[t][chunk][bin][2]; k_dist_finish sums a date's chunks in index order.
//
// Every step of a bin's sum -- the lane's columns in order, the wave tree, waves in order, chunks
// in order, the column split (a function of the bin's own longest row) -- depends on the bin's two
// edges and the date's inputs alone: not on the other bins, their number, order or grouping, nor
// on the other dates.  No atomics, no waiting between workgroups.
// LDS: the grid copy (8 KB) + edges (520 B) + the waves' pairs (4 KB).  Registers: nothing is
// indexed by the bin (edges and pairs live in LDS), so no instance has a private segment.
#pragma once
#include "cvq_moments_kernels.h"

namespace cvq {

constexpr int kDistMaxBins = 64;               // CVQ_MAX_BINS

// A ladder shared by every date (per_date == 0), passed as a kernel argument.
struct DistEdges {
    double e[kDistMaxBins + 1];
};

// edges != nullptr: the date's own ladder edges[t][nb + 1]; else U's.  Workgroup z serves bins
// [z * per_group, min(nb, (z + 1) * per_group)).
template <int COP, bool MSM, int DIM, int QT>
__global__ __launch_bounds__(kMomNT) void k_dist_pass(StaticDev S, const double* __restrict__ tA,
                                                      const double* __restrict__ tB, const double* __restrict__ pi,
                                                      const double* __restrict__ edges, DistEdges U, int nb,
                                                      int per_group, double* __restrict__ part) {
    constexpr int CS = moments_colsplit(DIM);
    __shared__ double sx[kMomMaxN];
    __shared__ double se[kDistMaxBins + 1];
    __shared__ double red[kMomWaves][2 * kDistMaxBins];
    const int n = S.n, q = QT;
    const long long t = blockIdx.x;
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
    const double lev = row_level(S, sx, rr_);

    // ---- row weights G[b] (outer axes contracted with pi_t) and the row context, as k_moments:
    // once per row, whatever the number of bins
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

    for (int b = b0; b < b1; ++b) {               // wave-uniform
        const double a = se[b - b0], c = se[b - b0 + 1];
        double m0 = 0.0, m1 = 0.0;
        if (c > a) {                              // a NaN edge, a repeated or a descending pair: exactly (0, 0)
            // ---- membership, k_moments' rule: columns (ka, kb]; column 0 is never a member (Q9)
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

// One thread per (date, bin): its chunks summed in index order.  m1_out may be nullptr.
__global__ __launch_bounds__(256) void k_dist_finish(long long T, int nb, int chunks, const double* __restrict__ part,
                                                     double* __restrict__ mass_out, double* __restrict__ m1_out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * nb) return;
    const long long t = idx / nb;
    const int b = (int)(idx % nb);
    const double* p = part + ((size_t)t * chunks * nb + b) * 2;
    double s0 = p[0], s1 = p[1];
    for (int c = 1; c < chunks; ++c) {
        s0 += p[(size_t)c * nb * 2];
        s1 += p[(size_t)c * nb * 2 + 1];
    }
    mass_out[idx] = s0;
    if (m1_out) m1_out[idx] = s1;
}

}  // namespace cvq
