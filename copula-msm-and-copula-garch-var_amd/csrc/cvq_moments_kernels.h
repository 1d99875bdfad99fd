// cvq_moments_kernels.h -- tail moments of a slab: m0 = sum of the node masses of (a, b] and
// m1 = sum of level x mass, the two sums behind the Expected Shortfall
//   es_t = m1_t / m0_t + ptf_mean      over (lower, var_t - ptf_mean].
// No reference counterpart (the reference stops at the VaR); membership, node values and the
// Delta weights are the slab paths' own (create_grids.py:102-108, Q5/Q6/Q9/Q10/Q15).
//
// Mapping: grid (dates x row chunks), 256 threads = 4 waves per workgroup, lane = row as in
// k_mass, so every column operand is wave-uniform.
//   2-D: a chunk is 64 rows; the four waves share them and take a quarter each of the chunk's
//        column range [min ka + 1, max kb] (a date of n <= 1024 rows is only 1-16 chunks, so
//        the column split is where a small batch gets its parallelism);
//   3-D: a chunk is 256 rows, one wave per 64 rows over all columns (n^2 rows: plenty of
//        chunks, and the per-row weights G[b] cost q^3 FMAs, so rows are not shared).
// A workgroup writes its partial (m0, m1) to part[t][chunk]; k_moments_finish sums a date's
// chunks in index order.  No atomics and no waiting between workgroups: a date's result is a
// fixed-order sum that depends on that date's inputs alone (bit-identical between runs and
// across batches).  LDS: the grid copy (8 KB) + 64 B.
#pragma once
#include "cvq_quad_kernels.h"

namespace cvq {

constexpr int kMomNT = 256;                    // threads per workgroup
constexpr int kMomWaves = kMomNT / 64;
constexpr int kMomMaxN = 1024;                 // LDS grid copy

__host__ __device__ constexpr int moments_colsplit(int dim) { return dim == 2 ? kMomWaves : 1; }
// outer rows per chunk: a function of the plan's geometry only, never of T
__host__ __device__ constexpr int moments_chunk_rows(int dim) { return 64 * (kMomWaves / moments_colsplit(dim)); }
__host__ __device__ constexpr int moments_chunks(int dim, int nrows) {
    return (nrows + moments_chunk_rows(dim) - 1) / moments_chunk_rows(dim);
}

// Per-date marginal tables into the moments scratch (k_tables' layout [T][dim][n]); TAB: the
// plan's direct t.ppf tables, as the fused slab paths evaluate their entries.
template <int COP, bool MSM, bool TAB>
__global__ __launch_bounds__(256) void k_moments_tables(StaticDev S, long long T, const double* __restrict__ a,
                                                        double* __restrict__ tA, double* __restrict__ tB) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * S.dim * S.n) return;
    const int i = (int)(idx % S.n);
    const long long td = idx / S.n;
    const int d = (int)(td % S.dim);
    double A, B;
    table_entry<COP, MSM, TAB>(S, a, td, d, i, &A, &B);
    tA[idx] = A;
    tB[idx] = B;
}

// bounds != nullptr: slab (bounds[t][0], bounds[t][1]]; else (lower, var[t] - ptf_mean].
template <int COP, bool MSM, int DIM, int QT>
__global__ __launch_bounds__(kMomNT) void k_moments(StaticDev S, const double* __restrict__ tA,
                                                    const double* __restrict__ tB, const double* __restrict__ pi,
                                                    const double* __restrict__ bounds, const double* __restrict__ var,
                                                    double lower, double ptf_mean, double* __restrict__ part) {
    constexpr int CS = moments_colsplit(DIM);
    __shared__ double sx[kMomMaxN];
    __shared__ double red[kMomWaves][2];
    const int n = S.n, q = QT;
    for (int j = threadIdx.x; j < n; j += kMomNT) sx[j] = S.x[j];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long t = blockIdx.x;
    const int r = (int)blockIdx.y * moments_chunk_rows(DIM) + (wave / CS) * 64 + lane;
    const bool live = r < S.nrows;
    const double a = bounds ? bounds[2 * t] : lower;
    const double b = bounds ? bounds[2 * t + 1] : var[t] - ptf_mean;

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

    // ---- membership (SolveTeam::count's rule over the whole inner axis): columns (ka, kb];
    // a NaN bound compares false with every node (empty slab); column 0 is never a member (Q9)
    const double lev = row_level(S, sx, rr_);
    int ka = 0, kb = 0;
    if (live && a == a && b == b) {
        ka = count_le(sx, inner_coord(S, a, lev), 0, n - 1);
        kb = count_le(sx, inner_coord(S, b, lev), 0, n - 1);
    }
    int jlo = kb > ka ? ka + 1 : n, jhi = kb > ka ? kb : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        jlo = min(jlo, __shfl_xor(jlo, o, 64));
        jhi = max(jhi, __shfl_xor(jhi, o, 64));
    }
    jlo = __builtin_amdgcn_readfirstlane(jlo);
    jhi = __builtin_amdgcn_readfirstlane(jhi);
    // this wave's share of the chunk's column range
    int j0 = jlo, j1 = jhi;
    if (CS > 1 && jhi >= jlo) {
        const int per = (jhi - jlo + CS) / CS;
        j0 = jlo + (wave % CS) * per;
        j1 = min(jhi, j0 + per - 1);
    }

    double m0 = 0.0, m1 = 0.0;
    if (j1 >= j0) {
        // ---- row weights G[b] (outer axes contracted with pi_t), as k_mass
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
            for (int c = 0; c < QT; ++c) {
                double g = 0.0;
#pragma unroll
                for (int bb = 0; bb < QT; ++bb) {
                    double h = 0.0;
#pragma unroll
                    for (int aa = 0; aa < QT; ++aa) h = fma(pit[(aa * q + bb) * q + c], f0[aa], h);
                    g = fma(h, f1[bb], g);
                }
                G[c] = g;
            }
        }
        RowCtx ctx;
        if (DIM == 2) ctx = make_row<COP, DIM>(S, At[i0], 0.0, Bt[i0]);
        else ctx = make_row<COP, DIM>(S, At[i0], At[n + i1], outer_B<COP>(Bt[i0], Bt[n + i1]));   // prod over axes in order
        for (int j = j0; j <= j1; ++j) {          // wave-uniform
            double W = 0.0;
#pragma unroll
            for (int bb = 0; bb < QT; ++bb) W = fma(G[bb], Fc[(size_t)bb * n + j], W);
            const double v = node_value<COP, MSM, DIM>(S, ctx, Ac[j], Bc[j], W);
            const double level = lev + S.w0 * sx[j];
            if (j > ka && j <= kb) {
                m0 += v;
                m1 += level * v;
            }
        }
    }
    m0 = wave_sum(m0);
    m1 = wave_sum(m1);
    if (lane == 0) { red[wave][0] = m0; red[wave][1] = m1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = red[0][0], s1 = red[0][1];
#pragma unroll
        for (int w = 1; w < kMomWaves; ++w) { s0 += red[w][0]; s1 += red[w][1]; }
        double* dst = part + ((size_t)t * gridDim.y + blockIdx.y) * 2;
        dst[0] = s0;
        dst[1] = s1;
    }
}

// One thread per date: its chunks summed in index order.  var == nullptr: out0 = m0, out1 = m1.
// Else the Expected Shortfall: out1 = m1 / m0 + ptf_mean, NaN where var[t] is NaN (Q3 brackets)
// or m0 == 0; out0 = m0 (may be nullptr).  (Not a template: defined in cvq_moments.hip's
// translation unit only; cvq_quantile.hip includes this header without it.)
#ifndef CVQ_NO_MOMENTS_FINISH
__global__ __launch_bounds__(256) void k_moments_finish(long long T, int chunks, const double* __restrict__ part,
                                                        const double* __restrict__ var, double ptf_mean,
                                                        double* __restrict__ out0, double* __restrict__ out1) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const double* p = part + (size_t)t * chunks * 2;
    double s0 = p[0], s1 = p[1];
    for (int c = 1; c < chunks; ++c) { s0 += p[2 * c]; s1 += p[2 * c + 1]; }
    if (!var) {
        out0[t] = s0;
        out1[t] = s1;
        return;
    }
    if (out0) out0[t] = s0;
    const double v = var[t];
    out1[t] = (v == v && s0 != 0.0) ? s1 / s0 + ptf_mean : __builtin_nan("");
}
#endif

}  // namespace cvq
