// cvq_attrib_kernels.h -- per-axis first moments of a slab: m0 = sum of the node masses of
// (a, b] and mx[c] = sum of x[i_c] x mass for every grid axis c, the sums behind the Euler
// allocation of the Expected Shortfall
//   contrib[t][c] = wa[c] mx[c] / m0      over (lower, var_t - ptf_mean],
//   wa[dim - 1] = w[0] (the inner axis), wa[c] = w[c + 1] for c < dim - 1 (Q10),
// so that sum_c wa[c] mx[c] = k_moments' m1 and sum_c contrib[t][c] = es_t - ptf_mean.
// No reference counterpart; membership, node values and the Delta weights are k_moments' own.
//
// Mapping: k_moments' exactly (grid (dates x row chunks), 256 threads, lane = row, the 2-D
// column split over the four waves, 3-D one wave per 64 rows).  The outer coordinates are
// constant along a row, so the column loop keeps two accumulators, s0 += v (k_moments' m0 in
// the same order: bit-identical) and sj += x[j] v; the outer axes' moments are x[i_c] s0 after
// the loop.  A workgroup writes its 1 + DIM partial sums to part[t][chunk]; k_attrib_finish
// sums a date's chunks in index order.  No atomics and no waiting between workgroups.
// LDS: the grid copy (8 KB) + 128 B.
#pragma once
#include "cvq_moments_kernels.h"

namespace cvq {

// bounds != nullptr: slab (bounds[t][0], bounds[t][1]]; else (lower, var[t] - ptf_mean].
template <int COP, bool MSM, int DIM, int QT>
__global__ __launch_bounds__(kMomNT) void k_attrib(StaticDev S, const double* __restrict__ tA,
                                                   const double* __restrict__ tB, const double* __restrict__ pi,
                                                   const double* __restrict__ bounds, const double* __restrict__ var,
                                                   double lower, double ptf_mean, double* __restrict__ part) {
    constexpr int CS = moments_colsplit(DIM);
    constexpr int NS = 1 + DIM;                  // sums per workgroup: m0, mx[0 .. DIM-1]
    __shared__ double sx[kMomMaxN];
    __shared__ double red[kMomWaves][NS];
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

    // ---- membership: columns (ka, kb], as k_moments (NaN bound: empty; column 0 never, Q9)
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

    double s0 = 0.0, sj = 0.0;
    if (j1 >= j0) {
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
            if (j > ka && j <= kb) {
                s0 += v;
                sj += sx[j] * v;
            }
        }
    }
    // axis moments of this lane's row: the outer coordinates times the row's mass, the inner
    // axis' own sum last (axis order = asset order)
    double s[NS];
    s[0] = s0;
    s[1] = sx[i0] * s0;
    if (DIM == 3) s[2] = sx[i1] * s0;
    s[DIM] = sj;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double w = wave_sum(s[k]);
        if (lane == 0) red[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int k = threadIdx.x;
        double acc = red[0][k];
#pragma unroll
        for (int w = 1; w < kMomWaves; ++w) acc += red[w][k];
        part[((size_t)t * gridDim.y + blockIdx.y) * NS + k] = acc;
    }
}

// One thread per date: its chunks summed in index order; the records are loaded eight at a time
// so that a lone date (3-D: 64 chunks) does not pay one load latency per chunk.  var == nullptr:
// out_m0 = m0, out_x[t][c] = mx[c].  Else the contributions of (lower, var[t] - ptf_mean]:
// out_x[t][c] = wa[c] mx[c] / m0, the whole row NaN where var[t] is NaN (Q3 brackets) or
// m0 == 0 (cvq_expected_shortfall's rules); out_m0 = m0 (may be nullptr).  wa: the weight of
// each axis in the membership rule (Q10), by axis.
struct AxisWeights { double wa[3]; };
constexpr int kAttribFinishBatch = 8;         // chunk records k_attrib_finish loads before it adds them

template <int DIM>
__global__ __launch_bounds__(256) void k_attrib_finish(long long T, int chunks, AxisWeights W,
                                                       const double* __restrict__ part,
                                                       const double* __restrict__ var, double* __restrict__ out_m0,
                                                       double* __restrict__ out_x) {
    constexpr int NS = 1 + DIM;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const double* p = part + (size_t)t * chunks * NS;
    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = p[k];
    int c = 1;
    for (; c + kAttribFinishBatch <= chunks; c += kAttribFinishBatch) {      // loads of a batch in flight together,
        double v[kAttribFinishBatch][NS];                                    // added in index order all the same
#pragma unroll
        for (int u = 0; u < kAttribFinishBatch; ++u)
#pragma unroll
            for (int k = 0; k < NS; ++k) v[u][k] = p[(size_t)(c + u) * NS + k];
#pragma unroll
        for (int u = 0; u < kAttribFinishBatch; ++u)
#pragma unroll
            for (int k = 0; k < NS; ++k) s[k] += v[u][k];
    }
    for (; c < chunks; ++c) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] += p[(size_t)c * NS + k];
    }
    if (out_m0) out_m0[t] = s[0];
    double* o = out_x + (size_t)t * DIM;
    if (!var) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) o[c] = s[1 + c];
        return;
    }
    const double v = var[t];
    const bool ok = v == v && s[0] != 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) o[c] = ok ? W.wa[c] * s[1 + c] / s[0] : __builtin_nan("");
}

}  // namespace cvq
