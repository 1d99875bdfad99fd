// cvq_quantile_kernels.h -- exact multi-level quantile solve (cvq_quantiles): a plain bisection
// of F(v) = mass of the slab (lower, v] on the nested-grid measure, without calc_var's quirks
// Q1-Q4, for up to CVQ_MAX_LEVELS levels per date.  No reference counterpart; membership, node
// values and Delta weights are the slab paths' own, F is cvq_slab_moments' m0.
//
// k_quant_pass is k_moments with C cut points per workgroup: same mapping (lane = row,
// wave-uniform columns, 2-D column split over the four waves, 3-D 256-row chunks), grid
// (dates x row chunks x levels).  A workgroup serves one (date, level): it takes the lower edge
// a and C ascending cuts c_1 < ... < c_C, evaluates every node of the union column range once and
// accumulates, per cut, the cumulative pair (sum v, sum level v) over (a, c_i] in registers.
// Partials go to part[t][level][chunk][cut][2]; k_quant_update (one thread per (date, level))
// sums a date's chunks in index order, forms F(c_i) = F(lo) + increment, descends the
// C = 2^s - 1 cuts by s binary decisions (the definition's rule F(mid) < alpha) and writes the
// next pass's state and cuts.  The cuts are the recursive (lo + hi) / 2 midpoints, so every
// decision point is bit for bit a sequential bisection's mid.  No atomics, no waiting between
// workgroups: fixed-order sums that depend on the date's own inputs alone.
//
// Schedule: opening pass (C = 9 from `lower`: min_var, the seven mids of the first three
// steps, max_var -- the same for every level, so one sweep over the tail serves them all)
// -> bracket test and the first three decisions -> ceil((K - 3) / 3) passes of C = 7 (three
// steps each, the last one the remaining K mod 3) -> closing pass (C = 2) over
// (lo, var - ptf_mean] for m0 and es.  The first three steps' cuts reach 7/8 of the way up the
// bracket: taken in a pass of their own they would sweep nearly the whole tail a second time.
#pragma once
#include "cvq_moments_kernels.h"

namespace cvq {

constexpr int kQuantMaxLevels = 8;             // CVQ_MAX_LEVELS
constexpr int kQuantCuts = 7;                  // cuts per bisection pass: three binary levels
constexpr int kQuantOpenCuts = kQuantCuts + 2; // the opening pass: min_var, the first seven mids, max_var
constexpr int kQuantState = 6;                 // doubles per (date, level): lo, hi, F(lo), M1(lo), live, F(hi0)

struct QuantLevels {
    double alpha[kQuantMaxLevels];
};

// The opening pass's lower edge and cuts (the same for every date and level).
struct QuantUniform {
    double a;
    double c[kQuantOpenCuts];
};

// st == nullptr: the opening pass, U's edge and first C cuts for every date (one level).
template <int COP, bool MSM, int DIM, int QT, int C>
__global__ __launch_bounds__(kMomNT) void k_quant_pass(StaticDev S, const double* __restrict__ tA,
                                                       const double* __restrict__ tB, const double* __restrict__ pi,
                                                       const double* __restrict__ st, const double* __restrict__ cuts,
                                                       QuantUniform U, double* __restrict__ part) {
    constexpr int CS = moments_colsplit(DIM);
    constexpr bool SKEW = C != kQuantOpenCuts;   // narrow passes: each lane walks its own columns
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

    // ---- membership, k_moments' rule per cut: columns (ka, kb[i]]; a NaN edge or cut compares
    // false with every node (a finished date's state is NaN: its workgroups fall through)
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
    // The loop below runs k over a wave-uniform range [j0, j1].  Opening pass: k is the column
    // itself over the chunk's union range [min ka + 1, max kb] (every column operand
    // wave-uniform, as k_moments).  Bisection / closing passes (SKEW): a row holds a few columns
    // at most, but neighbouring rows' ranges are shifted by about a column each, so the union
    // is ~64 columns wide whatever the bracket; there k counts from each lane's own ka + 1 and
    // the range is the longest row's length (per-lane column operands, neighbouring addresses).
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

// A date's chunks of one cut summed in index order.
__device__ inline void quant_sum(const double* p, int chunks, int C, int cut, double* s0, double* s1) {
    double a0 = p[2 * cut], a1 = p[2 * cut + 1];
    for (int k = 1; k < chunks; ++k) {
        a0 += p[(size_t)k * 2 * C + 2 * cut];
        a1 += p[(size_t)k * 2 * C + 2 * cut + 1];
    }
    *s0 = a0;
    *s1 = a1;
}

// The next pass's cuts: the three binary levels of (lo + hi) / 2 midpoints under (lo, hi), in
// ascending order (index 3 is the first mid, 1 / 5 the second level, the even ones the third).
__host__ __device__ inline void quant_cuts(double lo, double hi, double* c) {
    c[3] = (lo + hi) / 2;
    c[1] = (lo + c[3]) / 2;
    c[5] = (c[3] + hi) / 2;
    c[0] = (lo + c[1]) / 2;
    c[2] = (c[1] + c[3]) / 2;
    c[4] = (c[3] + c[5]) / 2;
    c[6] = (c[5] + hi) / 2;
}

// After a pass, one thread per (date, level): `steps` (0-3) binary decisions on the stored
// F(c_i) = F(lo) + increment_i, each the definition's "lo = mid if F(mid) < alpha else hi = mid"
// (never "first cut with F >= alpha": rounding may leave F non-monotone in the last ulp).
//   open: after the opening pass (part [T][1][chunks][9][2], shared by the levels, sums from
//     `lower`): first the bracket test F(min_var) < alpha <= F(max_var); a date outside it gets a
//     NaN state (its later workgroups find empty slabs) and keeps F(max_var);
//   else: after a bisection pass (part [T][L][chunks][7][2], sums from the state's lo).
//   last: write var and the closing pass's cut var - ptf_mean instead of the next cuts.
__global__ __launch_bounds__(256) void k_quant_update(long long T, int L, int chunks, QuantLevels lv, bool open,
                                                      QuantUniform U, int steps, bool last, double ptf_mean,
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
    const double var = (lo + hi) / 2 + ptf_mean;      // NaN outside the bracket
    var_out[idx] = var;
    c[0] = c[1] = var - ptf_mean;                     // cvq_expected_shortfall's upper edge
}

// After the closing pass (part [T][L][chunks][2][2] over (lo, var - ptf_mean]): m0 and
// es = m1 / m0 + ptf_mean as cvq_expected_shortfall forms them; outside the bracket es = NaN and
// m0 = F(max_var).
__global__ __launch_bounds__(256) void k_quant_finish(long long T, int L, int chunks, double ptf_mean,
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
        if (m0 != 0.0) es = m1 / m0 + ptf_mean;
    }
    if (es_out) es_out[idx] = es;
    if (m0_out) m0_out[idx] = m0;
}

}  // namespace cvq
