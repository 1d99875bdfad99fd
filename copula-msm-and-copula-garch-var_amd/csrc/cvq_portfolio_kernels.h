// cvq_portfolio_kernels.h -- exact quantiles for a batch of portfolio weights
// (cvq_portfolio_quantiles): cvq_quantiles' bisection of F(v) = mass of the slab (lower, v] for P
// weight vectors x L levels per date on one plan.  No reference counterpart.
//
// Nothing of the measure depends on the weights: the marginal tables, the row context, the q^3
// row-weight contraction G[] and node_value never read them.  Only the membership (row_level,
// inner_coord) and the level factor of the first moment do.  So the tables are built once per
// call, and a workgroup takes its portfolio's record (w0, w1, w2, w0_inv) from a device array
// [P][4] into a local StaticDev copy, on which the slab paths' own helpers run unchanged: the
// same expressions in the same order as a plan created with those weights, bit for bit.
//
// k_port_pass is k_quant_pass (same mapping, same partial layout per (date, portfolio, level),
// same fixed-order reduction) with grid z = portfolios (opening pass: its nine cuts are
// level-independent; in 3-D a workgroup serves a tile of portfolios and evaluates each node once
// for all of them) or portfolios x levels (the narrow passes, whose brackets differ per
// portfolio).  Partials, state and cuts are indexed (t P + p) L + l.  No atomics, no waiting
// between workgroups: a portfolio's result depends on its own record and its date's inputs alone.
#pragma once
// cvq_quantile_kernels.h defines its two plain (non-template) kernels in every unit that
// includes it.  This unit takes its helpers (quant_cuts, quant_sum), constants and structs only,
// so its copies of those two kernels get names of their own and cvq_quantile.hip keeps the
// originals.
#define k_quant_update k_quant_update_portfolio_unit
#define k_quant_finish k_quant_finish_portfolio_unit
#include "cvq_quantile_kernels.h"
#undef k_quant_update
#undef k_quant_finish

namespace cvq {

constexpr int kPortMax = 64;                   // CVQ_MAX_PORTFOLIOS
constexpr int kPortRec = 4;                    // doubles per weight record: w0, w1, w2, w0_inv

// The call's weight records and means, carried to the device array by k_port_setup's kernel
// argument (stream-ordered: no host buffer has to outlive the call).
struct PortRecords {
    double w[kPortMax][kPortRec];
    double mean[kPortMax];
};

__global__ __launch_bounds__(64) void k_port_setup(PortRecords R, int P, double* __restrict__ wrec,
                                                   double* __restrict__ mean) {
    const int p = threadIdx.x;
    if (p >= P) return;
#pragma unroll
    for (int i = 0; i < kPortRec; ++i) wrec[p * kPortRec + i] = R.w[p][i];
    mean[p] = R.mean[p];
}

// Lz: levels served by this pass (1: the opening pass, st == nullptr, U's edge and first C cuts
// for every date and portfolio).  PT = 1: grid z = P * Lz, one portfolio per workgroup.
// PT > 1 (3-D opening pass only): a workgroup serves the tile of PT portfolios from
// blockIdx.z * PT on one (date, row chunk), grid z = ceil(P / PT).  In 3-D there is no column
// split and a lane adds its own member nodes in ascending column order wherever the wave-uniform
// loop starts, so every node of the tile's union range is evaluated once and each slot's sums
// are those of its own workgroup at PT = 1, bit for bit.  Slots past P take the empty range.
template <int COP, bool MSM, int DIM, int QT, int C, int PT>
__global__ __launch_bounds__(kMomNT) void k_port_pass(StaticDev S0, const double* __restrict__ tA,
                                                      const double* __restrict__ tB, const double* __restrict__ pi,
                                                      const double* __restrict__ wrec, int P, int Lz,
                                                      const double* __restrict__ st, const double* __restrict__ cuts,
                                                      QuantUniform U, double* __restrict__ part) {
    constexpr int CS = moments_colsplit(DIM);
    constexpr bool SKEW = C != kQuantOpenCuts;   // narrow passes: each lane walks its own columns
    static_assert(PT == 1 || (DIM == 3 && !SKEW), "portfolio tiles: the 3-D opening pass only");
    __shared__ double sx[kMomMaxN];
    __shared__ double red[kMomWaves][2 * C * PT];
    const StaticDev& S = S0;
    const int n = S.n, q = QT;
    for (int j = threadIdx.x; j < n; j += kMomNT) sx[j] = S.x[j];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long t = blockIdx.x;
    const int p0 = PT == 1 ? (int)blockIdx.z / Lz : (int)blockIdx.z * PT;     // first portfolio served
    // PT == 1: (t P + p) Lz + l; a tile: (t P + p0), its slots follow
    const size_t tl = PT == 1 ? (size_t)t * gridDim.z + blockIdx.z : (size_t)t * P + p0;
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

    // ---- membership, k_quant_pass' rule per cut on each slot's weights: columns (ka, kb[i]].
    // The slot's record goes onto a copy of the plan's constants (wave-uniform loads), on which
    // the slab paths' own row_level / inner_coord run.
    double w0[PT], lev[PT];
    int ka[PT], kb[PT][C];
    int jlo = n, jhi = -1;
#pragma unroll
    for (int s = 0; s < PT; ++s) {
        const int p = min(p0 + s, P - 1);
        StaticDev Sp = S0;
        Sp.w0 = wrec[p * kPortRec];
        Sp.w1 = wrec[p * kPortRec + 1];
        Sp.w2 = wrec[p * kPortRec + 2];
        Sp.w0_inv = wrec[p * kPortRec + 3];
        w0[s] = Sp.w0;
        lev[s] = row_level(Sp, sx, rr_);
        int kbmax = 0;
        ka[s] = n;
#pragma unroll
        for (int i = 0; i < C; ++i) kb[s][i] = 0;
        if (live && a == a && p0 + s < P) {
            ka[s] = count_le(sx, inner_coord(Sp, a, lev[s]), 0, n - 1);
#pragma unroll
            for (int i = 0; i < C; ++i) {
                if (c[i] == c[i]) kb[s][i] = count_le(sx, inner_coord(Sp, c[i], lev[s]), 0, n - 1);
                kbmax = max(kbmax, kb[s][i]);
            }
        }
        // k's range, as k_quant_pass: the column itself over the chunk's union range (opening
        // pass), or the offset from each lane's own ka + 1 over the longest row's length (SKEW)
        if (kbmax > ka[s]) {
            jlo = min(jlo, SKEW ? 0 : ka[s] + 1);
            jhi = max(jhi, SKEW ? kbmax - ka[s] - 1 : kbmax);
        }
    }
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

    double m0[PT][C], m1[PT][C];
#pragma unroll
    for (int s = 0; s < PT; ++s)
#pragma unroll
        for (int i = 0; i < C; ++i) m0[s][i] = m1[s][i] = 0.0;
    if (j1 >= j0) {
        // ---- row weights G[b] (outer axes contracted with pi_t), as k_moments: weight-free
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
            const int jm = SKEW ? ka[0] + 1 + k : k;            // the column whose membership is tested
            const int j = SKEW ? min(jm, n - 1) : k;            // the column loaded (in the grid)
            double W = 0.0;
#pragma unroll
            for (int bb = 0; bb < QT; ++bb) W = fma(G[bb], Fc[(size_t)bb * n + j], W);
            const double v = node_value<COP, MSM, DIM>(S, ctx, Ac[j], Bc[j], W);
#pragma unroll
            for (int s = 0; s < PT; ++s) {
                const double lv = (lev[s] + w0[s] * sx[j]) * v;
                if (jm > ka[s]) {
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        if (jm <= kb[s][i]) {
                            m0[s][i] += v;
                            m1[s][i] += lv;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < PT; ++s)
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const double s0 = wave_sum(m0[s][i]), s1 = wave_sum(m1[s][i]);
            if (lane == 0) { red[wave][(s * C + i) * 2] = s0; red[wave][(s * C + i) * 2 + 1] = s1; }
        }
    __syncthreads();
    if (threadIdx.x < 2 * C * PT && p0 + (int)threadIdx.x / (2 * C) < P) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kMomWaves; ++w) s += red[w][threadIdx.x];
        const int slot = threadIdx.x / (2 * C), e = threadIdx.x % (2 * C);
        part[((tl + slot) * gridDim.y + blockIdx.y) * (2 * C) + e] = s;
    }
}

// k_quant_update per (date, portfolio, level): idx = (t P + p) L + l, the portfolio's own
// ptf_mean[p], var_out laid out [T][P][L].  open: the opening pass's partials are
// [T][P][chunks][9][2], shared by the levels of a (date, portfolio).
__global__ __launch_bounds__(256) void k_port_update(long long TP, int P, int L, int chunks, QuantLevels lv,
                                                     bool open, QuantUniform U, int steps, bool last,
                                                     const double* __restrict__ ptf_mean,
                                                     const double* __restrict__ part, double* __restrict__ st,
                                                     double* __restrict__ cuts, double* __restrict__ var_out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= TP * L) return;
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
    const double mean = ptf_mean[(idx / L) % P];
    const double var = (lo + hi) / 2 + mean;          // NaN outside the bracket
    var_out[idx] = var;
    c[0] = c[1] = var - mean;                         // the closing pass's upper edge
}

// k_quant_finish per (date, portfolio, level), outputs [T][P][L].
__global__ __launch_bounds__(256) void k_port_finish(long long TP, int P, int L, int chunks,
                                                     const double* __restrict__ ptf_mean,
                                                     const double* __restrict__ part, const double* __restrict__ st,
                                                     double* __restrict__ es_out, double* __restrict__ m0_out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= TP * L) return;
    const double* s = st + (size_t)idx * kQuantState;
    double m0 = s[5], es = __builtin_nan("");
    if (s[4] != 0.0) {
        double d0, d1;
        quant_sum(part + (size_t)idx * chunks * 4, chunks, 2, 0, &d0, &d1);
        m0 = s[2] + d0;
        const double m1 = s[3] + d1;
        if (m0 != 0.0) es = m1 / m0 + ptf_mean[(idx / L) % P];
    }
    if (es_out) es_out[idx] = es;
    if (m0_out) m0_out[idx] = m0;
}

}  // namespace cvq
