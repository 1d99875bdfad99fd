// cvq_portfolio.hip -- launch side of the batched-weights quantiles (own translation unit: its
// template instances compile in parallel with cvq_plan.hip, cvq_moments.hip, cvq_quantile.hip,
// cvq_attrib.hip and cvq_conditional.hip).
#include <hip/hip_runtime.h>

#define CVQ_NO_PLAN_KERNELS
#define CVQ_NO_MOMENTS_FINISH

#include "cvq_portfolio_kernels.h"

namespace cvq {
namespace {

struct PortLaunch {
    const StaticDev& S;
    long long T;
    int P;
    int L;                       // levels served by this pass (1: the opening pass); grid z = P * L
    hipStream_t stream;
    const double* a;
    const double* pi;
    double* tA;
    double* tB;
    const double* wrec;          // device [P][4]
    const double* st;            // nullptr: the opening pass's uniform edge and cuts (U)
    const double* cuts;
    QuantUniform U;
    double* part;
};

template <int COP, bool MSM>
void port_tables(const PortLaunch& L) {
    const long long total = L.T * L.S.dim * L.S.n;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (COP == CVQ_STUDENT && L.S.tk.q_c != nullptr)
        hipLaunchKernelGGL((k_moments_tables<COP, MSM, true>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.tA, L.tB);
    else
        hipLaunchKernelGGL((k_moments_tables<COP, MSM, false>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.tA, L.tB);
}

// Portfolios per workgroup in the 3-D opening pass.  Measured on cfg 4 (2000 dates, P = 8, L = 1):
// 222.3 ms at 1, 178.4 ms at 2, 280.8 ms at 4 (232-256 VGPRs: one or two waves per SIMD); no
// width uses scratch memory (profiles/portfolios).
constexpr int kPortTile = 2;

template <int COP, bool MSM, int DIM, int QT, int C>
void port_q(const PortLaunch& L) {
    constexpr int PT = (DIM == 3 && C == kQuantOpenCuts) ? kPortTile : 1;
    const unsigned z = PT == 1 ? (unsigned)(L.P * L.L) : (unsigned)((L.P + PT - 1) / PT);
    const dim3 grid((unsigned)L.T, (unsigned)moments_chunks(DIM, L.S.nrows), z);
    hipLaunchKernelGGL((k_port_pass<COP, MSM, DIM, QT, C, PT>), grid, dim3(kMomNT), 0, L.stream, L.S, L.tA, L.tB,
                       L.pi, L.wrec, L.P, L.L, L.st, L.cuts, L.U, L.part);
}

template <int COP, bool MSM, int DIM, int C>
void port_t(const PortLaunch& L) {
    if constexpr (!MSM) {
        port_q<COP, false, DIM, 1, C>(L);
    } else {
        switch (L.S.q) {
            case 1: port_q<COP, true, DIM, 1, C>(L); break;
            case 2: port_q<COP, true, DIM, 2, C>(L); break;
            case 3: port_q<COP, true, DIM, 3, C>(L); break;
            case 4: port_q<COP, true, DIM, 4, C>(L); break;
            case 5: port_q<COP, true, DIM, 5, C>(L); break;
            case 6: port_q<COP, true, DIM, 6, C>(L); break;
            case 7: port_q<COP, true, DIM, 7, C>(L); break;
            default: port_q<COP, true, DIM, 8, C>(L); break;
        }
    }
}

template <int COP, int C>
void port_cop(const PortLaunch& L) {
    const bool msm = L.S.model == CVQ_MSM;
    if (L.S.dim == 2) {
        if (msm) port_t<COP, true, 2, C>(L); else port_t<COP, false, 2, C>(L);
    } else if constexpr (COP != CVQ_PLACKETT) {
        if (msm) port_t<COP, true, 3, C>(L); else port_t<COP, false, 3, C>(L);
    }
}

template <int C>
void port_pass(const PortLaunch& L) {
    switch (L.S.copula) {
        case CVQ_GAUSSIAN: port_cop<CVQ_GAUSSIAN, C>(L); break;
        case CVQ_STUDENT: port_cop<CVQ_STUDENT, C>(L); break;
        case CVQ_PLACKETT: port_cop<CVQ_PLACKETT, C>(L); break;
        case CVQ_GUMBEL: port_cop<CVQ_GUMBEL, C>(L); break;
        case CVQ_PRODFORM: port_cop<CVQ_PRODFORM, C>(L); break;
        default: break;                                // launch_portfolios rejects unknown kinds
    }
}

}  // namespace

// doubles of scratch of one call: per (date, portfolio, level) the partial sums of the widest
// pass, state and cuts; then the weight records and means
size_t portfolio_scratch(int dim, int nrows, long long T, int P, int L) {
    const size_t per = (size_t)moments_chunks(dim, nrows) * 2 * kQuantOpenCuts + kQuantState + kQuantCuts;
    return (size_t)T * P * L * per + (size_t)kPortMax * (kPortRec + 1);
}

// Records -> tables -> opening pass (grid z = P; 3-D: ceil(P / kPortTile)) -> bracket test and the first steps ->
// ceil((K - 3) / 3) bisection passes (grid z = P L) with their updates -> closing pass -> finish,
// all in stream order.  tA / tB: scratch [T][dim][n]; work: portfolio_scratch doubles; wrec host
// [P][4] (w0, w1, w2, w0_inv), mean host [P], alpha host [L]; var_out / es_out / m0_out device
// [T][P][L] (the last two may be nullptr).
int launch_portfolios(const StaticDev& S, long long T, hipStream_t stream, const double* a, const double* pi,
                      double* tA, double* tB, double* work, const double* wrec, const double* mean, int P,
                      const double* alpha, int L, int K, double min_var, double max_var, double lower,
                      double* var_out, double* es_out, double* m0_out, size_t abi) {
    CVQ_REQUIRE(abi == kernel_abi_key(), CVQ_ERR_STATE, "libcvq objects built from different headers (rebuild all)");
    CVQ_REQUIRE(S.n <= kMomMaxN && S.q <= kMaxQ && (S.dim == 2 || S.dim == 3), CVQ_ERR_UNSUPPORTED,
                "portfolio quantiles support n <= 1024, q <= 8, dim 2 or 3");
    CVQ_REQUIRE(!(S.copula == CVQ_PLACKETT && S.dim != 2), CVQ_ERR_UNSUPPORTED, "Plackett is 2-dimensional");
    const int chunks = moments_chunks(S.dim, S.nrows);
    CVQ_REQUIRE(chunks <= 65535, CVQ_ERR_UNSUPPORTED, "too many row chunks");
    CVQ_REQUIRE(L >= 1 && L <= kQuantMaxLevels, CVQ_ERR_INVALID, "n_levels must be in [1, 8]");
    CVQ_REQUIRE(P >= 1 && P <= kPortMax, CVQ_ERR_INVALID, "n_portfolios must be in [1, 64]");
    QuantLevels lv{};
    for (int l = 0; l < L; ++l) lv.alpha[l] = alpha[l];
    PortRecords R{};
    for (int p = 0; p < P; ++p) {
        for (int i = 0; i < kPortRec; ++i) R.w[p][i] = wrec[p * kPortRec + i];
        R.mean[p] = mean[p];
    }
    const long long TP = T * P;
    const size_t TPL = (size_t)TP * L;
    double* d_wrec = work;
    double* d_mean = d_wrec + kPortMax * kPortRec;
    double* part = d_mean + kPortMax;
    double* st = part + TPL * chunks * 2 * kQuantOpenCuts;
    double* cuts = st + TPL * kQuantState;
    const dim3 ublocks((unsigned)((TPL + 255) / 256));

    hipLaunchKernelGGL(k_port_setup, dim3(1), dim3(64), 0, stream, R, P, d_wrec, d_mean);
    CVQ_HIP_CHECK(hipGetLastError());
    QuantUniform U{};                                 // min_var, the first three steps' mids, max_var
    U.a = lower;
    U.c[0] = min_var;
    quant_cuts(min_var, max_var, U.c + 1);
    U.c[kQuantOpenCuts - 1] = max_var;
    PortLaunch Q{S, T, P, 1, stream, a, pi, tA, tB, d_wrec, nullptr, nullptr, U, part};
    const bool msm = S.model == CVQ_MSM;
    switch (S.copula) {
        case CVQ_GAUSSIAN: if (msm) port_tables<CVQ_GAUSSIAN, true>(Q); else port_tables<CVQ_GAUSSIAN, false>(Q); break;
        case CVQ_STUDENT: if (msm) port_tables<CVQ_STUDENT, true>(Q); else port_tables<CVQ_STUDENT, false>(Q); break;
        case CVQ_PLACKETT: if (msm) port_tables<CVQ_PLACKETT, true>(Q); else port_tables<CVQ_PLACKETT, false>(Q); break;
        case CVQ_GUMBEL: if (msm) port_tables<CVQ_GUMBEL, true>(Q); else port_tables<CVQ_GUMBEL, false>(Q); break;
        case CVQ_PRODFORM: if (msm) port_tables<CVQ_PRODFORM, true>(Q); else port_tables<CVQ_PRODFORM, false>(Q); break;
        default: CVQ_REQUIRE(false, CVQ_ERR_INVALID, "unknown copula kind");
    }
    CVQ_HIP_CHECK(hipGetLastError());
    int left = K;
    for (bool open = true; open || left > 0; open = false) {
        const int steps = left < 3 ? left : 3;
        if (open) port_pass<kQuantOpenCuts>(Q); else port_pass<kQuantCuts>(Q);
        CVQ_HIP_CHECK(hipGetLastError());
        left -= steps;
        hipLaunchKernelGGL(k_port_update, ublocks, dim3(256), 0, stream, TP, P, L, chunks, lv, open, U, steps,
                           left == 0, d_mean, part, st, cuts, var_out);
        CVQ_HIP_CHECK(hipGetLastError());
        Q.L = L;                                      // from here on a workgroup serves one level
        Q.st = st;
        Q.cuts = cuts;
    }

    if (es_out || m0_out) {
        port_pass<2>(Q);
        CVQ_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_port_finish, ublocks, dim3(256), 0, stream, TP, P, L, chunks, d_mean, part, st, es_out,
                           m0_out);
        CVQ_HIP_CHECK(hipGetLastError());
    }
    return CVQ_OK;
}

}  // namespace cvq
