// cvq_quantile.hip -- launch side of the exact quantile solve (own translation unit: its
// template instances compile in parallel with cvq_plan.hip and cvq_moments.hip).
#include <hip/hip_runtime.h>

#define CVQ_NO_PLAN_KERNELS
#define CVQ_NO_MOMENTS_FINISH

#include "cvq_quantile_kernels.h"

namespace cvq {
namespace {

struct QuantLaunch {
    const StaticDev& S;
    long long T;
    int L;                       // grid z: levels served by this pass (1: the opening pass)
    hipStream_t stream;
    const double* a;
    const double* pi;
    double* tA;
    double* tB;
    const double* st;            // nullptr: the opening pass's uniform edge and cuts (U)
    const double* cuts;
    QuantUniform U;
    double* part;
};

template <int COP, bool MSM>
void quant_tables(const QuantLaunch& L) {
    const long long total = L.T * L.S.dim * L.S.n;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (COP == CVQ_STUDENT && L.S.tk.q_c != nullptr)
        hipLaunchKernelGGL((k_moments_tables<COP, MSM, true>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.tA, L.tB);
    else
        hipLaunchKernelGGL((k_moments_tables<COP, MSM, false>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.tA, L.tB);
}

template <int COP, bool MSM, int DIM, int QT, int C>
void quant_q(const QuantLaunch& L) {
    const dim3 grid((unsigned)L.T, (unsigned)moments_chunks(DIM, L.S.nrows), (unsigned)L.L);
    hipLaunchKernelGGL((k_quant_pass<COP, MSM, DIM, QT, C>), grid, dim3(kMomNT), 0, L.stream, L.S, L.tA, L.tB, L.pi,
                       L.st, L.cuts, L.U, L.part);
}

template <int COP, bool MSM, int DIM, int C>
void quant_t(const QuantLaunch& L) {
    if constexpr (!MSM) {
        quant_q<COP, false, DIM, 1, C>(L);
    } else {
        switch (L.S.q) {
            case 1: quant_q<COP, true, DIM, 1, C>(L); break;
            case 2: quant_q<COP, true, DIM, 2, C>(L); break;
            case 3: quant_q<COP, true, DIM, 3, C>(L); break;
            case 4: quant_q<COP, true, DIM, 4, C>(L); break;
            case 5: quant_q<COP, true, DIM, 5, C>(L); break;
            case 6: quant_q<COP, true, DIM, 6, C>(L); break;
            case 7: quant_q<COP, true, DIM, 7, C>(L); break;
            default: quant_q<COP, true, DIM, 8, C>(L); break;
        }
    }
}

template <int COP, int C>
void quant_cop(const QuantLaunch& L) {
    const bool msm = L.S.model == CVQ_MSM;
    if (L.S.dim == 2) {
        if (msm) quant_t<COP, true, 2, C>(L); else quant_t<COP, false, 2, C>(L);
    } else if constexpr (COP != CVQ_PLACKETT) {
        if (msm) quant_t<COP, true, 3, C>(L); else quant_t<COP, false, 3, C>(L);
    }
}

template <int C>
void quant_pass(const QuantLaunch& L) {
    switch (L.S.copula) {
        case CVQ_GAUSSIAN: quant_cop<CVQ_GAUSSIAN, C>(L); break;
        case CVQ_STUDENT: quant_cop<CVQ_STUDENT, C>(L); break;
        case CVQ_PLACKETT: quant_cop<CVQ_PLACKETT, C>(L); break;
        case CVQ_GUMBEL: quant_cop<CVQ_GUMBEL, C>(L); break;
        case CVQ_PRODFORM: quant_cop<CVQ_PRODFORM, C>(L); break;
        default: break;                                // launch_quantiles rejects unknown kinds
    }
}

}  // namespace

// doubles of scratch per (date, level): partial sums of the widest pass, state, cuts
size_t quantile_scratch(int dim, int nrows) {
    return (size_t)moments_chunks(dim, nrows) * 2 * kQuantOpenCuts + kQuantState + kQuantCuts;
}

// Tables -> opening pass -> bracket test and the first steps -> ceil((K - 3) / 3) bisection passes
// with their updates -> closing pass -> finish, all in stream order.  tA / tB: scratch [T][dim][n]; work: scratch of
// T * L * quantile_scratch doubles; var_out / es_out / m0_out device [T][L] (the last two may be
// nullptr).  alpha: host [L].
int launch_quantiles(const StaticDev& S, long long T, hipStream_t stream, const double* a, const double* pi,
                     double* tA, double* tB, double* work, const double* alpha, int L, int K, double min_var,
                     double max_var, double lower, double ptf_mean, double* var_out, double* es_out, double* m0_out,
                     size_t abi) {
    CVQ_REQUIRE(abi == kernel_abi_key(), CVQ_ERR_STATE, "libcvq objects built from different headers (rebuild all)");
    CVQ_REQUIRE(S.n <= kMomMaxN && S.q <= kMaxQ && (S.dim == 2 || S.dim == 3), CVQ_ERR_UNSUPPORTED,
                "quantiles support n <= 1024, q <= 8, dim 2 or 3");
    CVQ_REQUIRE(!(S.copula == CVQ_PLACKETT && S.dim != 2), CVQ_ERR_UNSUPPORTED, "Plackett is 2-dimensional");
    const int chunks = moments_chunks(S.dim, S.nrows);
    CVQ_REQUIRE(chunks <= 65535, CVQ_ERR_UNSUPPORTED, "too many row chunks");
    CVQ_REQUIRE(L >= 1 && L <= kQuantMaxLevels, CVQ_ERR_INVALID, "n_levels must be in [1, 8]");
    QuantLevels lv{};
    for (int l = 0; l < L; ++l) lv.alpha[l] = alpha[l];
    const size_t TL = (size_t)T * L;
    double* part = work;
    double* st = part + TL * chunks * 2 * kQuantOpenCuts;
    double* cuts = st + TL * kQuantState;
    const dim3 ublocks((unsigned)((TL + 255) / 256));

    QuantUniform U{};                                 // min_var, the first three steps' mids, max_var
    U.a = lower;
    U.c[0] = min_var;
    quant_cuts(min_var, max_var, U.c + 1);
    U.c[kQuantOpenCuts - 1] = max_var;
    QuantLaunch Q{S, T, 1, stream, a, pi, tA, tB, nullptr, nullptr, U, part};
    const bool msm = S.model == CVQ_MSM;
    switch (S.copula) {
        case CVQ_GAUSSIAN: if (msm) quant_tables<CVQ_GAUSSIAN, true>(Q); else quant_tables<CVQ_GAUSSIAN, false>(Q); break;
        case CVQ_STUDENT: if (msm) quant_tables<CVQ_STUDENT, true>(Q); else quant_tables<CVQ_STUDENT, false>(Q); break;
        case CVQ_PLACKETT: if (msm) quant_tables<CVQ_PLACKETT, true>(Q); else quant_tables<CVQ_PLACKETT, false>(Q); break;
        case CVQ_GUMBEL: if (msm) quant_tables<CVQ_GUMBEL, true>(Q); else quant_tables<CVQ_GUMBEL, false>(Q); break;
        case CVQ_PRODFORM: if (msm) quant_tables<CVQ_PRODFORM, true>(Q); else quant_tables<CVQ_PRODFORM, false>(Q); break;
        default: CVQ_REQUIRE(false, CVQ_ERR_INVALID, "unknown copula kind");
    }
    CVQ_HIP_CHECK(hipGetLastError());
    int left = K;
    for (bool open = true; open || left > 0; open = false) {
        const int steps = left < 3 ? left : 3;
        if (open) quant_pass<kQuantOpenCuts>(Q); else quant_pass<kQuantCuts>(Q);
        CVQ_HIP_CHECK(hipGetLastError());
        left -= steps;
        hipLaunchKernelGGL(k_quant_update, ublocks, dim3(256), 0, stream, T, L, chunks, lv, open, U, steps, left == 0,
                           ptf_mean, part, st, cuts, var_out);
        CVQ_HIP_CHECK(hipGetLastError());
        Q.L = L;                                      // from here on a workgroup serves one level
        Q.st = st;
        Q.cuts = cuts;
    }

    if (es_out || m0_out) {
        quant_pass<2>(Q);
        CVQ_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_quant_finish, ublocks, dim3(256), 0, stream, T, L, chunks, ptf_mean, part, st, es_out,
                           m0_out);
        CVQ_HIP_CHECK(hipGetLastError());
    }
    return CVQ_OK;
}

}  // namespace cvq
