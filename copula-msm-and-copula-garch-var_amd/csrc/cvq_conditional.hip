// cvq_conditional.hip -- launch side of the conditional quantiles (own translation unit: its
// template instances compile in parallel with cvq_plan.hip, cvq_moments.hip, cvq_quantile.hip
// and cvq_attrib.hip).
#include <hip/hip_runtime.h>

#include <limits>

#define CVQ_NO_PLAN_KERNELS
#define CVQ_NO_MOMENTS_FINISH

#include "cvq_conditional_kernels.h"

namespace cvq {
namespace {

struct CondLaunch {
    const StaticDev& S;
    long long T;
    int L;                       // grid z: levels served by this pass (1: the opening pass)
    hipStream_t stream;
    const double* a;
    const double* pi;
    double* tA;
    double* tB;
    const double* st;            // nullptr: the uniform edge and cuts (U)
    const double* cuts;
    CondUniform U;
    int axis;
    const double* cond;          // device [T][2]
    double* part;
};

template <int COP, bool MSM>
void cond_tables(const CondLaunch& L) {
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
void cond_q(const CondLaunch& L) {
    const dim3 grid((unsigned)L.T, (unsigned)moments_chunks(DIM, L.S.nrows), (unsigned)L.L);
    hipLaunchKernelGGL((k_cond_pass<COP, MSM, DIM, QT, C>), grid, dim3(kMomNT), 0, L.stream, L.S, L.tA, L.tB, L.pi,
                       L.st, L.cuts, L.U, L.axis, L.cond, L.part);
}

template <int COP, bool MSM, int DIM, int C>
void cond_t(const CondLaunch& L) {
    if constexpr (!MSM) {
        cond_q<COP, false, DIM, 1, C>(L);
    } else {
        switch (L.S.q) {
            case 1: cond_q<COP, true, DIM, 1, C>(L); break;
            case 2: cond_q<COP, true, DIM, 2, C>(L); break;
            case 3: cond_q<COP, true, DIM, 3, C>(L); break;
            case 4: cond_q<COP, true, DIM, 4, C>(L); break;
            case 5: cond_q<COP, true, DIM, 5, C>(L); break;
            case 6: cond_q<COP, true, DIM, 6, C>(L); break;
            case 7: cond_q<COP, true, DIM, 7, C>(L); break;
            default: cond_q<COP, true, DIM, 8, C>(L); break;
        }
    }
}

template <int COP, int C>
void cond_cop(const CondLaunch& L) {
    const bool msm = L.S.model == CVQ_MSM;
    if (L.S.dim == 2) {
        if (msm) cond_t<COP, true, 2, C>(L); else cond_t<COP, false, 2, C>(L);
    } else if constexpr (COP != CVQ_PLACKETT) {
        if (msm) cond_t<COP, true, 3, C>(L); else cond_t<COP, false, 3, C>(L);
    }
}

template <int C>
void cond_pass(const CondLaunch& L) {
    switch (L.S.copula) {
        case CVQ_GAUSSIAN: cond_cop<CVQ_GAUSSIAN, C>(L); break;
        case CVQ_STUDENT: cond_cop<CVQ_STUDENT, C>(L); break;
        case CVQ_PLACKETT: cond_cop<CVQ_PLACKETT, C>(L); break;
        case CVQ_GUMBEL: cond_cop<CVQ_GUMBEL, C>(L); break;
        case CVQ_PRODFORM: cond_cop<CVQ_PRODFORM, C>(L); break;
        default: break;                                // launch_conditional rejects unknown kinds
    }
}

}  // namespace

// doubles of scratch per (date, level): partial sums of the widest pass, state, cuts
size_t conditional_scratch(int dim, int nrows) {
    return (size_t)moments_chunks(dim, nrows) * 2 * kCondOpenCuts + kCondState + kQuantCuts;
}

// Tables -> opening pass (with the +inf cut for p_E) -> bracket test on alpha p_E and the first steps ->
// ceil((K - 3) / 3) bisection passes with their updates -> closing pass -> finish, all in stream
// order.  tA / tB: scratch [T][dim][n]; work: scratch of T * L * conditional_scratch doubles;
// cond device [T][2]; var_out / es_out / m0_out device [T][L], pe_out device [T] (the last three
// may be nullptr).  alpha: host [L].
int launch_conditional(const StaticDev& S, long long T, hipStream_t stream, const double* a, const double* pi,
                       double* tA, double* tB, double* work, int axis, const double* cond, const double* alpha, int L,
                       int K, double min_var, double max_var, double lower, double ptf_mean, double* var_out,
                       double* es_out, double* m0_out, double* pe_out, size_t abi) {
    CVQ_REQUIRE(abi == kernel_abi_key(), CVQ_ERR_STATE, "libcvq objects built from different headers (rebuild all)");
    CVQ_REQUIRE(S.n <= kMomMaxN && S.q <= kMaxQ && (S.dim == 2 || S.dim == 3), CVQ_ERR_UNSUPPORTED,
                "conditional quantiles support n <= 1024, q <= 8, dim 2 or 3");
    CVQ_REQUIRE(!(S.copula == CVQ_PLACKETT && S.dim != 2), CVQ_ERR_UNSUPPORTED, "Plackett is 2-dimensional");
    CVQ_REQUIRE(axis >= 0 && axis < S.dim, CVQ_ERR_INVALID, "axis must be in [0, dim)");
    const int chunks = moments_chunks(S.dim, S.nrows);
    CVQ_REQUIRE(chunks <= 65535, CVQ_ERR_UNSUPPORTED, "too many row chunks");
    CVQ_REQUIRE(L >= 1 && L <= kQuantMaxLevels, CVQ_ERR_INVALID, "n_levels must be in [1, 8]");
    QuantLevels lv{};
    for (int l = 0; l < L; ++l) lv.alpha[l] = alpha[l];
    const size_t TL = (size_t)T * L;
    double* part = work;
    double* st = part + TL * chunks * 2 * kCondOpenCuts;
    double* cuts = st + TL * kCondState;
    const dim3 ublocks((unsigned)((TL + 255) / 256));

    CondUniform U{};                                  // min_var, the first three steps' mids, max_var, +inf (p_E)
    U.a = lower;
    U.c[0] = min_var;
    quant_cuts(min_var, max_var, U.c + 1);
    U.c[kQuantOpenCuts - 1] = max_var;
    U.c[kCondOpenCuts - 1] = std::numeric_limits<double>::infinity();
    CondLaunch Q{S, T, 1, stream, a, pi, tA, tB, nullptr, nullptr, U, axis, cond, part};
    const bool msm = S.model == CVQ_MSM;
    switch (S.copula) {
        case CVQ_GAUSSIAN: if (msm) cond_tables<CVQ_GAUSSIAN, true>(Q); else cond_tables<CVQ_GAUSSIAN, false>(Q); break;
        case CVQ_STUDENT: if (msm) cond_tables<CVQ_STUDENT, true>(Q); else cond_tables<CVQ_STUDENT, false>(Q); break;
        case CVQ_PLACKETT: if (msm) cond_tables<CVQ_PLACKETT, true>(Q); else cond_tables<CVQ_PLACKETT, false>(Q); break;
        case CVQ_GUMBEL: if (msm) cond_tables<CVQ_GUMBEL, true>(Q); else cond_tables<CVQ_GUMBEL, false>(Q); break;
        case CVQ_PRODFORM: if (msm) cond_tables<CVQ_PRODFORM, true>(Q); else cond_tables<CVQ_PRODFORM, false>(Q); break;
        default: CVQ_REQUIRE(false, CVQ_ERR_INVALID, "unknown copula kind");
    }
    CVQ_HIP_CHECK(hipGetLastError());
    int left = K;
    for (bool open = true; open || left > 0; open = false) {
        const int steps = left < 3 ? left : 3;
        if (open) cond_pass<kCondOpenCuts>(Q); else cond_pass<kQuantCuts>(Q);
        CVQ_HIP_CHECK(hipGetLastError());
        left -= steps;
        hipLaunchKernelGGL(k_cond_update, ublocks, dim3(256), 0, stream, T, L, chunks, lv, open, U, steps, left == 0,
                           ptf_mean, part, st, cuts, var_out, pe_out);
        CVQ_HIP_CHECK(hipGetLastError());
        Q.L = L;                                      // from here on a workgroup serves one level
        Q.st = st;
        Q.cuts = cuts;
    }

    if (es_out || m0_out) {
        cond_pass<2>(Q);
        CVQ_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_cond_finish, ublocks, dim3(256), 0, stream, T, L, chunks, ptf_mean, part, st, es_out,
                           m0_out);
        CVQ_HIP_CHECK(hipGetLastError());
    }
    return CVQ_OK;
}

}  // namespace cvq
