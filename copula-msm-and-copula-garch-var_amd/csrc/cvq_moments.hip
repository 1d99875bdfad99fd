// cvq_moments.hip -- launch side of the tail-moment kernels (own translation unit: its
// template instances compile in parallel with cvq_plan.hip).
#include <hip/hip_runtime.h>

#define CVQ_NO_PLAN_KERNELS

#include "cvq_moments_kernels.h"

namespace cvq {
namespace {

struct MomentsLaunch {
    const StaticDev& S;
    long long T;
    hipStream_t stream;
    const double* a;
    const double* pi;
    double* tA;
    double* tB;
    const double* bounds;
    const double* var;
    double lower, ptf_mean;
    double* part;
};

template <int COP, bool MSM>
void moments_tables(const MomentsLaunch& L) {
    const long long total = L.T * L.S.dim * L.S.n;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (COP == CVQ_STUDENT && L.S.tk.q_c != nullptr)
        hipLaunchKernelGGL((k_moments_tables<COP, MSM, true>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.tA, L.tB);
    else
        hipLaunchKernelGGL((k_moments_tables<COP, MSM, false>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.tA, L.tB);
}

template <int COP, bool MSM, int DIM, int QT>
void moments_q(const MomentsLaunch& L) {
    const dim3 grid((unsigned)L.T, (unsigned)moments_chunks(DIM, L.S.nrows));
    hipLaunchKernelGGL((k_moments<COP, MSM, DIM, QT>), grid, dim3(kMomNT), 0, L.stream, L.S, L.tA, L.tB, L.pi,
                       L.bounds, L.var, L.lower, L.ptf_mean, L.part);
}

template <int COP, bool MSM, int DIM>
void moments_t(const MomentsLaunch& L) {
    if constexpr (!MSM) {
        moments_q<COP, false, DIM, 1>(L);
    } else {
        switch (L.S.q) {
            case 1: moments_q<COP, true, DIM, 1>(L); break;
            case 2: moments_q<COP, true, DIM, 2>(L); break;
            case 3: moments_q<COP, true, DIM, 3>(L); break;
            case 4: moments_q<COP, true, DIM, 4>(L); break;
            case 5: moments_q<COP, true, DIM, 5>(L); break;
            case 6: moments_q<COP, true, DIM, 6>(L); break;
            case 7: moments_q<COP, true, DIM, 7>(L); break;
            default: moments_q<COP, true, DIM, 8>(L); break;
        }
    }
}

template <int COP>
void moments_cop(const MomentsLaunch& L) {
    const bool msm = L.S.model == CVQ_MSM;
    if (msm) moments_tables<COP, true>(L); else moments_tables<COP, false>(L);
    if (L.S.dim == 2) {
        if (msm) moments_t<COP, true, 2>(L); else moments_t<COP, false, 2>(L);
    } else if constexpr (COP != CVQ_PLACKETT) {
        if (msm) moments_t<COP, true, 3>(L); else moments_t<COP, false, 3>(L);
    }
}

}  // namespace

int moments_chunk_count(int dim, int nrows) { return moments_chunks(dim, nrows); }

// Tables -> per-chunk partial moments -> per-date sums, in stream order.  tA / tB: scratch
// [T][dim][n] each; part: scratch [T][chunks][2].  bounds [T][2], or (var != nullptr) the slab
// (lower, var[t] - ptf_mean] and the Expected Shortfall in out1 (k_moments_finish).
int launch_moments(const StaticDev& S, long long T, hipStream_t stream, const double* a, const double* pi, double* tA,
                   double* tB, double* part, const double* bounds, const double* var, double lower, double ptf_mean,
                   double* out0, double* out1, size_t abi) {
    CVQ_REQUIRE(abi == kernel_abi_key(), CVQ_ERR_STATE, "libcvq objects built from different headers (rebuild all)");
    CVQ_REQUIRE(S.n <= kMomMaxN && S.q <= kMaxQ && (S.dim == 2 || S.dim == 3), CVQ_ERR_UNSUPPORTED,
                "tail moments support n <= 1024, q <= 8, dim 2 or 3");
    CVQ_REQUIRE(!(S.copula == CVQ_PLACKETT && S.dim != 2), CVQ_ERR_UNSUPPORTED, "Plackett is 2-dimensional");
    CVQ_REQUIRE(moments_chunks(S.dim, S.nrows) <= 65535, CVQ_ERR_UNSUPPORTED, "too many row chunks");
    const MomentsLaunch L{S, T, stream, a, pi, tA, tB, var ? nullptr : bounds, var, lower, ptf_mean, part};
    switch (S.copula) {
        case CVQ_GAUSSIAN: moments_cop<CVQ_GAUSSIAN>(L); break;
        case CVQ_STUDENT: moments_cop<CVQ_STUDENT>(L); break;
        case CVQ_PLACKETT: moments_cop<CVQ_PLACKETT>(L); break;
        case CVQ_GUMBEL: moments_cop<CVQ_GUMBEL>(L); break;
        case CVQ_PRODFORM: moments_cop<CVQ_PRODFORM>(L); break;
        default: CVQ_REQUIRE(false, CVQ_ERR_INVALID, "unknown copula kind");
    }
    CVQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_moments_finish, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, T,
                       moments_chunks(S.dim, S.nrows), part, var, ptf_mean, out0, out1);
    CVQ_HIP_CHECK(hipGetLastError());
    return CVQ_OK;
}

}  // namespace cvq
