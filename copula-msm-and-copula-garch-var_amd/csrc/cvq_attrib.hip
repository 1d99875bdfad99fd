// cvq_attrib.hip -- launch side of the per-axis moment kernels behind the risk contributions
// (own translation unit: its template instances compile in parallel with cvq_plan.hip,
// cvq_moments.hip and cvq_quantile.hip).
#include <hip/hip_runtime.h>

#define CVQ_NO_PLAN_KERNELS
#define CVQ_NO_MOMENTS_FINISH

#include "cvq_attrib_kernels.h"

namespace cvq {
namespace {

struct AttribLaunch {
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
void attrib_tables(const AttribLaunch& L) {
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
void attrib_q(const AttribLaunch& L) {
    const dim3 grid((unsigned)L.T, (unsigned)moments_chunks(DIM, L.S.nrows));
    hipLaunchKernelGGL((k_attrib<COP, MSM, DIM, QT>), grid, dim3(kMomNT), 0, L.stream, L.S, L.tA, L.tB, L.pi,
                       L.bounds, L.var, L.lower, L.ptf_mean, L.part);
}

template <int COP, bool MSM, int DIM>
void attrib_t(const AttribLaunch& L) {
    if constexpr (!MSM) {
        attrib_q<COP, false, DIM, 1>(L);
    } else {
        switch (L.S.q) {
            case 1: attrib_q<COP, true, DIM, 1>(L); break;
            case 2: attrib_q<COP, true, DIM, 2>(L); break;
            case 3: attrib_q<COP, true, DIM, 3>(L); break;
            case 4: attrib_q<COP, true, DIM, 4>(L); break;
            case 5: attrib_q<COP, true, DIM, 5>(L); break;
            case 6: attrib_q<COP, true, DIM, 6>(L); break;
            case 7: attrib_q<COP, true, DIM, 7>(L); break;
            default: attrib_q<COP, true, DIM, 8>(L); break;
        }
    }
}

template <int COP>
void attrib_cop(const AttribLaunch& L) {
    const bool msm = L.S.model == CVQ_MSM;
    if (msm) attrib_tables<COP, true>(L); else attrib_tables<COP, false>(L);
    if (L.S.dim == 2) {
        if (msm) attrib_t<COP, true, 2>(L); else attrib_t<COP, false, 2>(L);
    } else if constexpr (COP != CVQ_PLACKETT) {
        if (msm) attrib_t<COP, true, 3>(L); else attrib_t<COP, false, 3>(L);
    }
}

}  // namespace

// doubles of partial-sum scratch per date: [chunks][1 + dim]
size_t attrib_scratch(int dim, int nrows) { return (size_t)moments_chunks(dim, nrows) * (1 + dim); }

// Tables -> per-chunk partial sums -> per-date sums, in stream order.  tA / tB: scratch
// [T][dim][n] each (the moments' tables); part: scratch of T * attrib_scratch doubles.
// bounds [T][2]: out_m0 [T] = m0, out_x [T][dim] = mx; or (var != nullptr) the slab
// (lower, var[t] - ptf_mean] and the contributions in out_x, out_m0 may be nullptr
// (k_attrib_finish).
int launch_attrib(const StaticDev& S, long long T, hipStream_t stream, const double* a, const double* pi, double* tA,
                  double* tB, double* part, const double* bounds, const double* var, double lower, double ptf_mean,
                  double* out_m0, double* out_x, size_t abi) {
    CVQ_REQUIRE(abi == kernel_abi_key(), CVQ_ERR_STATE, "libcvq objects built from different headers (rebuild all)");
    CVQ_REQUIRE(S.n <= kMomMaxN && S.q <= kMaxQ && (S.dim == 2 || S.dim == 3), CVQ_ERR_UNSUPPORTED,
                "axis moments support n <= 1024, q <= 8, dim 2 or 3");
    CVQ_REQUIRE(!(S.copula == CVQ_PLACKETT && S.dim != 2), CVQ_ERR_UNSUPPORTED, "Plackett is 2-dimensional");
    CVQ_REQUIRE(moments_chunks(S.dim, S.nrows) <= 65535, CVQ_ERR_UNSUPPORTED, "too many row chunks");
    const AttribLaunch L{S, T, stream, a, pi, tA, tB, var ? nullptr : bounds, var, lower, ptf_mean, part};
    switch (S.copula) {
        case CVQ_GAUSSIAN: attrib_cop<CVQ_GAUSSIAN>(L); break;
        case CVQ_STUDENT: attrib_cop<CVQ_STUDENT>(L); break;
        case CVQ_PLACKETT: attrib_cop<CVQ_PLACKETT>(L); break;
        case CVQ_GUMBEL: attrib_cop<CVQ_GUMBEL>(L); break;
        case CVQ_PRODFORM: attrib_cop<CVQ_PRODFORM>(L); break;
        default: CVQ_REQUIRE(false, CVQ_ERR_INVALID, "unknown copula kind");
    }
    CVQ_HIP_CHECK(hipGetLastError());
    // the weight the membership rule gives each axis (Q10): the inner (last) axis takes w[0]
    AxisWeights W{};
    W.wa[0] = S.w1;
    W.wa[1] = S.dim == 3 ? S.w2 : S.w0;
    W.wa[2] = S.dim == 3 ? S.w0 : 0.0;
    const dim3 fgrid((unsigned)((T + 255) / 256));
    const int chunks = moments_chunks(S.dim, S.nrows);
    if (S.dim == 2)
        hipLaunchKernelGGL(k_attrib_finish<2>, fgrid, dim3(256), 0, stream, T, chunks, W, part, var, out_m0, out_x);
    else
        hipLaunchKernelGGL(k_attrib_finish<3>, fgrid, dim3(256), 0, stream, T, chunks, W, part, var, out_m0, out_x);
    CVQ_HIP_CHECK(hipGetLastError());
    return CVQ_OK;
}

}  // namespace cvq
