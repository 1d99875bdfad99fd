// cvq_dynamic_distribution.hip -- launch side of the per-date-record predictive distribution (own
// translation unit: its template instances compile in parallel with cvq_distribution.hip,
// cvq_dynamic.hip and the others).
#include <hip/hip_runtime.h>

#define CVQ_NO_PLAN_KERNELS
#define CVQ_NO_MOMENTS_FINISH

#include "cvq_dynamic_distribution_kernels.h"

namespace cvq {
namespace {

struct DynDistLaunch {
    const StaticDev& S;
    long long T;
    hipStream_t stream;
    const double* a;
    const double* pi;
    double* tA;
    double* tB;
    const double* rec;           // device [T][16]
    const double* edges;         // nullptr: U's ladder for every date
    DistEdges U;
    int nb, groups, per_group;
    double* part;
};

template <int COP, bool MSM>
void dyn_dist_tables(const DynDistLaunch& L) {
    const long long total = L.T * L.S.dim * L.S.n;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (COP == CVQ_STUDENT && L.S.tk.q_c != nullptr)
        hipLaunchKernelGGL((k_dyn_tables<COP, MSM, true>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.rec, L.tA, L.tB);
    else
        hipLaunchKernelGGL((k_dyn_tables<COP, MSM, false>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.rec, L.tA, L.tB);
}

template <int COP, bool MSM, int DIM, int QT>
void dyn_dist_q(const DynDistLaunch& L) {
    const dim3 grid((unsigned)L.T, (unsigned)moments_chunks(DIM, L.S.nrows), (unsigned)L.groups);
    hipLaunchKernelGGL((k_dyn_dist_pass<COP, MSM, DIM, QT>), grid, dim3(kMomNT), 0, L.stream, L.S, L.tA, L.tB, L.pi,
                       L.rec, L.edges, L.U, L.nb, L.per_group, L.part);
}

template <int COP, bool MSM, int DIM>
void dyn_dist_t(const DynDistLaunch& L) {
    if constexpr (!MSM) {
        dyn_dist_q<COP, false, DIM, 1>(L);
    } else {
        switch (L.S.q) {
            case 1: dyn_dist_q<COP, true, DIM, 1>(L); break;
            case 2: dyn_dist_q<COP, true, DIM, 2>(L); break;
            case 3: dyn_dist_q<COP, true, DIM, 3>(L); break;
            case 4: dyn_dist_q<COP, true, DIM, 4>(L); break;
            case 5: dyn_dist_q<COP, true, DIM, 5>(L); break;
            case 6: dyn_dist_q<COP, true, DIM, 6>(L); break;
            case 7: dyn_dist_q<COP, true, DIM, 7>(L); break;
            default: dyn_dist_q<COP, true, DIM, 8>(L); break;
        }
    }
}

template <int COP>
void dyn_dist_cop(const DynDistLaunch& L) {
    const bool msm = L.S.model == CVQ_MSM;
    if (msm) dyn_dist_tables<COP, true>(L); else dyn_dist_tables<COP, false>(L);
    if (L.S.dim == 2) {
        if (msm) dyn_dist_t<COP, true, 2>(L); else dyn_dist_t<COP, false, 2>(L);
    } else if constexpr (COP != CVQ_PLACKETT) {
        if (msm) dyn_dist_t<COP, true, 3>(L); else dyn_dist_t<COP, false, 3>(L);
    }
}

// Bin groups (grid z), cvq_distribution's rule: a small batch gets its parallelism from the bins.
// A bin's sums do not depend on the grouping, so the rule is free to look at T.
int dyn_dist_groups(long long T, int chunks, int nb) {
    constexpr long long kWantGroups = 1024;       // workgroups that fill the device about once
    const long long wgs = T * chunks;
    if (wgs >= kWantGroups) return 1;
    const long long g = (kWantGroups + wgs - 1) / wgs;
    return (int)(g < nb ? g : nb);
}

}  // namespace

// doubles at the head of a call's scratch: the date records [T][16] (dynamic_pack's layout)
size_t dynamic_distribution_upload_doubles(long long T) { return (size_t)T * kDynRec; }

// doubles of scratch of one call: the records, then the partial sums of every (date, chunk, bin)
size_t dynamic_distribution_scratch(int dim, int nrows, long long T, int nb) {
    return dynamic_distribution_upload_doubles(T) + (size_t)T * moments_chunks(dim, nrows) * nb * 2;
}

// Tables (the date's theta where they depend on it) -> per-chunk partial pairs of every bin ->
// per-(date, bin) sums, in stream order.  tA / tB: scratch [T][dim][n]; work:
// dynamic_distribution_scratch doubles whose head already holds the records [T][16] (uploaded by
// the caller in stream order); edges: device [T][nb + 1], or nullptr and shared: host [nb + 1];
// mass_out / m1_out device [T][nb] (the last may be nullptr).  The caller has passed
// distribution_check.
int launch_dynamic_distribution(const StaticDev& S, long long T, hipStream_t stream, const double* a,
                                const double* pi, double* tA, double* tB, double* work, const double* edges,
                                const double* shared, int nb, double* mass_out, double* m1_out, size_t abi) {
    CVQ_REQUIRE(abi == kernel_abi_key(), CVQ_ERR_STATE, "libcvq objects built from different headers (rebuild all)");
    CVQ_REQUIRE(S.n <= kMomMaxN && S.q <= kMaxQ && (S.dim == 2 || S.dim == 3), CVQ_ERR_UNSUPPORTED,
                "the distribution supports n <= 1024, q <= 8, dim 2 or 3");
    CVQ_REQUIRE(!(S.copula == CVQ_PLACKETT && S.dim != 2), CVQ_ERR_UNSUPPORTED, "Plackett is 2-dimensional");
    const int chunks = moments_chunks(S.dim, S.nrows);
    CVQ_REQUIRE(chunks <= 65535, CVQ_ERR_UNSUPPORTED, "too many row chunks");
    CVQ_REQUIRE(nb >= 1 && nb <= kDistMaxBins, CVQ_ERR_INVALID, "n_bins must be in [1, 64]");
    double* part = work + dynamic_distribution_upload_doubles(T);
    DynDistLaunch L{S, T, stream, a, pi, tA, tB, work, edges, DistEdges{}, nb, 1, nb, part};
    if (!edges)
        for (int b = 0; b <= nb; ++b) L.U.e[b] = shared[b];
    L.groups = dyn_dist_groups(T, chunks, nb);
    L.per_group = (nb + L.groups - 1) / L.groups;
    L.groups = (nb + L.per_group - 1) / L.per_group;          // no empty group
    switch (S.copula) {
        case CVQ_GAUSSIAN: dyn_dist_cop<CVQ_GAUSSIAN>(L); break;
        case CVQ_STUDENT: dyn_dist_cop<CVQ_STUDENT>(L); break;
        case CVQ_PLACKETT: dyn_dist_cop<CVQ_PLACKETT>(L); break;
        case CVQ_GUMBEL: dyn_dist_cop<CVQ_GUMBEL>(L); break;
        case CVQ_PRODFORM: dyn_dist_cop<CVQ_PRODFORM>(L); break;
        default: CVQ_REQUIRE(false, CVQ_ERR_INVALID, "unknown copula kind");
    }
    CVQ_HIP_CHECK(hipGetLastError());
    const long long TB = T * nb;
    hipLaunchKernelGGL(k_dist_finish_dyndist_unit, dim3((unsigned)((TB + 255) / 256)), dim3(256), 0, stream, T, nb,
                       chunks, part, mass_out, m1_out);
    CVQ_HIP_CHECK(hipGetLastError());
    return CVQ_OK;
}

}  // namespace cvq
