// cvq_dynamic.hip -- launch side of the per-date-record quantiles (own translation unit: its
// template instances compile in parallel with cvq_plan.hip, cvq_moments.hip, cvq_quantile.hip,
// cvq_attrib.hip, cvq_conditional.hip and cvq_portfolio.hip).
#include <hip/hip_runtime.h>

#define CVQ_NO_PLAN_KERNELS
#define CVQ_NO_MOMENTS_FINISH

#include "cvq_dynamic_kernels.h"

namespace cvq {
namespace {

struct DynLaunch {
    const StaticDev& S;
    long long T;
    int L;                       // grid z: levels served by this pass (1: the opening pass)
    hipStream_t stream;
    const double* a;
    const double* pi;
    double* tA;
    double* tB;
    const double* rec;           // device [T][16]
    const double* st;            // nullptr: the opening pass's uniform edge and cuts (U)
    const double* cuts;
    QuantUniform U;
    double* part;
};

template <int COP, bool MSM>
void dyn_tables(const DynLaunch& L) {
    const long long total = L.T * L.S.dim * L.S.n;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (COP == CVQ_STUDENT && L.S.tk.q_c != nullptr)
        hipLaunchKernelGGL((k_dyn_tables<COP, MSM, true>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.rec, L.tA, L.tB);
    else
        hipLaunchKernelGGL((k_dyn_tables<COP, MSM, false>), dim3(blocks), dim3(256), 0, L.stream, L.S, L.T, L.a,
                           L.rec, L.tA, L.tB);
}

template <int COP, bool MSM, int DIM, int QT, int C>
void dyn_q(const DynLaunch& L) {
    const dim3 grid((unsigned)L.T, (unsigned)moments_chunks(DIM, L.S.nrows), (unsigned)L.L);
    hipLaunchKernelGGL((k_dyn_pass<COP, MSM, DIM, QT, C>), grid, dim3(kMomNT), 0, L.stream, L.S, L.tA, L.tB, L.pi,
                       L.rec, L.st, L.cuts, L.U, L.part);
}

template <int COP, bool MSM, int DIM, int C>
void dyn_t(const DynLaunch& L) {
    if constexpr (!MSM) {
        dyn_q<COP, false, DIM, 1, C>(L);
    } else {
        switch (L.S.q) {
            case 1: dyn_q<COP, true, DIM, 1, C>(L); break;
            case 2: dyn_q<COP, true, DIM, 2, C>(L); break;
            case 3: dyn_q<COP, true, DIM, 3, C>(L); break;
            case 4: dyn_q<COP, true, DIM, 4, C>(L); break;
            case 5: dyn_q<COP, true, DIM, 5, C>(L); break;
            case 6: dyn_q<COP, true, DIM, 6, C>(L); break;
            case 7: dyn_q<COP, true, DIM, 7, C>(L); break;
            default: dyn_q<COP, true, DIM, 8, C>(L); break;
        }
    }
}

template <int COP, int C>
void dyn_cop(const DynLaunch& L) {
    const bool msm = L.S.model == CVQ_MSM;
    if (L.S.dim == 2) {
        if (msm) dyn_t<COP, true, 2, C>(L); else dyn_t<COP, false, 2, C>(L);
    } else if constexpr (COP != CVQ_PLACKETT) {
        if (msm) dyn_t<COP, true, 3, C>(L); else dyn_t<COP, false, 3, C>(L);
    }
}

template <int C>
void dyn_pass(const DynLaunch& L) {
    switch (L.S.copula) {
        case CVQ_GAUSSIAN: dyn_cop<CVQ_GAUSSIAN, C>(L); break;
        case CVQ_STUDENT: dyn_cop<CVQ_STUDENT, C>(L); break;
        case CVQ_PLACKETT: dyn_cop<CVQ_PLACKETT, C>(L); break;
        case CVQ_GUMBEL: dyn_cop<CVQ_GUMBEL, C>(L); break;
        case CVQ_PRODFORM: dyn_cop<CVQ_PRODFORM, C>(L); break;
        default: break;                                // launch_dynamic rejects unknown kinds
    }
}

}  // namespace

// The head of a call's scratch, uploaded per call: the records [T][16], then the means [T].
size_t dynamic_upload_doubles(long long T) { return (size_t)T * (kDynRec + 1); }
size_t dynamic_mean_offset(long long T) { return (size_t)T * kDynRec; }

// Date t's record in recs [T][16]: theta, term1, Ri[9], w0, w1, w2, w0_inv, pad.  w: {w0, w1, w2, w0_inv}.
void dynamic_pack(double* recs, long long t, double theta, double term1, const double* Ri, const double* w) {
    double* rec = recs + (size_t)t * kDynRec;
    rec[kDynTheta] = theta;
    rec[kDynTerm1] = term1;
    for (int i = 0; i < 9; ++i) rec[kDynRi + i] = Ri[i];
    for (int i = 0; i < 3; ++i) rec[kDynW + i] = w[i];
    rec[kDynW0Inv] = w[3];
    rec[kDynRec - 1] = 0.0;
}

// doubles of scratch of one call: the date records and means, then per (date, level) the partial
// sums of the widest pass, state and cuts
size_t dynamic_scratch(int dim, int nrows, long long T, int L) {
    const size_t per = (size_t)moments_chunks(dim, nrows) * 2 * kQuantOpenCuts + kQuantState + kQuantCuts;
    return dynamic_upload_doubles(T) + (size_t)T * L * per;
}

// Tables -> opening pass (grid z = 1) -> bracket test and the first steps -> ceil((K - 3) / 3)
// bisection passes (grid z = L) with their updates -> closing pass -> finish, all in stream order.
// tA / tB: scratch [T][dim][n]; work: dynamic_scratch doubles whose head already holds the records
// [T][16] and the means [T] (uploaded by the caller in stream order); alpha host [L]; var_out /
// es_out / m0_out device [T][L] (the last two may be nullptr).
int launch_dynamic(const StaticDev& S, long long T, hipStream_t stream, const double* a, const double* pi,
                   double* tA, double* tB, double* work, const double* alpha, int L, int K, double min_var,
                   double max_var, double lower, double* var_out, double* es_out, double* m0_out, size_t abi) {
    CVQ_REQUIRE(abi == kernel_abi_key(), CVQ_ERR_STATE, "libcvq objects built from different headers (rebuild all)");
    CVQ_REQUIRE(S.n <= kMomMaxN && S.q <= kMaxQ && (S.dim == 2 || S.dim == 3), CVQ_ERR_UNSUPPORTED,
                "dynamic quantiles support n <= 1024, q <= 8, dim 2 or 3");
    CVQ_REQUIRE(!(S.copula == CVQ_PLACKETT && S.dim != 2), CVQ_ERR_UNSUPPORTED, "Plackett is 2-dimensional");
    const int chunks = moments_chunks(S.dim, S.nrows);
    CVQ_REQUIRE(chunks <= 65535, CVQ_ERR_UNSUPPORTED, "too many row chunks");
    CVQ_REQUIRE(L >= 1 && L <= kQuantMaxLevels, CVQ_ERR_INVALID, "n_levels must be in [1, 8]");
    QuantLevels lv{};
    for (int l = 0; l < L; ++l) lv.alpha[l] = alpha[l];
    const size_t TL = (size_t)T * L;
    const double* d_rec = work;
    const double* d_mean = d_rec + (size_t)T * kDynRec;
    double* part = work + dynamic_upload_doubles(T);
    double* st = part + TL * chunks * 2 * kQuantOpenCuts;
    double* cuts = st + TL * kQuantState;
    const dim3 ublocks((unsigned)((TL + 255) / 256));

    QuantUniform U{};                                 // min_var, the first three steps' mids, max_var
    U.a = lower;
    U.c[0] = min_var;
    quant_cuts(min_var, max_var, U.c + 1);
    U.c[kQuantOpenCuts - 1] = max_var;
    DynLaunch Q{S, T, 1, stream, a, pi, tA, tB, d_rec, nullptr, nullptr, U, part};
    const bool msm = S.model == CVQ_MSM;
    switch (S.copula) {
        case CVQ_GAUSSIAN: if (msm) dyn_tables<CVQ_GAUSSIAN, true>(Q); else dyn_tables<CVQ_GAUSSIAN, false>(Q); break;
        case CVQ_STUDENT: if (msm) dyn_tables<CVQ_STUDENT, true>(Q); else dyn_tables<CVQ_STUDENT, false>(Q); break;
        case CVQ_PLACKETT: if (msm) dyn_tables<CVQ_PLACKETT, true>(Q); else dyn_tables<CVQ_PLACKETT, false>(Q); break;
        case CVQ_GUMBEL: if (msm) dyn_tables<CVQ_GUMBEL, true>(Q); else dyn_tables<CVQ_GUMBEL, false>(Q); break;
        case CVQ_PRODFORM: if (msm) dyn_tables<CVQ_PRODFORM, true>(Q); else dyn_tables<CVQ_PRODFORM, false>(Q); break;
        default: CVQ_REQUIRE(false, CVQ_ERR_INVALID, "unknown copula kind");
    }
    CVQ_HIP_CHECK(hipGetLastError());
    int left = K;
    for (bool open = true; open || left > 0; open = false) {
        const int steps = left < 3 ? left : 3;
        if (open) dyn_pass<kQuantOpenCuts>(Q); else dyn_pass<kQuantCuts>(Q);
        CVQ_HIP_CHECK(hipGetLastError());
        left -= steps;
        hipLaunchKernelGGL(k_dyn_update, ublocks, dim3(256), 0, stream, T, L, chunks, lv, open, U, steps, left == 0,
                           d_mean, part, st, cuts, var_out);
        CVQ_HIP_CHECK(hipGetLastError());
        Q.L = L;                                      // from here on a workgroup serves one level
        Q.st = st;
        Q.cuts = cuts;
    }

    if (es_out || m0_out) {
        dyn_pass<2>(Q);
        CVQ_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_dyn_finish, ublocks, dim3(256), 0, stream, T, L, chunks, d_mean, part, st, es_out,
                           m0_out);
        CVQ_HIP_CHECK(hipGetLastError());
    }
    return CVQ_OK;
}

}  // namespace cvq
