// cvq_gas.hip -- score-driven time-varying copula (cvq_gas_loglik, cvq_gas_path): validation,
// staging and launches of the kernels in cvq_gas_kernels.h.
#include <algorithm>
#include <cmath>
#include <string>

#include "cvq_gas_kernels.h"

using namespace cvq;
using namespace cvq::gas;

namespace {

struct GasBuf {
    double* p = nullptr;
    ~GasBuf() { if (p) (void)hipFree(p); }
};

struct GasKind {
    int kind;          // kGauss .. kJoe
    int rotated;       // survival Gumbel / survival Joe
};

// Everything that can be refused without a device.  On success *k names the kernel kind.
int gas_validate(int32_t copula, int32_t survival, int32_t dim, double nu, const double* u, int64_t N, int32_t mem,
                 GasKind* k) {
    CVQ_REQUIRE(dim == 2 || dim == 3, CVQ_ERR_INVALID, "dim must be 2 or 3");
    CVQ_REQUIRE(mem == CVQ_MEM_HOST || mem == CVQ_MEM_DEVICE, CVQ_ERR_INVALID, "mem must be CVQ_MEM_HOST or CVQ_MEM_DEVICE");
    int rot = 0;
    switch (copula) {
        case CVQ_GAUSSIAN: k->kind = kGauss; break;
        case CVQ_STUDENT: k->kind = kStudent; break;
        case CVQ_PLACKETT: k->kind = kPlackett; break;
        case CVQ_GUMBEL: k->kind = kGumbel; rot = survival != 0; break;
        case CVQ_GUMBEL_SURVIVAL: k->kind = kGumbel; rot = 1; break;
        case CVQ_FRANK: k->kind = kFrank; break;
        case CVQ_JOE: k->kind = kJoe; rot = survival != 0; break;
        case CVQ_JOE_SURVIVAL: k->kind = kJoe; rot = 1; break;
        default: CVQ_REQUIRE(false, CVQ_ERR_UNSUPPORTED, "unknown copula kind");
    }
    k->rotated = rot;
    CVQ_REQUIRE(dim == 2 || (k->kind != kGauss && k->kind != kStudent), CVQ_ERR_UNSUPPORTED,
                "the score-driven Gaussian / Student copula is built for 2 assets (one correlation)");
    CVQ_REQUIRE(dim == 2 || k->kind != kPlackett, CVQ_ERR_UNSUPPORTED, "Plackett copula is only defined for 2 assets");
    CVQ_REQUIRE(survival == 0 || k->kind == kGumbel || k->kind == kJoe, CVQ_ERR_INVALID,
                "the survival flag applies to the Gumbel and Joe kinds only");
    CVQ_REQUIRE(k->kind != kStudent || (std::isfinite(nu) && nu > 0.0), CVQ_ERR_INVALID, "Student nu must be finite and > 0");
    if (mem == CVQ_MEM_HOST) {
        for (int64_t t = 0; t < N; ++t)
            for (int i = 0; i < dim; ++i) {
                const double v = u[t * dim + i];
                if (!(v > 0.0 && v < 1.0)) {
                    set_error("u must lie strictly inside (0, 1) at row " + std::to_string((long long)t));
                    return CVQ_ERR_INVALID;
                }
            }
    }
    return CVQ_OK;
}

template <int KIND, int DIM>
void launch_prep(const TConst& tk, double nu, double cst, int rot, const double* u, long long N, double* w) {
    hipLaunchKernelGGL((k_gas_prep<KIND, DIM>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, tk, nu, cst, rot, u,
                       N, w);
}
template <int KIND, int DIM>
void launch_ll(const double* p, long long B, const double* w, long long N, double nu, double* out) {
    hipLaunchKernelGGL((k_gas_loglik<KIND, DIM>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, 0, p, B, w, N, nu, out);
}
template <int KIND, int DIM>
void launch_path(const double* p, const double* w, long long N, double nu, double* th, double* lc) {
    hipLaunchKernelGGL((k_gas_path<KIND, DIM>), dim3(1), dim3(64), 0, 0, p, w, N, nu, th, lc);
}

#define GAS_DISPATCH(FN, ...)                                                           \
    do {                                                                                \
        switch (k.kind * 4 + dim) {                                                     \
            case kGauss * 4 + 2: FN<kGauss, 2>(__VA_ARGS__); break;                     \
            case kStudent * 4 + 2: FN<kStudent, 2>(__VA_ARGS__); break;                 \
            case kPlackett * 4 + 2: FN<kPlackett, 2>(__VA_ARGS__); break;               \
            case kGumbel * 4 + 2: FN<kGumbel, 2>(__VA_ARGS__); break;                   \
            case kGumbel * 4 + 3: FN<kGumbel, 3>(__VA_ARGS__); break;                   \
            case kFrank * 4 + 2: FN<kFrank, 2>(__VA_ARGS__); break;                     \
            case kFrank * 4 + 3: FN<kFrank, 3>(__VA_ARGS__); break;                     \
            case kJoe * 4 + 2: FN<kJoe, 2>(__VA_ARGS__); break;                         \
            default: FN<kJoe, 3>(__VA_ARGS__); break;                                   \
        }                                                                               \
    } while (0)

// u (host|device) -> the prepared rows w [N][kGasW(dim)] on the device
int gas_prepare(const GasKind& k, int dim, double nu, const double* u, int64_t N, int32_t mem, GasBuf& ubuf, GasBuf& cf,
                GasBuf& wbuf) {
    const double* d_u = u;
    if (mem != CVQ_MEM_DEVICE) {
        CVQ_HIP_CHECK(hipMalloc((void**)&ubuf.p, (size_t)N * dim * sizeof(double)));
        CVQ_HIP_CHECK(hipMemcpy(ubuf.p, u, (size_t)N * dim * sizeof(double), hipMemcpyHostToDevice));
        d_u = ubuf.p;
    }
    TConst tk{};
    double cst = 0.0;
    if (k.kind == kStudent) {
        int rc = make_tconst(nu, &tk, &cf.p);
        if (rc) return rc;
        cst = std::lgamma(0.5 * (nu + 2.0)) + std::lgamma(0.5 * nu) - 2.0 * std::lgamma(0.5 * (nu + 1.0));
    }
    CVQ_HIP_CHECK(hipMalloc((void**)&wbuf.p, (size_t)N * kGasW(dim) * sizeof(double)));
    GAS_DISPATCH(launch_prep, tk, nu, cst, k.rotated, d_u, (long long)N, wbuf.p);
    CVQ_HIP_CHECK(hipGetLastError());
    return CVQ_OK;
}

}  // namespace

extern "C" {

int32_t cvq_gas_loglik(int32_t device, int32_t copula, int32_t survival, int32_t dim, double nu, const double* params,
                       int64_t B, const double* u, int64_t N, double* ll_out, int32_t mem) {
    CVQ_REQUIRE(params && u && ll_out, CVQ_ERR_INVALID, "NULL argument");
    CVQ_REQUIRE(B >= 1 && N >= 1, CVQ_ERR_INVALID, "B and N must be >= 1");
    GasKind k{};
    int rc = gas_validate(copula, survival, dim, nu, u, N, mem, &k);
    if (rc) return rc;
    CVQ_DEVICE_SCOPE(device);
    GasBuf ubuf, cf, wbuf, pbuf, obuf;
    if ((rc = gas_prepare(k, dim, nu, u, N, mem, ubuf, cf, wbuf))) return rc;
    CVQ_HIP_CHECK(hipMalloc((void**)&pbuf.p, (size_t)B * 3 * sizeof(double)));
    CVQ_HIP_CHECK(hipMemcpy(pbuf.p, params, (size_t)B * 3 * sizeof(double), hipMemcpyHostToDevice));
    double* d_out = ll_out;
    if (mem != CVQ_MEM_DEVICE) {
        CVQ_HIP_CHECK(hipMalloc((void**)&obuf.p, (size_t)B * sizeof(double)));
        d_out = obuf.p;
    }
    GAS_DISPATCH(launch_ll, pbuf.p, (long long)B, wbuf.p, (long long)N, nu, d_out);
    CVQ_HIP_CHECK(hipGetLastError());
    CVQ_HIP_CHECK(hipDeviceSynchronize());               // the scratch above is freed on return
    if (mem != CVQ_MEM_DEVICE) CVQ_HIP_CHECK(hipMemcpy(ll_out, obuf.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost));
    return CVQ_OK;
}

int32_t cvq_gas_path(int32_t device, int32_t copula, int32_t survival, int32_t dim, double nu, const double* params,
                     const double* u, int64_t N, double* theta_out, double* logc_out, int32_t mem) {
    CVQ_REQUIRE(params && u && theta_out, CVQ_ERR_INVALID, "NULL argument");
    CVQ_REQUIRE(N >= 1, CVQ_ERR_INVALID, "N must be >= 1");
    GasKind k{};
    int rc = gas_validate(copula, survival, dim, nu, u, N, mem, &k);
    if (rc) return rc;
    CVQ_DEVICE_SCOPE(device);
    GasBuf ubuf, cf, wbuf, pbuf, tbuf, lbuf;
    if ((rc = gas_prepare(k, dim, nu, u, N, mem, ubuf, cf, wbuf))) return rc;
    CVQ_HIP_CHECK(hipMalloc((void**)&pbuf.p, 3 * sizeof(double)));
    CVQ_HIP_CHECK(hipMemcpy(pbuf.p, params, 3 * sizeof(double), hipMemcpyHostToDevice));
    double *d_th = theta_out, *d_lc = logc_out;
    if (mem != CVQ_MEM_DEVICE) {
        CVQ_HIP_CHECK(hipMalloc((void**)&tbuf.p, (size_t)(N + 1) * sizeof(double)));
        d_th = tbuf.p;
        if (logc_out) {
            CVQ_HIP_CHECK(hipMalloc((void**)&lbuf.p, (size_t)N * sizeof(double)));
            d_lc = lbuf.p;
        }
    }
    GAS_DISPATCH(launch_path, pbuf.p, wbuf.p, (long long)N, nu, d_th, d_lc);
    CVQ_HIP_CHECK(hipGetLastError());
    CVQ_HIP_CHECK(hipDeviceSynchronize());
    if (mem != CVQ_MEM_DEVICE) {
        CVQ_HIP_CHECK(hipMemcpy(theta_out, tbuf.p, (size_t)(N + 1) * sizeof(double), hipMemcpyDeviceToHost));
        if (logc_out) CVQ_HIP_CHECK(hipMemcpy(logc_out, lbuf.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    }
    return CVQ_OK;
}

}  // extern "C"
