// cvq_gas_kernels.h -- score-driven (GAS) time-varying copula: the batched log-likelihood and the
// filtered parameter path of the recursion (DESIGN.md §4 "Score-driven copula")
//     f_0 = omega / (1 - beta),  theta_t = link(f_t),  l_t = log c(u_t; theta_t),
//     s_t = d l_t / d f,  f_{t+1} = clamp(omega + beta f_t + alpha s_t, -40, 40).
// The recursion is sequential in t and independent between candidates (omega, alpha, beta): one
// thread per candidate, every lane reading the same row (a wave-uniform address), a plain sum in
// row order.  The score is exact: each log-density is written once over a scalar type T and
// instantiated on Dual, a forward-mode (value, d/df) pair, so no family's derivative is derived
// by hand and none is a finite difference.  Everything of a row that does not depend on f -- the
// Gaussian / Student quantiles, the Gumbel and Joe logarithms, the Student margins' term -- is
// computed once per call by k_gas_prep into kGasW(DIM) doubles per row.
// -ffp-contract=off: no FMA is written here, so none is emitted.
#pragma once
#include "cvq_common.h"

namespace cvq {
namespace gas {

constexpr double kFClamp = 40.0;
// kernel kinds (the two rotations share their family's instances: only k_gas_prep reads the flag)
constexpr int kGauss = 0, kStudent = 1, kPlackett = 2, kGumbel = 3, kFrank = 4, kJoe = 5;
__host__ __device__ constexpr int kGasW(int dim) { return 2 * dim; }

// ---------------------------------------------------------------- forward-mode dual numbers
struct Dual {
    double v, d;
};
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator+(Dual a, double b) { return {a.v + b, a.d}; }
__device__ __forceinline__ Dual operator+(double a, Dual b) { return {a + b.v, b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, double b) { return {a.v - b, a.d}; }
__device__ __forceinline__ Dual operator-(double a, Dual b) { return {a - b.v, -b.d}; }
__device__ __forceinline__ Dual operator-(Dual a) { return {-a.v, -a.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, double b) { return {a.v * b, a.d * b}; }
__device__ __forceinline__ Dual operator*(double a, Dual b) { return {a * b.v, a * b.d}; }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) {
    const double q = a.v / b.v;
    return {q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Dual operator/(Dual a, double b) { return {a.v / b, a.d / b}; }
__device__ __forceinline__ Dual operator/(double a, Dual b) {
    const double q = a / b.v;
    return {q, -(q * b.d) / b.v};
}
__device__ __forceinline__ Dual xlog(Dual a) { return {log(a.v), a.d / a.v}; }
__device__ __forceinline__ Dual xexp(Dual a) {
    const double e = exp(a.v);
    return {e, e * a.d};
}
__device__ __forceinline__ Dual xlog1p(Dual a) { return {log1p(a.v), a.d / (1.0 + a.v)}; }
__device__ __forceinline__ Dual xexpm1(Dual a) { return {expm1(a.v), exp(a.v) * a.d}; }
__device__ __forceinline__ double val(Dual a) { return a.v; }

__device__ __forceinline__ double xlog(double a) { return log(a); }
__device__ __forceinline__ double xexp(double a) { return exp(a); }
__device__ __forceinline__ double xlog1p(double a) { return log1p(a); }
__device__ __forceinline__ double xexpm1(double a) { return expm1(a); }
__device__ __forceinline__ double val(double a) { return a; }

// log(1 - e^-y), y > 0 (copulas._log1mexp)
template <class T>
__device__ __forceinline__ T log1mexp(T y) {
    if (val(y) > 0.6931471805599453) return xlog1p(-xexp(-y));
    return xlog(-xexpm1(-y));
}

// ---------------------------------------------------------------- links
// sigma(f) = 1 / (1 + e^-f); the correlation link 0.99 (2 sigma - 1) = 0.99 (1 - e^-f) / (1 + e^-f)
// is taken in that second form, which does not cancel near f = 0.
template <int KIND, class T>
__device__ __forceinline__ T link(T f) {
    const T e = xexp(-f);
    if (KIND == kGauss || KIND == kStudent) return 0.99 * (-xexpm1(-f) / (1.0 + e));
    const T sg = 1.0 / (1.0 + e);
    if (KIND == kPlackett) return 0.1 * xexp((4.0 * 2.302585092994046) * sg);      // 0.1 * 10^(4 sigma)
    if (KIND == kFrank) return 1e-3 + (32.0 - 1e-3) * sg;
    return 1.0001 + (16.0 - 1.0001) * sg;                                          // Gumbel, Joe
}

// ---------------------------------------------------------------- log densities
// w: the row's kGasW(DIM) prepared values (k_gas_prep); th: the copula parameter.

// product-form Archimedean tail shared by Frank and Joe (copulas._product_form_log_density)
template <int DIM, class T>
__device__ __forceinline__ T product_form(const T* a, const T* B, T p0, T q0, T kappa, T c2, T c3, T lc) {
    T S = a[0] + a[1], sB = B[0] + B[1];
    if (DIM == 3) { S = S + a[2]; sB = sB + B[2]; }
    const T om = q0 - p0 * xexpm1(-S);
    const T p = p0 * xexp(-S);
    const T poly = DIM == 2 ? om + c2 * p : om * om + p * (c2 * om + c3 * p);
    return sB + lc - S + (kappa - (double)DIM) * xlog(om) + xlog(poly);
}

template <int KIND, int DIM, class T>
__device__ __forceinline__ T log_density(const double* __restrict__ w, T th, double nu) {
    if (KIND == kGauss) {                     // w = (x, y): -log(1 - r^2)/2 - (r^2 (x^2 + y^2) - 2 r x y) / (2 (1 - r^2))
        const double x = w[0], y = w[1];
        const T om = 1.0 - th * th;
        return -0.5 * xlog(om) - (th * th * (x * x + y * y) - 2.0 * th * (x * y)) / (2.0 * om);
    }
    if (KIND == kStudent) {                   // w = (x, y, base): base = the constants and the margins' term
        const double x = w[0], y = w[1];
        const T om = 1.0 - th * th;
        const T q = ((x * x + y * y) - 2.0 * th * (x * y)) / om;
        return w[2] - 0.5 * xlog(om) - (0.5 * (nu + 2.0)) * xlog1p(q / nu);
    }
    if (KIND == kPlackett) {                  // w = (s, u + v, 1 - u - v), s = u + v - 2 u v  (Q11 formula)
        const T t1 = th - 1.0;
        const T num = th * (1.0 + t1 * w[0]);
        const T ab = (1.0 + t1 * w[1]) * (1.0 + t1 * w[2]);
        return xlog(num) - xlog(ab * ab);
    }
    if (KIND == kGumbel) {                    // w = (lx_0 .. lx_{d-1}, sum ell, sum lx), x = -ell
        T t[DIM];
        double m = -pos_inf();
#pragma unroll
        for (int i = 0; i < DIM; ++i) { t[i] = th * w[i]; m = val(t[i]) > m ? val(t[i]) : m; }
        T se = xexp(t[0] - m);
#pragma unroll
        for (int i = 1; i < DIM; ++i) se = se + xexp(t[i] - m);
        const T logA = (m + xlog(se)) / th;
        const T A = xexp(logA);
        const T t1 = th - 1.0;
        const T poly = DIM == 2 ? A + t1 : A * A + 3.0 * t1 * A + t1 * (2.0 * th - 1.0);
        return -A - w[DIM] + t1 * w[DIM + 1] + (1.0 - (double)DIM * th) * logA + xlog(poly);
    }
    if (KIND == kFrank) {                     // w = (u_0 .. u_{d-1})
        const T g = -xexpm1(-th), lg = log1mexp(th), eth = xexp(-th), lth = xlog(th);
        T a[DIM], B[DIM];
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
            const double u = w[i];
            const T X = eth * xexpm1(th * (1.0 - u)) / g;
            if (val(X) <= 0.5) a[i] = -xlog1p(-X);
            else a[i] = lg - log1mexp(th * u);
            B[i] = lth - th * u + a[i] - lg;
        }
        const T one = th * 0.0 + 1.0, zero = th * 0.0;
        return product_form<DIM, T>(a, B, g, eth, zero, DIM == 2 ? one : 3.0 * one, DIM == 2 ? zero : 2.0 * one,
                                    lg - lth);
    }
    {                                         // Joe: w = (l_0 .. l_{d-1}), l = log1p(-u) (survival: log u)
        const T lth = xlog(th);
        T a[DIM], B[DIM];
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
            a[i] = -log1mexp(-(th * w[i]));
            B[i] = lth + (th - 1.0) * w[i] + a[i];
        }
        const T kap = 1.0 / th, k = 1.0 - kap;
        const T one = th * 0.0 + 1.0, zero = th * 0.0;
        return product_form<DIM, T>(a, B, one, zero, kap, DIM == 2 ? k : 3.0 * k, DIM == 2 ? zero : k * (1.0 + k),
                                    -lth);
    }
}

// ---------------------------------------------------------------- per-row preparation
// One thread per row.  fam: the cvq.h copula code (the rotation of Gumbel / Joe is read here only).
template <int KIND, int DIM>
__global__ void k_gas_prep(TConst tk, double nu, double cst, int rotated, const double* __restrict__ u, long long N,
                           double* __restrict__ w) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    constexpr int W = kGasW(DIM);
    const double* ur = u + t * DIM;
    double* o = w + t * W;
#pragma unroll
    for (int j = 0; j < W; ++j) o[j] = 0.0;
    if (KIND == kGauss) {
        o[0] = ndtri(ur[0]);
        o[1] = ndtri(ur[1]);
    } else if (KIND == kStudent) {
        const double x = stdtrit(tk, ur[0]), y = stdtrit(tk, ur[1]);
        o[0] = x;
        o[1] = y;
        o[2] = cst + (0.5 * (nu + 1.0)) * (log1p(x * x / nu) + log1p(y * y / nu));
    } else if (KIND == kPlackett) {
        const double a = ur[0], b = ur[1];
        o[0] = a + b - 2.0 * a * b;
        o[1] = a + b;
        o[2] = 1.0 - a - b;
    } else if (KIND == kGumbel) {
        double se = 0.0, sl = 0.0;
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
            const double ell = rotated ? log1p(-ur[i]) : log(ur[i]);
            const double lx = log(-ell);
            o[i] = lx;
            se += ell;
            sl += lx;
        }
        o[DIM] = se;
        o[DIM + 1] = sl;
    } else if (KIND == kFrank) {
#pragma unroll
        for (int i = 0; i < DIM; ++i) o[i] = ur[i];
    } else {
#pragma unroll
        for (int i = 0; i < DIM; ++i) o[i] = rotated ? log(ur[i]) : log1p(-ur[i]);
    }
    // a margin that is not strictly inside (0, 1) poisons its row (device memory is not validated on the host)
    bool ok = true;
#pragma unroll
    for (int i = 0; i < DIM; ++i) ok = ok && (ur[i] > 0.0) && (ur[i] < 1.0);
    if (!ok) {
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = __builtin_nan("");
    }
}

// ---------------------------------------------------------------- the recursion
struct Cand {
    double omega, alpha, beta, f;
    bool ok;
};
__device__ __forceinline__ bool finite_d(double x) { return fabs(x) < pos_inf(); }   // false for NaN too

__device__ __forceinline__ Cand cand_init(const double* __restrict__ pr) {
    Cand c;
    c.omega = pr[0];
    c.alpha = pr[1];
    c.beta = pr[2];
    c.ok = finite_d(c.omega) && finite_d(c.alpha) && finite_d(c.beta) && fabs(c.beta) < 1.0;
    c.f = c.omega / (1.0 - c.beta);
    c.ok = c.ok && finite_d(c.f);                     // f_0 is not clamped: the clamp belongs to the update
    return c;
}

// One row: theta_t and l_t out, f advanced.  A non-finite f, s or l ends the candidate (ok = false).
template <int KIND, int DIM>
__device__ __forceinline__ void gas_step(Cand& c, const double* __restrict__ w, double nu, double* theta, double* ell) {
    const Dual th = link<KIND, Dual>(Dual{c.f, 1.0});
    const Dual L = log_density<KIND, DIM, Dual>(w, th, nu);
    *theta = th.v;
    *ell = L.v;
    double fn = c.omega + c.beta * c.f + c.alpha * L.d;
    c.ok = c.ok && finite_d(L.v) && finite_d(L.d) && finite_d(fn);
    fn = fn > kFClamp ? kFClamp : (fn < -kFClamp ? -kFClamp : fn);
    c.f = fn;
}

template <int KIND, int DIM>
__global__ void __launch_bounds__(64)
k_gas_loglik(const double* __restrict__ prm, long long B, const double* __restrict__ w, long long N, double nu,
             double* __restrict__ out) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    constexpr int W = kGasW(DIM);
    Cand c = cand_init(prm + 3 * b);
    double acc = 0.0;
    for (long long t = 0; t < N && c.ok; ++t) {
        double theta, ell;
        gas_step<KIND, DIM>(c, w + t * W, nu, &theta, &ell);
        acc += ell;
    }
    out[b] = c.ok ? acc : __builtin_nan("");
}

// One candidate, one thread: theta_out [N + 1], logc_out [N] or nullptr.  From the row whose l, s or
// next f is not finite on: logc NaN from that row, theta NaN from the next.
template <int KIND, int DIM>
__global__ void __launch_bounds__(64)
k_gas_path(const double* __restrict__ prm, const double* __restrict__ w, long long N, double nu,
           double* __restrict__ theta_out, double* __restrict__ logc_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    constexpr int W = kGasW(DIM);
    const double qnan = __builtin_nan("");
    Cand c = cand_init(prm);
    long long t = 0;
    for (; t < N && c.ok; ++t) {
        double theta, ell;
        gas_step<KIND, DIM>(c, w + t * W, nu, &theta, &ell);
        theta_out[t] = theta;
        if (logc_out) logc_out[t] = c.ok ? ell : qnan;
    }
    if (c.ok) {
        theta_out[N] = link<KIND, double>(c.f);
        return;
    }
    for (long long s = t; s <= N; ++s) theta_out[s] = qnan;
    if (logc_out)
        for (long long s = t; s < N; ++s) logc_out[s] = qnan;
}

}  // namespace gas
}  // namespace cvq
