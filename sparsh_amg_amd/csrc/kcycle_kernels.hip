// kcycle_kernels.hip -- the K step of the K-cycle (Notay): two steps of flexible CG on a coarse level, each preconditioned by the
// cycle below.  Besides its two inner cycles and two SpMVs a K step issues six launches and never waits
// for the host:
//   kc_dot_kernel<2>    c.v and c.b, c read once
//   kc_scal1_kernel     rho1, alpha1, q and the first guard
//   kc_resid_kernel     r = b - q v
//   kc_dot_kernel<3>    d.v, d.w and d.r, d read once
//   kc_scal2_kernel     gamma, beta, alpha2, rho2, k1, k2 and the second guard
//   kc_combine_kernel   x = k1 c + k2 d
// The levels a K step runs on hold 10^3 .. 10^6 rows: 256-thread workgroups, one per 2048 rows and never more than kKcMaxGrid, so the
// smallest levels are one workgroup and a 10^6-row level is 489 of them with four 16-byte loads per thread and vector.  Reductions
// are per-thread sums in index order, a fixed wave / workgroup tree, then one workgroup that adds the per-workgroup partial sums in a
// fixed order: no floating-point atomics, bitwise reproducible run to run.  The file is built with -ffp-contract=off, so every
// product and sum of the two vector updates is rounded on its own, as in the Chebyshev step.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

#include <algorithm>

namespace sparsh {

namespace {

constexpr int kKcBlock = 256;

__device__ __forceinline__ double kc_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// NS sums over the workgroup, valid in thread 0; red holds NS * kKcBlock / 64 doubles
template <int NS>
__device__ __forceinline__ void kc_block_sum(double (&acc)[NS], double *red)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        acc[s] = kc_wave_sum(acc[s]);
        if (lane == 0) red[s * (kKcBlock / 64) + w] = acc[s];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < kKcBlock / 64; ++k) t += red[s * (kKcBlock / 64) + k];
            acc[s] = t;
        }
    }
}

// partial[s * kKcMaxGrid + workgroup] = sum over the workgroup's rows of a_i * y_s,i for s < NS.  A thread owns pairs of neighbouring
// rows (one 16-byte load per vector), pair index ascending; all vectors are 16-byte aligned.
template <int NS>
__global__ __launch_bounds__(kKcBlock) void kc_dot_kernel(int n, const double *__restrict__ a, const double *__restrict__ y0,
                                                           const double *__restrict__ y1, const double *__restrict__ y2,
                                                           double *__restrict__ partial)
{
    __shared__ double red[NS * (kKcBlock / 64)];
    const double *y[3] = {y0, y1, y2};
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    const long stride = 2L * kKcBlock * gridDim.x;
    for (long i = 2L * (blockIdx.x * kKcBlock + threadIdx.x); i < n; i += stride) {
        if (i + 1 < n) {
            const double2 av = *reinterpret_cast<const double2 *>(a + i);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double2 yv = *reinterpret_cast<const double2 *>(y[s] + i);
                acc[s] += av.x * yv.x;
                acc[s] += av.y * yv.y;
            }
        } else {
            const double av = a[i];
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] += av * y[s][i];
        }
    }
    kc_block_sum<NS>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) partial[s * kKcMaxGrid + blockIdx.x] = acc[s];
    }
}

// the NS sums of nblk <= kKcMaxGrid partials each: thread t adds partial[t], partial[t + 256], ... in that order, then the tree
template <int NS>
__device__ __forceinline__ void kc_total(const double *__restrict__ partial, int nblk, double (&sum)[NS], double *red)
{
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double t = 0.0;
        for (int k = threadIdx.x; k < nblk; k += kKcBlock) t += partial[s * kKcMaxGrid + k];
        sum[s] = t;
    }
    kc_block_sum<NS>(sum, red);
}

__device__ __forceinline__ bool kc_usable(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }  // finite and > 0 (false for a NaN)

// rho1 = c.v ; alpha1 = c.b ; q = alpha1 / rho1, or 1 when rho1 is not finite and > 0 (the step then becomes the W step)
__global__ __launch_bounds__(kKcBlock) void kc_scal1_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ s)
{
    __shared__ double red[2 * (kKcBlock / 64)];
    double sum[2];
    kc_total<2>(partial, nblk, sum, red);
    if (threadIdx.x != 0) return;
    const double rho1 = sum[0], alpha1 = sum[1];
    s[KC_RHO1] = rho1;
    s[KC_ALPHA1] = alpha1;
    s[KC_Q] = kc_usable(rho1) ? alpha1 / rho1 : 1.0;
}

// gamma = d.v ; beta = d.w ; alpha2 = d.r ; rho2 = beta - gamma^2 / rho1 ; k1 = q - gamma alpha2 / (rho1 rho2) ; k2 = alpha2 / rho2.
// rho1 unusable: rho2 = 0 (not formed), k1 = k2 = 1.  Otherwise rho2 unusable: k1 = q, k2 = 0.
__global__ __launch_bounds__(kKcBlock) void kc_scal2_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ s)
{
    __shared__ double red[3 * (kKcBlock / 64)];
    double sum[3];
    kc_total<3>(partial, nblk, sum, red);
    if (threadIdx.x != 0) return;
    const double gamma = sum[0], beta = sum[1], alpha2 = sum[2];
    const double rho1 = s[KC_RHO1], q = s[KC_Q];
    double rho2 = 0.0, k1 = 1.0, k2 = 1.0;
    if (kc_usable(rho1)) {
        const double g2 = gamma * gamma;
        rho2 = beta - g2 / rho1;
        if (kc_usable(rho2)) {
            const double num = gamma * alpha2, den = rho1 * rho2;
            k1 = q - num / den;
            k2 = alpha2 / rho2;
        } else {
            k1 = q;
            k2 = 0.0;
        }
    }
    s[KC_GAMMA] = gamma;
    s[KC_BETA] = beta;
    s[KC_ALPHA2] = alpha2;
    s[KC_RHO2] = rho2;
    s[KC_K1] = k1;
    s[KC_K2] = k2;
}

// r_i = b_i - q v_i, the product rounded before the subtraction
__global__ __launch_bounds__(kKcBlock) void kc_resid_kernel(int n, const double *__restrict__ s, const double *__restrict__ b,
                                                             const double *__restrict__ v, double *__restrict__ r)
{
    const double q = s[KC_Q];
    const long stride = 2L * kKcBlock * gridDim.x;
    for (long i = 2L * (blockIdx.x * kKcBlock + threadIdx.x); i < n; i += stride) {
        if (i + 1 < n) {
            const double2 bv = *reinterpret_cast<const double2 *>(b + i);
            const double2 vv = *reinterpret_cast<const double2 *>(v + i);
            double2 o;
            o.x = bv.x - q * vv.x;
            o.y = bv.y - q * vv.y;
            *reinterpret_cast<double2 *>(r + i) = o;
        } else {
            r[i] = b[i] - q * v[i];
        }
    }
}

// x_i = k1 c_i + k2 d_i, both products rounded before the sum; x may be d (an element is read before it is written, by its own thread)
__global__ __launch_bounds__(kKcBlock) void kc_combine_kernel(int n, const double *__restrict__ s, const double *__restrict__ c, const double *d,
                                                               double *x)
{
    const double k1 = s[KC_K1], k2 = s[KC_K2];
    const long stride = 2L * kKcBlock * gridDim.x;
    for (long i = 2L * (blockIdx.x * kKcBlock + threadIdx.x); i < n; i += stride) {
        if (i + 1 < n) {
            const double2 cv = *reinterpret_cast<const double2 *>(c + i);
            const double2 dv = *reinterpret_cast<const double2 *>(d + i);
            double2 o;
            o.x = k1 * cv.x + k2 * dv.x;
            o.y = k1 * cv.y + k2 * dv.y;
            *reinterpret_cast<double2 *>(x + i) = o;
        } else {
            x[i] = k1 * c[i] + k2 * d[i];
        }
    }
}

}  // namespace

int kc_grid(int n) { return std::max(1, std::min(kKcMaxGrid, (n + 2 * kKcBlock * 4 - 1) / (2 * kKcBlock * 4))); }

int launch_kc_dot2(int n, const double *c, const double *v, const double *b, double *partial, hipStream_t st)
{
    const int g = kc_grid(n);
    hipLaunchKernelGGL(kc_dot_kernel<2>, dim3(g), dim3(kKcBlock), 0, st, n, c, v, b, (const double *)nullptr, partial);
    return g;
}

int launch_kc_dot3(int n, const double *d, const double *v, const double *w, const double *r, double *partial, hipStream_t st)
{
    const int g = kc_grid(n);
    hipLaunchKernelGGL(kc_dot_kernel<3>, dim3(g), dim3(kKcBlock), 0, st, n, d, v, w, r, partial);
    return g;
}

void launch_kc_scal1(const double *partial, int nblk, double *s, hipStream_t st)
{
    hipLaunchKernelGGL(kc_scal1_kernel, dim3(1), dim3(kKcBlock), 0, st, partial, nblk, s);
}

void launch_kc_scal2(const double *partial, int nblk, double *s, hipStream_t st)
{
    hipLaunchKernelGGL(kc_scal2_kernel, dim3(1), dim3(kKcBlock), 0, st, partial, nblk, s);
}

void launch_kc_resid(int n, const double *s, const double *b, const double *v, double *r, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(kc_resid_kernel, dim3(kc_grid(n)), dim3(kKcBlock), 0, st, n, s, b, v, r);
}

void launch_kc_combine(int n, const double *s, const double *c, const double *d, double *x, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(kc_combine_kernel, dim3(kc_grid(n)), dim3(kKcBlock), 0, st, n, s, c, d, x);
}

}  // namespace sparsh
