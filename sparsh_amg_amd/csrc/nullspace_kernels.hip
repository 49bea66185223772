// nullspace_kernels.hip -- projection onto mean zero, x -= mean(x), for systems whose null space is the constant vector (pure
// Neumann / fully periodic Poisson problems).  Two launches, no host read and no floating-point atomics:
//   ns_sum_kernel      one partial sum of x per workgroup
//   ns_project_kernel  every workgroup adds the partial sums in the same fixed order, so all of them hold the same sum S bit for bit;
//                      m = S / n ; x_i = x_i - m ; optionally the partial sums of (x_i - m) * r_i for the engine's finalize kernel;
//                      workgroup 0 writes m to its scalar slot
// Both are grid-stride passes over at most kNsGridMax workgroups of kBlock threads (the grid of launch_dot).  A caller's _dev vector
// is only 8-byte aligned: the body runs on 16-byte loads from the first aligned element on, the element in front of it (head) and an
// odd last one (tail) are taken as scalars by thread 0 of workgroup 0.  The order of additions is fixed: inside a lane by ascending
// index, then the wave's shuffle tree, then the workgroup's waves in ascending order, then the partials as described above -- results
// are bitwise reproducible run to run (they may differ in the last bits between the two alignments of the same data, which assign
// the elements to other lanes).  The file is built with -ffp-contract=off: x_i - m and its product with r_i are rounded separately,
// so the dot is the dot of the stored vector.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

#include <cstdint>

namespace sparsh {

namespace {

constexpr int kNsGridMax = 2048;  // as launch_dot: ~8 workgroups per CU, the rest by grid stride

__device__ __forceinline__ double ns_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// sum over the workgroup, valid in thread 0; red holds kBlock / 64 doubles
__device__ __forceinline__ double ns_block_sum(double v, double *red)
{
    v = ns_wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) s += red[k];
    }
    return s;
}

// head = 1 when x[0] sits in front of the first 16-byte boundary
__device__ __forceinline__ int ns_head(const double *x, int n) { return (n > 0 && (reinterpret_cast<uintptr_t>(x) & 15) != 0) ? 1 : 0; }

__global__ __launch_bounds__(kBlock) void ns_sum_kernel(int n, const double *__restrict__ x, double *__restrict__ partial)
{
    __shared__ double red[kBlock / 64];
    const int head = ns_head(x, n);
    const long npair = (n - head) >> 1;
    const double2 *__restrict__ xv = reinterpret_cast<const double2 *>(x + head);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    double acc = 0.0;
    if (first && head) acc = x[0];
    const long stride = (long)gridDim.x * kBlock;
    for (long k = (long)blockIdx.x * kBlock + threadIdx.x; k < npair; k += stride) {
        const double2 v = xv[k];
        acc += v.x;
        acc += v.y;
    }
    if (first && head + 2 * npair < n) acc += x[n - 1];
    const double t = ns_block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

template <bool DOT>
__global__ __launch_bounds__(kBlock) void ns_project_kernel(int n, const double *__restrict__ partial, int nblk, double *__restrict__ x,
                                                             const double *__restrict__ r, double *__restrict__ dot_partial,
                                                             double *__restrict__ mean_slot)
{
    __shared__ double red[kBlock / 64];
    __shared__ double mean_sh;
    // the same additions in the same order in every workgroup: thread t takes partial[t], partial[t + kBlock], ...
    double s = 0.0;
    for (int k = threadIdx.x; k < nblk; k += kBlock) s += partial[k];
    const double S = ns_block_sum(s, red);
    if (threadIdx.x == 0) {
        mean_sh = S / (double)n;
        if (blockIdx.x == 0) *mean_slot = mean_sh;
    }
    __syncthreads();
    const double m = mean_sh;

    const int head = ns_head(x, n);
    const long npair = (n - head) >> 1;
    double2 *__restrict__ xv = reinterpret_cast<double2 *>(x + head);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    // r need not share x's alignment: 16-byte loads where it does, two 8-byte loads where it does not (uniform branch)
    const bool r_pairs = DOT && (reinterpret_cast<uintptr_t>(r + head) & 15) == 0;
    double acc = 0.0;
    if (first && head) {
        const double v = x[0] - m;
        x[0] = v;
        if (DOT) acc += v * r[0];
    }
    const long stride = (long)gridDim.x * kBlock;
    for (long k = (long)blockIdx.x * kBlock + threadIdx.x; k < npair; k += stride) {
        double2 v = xv[k];
        v.x = v.x - m;
        v.y = v.y - m;
        xv[k] = v;
        if (DOT) {
            double2 rv;
            if (r_pairs) {
                rv = reinterpret_cast<const double2 *>(r + head)[k];
            } else {
                rv.x = r[head + 2 * k];
                rv.y = r[head + 2 * k + 1];
            }
            acc += v.x * rv.x;
            acc += v.y * rv.y;
        }
    }
    if (first && head + 2 * npair < n) {
        const double v = x[n - 1] - m;
        x[n - 1] = v;
        if (DOT) acc += v * r[n - 1];
    }
    if (DOT) {
        __syncthreads();  // red is reused
        const double t = ns_block_sum(acc, red);
        if (threadIdx.x == 0) dot_partial[blockIdx.x] = t;
    }
}

}  // namespace

int ns_grid(int n)
{
    int g = (n + kBlock * 2 - 1) / (kBlock * 2);
    if (g < 1) g = 1;
    return g > kNsGridMax ? kNsGridMax : g;
}

void launch_sum(int n, const double *x, double *partial, int *nblk, hipStream_t st)
{
    const int g = ns_grid(n);
    *nblk = g;
    hipLaunchKernelGGL(ns_sum_kernel, dim3(g), dim3(kBlock), 0, st, n, x, partial);
}

void launch_project(int n, const double *partial, int nblk, double *x, const double *r, double *dot_partial, double *mean_slot,
                    hipStream_t st)
{
    const int g = ns_grid(n);
    if (r)
        hipLaunchKernelGGL(ns_project_kernel<true>, dim3(g), dim3(kBlock), 0, st, n, partial, nblk, x, r, dot_partial, mean_slot);
    else
        hipLaunchKernelGGL(ns_project_kernel<false>, dim3(g), dim3(kBlock), 0, st, n, partial, nblk, x, r, dot_partial, mean_slot);
}

}  // namespace sparsh
