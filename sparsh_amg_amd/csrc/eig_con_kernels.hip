// eig_con_kernels.hip -- the projection of the constrained LOBPCG eigensolver: V <- V - Y G^-1 (BY)^T V on
// interleaved blocks, G = Y^T (BY).
//
// Storage is that of eig_kernels.hip.  The mt <= kEigConMax constraints are kept as ceil(mt / W) interleaved blocks of the solve's
// width W, block b at Y + b * n * W and constraint j in column j % W of block j / W; the columns past mt hold zeros.  One projection
// is the Gram launch of eig_kernels.hip with its finalise, then one kernel: the Gram launch on the pairs (BY_b, V) writes
// C = (BY)^T V (mt x W, row-major), then eig_con_apply_kernel subtracts Y (G^-1 C).  No host read, no atomics.
//
// Arithmetic contract: every product and every sum is rounded on its own (the library is built with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sparsh {

namespace {

using d2c = double __attribute__((ext_vector_type(2)));

// dst_ic = src_ic - sum_j Y_ij coef_jc, coef = G^-1 C.
// Every workgroup first forms coef in LDS with the same products in the same order (coef_jc = sum_i Ginv_ji C_ic, i ascending from
// the product of i = 0), so all of them hold the same bits, as the mean of ns_project_kernel.  A lane then owns two neighbouring
// columns of one row: it reads the row of every Y block 16 bytes at a time (the W / 2 lanes of a row share these cache lines), the
// coefficients of its two columns come out of LDS as one 16-byte read that the lanes of a wave share between W / 2 addresses, and the
// running sum over j ascending starts with the product of j = 0; one subtraction at the end.  A lane loads its own 16 bytes of src
// before it stores them to dst, so dst may be src (neither is __restrict__); Y must be neither.  Padding columns of src are zero:
// those of C and coef are then zero and those of dst come out as 0 - 0.
template <int W>
__global__ __launch_bounds__(kBlock) void eig_con_apply_kernel(int n, int mt, const double *__restrict__ Y, size_t ystride,
                                                                const double *__restrict__ Ginv, const double *__restrict__ C, const double *src,
                                                                double *dst)
{
    constexpr int LPR = W / 2;
    constexpr int RP = kBlock / LPR;
    __shared__ double sg[kEigConMax * kEigConMax];
    __shared__ double sc[kEigConMax * W];
    __shared__ __attribute__((aligned(16))) double coef[kEigConMax * W];
    for (int i = threadIdx.x; i < mt * mt; i += kBlock) sg[i] = Ginv[i];
    for (int i = threadIdx.x; i < mt * W; i += kBlock) sc[i] = C[i];
    __syncthreads();
    if (threadIdx.x < mt * W) {
        const int j = threadIdx.x / W, c = threadIdx.x % W;
        double s = sg[j * mt] * sc[c];
        for (int i = 1; i < mt; ++i) {
            const double t = sg[j * mt + i] * sc[i * W + c];
            s = s + t;
        }
        coef[threadIdx.x] = s;
    }
    __syncthreads();
    const int c = 2 * (threadIdx.x % LPR);
    for (size_t row = (size_t)blockIdx.x * RP + threadIdx.x / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const size_t base = row * W;
        d2c acc = {0.0, 0.0};
        for (int j0 = 0; j0 < mt; j0 += W) {
            const double *__restrict__ yr = Y + (size_t)(j0 / W) * ystride + base;
#pragma unroll
            for (int a = 0; a < W; a += 2) {
                const int j = j0 + a;
                if (j < mt) {
                    const d2c y = *reinterpret_cast<const d2c *>(yr + a);
                    const d2c c0 = *reinterpret_cast<const d2c *>(coef + j * W + c);
                    const d2c t0 = {y.x * c0.x, y.x * c0.y};
                    acc = j == 0 ? t0 : acc + t0;
                    if (j + 1 < mt) {
                        const d2c c1 = *reinterpret_cast<const d2c *>(coef + (j + 1) * W + c);
                        const d2c t1 = {y.y * c1.x, y.y * c1.y};
                        acc = acc + t1;
                    }
                }
            }
        }
        const d2c v = *reinterpret_cast<const d2c *>(src + base + c);
        *reinterpret_cast<d2c *>(dst + base + c) = v - acc;
    }
}

// column `col` of an interleaved block <- value (the implicit constant constraint of a null-space handle; once per solve)
__global__ __launch_bounds__(kBlock) void eig_con_fill_column_kernel(int n, int W, int col, double value, double *__restrict__ v)
{
    for (size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x; row < (size_t)n; row += (size_t)gridDim.x * kBlock) v[row * W + col] = value;
}

}  // namespace

void launch_eig_con_fill_column(int n, int W, int col, double value, double *v, hipStream_t st)
{
    const long g = ((long)n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(eig_con_fill_column_kernel, dim3(g > kMultiGridMax ? kMultiGridMax : (int)g), dim3(kBlock), 0, st, n, W, col, value, v);
}

void launch_eig_con_project(int n, int W, int mt, const double *Y, const double *BY, const double *Ginv, const double *src, double *dst,
                            double *C, double *partial, hipStream_t st)
{
    const size_t stride = (size_t)n * W;
    const int nblk = (mt + W - 1) / W;  // <= 9 <= kEigPairs: one Gram launch
    GramPairs prs{};
    for (int b = 0; b < nblk; ++b) {
        prs.u[b] = BY + (size_t)b * stride;
        prs.v[b] = src;
        prs.dst[b] = b * W * W;
    }
    launch_gram_multi(n, W, nblk, prs, partial, C, W, st);
    const int rp = kBlock / (W / 2);
    const long passes = ((long)n + rp - 1) / rp;
    const int g = passes < 1 ? 1 : (passes > kMultiGridMax ? kMultiGridMax : (int)passes);
    switch (W) {
    case 2: hipLaunchKernelGGL(eig_con_apply_kernel<2>, dim3(g), dim3(kBlock), 0, st, n, mt, Y, stride, Ginv, C, src, dst); break;
    case 4: hipLaunchKernelGGL(eig_con_apply_kernel<4>, dim3(g), dim3(kBlock), 0, st, n, mt, Y, stride, Ginv, C, src, dst); break;
    default: hipLaunchKernelGGL(eig_con_apply_kernel<8>, dim3(g), dim3(kBlock), 0, st, n, mt, Y, stride, Ginv, C, src, dst); break;
    }
}

}  // namespace sparsh
