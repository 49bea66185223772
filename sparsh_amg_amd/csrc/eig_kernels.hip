// eig_kernels.hip -- the block kernels of the LOBPCG eigensolver: Gram matrices of interleaved blocks, the
// eigen-residual and the subspace update.
//
// Storage is that of multi_kernels.hip: a block of W vectors (W = 2, 4 or 8) is row-interleaved, element (row i, column c) at
// v[i * W + c], 16-byte aligned.  As there, a lane owns two neighbouring columns of one row and the W / 2 lanes of a row sit side by
// side in one wave: every access of a lane's own columns is a 16-byte load or store and a wave's accesses are contiguous.
//
// Arithmetic contract: every product and every sum is rounded on its own (the library is built with -ffp-contract=off).  Reductions
// write one partial per sum and workgroup and are combined in a fixed order without atomics: the same input gives the same bits.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sparsh {

namespace {

using d2e = double __attribute__((ext_vector_type(2)));

constexpr int kEigUpdateMaxGrid = 2048;  // the update reduces nothing: ~8 workgroups per CU, as the elementwise block kernels

__device__ __forceinline__ double eig_wave_sum_down(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// ------------------------------------------------------------------ Gram matrices

// partial[(pair * W * W + a * W + b) * gridDim.x + workgroup] = this workgroup's share of sum_i U_ia V_ib, for the pair blockIdx.y of
// the list.  A lane owns the rows a, a + 1 of the W x W product of one matrix row: 2 W accumulators, not W * W, so no instance is
// near the register limit; the W / 2 lanes of a row read the row of V together (the same cache lines) and their own 16 bytes of U.
// A lane adds its rows in ascending order; the lanes that own the same two columns of U are then added by a fixed butterfly inside
// every wave and the four waves in order, as the block sums of multi_kernels.hip.
template <int W>
__global__ __launch_bounds__(kBlock) void gram_multi_kernel(int n, GramPairs prs, double *__restrict__ partial)
{
    constexpr int LPR = W / 2;        // lanes per row
    constexpr int RP = kBlock / LPR;  // rows per pass
    __shared__ double red[(kBlock / 64) * W * W];
    const double *__restrict__ U = prs.u[blockIdx.y];
    const double *__restrict__ V = prs.v[blockIdx.y];
    const int tid = threadIdx.x;
    const int a = 2 * (tid % LPR);
    d2e acc[W];
#pragma unroll
    for (int b = 0; b < W; ++b) acc[b] = d2e{0.0, 0.0};
    for (size_t row = (size_t)blockIdx.x * RP + tid / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const d2e u = *reinterpret_cast<const d2e *>(U + row * W + a);
#pragma unroll
        for (int b = 0; b < W; b += 2) {
            const d2e v = *reinterpret_cast<const d2e *>(V + row * W + b);
            acc[b].x += u.x * v.x;
            acc[b].y += u.y * v.x;
            acc[b + 1].x += u.x * v.y;
            acc[b + 1].y += u.y * v.y;
        }
    }
#pragma unroll
    for (int b = 0; b < W; ++b) {
#pragma unroll
        for (int off = 32; off >= LPR; off >>= 1) {
            acc[b].x += __shfl_xor(acc[b].x, off, 64);
            acc[b].y += __shfl_xor(acc[b].y, off, 64);
        }
    }
    const int lane = tid & 63, w = tid >> 6;
    if (lane < LPR) {
#pragma unroll
        for (int b = 0; b < W; ++b) {
            red[w * W * W + a * W + b] = acc[b].x;
            red[w * W * W + (a + 1) * W + b] = acc[b].y;
        }
    }
    __syncthreads();
    if (tid < W * W) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) s += red[k * W * W + tid];
        partial[((size_t)blockIdx.y * W * W + tid) * gridDim.x + blockIdx.x] = s;
    }
}

// one wave per (pair, entry): the nblk partials are added in a fixed order (lane l takes l, l + 64, ..., then the shuffle tree) and
// stored at G[dst[pair] + a * ldg + b]
__global__ __launch_bounds__(kBlock) void gram_finalize_kernel(int W, int npairs, GramPairs prs, const double *__restrict__ partial, int nblk,
                                                                double *__restrict__ G, int ldg)
{
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (item >= npairs * W * W) return;  // whole wave leaves
    const int pair = item / (W * W), e = item % (W * W);
    const double *__restrict__ p = partial + (size_t)item * nblk;
    double v = 0.0;
    for (int i = lane; i < nblk; i += 64) v += p[i];
    v = eig_wave_sum_down(v);
    if (lane == 0) G[prs.dst[pair] + (e / W) * ldg + (e % W)] = v;
}

// ------------------------------------------------------------------ residual

// per-column sum over a workgroup whose thread t holds a value of column t % W (column_block_sum of multi_kernels.hip)
template <int W>
__device__ __forceinline__ double eig_column_block_sum(double v, double *red)
{
#pragma unroll
    for (int off = 32; off >= W; off >>= 1) v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane < W) red[w * kMultiMax + lane] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x < W) {
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) s += red[k * kMultiMax + threadIdx.x];
    }
    return s;
}

// R = AX - X * theta_c (the product and the subtraction are two roundings); partial[c * gridDim.x + workgroup] = the share of
// R_c . R_c.  The grid stride is a multiple of W: a thread stays in its column.
template <int W>
__global__ __launch_bounds__(kBlock) void eig_residual_kernel(int n, const double *__restrict__ AX, const double *__restrict__ X,
                                                               const double *__restrict__ theta, double *__restrict__ R,
                                                               double *__restrict__ partial)
{
    __shared__ double red[(kBlock / 64) * kMultiMax];
    const double th = theta[threadIdx.x % W];
    const size_t total = (size_t)n * W;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        const double t = X[i] * th;
        const double r = AX[i] - t;
        R[i] = r;
        acc += r * r;
    }
    const double t = eig_column_block_sum<W>(acc, red);
    if (threadIdx.x < W) partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
}

// out[c] = sqrt of the sum of column c's partials, one wave per column
__global__ __launch_bounds__(kMultiMax * 64) void eig_norm_finalize_kernel(int W, const double *__restrict__ partial, int nblk, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    if (c >= W) return;
    double v = 0.0;
    for (int i = lane; i < nblk; i += 64) v += partial[(size_t)c * nblk + i];
    v = eig_wave_sum_down(v);
    if (lane == 0) out[c] = sqrt(v);
}

// ------------------------------------------------------------------ residual of the pencil (A, B)

// R = AX - BX * theta_c (two roundings); rr[c * nblk + j] and bb[c * nblk + j] = the shares of R_c . R_c and BX_c . BX_c, nblk =
// eig_grid(n, W) = gridDim.x * 2 (rounded up).  A lane owns two neighbouring columns of one row (16-byte accesses).  The sums are those
// of eig_residual_kernel, bit for bit: with B = I the two solvers see the same residual norms.  There thread t of workgroup j adds the
// elements (j + m * nblk) * 256 + t, m ascending; here one half of a workgroup (128 lanes) stands for workgroup j = 2 * blockIdx.x +
// half, and its lane q holds the sums of t = 2 q and 2 q + 1 in the two components.  A 64-row wave of that kernel is 32 lanes here,
// so its butterfly over t ^ 32 ... t ^ W is the one over q ^ 16 ... q ^ (W / 2), and its four waves are added in the same order.
template <int W>
__global__ __launch_bounds__(kBlock) void eig_residual_gen_kernel(int n, int nblk, const double *__restrict__ AX, const double *__restrict__ BX,
                                                                   const double *__restrict__ theta, double *__restrict__ R,
                                                                   double *__restrict__ rr, double *__restrict__ bb)
{
    constexpr int HALF = kBlock / 2;  // lanes that stand for one workgroup of eig_residual_kernel
    __shared__ double red[2][2][HALF / 32][kMultiMax];  // quantity, half, 32-lane group, column
    const int half = threadIdx.x / HALF, q = threadIdx.x % HALF;
    const int j = 2 * blockIdx.x + half;
    const int col = (2 * q) % W;
    const d2e th = {theta[col], theta[col + 1]};
    const size_t total = (size_t)n * W;  // even: a pair never straddles the end
    d2e acc = {0.0, 0.0}, bacc = {0.0, 0.0};
    if (j < nblk) {
        for (size_t i = (size_t)j * kBlock + 2 * q; i < total; i += (size_t)nblk * kBlock) {
            const d2e bx = *reinterpret_cast<const d2e *>(BX + i);
            const d2e ax = *reinterpret_cast<const d2e *>(AX + i);
            const d2e t = bx * th;
            const d2e r = ax - t;
            *reinterpret_cast<d2e *>(R + i) = r;
            acc += r * r;
            bacc += bx * bx;
        }
    }
#pragma unroll
    for (int off = 16; off >= W / 2; off >>= 1) {
        acc.x += __shfl_xor(acc.x, off, 64);
        acc.y += __shfl_xor(acc.y, off, 64);
        bacc.x += __shfl_xor(bacc.x, off, 64);
        bacc.y += __shfl_xor(bacc.y, off, 64);
    }
    const int l32 = q & 31, g32 = q >> 5;
    if (l32 < W / 2) {
        red[0][half][g32][2 * l32] = acc.x;
        red[0][half][g32][2 * l32 + 1] = acc.y;
        red[1][half][g32][2 * l32] = bacc.x;
        red[1][half][g32][2 * l32 + 1] = bacc.y;
    }
    __syncthreads();
    if (threadIdx.x < 4 * W) {
        const int what = threadIdx.x / (2 * W), hh = (threadIdx.x / W) % 2, c = threadIdx.x % W;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < HALF / 32; ++k) s += red[what][hh][k][c];
        const int jj = 2 * blockIdx.x + hh;
        if (jj < nblk) (what ? bb : rr)[(size_t)c * nblk + jj] = s;
    }
}

// blockIdx.x = 0: out0[c] = sqrt of the sum of column c's partials in p0; 1: out1 from p1.  One wave per column, the order of
// eig_norm_finalize_kernel.
__global__ __launch_bounds__(kMultiMax * 64) void eig_norm2_finalize_kernel(int W, const double *__restrict__ p0, const double *__restrict__ p1, int nblk,
                                                                             double *__restrict__ out0, double *__restrict__ out1)
{
    const double *__restrict__ partial = blockIdx.x ? p1 : p0;
    double *__restrict__ out = blockIdx.x ? out1 : out0;
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    if (c >= W) return;
    double v = 0.0;
    for (int i = lane; i < nblk; i += 64) v += partial[(size_t)c * nblk + i];
    v = eig_wave_sum_down(v);
    if (lane == 0) out[c] = sqrt(v);
}

// ------------------------------------------------------------------ update

// the two entries j, j + 1 of sum_{c < k} B_ic C_cj, c ascending, continuing the running sum `acc` (first: the sum starts with the
// product of c = 0).  B's row is read 16 bytes at a time; sc holds the W x W coefficient matrix in LDS.
template <int W>
__device__ __forceinline__ d2e eig_row_times(const double *B, size_t base, const double *sc, int j, int k, d2e acc, bool first)
{
#pragma unroll
    for (int c = 0; c < W; c += 2) {
        if (c < k) {
            const d2e b = *reinterpret_cast<const d2e *>(B + base + c);
            const d2e c0 = *reinterpret_cast<const d2e *>(sc + c * W + j);
            const d2e t0 = {b.x * c0.x, b.x * c0.y};
            acc = (first && c == 0) ? t0 : acc + t0;
            if (c + 1 < k) {
                const d2e c1 = *reinterpret_cast<const d2e *>(sc + (c + 1) * W + j);
                const d2e t1 = {b.y * c1.x, b.y * c1.y};
                acc = acc + t1;
            }
        }
    }
    return acc;
}

// P' = W Cw + P Cp ; X' = X Cx + P' ; AP' = AW Cw + AP Cp ; AX' = AX Cx + AP' on the columns j < k (the others are written as zeros),
// every sum over c < k ascending.  All loads of a row come before its stores and the lanes of a row share a wave, so an output may be
// the block it replaces (Xo == X, Po == P, ...): none of the pointers is __restrict__.
template <int W>
__global__ __launch_bounds__(kBlock) void eig_update_kernel(int n, int k, const double *X, const double *Wb, const double *P, const double *AX,
                                                             const double *AW, const double *AP, const double *__restrict__ coef, double *Xo,
                                                             double *Po, double *AXo, double *APo)
{
    constexpr int LPR = W / 2;
    constexpr int RP = kBlock / LPR;
    __shared__ __attribute__((aligned(16))) double sc[3 * W * W];  // Cx, Cw, Cp
    for (int i = threadIdx.x; i < 3 * W * W; i += kBlock) sc[i] = coef[i];
    __syncthreads();
    const double *cx = sc, *cw = sc + W * W, *cp = sc + 2 * W * W;
    const int j = 2 * (threadIdx.x % LPR);
    const d2e zero = {0.0, 0.0};
    for (size_t row = (size_t)blockIdx.x * RP + threadIdx.x / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const size_t base = row * W;
        d2e p = eig_row_times<W>(Wb, base, cw, j, k, zero, true);
        p = eig_row_times<W>(P, base, cp, j, k, p, false);
        d2e ap = eig_row_times<W>(AW, base, cw, j, k, zero, true);
        ap = eig_row_times<W>(AP, base, cp, j, k, ap, false);
        d2e x = eig_row_times<W>(X, base, cx, j, k, zero, true);
        d2e ax = eig_row_times<W>(AX, base, cx, j, k, zero, true);
        x = x + p;
        ax = ax + ap;
        if (j >= k) x = ax = p = ap = zero;
        else if (j + 1 >= k) x.y = ax.y = p.y = ap.y = 0.0;
        *reinterpret_cast<d2e *>(Po + base + j) = p;
        *reinterpret_cast<d2e *>(APo + base + j) = ap;
        *reinterpret_cast<d2e *>(Xo + base + j) = x;
        *reinterpret_cast<d2e *>(AXo + base + j) = ax;
    }
}

// eig_update_kernel with B S carried along: BP' = BW Cw + BP Cp ; BX' = BX Cx + BP' with the same coefficients and the same order of
// sums.  Nine blocks in, six out; all loads of a row come before its stores, so an output may be the block it replaces.
template <int W>
__global__ __launch_bounds__(kBlock) void eig_update_gen_kernel(int n, int k, const double *X, const double *Wb, const double *P, const double *AX,
                                                                 const double *AW, const double *AP, const double *BX, const double *BW,
                                                                 const double *BP, const double *__restrict__ coef, double *Xo, double *Po,
                                                                 double *AXo, double *APo, double *BXo, double *BPo)
{
    constexpr int LPR = W / 2;
    constexpr int RP = kBlock / LPR;
    __shared__ __attribute__((aligned(16))) double sc[3 * W * W];  // Cx, Cw, Cp
    for (int i = threadIdx.x; i < 3 * W * W; i += kBlock) sc[i] = coef[i];
    __syncthreads();
    const double *cx = sc, *cw = sc + W * W, *cp = sc + 2 * W * W;
    const int j = 2 * (threadIdx.x % LPR);
    const d2e zero = {0.0, 0.0};
    for (size_t row = (size_t)blockIdx.x * RP + threadIdx.x / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const size_t base = row * W;
        d2e p = eig_row_times<W>(Wb, base, cw, j, k, zero, true);
        p = eig_row_times<W>(P, base, cp, j, k, p, false);
        d2e ap = eig_row_times<W>(AW, base, cw, j, k, zero, true);
        ap = eig_row_times<W>(AP, base, cp, j, k, ap, false);
        d2e bp = eig_row_times<W>(BW, base, cw, j, k, zero, true);
        bp = eig_row_times<W>(BP, base, cp, j, k, bp, false);
        d2e x = eig_row_times<W>(X, base, cx, j, k, zero, true);
        d2e ax = eig_row_times<W>(AX, base, cx, j, k, zero, true);
        d2e bx = eig_row_times<W>(BX, base, cx, j, k, zero, true);
        x = x + p;
        ax = ax + ap;
        bx = bx + bp;
        if (j >= k) x = ax = bx = p = ap = bp = zero;
        else if (j + 1 >= k) x.y = ax.y = bx.y = p.y = ap.y = bp.y = 0.0;
        *reinterpret_cast<d2e *>(Po + base + j) = p;
        *reinterpret_cast<d2e *>(APo + base + j) = ap;
        *reinterpret_cast<d2e *>(BPo + base + j) = bp;
        *reinterpret_cast<d2e *>(Xo + base + j) = x;
        *reinterpret_cast<d2e *>(AXo + base + j) = ax;
        *reinterpret_cast<d2e *>(BXo + base + j) = bx;
    }
}

}  // namespace

#define EIG_DISPATCH(W, CALL) \
    switch (W) {              \
    case 2: { constexpr int kW = 2; CALL; } break; \
    case 4: { constexpr int kW = 4; CALL; } break; \
    default: { constexpr int kW = 8; CALL; } break; \
    }

int eig_grid(int n, int W)
{
    const int rp = kBlock / (W / 2);
    const long g = ((long)n + rp - 1) / rp;
    return g < 1 ? 1 : (g > kEigMaxGrid ? kEigMaxGrid : (int)g);
}

int launch_gram_multi(int n, int W, int npairs, const GramPairs &prs, double *partial, double *G, int ldg, hipStream_t st)
{
    const int g = eig_grid(n, W);
    if (npairs <= 0) return g;
    EIG_DISPATCH(W, hipLaunchKernelGGL(gram_multi_kernel<kW>, dim3(g, npairs), dim3(kBlock), 0, st, n, prs, partial));
    const int waves = npairs * W * W;
    hipLaunchKernelGGL(gram_finalize_kernel, dim3((waves + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, st, W, npairs, prs, partial, g, G, ldg);
    return g;
}

void launch_eig_residual(int n, int W, const double *AX, const double *X, const double *theta, double *R, double *partial, double *norms,
                         hipStream_t st)
{
    const int g = eig_grid(n, W);
    EIG_DISPATCH(W, hipLaunchKernelGGL(eig_residual_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, AX, X, theta, R, partial));
    hipLaunchKernelGGL(eig_norm_finalize_kernel, dim3(1), dim3(kMultiMax * 64), 0, st, W, partial, g, norms);
}

void launch_eig_update(int n, int W, int k, const double *X, const double *Wb, const double *P, const double *AX, const double *AW,
                       const double *AP, const double *coef, double *Xo, double *Po, double *AXo, double *APo, hipStream_t st)
{
    // no partial sums to bound the grid here: one workgroup per pass of rows up to ~8 workgroups per CU, so that enough loads are in
    // flight (rows are independent: the grid does not change a bit of the result)
    const long passes = ((long)n + kBlock / (W / 2) - 1) / (kBlock / (W / 2));
    const int g = passes < 1 ? 1 : (passes > kEigUpdateMaxGrid ? kEigUpdateMaxGrid : (int)passes);
    EIG_DISPATCH(W, hipLaunchKernelGGL(eig_update_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, k, X, Wb, P, AX, AW, AP, coef, Xo, Po, AXo, APo));
}

void launch_eig_residual_gen(int n, int W, const double *AX, const double *BX, const double *theta, double *R, double *partial, double *rnorms,
                             double *bnorms, hipStream_t st)
{
    const int g = eig_grid(n, W);
    double *rr = partial, *bb = partial + (size_t)W * g;
    EIG_DISPATCH(W, hipLaunchKernelGGL(eig_residual_gen_kernel<kW>, dim3((g + 1) / 2), dim3(kBlock), 0, st, n, g, AX, BX, theta, R, rr, bb));
    hipLaunchKernelGGL(eig_norm2_finalize_kernel, dim3(2), dim3(kMultiMax * 64), 0, st, W, rr, bb, g, rnorms, bnorms);
}

void launch_eig_update_gen(int n, int W, int k, const double *const in[9], const double *coef, double *const out[6], hipStream_t st)
{
    const long passes = ((long)n + kBlock / (W / 2) - 1) / (kBlock / (W / 2));  // the grid of launch_eig_update
    const int g = passes < 1 ? 1 : (passes > kEigUpdateMaxGrid ? kEigUpdateMaxGrid : (int)passes);
    EIG_DISPATCH(W, hipLaunchKernelGGL(eig_update_gen_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, k, in[0], in[1], in[2], in[3], in[4], in[5], in[6],
                                       in[7], in[8], coef, out[0], out[1], out[2], out[3], out[4], out[5]));
}

}  // namespace sparsh
