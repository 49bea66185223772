// bcg_kernels.hip -- the kernels of block CG: the small dense solve that survives dependent columns, the coupled
// X / R update with its residual norms, the direction update and the finalise.
//
// Storage is that of multi_kernels.hip and eig_kernels.hip: a block of W vectors (W = 2, 4 or 8) is row-interleaved, element (row i,
// column c) at v[i * W + c], 16-byte aligned.  A lane owns two neighbouring columns of one row and the W / 2 lanes of a row sit side by
// side in one wave: a lane's own accesses are 16-byte loads and stores and a wave's accesses are contiguous.  The W x W coefficients
// are read from device memory once per workgroup into LDS; every lane of a wave then reads the same LDS address in the same
// instruction (a broadcast, no bank conflict).
//
// Arithmetic contract: every product and every sum is rounded on its own (the library is built with -ffp-contract=off); sums over the
// columns run with c ascending from the product of c = 0.  Reductions write one partial per column and workgroup and are combined in
// a fixed order without atomics.  Every kernel leaves at once when the solve's `done` flag is set, so the iterations a host that
// reads the flag only every check_every iterations queues past convergence change nothing.
#include <hip/hip_runtime.h>

#include "bcg_small.hpp"
#include "kernels.hpp"

namespace sparsh {

namespace {

using d2b = double __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double bcg_wave_sum_down(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// ------------------------------------------------------------------ small solve

// One wavefront.  factor != 0: LDL^T of G with dropped directions (lane 0; k <= 8, a few hundred flops), kept in device memory for
// the call with factor == 0 that solves with the same G later in the iteration; the rank, the running minimum rank and the count of
// dropped directions are updated, and a rank of 0 ends the solve as a numeric failure.  Then lane c < k solves column c of
// coef = sign * pinv(G) C from the factor in LDS, and the W x W result (zero rows for dropped and padding columns, zero padding
// columns) goes out row-major.
__global__ __launch_bounds__(64) void bcg_small_kernel(int W, int k, int factor, const double *__restrict__ G, const double *__restrict__ C,
                                                        double sign, BcgState s, double *__restrict__ coef, int it)
{
    __shared__ double sG[kBcgMax * kBcgMax], sC[kBcgMax * kBcgMax], sL[kBcgMax * kBcgMax], sO[kBcgMax * kBcgMax], sd[kBcgMax];
    __shared__ double sy[kBcgMax][kBcgMax];
    __shared__ int skeep[kBcgMax];
    if (s.flags[BF_DONE]) return;
    const int t = threadIdx.x;
    if (t < W * W) {
        sG[t] = G[t];
        sC[t] = C[t];
        sO[t] = 0.0;
    }
    if (!factor) {
        sL[t] = s.L[t];
        if (t < kBcgMax) {
            sd[t] = s.d[t];
            skeep[t] = s.flags[BF_KEEP + t];
        }
    } else {
        sL[t] = 0.0;
        if (t < kBcgMax) {
            sd[t] = 0.0;
            skeep[t] = 0;
        }
    }
    __syncthreads();
    if (factor) {
        if (t == 0) {
            const int rank = bcg_factor(k, sG, W, sL, sd, skeep);
            s.flags[BF_RANK] = rank;
            if (rank < s.flags[BF_MIN_RANK]) s.flags[BF_MIN_RANK] = rank;
            s.flags[BF_DROPPED] += k - rank;
            if (rank == 0) {  // no direction left although some residual is above tol
                s.flags[BF_NUMERIC] = 1;
                s.flags[BF_ITERS] = it;
                s.flags[BF_DONE] = 1;
            }
        }
        __syncthreads();
        s.L[t] = sL[t];
        if (t < kBcgMax) {
            s.d[t] = sd[t];
            s.flags[BF_KEEP + t] = skeep[t];
        }
    }
    if (t < k) bcg_solve_column(k, sL, sd, skeep, sC, W, t, sign, sO, W, sy[t]);
    __syncthreads();
    if (t < W * W) coef[t] = sO[t];
}

// ------------------------------------------------------------------ streaming kernels

// the two entries j, j + 1 of sum_{c < k} B_ic C_cj, c ascending, the sum starting with the product of c = 0.  B's row is read 16 bytes
// at a time; sc holds the W x W coefficient matrix in LDS.
template <int W>
__device__ __forceinline__ d2b bcg_row_times(const double *B, size_t base, const double *sc, int j, int k)
{
    d2b acc = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < W; c += 2) {
        if (c < k) {
            const d2b b = *reinterpret_cast<const d2b *>(B + base + c);
            const d2b c0 = *reinterpret_cast<const d2b *>(sc + c * W + j);
            const d2b t0 = {b.x * c0.x, b.x * c0.y};
            acc = c == 0 ? t0 : acc + t0;
            if (c + 1 < k) {
                const d2b c1 = *reinterpret_cast<const d2b *>(sc + (c + 1) * W + j);
                const d2b t1 = {b.y * c1.x, b.y * c1.y};
                acc = acc + t1;
            }
        }
    }
    return acc;
}

// X' = X + P alpha ; R' = R - Q alpha on the columns j < k (the others are written as zeros) ; partial[c * gridDim.x + workgroup] = this
// workgroup's share of R'_c . R'_c.  A lane adds its rows in ascending order; the lanes that own the same two columns are added by a
// fixed butterfly inside every wave and the four waves in order.  Xo may be X and Ro may be R (none of those pointers is
// __restrict__): a lane reads and writes only its own two columns of X and R.
template <int W>
__global__ __launch_bounds__(kBlock) void bcg_update_kernel(int n, int k, const int *__restrict__ done, const double *X, const double *R,
                                                             const double *__restrict__ P, const double *__restrict__ Q,
                                                             const double *__restrict__ alpha, double *Xo, double *Ro,
                                                             double *__restrict__ partial)
{
    constexpr int LPR = W / 2;
    constexpr int RP = kBlock / LPR;
    __shared__ __attribute__((aligned(16))) double sc[W * W];
    __shared__ double red[(kBlock / 64) * W];
    if (done && *done) return;
    for (int i = threadIdx.x; i < W * W; i += kBlock) sc[i] = alpha[i];
    __syncthreads();
    const int j = 2 * (threadIdx.x % LPR);
    d2b acc = {0.0, 0.0};
    for (size_t row = (size_t)blockIdx.x * RP + threadIdx.x / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const size_t base = row * W;
        const d2b pa = bcg_row_times<W>(P, base, sc, j, k);
        const d2b qa = bcg_row_times<W>(Q, base, sc, j, k);
        d2b x = *reinterpret_cast<const d2b *>(X + base + j);
        d2b r = *reinterpret_cast<const d2b *>(R + base + j);
        x = x + pa;
        r = r - qa;
        if (j >= k) x = r = d2b{0.0, 0.0};
        else if (j + 1 >= k) x.y = r.y = 0.0;
        *reinterpret_cast<d2b *>(Xo + base + j) = x;
        *reinterpret_cast<d2b *>(Ro + base + j) = r;
        acc += r * r;
    }
#pragma unroll
    for (int off = 32; off >= LPR; off >>= 1) {
        acc.x += __shfl_xor(acc.x, off, 64);
        acc.y += __shfl_xor(acc.y, off, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane < LPR) {
        red[w * W + j] = acc.x;
        red[w * W + j + 1] = acc.y;
    }
    __syncthreads();
    if (threadIdx.x < W) {
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < kBlock / 64; ++q) sum += red[q * W + threadIdx.x];
        partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = sum;
    }
}

// P' = Z + P beta on the columns j < k (the others are written as zeros).  Po may be P: every lane of a row reads the whole row of P
// and stores two of its columns, and the W / 2 lanes of a row sit in one wave, which issues one instruction for all its lanes, the
// row's loads (program order, no __restrict__ on P / Po) ahead of its store.  That is a guarantee of wave-lockstep execution, as in
// eig_update_kernel, not of C++ ordering between threads: a layout that spreads a row over two waves would need a second buffer.
template <int W>
__global__ __launch_bounds__(kBlock) void bcg_dir_kernel(int n, int k, const int *__restrict__ done, const double *__restrict__ Z, const double *P,
                                                          const double *__restrict__ beta, double *Po)
{
    constexpr int LPR = W / 2;
    constexpr int RP = kBlock / LPR;
    __shared__ __attribute__((aligned(16))) double sc[W * W];
    if (done && *done) return;
    for (int i = threadIdx.x; i < W * W; i += kBlock) sc[i] = beta[i];
    __syncthreads();
    const int j = 2 * (threadIdx.x % LPR);
    for (size_t row = (size_t)blockIdx.x * RP + threadIdx.x / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const size_t base = row * W;
        const d2b pb = bcg_row_times<W>(P, base, sc, j, k);
        d2b p = *reinterpret_cast<const d2b *>(Z + base + j);
        p = p + pb;
        if (j >= k) p = d2b{0.0, 0.0};
        else if (j + 1 >= k) p.y = 0.0;
        *reinterpret_cast<d2b *>(Po + base + j) = p;
    }
}

// ------------------------------------------------------------------ finalise

// One wave per column adds the nblk partials of rn_c^2 in a fixed order (lane l takes l, l + 64, ..., then the shuffle tree); thread 0
// then takes the square roots and decides, columns ascending.  it < 0: the start of a solve (the flags and counters are reset, no
// history entry, iters = 0); it >= 0: the end of iteration it + 1.  done = every column c < nrhs has rn_c <= tol; a NaN in any of them
// ends the solve as a numeric failure.
__global__ __launch_bounds__(kBcgMax * 64) void bcg_finalize_kernel(int W, int nrhs, const double *__restrict__ partial, int nblk, BcgState s,
                                                                     double tol, double *__restrict__ hist, int hist_cap, int it)
{
    __shared__ double sums[kBcgMax];
    if (it >= 0 && s.flags[BF_DONE]) return;
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    if (c < W) {
        double v = 0.0;
        for (int i = lane; i < nblk; i += 64) v += partial[(size_t)c * nblk + i];
        v = bcg_wave_sum_down(v);
        if (lane == 0) sums[c] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    bool all = true, nan = false;
    for (int q = 0; q < nrhs; ++q) {
        const double res = sqrt(sums[q]);
        s.res[q] = res;
        if (it >= 0 && hist && it < hist_cap) hist[(size_t)q * hist_cap + it] = res;
        if (!(res == res)) nan = true;
        if (!(res <= tol)) all = false;
    }
    if (it < 0) {
        for (int q = 0; q < kBcgMax; ++q) s.flags[BF_KEEP + q] = 0;
        s.flags[BF_RANK] = 0;
        s.flags[BF_MIN_RANK] = nrhs;
        s.flags[BF_DROPPED] = 0;
    }
    s.flags[BF_ITERS] = it + 1;
    s.flags[BF_NUMERIC] = nan ? 1 : 0;
    s.flags[BF_DONE] = (all || nan) ? 1 : 0;
}

}  // namespace

#define BCG_DISPATCH(W, CALL) \
    switch (W) {              \
    case 2: { constexpr int kW = 2; CALL; } break; \
    case 4: { constexpr int kW = 4; CALL; } break; \
    default: { constexpr int kW = 8; CALL; } break; \
    }

int bcg_grid(int n, int W)
{
    const int rp = kBlock / (W / 2);
    const long g = ((long)n + rp - 1) / rp;
    return g < 1 ? 1 : (g > kBcgMaxGrid ? kBcgMaxGrid : (int)g);
}

void launch_bcg_small(int W, int k, bool factor, const double *G, const double *C, double sign, const BcgState &s, double *coef, int it,
                      hipStream_t st)
{
    hipLaunchKernelGGL(bcg_small_kernel, dim3(1), dim3(64), 0, st, W, k, factor ? 1 : 0, G, C, sign, s, coef, it);
}

int launch_bcg_update(int n, int W, int k, const int *done, const double *X, const double *R, const double *P, const double *Q,
                      const double *alpha, double *Xo, double *Ro, double *partial, hipStream_t st)
{
    const int g = bcg_grid(n, W);
    BCG_DISPATCH(W, hipLaunchKernelGGL(bcg_update_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, k, done, X, R, P, Q, alpha, Xo, Ro, partial));
    return g;
}

void launch_bcg_dir(int n, int W, int k, const int *done, const double *Z, const double *P, const double *beta, double *Po, hipStream_t st)
{
    const int g = bcg_grid(n, W);
    BCG_DISPATCH(W, hipLaunchKernelGGL(bcg_dir_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, k, done, Z, P, beta, Po));
}

void launch_bcg_finalize(int W, int nrhs, const double *partial, int nblk, const BcgState &s, double tol, double *hist, int hist_cap, int it,
                         hipStream_t st)
{
    hipLaunchKernelGGL(bcg_finalize_kernel, dim3(1), dim3(kBcgMax * 64), 0, st, W, nrhs, partial, nblk, s, tol, hist, hist_cap, it);
}

}  // namespace sparsh
