// multi_kernels.hip -- block of up to 8 right-hand sides: the kernels of the block V-cycle and of block PCG.
//
// Storage: a block of W vectors (W = 2, 4 or 8) is row-interleaved, element (row i, column c) at v[i * W + c].  A kernel reads the
// operator once for all W columns: the col / val run of a row block is staged in LDS with unit-stride loads, then a lane owns
// two neighbouring columns of one row of a pass over 512 / W rows -- the W / 2 lanes of a row read the same LDS entry (a broadcast)
// and gather W * 8 contiguous bytes of x, 16 bytes per lane.
//
// Arithmetic contract, per column, that of the single-vector kernels (kernels.hip): a row sum adds the separately rounded products
// one by one in stored order from +0.0, a row longer than the LDS buffer chunk by chunk in stored order as well; the epilogues are
// the expressions of row_epilogue.  Reductions: one partial per column and workgroup at partial[c * nblk + workgroup], combined in a
// fixed order without atomics.  The CSR launches keep the placement policy of csr_placement (non-temporal matrix stream and the XCD
// remap, decided on the bytes one block sweep streams); placement only, results unchanged.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sparsh {

namespace {

inline int multi_grid(size_t elements)
{
    size_t g = (elements + kBlock * 2 - 1) / (kBlock * 2);
    if (g < 1) g = 1;
    return g > (size_t)kMultiGridMax ? kMultiGridMax : (int)g;
}

__device__ __forceinline__ double wave_sum_down(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// per-column sum over a workgroup whose thread t holds a value of column t % W: a fixed butterfly inside every wave, then the four
// waves in order.  Thread c < W returns column c's sum; red holds (kBlock / 64) * kMultiMax doubles.
template <int W>
__device__ __forceinline__ double column_block_sum(double v, double *red)
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

using d2m = double __attribute__((ext_vector_type(2)));

// Workgroups are dealt round-robin over the 8 XCDs: remap = 1 gives XCD x the x-th contiguous eighth of the row blocks, remap = G > 1
// the groups x, x + 8, ... of G consecutive row blocks (the mapping of the single-vector kernels, csr_placement).  Placement only.
__device__ __forceinline__ int multi_xcd_remap(int b, int nblk, int mode)
{
    const int xcd = b & 7, i = b >> 3;
    if (mode == 1) return xcd * ((nblk + 7) >> 3) + i;
    return ((i / mode) * 8 + xcd) * mode + (i % mode);
}

inline int multi_remap_grid(int nblk, int mode)
{
    if (mode <= 0) return nblk;
    const int q = 8 * (mode == 1 ? 1 : mode);
    return ((nblk + q - 1) / q) * q;
}

// the sums of a workgroup whose lane owns the columns 2 (lane % LPR) and 2 (lane % LPR) + 1 (LPR = W / 2 lanes per row): a fixed
// butterfly inside every wave, then the four waves in order.  Thread c < W returns column c's sum.
template <int W>
__device__ __forceinline__ double column_pair_block_sum(double v0, double v1, double *red)
{
    constexpr int LPR = W / 2;
#pragma unroll
    for (int off = 32; off >= LPR; off >>= 1) {
        v0 += __shfl_xor(v0, off, 64);
        v1 += __shfl_xor(v1, off, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane < LPR) {
        red[w * kMultiMax + 2 * lane] = v0;
        red[w * kMultiMax + 2 * lane + 1] = v1;
    }
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x < W) {
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) s += red[k * kMultiMax + threadIdx.x];
    }
    return s;
}

// what happens to the row sums of (row, columns c and c + 1), c even: the expressions of row_epilogue per column, 16-byte loads and
// stores; returns the two contributions to the fused reduction
template <int W, int OP>
__device__ __forceinline__ d2m multi_epilogue(const MultiArgs &a, int row, int c, d2m sum, d2m bi, d2m xi, double di)
{
    d2m *y = reinterpret_cast<d2m *>(a.y + (size_t)row * W + c);
    d2m out = {0.0, 0.0};
    if constexpr (OP == OP_SPMV) {
        *y = sum;
    } else if constexpr (OP == OP_RESID) {
        d2m r;
        r.x = 1.0 * bi.x + (-1.0) * sum.x;
        r.y = 1.0 * bi.y + (-1.0) * sum.y;
        *y = r;
    } else if constexpr (OP == OP_JACOBI) {
        const double h0 = 1.0 * bi.x + (-1.0) * sum.x, h1 = 1.0 * bi.y + (-1.0) * sum.y;
        d2m r;
        r.x = xi.x + a.omega * h0 / di;
        r.y = xi.y + a.omega * h1 / di;
        *y = r;
    } else if constexpr (OP == OP_ADD) {
        const d2m old = *y;
        d2m r;
        r.x = sum.x + old.x;
        r.y = sum.y + old.y;
        *y = r;
    } else if constexpr (OP == OP_SPMV_DOT) {
        *y = sum;
        out.x = xi.x * sum.x;
        out.y = xi.y * sum.y;
    }
    return out;
}

template <bool NT, class T>
__device__ __forceinline__ T multi_ld(const T *p)
{
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

// NT: the matrix stream is read with non-temporal loads (operators that do not stay in the memory-side cache between sweeps)
template <int W, int OP, bool NT>
__global__ __launch_bounds__(kBlock) void csr_multi_kernel(const int4 *__restrict__ rowblk, int nblk, int remap, const int *__restrict__ rowptr,
                                                            const int *__restrict__ col, const double *__restrict__ val, MultiArgs a)
{
    __shared__ double sval[kStreamNnz];
    __shared__ int scol[kStreamNnz];
    __shared__ double red[(kBlock / 64) * kMultiMax];
    const int bid = remap ? multi_xcd_remap(blockIdx.x, nblk, remap) : blockIdx.x;
    if (bid >= nblk) return;  // whole workgroup leaves together
    const int tid = threadIdx.x;
    const int4 br = rowblk[bid];
    const int r0 = br.x, r1 = br.y, j0 = br.z, j1 = br.w;
    const double *x = a.x;
    constexpr int LPR = W / 2;        // lanes per row: a lane owns two neighbouring columns (16-byte accesses)
    constexpr int RP = kBlock / LPR;  // rows per pass
    const int rl = tid / LPR, c = 2 * (tid % LPR);
    constexpr bool need_b = OP == OP_RESID || OP == OP_JACOBI;
    constexpr bool need_xi = OP == OP_JACOBI || OP == OP_SPMV_DOT;
    const d2m zero = {0.0, 0.0};
    d2m acc = zero;
    if (r1 - r0 == 1 && j1 - j0 > kStreamNnz) {
        // one long row: chunk by chunk through LDS, every chunk added in stored order by the LPR threads that own the row's columns
        d2m sum = zero;
        for (int c0 = j0; c0 < j1; c0 += kStreamNnz) {
            const int c1 = c0 + kStreamNnz < j1 ? c0 + kStreamNnz : j1;
            for (int j = c0 + tid; j < c1; j += kBlock) {
                scol[j - c0] = multi_ld<NT>(col + j);
                sval[j - c0] = multi_ld<NT>(val + j);
            }
            __syncthreads();
            if (tid < LPR)
                for (int k = 0; k < c1 - c0; ++k) {
                    const d2m xv = *reinterpret_cast<const d2m *>(x + (size_t)scol[k] * W + c);
                    const double v = sval[k];
                    sum.x = sum.x + v * xv.x;
                    sum.y = sum.y + v * xv.y;
                }
            __syncthreads();
        }
        if (tid < LPR) {
            const size_t i = (size_t)r0 * W + c;
            const d2m bi = need_b ? *reinterpret_cast<const d2m *>(a.b + i) : zero;
            const d2m xi = need_xi ? *reinterpret_cast<const d2m *>(x + i) : zero;
            acc = multi_epilogue<W, OP>(a, r0, c, sum, bi, xi, OP == OP_JACOBI ? a.d[r0] : 1.0);
        }
    } else {
        // the block's col / val run -> LDS with unit-stride loads, four per thread in flight (index clamped into the run)
        const int jlast = j1 - 1;
        for (int j = j0 + tid; j < j1; j += 4 * kBlock) {
            int cc[4];
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int jj = j + u * kBlock;
                jj = jj < jlast ? jj : jlast;
                cc[u] = multi_ld<NT>(col + jj);
                v[u] = multi_ld<NT>(val + jj);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int jj = j + u * kBlock;
                if (jj < j1) {
                    scol[jj - j0] = cc[u];
                    sval[jj - j0] = v[u];
                }
            }
        }
        __syncthreads();
        for (int rb = r0; rb < r1; rb += RP) {
            const int row = rb + rl;
            if (row < r1) {
                const int s = rowptr[row] - j0, e = rowptr[row + 1] - j0;
                const size_t i = (size_t)row * W + c;
                const d2m bi = need_b ? *reinterpret_cast<const d2m *>(a.b + i) : zero;
                const d2m xi = need_xi ? *reinterpret_cast<const d2m *>(x + i) : zero;
                const double di = OP == OP_JACOBI ? a.d[row] : 1.0;
                d2m sum = zero;
                for (int k = s; k < e; k += 4) {  // four (col, val) pairs and their gathers in flight, the adds stay sequential
                    int cc[4];
                    double v[4];
                    d2m xv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int kk = k + u < e ? k + u : e - 1;
                        cc[u] = scol[kk];
                        v[u] = sval[kk];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) xv[u] = (k + u < e) ? *reinterpret_cast<const d2m *>(x + (size_t)cc[u] * W + c) : zero;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const double t0 = v[u] * xv[u].x, t1 = v[u] * xv[u].y;
                        sum.x = (k + u < e) ? sum.x + t0 : sum.x;
                        sum.y = (k + u < e) ? sum.y + t1 : sum.y;
                    }
                }
                const d2m t = multi_epilogue<W, OP>(a, row, c, sum, bi, xi, di);
                acc.x += t.x;
                acc.y += t.y;
            }
        }
    }
    if constexpr (OP == OP_SPMV_DOT) {
        __syncthreads();
        const double t = column_pair_block_sum<W>(acc.x, acc.y, red);
        if (tid < W) a.partial[(size_t)tid * nblk + bid] = t;
    }
}


// ------------------------------------------------------------------ layout

// v[i * W + c] = B[c * ld + i] for c < nrhs, 0 in the padding columns
__global__ __launch_bounds__(kBlock) void interleave_kernel(int n, int nrhs, int W, const double *__restrict__ B, long ld, double *__restrict__ v)
{
    const size_t total = (size_t)n * W;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        const size_t row = i / W;
        const int c = (int)(i % W);
        v[i] = c < nrhs ? B[(size_t)c * ld + row] : 0.0;
    }
}

// X[c * ld + i] = v[i * W + c] for c < nrhs
__global__ __launch_bounds__(kBlock) void deinterleave_kernel(int n, int nrhs, int W, const double *__restrict__ v, double *__restrict__ X, long ld)
{
    const size_t total = (size_t)n * nrhs;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        const size_t c = i / n, row = i % n;
        X[c * ld + row] = v[row * W + c];
    }
}

// ------------------------------------------------------------------ cycle

// jacobi_zero_kernel per column: x = omega * b / d (d == nullptr: the constant diagonal dconst)
__global__ __launch_bounds__(kBlock) void jacobi_zero_multi_kernel(int n, int W, const double *__restrict__ b, const double *__restrict__ d,
                                                                    double dconst, double omega, double *__restrict__ x)
{
    const size_t total = (size_t)n * W;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock)
        x[i] = omega * b[i] / (d ? d[i / W] : dconst);
}

// prolong_agg_kernel per column
__global__ __launch_bounds__(kBlock) void prolong_agg_multi_kernel(int n, int W, const int *__restrict__ agg, const double *__restrict__ xc,
                                                                    double *__restrict__ xf)
{
    const size_t total = (size_t)n * W;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        const size_t row = i / W, c = i % W;
        xf[i] = 1.0 * xc[(size_t)agg[row] * W + c] + xf[i];
    }
}

// restrict_agg_kernel per column: the members of aggregate J added in stored order
__global__ __launch_bounds__(kBlock) void restrict_agg_multi_kernel(int nc, int W, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                                     const double *__restrict__ r, double *__restrict__ bc)
{
    const size_t total = (size_t)nc * W;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        const size_t J = i / W, c = i % W;
        const int j0 = rowptr[J], j1 = rowptr[J + 1];
        double sum = 0.0;
        for (int j = j0; j < j1; ++j) sum = sum + r[(size_t)col[j] * W + c];
        bc[i] = sum;
    }
}

// gemv_kernel for W columns: one wave per row of the inverse, which is read once; every column keeps gemv_kernel's order of
// additions (lane l takes the entry pairs 2l, 2l + 128, ..., lane 0 the odd last entry, then the same shuffle tree)
template <int W>
__global__ __launch_bounds__(kBlock) void gemv_multi_kernel(int n, const double *__restrict__ M, const double *__restrict__ b, double *__restrict__ x)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= n) return;  // whole wave leaves
    const double *__restrict__ m = M + (size_t)row * n;
    double acc[W];
#pragma unroll
    for (int c = 0; c < W; ++c) acc[c] = 0.0;
    const int n2 = n & ~1;
    for (int j = lane * 2; j < n2; j += 128) {
        const double m0 = m[j], m1 = m[j + 1];
        const double *b0 = b + (size_t)j * W;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            acc[c] += m0 * b0[c];
            acc[c] += m1 * b0[W + c];
        }
    }
    if (lane == 0 && n2 < n) {
#pragma unroll
        for (int c = 0; c < W; ++c) acc[c] += m[n2] * b[(size_t)n2 * W + c];
    }
#pragma unroll
    for (int c = 0; c < W; ++c) {
        const double s = wave_sum_down(acc[c]);
        if (lane == 0) x[(size_t)row * W + c] = s;
    }
}

// ------------------------------------------------------------------ block PCG

// partial[c * gridDim + workgroup] = this workgroup's share of x_c . y_c (the grid stride is a multiple of W: a thread stays in its column)
template <int W>
__global__ __launch_bounds__(kBlock) void dot_multi_kernel(int n, const double *__restrict__ x, const double *__restrict__ y, double *__restrict__ partial)
{
    __shared__ double red[(kBlock / 64) * kMultiMax];
    const size_t total = (size_t)n * W;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) acc += x[i] * y[i];
    const double t = column_block_sum<W>(acc, red);
    if (threadIdx.x < W) partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
}

// x += alpha_c p ; r += (-alpha_c) Ap ; partials of r.r.  A frozen column's x and r are not written (predicated, so nothing of a
// NaN in its p or alpha reaches them)
template <int W>
__global__ __launch_bounds__(kBlock) void cg_update_multi_kernel(int n, MultiState s, const double *__restrict__ p, const double *__restrict__ Ap,
                                                                  double *__restrict__ x, double *__restrict__ r, double *__restrict__ partial)
{
    __shared__ double red[(kBlock / 64) * kMultiMax];
    const int c = threadIdx.x % W;
    const double alpha = s.scal[MS_ALPHA * kMultiMax + c], nalpha = s.scal[MS_NALPHA * kMultiMax + c];
    const bool live = s.frozen[c] == 0;
    const size_t total = (size_t)n * W;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        double ri = r[i];
        if (live) {
            x[i] = x[i] + alpha * p[i];
            ri = ri + nalpha * Ap[i];
            r[i] = ri;
        }
        acc += ri * ri;
    }
    const double t = column_block_sum<W>(acc, red);
    if (threadIdx.x < W) partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
}

// p = 1.0 z + beta_c p on the columns that are not frozen
template <int W>
__global__ __launch_bounds__(kBlock) void p_update_multi_kernel(int n, MultiState s, const double *__restrict__ z, double *__restrict__ p)
{
    const int c = threadIdx.x % W;
    const double beta = s.scal[MS_BETA * kMultiMax + c];
    if (s.frozen[c] != 0) return;
    const size_t total = (size_t)n * W;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) p[i] = 1.0 * z[i] + beta * p[i];
}

// One workgroup: wave (a, c) adds array a's partials of column c in a fixed order, then thread c applies `code` to column c.
constexpr int kMultiFinBlock = 1024;

__global__ __launch_bounds__(kMultiFinBlock) void finalize_multi_kernel(int code, int W, int nrhs, const double *__restrict__ p0, int n0,
                                                                         const double *__restrict__ p1, int n1, MultiState s, int slot,
                                                                         double tol, double *__restrict__ hist, int hist_cap, int it)
{
    __shared__ double sums[2][kMultiMax];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int arr = w >> 3, c = w & 7;
    if (c < W && (arr == 0 || p1)) {
        const double *p = arr == 0 ? p0 + (size_t)c * n0 : p1 + (size_t)c * n1;
        const int n = arr == 0 ? n0 : n1;
        double v = 0.0;
        for (int i = lane; i < n; i += 64) v += p[i];
        v = wave_sum_down(v);
        if (lane == 0) sums[arr][c] = v;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= W) return;
    const double s0 = sums[0][t];
    double *sc = s.scal;
    auto freeze_on = [&](double res, int iters) {  // ||r|| <= tol: converged; NaN: numeric failure; the column is never written again
        if (res <= tol || !(res == res)) {
            s.frozen[t] = 1;
            s.iters[t] = iters;
            s.status[t] = (res == res) ? 0 : kMultiStatusNumeric;
        }
    };
    switch (code) {
    case MFIN_STORE: sc[slot * kMultiMax + t] = s0; break;
    case MFIN_INIT: {  // ||r0||, and the columns that start frozen: the padding and those already at tol
        const double res = sqrt(s0);
        sc[MS_RES * kMultiMax + t] = res;
        s.frozen[t] = 0;
        s.iters[t] = 0;
        s.status[t] = 0;
        if (t >= nrhs) s.frozen[t] = 1;
        else freeze_on(res, 0);
    } break;
    case MFIN_ALPHA: {  // FIN_PCG_ALPHA
        sc[MS_PAP * kMultiMax + t] = s0;
        const double alpha = sc[MS_RZ * kMultiMax + t] / s0;
        sc[MS_ALPHA * kMultiMax + t] = alpha;
        sc[MS_NALPHA * kMultiMax + t] = -alpha;
    } break;
    case MFIN_BETA_RES: {  // FIN_PCG_BETA_RES
        sc[MS_BETA * kMultiMax + t] = s0 / sc[MS_RZ * kMultiMax + t];
        sc[MS_RZ * kMultiMax + t] = s0;
        if (s.frozen[t] == 0) {
            const double res = sqrt(sums[1][t]);
            sc[MS_RES * kMultiMax + t] = res;
            if (hist && it < hist_cap) hist[(size_t)t * hist_cap + it] = res;
            s.iters[t] = it + 1;
            freeze_on(res, it + 1);
        }
    } break;
    default: break;
    }
}

template <int W, bool NT>
int launch_csr_multi_w(const DevCsr &A, CsrOp op, const MultiArgs &a, int remap, hipStream_t st)
{
    if (A.nblk <= 0) return 0;
    const int4 *rec = reinterpret_cast<const int4 *>(A.rowblk);
    const dim3 grid(multi_remap_grid(A.nblk, remap)), block(kBlock);
    switch (op) {
    case OP_SPMV: hipLaunchKernelGGL((csr_multi_kernel<W, OP_SPMV, NT>), grid, block, 0, st, rec, A.nblk, remap, A.rowptr, A.col, A.val, a); break;
    case OP_SPMV_DOT: hipLaunchKernelGGL((csr_multi_kernel<W, OP_SPMV_DOT, NT>), grid, block, 0, st, rec, A.nblk, remap, A.rowptr, A.col, A.val, a); break;
    case OP_RESID: hipLaunchKernelGGL((csr_multi_kernel<W, OP_RESID, NT>), grid, block, 0, st, rec, A.nblk, remap, A.rowptr, A.col, A.val, a); break;
    case OP_JACOBI: hipLaunchKernelGGL((csr_multi_kernel<W, OP_JACOBI, NT>), grid, block, 0, st, rec, A.nblk, remap, A.rowptr, A.col, A.val, a); break;
    case OP_ADD: hipLaunchKernelGGL((csr_multi_kernel<W, OP_ADD, NT>), grid, block, 0, st, rec, A.nblk, remap, A.rowptr, A.col, A.val, a); break;
    default: return 0;
    }
    return A.nblk;
}


}  // namespace

// dispatch on the width: W is 2, 4 or 8 (multi_width)
#define MULTI_DISPATCH(W, CALL) \
    switch (W) {                \
    case 2: { constexpr int kW = 2; CALL; } break; \
    case 4: { constexpr int kW = 4; CALL; } break; \
    default: { constexpr int kW = 8; CALL; } break; \
    }

void multi_placement(const DevCsr &A, int W, const KernelConfig &cfg, bool *nt, int *remap)
{
    *nt = cfg.nt;
    *remap = cfg.remap;
    if (cfg.auto_policy) {
        // the rule of csr_placement on what one block sweep streams: beyond the memory-side cache the matrix goes past the caches and
        // all XCDs walk one neighbourhood (groups of 16 row blocks); below it one contiguous eighth of the row blocks per XCD
        const size_t bytes = (size_t)A.nnz * 12 + (size_t)A.nrow * (12 + 24 * (size_t)W);
        *nt = bytes > ((size_t)240 << 20);
        *remap = *nt ? 16 : 1;
    }
}

int launch_csr_multi(const DevCsr &A, int W, CsrOp op, const MultiArgs &a, hipStream_t st, const KernelConfig &cfg)
{
    bool nt;
    int remap;
    multi_placement(A, W, cfg, &nt, &remap);
    int nb = 0;
    if (nt) {
        MULTI_DISPATCH(W, nb = (launch_csr_multi_w<kW, true>(A, op, a, remap, st)));
    } else {
        MULTI_DISPATCH(W, nb = (launch_csr_multi_w<kW, false>(A, op, a, remap, st)));
    }
    return nb;
}

void launch_interleave(int n, int nrhs, int W, const double *B, long ld, double *v, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(interleave_kernel, dim3(multi_grid((size_t)n * W)), dim3(kBlock), 0, st, n, nrhs, W, B, ld, v);
}

void launch_deinterleave(int n, int nrhs, int W, const double *v, double *X, long ld, hipStream_t st)
{
    if (n <= 0 || nrhs <= 0) return;
    hipLaunchKernelGGL(deinterleave_kernel, dim3(multi_grid((size_t)n * nrhs)), dim3(kBlock), 0, st, n, nrhs, W, v, X, ld);
}

void launch_jacobi_zero_multi(int n, int W, const double *b, const double *d, double dconst, double omega, double *x, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(jacobi_zero_multi_kernel, dim3(multi_grid((size_t)n * W)), dim3(kBlock), 0, st, n, W, b, d, dconst, omega, x);
}

void launch_prolong_agg_multi(int n, int W, const int *agg, const double *xc, double *xf, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(prolong_agg_multi_kernel, dim3(multi_grid((size_t)n * W)), dim3(kBlock), 0, st, n, W, agg, xc, xf);
}

void launch_restrict_agg_multi(int nc, int W, const int *rowptr, const int *col, const double *r, double *bc, hipStream_t st)
{
    if (nc <= 0) return;
    hipLaunchKernelGGL(restrict_agg_multi_kernel, dim3(multi_grid((size_t)nc * W)), dim3(kBlock), 0, st, nc, W, rowptr, col, r, bc);
}

void launch_gemv_multi(int n, int W, const double *M, const double *b, double *x, hipStream_t st)
{
    if (n <= 0) return;
    const dim3 grid((n + kBlock / 64 - 1) / (kBlock / 64)), block(kBlock);
    MULTI_DISPATCH(W, hipLaunchKernelGGL(gemv_multi_kernel<kW>, grid, block, 0, st, n, M, b, x));
}

int launch_dot_multi(int n, int W, const double *x, const double *y, double *partial, hipStream_t st)
{
    const int g = multi_grid((size_t)n * W);
    MULTI_DISPATCH(W, hipLaunchKernelGGL(dot_multi_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, x, y, partial));
    return g;
}

int launch_cg_update_multi(int n, int W, const MultiState &s, const double *p, const double *Ap, double *x, double *r, double *partial,
                           hipStream_t st)
{
    const int g = multi_grid((size_t)n * W);
    MULTI_DISPATCH(W, hipLaunchKernelGGL(cg_update_multi_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, s, p, Ap, x, r, partial));
    return g;
}

void launch_p_update_multi(int n, int W, const MultiState &s, const double *z, double *p, hipStream_t st)
{
    const int g = multi_grid((size_t)n * W);
    MULTI_DISPATCH(W, hipLaunchKernelGGL(p_update_multi_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, s, z, p));
}

void launch_finalize_multi(MultiFin code, int W, int nrhs, const double *p0, int n0, const double *p1, int n1, const MultiState &s, int slot,
                           double tol, double *hist, int hist_cap, int it, hipStream_t st)
{
    hipLaunchKernelGGL(finalize_multi_kernel, dim3(1), dim3(kMultiFinBlock), 0, st, (int)code, W, nrhs, p0, n0, p1, n1, s, slot, tol, hist,
                       hist_cap, it);
}

}  // namespace sparsh
