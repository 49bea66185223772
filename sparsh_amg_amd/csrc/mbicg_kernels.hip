// mbicg_kernels.hip -- the kernels of block BiCGStab: two sums per column from one pass, the half step
// S = R - alpha AP, the update of X and R with the partial sums of the next two scalars, the direction update and the finalise.
//
// Storage is that of multi_kernels.hip: a block of W vectors (W = 2, 4 or 8) is row-interleaved, element (row i, column c) at
// v[i * W + c], 16-byte aligned; every access is a 16-byte load or store of two neighbouring columns.  In the two launches without a
// reduction (S, P) a lane owns two neighbouring columns of one row of a pass over 512 / W rows, the W / 2 lanes of a row side by side
// in one wave; in the two with one (dot2, X / R) a lane owns a whole row, W / 2 such accesses.  Every launch is a grid-stride loop
// of at most kMultiGridMax workgroups over the rows.
//
// Arithmetic contract, per column, that of bicg_s_kernel / bicg_xr_kernel / bicg_p_kernel and of FIN_BICG_ALPHA / OMEGA / BETA
// (kernels.hip), parentheses included; every product and every sum is rounded on its own (-ffp-contract=off).  Columns never meet:
// every scalar is read per column from the device state, and every store to a column whose `frozen` flag is set is predicated off,
// so a frozen column keeps its bits whatever its scalars hold.  Reductions: one partial per column and workgroup at
// partial[c * gridDim.x + workgroup], added by the one-workgroup finalise; per column the terms are added in the order of the
// single-vector kernels (dot2_kernel, bicg_xr_kernel, finalize_kernel), so the sums do not depend on the width and a column's
// scalars are those of a single solve of that column bit for bit.  No atomics.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sparsh {

namespace {

using d2q = double __attribute__((ext_vector_type(2)));

__device__ __forceinline__ d2q mb_ld(const double *p) { return *reinterpret_cast<const d2q *>(p); }

// the store of a lane's two columns, each under its own flag
__device__ __forceinline__ void mb_st(double *p, d2q v, bool live0, bool live1)
{
    if (live0 && live1) *reinterpret_cast<d2q *>(p) = v;
    else if (live0) p[0] = v.x;
    else if (live1) p[1] = v.y;
}

__device__ __forceinline__ double mb_wave_sum_down(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// The reducing launches give a lane one whole row of the block (W / 2 loads of 16 bytes; a wave covers 64 consecutive rows, W * 512
// contiguous bytes): column c's terms then meet in exactly the order of the single-vector kernels (dot2_kernel, bicg_xr_kernel: thread
// t of workgroup w adds the rows 256 w + t, + 256 g, ... from +0.0, the shuffle tree per wave, the four waves in order), so a column of
// a block takes the single solve's alpha, omega and beta bit for bit whatever the width.  red holds 2 * (kBlock / 64) * W doubles.
template <int W>
__device__ __forceinline__ void mb_store_partials(double (&a0)[W], double (&a1)[W], double *red, double *__restrict__ part0,
                                                  double *__restrict__ part1)
{
    constexpr int NW = kBlock / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        const double t0 = mb_wave_sum_down(a0[c]), t1 = mb_wave_sum_down(a1[c]);
        if (lane == 0) {
            red[w * W + c] = t0;
            red[(NW + w) * W + c] = t1;
        }
    }
    __syncthreads();
    if (threadIdx.x < W) {
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            s0 += red[k * W + threadIdx.x];
            s1 += red[(NW + k) * W + threadIdx.x];
        }
        part0[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s0;
        part1[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s1;
    }
}

// part0: shares of a_c . b_c ; part1: shares of c_c . d_c.  The four blocks may be one another (nothing is written to them).
template <int W>
__global__ __launch_bounds__(kBlock) void dot2_multi_kernel(int n, const double *a, const double *b, const double *c, const double *d,
                                                             double *__restrict__ part0, double *__restrict__ part1)
{
    __shared__ double red[2 * (kBlock / 64) * W];
    double a0[W], a1[W];
#pragma unroll
    for (int j = 0; j < W; ++j) a0[j] = a1[j] = 0.0;
    for (size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x; row < (size_t)n; row += (size_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < W; j += 2) {
            const size_t i = row * W + j;
            const d2q av = mb_ld(a + i), bv = mb_ld(b + i), cv = mb_ld(c + i), dv = mb_ld(d + i);
            a0[j] += av.x * bv.x;
            a0[j + 1] += av.y * bv.y;
            a1[j] += cv.x * dv.x;
            a1[j + 1] += cv.y * dv.y;
        }
    }
    mb_store_partials<W>(a0, a1, red, part0, part1);
}

// S = R - alpha_c AP on the columns that are not frozen
template <int W>
__global__ __launch_bounds__(kBlock) void bicg_s_multi_kernel(int n, MbicgState st, const double *__restrict__ R, const double *__restrict__ AP,
                                                               double *__restrict__ S)
{
    constexpr int LPR = W / 2;
    constexpr int RP = kBlock / LPR;
    const int j = 2 * (threadIdx.x % LPR);
    const bool live0 = st.frozen[j] == 0, live1 = st.frozen[j + 1] == 0;
    if (!live0 && !live1) return;
    const double al0 = st.scal[MB_ALPHA * kMultiMax + j], al1 = st.scal[MB_ALPHA * kMultiMax + j + 1];
    for (size_t row = (size_t)blockIdx.x * RP + threadIdx.x / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const size_t i = row * W + j;
        const d2q r = mb_ld(R + i), ap = mb_ld(AP + i);
        d2q s;
        s.x = r.x - al0 * ap.x;
        s.y = r.y - al1 * ap.y;
        mb_st(S + i, s, live0, live1);
    }
}

// X = (X + alpha_c P1) + omega_c S1 ; R = S - omega_c AS on the columns that are not frozen ; part0: shares of R_c . R0_c ; part1:
// shares of R_c . R_c (a frozen column's shares are those of the R it keeps; its finalise is predicated off as well).  A lane owns a
// row, as in dot2_multi_kernel.
template <int W>
__global__ __launch_bounds__(kBlock) void bicg_xr_multi_kernel(int n, MbicgState st, const double *__restrict__ P1, const double *__restrict__ S1,
                                                                const double *__restrict__ S, const double *__restrict__ AS,
                                                                const double *__restrict__ R0, double *__restrict__ X, double *__restrict__ R,
                                                                double *__restrict__ part0, double *__restrict__ part1)
{
    __shared__ double red[2 * (kBlock / 64) * W];
    double a0[W], a1[W], al[W], om[W];
    bool live[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        a0[j] = a1[j] = 0.0;
        al[j] = st.scal[MB_ALPHA * kMultiMax + j];
        om[j] = st.scal[MB_OMEGA1 * kMultiMax + j];
        live[j] = st.frozen[j] == 0;
    }
    for (size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x; row < (size_t)n; row += (size_t)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < W; j += 2) {
            const size_t i = row * W + j;
            d2q r = mb_ld(R + i);
            if (live[j] || live[j + 1]) {
                const d2q x = mb_ld(X + i), p1 = mb_ld(P1 + i), s1 = mb_ld(S1 + i), s = mb_ld(S + i), as = mb_ld(AS + i);
                d2q xn;
                xn.x = (x.x + al[j] * p1.x) + om[j] * s1.x;
                xn.y = (x.y + al[j + 1] * p1.y) + om[j + 1] * s1.y;
                if (live[j]) r.x = s.x - om[j] * as.x;
                if (live[j + 1]) r.y = s.y - om[j + 1] * as.y;
                mb_st(X + i, xn, live[j], live[j + 1]);
                mb_st(R + i, r, live[j], live[j + 1]);
            }
            const d2q r0 = mb_ld(R0 + i);
            a0[j] += r.x * r0.x;
            a0[j + 1] += r.y * r0.y;
            a1[j] += r.x * r.x;
            a1[j + 1] += r.y * r.y;
        }
    }
    mb_store_partials<W>(a0, a1, red, part0, part1);
}

// P = R + beta_c (P - omega_c AP) on the columns that are not frozen
template <int W>
__global__ __launch_bounds__(kBlock) void bicg_p_multi_kernel(int n, MbicgState st, const double *__restrict__ R, const double *__restrict__ AP,
                                                               double *__restrict__ P)
{
    constexpr int LPR = W / 2;
    constexpr int RP = kBlock / LPR;
    const int j = 2 * (threadIdx.x % LPR);
    const bool live0 = st.frozen[j] == 0, live1 = st.frozen[j + 1] == 0;
    if (!live0 && !live1) return;
    const double be0 = st.scal[MB_BETA * kMultiMax + j], be1 = st.scal[MB_BETA * kMultiMax + j + 1];
    const double om0 = st.scal[MB_OMEGA1 * kMultiMax + j], om1 = st.scal[MB_OMEGA1 * kMultiMax + j + 1];
    for (size_t row = (size_t)blockIdx.x * RP + threadIdx.x / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const size_t i = row * W + j;
        const d2q r = mb_ld(R + i), ap = mb_ld(AP + i), p = mb_ld(P + i);
        d2q pn;
        pn.x = r.x + be0 * (p.x - om0 * ap.x);
        pn.y = r.y + be1 * (p.y - om1 * ap.y);
        mb_st(P + i, pn, live0, live1);
    }
}

// One workgroup of 1024 threads.  The partials of every column and array are added in finalize_kernel's order (thread t takes p[t],
// p[t + 1024], ..., the shuffle tree per wave, the sixteen waves in order from +0.0), then thread c applies `code` to column c.  A
// frozen column is left alone by every code but MBFIN_INIT, which starts a solve.
constexpr int kMbicgFinBlock = 1024;

__global__ __launch_bounds__(kMbicgFinBlock) void finalize_mbicg_kernel(int code, int W, int nrhs, const double *__restrict__ p0, int n0,
                                                                         const double *__restrict__ p1, int n1, MbicgState s, double tol,
                                                                         double *__restrict__ hist, int hist_cap, int it)
{
    constexpr int NW = kMbicgFinBlock / 64;
    __shared__ double red[2][kMultiMax][NW];
    __shared__ double sums[2][kMultiMax];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int arr = 0; arr < (p1 ? 2 : 1); ++arr)
        for (int c = 0; c < W; ++c) {
            const double *p = arr == 0 ? p0 + (size_t)c * n0 : p1 + (size_t)c * n1;
            const int n = arr == 0 ? n0 : n1;
            double v = 0.0;
            for (int i = threadIdx.x; i < n; i += kMbicgFinBlock) v += p[i];
            v = mb_wave_sum_down(v);
            if (lane == 0) red[arr][c][w] = v;
        }
    __syncthreads();
    if (threadIdx.x < 2 * kMultiMax) {
        const int arr = threadIdx.x / kMultiMax, c = threadIdx.x % kMultiMax;
        double v = 0.0;
        if (c < W && (arr == 0 || p1))
            for (int k = 0; k < NW; ++k) v += red[arr][c][k];
        sums[arr][c] = v;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= W) return;
    const double s0 = sums[0][t], s1 = p1 ? sums[1][t] : 0.0;
    double *sc = s.scal;
    auto freeze_on = [&](double res, int iters) {  // ||r|| <= tol: converged; NaN: numeric failure; the column is never written again
        if (res <= tol || !(res == res)) {
            s.frozen[t] = 1;
            s.iters[t] = iters;
            s.status[t] = (res == res) ? 0 : kMultiStatusNumeric;
        }
    };
    if (code == MBFIN_INIT) {  // ||r0||, and the columns that start frozen: the padding and those already at tol
        for (int k = 0; k < MB_COUNT; ++k) sc[k * kMultiMax + t] = 0.0;
        const double res = sqrt(s0);
        sc[MB_RES * kMultiMax + t] = res;
        s.frozen[t] = 0;
        s.iters[t] = 0;
        s.status[t] = 0;
        if (t >= nrhs) s.frozen[t] = 1;
        else freeze_on(res, 0);
        return;
    }
    if (s.frozen[t] != 0) return;
    switch (code) {
    case MBFIN_ALPHA: {  // FIN_BICG_ALPHA: s0 = r.r0, s1 = Ap.r0
        sc[MB_ALPHA1 * kMultiMax + t] = s0;
        sc[MB_APR0 * kMultiMax + t] = s1;
        sc[MB_ALPHA * kMultiMax + t] = s0 / s1;
    } break;
    case MBFIN_OMEGA: {  // FIN_BICG_OMEGA: s0 = As.s, s1 = As.As; s = 0 after the half step gives omega = 0 as in the single loop
        sc[MB_ASS * kMultiMax + t] = s0;
        sc[MB_ASAS * kMultiMax + t] = s1;
        sc[MB_OMEGA1 * kMultiMax + t] = (s1 == 0.0) ? 0.0 : s0 / s1;
    } break;
    case MBFIN_BETA_RES: {  // FIN_BICG_BETA: s0 = r.r0, s1 = r.r
        double beta = s0 / sc[MB_ALPHA1 * kMultiMax + t];
        beta = beta * (sc[MB_ALPHA * kMultiMax + t] / sc[MB_OMEGA1 * kMultiMax + t]);
        sc[MB_BETA * kMultiMax + t] = beta;
        sc[MB_RR0 * kMultiMax + t] = s0;
        const double res = sqrt(s1);
        sc[MB_RES * kMultiMax + t] = res;
        if (hist && it < hist_cap) hist[(size_t)t * hist_cap + it] = res;
        s.iters[t] = it + 1;
        freeze_on(res, it + 1);
    } break;
    default: break;
    }
}

}  // namespace

#define MBICG_DISPATCH(W, CALL) \
    switch (W) {                \
    case 2: { constexpr int kW = 2; CALL; } break; \
    case 4: { constexpr int kW = 4; CALL; } break; \
    default: { constexpr int kW = 8; CALL; } break; \
    }

int mbicg_grid(int n, int W)
{
    const int rp = kBlock / (W / 2);
    const long g = ((long)n + rp - 1) / rp;
    return g < 1 ? 1 : (g > kMultiGridMax ? kMultiGridMax : (int)g);
}

// the grid of the single-vector elementwise launches (ew_grid): a lane owns a row
int mbicg_reduce_grid(int n)
{
    const long g = ((long)n + 2 * kBlock - 1) / (2 * kBlock);
    return g < 1 ? 1 : (g > kMultiGridMax ? kMultiGridMax : (int)g);
}

int launch_dot2_multi(int n, int W, const double *a, const double *b, const double *c, const double *d, double *part0, double *part1,
                      hipStream_t st)
{
    const int g = mbicg_reduce_grid(n);
    MBICG_DISPATCH(W, hipLaunchKernelGGL(dot2_multi_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, a, b, c, d, part0, part1));
    return g;
}

void launch_bicg_s_multi(int n, int W, const MbicgState &s, const double *R, const double *AP, double *S, hipStream_t st)
{
    const int g = mbicg_grid(n, W);
    MBICG_DISPATCH(W, hipLaunchKernelGGL(bicg_s_multi_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, s, R, AP, S));
}

int launch_bicg_xr_multi(int n, int W, const MbicgState &s, const double *P1, const double *S1, const double *S, const double *AS,
                         const double *R0, double *X, double *R, double *part0, double *part1, hipStream_t st)
{
    const int g = mbicg_reduce_grid(n);
    MBICG_DISPATCH(W, hipLaunchKernelGGL(bicg_xr_multi_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, s, P1, S1, S, AS, R0, X, R, part0, part1));
    return g;
}

void launch_bicg_p_multi(int n, int W, const MbicgState &s, const double *R, const double *AP, double *P, hipStream_t st)
{
    const int g = mbicg_grid(n, W);
    MBICG_DISPATCH(W, hipLaunchKernelGGL(bicg_p_multi_kernel<kW>, dim3(g), dim3(kBlock), 0, st, n, s, R, AP, P));
}

void launch_finalize_mbicg(MbicgFin code, int W, int nrhs, const double *p0, int n0, const double *p1, int n1, const MbicgState &s, double tol,
                           double *hist, int hist_cap, int it, hipStream_t st)
{
    hipLaunchKernelGGL(finalize_mbicg_kernel, dim3(1), dim3(kMbicgFinBlock), 0, st, (int)code, W, nrhs, p0, n0, p1, n1, s, tol, hist, hist_cap,
                       it);
}

}  // namespace sparsh
