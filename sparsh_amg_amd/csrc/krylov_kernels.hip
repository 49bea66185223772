// krylov_kernels.hip -- device code of restarted GMRES (Engine::gmres): block Gram-Schmidt against the Krylov basis and the
// small kernels that keep the Hessenberg column, the Givens rotations, g and y in device memory.
//
// The basis is m + 1 vectors of `stride` elements each, v_k = V + k * stride.  Orthogonalising w against v_0..v_{nv-1} is
//   gs_dot         partial[k][blk] = sum over the workgroup's rows of v_k[i] * w[i]            (one pass over V and w)
//   gs_finalize    h[k] = sum of partial[k][*] in a fixed order                                 (one workgroup per k)
//   gs_update      w[i] = w[i] - h_0 v_0[i] - ... - h_{nv-1} v_{nv-1}[i], k ascending, and in the same pass the partial sums
//                  of v_k . w_new and of w_new . w_new
// Every thread keeps K partial sums in registers; K is a compile-time chunk (4, 8 or 16, the smallest that holds nv; at 32 the
// K + 1 sums and K loaded values no longer fit the 128 registers that four waves per SIMD leave a thread, and the compiler spills).  More
// than kGsMaxK vectors take several launches.  No atomics: per-workgroup partials, added in a fixed order, so two runs agree
// bitwise.  Products and subtractions round separately (-ffp-contract=off), like every other kernel of the library.
//
// The kernels are templates on the element type of the basis.  double: one row per thread and grid-stride step.  float
// (SPARSH_BASIS_FP32): the stride is a multiple of 4 floats with zeros behind row n, a thread takes 4 consecutive rows (2 at K = 16)
// with one float4 / float2 load per basis vector and double2 loads of w; every stored value is widened to double before it is used,
// so all products and sums are fp64 and the order per row (k ascending) is that of the double kernels.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.hpp"

namespace sparsh {

namespace {

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

constexpr int kWaves = kBlock / 64;

// sums[k] of every wave -> red[wave][k]; after the barrier thread k adds the kWaves entries of sum k in wave order.
// Sum k of the workgroup is returned in thread k (k < count); other threads return 0.
template <int NS>
__device__ __forceinline__ double block_sums(const double (&acc)[NS], int count, double (*red)[NS])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        if (k < count) {
            const double t = wave_sum(acc[k]);
            if (lane == 0) red[w][k] = t;
        }
    }
    __syncthreads();
    double s = 0.0;
    if ((int)threadIdx.x < count) {
#pragma unroll
        for (int q = 0; q < kWaves; ++q) s += red[q][threadIdx.x];
    }
    return s;
}

// Rows a thread handles per grid-stride step.  double basis: 1.  float basis: 4 consecutive rows while K <= 8 and 2 at K = 16, so
// that a basis vector is read with one 16- or 8-byte load per thread and w with double2 loads.
template <typename T, int K>
constexpr int kGsRows = sizeof(T) == 8 ? 1 : (K <= 8 ? 4 : 2);
// (an int row index would wrap in `i += step` within R * gridDim.x * kBlock rows of 2^31)
template <int R>
using gs_index = std::conditional_t<R == 1, int, long>;

// R consecutive stored values of one basis vector from row i, a multiple of R.  The float basis has a stride that is a multiple of
// 4 and zeros behind row n, so the vector load of the last group stays inside the vector and brings zeros.
template <int R>
__device__ __forceinline__ void load_basis(const double *__restrict__ v, long i, double (&out)[R])
{
    static_assert(R == 1, "a double basis is read row by row");
    out[0] = v[i];
}
template <int R>
__device__ __forceinline__ void load_basis(const float *__restrict__ v, long i, float (&out)[R])
{
    static_assert(R == 2 || R == 4, "float2 or float4");
    if constexpr (R == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(v + i);
        out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.w;
    } else {
        const float2 q = *reinterpret_cast<const float2 *>(v + i);
        out[0] = q.x, out[1] = q.y;
    }
}

// rows i .. i + R - 1 of a vector of n doubles (16-byte aligned, i a multiple of R): double2 loads on a full group, row by row and
// 0 for the rows past n on the last one
template <int R>
__device__ __forceinline__ void load_rows(const double *p, long i, int n, double (&out)[R])
{
    if constexpr (R == 1) {
        out[0] = p[i];
    } else if (i + R <= n) {
#pragma unroll
        for (int r = 0; r < R; r += 2) {
            const double2 q = *reinterpret_cast<const double2 *>(p + i + r);
            out[r] = q.x, out[r + 1] = q.y;
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) out[r] = i + r < n ? p[i + r] : 0.0;
    }
}
template <int R>
__device__ __forceinline__ void store_rows(double *p, long i, int n, const double (&s)[R])
{
    if constexpr (R == 1) {
        p[i] = s[0];
    } else if (i + R <= n) {
#pragma unroll
        for (int r = 0; r < R; r += 2) *reinterpret_cast<double2 *>(p + i + r) = make_double2(s[r], s[r + 1]);
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (i + r < n) p[i + r] = s[r];
    }
}

// partial[k * gridDim.x + blockIdx.x] = sum over this workgroup's rows of v_k[i] * w[i], k < nv <= K;
// ww_partial[blockIdx.x] = the same of w[i] * w[i] (nullptr: not wanted).  T = float: the stored value widened to double, fp64 sums.
template <typename T, int K>
__global__ __launch_bounds__(kBlock, 4) void gs_dot_kernel(int n, long stride, const T *__restrict__ V, int nv,
                                                            const double *__restrict__ w, double *__restrict__ partial,
                                                            double *__restrict__ ww_partial)
{
    constexpr int R = kGsRows<T, K>;
    using I = gs_index<R>;
    __shared__ double red[kWaves][K + 1];
    double acc[K + 1];
#pragma unroll
    for (int k = 0; k <= K; ++k) acc[k] = 0.0;
    for (I i = (I)(blockIdx.x * kBlock + threadIdx.x) * R; i < n; i += (I)(gridDim.x * kBlock) * R) {
        double wi[R];
        load_rows<R>(w, i, n, wi);
        T v[K][R];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k < nv) {
                load_basis<R>(V + (long)k * stride, i, v[k]);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) v[k][r] = 0;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += (double)v[k][r] * wi[r];
            acc[K] += wi[r] * wi[r];
        }
    }
    if (ww_partial) {  // w.w rides as sum number nv
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (k == nv) acc[k] = acc[K];
    }
    const int count = ww_partial ? nv + 1 : nv;
    const double s = block_sums<K + 1>(acc, count, red);
    const int t = threadIdx.x;
    if (t < nv) partial[(long)t * gridDim.x + blockIdx.x] = s;
    else if (t == nv && ww_partial) ww_partial[blockIdx.x] = s;
}

// w_out[i] = s, s = w_in[i] (0 when w_in == nullptr), then s = s - h[k] * v_k[i] for k = 0..nv-1 in that order.
// DOTS: partial[k * gridDim.x + blockIdx.x] = workgroup sum of v_k[i] * s.  ww_partial (may be nullptr): of s * s.
// w_in and w_out may be the same vector; neither may be one of v_0..v_{nv-1}.
template <typename T, int K, bool DOTS>
__global__ __launch_bounds__(kBlock, 4) void gs_update_kernel(int n, long stride, const T *__restrict__ V, int nv,
                                                               const double *__restrict__ h, const double *w_in, double *w_out,
                                                               double *__restrict__ partial, double *__restrict__ ww_partial)
{
    constexpr int R = kGsRows<T, K>;
    using I = gs_index<R>;
    constexpr int NS = DOTS ? K + 1 : 1;
    __shared__ double red[kWaves][NS];
    double hk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) hk[k] = k < nv ? h[k] : 0.0;
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    double ww = 0.0;
    for (I i = (I)(blockIdx.x * kBlock + threadIdx.x) * R; i < n; i += (I)(gridDim.x * kBlock) * R) {
        double s[R];
        if (w_in) {
            load_rows<R>(w_in, i, n, s);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) s[r] = 0.0;
        }
        T v[K][R];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k < nv) {
                load_basis<R>(V + (long)k * stride, i, v[k]);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) v[k][r] = 0;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int k = 0; k < K; ++k) s[r] = s[r] - hk[k] * (double)v[k][r];  // (k >= nv: s - 0 * 0 == s)
        }
        store_rows<R>(w_out, i, n, s);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (DOTS) {
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] += (double)v[k][r] * s[r];
            }
            ww += s[r] * s[r];  // (rows past n: 0)
        }
    }
    if constexpr (DOTS) {
        const bool want_ww = ww_partial != nullptr;
#pragma unroll
        for (int k = 0; k <= K; ++k)
            if (k == nv) acc[k] = ww;
        const double s = block_sums<NS>(acc, want_ww ? nv + 1 : nv, red);
        const int t = threadIdx.x;
        if (t < nv) partial[(long)t * gridDim.x + blockIdx.x] = s;
        else if (t == nv && want_ww) ww_partial[blockIdx.x] = s;
    } else if (ww_partial) {
        acc[0] = ww;
        const double s = block_sums<NS>(acc, 1, red);
        if (threadIdx.x == 0) ww_partial[blockIdx.x] = s;
    }
}

// sum of p[0, n) by one workgroup of kBlock threads in a fixed order; valid in thread 0
__device__ __forceinline__ double fixed_sum(const double *__restrict__ p, int n, double *red)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) a += p[i];
    a = wave_sum(a);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = a;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int q = 0; q < kWaves; ++q) s += red[q];
    return s;
}

// out[k] = sum of partial[k * nblk .. + nblk): workgroup k
__global__ __launch_bounds__(kBlock) void gs_finalize_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ out)
{
    __shared__ double red[kWaves];
    const double s = fixed_sum(partial + (long)blockIdx.x * nblk, nblk, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// v[i] = w[i] / *d ; *d not > 0 (lucky breakdown): v = 0 and no division.
// T = double: in place (w == v, vd unused), one row per thread.
// T = float: q = w[i] / *d rounded once to float (round to nearest) goes to v[i] and the same rounded value, widened back, to vd[i],
// the fp64 vector the next step feeds to M / A.  Four rows per thread; v has zeros behind row n and keeps them.
template <typename T>
__global__ __launch_bounds__(kBlock) void gs_scale_kernel(int n, const double *w, T *v, double *vd, const double *__restrict__ d)
{
    const double h = *d;
    const bool ok = h > 0.0;
    if constexpr (sizeof(T) == 8) {
        for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) v[i] = ok ? w[i] / h : 0.0;
    } else {
        for (long i = (long)(blockIdx.x * kBlock + threadIdx.x) * 4; i < n; i += (long)(gridDim.x * kBlock) * 4) {
            double x[4];
            load_rows<4>(w, i, n, x);
            float q[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                q[r] = ok ? (float)(x[r] / h) : 0.f;  // (rows past n: 0 / h = 0)
                x[r] = (double)q[r];
            }
            *reinterpret_cast<float4 *>(v + i) = make_float4(q[0], q[1], q[2], q[3]);
            store_rows<4>(vd, i, n, x);
        }
    }
}

// End of inner iteration j, one workgroup: h = hcol + ccol (the two Gram-Schmidt passes), h_{j+1} = sqrt(sum of ww_partial); the j earlier
// rotations are applied to the column, rotation j is formed and applied to g; hist[slot] = |g_{j+1}|.  j == 0 starts a cycle: g = (beta, 0, ..).
__global__ __launch_bounds__(kBlock) void gmres_step_kernel(int j, const double *__restrict__ ww_partial, int nblk, GmresState s,
                                                             const double *__restrict__ beta, double *__restrict__ hist, int slot)
{
    __shared__ double red[kWaves];
    __shared__ double col[kGmresMaxRestart + 1], cs[kGmresMaxRestart], sn[kGmresMaxRestart];
    const int t = threadIdx.x;
    if (t <= j) col[t] = s.hcol[t] + s.ccol[t];
    if (t < j) {
        cs[t] = s.cs[t];
        sn[t] = s.sn[t];
    }
    const double ww = fixed_sum(ww_partial, nblk, red);  // (its barrier also publishes col, cs, sn)
    if (t == 0) {
        const double hn = sqrt(ww);
        *s.hnext = hn;
        for (int k = 0; k < j; ++k) {
            const double a = col[k], b = col[k + 1];
            col[k] = cs[k] * a + sn[k] * b;
            col[k + 1] = cs[k] * b - sn[k] * a;
        }
        const double a = col[j];
        const double d = sqrt(a * a + hn * hn);
        double c = 1.0, z = 0.0;
        if (d != 0.0) {  // (a NaN takes this branch and reaches the history)
            c = a / d;
            z = hn / d;
        }
        col[j] = c * a + z * hn;
        s.cs[j] = c;
        s.sn[j] = z;
        const double gj = j == 0 ? *beta : s.g[j];
        s.g[j] = c * gj;
        const double gn = -z * gj;
        s.g[j + 1] = gn;
        hist[slot] = fabs(gn);
    }
    __syncthreads();
    if (t <= j) s.R[(long)j * kGmresMaxRestart + t] = col[t];
}

// y = R^{-1} g over the first k columns, one wave; ny = -y (the update kernel subtracts).  A zero pivot (a step taken after a
// lucky breakdown) gives y_i = 0.
__global__ __launch_bounds__(64) void gmres_solve_kernel(int k, GmresState s)
{
    const int l = threadIdx.x;
    double yl = 0.0;
    for (int i = k - 1; i >= 0; --i) {
        double t = (l > i && l < k) ? s.R[(long)l * kGmresMaxRestart + i] * yl : 0.0;
        t = wave_sum(t);
        t = __shfl(t, 0, 64);
        const double piv = s.R[(long)i * kGmresMaxRestart + i];
        const double yi = piv != 0.0 ? (s.g[i] - t) / piv : 0.0;
        if (l == i) yl = yi;
    }
    if (l < k) s.ny[l] = -yl;
}

inline int gs_pick(int nv) { return nv <= 4 ? 4 : nv <= 8 ? 8 : 16; }

}  // namespace

int gs_grid(int n)
{
    int g = (n + kBlock * 2 - 1) / (kBlock * 2);
    if (g < 1) g = 1;
    return g > 2048 ? 2048 : g;  // grid-stride beyond ~8 workgroups per CU, as the other element-wise kernels
}

namespace {
template <typename T>
void gs_dot_any(int n, long stride, const T *V, int nv, const double *w, double *partial, double *ww_partial, hipStream_t st)
{
    const int g = gs_grid(n);
    for (int k0 = 0; k0 < nv; k0 += kGsMaxK) {
        const int cnt = nv - k0 < kGsMaxK ? nv - k0 : kGsMaxK;
        double *ww = k0 + cnt == nv ? ww_partial : nullptr;
        const T *Vc = V + (long)k0 * stride;
        double *pc = partial + (long)k0 * g;
        switch (gs_pick(cnt)) {
        case 4: hipLaunchKernelGGL((gs_dot_kernel<T, 4>), dim3(g), dim3(kBlock), 0, st, n, stride, Vc, cnt, w, pc, ww); break;
        case 8: hipLaunchKernelGGL((gs_dot_kernel<T, 8>), dim3(g), dim3(kBlock), 0, st, n, stride, Vc, cnt, w, pc, ww); break;
        default: hipLaunchKernelGGL((gs_dot_kernel<T, 16>), dim3(g), dim3(kBlock), 0, st, n, stride, Vc, cnt, w, pc, ww); break;
        }
    }
}

template <typename T, bool DOTS>
void gs_update_one(int g, int n, long stride, const T *V, int nv, const double *h, const double *w_in, double *w_out, double *partial,
                   double *ww, hipStream_t st)
{
    switch (gs_pick(nv)) {
    case 4: hipLaunchKernelGGL((gs_update_kernel<T, 4, DOTS>), dim3(g), dim3(kBlock), 0, st, n, stride, V, nv, h, w_in, w_out, partial, ww); break;
    case 8: hipLaunchKernelGGL((gs_update_kernel<T, 8, DOTS>), dim3(g), dim3(kBlock), 0, st, n, stride, V, nv, h, w_in, w_out, partial, ww); break;
    default: hipLaunchKernelGGL((gs_update_kernel<T, 16, DOTS>), dim3(g), dim3(kBlock), 0, st, n, stride, V, nv, h, w_in, w_out, partial, ww); break;
    }
}

template <typename T>
void gs_update_any(int n, long stride, const T *V, int nv, const double *h, const double *w_in, double *w_out, double *partial,
                   double *ww_partial, hipStream_t st)
{
    const int g = gs_grid(n);
    if (nv <= kGsMaxK) {
        if (partial) gs_update_one<T, true>(g, n, stride, V, nv, h, w_in, w_out, partial, ww_partial, st);
        else gs_update_one<T, false>(g, n, stride, V, nv, h, w_in, w_out, nullptr, ww_partial, st);
        return;
    }
    // more vectors than one launch holds: update-only launches over ascending chunks (the same subtractions in the same order),
    // then the sums of the finished vector
    for (int k0 = 0; k0 < nv; k0 += kGsMaxK) {
        const int cnt = nv - k0 < kGsMaxK ? nv - k0 : kGsMaxK;
        const bool lastc = k0 + cnt == nv;
        gs_update_one<T, false>(g, n, stride, V + (long)k0 * stride, cnt, h + k0, k0 == 0 ? w_in : w_out, w_out, nullptr,
                                (lastc && !partial) ? ww_partial : nullptr, st);
    }
    if (partial) gs_dot_any(n, stride, V, nv, w_out, partial, ww_partial, st);
}
}  // namespace

void launch_gs_dot(int n, long stride, const double *V, int nv, const double *w, double *partial, double *ww_partial, hipStream_t st)
{
    gs_dot_any(n, stride, V, nv, w, partial, ww_partial, st);
}

void launch_gs_dot(int n, long stride, const float *V, int nv, const double *w, double *partial, double *ww_partial, hipStream_t st)
{
    gs_dot_any(n, stride, V, nv, w, partial, ww_partial, st);
}

void launch_gs_update(int n, long stride, const double *V, int nv, const double *h, const double *w_in, double *w_out, double *partial,
                      double *ww_partial, hipStream_t st)
{
    gs_update_any(n, stride, V, nv, h, w_in, w_out, partial, ww_partial, st);
}

void launch_gs_update(int n, long stride, const float *V, int nv, const double *h, const double *w_in, double *w_out, double *partial,
                      double *ww_partial, hipStream_t st)
{
    gs_update_any(n, stride, V, nv, h, w_in, w_out, partial, ww_partial, st);
}

void launch_gs_finalize(const double *partial, int nblk, int rows, double *out, hipStream_t st)
{
    if (rows <= 0) return;
    hipLaunchKernelGGL(gs_finalize_kernel, dim3(rows), dim3(kBlock), 0, st, partial, nblk, out);
}

void launch_gs_scale(int n, double *v, const double *d, hipStream_t st)
{
    hipLaunchKernelGGL(gs_scale_kernel<double>, dim3(gs_grid(n)), dim3(kBlock), 0, st, n, v, v, nullptr, d);
}

void launch_gs_scale(int n, const double *w, float *v, double *vd, const double *d, hipStream_t st)
{
    hipLaunchKernelGGL(gs_scale_kernel<float>, dim3(gs_grid(n)), dim3(kBlock), 0, st, n, w, v, vd, d);
}

void launch_gmres_step(int j, const double *ww_partial, int nblk, const GmresState &s, const double *beta, double *hist, int slot,
                       hipStream_t st)
{
    hipLaunchKernelGGL(gmres_step_kernel, dim3(1), dim3(kBlock), 0, st, j, ww_partial, nblk, s, beta, hist, slot);
}

void launch_gmres_solve(int k, const GmresState &s, hipStream_t st)
{
    hipLaunchKernelGGL(gmres_solve_kernel, dim3(1), dim3(64), 0, st, k, s);
}

}  // namespace sparsh
