// eig_ortho_kernels.hip -- the kernels of the LOBPCG eigensolver under SPARSH_EIG_BASIS_ORTHO: the active mask
// on the device, the small Cholesky step of an orthonormalisation, the transform V <- V T of interleaved blocks in place, and the
// masked subtraction W <- W0 - X C.
//
// Storage is that of eig_kernels.hip: a block of W vectors (W = 2, 4 or 8) is row-interleaved, element (row i, column c) at
// v[i * W + c], 16-byte aligned; a lane owns two neighbouring columns of one row and the W / 2 lanes of a row sit side by side in one
// wave.  Masks are W doubles, 1.0 for a column that is in and 0.0 for one that is out, so that they travel with the Gram matrices.
//
// Arithmetic contract: every product and every sum is rounded on its own (the library is built with -ffp-contract=off).  Nothing here
// reduces over rows and nothing uses atomics: the same input gives the same bits whatever the grid.
#include <hip/hip_runtime.h>

#include "eig_chol.hpp"
#include "kernels.hpp"

namespace sparsh {

namespace {

using d2o = double __attribute__((ext_vector_type(2)));

constexpr int kEigOrthoMaxGrid = 2048;  // streaming kernels without partial sums: ~8 workgroups per CU, as the update of eig_kernels.hip

// masks[c] = 1.0 when column c < k is active by the rule of step 2 on the norms the residual's finalise wrote, 0.0 otherwise (padding
// columns too): rn_c > tol |theta_c| for the standard problem, rn_c > (tol |theta_c|) bn_c for the pencil (A, B).  A NaN norm makes the
// column inactive here; the host has refused it by then.  The masks of W and P (masks + W, masks + 2 W) are cleared for the iteration.
__global__ __launch_bounds__(64) void eig_active_mask_kernel(int W, int k, int gen, double tol, const double *__restrict__ theta,
                                                             const double *__restrict__ rn, const double *__restrict__ bn,
                                                             double *__restrict__ masks)
{
    const int c = threadIdx.x;
    if (c >= W) return;
    bool on = false;
    if (c < k) {
        const double bound = tol * fabs(theta[c]);
        on = gen ? rn[c] > bound * bn[c] : rn[c] > bound;
    }
    masks[c] = on ? 1.0 : 0.0;
    masks[W + c] = 0.0;
    masks[2 * W + c] = 0.0;
}

// one wavefront: G (W x W row-major, upper triangle) and the mask come into LDS, lane 0 runs eig_chol (the host's body, the same bits),
// then the wave writes T (W x W row-major) and the mask of the kept columns.  mask_out may be mask_in.
__global__ __launch_bounds__(64) void eig_chol_kernel(int W, const double *__restrict__ G, const double *mask_in, double *__restrict__ T,
                                                      double *mask_out)
{
    constexpr int M = kEigCholMax;
    __shared__ double sG[M * M], sT[M * M], sL[M * M], sd[M], sz[M], smi[M], smo[M];
    const int t = threadIdx.x;
    if (t < W * W) sG[t] = G[t];
    if (t < W) smi[t] = mask_in[t];
    __syncthreads();
    if (t == 0) (void)eig_chol(W, sG, W, smi, sT, W, smo, sL, sd, sz);
    __syncthreads();
    if (t < W * W) T[t] = sT[t];
    if (t < W) mask_out[t] = smo[t];
}

// the two entries j, j + 1 of sum_{c < k} V_ic T_cj, c ascending from the product of c = 0 (eig_row_times of eig_kernels.hip); the row
// is read 16 bytes at a time and st holds the W x W matrix in LDS
template <int W>
__device__ __forceinline__ d2o ortho_row_times(const double *V, size_t base, const double *st, int j, int k)
{
    d2o acc = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < W; c += 2) {
        if (c < k) {
            const d2o b = *reinterpret_cast<const d2o *>(V + base + c);
            const d2o c0 = *reinterpret_cast<const d2o *>(st + c * W + j);
            const d2o t0 = {b.x * c0.x, b.x * c0.y};
            acc = c == 0 ? t0 : acc + t0;
            if (c + 1 < k) {
                const d2o c1 = *reinterpret_cast<const d2o *>(st + (c + 1) * W + j);
                const d2o t1 = {b.y * c1.x, b.y * c1.y};
                acc = acc + t1;
            }
        }
    }
    return acc;
}

// V <- V T in place on nb <= 3 blocks with the same T (k x k inside W x W, row-major), columns j >= k written as zeros.  All loads of
// a row come before its stores and the lanes of a row share a wave, as in eig_update_kernel.  Rows are independent.
template <int W>
__global__ __launch_bounds__(kBlock) void eig_transform_kernel(int n, int k, int nb, double *V0, double *V1, double *V2,
                                                                const double *__restrict__ T)
{
    constexpr int LPR = W / 2;
    constexpr int RP = kBlock / LPR;
    __shared__ __attribute__((aligned(16))) double st[W * W];
    for (int i = threadIdx.x; i < W * W; i += kBlock) st[i] = T[i];
    __syncthreads();
    const int j = 2 * (threadIdx.x % LPR);
    for (size_t row = (size_t)blockIdx.x * RP + threadIdx.x / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const size_t base = row * W;
        d2o o0 = ortho_row_times<W>(V0, base, st, j, k), o1 = {0.0, 0.0}, o2 = {0.0, 0.0};
        if (nb > 1) o1 = ortho_row_times<W>(V1, base, st, j, k);
        if (nb > 2) o2 = ortho_row_times<W>(V2, base, st, j, k);
        if (j >= k) o0 = o1 = o2 = d2o{0.0, 0.0};
        else if (j + 1 >= k) o0.y = o1.y = o2.y = 0.0;
        *reinterpret_cast<d2o *>(V0 + base + j) = o0;
        if (nb > 1) *reinterpret_cast<d2o *>(V1 + base + j) = o1;
        if (nb > 2) *reinterpret_cast<d2o *>(V2 + base + j) = o2;
    }
}

// dst_ic = src_ic - sum_{j < k} X_ij C_jc on the columns of the mask, exact zeros on the others (whatever src holds there).  Every
// workgroup holds the same C (W x W row-major) and mask in LDS; the order is that of eig_con_apply_kernel: the running sum over j
// ascending starts with the product of j = 0, one subtraction at the end.  A lane loads its own 16 bytes of src before it stores
// them to dst, so dst may be src (neither is __restrict__); X must be neither.
template <int W>
__global__ __launch_bounds__(kBlock) void eig_ortho_apply_kernel(int n, int k, const double *__restrict__ X, const double *__restrict__ C,
                                                                  const double *__restrict__ mask, const double *src, double *dst)
{
    constexpr int LPR = W / 2;
    constexpr int RP = kBlock / LPR;
    __shared__ __attribute__((aligned(16))) double sc[W * W];
    __shared__ double sm[W];
    for (int i = threadIdx.x; i < W * W; i += kBlock) sc[i] = C[i];
    if (threadIdx.x < W) sm[threadIdx.x] = mask[threadIdx.x];
    __syncthreads();
    const int c = 2 * (threadIdx.x % LPR);
    const bool on0 = c < k && sm[c] != 0.0, on1 = c + 1 < k && sm[c + 1] != 0.0;
    for (size_t row = (size_t)blockIdx.x * RP + threadIdx.x / LPR; row < (size_t)n; row += (size_t)gridDim.x * RP) {
        const size_t base = row * W;
        const d2o acc = ortho_row_times<W>(X, base, sc, c, k);
        const d2o v = *reinterpret_cast<const d2o *>(src + base + c);
        const d2o w = v - acc;
        d2o o;
        o.x = on0 ? w.x : 0.0;
        o.y = on1 ? w.y : 0.0;
        *reinterpret_cast<d2o *>(dst + base + c) = o;
    }
}

int ortho_grid(int n, int W)
{
    const long passes = ((long)n + kBlock / (W / 2) - 1) / (kBlock / (W / 2));
    return passes < 1 ? 1 : (passes > kEigOrthoMaxGrid ? kEigOrthoMaxGrid : (int)passes);
}

}  // namespace

void launch_eig_active_mask(int W, int k, bool gen, double tol, const double *theta, const double *rn, const double *bn, double *masks,
                            hipStream_t st)
{
    hipLaunchKernelGGL(eig_active_mask_kernel, dim3(1), dim3(64), 0, st, W, k, gen ? 1 : 0, tol, theta, rn, bn, masks);
}

void launch_eig_chol_small(int W, const double *G, const double *mask_in, double *T, double *mask_out, hipStream_t st)
{
    hipLaunchKernelGGL(eig_chol_kernel, dim3(1), dim3(64), 0, st, W, G, mask_in, T, mask_out);
}

void launch_eig_transform(int n, int W, int k, int nb, double *const V[3], const double *T, hipStream_t st)
{
    const int g = ortho_grid(n, W);
    double *v0 = V[0], *v1 = nb > 1 ? V[1] : nullptr, *v2 = nb > 2 ? V[2] : nullptr;
    switch (W) {
    case 2: hipLaunchKernelGGL(eig_transform_kernel<2>, dim3(g), dim3(kBlock), 0, st, n, k, nb, v0, v1, v2, T); break;
    case 4: hipLaunchKernelGGL(eig_transform_kernel<4>, dim3(g), dim3(kBlock), 0, st, n, k, nb, v0, v1, v2, T); break;
    default: hipLaunchKernelGGL(eig_transform_kernel<8>, dim3(g), dim3(kBlock), 0, st, n, k, nb, v0, v1, v2, T); break;
    }
}

void launch_eig_ortho_apply(int n, int W, int k, const double *X, const double *C, const double *mask, const double *src, double *dst,
                            hipStream_t st)
{
    const int g = ortho_grid(n, W);
    switch (W) {
    case 2: hipLaunchKernelGGL(eig_ortho_apply_kernel<2>, dim3(g), dim3(kBlock), 0, st, n, k, X, C, mask, src, dst); break;
    case 4: hipLaunchKernelGGL(eig_ortho_apply_kernel<4>, dim3(g), dim3(kBlock), 0, st, n, k, X, C, mask, src, dst); break;
    default: hipLaunchKernelGGL(eig_ortho_apply_kernel<8>, dim3(g), dim3(kBlock), 0, st, n, k, X, C, mask, src, dst); break;
    }
}

}  // namespace sparsh
