// bcg_small.hpp -- the small dense solve of block CG: coef = sign * pinv(G) C for a Gram matrix G = P^T A P whose
// columns may be dependent, equal, zero or already converged.  One body for the host (sparsh_debug_bcg_small) and the device
// (bcg_small_kernel): only + - * / on doubles, every product and sum rounded on its own, every sum ascending, so both give the same
// bits.
#pragma once

#include <hip/hip_runtime.h>

namespace sparsh {

constexpr int kBcgMax = 8;              // SPARSH_MAX_RHS
constexpr double kBcgPivot = 1e-14;     // a pivot d_j <= kBcgPivot * g_jj drops direction j: the square of kEigBreakdownPivot

// LDL^T of the symmetric G of order k <= 8 (row-major with leading dimension ldg; only the upper triangle is read), no square roots,
// with dropped directions:
//   d_j  = g_jj - sum_{m < j, kept} (l_jm l_jm) d_m
//   keep_j = g_jj > 0 and d_j > 1e-14 g_jj   (a NaN fails both)
//   l_ij = (g_ij - sum_{m < j, kept} (l_im l_jm) d_m) / d_j   for i > j, j kept
// L is kBcgMax x kBcgMax row-major (strictly lower part written for kept j), d and keep hold k entries.  Returns the rank.
__host__ __device__ inline int bcg_factor(int k, const double *G, int ldg, double *L, double *d, int *keep)
{
    int rank = 0;
    for (int j = 0; j < k; ++j) {
        const double gjj = G[j * ldg + j];
        double acc = 0.0;
        for (int m = 0; m < j; ++m)
            if (keep[m]) {
                const double ll = L[j * kBcgMax + m] * L[j * kBcgMax + m];
                acc += ll * d[m];
            }
        const double dj = gjj - acc;
        d[j] = dj;
        keep[j] = (gjj > 0.0 && dj > kBcgPivot * gjj) ? 1 : 0;
        if (!keep[j]) continue;
        ++rank;
        for (int i = j + 1; i < k; ++i) {
            double s = 0.0;
            for (int m = 0; m < j; ++m)
                if (keep[m]) {
                    const double ll = L[i * kBcgMax + m] * L[j * kBcgMax + m];
                    s += ll * d[m];
                }
            const double t = G[j * ldg + i] - s;  // g_ij read from the upper triangle
            L[i * kBcgMax + j] = t / dj;
        }
    }
    return rank;
}

// Column c of coef = sign * pinv(G) C on the kept index set: forward, diagonal and backward substitution, sums ascending.  C and coef
// are row-major with leading dimensions ldc and ldo; rows of dropped directions are written as zeros.  y: kBcgMax doubles of scratch.
__host__ __device__ inline void bcg_solve_column(int k, const double *L, const double *d, const int *keep, const double *C, int ldc, int c,
                                                 double sign, double *coef, int ldo, double *y)
{
    for (int i = 0; i < k; ++i) {
        if (!keep[i]) continue;
        double s = 0.0;
        for (int m = 0; m < i; ++m)
            if (keep[m]) s += L[i * kBcgMax + m] * y[m];
        y[i] = C[i * ldc + c] - s;
    }
    for (int i = 0; i < k; ++i)
        if (keep[i]) y[i] = y[i] / d[i];
    for (int i = k - 1; i >= 0; --i) {
        if (!keep[i]) continue;
        double s = 0.0;
        for (int m = i + 1; m < k; ++m)
            if (keep[m]) s += L[m * kBcgMax + i] * y[m];
        y[i] = y[i] - s;
    }
    for (int i = 0; i < k; ++i) coef[i * ldo + c] = keep[i] ? sign * y[i] : 0.0;
}

}  // namespace sparsh
