// eig_chol.hpp -- the small step of one orthonormalisation of the LOBPCG eigensolver under SPARSH_EIG_BASIS_ORTHO (DESIGN.md section
// 5i), beside eig_small.cpp: from G = V^T (B V) of a block V the upper-triangular T for which V T is B-orthonormal on the kept columns.
// One body for the host (sparsh_debug_eig_chol) and the device (eig_chol_kernel): + - * / and sqrt on doubles, all correctly rounded on
// both, every product and sum rounded on its own, every sum over p ascending as in eig_small's Cholesky, so both give the same bits.
#pragma once

#include <hip/hip_runtime.h>

namespace sparsh {

constexpr int kEigCholMax = 8;              // SPARSH_MAX_RHS
constexpr double kEigCholPivot = 1e-7;      // kEigBreakdownPivot of step 5

// G: order m <= 8, row-major with leading dimension ldg; only the upper triangle is read, and only the rows and columns i with
// mask_in[i] != 0.  D = diag(G)^-1/2, D G D = L L^T row by row over the kept columns, T = D L^-T (m x m row-major with leading
// dimension ldt, upper triangular; rows and columns of columns that are not kept are zero).  A column of the mask is dropped, not
// kept, when its diagonal is not finite and positive or its pivot is below kEigCholPivot (a NaN fails the comparison); mask_out[i] = 1
// for the kept columns, 0 for all others.  mask_out may be mask_in.  L: kEigCholMax * kEigCholMax doubles of scratch, d and z:
// kEigCholMax each.  Returns the number of dropped columns.
__host__ __device__ inline int eig_chol(int m, const double *G, int ldg, const double *mask_in, double *T, int ldt, double *mask_out, double *L,
                                        double *d, double *z)
{
    constexpr int M = kEigCholMax;
    bool kept[M];
    int dropped = 0;
    for (int i = 0; i < m; ++i) {
        kept[i] = false;
        if (mask_in[i] == 0.0) continue;
        const double g = G[i * ldg + i];
        if (!(g > 0.0) || !(g <= 1.7976931348623157e308)) {  // not positive, infinite or NaN
            ++dropped;
            continue;
        }
        d[i] = 1.0 / sqrt(g);
        for (int j = 0; j < i; ++j) {
            if (!kept[j]) continue;
            double s = d[i] * G[j * ldg + i] * d[j];
            for (int p = 0; p < j; ++p)
                if (kept[p]) s -= L[i * M + p] * L[j * M + p];
            L[i * M + j] = s / L[j * M + j];
        }
        double s = d[i] * g * d[i];
        for (int p = 0; p < i; ++p)
            if (kept[p]) s -= L[i * M + p] * L[i * M + p];
        const double piv = s > 0.0 ? sqrt(s) : 0.0;
        if (!(piv >= kEigCholPivot)) {
            ++dropped;
            continue;
        }
        L[i * M + i] = piv;
        kept[i] = true;
    }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) T[i * ldt + j] = 0.0;
    for (int j = 0; j < m; ++j) {  // column j of L^-T: L^T z = e_j backward over the kept rows
        if (!kept[j]) continue;
        for (int i = j; i >= 0; --i) {
            if (!kept[i]) continue;
            double s = i == j ? 1.0 : 0.0;
            for (int p = i + 1; p <= j; ++p)
                if (kept[p]) s -= L[p * M + i] * z[p];
            z[i] = s / L[i * M + i];
            T[i * ldt + j] = d[i] * z[i];
        }
    }
    for (int i = 0; i < m; ++i) mask_out[i] = kept[i] ? 1.0 : 0.0;
    return dropped;
}

}  // namespace sparsh
