// eig_small.cpp -- the host Rayleigh-Ritz step of the LOBPCG eigensolver: scaling, Cholesky, reduction to a
// standard problem and cyclic Jacobi on a pencil of order m <= 24.  Host only, like box_plan.cpp and cheby_bounds.cpp.
#include "eig_small.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sparsh {

int eig_small(int m, int k, const double *GA, const double *GB, double *theta, double *C)
{
    constexpr int M = kEigSmallMax;
    if (m < 1 || m > M || k < 1 || k > m) return 1;
    double d[M], L[M][M], T[M][M], Y[M][M];
    auto up = [m](const double *G, int i, int j) { return i <= j ? G[i * m + j] : G[j * m + i]; };  // the upper triangle, mirrored
    for (int i = 0; i < m; ++i) {
        const double g = GB[i * m + i];
        if (!(g > 0.0) || !std::isfinite(g)) return 1;
        d[i] = 1.0 / std::sqrt(g);
    }
    // Cholesky factor of D GB D, row by row
    for (int i = 0; i < m; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = d[i] * up(GB, i, j) * d[j];
            for (int p = 0; p < j; ++p) s -= L[i][p] * L[j][p];
            if (i == j) {
                const double piv = s > 0.0 ? std::sqrt(s) : 0.0;
                if (!(piv >= kEigBreakdownPivot)) return 1;  // (a NaN lands here too)
                L[i][i] = piv;
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    // T = L^-1 (D GA D) L^-T: a forward substitution on the columns, then one on the rows
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) T[i][j] = d[i] * up(GA, i, j) * d[j];
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            double s = T[i][j];
            for (int p = 0; p < i; ++p) s -= L[i][p] * T[p][j];
            T[i][j] = s / L[i][i];
        }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            double s = T[i][j];
            for (int p = 0; p < j; ++p) s -= L[j][p] * T[i][p];
            T[i][j] = s / L[j][j];
        }
    for (int i = 0; i < m; ++i)
        for (int j = i + 1; j < m; ++j) T[i][j] = T[j][i] = 0.5 * (T[i][j] + T[j][i]);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) Y[i][j] = i == j ? 1.0 : 0.0;
    // cyclic Jacobi, rows and columns in order, until the off-diagonal norm is at most eps ||T||_F
    const double eps = std::numeric_limits<double>::epsilon();
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < m; ++i) {
            diag += T[i][i] * T[i][i];
            for (int j = i + 1; j < m; ++j) off += 2.0 * T[i][j] * T[i][j];
        }
        if (!std::isfinite(off + diag)) return 1;
        if (std::sqrt(off) <= eps * std::sqrt(off + diag)) break;
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = T[p][q];
                if (apq == 0.0) continue;
                const double tau = (T[q][q] - T[p][p]) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int r = 0; r < m; ++r) {
                    const double a = T[r][p], b = T[r][q];
                    T[r][p] = c * a - s * b;
                    T[r][q] = s * a + c * b;
                }
                for (int r = 0; r < m; ++r) {
                    const double a = T[p][r], b = T[q][r];
                    T[p][r] = c * a - s * b;
                    T[q][r] = s * a + c * b;
                }
                T[p][q] = T[q][p] = 0.0;
                for (int r = 0; r < m; ++r) {
                    const double a = Y[r][p], b = Y[r][q];
                    Y[r][p] = c * a - s * b;
                    Y[r][q] = s * a + c * b;
                }
            }
    }
    int order[M];
    for (int i = 0; i < m; ++i) order[i] = i;
    std::stable_sort(order, order + m, [&](int a, int b) { return T[a][a] < T[b][b]; });
    // C = D L^-T Y[:, :k]: a backward substitution per column
    for (int j = 0; j < k; ++j) {
        const int col = order[j];
        double z[M];
        for (int i = m - 1; i >= 0; --i) {
            double s = Y[i][col];
            for (int p = i + 1; p < m; ++p) s -= L[p][i] * z[p];
            z[i] = s / L[i][i];
        }
        for (int i = 0; i < m; ++i) C[i * k + j] = d[i] * z[i];
        theta[j] = T[col][col];
    }
    return 0;
}

int eig_spd_inverse(int m, const double *G, double *Ginv)
{
    constexpr int M = kEigSmallMax;
    if (m < 1 || m > M) return 1;
    double d[M], L[M][M], Z[M][M];
    auto up = [m](const double *A, int i, int j) { return i <= j ? A[i * m + j] : A[j * m + i]; };
    for (int i = 0; i < m; ++i) {
        const double g = G[i * m + i];
        if (!(g > 0.0) || !std::isfinite(g)) return 1;
        d[i] = 1.0 / std::sqrt(g);
    }
    for (int i = 0; i < m; ++i)  // the Cholesky factor and breakdown rule of eig_small
        for (int j = 0; j <= i; ++j) {
            double s = d[i] * up(G, i, j) * d[j];
            for (int p = 0; p < j; ++p) s -= L[i][p] * L[j][p];
            if (i == j) {
                const double piv = s > 0.0 ? std::sqrt(s) : 0.0;
                if (!(piv >= kEigBreakdownPivot)) return 1;
                L[i][i] = piv;
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    // L Z' = I forward, then L^T Z = Z' backward, column by column
    for (int j = 0; j < m; ++j) {
        double z[M];
        for (int i = 0; i < m; ++i) {
            double s = i == j ? 1.0 : 0.0;
            for (int p = 0; p < i; ++p) s -= L[i][p] * z[p];
            z[i] = s / L[i][i];
        }
        for (int i = m - 1; i >= 0; --i) {
            double s = z[i];
            for (int p = i + 1; p < m; ++p) s -= L[p][i] * Z[p][j];
            Z[i][j] = s / L[i][i];
        }
    }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) Ginv[i * m + j] = d[i] * (0.5 * (Z[i][j] + Z[j][i])) * d[j];
    return 0;
}

}  // namespace sparsh
