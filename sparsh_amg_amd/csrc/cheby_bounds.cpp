// Spectral bounds and coefficients of the Chebyshev smoother (cheby_bounds.hpp).  Host only.
#include "cheby_bounds.hpp"

#include <cmath>
#include <cstdint>
#include <vector>

namespace sparsh {

namespace {

// largest eigenvalue of the symmetric tridiagonal matrix (alpha, beta) of order k: bisection on the Sturm count
double tridiag_largest(const std::vector<double> &alpha, const std::vector<double> &beta, int k)
{
    if (k == 1) return alpha[0];
    double lo = alpha[0], hi = alpha[0];
    for (int i = 0; i < k; ++i) {
        const double r = (i > 0 ? std::fabs(beta[i - 1]) : 0.0) + (i + 1 < k ? std::fabs(beta[i]) : 0.0);
        lo = std::fmin(lo, alpha[i] - r);
        hi = std::fmax(hi, alpha[i] + r);
    }
    // eigenvalues below x = negative pivots of T - x I
    auto below = [&](double x) {
        int c = 0;
        double q = alpha[0] - x;
        if (q < 0.0) ++c;
        for (int i = 1; i < k; ++i) {
            if (q == 0.0) q = 1e-300;
            q = alpha[i] - x - beta[i - 1] * beta[i - 1] / q;
            if (q < 0.0) ++c;
        }
        return c;
    };
    for (int it = 0; it < 200; ++it) {
        const double mid = lo + (hi - lo) * 0.5;
        if (!(mid > lo && mid < hi)) break;
        if (below(mid) >= k) hi = mid;  // all k eigenvalues below mid
        else lo = mid;
    }
    return lo;
}

double dot_ascending(int n, const double *x, const double *y)
{
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += x[i] * y[i];
    return s;
}

}  // namespace

ChebyBounds cheby_bounds(int n, const int *rowptr, const int *col, const double *val, const double *diag, int steps)
{
    ChebyBounds out;
    if (n <= 0) return out;
    double g = 0.0;
    int bad = 0;
#pragma omp parallel for schedule(static) reduction(max : g) reduction(+ : bad)
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        for (int j = rowptr[i]; j < rowptr[i + 1]; ++j) s += std::fabs(val[j]);
        const double q = s / std::fabs(diag[i]);
        if (q > g) g = q;
        if (!(diag[i] > 0.0) || !std::isfinite(diag[i])) ++bad;
    }
    out.gershgorin = g;
    out.lmax = g;
    if (bad) return out;  // S = D^-1/2 A D^-1/2 does not exist: the Gershgorin bound alone

    const int m = steps < n ? steps : n;
    std::vector<double> is((size_t)n), q((size_t)n), qp((size_t)n, 0.0), t((size_t)n), w((size_t)n);
    for (int i = 0; i < n; ++i) {
        is[i] = 1.0 / std::sqrt(diag[i]);
        q[i] = (double)(uint32_t)((uint32_t)i * 2654435761u) / 4294967296.0 - 0.5;
    }
    const double nrm = std::sqrt(dot_ascending(n, q.data(), q.data()));
    for (int i = 0; i < n; ++i) q[i] = q[i] / nrm;
    std::vector<double> alpha, beta;
    double b_prev = 0.0;
    for (int k = 0; k < m; ++k) {
        // w = S q
#pragma omp parallel for schedule(static)
        for (int i = 0; i < n; ++i) t[i] = is[i] * q[i];
#pragma omp parallel for schedule(static)
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int j = rowptr[i]; j < rowptr[i + 1]; ++j) s += val[j] * t[col[j]];
            w[i] = is[i] * s;
        }
        const double sq = std::sqrt(dot_ascending(n, w.data(), w.data()));
        const double a = dot_ascending(n, q.data(), w.data());
        for (int i = 0; i < n; ++i) w[i] = w[i] - a * q[i] - b_prev * qp[i];
        const double b = std::sqrt(dot_ascending(n, w.data(), w.data()));
        alpha.push_back(a);
        if (k + 1 == m || !(b >= 1e-14 * sq)) break;  // invariant subspace (or a non-finite operator): the Ritz values so far
        beta.push_back(b);
        for (int i = 0; i < n; ++i) {
            qp[i] = q[i];
            q[i] = w[i] / b;
        }
        b_prev = b;
    }
    const double ritz = tridiag_largest(alpha, beta, (int)alpha.size());
    if (!(ritz > 0.0) || !std::isfinite(ritz)) return out;
    out.lanczos = ritz;
    out.lmax = std::fmin(1.1 * ritz, g);
    return out;
}

void cheby_coefficients(double lmax, double ratio, int degree, double *c1, double *c2)
{
    const double lmin = lmax / ratio;
    const double theta = (lmax + lmin) / 2.0, delta = (lmax - lmin) / 2.0, sigma = theta / delta;
    double rho = 1.0 / sigma;
    c1[0] = 0.0;
    c2[0] = 1.0 / theta;
    for (int k = 1; k < degree; ++k) {
        const double rho_k = 1.0 / (2.0 * sigma - rho);
        c1[k] = rho_k * rho;
        c2[k] = 2.0 * rho_k / delta;
        rho = rho_k;
    }
}

}  // namespace sparsh
