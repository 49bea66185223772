// Spectral bounds and coefficients of the Chebyshev polynomial smoother.  Pure host code, no HIP: plain g++ compiles it.
//
// The smoother is a Chebyshev polynomial in D^-1 A on the interval [lmin, lmax], lmax an upper bound of the spectrum of
// S = D^-1/2 A D^-1/2 and lmin = lmax / ratio.  Neither bound alone is usable: Gershgorin overshoots by up to
// 3x on unstructured levels, a few Lanczos (or power) steps undershoot and the polynomial then amplifies the top of the spectrum.
// Hence lmax = min(1.1 * lanczos, gershgorin).
#pragma once

namespace sparsh {

constexpr int kChebyDefaultDegree = 4, kChebyMaxDegree = 16;
constexpr int kChebyDefaultSteps = 10, kChebyMaxSteps = 64;
constexpr double kChebyDefaultRatio = 30.0;

struct ChebyBounds {
    double gershgorin = 0.0;  // max_i sum_j |a_ij| / |a_ii|, a row's terms added one by one in stored order
    double lanczos = 0.0;     // largest Ritz value of S after min(steps, n) Lanczos steps; 0 when some a_ii is not positive and finite
    double lmax = 0.0;        // min(1.1 * lanczos, gershgorin); gershgorin alone when lanczos = 0
};

// diag = the level's diagonal as the kernels see it (first entry with col == row of every row, 0 where a row has none).  The value
// does not depend on the number of threads: rows are summed in stored order and every dot product in ascending row order.
ChebyBounds cheby_bounds(int n, const int *rowptr, const int *col, const double *val, const double *diag, int steps);

// coefficients of a degree-m leg on [lmax / ratio, lmax]: step k adds d_k = c1[k] * d_{k-1} + c2[k] * D^-1 (b - A x_k) to the iterate
// (c1[0] = 0).  Doubles, one rounding per operation (the library is built with -ffp-contract=off).
void cheby_coefficients(double lmax, double ratio, int degree, double *c1, double *c2);

}  // namespace sparsh
