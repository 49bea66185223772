// eig_small.hpp -- the host Rayleigh-Ritz step of the LOBPCG eigensolver.  Host only: no HIP, no engine.
#pragma once

namespace sparsh {

constexpr int kEigSmallMax = 24;              // order of the compacted pencil: 3 blocks of at most 8 columns
constexpr double kEigBreakdownPivot = 1e-7;   // a Cholesky pivot of the scaled Gram matrix below this is a breakdown

// The k lowest eigenpairs of the pencil (GA, GB) of order m (row-major, symmetric, GB positive definite; only the upper triangles
// are read):
//   D = diag(GB)^-1/2 ; D GB D = L L^T ; T = L^-1 (D GA D) L^-T, symmetrised ; T = Y diag(theta) Y^T by cyclic Jacobi to an
//   off-diagonal norm of at most eps ||T||_F, theta ascending ; C = D L^-T Y[:, :k]  (m x k, row-major), so that C^T GB C = I.
// Returns 0, or 1 for a breakdown: a diagonal entry of GB that is not finite and positive, or a pivot L_ii that is not >= 1e-7
// (a condition number near 1e14 of the scaled Gram matrix: past it the Ritz values carry no digits).  Nothing is written then.
int eig_small(int m, int k, const double *GA, const double *GB, double *theta, double *C);

// The inverse of the symmetric positive definite G of order m <= 24 (row-major; only the upper triangle is read) by the scaling and
// Cholesky factorisation above and two triangular solves per column: Ginv = D L^-T L^-1 D, symmetrised.  Returns 0, or 1 under the
// breakdown rule above (G is then numerically rank deficient); nothing is written then.
int eig_spd_inverse(int m, const double *G, double *Ginv);

}  // namespace sparsh
