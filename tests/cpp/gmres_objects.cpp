// Solver_PGMRES_1 and Solver_GMRES_1 of the drop-in layer, used the way main.cpp uses its neighbours: readcoo -> sp_matrix_fill ->
// sp_matrix_fill_diagonal -> solver.  Exit status 0: the preconditioned solve reached ||b - A x|| <= 1.001e-8 and the
// unpreconditioned one, stopped by the iteration cap, reduced the residual.
#include "AMG.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

static double residual(const sp_matrix_mg &A, const double *b, const double *x)
{
    double rr = 0.0;
    for (int i = 0; i < A.nrow; i++) {
        double s = 0.0;
        for (int j = A.rowptr[i]; j < A.rowptr[i + 1]; j++) s += A.val[j] * x[A.colindex[j]];
        rr += (b[i] - s) * (b[i] - s);
    }
    return std::sqrt(rr);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    sp_matrix_mg *A = new sp_matrix_mg();
    double *b;
    readcoo(argv[1], argv[2], A, b);
    A->sp_matrix_fill();
    A->sp_matrix_fill_diagonal();
    const int n = A->nrow;
    setenv("SPARSH_PRINT", "0", 1);
    int status = 0;

    double *x = new double[n]();
    const double r0 = residual(*A, b, x);
    Solver_PGMRES_1(*A, b, x);
    const double rp = residual(*A, b, x);
    std::printf("PGMRES residual %.6e (from %.6e)\n", rp, r0);
    if (!(rp <= 1.001e-8)) status |= 1;

    setenv("SPARSH_MAXIT", "90", 1);  // three restart cycles of the default length
    double *y = new double[n]();
    Solver_GMRES_1(*A, b, y);
    const double rg = residual(*A, b, y);
    std::printf("GMRES residual after the cap %.6e (from %.6e)\n", rg, r0);
    if (!(rg < r0)) status |= 2;

    A->~sp_matrix_mg();
    delete[] x;
    delete[] y;
    delete[] b;
    return status;
}
