"""Block CG without a device: the small solve with dropped directions against numpy.linalg.lstsq on the kept
index set, sparsh_debug_bcg_small against its numpy restatement bit for bit, the restated loop against numpy.linalg.solve and against
textbook PCG, and the argument and state errors of SPARSH_BCG through the block entry points.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from bcg_restatement import bcg, degenerate_block, pcg, small, small_cases
from test_multi_rhs_host import raw_solve_multi

QUIET = dict(print_setup=0, print_solve=0)
EPS = np.finfo(np.float64).eps
CASES = small_cases()


@pytest.mark.parametrize("name,G,Cm,keep", CASES, ids=[c[0] for c in CASES])
def test_small_is_the_least_squares_solution_on_the_kept_set(name, G, Cm, keep):
    """LDL^T with substitution is backward stable: the computed coefficients solve a system perturbed by c k eps, so they are within
    c k eps cond(G_kept) of the exact ones; c = 100 covers the growth of the substitutions on orders up to 8."""
    k = len(keep)
    for sign in (1.0, -1.0):
        coef, mask, rank = small(G, Cm, sign)
        assert list(mask) == keep and rank == sum(keep), (name, mask)
        kept = np.flatnonzero(mask)
        assert np.all(coef[mask == 0] == 0.0), name
        if len(kept) == 0:
            continue
        Gk = np.triu(G) + np.triu(G, 1).T  # the upper triangle is what is read
        Gk = Gk[np.ix_(kept, kept)]
        want = sign * np.linalg.lstsq(Gk, Cm[kept], rcond=None)[0]
        err = np.abs(coef[kept] - want).max() / np.abs(want).max()
        bound = 100 * k * EPS * np.linalg.cond(Gk)
        print(name, sign, "rank", rank, "relative error", err, "bound", bound)
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("name,G,Cm,keep", CASES, ids=[c[0] for c in CASES])
def test_debug_entry_is_the_restatement_bit_for_bit(name, G, Cm, keep):
    for sign in (1.0, -1.0):
        coef, mask, rank = small(G, Cm, sign)
        got, gmask, grank = sa.bcg_small(G, Cm, sign)
        assert grank == rank and np.array_equal(gmask, mask), name
        assert np.array_equal(got, coef), (name, np.abs(got - coef).max())
    # only the upper triangle is read
    junk = np.array(G)
    junk[np.tril_indices(len(keep), -1)] = 123.0
    assert np.array_equal(sa.bcg_small(junk, Cm)[0], small(G, Cm)[0]), name


def test_debug_entry_refuses_bad_arguments():
    G = np.eye(2)
    out, keep = np.zeros((2, 2)), np.zeros(2, dtype=np.int32)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    dp = lambda a: a.ctypes.data_as(DP)  # noqa: E731
    f = sa.lib.sparsh_debug_bcg_small
    for k in (0, -1, 9):
        assert f(k, dp(G), dp(G), 1.0, dp(out), keep.ctypes.data_as(IP)) == sa.SPARSH_EINVAL
    assert f(2, None, dp(G), 1.0, dp(out), keep.ctypes.data_as(IP)) == sa.SPARSH_EINVAL
    assert f(2, dp(G), dp(G), 1.0, dp(out), None) == sa.SPARSH_EINVAL
    assert f(2, dp(G), dp(G), 1.0, dp(out), keep.ctypes.data_as(IP)) == 2


# ---------------------------------------------------------------------------- the restated loop

@pytest.fixture(scope="module")
def dense():
    """a dense SPD system of 80 rows with eigenvalues >= 1 (so ||A^-1|| <= 1) and a dense SPD preconditioner"""
    rng = np.random.default_rng(5)
    n = 80
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.geomspace(1.0, 100.0, n)) @ Q.T
    A = 0.5 * (A + A.T)
    D = np.diag(np.diag(A))
    M = np.linalg.inv(D + 0.5 * (A - D))  # SPD here: checked below
    M = 0.5 * (M + M.T)
    assert np.linalg.eigvalsh(M).min() > 0
    return A, M, rng.standard_normal((n, 8))


TOL = 1e-9


def run(A, M, B, chunk=0):
    return bcg(lambda V: A @ V, lambda V: M @ V, B, np.zeros_like(B), TOL, 400, chunk)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_restatement_agrees_with_a_direct_solve(dense, k):
    """||A^-1|| <= 1, so a residual of tol is an error of at most tol; the recurrence residual drifts from the true one by rounding
    noise far below tol on this system, for which a factor of 2 is left."""
    A, M, B = dense
    X, hist, info = run(A, M, B[:, :k])
    assert info["status"] == "ok" and info["min_rank"] == k and info["dropped"] == 0
    assert hist.shape == (info["iterations"], k) and np.all(hist[-1] <= TOL) and not np.all(hist[-2] <= TOL)
    err = np.linalg.norm(X - np.linalg.solve(A, B[:, :k]), axis=0)
    print(k, "iterations", info["iterations"], "largest error", err.max())
    assert np.all(err <= 2 * TOL)


def test_more_columns_take_fewer_iterations(dense):
    A, M, B = dense
    its = [run(A, M, B[:, :k])[2]["iterations"] for k in (1, 2, 4, 8)]
    print("iterations for k = 1, 2, 4, 8:", its)
    assert its[0] > its[1] > its[2] > its[3]


def test_one_column_follows_textbook_pcg(dense):
    """With one column alpha = p.r / p.Ap and beta = -q.z / p.q are PCG's z.r / p.Ap and z'.r' / z.r in exact arithmetic.  In
    floating point the two forms differ by rounding noise amplified by the condition of the preconditioned operator (at
    most 100 here, some 30 iterations): 1e-6 is far above that and far below the O(1) change any error in a coefficient makes."""
    A, M, B = dense
    b = B[:, 0]
    X, hist, info = run(A, M, B[:, :1])
    x, h = pcg(lambda v: A @ v, lambda v: M @ v, b, np.zeros_like(b), TOL, 400)
    assert abs(len(h) - info["iterations"]) <= 1
    m = min(len(h), len(hist))
    big = h[:m] > 100 * TOL
    rel = np.abs(hist[:m, 0] - h[:m])[big] / h[:m][big]
    print("iterations", info["iterations"], len(h), "largest relative history difference", rel.max())
    assert big.sum() > 10 and rel.max() <= 1e-6


def test_degenerate_blocks_lose_rank_not_the_solve(dense):
    A, M, B = dense
    Bd = degenerate_block(B)
    X, hist, info = run(A, M, Bd)
    print("degenerate: iterations", info["iterations"], "ranks", info["ranks"])
    assert info["status"] == "ok" and info["min_rank"] == 5 and max(info["ranks"]) == 5
    assert not np.isnan(X).any()
    assert np.all(np.linalg.norm(X - np.linalg.solve(A, Bd), axis=0) <= 2 * TOL)
    assert np.array_equal(X[:, 3], np.zeros(len(X)))
    # a column scaled by 1e-6 and a smooth column converge with the rest at full rank
    Bs = np.array(B)
    Bs[:, 2] *= 1e-6
    Bs[:, 4] = A @ np.ones(len(A))
    X, hist, info = run(A, M, Bs)
    assert info["status"] == "ok" and info["min_rank"] == 8
    assert np.all(np.linalg.norm(X - np.linalg.solve(A, Bs), axis=0) <= 2 * TOL)
    # every column zero: nothing to do; every column already solved: nothing to do
    X, hist, info = run(A, M, np.zeros((len(A), 3)))
    assert info["status"] == "ok" and info["iterations"] == 0 and np.array_equal(X, np.zeros((len(A), 3)))
    Xs = np.linalg.solve(A, B[:, :2])
    X, hist, info = bcg(lambda V: A @ V, lambda V: M @ V, A @ Xs, Xs, TOL, 10)
    assert info["iterations"] == 0 and np.array_equal(X, Xs)


def test_the_cap_and_a_nan_are_reported(dense):
    A, M, B = dense
    X, hist, info = bcg(lambda V: A @ V, lambda V: M @ V, B[:, :3], np.zeros((len(A), 3)), TOL, 4)
    assert info["status"] == "noconv" and info["iterations"] == 4 and hist.shape == (4, 3)
    Bn = np.array(B[:, :3])
    Bn[7, 1] = np.nan
    assert bcg(lambda V: A @ V, lambda V: M @ V, Bn, np.zeros((len(A), 3)), TOL, 4)[2]["status"] == "numeric"


def test_chunked_gram_sums_change_only_the_last_bits(dense):
    A, M, B = dense
    (_, h0, i0), (_, h1, i1) = run(A, M, B, 0), run(A, M, B, 16)
    assert abs(i0["iterations"] - i1["iterations"]) <= 1
    m = min(len(h0), len(h1))
    big = h0[:m] > 100 * TOL
    assert (np.abs(h0[:m] - h1[:m])[big] / h0[:m][big]).max() <= 1e-6


# ---------------------------------------------------------------------------- C ABI without a device

@pytest.fixture(scope="module")
def problem():
    rp, ci, v = problems.poisson2d(40)
    n = len(rp) - 1
    return rp, ci, v, n, np.ones((n, 8), order="F"), np.zeros((n, 8), order="F")


def test_the_method_constant():
    assert sa.SPARSH_BCG == 8 and sa.BLOCK_METHODS == {"bcg": 8}
    assert "bcg" not in sa.METHODS  # a method of solve_multi only


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_bcg_arguments_and_state_without_a_device(problem, dev, prepared):
    rp, ci, v, n, B, X = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    m = sa.SPARSH_BCG
    for nrhs in (0, -1, 9, 100):
        assert raw_solve_multi(A, m, nrhs, B, n, X, n, dev=dev) == sa.SPARSH_EINVAL, nrhs
        assert b"nrhs" in sa.lib.sparsh_last_error()
    assert raw_solve_multi(A, m, 4, None, n, X, n, dev=dev) == sa.SPARSH_EINVAL
    assert raw_solve_multi(A, m, 4, B, n, None, n, dev=dev) == sa.SPARSH_EINVAL
    assert raw_solve_multi(A, m, 4, B, n, X, n, iters=False, dev=dev) == sa.SPARSH_EINVAL
    assert raw_solve_multi(A, m, 4, B, n, X, n, status=False, dev=dev) == sa.SPARSH_EINVAL
    assert b"NULL" in sa.lib.sparsh_last_error()
    assert raw_solve_multi(A, m, 4, B, n - 1, X, n, dev=dev) == sa.SPARSH_EINVAL
    assert raw_solve_multi(A, m, 4, B, n, X, n - 1, dev=dev) == sa.SPARSH_EINVAL
    assert b"ldb" in sa.lib.sparsh_last_error()
    # every other method that is not SPARSH_PCG is still refused
    for method in (sa.SPARSH_AMG, sa.SPARSH_CG, sa.SPARSH_BICG, sa.SPARSH_PBICG, sa.SPARSH_GMRES, sa.SPARSH_PGMRES, sa.SPARSH_FCG, 9, 17, -1):
        assert raw_solve_multi(A, method, 4, B, n, X, n, dev=dev) == sa.SPARSH_EINVAL, method
        assert b"SPARSH_BCG" in sa.lib.sparsh_last_error()
    # valid arguments: the call order is what is wrong
    for nrhs in (1, 4, 8):
        assert raw_solve_multi(A, m, nrhs, B, n, X, n, dev=dev) == sa.SPARSH_ESTATE, nrhs


def test_bcg_is_refused_where_block_pcg_is(problem):
    rp, ci, v, n, B, X = problem
    m = sa.SPARSH_BCG
    A = sa.sp_matrix_mg(rp, ci, v)
    A.set_smoother("sor", 0, "symmetric")
    assert raw_solve_multi(A, m, 4, B, n, X, n) == sa.SPARSH_EINVAL
    assert b"Jacobi" in sa.lib.sparsh_last_error()
    A.set_smoother("jacobi")
    assert raw_solve_multi(A, m, 4, B, n, X, n) == sa.SPARSH_ESTATE
    F = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, precond_fp32=1), host_only=True)
    assert raw_solve_multi(F, m, 4, B, n, X, n) == sa.SPARSH_EINVAL
    assert b"precond_fp32" in sa.lib.sparsh_last_error()
    N = sa.sp_matrix_mg(*problems.poisson3d_neumann(6, 5, 4)).set_nullspace("constant")
    N.setup(sa.default_params(**QUIET), host_only=True)
    nn = N.nrow
    assert raw_solve_multi(N, m, 2, np.ones((nn, 2), order="F"), nn, np.zeros((nn, 2), order="F"), nn) == sa.SPARSH_EINVAL
    assert b"null space" in sa.lib.sparsh_last_error()
    with pytest.raises(sa.SparshError) as e:
        sa.sp_matrix_mg(rp, ci, v).solve_multi("bcg", B[:, :4], X[:, :4].copy())
    assert e.value.code == sa.SPARSH_ESTATE
    # the single-vector entry point does not know the method
    with pytest.raises((sa.SparshError, KeyError)):
        sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET), host_only=True).solve("bcg", B[:, 0].copy(), X[:, 0].copy())


def test_bcg_info_is_zero_on_a_fresh_handle(problem):
    rp, ci, v, n, _, _ = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    zeros = dict(iterations=0, min_rank=0, dropped=0, bytes=0)
    assert A.bcg_info() == zeros
    A.setup(sa.default_params(**QUIET), host_only=True)
    assert A.bcg_info() == zeros
    assert sa.lib.sparsh_bcg_info(None, None, None, None, None) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_bcg_info(A._h, None, None, None, None) == sa.SPARSH_OK
