"""Lowest eigenpairs by AMG-preconditioned LOBPCG on the block path: the three kernels through their
operator-level hooks (the Gram launch exactly on integer data, the residual and the update bitwise against numpy), whole solves
against analytic eigenvalues and against the numpy restatement driven by the handle's own block SpMV and block V-cycle, soft locking,
the iteration cap, reproducibility, isolation from the linear solvers, the life cycle of the solver's memory and the refusals.
GPU box only."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import hist_tolerance
from eig_restatement import lobpcg, update

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
RAGGED = (1, 2, 63, 64, 65, 255, 257, 1080, 70001)  # below, at and above a wave, a pass of a workgroup, several workgroups
TOL = 1e-8

INPUTS = {
    "p3_12_10_9": lambda: problems.poisson3d(12, 10, 9),
    "p3_8": lambda: problems.poisson3d(8),
    "p2_40": lambda: problems.poisson2d(40),
    "fem_3000": lambda: problems.fem_unstructured(3000),
}
GRIDS = {"p3_12_10_9": (12, 10, 9), "p3_8": (8, 8, 8), "p2_40": (40, 40)}
# (input, k, max_iters); the eigenvalues 2-4 of p3_8 are a triple: eigenvalues and residuals are asserted, never vectors
SOLVES = [("p3_12_10_9", 1, 0), ("p3_12_10_9", 3, 0), ("p3_12_10_9", 4, 0), ("p3_12_10_9", 8, 0), ("p3_8", 4, 0), ("p3_8", 7, 0),
          ("p2_40", 6, 0), ("fem_3000", 4, 300)]


@functools.lru_cache(maxsize=None)
def csr(name):
    return INPUTS[name]()


@functools.lru_cache(maxsize=None)
def handle(name):
    return sa.sp_matrix_mg(*csr(name)).setup(sa.default_params(**QUIET))


@functools.lru_cache(maxsize=None)
def scipy_matrix(name):
    rp, ci, v = csr(name)
    return sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, len(rp) - 1))


def analytic(name, k):
    dims = GRIDS[name]
    lam = np.zeros(dims) + 2.0 * len(dims)
    for ax, d in enumerate(dims):
        shape = [1] * len(dims)
        shape[ax] = d
        lam = lam - 2.0 * np.cos(np.arange(1, d + 1) * np.pi / (d + 1)).reshape(shape)
    return np.sort(lam.ravel())[:k]


# ---------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("n", RAGGED)
def test_gram_is_exact_on_small_integers(n):
    A = handle("p3_8")
    rng = np.random.default_rng(n)
    for nu, nv in ((1, 1), (2, 1), (3, 3), (4, 5), (7, 8), (8, 8)):
        U, V = rng.integers(-8, 9, (n, nu)).astype(np.float64), rng.integers(-8, 9, (n, nv)).astype(np.float64)
        G = A.op_gram_multi(U, V)  # every partial sum is an integer below 2^53: any order gives the same bits
        assert np.array_equal(G, U.T @ V), (n, nu, nv)


@pytest.mark.parametrize("n", (65, 1080, 70001))
def test_gram_of_normal_data_is_accurate_and_reproducible(n):
    A = handle("p3_8")
    rng = np.random.default_rng(100 + n)
    for nu, nv in ((1, 2), (4, 4), (5, 3), (8, 8)):
        U, V = rng.standard_normal((n, nu)), rng.standard_normal((n, nv))
        G = A.op_gram_multi(U, V)
        assert np.all(np.abs(G - U.T @ V) <= 1e-12 * (np.abs(U).T @ np.abs(V))), (n, nu, nv)
        assert np.array_equal(G, A.op_gram_multi(U, V))
    X = rng.standard_normal((n, 6))
    G = A.op_gram_multi(X, X)  # one block on both sides, as X^T X in the solver
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("k", range(1, 9))
def test_residual_is_bitwise_numpy(k):
    A = handle("p3_8")
    rng = np.random.default_rng(k)
    for n in RAGGED:
        AX, X, theta = rng.standard_normal((n, k)), rng.standard_normal((n, k)), rng.standard_normal(k) * 3.0
        R, norms = A.op_eig_residual(AX, X, theta)
        want = AX - X * theta
        assert np.array_equal(R, want), (n, k)
        assert np.allclose(norms, np.linalg.norm(want, axis=0), rtol=1e-12, atol=0.0), (n, k)


@pytest.mark.parametrize("k", (1, 2, 3, 5, 8))
def test_update_is_bitwise_the_stated_order(k):
    A = handle("p3_8")
    rng = np.random.default_rng(40 + k)
    for n in (1, 63, 65, 257, 1080, 70001):
        blocks = [rng.standard_normal((n, k)) for _ in range(6)]
        coefs = [rng.standard_normal((k, k)) for _ in range(3)]
        for masked in (False, True):
            if masked:  # rows of inactive columns are zero; no P at all (the first iteration)
                coefs[1][rng.integers(0, k), :] = 0.0
                coefs[2][:, :] = 0.0
            want = update(*blocks, *coefs)
            got = A.op_eig_update(*blocks, *coefs)
            for name, g, w in zip(("X", "P", "AX", "AP"), got, want):
                assert np.array_equal(g, w), (n, k, masked, name)
        got = A.op_eig_update(*blocks, *coefs, in_place=True)  # every output replaces its block on the device
        for name, g, w in zip(("X", "P", "AX", "AP"), got, want):
            assert np.array_equal(g, w), (n, k, "in place", name)


# ---------------------------------------------------------------------------- solver

@functools.lru_cache(maxsize=None)
def solved(name, k, max_iters):
    return handle(name).eigs(k, tol=TOL, max_iters=max_iters)


@functools.lru_cache(maxsize=None)
def restated(name, k, max_iters):
    """the numpy restatement with the handle's own block SpMV and block V-cycle (hooks of the block path).  Its Gram matrices come
    from the Gram launch (exact on integers, test_gram_is_exact_on_small_integers) rather than from numpy: inside a multiple
    eigenvalue (p3_8: eigenvalues 2-4) the Ritz vectors, and with them each column's residual, hang on the last bits of the Gram
    matrices, and only equal bits there let the two histories be compared column by column"""
    A = handle(name)
    X0 = np.random.default_rng(0).standard_normal((A.nrow, k))
    return lobpcg(lambda X: A.op_spmv_dot_multi(0, X)[0], lambda R: A.op_precond_multi(R), X0, tol=TOL, max_iters=max_iters or A.params.max_iter,
                  gram=A.op_gram_multi)


@pytest.mark.parametrize("name,k,max_iters", SOLVES)
def test_solver_finds_the_lowest_eigenpairs(name, k, max_iters):
    lam, X, iters, hist, status = solved(name, k, max_iters)
    M = scipy_matrix(name)
    assert np.all(status == sa.SPARSH_OK)
    assert np.all(np.diff(lam) >= 0)
    if name in GRIDS:
        ref = analytic(name, k)
        assert np.all(np.abs(lam - ref) <= TOL * ref), (lam, ref)
    norm_inf = abs(M).sum(axis=1).max()
    res = np.linalg.norm(M @ X - X * lam, axis=0)
    orth = np.max(np.abs(X.T @ X - np.eye(k)))
    print(f"{name} k={k}: {hist.shape[1] - 1} iterations, iters {iters.tolist()}, max residual / (tol lam) "
          f"{np.max(res / (TOL * lam)):.3f}, orthonormality {orth:.2e}, restarts {handle(name).eig_info()['restarts']}")
    assert np.all(res <= TOL * lam + 1e-12 * norm_inf * np.linalg.norm(X, axis=0))
    assert orth <= 1e-12
    assert hist.shape[1] >= iters.max() + 1  # the evaluation that ends the solve is recorded too


@pytest.mark.parametrize("name,k,max_iters", SOLVES)
def test_solver_follows_the_restatement(name, k, max_iters):
    lam, X, iters, hist, status = solved(name, k, max_iters)
    ref = restated(name, k, max_iters)
    assert not ref["breakdown"]
    nit, nit_ref = hist.shape[1] - 1, ref["hist"].shape[1] - 1
    m = min(nit, nit_ref) + 1
    err = np.abs(hist[:, :m] - ref["hist"][:, :m]) / ref["hist"][:, :m]
    tol = np.array([hist_tolerance(ref["hist"][c, :m]) for c in range(k)])
    print(f"{name} k={k}: {nit} iterations, restatement {nit_ref}; worst history deviation / tolerance {np.max(err / tol):.3e}")
    assert abs(nit - nit_ref) <= max(2, 0.1 * nit_ref)
    assert np.all(err <= tol), f"max history deviation / tolerance {np.max(err / tol):.3e} at {np.unravel_index(np.argmax(err / tol), err.shape)}"


def test_soft_locking_leaves_a_converged_column_alone():
    name, k = "p3_12_10_9", 3
    A = handle(name)
    nx, ny, nz = GRIDS[name]
    sx, sy, sz = (np.sin(np.arange(1, d + 1) * np.pi / (d + 1)) for d in (nx, ny, nz))
    v = (sz[:, None, None] * sy[None, :, None] * sx[None, None, :]).ravel()  # x runs fastest: the lowest eigenvector
    X0 = np.random.default_rng(5).standard_normal((A.nrow, k))
    X0[:, 0] = v
    lam, X, iters, hist, status = A.eigs(k, X0=X0, tol=TOL)
    assert np.all(status == sa.SPARSH_OK)
    assert iters[0] in (0, 1), iters
    assert iters[1:].min() > 1
    ref = analytic(name, k)
    assert np.all(np.abs(lam - ref) <= TOL * ref)
    assert abs(abs(X[:, 0] @ v) / np.linalg.norm(v) - 1.0) <= 1e-8


def test_cap_returns_the_last_ritz_pairs():
    name, k = "p3_12_10_9", 4
    A, M = handle(name), scipy_matrix(name)
    lam, X, iters, hist, status = A.eigs(k, tol=TOL, max_iters=3)
    assert A.last_eigs_rc == sa.SPARSH_ENOCONV
    assert np.any(status == sa.SPARSH_ENOCONV) and set(status.tolist()) <= {sa.SPARSH_OK, sa.SPARSH_ENOCONV}
    assert iters.max() == 3 and hist.shape[1] == 4
    assert np.max(np.abs(X.T @ X - np.eye(k))) <= 1e-12
    rq = np.einsum("ij,ij->j", X, M @ X) / np.einsum("ij,ij->j", X, X)
    assert np.all(np.abs(lam - rq) <= 1e-12 * np.abs(rq))
    assert np.all(np.diff(lam) >= 0)


def test_reproducible_and_isolated_from_the_linear_solvers():
    name = "p3_12_10_9"
    A = handle(name)
    n = A.nrow
    rng = np.random.default_rng(9)
    b, B = rng.standard_normal(n), rng.standard_normal((n, 3))

    def linear():
        x, Xm = np.zeros(n), np.zeros((n, 3))
        A.solve("pcg", b, x)
        A.solve_multi("pcg", B, Xm)
        return x, Xm

    x0, X0 = linear()
    lam1, V1, *_ = A.eigs(3, tol=TOL)
    x1, X1 = linear()
    lam2, V2, *_ = A.eigs(3, tol=TOL)
    assert np.array_equal(lam1, lam2) and np.array_equal(V1, V2)
    assert np.array_equal(x0, x1) and np.array_equal(X0, X1)
    A.eigs(8, tol=TOL, max_iters=2)  # another width: the solver's blocks are replaced
    lam3, V3, *_ = A.eigs(3, tol=TOL)
    assert np.array_equal(lam1, lam3) and np.array_equal(V1, V3)
    x2, X2 = linear()
    assert np.array_equal(x0, x2) and np.array_equal(X0, X2)


def test_memory_life_cycle():
    A = sa.sp_matrix_mg(*csr("p3_8")).setup(sa.default_params(**QUIET))
    n = A.nrow
    assert A.eig_info() == dict(width=0, bytes=0, restarts=0)

    def documented(W):  # include/sparsh_amg.h: seven blocks, partial sums, Gram matrices and norms, coefficients and theta
        return 8 * (7 * n * W + (12 * W * W + W) * 512 + 18 * W * W + W + 3 * W * W + W)

    A.eigs(3, tol=TOL, max_iters=2)
    info = A.eig_info()
    assert (info["width"], info["bytes"]) == (4, documented(4))
    A.eigs(8, tol=TOL, max_iters=2)
    info = A.eig_info()
    assert (info["width"], info["bytes"]) == (8, documented(8))
    A.setup(sa.default_params(**QUIET))
    assert A.eig_info() == dict(width=0, bytes=0, restarts=0)
    A.close()


def test_device_refusals():
    rp, ci, v = csr("p3_8")
    for prepare, word in ((lambda A: A.set_smoother("sor", 0, "symmetric"), "Jacobi"), (lambda A: A.set_smoother("chebyshev"), "Jacobi"),
                          (lambda A: A.set_cycle("w"), "V-cycle"), (lambda A: A.set_cycle("k"), "V-cycle")):
        A = sa.sp_matrix_mg(rp, ci, v)
        prepare(A)
        A.setup(sa.default_params(**QUIET))
        with pytest.raises(sa.SparshError) as e:
            A.eigs(2)
        assert e.value.code == sa.SPARSH_EINVAL and word in str(e.value)
        A.close()
    N = sa.sp_matrix_mg(*problems.poisson3d_neumann(8))
    N.set_nullspace("constant")
    N.setup(sa.default_params(**QUIET))
    with pytest.raises(sa.SparshError) as e:
        N.eigs(2)
    assert e.value.code == sa.SPARSH_EINVAL and "null space" in str(e.value)
    N.close()


def test_rank_deficient_or_nan_start_block_is_enumeric():
    A = handle("p3_8")
    X0 = np.random.default_rng(2).standard_normal((A.nrow, 3))
    X0[:, 2] = X0[:, 0]
    with pytest.raises(sa.SparshError) as e:
        A.eigs(3, X0=X0)
    assert e.value.code == sa.SPARSH_ENUMERIC and "rank deficient" in str(e.value)
    X0[5, 2] = np.nan
    with pytest.raises(sa.SparshError) as e:
        A.eigs(3, X0=X0)
    assert e.value.code == sa.SPARSH_ENUMERIC and "NaN" in str(e.value)
    lam, *_ = A.eigs(3)  # the handle is as good as before
    assert np.all(np.abs(lam - analytic("p3_8", 3)) <= TOL * analytic("p3_8", 3))
