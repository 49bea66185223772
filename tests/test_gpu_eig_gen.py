"""The generalised eigenproblem A x = lambda B x on the block path: the two new kernels through their
operator-level hooks, bitwise against numpy; the block SpMV with the stored B; B = I against the standard solver, bit for bit; whole
solves against the dense pencil and against the numpy restatement driven by the handle's own block operators; the life cycle of B
and of the three extra blocks; an indefinite B.  GPU box only."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import hist_tolerance
from eig_gen_restatement import CAP, PENCILS, SOLVES, TOL, check_solution, dense_reference, diag_b, lobpcg_gen, update_gen

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
RAGGED = (1, 2, 63, 64, 65, 255, 257, 1080, 70001)  # below, at and above a wave, a pass of a workgroup, several workgroups


@functools.lru_cache(maxsize=None)
def lender():
    """a ready handle: the kernel hooks borrow its stream only"""
    return sa.sp_matrix_mg(*problems.poisson3d(8)).setup(sa.default_params(**QUIET))


# ---------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("k", range(1, 9))
def test_residual_is_bitwise_numpy(k):
    A = lender()
    rng = np.random.default_rng(k)
    for n in RAGGED:
        AX, BX, theta = rng.standard_normal((n, k)), rng.standard_normal((n, k)), rng.standard_normal(k) * 3.0
        R, rn, bn = A.op_eig_residual_gen(AX, BX, theta)
        want = AX - BX * theta
        assert np.array_equal(R, want), (n, k)
        assert np.allclose(rn, np.linalg.norm(want, axis=0), rtol=1e-12, atol=0.0), (n, k)
        assert np.allclose(bn, np.linalg.norm(BX, axis=0), rtol=1e-12, atol=0.0), (n, k)
        # the norms of R carry the bits of the standard kernel's: with B = I the two solvers stop on the same numbers
        R2, rn2 = A.op_eig_residual(AX, BX, theta)
        assert np.array_equal(R, R2) and np.array_equal(rn, rn2), (n, k)


@pytest.mark.parametrize("k", (1, 2, 3, 5, 8))
def test_update_is_bitwise_the_restatement(k):
    A = lender()
    rng = np.random.default_rng(40 + k)
    names = ("X", "P", "AX", "AP", "BX", "BP")
    for n in (1, 63, 65, 257, 1080, 70001):
        blocks = [rng.standard_normal((n, k)) for _ in range(9)]
        coefs = [rng.standard_normal((k, k)) for _ in range(3)]
        for masked in (False, True):
            if masked:  # a zeroed row of Cw (an inactive column) and Cp = 0 (the first iteration)
                coefs[1][rng.integers(0, k), :] = 0.0
                coefs[2][:, :] = 0.0
            want = update_gen(*blocks, *coefs)
            got = A.op_eig_update_gen(blocks, *coefs)
            for name, g, w in zip(names, got, want):
                assert np.array_equal(g, w), (n, k, masked, name)
        got = A.op_eig_update_gen(blocks, *coefs, in_place=True)  # every output replaces its block on the device
        for name, g, w in zip(names, got, want):
            assert np.array_equal(g, w), (n, k, "in place", name)


# ---------------------------------------------------------------------------- handles

@functools.lru_cache(maxsize=None)
def pencil(name):
    return PENCILS[name][0]()


@functools.lru_cache(maxsize=None)
def handle(name):
    A, B = pencil(name)
    return sa.sp_matrix_mg(*A).setup(sa.default_params(**QUIET, **PENCILS[name][1])).set_eig_b(*B)


@functools.lru_cache(maxsize=None)
def reference(name):
    return dense_reference(*pencil(name), 8)


def test_block_spmv_with_b_is_bitwise_the_single_vector_operator():
    rng = np.random.default_rng(21)
    # the mass matrix: against the single-vector SpMV of a handle whose operator is M itself
    A = handle("fem_1l")
    M = pencil("fem_1l")[1]
    S = sa.sp_matrix_mg(*M).setup(sa.default_params(**QUIET))
    X = rng.standard_normal((A.nrow, 8))
    want = np.column_stack([S.op_spmv_dot(0, X[:, c])[0] for c in range(8)])
    for k in (1, 2, 3, 4, 5, 8):  # every width, with and without padding columns
        assert np.array_equal(A.op_eig_b_multi(X[:, :k]), want[:, :k]), k
    S.close()
    # a diagonal B: one product per row
    D = handle("p3_diag")
    d = diag_b(D.nrow)[2]
    X = rng.standard_normal((D.nrow, 8))
    for k in (1, 2, 3, 4, 5, 8):
        assert np.array_equal(D.op_eig_b_multi(X[:, :k]), X[:, :k] * d[:, None]), k
    assert D.eig_b_info()["nnz"] == D.nrow and A.eig_b_info()["nnz"] == len(M[1])
    assert A.eig_b_info()["is_set"] and A.eig_b_info()["bytes"] >= 12 * len(M[1])


# ---------------------------------------------------------------------------- B = I

@pytest.mark.parametrize("k", (4, 7))
def test_identity_b_gives_the_bits_of_the_standard_solver(k):
    A = sa.sp_matrix_mg(*problems.poisson3d(8)).setup(sa.default_params(**QUIET))
    n = A.nrow
    lam, X, iters, hist, status = A.eigs(k, tol=TOL)
    A.set_eig_b(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    glam, gX, giters, ghist, gstatus = A.eigs_gen(k, tol=TOL)
    assert np.all(status == sa.SPARSH_OK) and np.all(gstatus == sa.SPARSH_OK)
    nit, gnit = hist.shape[1] - 1, ghist.shape[1] - 1
    print(f"k={k}: {nit} iterations, generalised {gnit}")
    assert abs(nit - gnit) <= 1  # the stopping rule multiplies by ||x_c||, which is 1 only to rounding
    m = min(nit, gnit) + 1
    assert np.array_equal(hist[:, :m], ghist[:, :m])
    if nit != gnit:  # the pairs after the iterations both ran: stop both there
        lam, X, *_ = A.eigs(k, tol=TOL, max_iters=m - 1)
        glam, gX, *_ = A.eigs_gen(k, tol=TOL, max_iters=m - 1)
    assert np.array_equal(lam, glam) and np.array_equal(X, gX)
    A.close()


# ---------------------------------------------------------------------------- whole solves

@functools.lru_cache(maxsize=None)
def solved(name, k):
    return handle(name).eigs_gen(k, tol=TOL, max_iters=CAP)


@functools.lru_cache(maxsize=None)
def restated(name, k):
    """the restatement with the handle's own block SpMVs, block V-cycle and Gram launch (test_gpu_eig.restated says why the last)"""
    A = handle(name)
    X0 = np.random.default_rng(0).standard_normal((A.nrow, k))
    return lobpcg_gen(lambda X: A.op_spmv_dot_multi(0, X)[0], A.op_eig_b_multi, A.op_precond_multi, X0, tol=TOL, max_iters=CAP,
                      gram=A.op_gram_multi)


@pytest.mark.parametrize("name,k", SOLVES)
def test_solver_finds_the_lowest_pairs_of_the_pencil(name, k):
    lam, X, iters, hist, status = solved(name, k)
    H = handle(name)
    print(f"{name} k={k}: {H.nlevels} levels, {hist.shape[1] - 1} iterations, iters {iters.tolist()}, restarts {H.eig_info()['restarts']}, "
          f"final residual norms {hist[:, -1].tolist()}")
    assert np.all(status == sa.SPARSH_OK), hist[:, -1]
    assert H.last_eigs_rc == sa.SPARSH_OK
    check_solution(name, k, lam, X, *pencil(name), reference(name))
    assert hist.shape[1] >= iters.max() + 1  # the evaluation that ends the solve is recorded too


@pytest.mark.parametrize("name,k", SOLVES)
def test_solver_follows_the_restatement(name, k):
    lam, X, iters, hist, status = solved(name, k)
    ref = restated(name, k)
    assert not ref["breakdown"]
    nit, nit_ref = hist.shape[1] - 1, ref["hist"].shape[1] - 1
    m = min(nit, nit_ref) + 1
    err = np.abs(hist[:, :m] - ref["hist"][:, :m]) / ref["hist"][:, :m]
    tol = np.array([hist_tolerance(ref["hist"][c, :m]) for c in range(k)])
    print(f"{name} k={k}: {nit} iterations, restatement {nit_ref}; worst history deviation / tolerance {np.max(err / tol):.3e}")
    assert abs(nit - nit_ref) <= max(2, 0.1 * nit_ref)
    assert np.all(err <= tol), f"max history deviation / tolerance {np.max(err / tol):.3e} at {np.unravel_index(np.argmax(err / tol), err.shape)}"


def test_eigs_gen_dev_gives_the_bits_of_eigs_gen():
    name, k = "p3_diag", 3
    A = handle(name)
    n = A.nrow
    lam, X, iters, hist, status = solved(name, k)
    X0 = np.asfortranarray(np.random.default_rng(0).standard_normal((n, k)))
    d = A.dev_alloc(X0.nbytes)
    A.h2d(d, X0.T)  # (h2d sends a C-ordered copy: the transpose's is the column-major block)
    dlam, diters, dhist, dstatus, sec, rc = A.eigs_gen_dev(k, d, n, tol=TOL, max_iters=CAP)
    out = np.zeros_like(X0, order="F")
    A.d2h(out, d)
    A.dev_free(d)
    assert rc == sa.SPARSH_OK and sec > 0.0
    assert np.array_equal(dlam, lam) and np.array_equal(out, X) and np.array_equal(dhist, hist) and np.array_equal(diters, iters)


# ---------------------------------------------------------------------------- life cycle

def test_life_cycle_of_b_and_of_the_extra_blocks():
    rp, ci, v = problems.poisson3d(12, 10, 9)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
    n = A.nrow
    rng = np.random.default_rng(9)
    b, Bm = rng.standard_normal(n), rng.standard_normal((n, 3))

    def others():
        x, Xm = np.zeros(n), np.zeros((n, 3))
        A.solve("pcg", b, x)
        A.solve_multi("pcg", Bm, Xm)
        lam, V, *_ = A.eigs(3, tol=TOL)
        return x, Xm, lam, V

    assert A.eig_b_info() == dict(is_set=False, nnz=0, bytes=0)
    with pytest.raises(sa.SparshError) as e:
        A.eigs_gen(3)
    assert e.value.code == sa.SPARSH_ESTATE and "sparsh_eig_set_b" in str(e.value)
    before = others()
    std = A.eig_info()  # the standard solver's reservation for width 4
    A.set_eig_b(*diag_b(n))
    info = A.eig_b_info()
    assert info["is_set"] and info["nnz"] == n and info["bytes"] > 0
    assert A.eig_info()["bytes"] == std["bytes"]  # B is not the solver's block memory, and nothing is reserved before a generalised call
    lam1, V1, *_ = A.eigs_gen(3, tol=TOL)
    assert A.eig_info()["width"] == 4 and A.eig_info()["bytes"] == std["bytes"] + 3 * n * 4 * 8  # exactly three blocks more
    after = others()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert A.eig_info()["bytes"] == std["bytes"] + 3 * n * 4 * 8  # counted from then on, for this width
    lam2, V2, *_ = A.eigs_gen(3, tol=TOL)
    assert np.array_equal(lam1, lam2) and np.array_equal(V1, V2)
    # a replacement, then the two ways of dropping B
    A.set_eig_b(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0))
    lam3, *_ = A.eigs_gen(3, tol=TOL)
    assert np.all(np.abs(2.0 * lam3 - after[2]) <= 1e-7 * after[2])  # B = 2 I halves the eigenvalues
    A.set_eig_b(None)
    assert A.eig_b_info() == dict(is_set=False, nnz=0, bytes=0)
    with pytest.raises(sa.SparshError) as e:
        A.eigs_gen(3)
    assert e.value.code == sa.SPARSH_ESTATE
    A.set_eig_b(*diag_b(n))
    A.setup(sa.default_params(**QUIET))
    assert A.eig_b_info() == dict(is_set=False, nnz=0, bytes=0)
    assert A.eig_info() == dict(width=0, bytes=0, restarts=0)
    A.close()


def test_indefinite_b_is_enumeric_at_the_start():
    A = sa.sp_matrix_mg(*problems.poisson3d(8)).setup(sa.default_params(**QUIET))
    n = A.nrow
    B = sp.identity(n, format="lil")
    B[0, 1] = B[1, 0] = 2.0  # the block [[1, 2], [2, 1]]: eigenvalues 3 and -1, and a positive diagonal
    B = B.tocsr()
    B.sort_indices()
    A.set_eig_b(B.indptr.astype(np.int32), B.indices.astype(np.int32), B.data)
    X0 = np.zeros((n, 2))
    X0[0, 0], X0[1, 0] = 1.0, -1.0  # x^T B x = -2
    X0[5, 1] = 1.0
    Xf = np.asfortranarray(X0)
    lam, hist, iters, status = np.zeros(2), np.zeros((2, 4)), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = sa.lib.sparsh_eigs_gen(A._h, 2, Xf.ctypes.data_as(DP), n, TOL, 0, lam.ctypes.data_as(DP), hist.ctypes.data_as(DP), 4,
                                iters.ctypes.data_as(IP), status.ctypes.data_as(IP))
    msg = sa.lib.sparsh_last_error().decode()
    assert rc == sa.SPARSH_ENUMERIC and "breakdown at the start" in msg and "positive definite" in msg
    assert np.all(status == sa.SPARSH_ENUMERIC)
    assert np.array_equal(Xf, X0)  # X is not written
    with pytest.raises(sa.SparshError) as e:
        A.eigs_gen(2, X0=X0)
    assert e.value.code == sa.SPARSH_ENUMERIC
    A.set_eig_b(None)
    lam, *_ = A.eigs(2, tol=TOL)  # the handle is as good as before
    assert np.all(lam > 0)
    A.close()
