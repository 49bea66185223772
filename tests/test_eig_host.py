"""The host side of the LOBPCG eigensolver: the Rayleigh-Ritz step sparsh_debug_eig_small against
scipy.linalg.eigh, its breakdown rule, the numpy restatement of the whole algorithm against analytic eigenvalues, and the argument
and state errors of sparsh_eigs / sparsh_eigs_dev / sparsh_eig_info on handles without a device.  CPU only."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from eig_restatement import lobpcg, small_eig

QUIET = dict(print_setup=0, print_solve=0)
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
ORDERS = (1, 2, 3, 8, 9, 16, 24)
Q_COND = 30.0  # condition number of Q before its columns are scaled (the Gram matrix has its square)


def pencil(m, seed):
    """GB = Q^T Q, GA = Q^T K Q: Q tall with singular values 1 .. 1 / Q_COND, its columns then scaled over 1e-6 .. 1e6 (so the
    solver's diagonal scaling matters), K = diag(1, 2, ...)."""
    rng = np.random.default_rng(seed)
    N = 2 * m + 8
    U, _ = np.linalg.qr(rng.standard_normal((N, m)))
    V, _ = np.linalg.qr(rng.standard_normal((m, m)))
    s = np.geomspace(1.0, 1.0 / Q_COND, m) if m > 1 else np.ones(1)
    Q = (U * s) @ V.T
    Q = Q * (np.geomspace(1e-6, 1e6, m)[rng.permutation(m)] if m > 1 else 1e-6)
    K = np.arange(1.0, N + 1)
    return Q.T @ (K[:, None] * Q), Q.T @ Q


def pencil_errors(GA, GB, theta, Cm):
    k = len(theta)
    w = scipy.linalg.eigh(GA, GB, eigvals_only=True)[:k]
    res = GA @ Cm - (GB @ Cm) * theta
    return (np.max(np.abs(theta - w) / np.abs(w)), np.max(np.abs(Cm.T @ GB @ Cm - np.eye(k))),
            np.max(np.linalg.norm(res, axis=0) / np.linalg.norm(GA @ Cm, axis=0)))


@pytest.mark.parametrize("m", ORDERS)
@pytest.mark.parametrize("solver", ["restatement", "library"])
def test_small_eigenproblem_matches_scipy_eigh(m, solver):
    for k in sorted({1, min(m, 8)}):
        for seed in range(3):
            GA, GB = pencil(m, 10 * m + seed)
            bad, theta, Cm = small_eig(GA, GB, k) if solver == "restatement" else sa.eig_small(GA, GB, k)
            assert bad == 0
            assert np.all(np.diff(theta) >= 0)
            e_theta, e_orth, e_res = pencil_errors(GA, GB, theta, Cm)
            print(f"{solver} m={m} k={k} seed={seed}: theta {e_theta:.2e} orthonormality {e_orth:.2e} residual {e_res:.2e}")
            assert e_theta <= 1e-12 and e_orth <= 1e-12 and e_res <= 1e-12


@pytest.mark.parametrize("m", ORDERS)
def test_restatement_and_library_give_the_same_bits(m):
    """the restatement adds in the library's order, so a solve restated with the device's own Gram matrices follows the engine exactly
    -- also inside a multiple eigenvalue, where the Ritz vectors hang on the last bits"""
    k = min(m, 8)
    GA, GB = pencil(m, 77 + m)
    rng = np.random.default_rng(m)
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    lam = np.maximum(1.0, np.arange(m) - 1.0)  # a triple eigenvalue at the bottom (m >= 3)
    for ga, gb in ((GA, GB), ((Q * lam) @ Q.T, np.eye(m) + 1e-3 * (Q + Q.T))):
        bad, theta, Cm = sa.eig_small(ga, gb, k)
        bad2, theta2, Cm2 = small_eig(ga, gb, k)
        assert bad == bad2 == 0
        assert np.array_equal(theta, theta2) and np.array_equal(Cm, Cm2)


def test_small_eigenproblem_reads_the_upper_triangles_only():
    GA, GB = pencil(9, 5)
    _, theta, Cm = sa.eig_small(GA, GB, 4)
    _, theta2, Cm2 = sa.eig_small(np.triu(GA) + 7.0 * np.tril(GA, -1), np.triu(GB) - np.tril(GB, -1), 4)
    assert np.array_equal(theta, theta2) and np.array_equal(Cm, Cm2)


def test_breakdown_rule():
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((30, 6))
    Q[:, 4] = Q[:, 1]  # two equal columns: the scaled Gram matrix is singular
    K = np.arange(1.0, 31.0)
    GA, GB = Q.T @ (K[:, None] * Q), Q.T @ Q
    assert sa.eig_small(GA, GB, 3)[0] == 1
    assert small_eig(GA, GB, 3)[0] == 1
    # unit diagonal and a smallest Cholesky pivot of 1e-3: far from the 1e-7 of the rule
    c = np.sqrt(1.0 - 1e-6)
    GB = np.array([[1.0, c], [c, 1.0]])
    GA = np.array([[1.0, c * 1.5], [c * 1.5, 2.0]])
    bad, theta, Cm = sa.eig_small(GA, GB, 2)
    assert bad == 0 and small_eig(GA, GB, 2)[0] == 0
    assert np.allclose(theta, scipy.linalg.eigh(GA, GB, eigvals_only=True), rtol=1e-8)
    # a pivot just under the rule, a non-positive and a NaN diagonal entry
    c = np.sqrt(1.0 - 0.25e-14)
    assert sa.eig_small(np.eye(2), np.array([[1.0, c], [c, 1.0]]), 1)[0] == 1
    assert sa.eig_small(np.eye(2), np.diag([1.0, 0.0]), 1)[0] == 1
    assert sa.eig_small(np.eye(2), np.diag([1.0, np.nan]), 1)[0] == 1
    # bad orders are bad arguments
    for m, k in ((0, 1), (25, 1), (4, 0), (4, 5), (12, 9)):
        z = np.zeros(max(m * m, 1))
        assert sa.lib.sparsh_debug_eig_small(m, k, z.ctypes.data_as(DP), z.ctypes.data_as(DP), z.ctypes.data_as(DP), z.ctypes.data_as(DP)) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_debug_eig_small(2, 1, None, None, None, None) == sa.SPARSH_EINVAL


def analytic_poisson3d(nx, ny, nz, k):
    lam = (6.0 - 2.0 * np.cos(np.arange(1, nx + 1) * np.pi / (nx + 1))[:, None, None]
           - 2.0 * np.cos(np.arange(1, ny + 1) * np.pi / (ny + 1))[None, :, None]
           - 2.0 * np.cos(np.arange(1, nz + 1) * np.pi / (nz + 1))[None, None, :])
    return np.sort(lam.ravel())[:k]


@pytest.mark.parametrize("dims,k", [((8, 8, 8), 4), ((12, 10, 9), 3)])
def test_restatement_reaches_the_analytic_eigenvalues(dims, k):
    rp, ci, v = problems.poisson3d(*dims)
    n = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    lu = spla.splu(A.tocsc())
    tol = 1e-8
    X0 = np.random.default_rng(0).standard_normal((n, k))
    out = lobpcg(lambda X: A @ X, lambda R: lu.solve(R), X0, tol=tol, max_iters=100)
    assert not out["breakdown"] and not out["status"].any()
    ref = analytic_poisson3d(*dims, k)
    assert np.all(np.diff(out["lam"]) >= 0)
    assert np.all(np.abs(out["lam"] - ref) <= tol * ref), (out["lam"], ref)
    X = out["X"]
    assert np.max(np.abs(X.T @ X - np.eye(k))) <= 1e-12
    assert np.all(np.linalg.norm(A @ X - X * out["lam"], axis=0) <= tol * out["lam"] + 1e-12 * 12.0)
    assert out["hist"].shape[0] == k and out["hist"].shape[1] >= out["iters"].max() + 1  # the evaluation that ends the solve is recorded


# ---------------------------------------------------------------------------- refusals without a device

def raw_eigs(A, nev, X, ldx, tol=1e-8, max_iters=0, hist_cap=4, lam=True, hist=True, iters=True, status=True, dev=False):
    """the C entry point itself: X a numpy array or None (a NULL pointer)"""
    h = np.zeros((8, max(hist_cap, 1)))
    la, it, st = np.zeros(8), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    args = [A._h, nev, None if X is None else X.ctypes.data_as(C.c_void_p if dev else DP), ldx, tol, max_iters,
            la.ctypes.data_as(DP) if lam else None, h.ctypes.data_as(DP) if hist else None, hist_cap,
            it.ctypes.data_as(IP) if iters else None, st.ctypes.data_as(IP) if status else None]
    if dev:
        args.append(None)
    return (sa.lib.sparsh_eigs_dev if dev else sa.lib.sparsh_eigs)(*args)


@pytest.fixture(scope="module")
def problem():
    rp, ci, v = problems.poisson2d(40)
    n = len(rp) - 1
    return rp, ci, v, n, np.ones((n, 8), order="F")


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_bad_arguments_are_einval_without_a_device(problem, dev, prepared):
    rp, ci, v, n, X = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    for nev in (0, -1, 9, 100):
        assert raw_eigs(A, nev, X, n, dev=dev) == sa.SPARSH_EINVAL, nev
        assert b"nev" in sa.lib.sparsh_last_error()
    assert raw_eigs(A, 4, None, n, dev=dev) == sa.SPARSH_EINVAL
    assert raw_eigs(A, 4, X, n, lam=False, dev=dev) == sa.SPARSH_EINVAL
    assert raw_eigs(A, 4, X, n, hist=False, dev=dev) == sa.SPARSH_EINVAL
    assert raw_eigs(A, 4, X, n, iters=False, dev=dev) == sa.SPARSH_EINVAL
    assert raw_eigs(A, 4, X, n, status=False, dev=dev) == sa.SPARSH_EINVAL
    assert b"NULL" in sa.lib.sparsh_last_error()
    assert raw_eigs(A, 4, X, n, hist_cap=-1, dev=dev) == sa.SPARSH_EINVAL
    assert raw_eigs(A, 4, X, n - 1, dev=dev) == sa.SPARSH_EINVAL
    assert raw_eigs(A, 4, X, 0, dev=dev) == sa.SPARSH_EINVAL
    assert b"ldx" in sa.lib.sparsh_last_error()
    for tol in (0.0, -1e-8, np.inf, -np.inf, np.nan):
        assert raw_eigs(A, 4, X, n, tol=tol, dev=dev) == sa.SPARSH_EINVAL, tol
        assert b"tol" in sa.lib.sparsh_last_error()
    # valid arguments (a history is optional with hist_cap = 0): the call order is what is wrong
    assert raw_eigs(A, 4, X, n, dev=dev) == sa.SPARSH_ESTATE
    assert raw_eigs(A, 1, X, n + 5, dev=dev) == sa.SPARSH_ESTATE
    assert raw_eigs(A, 8, X, n, hist_cap=0, hist=False, max_iters=-3, dev=dev) == sa.SPARSH_ESTATE


@pytest.mark.parametrize("dev", [False, True])
def test_nev_above_the_number_of_rows_is_einval(dev):
    rp, ci, v = problems.poisson2d(2)  # 4 rows
    A = sa.sp_matrix_mg(rp, ci, v)
    X = np.ones((4, 8), order="F")
    assert raw_eigs(A, 5, X, 4, dev=dev) == sa.SPARSH_EINVAL
    assert b"rows" in sa.lib.sparsh_last_error()
    assert raw_eigs(A, 4, X, 4, dev=dev) == sa.SPARSH_ESTATE


@pytest.mark.parametrize("dev", [False, True])
def test_handles_an_eigen_solve_cannot_run_on_are_einval(problem, dev):
    rp, ci, v, n, X = problem
    # a smoother other than Jacobi, selected before or after the host setup; Jacobi again lifts the refusal
    A = sa.sp_matrix_mg(rp, ci, v)
    for kind, order in (("sor", "symmetric"), ("sor", "forward"), ("chebyshev", "forward")):
        A.set_smoother(kind, 0, order)
        assert raw_eigs(A, 4, X, n, dev=dev) == sa.SPARSH_EINVAL, kind
        assert b"Jacobi" in sa.lib.sparsh_last_error()
    A.setup(sa.default_params(**QUIET), host_only=True)
    assert raw_eigs(A, 4, X, n, dev=dev) == sa.SPARSH_EINVAL
    A.set_smoother("jacobi")
    assert raw_eigs(A, 4, X, n, dev=dev) == sa.SPARSH_ESTATE
    # W- and K-cycles
    for kind in ("w", "k"):
        A.set_cycle(kind)
        assert raw_eigs(A, 4, X, n, dev=dev) == sa.SPARSH_EINVAL, kind
        assert b"V-cycle" in sa.lib.sparsh_last_error()
    A.set_cycle("v")
    assert raw_eigs(A, 4, X, n, dev=dev) == sa.SPARSH_ESTATE
    # params.precond_fp32
    F = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, precond_fp32=1), host_only=True)
    assert raw_eigs(F, 4, X, n, dev=dev) == sa.SPARSH_EINVAL
    assert b"precond_fp32" in sa.lib.sparsh_last_error()
    # a null-space handle
    rpn, cin, vn = problems.poisson3d_neumann(6)
    N = sa.sp_matrix_mg(rpn, cin, vn)
    N.set_nullspace("constant")
    N.setup(sa.default_params(**QUIET), host_only=True)
    assert raw_eigs(N, 4, np.ones((216, 4), order="F"), 216, dev=dev) == sa.SPARSH_EINVAL
    assert b"null space" in sa.lib.sparsh_last_error()
    # a handle with a multi-rank transport installed
    group = sa.comm_group_create(2)
    try:
        P = sa.sp_matrix_mg(rp, ci, v)
        P.comm_init_group(group, 0)
        assert raw_eigs(P, 4, X, n, dev=dev) == sa.SPARSH_EINVAL
        assert b"partitioned" in sa.lib.sparsh_last_error()
        P.close()
    finally:
        sa.comm_group_destroy(group)


def test_python_wrappers_raise_the_same_codes(problem):
    rp, ci, v, n, X = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    with pytest.raises(sa.SparshError) as e:
        A.eigs(4)
    assert e.value.code == sa.SPARSH_ESTATE
    for k in (0, 9):
        with pytest.raises(sa.SparshError) as e:
            A.eigs(k)
        assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.eigs(4, tol=0.0)
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(ValueError):
        A.eigs(3, X0=X[:, :4])
    for call in (lambda: A.op_gram_multi(X[:, :2], X[:, :3]), lambda: A.op_eig_residual(X[:, :2], X[:, :2], np.ones(2)),
                 lambda: A.bench_op_multi("eig_gram", 0, nrhs=4)):
        with pytest.raises(sa.SparshError) as e:
            call()
        assert e.value.code == sa.SPARSH_ESTATE


def test_eig_info_is_zero_on_a_fresh_handle(problem):
    rp, ci, v, n, _ = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    assert A.eig_info() == dict(width=0, bytes=0, restarts=0)
    A.setup(sa.default_params(**QUIET), host_only=True)
    assert A.eig_info() == dict(width=0, bytes=0, restarts=0)
    assert sa.lib.sparsh_eig_info(None, None, None, None) == sa.SPARSH_EINVAL
