"""The host side of the constrained LOBPCG eigensolver: the argument and state errors of sparsh_eigs_con /
sparsh_eigs_con_dev / sparsh_eig_con_info on handles without a device, null-space handles let through, the numpy restatement on a
singular operator and past the first block of eigenvalues, and the dumbbell graph of problems.py.  CPU only."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from eig_con_restatement import DUMBBELL, Projector, lobpcg_con, spd_inverse

QUIET = dict(print_setup=0, print_solve=0)
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def raw_eigs(A, nev, X, ldx, dev=False):
    """sparsh_eigs / sparsh_eigs_dev themselves with good arguments"""
    h, la, it, st = np.zeros((8, 4)), np.zeros(8), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    args = [A._h, nev, X.ctypes.data_as(C.c_void_p if dev else DP), ldx, 1e-8, 0, la.ctypes.data_as(DP), h.ctypes.data_as(DP), 4,
            it.ctypes.data_as(IP), st.ctypes.data_as(IP)]
    return (sa.lib.sparsh_eigs_dev if dev else sa.lib.sparsh_eigs)(*(args + ([None] if dev else [])))


def raw_eigs_con(A, nev, X, ldx, ncon=0, Y=None, ldy=0, gen=0, tol=1e-8, max_iters=0, hist_cap=4, lam=True, hist=True, iters=True, status=True,
                 dev=False):
    """the C entry point itself: X, Y numpy arrays or None (NULL pointers)"""
    h = np.zeros((8, max(hist_cap, 1)))
    la, it, st = np.zeros(8), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    ptr = C.c_void_p if dev else DP
    args = [A._h, gen, nev, None if X is None else X.ctypes.data_as(ptr), ldx, ncon, None if Y is None else Y.ctypes.data_as(ptr), ldy, tol,
            max_iters, la.ctypes.data_as(DP) if lam else None, h.ctypes.data_as(DP) if hist else None, hist_cap,
            it.ctypes.data_as(IP) if iters else None, st.ctypes.data_as(IP) if status else None]
    if dev:
        args.append(None)
    return (sa.lib.sparsh_eigs_con_dev if dev else sa.lib.sparsh_eigs_con)(*args)


@pytest.fixture(scope="module")
def problem():
    rp, ci, v = problems.poisson2d(40)
    n = len(rp) - 1
    return rp, ci, v, n, np.ones((n, 8), order="F"), np.ones((n, 17), order="F")


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_bad_arguments_are_einval_without_a_device(problem, dev, prepared):
    rp, ci, v, n, X, Y = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    err = sa.lib.sparsh_last_error
    # what sparsh_eigs refuses
    for nev in (0, -1, 9, 100):
        assert raw_eigs_con(A, nev, X, n, dev=dev) == sa.SPARSH_EINVAL and b"nev" in err()
    assert raw_eigs_con(A, 4, None, n, dev=dev) == sa.SPARSH_EINVAL
    for missing in ("lam", "hist", "iters", "status"):
        assert raw_eigs_con(A, 4, X, n, dev=dev, **{missing: False}) == sa.SPARSH_EINVAL and b"NULL" in err()
    assert raw_eigs_con(A, 4, X, n, hist_cap=-1, dev=dev) == sa.SPARSH_EINVAL
    assert raw_eigs_con(A, 4, X, n - 1, dev=dev) == sa.SPARSH_EINVAL and b"ldx" in err()
    for tol in (0.0, -1e-8, np.inf, np.nan):
        assert raw_eigs_con(A, 4, X, n, tol=tol, dev=dev) == sa.SPARSH_EINVAL and b"tol" in err()
    # the constraints
    for ncon in (-1, 17, 100):
        assert raw_eigs_con(A, 4, X, n, ncon, Y, n, dev=dev) == sa.SPARSH_EINVAL and b"ncon" in err()
    assert raw_eigs_con(A, 4, X, n, 3, None, n, dev=dev) == sa.SPARSH_EINVAL and b"NULL" in err()
    assert raw_eigs_con(A, 4, X, n, 3, Y, n - 1, dev=dev) == sa.SPARSH_EINVAL and b"ldy" in err()
    assert raw_eigs_con(A, 4, X, n, 3, Y, 0, dev=dev) == sa.SPARSH_EINVAL and b"ldy" in err()
    for gen in (-1, 2):
        assert raw_eigs_con(A, 4, X, n, 3, Y, n, gen=gen, dev=dev) == sa.SPARSH_EINVAL and b"gen" in err()
    # valid arguments: the call order is what is wrong (no setup, or no device; gen = 1: no B either)
    assert raw_eigs_con(A, 4, X, n, dev=dev) == sa.SPARSH_ESTATE  # Y may be NULL and ldy anything with ncon = 0
    assert raw_eigs_con(A, 8, X, n + 5, 16, Y, n + 1, dev=dev) == sa.SPARSH_ESTATE
    assert raw_eigs_con(A, 1, X, n, 1, Y, n, gen=1, hist_cap=0, hist=False, dev=dev) == sa.SPARSH_ESTATE


@pytest.mark.parametrize("dev", [False, True])
def test_pairs_and_constraints_above_the_number_of_rows_are_einval(dev):
    rp, ci, v = problems.poisson2d(3)  # 9 rows
    A = sa.sp_matrix_mg(rp, ci, v)
    X, Y = np.ones((9, 8), order="F"), np.ones((9, 16), order="F")
    assert raw_eigs_con(A, 4, X, 9, 6, Y, 9, dev=dev) == sa.SPARSH_EINVAL and b"rows" in sa.lib.sparsh_last_error()
    assert raw_eigs_con(A, 4, X, 9, 5, Y, 9, dev=dev) == sa.SPARSH_ESTATE
    # a null-space handle counts its constant vector
    rp, ci, v = problems.poisson3d_neumann(2)  # 8 rows
    N = sa.sp_matrix_mg(rp, ci, v)
    N.set_nullspace("constant")
    N.setup(sa.default_params(**QUIET), host_only=True)
    X, Y = np.ones((8, 8), order="F"), np.ones((8, 16), order="F")
    assert raw_eigs_con(N, 4, X, 8, 4, Y, 8, dev=dev) == sa.SPARSH_EINVAL and b"rows" in sa.lib.sparsh_last_error()
    assert raw_eigs_con(N, 4, X, 8, 3, Y, 8, dev=dev) == sa.SPARSH_ESTATE


@pytest.mark.parametrize("dev", [False, True])
def test_handles_a_constrained_solve_cannot_run_on(problem, dev):
    rp, ci, v, n, X, Y = problem
    err = sa.lib.sparsh_last_error
    A = sa.sp_matrix_mg(rp, ci, v)
    A.set_smoother("sor", 0, "symmetric")
    assert raw_eigs_con(A, 4, X, n, 2, Y, n, dev=dev) == sa.SPARSH_EINVAL and b"Jacobi" in err()
    A.set_smoother("jacobi")
    A.set_cycle("w")
    assert raw_eigs_con(A, 4, X, n, 2, Y, n, dev=dev) == sa.SPARSH_EINVAL and b"V-cycle" in err()
    A.set_cycle("v")
    assert raw_eigs_con(A, 4, X, n, 2, Y, n, dev=dev) == sa.SPARSH_ESTATE
    F = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, precond_fp32=1), host_only=True)
    assert raw_eigs_con(F, 4, X, n, dev=dev) == sa.SPARSH_EINVAL and b"precond_fp32" in err()
    group = sa.comm_group_create(2)
    try:
        P = sa.sp_matrix_mg(rp, ci, v)
        P.comm_init_group(group, 0)
        assert raw_eigs_con(P, 4, X, n, dev=dev) == sa.SPARSH_EINVAL and b"partitioned" in err()
        P.close()
    finally:
        sa.comm_group_destroy(group)


@pytest.mark.parametrize("dev", [False, True])
def test_a_null_space_handle_is_accepted_here_and_still_refused_by_eigs(dev):
    rp, ci, v = problems.poisson3d_neumann(6)
    N = sa.sp_matrix_mg(rp, ci, v)
    N.set_nullspace("constant")
    N.setup(sa.default_params(**QUIET), host_only=True)
    X, Y = np.ones((216, 4), order="F"), np.ones((216, 2), order="F")
    assert raw_eigs_con(N, 4, X, 216, dev=dev) == sa.SPARSH_ESTATE  # accepted: only the device is missing
    assert raw_eigs_con(N, 4, X, 216, 2, Y, 216, dev=dev) == sa.SPARSH_ESTATE
    assert raw_eigs(N, 4, X, 216, dev=dev) == sa.SPARSH_EINVAL and b"null space" in sa.lib.sparsh_last_error()
    assert N.eig_con_info() == dict(ncon_total=0, implicit_constant=0, bytes=0)  # nothing reserved yet
    # B for the normalised cut: sparsh_eig_con_set_b lets the handle through, sparsh_eig_set_b does not; B's own defects come first
    rpb, cib, vb = np.arange(217, dtype=np.int32), np.arange(216, dtype=np.int32), np.full(216, 2.0)
    b_args = lambda v: (N._h, rpb.ctypes.data_as(IP), cib.ctypes.data_as(IP), v.ctypes.data_as(DP))
    assert sa.lib.sparsh_eig_con_set_b(*b_args(vb)) == sa.SPARSH_ESTATE
    assert sa.lib.sparsh_eig_set_b(*b_args(vb)) == sa.SPARSH_EINVAL and b"null space" in sa.lib.sparsh_last_error()
    assert sa.lib.sparsh_eig_con_set_b(*b_args(-vb)) == sa.SPARSH_EINVAL and b"diagonal" in sa.lib.sparsh_last_error()
    assert sa.lib.sparsh_eig_con_set_b(N._h, None, None, None) == sa.SPARSH_OK
    with pytest.raises(sa.SparshError) as e:
        N.set_eig_b(rpb, cib, vb, con=True)
    assert e.value.code == sa.SPARSH_ESTATE
    N.set_smoother("sor", 0, "symmetric")
    assert sa.lib.sparsh_eig_con_set_b(*b_args(vb)) == sa.SPARSH_EINVAL and b"Jacobi" in sa.lib.sparsh_last_error()


def test_python_wrappers_and_info_on_a_fresh_handle(problem):
    rp, ci, v, n, X, Y = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    assert A.eig_con_info() == dict(ncon_total=0, implicit_constant=0, bytes=0)
    assert sa.lib.sparsh_eig_con_info(None, None, None, None) == sa.SPARSH_EINVAL
    for call, code in ((lambda: A.eigs_con(4), sa.SPARSH_ESTATE), (lambda: A.eigs_con(4, Y=Y[:, :3]), sa.SPARSH_ESTATE),
                       (lambda: A.eigs_con(4, Y=Y[:, :3], gen=True), sa.SPARSH_ESTATE), (lambda: A.eigs_con(9), sa.SPARSH_EINVAL),
                       (lambda: A.eigs_con(4, Y=Y), sa.SPARSH_EINVAL), (lambda: A.eigs_con(4, tol=0.0), sa.SPARSH_EINVAL),
                       (lambda: A.op_eig_con_project(Y[:5, :2], Y[:5, :2], np.eye(2), X[:5, :2]), sa.SPARSH_ESTATE),
                       (lambda: A.bench_op_multi("eig_con_project", 0, nrhs=8), sa.SPARSH_ESTATE)):
        with pytest.raises(sa.SparshError) as e:
            call()
        assert e.value.code == code
    with pytest.raises(ValueError):
        A.eigs_con(4, Y=np.ones((n + 1, 2)))
    A.setup(sa.default_params(**QUIET), host_only=True)
    assert A.eig_con_info() == dict(ncon_total=0, implicit_constant=0, bytes=0)


# ---------------------------------------------------------------------------- the restatement

def test_spd_inverse_and_its_breakdown_rule():
    rng = np.random.default_rng(1)
    for m in (1, 2, 9, 17):
        Q = rng.standard_normal((3 * m + 2, m)) * np.geomspace(1e-4, 1e4, m)
        G = Q.T @ Q
        bad, Gi = spd_inverse(G)
        assert bad == 0
        d = 1.0 / np.sqrt(np.diag(G))
        assert np.max(np.abs(d[:, None] * (G @ Gi) / d[None, :] - np.eye(m))) <= 1e-10
        assert np.allclose(Gi, Gi.T, rtol=1e-14, atol=0.0)
    Q = rng.standard_normal((20, 4))
    Q[:, 3] = Q[:, 1]
    assert spd_inverse(Q.T @ Q)[0] == 1
    assert spd_inverse(np.diag([1.0, 0.0]))[0] == 1


def test_restatement_solves_a_singular_operator_under_the_constant_constraint():
    dims = (6, 5, 4)
    rp, ci, v = problems.poisson3d_neumann(*dims)
    n, k, tol = len(rp) - 1, 4, 1e-8
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    lu = spla.splu((A + 1e-3 * sp.identity(n)).tocsc())  # a definite stand-in for the cycle
    out = lobpcg_con(lambda X: A @ X, lambda R: lu.solve(R), np.random.default_rng(0).standard_normal((n, k)), np.ones((n, 1)), tol=tol,
                     max_iters=200)
    assert not out["rank_deficient"] and not out["breakdown"] and not out["status"].any()
    lam = sum(np.ix_(*[2.0 - 2.0 * np.cos(np.pi * np.arange(d) / d) for d in dims]))
    ref = np.sort(lam.ravel())[1:k + 1]
    assert np.all(np.abs(out["lam"] - ref) <= tol * ref), (out["lam"], ref)
    X = out["X"]
    assert np.max(np.abs(X.T @ X - np.eye(k))) <= 1e-12
    assert np.max(np.abs(np.ones(n) @ X)) <= 1e-10
    # the constant vector itself as the only constraint twice over is rank deficient
    assert lobpcg_con(lambda X: A @ X, lambda R: R, np.ones((n, 1)), np.ones((n, 2)))["rank_deficient"]


def test_restatement_continues_past_a_first_block_of_pairs():
    rp, ci, v = problems.poisson3d(6, 5, 4)
    n, tol = len(rp) - 1, 1e-9
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    Bd = 1.0 + (np.arange(n) % 7) / 3.0
    lu = spla.splu(A.tocsc())
    w, V = scipy.linalg.eigh(A.toarray(), np.diag(Bd))
    out = lobpcg_con(lambda X: A @ X, lambda R: lu.solve(R), np.random.default_rng(3).standard_normal((n, 3)), V[:, :4],
                     apply_B=lambda X: Bd[:, None] * X, tol=tol, max_iters=200)
    assert not out["breakdown"] and not out["status"].any()
    assert np.all(np.abs(out["lam"] - w[4:7]) <= 1e-7 * w[4:7]), (out["lam"], w[4:7])
    assert np.max(np.abs(V[:, :4].T @ (Bd[:, None] * out["X"]))) <= 1e-10
    Pi = Projector(V[:, :4], Bd[:, None] * V[:, :4])
    Z = Pi(np.random.default_rng(4).standard_normal((n, 3)))
    assert np.max(np.abs((Bd[:, None] * V[:, :4]).T @ Z)) <= 1e-12


# ---------------------------------------------------------------------------- the dumbbell graph

def test_dumbbell_laplacian_and_its_fiedler_vector():
    a, bridge = DUMBBELL
    rp, ci, v, deg = problems.dumbbell_laplacian(a, bridge)
    m, n = a ** 3, 2 * a ** 3 + bridge
    assert len(rp) == n + 1 and rp.dtype == np.int32 and ci.dtype == np.int32 and len(deg) == n
    L = sp.csr_matrix((v, ci, rp), shape=(n, n))
    assert all(np.all(np.diff(ci[rp[i]:rp[i + 1]]) > 0) for i in range(n))  # sorted columns
    assert abs(L - L.T).max() == 0.0
    assert np.all(L @ np.ones(n) == 0.0)
    assert np.array_equal(L.diagonal(), deg)
    off = L - sp.diags(L.diagonal())
    assert set(off.data.tolist()) == {-1.0}
    assert L.nnz == n + 2 * (2 * 3 * a * a * (a - 1) + bridge + 1)  # two cubes' grid edges and the chain's, both directions
    assert deg[m - 1] == 4 and deg[m + bridge] == 4 and np.all(deg[m:m + bridge] == 2)  # the corridor's ends: corners of the cubes
    w, V = np.linalg.eigh(L.toarray())
    assert abs(w[0]) <= 1e-12 and w[1] > 1e-3
    assert w[2] - w[1] > 0.1 * w[1]  # the second-smallest eigenvalue is simple
    f = V[:, 1]
    assert np.all(np.sign(f[:m]) == np.sign(f[0])) and np.all(np.sign(f[m + bridge:]) == -np.sign(f[0]))
    wn, Vn = scipy.linalg.eigh(L.toarray(), np.diag(deg))  # the normalised cut separates the cubes too
    g = Vn[:, 1]
    assert wn[2] - wn[1] > 0.1 * wn[1]
    assert np.all(np.sign(g[:m]) == np.sign(g[0])) and np.all(np.sign(g[m + bridge:]) == -np.sign(g[0]))
