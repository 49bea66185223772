"""The host side of the generalised eigenproblem A x = lambda B x: problems.fem_pencil, every argument and
state error of sparsh_eig_set_b / sparsh_eig_b_info / sparsh_eigs_gen / sparsh_eigs_gen_dev on handles without a device, and the numpy
restatement of the algorithm, preconditioned by the CPU oracle's V-cycle, against scipy.linalg.eigh(A, B).  CPU only."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from eig_gen_restatement import CAP, PENCILS, SOLVES, TOL, check_solution, dense_reference, diag_b, lobpcg_gen

QUIET = dict(print_setup=0, print_solve=0)
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


# ---------------------------------------------------------------------------- the FEM pencil

def test_fem_pencil_is_fem_unstructured_and_its_mass_matrix():
    for npts, kw in ((3000, {}), (500, dict(seed=7, dt=0.05, ordering="random"))):
        A, M = problems.fem_pencil(npts, **kw)
        ref = problems.fem_unstructured(npts, **kw)
        for a, r in zip(A, ref):
            assert a.dtype == r.dtype and np.array_equal(a, r)
        assert np.array_equal(M[0], A[0]) and np.array_equal(M[1], A[1])  # A's stored pattern
        assert M[0].dtype == np.int32 and M[1].dtype == np.int32 and M[2].dtype == np.float64
        Ms = sp.csr_matrix((M[2], M[1], M[0]), shape=(npts, npts))
        As = sp.csr_matrix((A[2], A[1], A[0]), shape=(npts, npts))
        assert abs(Ms - Ms.T).max() <= 1e-15 * abs(Ms).max()
        assert np.all(Ms.diagonal() > 0.0)
        # A - M = dt K and K annihilates the constant vector: every row of K sums to zero up to the rounding of its entries
        K = As - Ms
        assert np.max(np.abs(K @ np.ones(npts))) <= 1e-13 * abs(K).sum(axis=1).max()
        assert np.all(np.linalg.eigvalsh(Ms.toarray()[:200, :200]) > 0.0)


# ---------------------------------------------------------------------------- sparsh_eig_set_b without a device

def raw_set_b(A, rp, ci, v):
    return sa.lib.sparsh_eig_set_b(A._h, None if rp is None else rp.ctypes.data_as(IP), None if ci is None else ci.ctypes.data_as(IP),
                                   None if v is None else v.ctypes.data_as(DP))


def valid_b(n):
    """tridiagonal, SPD, n rows"""
    B = sp.diags([np.full(n - 1, 0.25), np.full(n, 1.0), np.full(n - 1, 0.25)], [-1, 0, 1], format="csr")
    B.sort_indices()
    return B.indptr.astype(np.int32), B.indices.astype(np.int32), B.data.astype(np.float64)


def defects(n):
    """(word of the message, rowptr, col, val): every SPARSH_EINVAL case of sparsh_eig_set_b"""
    rp, ci, v = valid_b(n)
    out = []

    def case(word, rp=rp, ci=ci, v=v):
        out.append((word, rp, ci, v))

    case(b"NULL", ci=None)
    case(b"NULL", v=None)
    r = rp.copy(); r[0] = 1
    case(b"rowptr[0]", rp=r)
    r = rp.copy(); r[5] = r[4] - 1
    case(b"non-decreasing", rp=r)
    c = ci.copy(); c[rp[3]] = -1
    case(b"out of range", ci=c)
    c = ci.copy(); c[rp[n] - 1] = n
    case(b"out of range", ci=c)
    c = ci.copy(); c[rp[3]], c[rp[3] + 1] = ci[rp[3] + 1], ci[rp[3]]
    case(b"ascending", ci=c)
    c = ci.copy(); c[rp[3] + 1] = c[rp[3]]  # a repeated column
    case(b"ascending", ci=c)
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy(); w[rp[2]] = bad
        case(b"finite", v=w)
    c = ci.copy(); c[rp[0]] = 1; c[rp[0] + 1] = 2  # row 0: columns (1, 2), no diagonal
    case(b"diagonal", ci=c)
    for bad in (0.0, -1.0):
        w = v.copy(); w[rp[4] + 1] = bad  # row 4: columns (3, 4, 5)
        assert ci[rp[4] + 1] == 4
        case(b"diagonal", v=w)
    w = v.copy(); w[rp[4]] = 0.25 + 1e-11  # b_43 alone: |b_43 - b_34| = 1e-11 > 1e-12 max|b|
    case(b"symmetric", v=w)
    # a missing transpose entry counts as 0: drop b_10 from a B that keeps b_01
    keep = np.ones(len(ci), dtype=bool); keep[rp[1]] = False
    r = rp.copy(); r[2:] -= 1
    case(b"symmetric", rp=r, ci=ci[keep].copy(), v=v[keep].copy())
    return out


@pytest.fixture(scope="module")
def problem():
    rp, ci, v = problems.poisson2d(12)
    return rp, ci, v, len(rp) - 1


@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_set_b_defects_are_einval_without_a_device(problem, prepared):
    rp, ci, v, n = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    for word, brp, bci, bv in defects(n):
        assert raw_set_b(A, brp, bci, bv) == sa.SPARSH_EINVAL, word
        assert word in sa.lib.sparsh_last_error(), (word, sa.lib.sparsh_last_error())
    assert sa.lib.sparsh_eig_set_b(None, None, None, None) == sa.SPARSH_EINVAL
    # an asymmetry at the bound itself passes the argument checks: the call order is what is wrong then
    brp, bci, bv = valid_b(n)
    w = bv.copy(); w[brp[4]] = 0.25 + 0.5e-12
    assert raw_set_b(A, brp, bci, w) == sa.SPARSH_ESTATE
    assert raw_set_b(A, brp, bci, bv) == sa.SPARSH_ESTATE
    assert raw_set_b(A, *diag_b(n)) == sa.SPARSH_ESTATE
    assert raw_set_b(A, None, None, None) == sa.SPARSH_OK  # dropping a B that is not there
    assert A.eig_b_info() == dict(is_set=False, nnz=0, bytes=0)
    assert sa.lib.sparsh_eig_b_info(None, None, None, None) == sa.SPARSH_EINVAL


def test_set_b_on_a_handle_the_block_path_refuses_is_einval(problem):
    rp, ci, v, n = problem
    B = valid_b(n)
    A = sa.sp_matrix_mg(rp, ci, v)
    A.set_smoother("sor", 0, "symmetric")
    assert raw_set_b(A, *B) == sa.SPARSH_EINVAL and b"Jacobi" in sa.lib.sparsh_last_error()
    A.set_smoother("jacobi")
    A.set_cycle("w")
    assert raw_set_b(A, *B) == sa.SPARSH_EINVAL and b"V-cycle" in sa.lib.sparsh_last_error()
    A.set_cycle("v")
    assert raw_set_b(A, *B) == sa.SPARSH_ESTATE
    F = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, precond_fp32=1), host_only=True)
    assert raw_set_b(F, *B) == sa.SPARSH_EINVAL and b"precond_fp32" in sa.lib.sparsh_last_error()
    rpn, cin, vn = problems.poisson3d_neumann(5)
    N = sa.sp_matrix_mg(rpn, cin, vn)
    N.set_nullspace("constant")
    N.setup(sa.default_params(**QUIET), host_only=True)
    assert raw_set_b(N, *valid_b(125)) == sa.SPARSH_EINVAL and b"null space" in sa.lib.sparsh_last_error()
    # a defect of B is named before the handle's
    assert raw_set_b(N, valid_b(125)[0], None, None) == sa.SPARSH_EINVAL and b"NULL" in sa.lib.sparsh_last_error()


def raw_eigs_gen(A, nev, X, ldx, tol=1e-8, hist_cap=4, dev=False):
    h = np.zeros((8, max(hist_cap, 1)))
    la, it, st = np.zeros(8), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    args = [A._h, nev, None if X is None else X.ctypes.data_as(C.c_void_p if dev else DP), ldx, tol, 0, la.ctypes.data_as(DP),
            h.ctypes.data_as(DP), hist_cap, it.ctypes.data_as(IP), st.ctypes.data_as(IP)]
    if dev:
        args.append(None)
    return (sa.lib.sparsh_eigs_gen_dev if dev else sa.lib.sparsh_eigs_gen)(*args)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_eigs_gen_arguments_and_state_without_a_device(problem, dev, prepared):
    rp, ci, v, n = problem
    X = np.ones((n, 8), order="F")
    A = sa.sp_matrix_mg(rp, ci, v)
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    for nev in (0, 9):
        assert raw_eigs_gen(A, nev, X, n, dev=dev) == sa.SPARSH_EINVAL and b"nev" in sa.lib.sparsh_last_error()
    assert raw_eigs_gen(A, 4, None, n, dev=dev) == sa.SPARSH_EINVAL and b"NULL" in sa.lib.sparsh_last_error()
    assert raw_eigs_gen(A, 4, X, n - 1, dev=dev) == sa.SPARSH_EINVAL and b"ldx" in sa.lib.sparsh_last_error()
    assert raw_eigs_gen(A, 4, X, n, tol=0.0, dev=dev) == sa.SPARSH_EINVAL and b"tol" in sa.lib.sparsh_last_error()
    assert raw_eigs_gen(A, 4, X, n, hist_cap=-1, dev=dev) == sa.SPARSH_EINVAL
    assert raw_eigs_gen(A, 4, X, n, dev=dev) == sa.SPARSH_ESTATE  # no B (and no setup)
    A.set_cycle("k")
    assert raw_eigs_gen(A, 4, X, n, dev=dev) == sa.SPARSH_EINVAL and b"V-cycle" in sa.lib.sparsh_last_error()


def test_python_wrappers_raise_the_same_codes(problem):
    rp, ci, v, n = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    for word, brp, bci, bv in defects(n):
        if bci is None or bv is None:
            continue
        with pytest.raises(sa.SparshError) as e:
            A.set_eig_b(brp, bci, bv)
        assert e.value.code == sa.SPARSH_EINVAL and word.decode() in str(e.value)
    with pytest.raises(sa.SparshError) as e:
        A.set_eig_b(valid_b(n)[0])
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(ValueError):
        A.set_eig_b(*valid_b(n + 1))
    with pytest.raises(sa.SparshError) as e:
        A.set_eig_b(*valid_b(n))
    assert e.value.code == sa.SPARSH_ESTATE
    assert A.set_eig_b(None) is A
    for call in (lambda: A.eigs_gen(4), lambda: A.op_eig_b_multi(np.ones((n, 2))),
                 lambda: A.op_eig_residual_gen(np.ones((5, 2)), np.ones((5, 2)), np.ones(2)),
                 lambda: A.op_eig_update_gen([np.ones((5, 2))] * 9, *[np.eye(2)] * 3),
                 lambda: A.bench_op_multi("eig_update_gen", 0, nrhs=4), lambda: A.bench_op_multi("eig_b_spmv", 0, nrhs=4)):
        with pytest.raises(sa.SparshError) as e:
            call()
        assert e.value.code == sa.SPARSH_ESTATE
    for k in (0, 9):
        with pytest.raises(sa.SparshError) as e:
            A.eigs_gen(k)
        assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.bench_op_multi(6, 0, nrhs=4)
    assert e.value.code == sa.SPARSH_EINVAL


# ---------------------------------------------------------------------------- the restatement with the oracle's V-cycle

@functools.lru_cache(maxsize=None)
def pencil(name):
    return PENCILS[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    return dense_reference(*pencil(name), 8)


@functools.lru_cache(maxsize=None)
def hierarchy(name):
    A, _ = pencil(name)
    return oracle.Hierarchy(oracle.Csr(*A), oracle.params(**PENCILS[name][1]))


# the whole solves of the GPU suite, and the rest of the one-level row of the issue's table
@pytest.mark.parametrize("name,k", SOLVES + [("fem_1l", 1), ("fem_1l", 4)])
def test_restatement_with_the_oracle_cycle_matches_dense_eigh(name, k):
    A, B = pencil(name)
    n = len(A[0]) - 1
    As, Bs = sp.csr_matrix((A[2], A[1], A[0]), shape=(n, n)), sp.csr_matrix((B[2], B[1], B[0]), shape=(n, n))
    H = hierarchy(name)

    def cycle(R):  # one V-cycle from a zero guess, a column at a time
        return np.column_stack([H.solve(np.ascontiguousarray(R[:, c]), iterations=1)[0] for c in range(R.shape[1])])

    X0 = np.random.default_rng(0).standard_normal((n, k))
    out = lobpcg_gen(lambda X: As @ X, lambda X: Bs @ X, cycle, X0, tol=TOL, max_iters=CAP)
    assert not out["breakdown"]
    nit = out["hist"].shape[1] - 1
    print(f"{name} k={k}: {H.nlevels} levels, {nit} iterations, restarts {out['restarts']}")
    assert not out["status"].any(), f"not converged in {CAP} iterations"
    if (name, k) in SOLVES:
        assert nit <= CAP // 2  # the condition under which the case stays in the GPU list
    check_solution(name, k, out["lam"], out["X"], A, B, reference(name))


def test_restatement_with_the_identity_is_the_standard_restatement():
    from eig_restatement import lobpcg
    rp, ci, v = problems.poisson3d(6)
    n = len(rp) - 1
    As = sp.csr_matrix((v, ci, rp), shape=(n, n))
    d = 1.0 / As.diagonal()
    X0 = np.random.default_rng(1).standard_normal((n, 4))
    std = lobpcg(lambda X: As @ X, lambda R: R * d[:, None], X0, tol=1e-6, max_iters=40)
    gen = lobpcg_gen(lambda X: As @ X, lambda X: X.copy(), lambda R: R * d[:, None], X0, tol=1e-6, max_iters=40)
    m = min(std["hist"].shape[1], gen["hist"].shape[1])
    assert abs(std["hist"].shape[1] - gen["hist"].shape[1]) <= 1  # the stopping rule multiplies by ||x_c||, 1 only to rounding
    assert np.array_equal(std["hist"][:, :m], gen["hist"][:, :m])
