"""Eigenpairs under constraints on the block path: the projection through its operator-level hook (exact on
integer data, bitwise the stated order on normal data, in place and out of place), whole solves on null-space handles against
analytic and dense eigenvalues (the standard problem and the normalised cut), the drift of the constraint against the numpy
restatement, pairs 9..15 by deflation, the Fiedler vector of a dumbbell graph, the zero-constraint path bit for bit against the old
solvers, rank-deficient constraints and the life cycle of the constraint memory.  GPU box only."""
import functools

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from eig_con_restatement import DUMBBELL, apply_projection, lobpcg_con
from eig_gen_restatement import pencil_fem

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
TOL = 1e-8
SIZES = (1, 2, 63, 64, 65, 255, 257, 1080, 70001)
PAST_A_GRID_STRIDE = 2048 * 256 * 2 + 3
KS, MS = (1, 2, 3, 5, 8), (1, 2, 8, 9, 17)
BOXES = {"small": (12, 10, 9), "large": (24, 20, 18)}


@functools.lru_cache(maxsize=None)
def lender():
    """a ready handle: the kernel hook borrows its stream only"""
    return sa.sp_matrix_mg(*problems.poisson3d(8)).setup(sa.default_params(**QUIET))


# ---------------------------------------------------------------------------- kernels

def exact_case(rng, n, k, m):
    """V of integers in [-8, 8]; Y of +-1 columns on disjoint supports of power-of-two sizes 2^p_j; BY = Y; Ginv = diag(2^-p_j): every
    sum is an integer below 2^53 and every coefficient a dyadic rational, so any order of summation gives the same bits"""
    p = max(int(np.log2(n // m)), 0)
    ps = [p - (j % 2 if p > 0 else 0) for j in range(m)]
    Y = np.zeros((n, m))
    rows = rng.permutation(n)
    at = 0
    for j, pj in enumerate(ps):
        Y[rows[at:at + 2 ** pj], j] = rng.choice([-1.0, 1.0], 2 ** pj)
        at += 2 ** pj
    return Y, np.diag(0.5 ** np.array(ps, dtype=np.float64)), rng.integers(-8, 9, (n, k)).astype(np.float64)


def check_exact(n, combos):
    A = lender()
    rng = np.random.default_rng(n)
    for k, m in combos:
        if n < m:
            continue
        Y, Ginv, V = exact_case(rng, n, k, m)
        Vout, Cm = A.op_eig_con_project(Y, Y, Ginv, V)
        assert np.array_equal(Cm, Y.T @ V), (n, k, m)
        assert np.array_equal(Vout, V - Y @ (Ginv @ (Y.T @ V))), (n, k, m)
        Vin, _ = A.op_eig_con_project(Y, Y, Ginv, V, in_place=True)
        assert np.array_equal(Vin, Vout), (n, k, m, "in place")


def check_normal(n, combos):
    A = lender()
    rng = np.random.default_rng(1000 + n)
    for k, m in combos:
        Y, BY, V = rng.standard_normal((n, m)), rng.standard_normal((n, m)), rng.standard_normal((n, k))
        Ginv = rng.standard_normal((m, m))
        Vout, Cm = A.op_eig_con_project(Y, BY, Ginv, V)
        assert np.all(np.abs(Cm - BY.T @ V) <= 1e-12 * (np.abs(BY).T @ np.abs(V))), (n, k, m)  # the Gram launch's bound
        assert np.array_equal(Vout, apply_projection(Y, Ginv, Cm, V)), (n, k, m)  # the stated order, given the device's own C
        Vin, Cin = A.op_eig_con_project(Y, BY, Ginv, V, in_place=True)
        assert np.array_equal(Vin, Vout) and np.array_equal(Cin, Cm), (n, k, m, "in place")
        V2, C2 = A.op_eig_con_project(Y, BY, Ginv, V)
        assert np.array_equal(V2, Vout) and np.array_equal(C2, Cm), (n, k, m, "run to run")


@pytest.mark.parametrize("n", SIZES)
def test_projection_is_exact_on_integer_data(n):
    check_exact(n, [(k, m) for k in KS for m in MS])


@pytest.mark.parametrize("n", SIZES)
def test_projection_is_bitwise_the_stated_order(n):
    check_normal(n, [(k, m) for k in KS for m in MS])


@pytest.mark.parametrize("k,m", [(1, 2), (3, 9), (8, 17)])
def test_projection_past_a_full_grid_stride(k, m):
    check_exact(PAST_A_GRID_STRIDE, [(k, m)])
    check_normal(PAST_A_GRID_STRIDE, [(k, m)])


def test_padding_columns_come_back_untouched():
    """k = 3 in a block of width 4, m = 5 in two blocks of width 4.  A lane stores both columns of its pair, so the padding column of
    the block cannot carry a sentinel through the launch: the hook reads the whole device block back and returns SPARSH_ENUMERIC
    unless every padding entry is still zero, out of place and in place."""
    A = lender()
    rng = np.random.default_rng(7)
    for n in (5, 257, 1080):
        Y, V = np.linalg.qr(rng.standard_normal((n, 5)))[0], rng.standard_normal((n, 3))
        Ginv = np.linalg.inv(Y.T @ Y)
        for in_place in (False, True):
            Vout, Cm = A.op_eig_con_project(Y, Y, Ginv, V, in_place=in_place)
            assert Vout.shape == (n, 3) and Cm.shape == (5, 3)
            assert np.max(np.abs(Y.T @ Vout)) <= 1e-12 * np.max(np.abs(Y).T @ np.abs(V))


# ---------------------------------------------------------------------------- handles and references

@functools.lru_cache(maxsize=None)
def neumann_csr(box):
    return problems.poisson3d_neumann(*BOXES[box])


@functools.lru_cache(maxsize=None)
def neumann(box):
    """the singular handle; on the small box with B = diag(degrees) set for the normalised cut"""
    rp, ci, v = neumann_csr(box)
    A = sa.sp_matrix_mg(rp, ci, v)
    A.set_nullspace("constant")
    A.setup(sa.default_params(**QUIET, limit_upper=300, limit_lower=100))
    if box == "small":
        n = A.nrow
        A.set_eig_b(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), degrees(box), con=True)
    return A


@functools.lru_cache(maxsize=None)
def neumann_matrix(box):
    rp, ci, v = neumann_csr(box)
    return sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, len(rp) - 1))


def degrees(box):
    return neumann_matrix(box).diagonal().copy()


def analytic_neumann(box, k):
    lam = sum(np.ix_(*[2.0 - 2.0 * np.cos(np.pi * np.arange(d) / d) for d in BOXES[box]]))
    return np.sort(lam.ravel())[1:k + 1]  # the zero dropped


@functools.lru_cache(maxsize=None)
def ncut_reference():
    L = neumann_matrix("small")
    return scipy.linalg.eigh(L.toarray(), np.diag(degrees("small")), eigvals_only=True, subset_by_index=[1, 8])


@functools.lru_cache(maxsize=None)
def solved(box, k, gen):
    return neumann(box).eigs_con(k, gen=gen, tol=TOL)


# ---------------------------------------------------------------------------- singular problems

@pytest.mark.parametrize("k", (1, 4, 8))
@pytest.mark.parametrize("box", ("small", "large"))
def test_singular_standard_problem(box, k):
    lam, X, iters, hist, status = solved(box, k, False)
    M = neumann_matrix(box)
    ref = analytic_neumann(box, k)
    res = np.linalg.norm(M @ X - X * lam, axis=0)
    orth = np.max(np.abs(X.T @ X - np.eye(k)))
    print(f"{box} k={k}: {hist.shape[1] - 1} iterations, max |lam - ref| / (tol ref) {np.max(np.abs(lam - ref) / (TOL * ref)):.3f}, "
          f"max residual / (tol lam) {np.max(res / (TOL * lam)):.3f}, orthonormality {orth:.2e}, max |1^T x| {np.max(np.abs(X.sum(axis=0))):.2e}")
    assert np.all(status == sa.SPARSH_OK)
    assert np.all(np.diff(lam) >= 0)
    assert np.all(np.abs(lam - ref) <= TOL * ref), (lam, ref)
    assert np.all(res <= TOL * lam + 1e-12 * abs(M).sum(axis=1).max() * np.linalg.norm(X, axis=0))
    assert orth <= 1e-12


@pytest.mark.parametrize("k", (1, 4, 8))
def test_normalised_cut(k):
    lam, X, iters, hist, status = solved("small", k, True)
    L, D = neumann_matrix("small"), degrees("small")
    ref = ncut_reference()[:k]
    rn = np.linalg.norm(L @ X - (D[:, None] * X) * lam, axis=0)
    orth = np.max(np.abs(X.T @ (D[:, None] * X) - np.eye(k)))
    bound = rn / np.sqrt(D.min())  # the residual bound of a B-normalised vector: |lam - ref| <= ||B^-1/2 r|| <= ||r|| / sqrt(min b)
    print(f"ncut k={k}: {hist.shape[1] - 1} iterations, max |lam - ref| / bound {np.max(np.abs(lam - ref) / bound):.3e}, D-orthonormality {orth:.2e}")
    assert np.all(status == sa.SPARSH_OK)
    assert np.all(np.abs(lam - ref) <= bound), (lam, ref, bound)
    assert orth <= 1e-12


@functools.lru_cache(maxsize=None)
def restated(box, gen):
    """the numpy restatement on the start block of eigs_con(8).  The block V-cycle hook refuses a null-space handle, so the
    preconditioner here is a sparse LU of the shifted operator; the drift compared below is rounding noise of the projection and
    the update, which both sides do alike"""
    M = neumann_matrix(box)
    n = M.shape[0]
    D = degrees(box)
    lu = spla.splu((M + 1e-2 * sp.identity(n)).tocsc())
    X0 = np.random.default_rng(0).standard_normal((n, 8))
    return lobpcg_con(lambda X: M @ X, lambda R: lu.solve(R), X0, np.ones((n, 1)), apply_B=(lambda X: D[:, None] * X) if gen else None,
                      tol=TOL, max_iters=300)


@pytest.mark.parametrize("box,gen", [("small", False), ("large", False), ("small", True)])
def test_constraint_drift_is_rounding_noise(box, gen):
    lam, X, *_ = solved(box, 8, gen)
    ref = restated(box, gen)
    assert not ref["breakdown"] and not ref["rank_deficient"]
    n = X.shape[0]
    u = degrees(box) if gen else np.ones(n)
    v = np.abs(u @ X)
    v_ref = np.abs(u @ ref["X"])
    floor = n * 2.0 ** -53 * np.mean(np.abs(u[:, None] * X), axis=0)
    print(f"{box} gen={gen}: drift {v.max():.3e}, restatement {v_ref.max():.3e}, floor {floor.max():.3e}, "
          f"worst device / max(restatement, floor) {np.max(v / np.maximum(v_ref, floor)):.3f}")
    assert np.all(v <= 10.0 * np.maximum(v_ref, floor)), (v, v_ref, floor)


# ---------------------------------------------------------------------------- more than 8 pairs

def test_pairs_nine_to_fifteen_by_deflation():
    A = sa.sp_matrix_mg(*problems.poisson3d(12, 10, 9)).setup(sa.default_params(**QUIET))
    lam1, X1, *_ = A.eigs(8, tol=TOL)
    lam2, X2, iters, hist, status = A.eigs_con(7, Y=X1, tol=TOL)
    lam = sum(np.ix_(*[2.0 - 2.0 * np.cos(np.pi * np.arange(1, d + 1) / (d + 1)) for d in (12, 10, 9)]))
    ref = np.sort(lam.ravel())[8:15]
    # TOL ref: the stopping rule; 8 TOL lam1.max(): the first-order effect of deflating against eight vectors converged only to TOL
    bound = TOL * ref + 8 * TOL * lam1.max()
    print(f"pairs 9..15: {hist.shape[1] - 1} iterations, max |lam - ref| / bound {np.max(np.abs(lam2 - ref) / bound):.3e}, "
          f"max |X1^T X2| {np.max(np.abs(X1.T @ X2)):.2e}")
    assert np.all(status == sa.SPARSH_OK)
    assert np.all(np.abs(lam2 - ref) <= bound), (lam2, ref)
    assert np.max(np.abs(X1.T @ X2)) <= 1e-7
    assert np.max(np.abs(X2.T @ X2 - np.eye(7))) <= 1e-12
    assert A.eig_con_info() == dict(ncon_total=8, implicit_constant=0, bytes=8 * (8 * A.nrow + 64 + 64 + 64))
    A.close()


def test_pencil_pairs_five_to_eight_by_deflation():
    """the dense pencil's value 9 lies 18 % above value 8 (1.6302, 1.9213), so four pairs end on a gap"""
    (rpa, cia, va), (rpb, cib, vb) = pencil_fem()
    n = len(rpa) - 1
    A = sa.sp_matrix_mg(rpa, cia, va).setup(sa.default_params(**QUIET, limit_upper=400, limit_lower=200))
    A.set_eig_b(rpb, cib, vb)
    K, Mb = sp.csr_matrix((va, cia, rpa), shape=(n, n)), sp.csr_matrix((vb, cib, rpb), shape=(n, n))
    w = scipy.linalg.eigh(K.toarray(), Mb.toarray(), eigvals_only=True, subset_by_index=[0, 8])
    assert w[8] - w[7] > 0.01 * w[7]
    lam1, X1, *_ = A.eigs_gen(4, tol=TOL, max_iters=300)
    lam2, X2, iters, hist, status = A.eigs_con(4, Y=X1, gen=True, tol=TOL, max_iters=300)
    bound = TOL * w[4:8] + 8 * TOL * lam1.max()  # the bound of test_pairs_nine_to_fifteen_by_deflation, as it stands there
    cross = np.max(np.abs(X1.T @ (Mb @ X2)))
    print(f"pencil pairs 5..8: {hist.shape[1] - 1} iterations, max |lam - ref| / bound {np.max(np.abs(lam2 - w[4:8]) / bound):.3e}, "
          f"max |X1^T B X2| {cross:.2e}")
    assert np.all(status == sa.SPARSH_OK)
    assert np.all(np.abs(lam2 - w[4:8]) <= bound), (lam2, w[4:8])
    assert cross <= 1e-7
    assert np.max(np.abs(X2.T @ (Mb @ X2) - np.eye(4))) <= 1e-12
    A.close()


# ---------------------------------------------------------------------------- the Fiedler vector

def test_fiedler_vector_separates_the_dumbbell():
    a, bridge = DUMBBELL
    rp, ci, v, deg = problems.dumbbell_laplacian(a, bridge)
    m, n = a ** 3, len(rp) - 1
    L = sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray()
    A = sa.sp_matrix_mg(rp, ci, v)
    A.set_nullspace("constant")
    A.setup(sa.default_params(**QUIET))
    lam, X, iters, hist, status = A.eigs_con(1, tol=TOL)
    ref = np.linalg.eigvalsh(L)[1]
    assert status[0] == sa.SPARSH_OK
    assert abs(lam[0] - ref) <= TOL * ref, (lam, ref)
    f = X[:, 0]
    assert np.all(np.sign(f[:m]) == np.sign(f[0])) and np.all(np.sign(f[m + bridge:]) == -np.sign(f[0]))
    A.set_eig_b(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), deg, con=True)
    lamn, Xn, _, _, statusn = A.eigs_con(1, gen=True, tol=TOL)
    refn = scipy.linalg.eigh(L, np.diag(deg), eigvals_only=True, subset_by_index=[1, 1])[0]
    g = Xn[:, 0]
    rn = np.linalg.norm(L @ g - lamn[0] * deg * g)
    assert statusn[0] == sa.SPARSH_OK and abs(lamn[0] - refn) <= rn / np.sqrt(deg.min())
    assert np.all(np.sign(g[:m]) == np.sign(g[0])) and np.all(np.sign(g[m + bridge:]) == -np.sign(g[0]))
    A.close()


# ---------------------------------------------------------------------------- no constraints = the old solver

def documented_eig_bytes(n, W, gen):  # include/sparsh_amg.h; test_gpu_eig.py::test_memory_life_cycle
    return 8 * ((10 if gen else 7) * n * W + (12 * W * W + W) * 512 + 18 * W * W + W + 3 * W * W + W)


def test_no_constraints_is_eigs_bit_for_bit():
    A = sa.sp_matrix_mg(*problems.poisson3d(12, 10, 9)).setup(sa.default_params(**QUIET))
    want = A.eigs(4, tol=TOL)
    got = A.eigs_con(4, tol=TOL)
    for w, g in zip(want, got):
        assert np.array_equal(w, g)
    assert A.eig_con_info() == dict(ncon_total=0, implicit_constant=0, bytes=0)
    assert A.eig_info()["bytes"] == documented_eig_bytes(A.nrow, 4, False)
    A.eigs_con(4, Y=np.random.default_rng(1).standard_normal((A.nrow, 3)), tol=TOL, max_iters=2)  # a constrained call in between
    again = A.eigs(4, tol=TOL)
    for w, g in zip(want, again):
        assert np.array_equal(w, g)
    assert A.eig_info()["bytes"] == documented_eig_bytes(A.nrow, 4, False)
    A.close()


def test_no_constraints_is_eigs_gen_bit_for_bit():
    (rpa, cia, va), (rpb, cib, vb) = pencil_fem()
    A = sa.sp_matrix_mg(rpa, cia, va).setup(sa.default_params(**QUIET, limit_upper=400, limit_lower=200))
    A.set_eig_b(rpb, cib, vb)
    want = A.eigs_gen(4, tol=TOL, max_iters=300)
    got = A.eigs_con(4, gen=True, tol=TOL, max_iters=300)
    for w, g in zip(want, got):
        assert np.array_equal(w, g)
    assert A.eig_con_info()["bytes"] == 0
    assert A.eig_info()["bytes"] == documented_eig_bytes(A.nrow, 4, True)
    A.eigs_con(4, Y=np.random.default_rng(1).standard_normal((A.nrow, 3)), gen=True, tol=TOL, max_iters=2)  # a constrained call in between
    assert A.eig_con_info()["ncon_total"] == 3 and A.eig_con_info()["bytes"] > 0
    again = A.eigs_gen(4, tol=TOL, max_iters=300)
    for w, g in zip(want, again):
        assert np.array_equal(w, g)
    assert A.eig_info()["bytes"] == documented_eig_bytes(A.nrow, 4, True)
    A.close()


def test_generalised_call_without_a_b_is_estate():
    """on a ready handle: the check of the entry points themselves, host and device form (without a device the missing setup answers
    first)"""
    A = sa.sp_matrix_mg(*problems.poisson3d(8)).setup(sa.default_params(**QUIET))
    with pytest.raises(sa.SparshError) as e:
        A.eigs_con(1, gen=True)
    assert e.value.code == sa.SPARSH_ESTATE and "sparsh_eig_set_b" in str(e.value)
    n = A.nrow
    xd = A.dev_alloc(8 * n)
    A.h2d(xd, np.ones(n))
    with pytest.raises(sa.SparshError) as e:
        A.eigs_con_dev(1, xd, n, gen=True)
    assert e.value.code == sa.SPARSH_ESTATE and "sparsh_eig_set_b" in str(e.value)
    lam, iters, hist, status, sec, rc = A.eigs_con_dev(1, xd, n)  # the standard problem runs on the same handle
    assert rc == sa.SPARSH_OK and abs(lam[0] - (6.0 - 6.0 * np.cos(np.pi / 9))) <= TOL * lam[0]
    A.dev_free(xd)
    A.close()


# ---------------------------------------------------------------------------- rank-deficient constraints, memory

def test_rank_deficient_constraints_are_enumeric():
    A = sa.sp_matrix_mg(*problems.poisson3d(12, 10, 9)).setup(sa.default_params(**QUIET))
    lam1, X1, *_ = A.eigs(2, tol=TOL)
    with pytest.raises(sa.SparshError) as e:
        A.eigs_con(2, Y=np.hstack([X1, X1[:, :1]]))  # a repeated column
    assert e.value.code == sa.SPARSH_ENUMERIC and "rank deficient" in str(e.value)
    assert A.eig_con_info() == dict(ncon_total=0, implicit_constant=0, bytes=0)  # unusable constraints are not left in force
    # the handle solves afterwards: pairs 3 and 4 (0.4735 and 0.5210; the next value is 0.6445) by deflation against the two vectors.
    # (Constraints that span no invariant subspace would not do here: A x - lam x is then a combination of them at the solution and
    # the stopping rule, which looks at the unprojected residual, is never met.)
    lam, X, _, _, status = A.eigs_con(2, Y=X1, tol=TOL)
    grid = sum(np.ix_(*[2.0 - 2.0 * np.cos(np.pi * np.arange(1, d + 1) / (d + 1)) for d in (12, 10, 9)]))
    ref = np.sort(grid.ravel())[2:4]
    assert np.all(status == sa.SPARSH_OK) and A.last_eigs_rc == sa.SPARSH_OK
    assert np.all(np.abs(lam - ref) <= TOL * ref + 8 * TOL * lam1.max()), (lam, ref)
    A.close()
    N = neumann("large")
    with pytest.raises(sa.SparshError) as e:
        N.eigs_con(2, Y=np.ones((N.nrow, 1)))  # the constant vector is already a constraint of this handle
    assert e.value.code == sa.SPARSH_ENUMERIC and "rank deficient" in str(e.value)
    lam, *_ = N.eigs_con(2, tol=TOL)
    ref = analytic_neumann("large", 2)
    assert np.all(np.abs(lam - ref) <= TOL * ref)


def test_constraint_memory_life_cycle():
    rp, ci, v = problems.poisson3d_neumann(8)
    A = sa.sp_matrix_mg(rp, ci, v)
    A.set_nullspace("constant")
    A.setup(sa.default_params(**QUIET))
    n = A.nrow
    assert A.eig_con_info() == dict(ncon_total=0, implicit_constant=0, bytes=0)

    def documented(W, mt, gen):  # include/sparsh_amg.h: the blocks of Y (and of BY), G in padded order, its inverse, C
        nblk = -(-mt // W)
        return 8 * ((2 if gen else 1) * nblk * n * W + (nblk * W) ** 2 + mt * mt + nblk * W * W)

    A.eigs_con(3, tol=TOL, max_iters=2)
    assert A.eig_con_info() == dict(ncon_total=1, implicit_constant=1, bytes=documented(4, 1, False))
    assert A.eig_info()["bytes"] == documented_eig_bytes(n, 4, False)  # the constraint blocks are not counted there
    Y = np.random.default_rng(3).standard_normal((n, 5))
    A.eigs_con(3, Y=Y, tol=TOL, max_iters=2)  # another count: replaced
    assert A.eig_con_info() == dict(ncon_total=6, implicit_constant=1, bytes=documented(4, 6, False))
    A.eigs_con(8, Y=Y, tol=TOL, max_iters=2)  # another width: replaced with the solver's blocks
    assert A.eig_con_info() == dict(ncon_total=6, implicit_constant=1, bytes=documented(8, 6, False))
    t = A.bench_op_multi("eig_con_project", 0, nrhs=8, reps=3)
    assert t > 0.0
    with pytest.raises(sa.SparshError) as e:
        A.bench_op_multi("eig_con_project", 0, nrhs=4, reps=3)  # no constrained solve of that width is resident
    assert e.value.code == sa.SPARSH_ESTATE
    A.setup(sa.default_params(**QUIET))
    assert A.eig_con_info() == dict(ncon_total=0, implicit_constant=0, bytes=0)
    A.close()
