"""Block BiCGStab without a device: the argument and state errors of SPARSH_MBICG through the block entry
points, its refusal by the single-vector entry points, the refusals of the handles a block solve cannot run on, mbicg_info() before
a solve, the generator of the unsymmetric test operator, and the numpy restatement of the kernels and of the loop anchored on the
restatement of the single-vector loop.  CPU only."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
import krylov_ops_restatement as kr
import mbicg_restatement as mr
from test_multi_rhs_host import raw_solve_multi

QUIET = dict(print_setup=0, print_solve=0)
TOL = 1e-8


@pytest.fixture(scope="module")
def problem():
    rp, ci, v = problems.convection_diffusion(40, 37)
    n = len(rp) - 1
    return rp, ci, v, n, np.ones((n, 8), order="F"), np.zeros((n, 8), order="F")


def test_the_method_constant():
    assert sa.SPARSH_MBICG == 10 and sa.UNSYMMETRIC_BLOCK_METHODS == {"mbicg": 10}
    assert "mbicg" not in sa.METHODS and "mbicg" not in sa.FLEXIBLE_METHODS  # a method of solve_multi only
    assert sa._method("mbicg") == 10
    assert len(sa.MBICG_SLOTS) == sa.SPARSH_MBICG_SCALARS == len(mr.SLOTS) and sa.MBICG_SLOTS == mr.SLOTS
    assert [sa.multi_width(k) for k in range(1, 9)] == [mr.width(k) for k in range(1, 9)] == [2, 2, 4, 4, 8, 8, 8, 8]


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_mbicg_arguments_and_state_without_a_device(problem, dev, prepared):
    rp, ci, v, n, B, X = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    m = sa.SPARSH_MBICG
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
    # the single-vector BiCGStab and every number that is no block method stay refused, and the message names all three block methods
    for method in (sa.SPARSH_AMG, sa.SPARSH_CG, sa.SPARSH_BICG, sa.SPARSH_PBICG, sa.SPARSH_GMRES, sa.SPARSH_PGMRES, sa.SPARSH_FCG, 9, 11, 17, -1):
        assert raw_solve_multi(A, method, 4, B, n, X, n, dev=dev) == sa.SPARSH_EINVAL, method
        msg = sa.lib.sparsh_last_error()
        assert b"SPARSH_PCG" in msg and b"SPARSH_BCG" in msg and b"SPARSH_MBICG" in msg
    # valid arguments: the call order is what is wrong
    for nrhs in (1, 4, 8):
        assert raw_solve_multi(A, m, nrhs, B, n, X, n, dev=dev) == sa.SPARSH_ESTATE, nrhs


@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_single_vector_entry_points_refuse_the_method(problem, prepared):
    rp, ci, v, n, B, X = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    b, x, hist, it = np.ones(n), np.zeros(n), np.zeros(4), np.zeros(1, dtype=np.int32)
    m = sa.SPARSH_MBICG
    assert sa.lib.sparsh_solve(A._h, m, sa._dp(b), sa._dp(x), sa._dp(hist), 4, sa._ip(it)) == sa.SPARSH_EINVAL
    assert b"SPARSH_MBICG" in sa.lib.sparsh_last_error()
    assert sa.lib.sparsh_solve_dev(A._h, m, None, None, 0, sa._dp(hist), 4, sa._ip(it), None) == sa.SPARSH_EINVAL
    assert b"SPARSH_MBICG" in sa.lib.sparsh_last_error()
    assert sa.lib.sparsh_krylov_init_dev(A._h, m, None, None) == sa.SPARSH_EINVAL
    assert b"SPARSH_MBICG" in sa.lib.sparsh_last_error()
    with pytest.raises((sa.SparshError, KeyError)):
        A.solve("mbicg", b, x)
    # the methods those calls know come as far as the readiness check, as before
    assert sa.lib.sparsh_solve(A._h, sa.SPARSH_PBICG, sa._dp(b), sa._dp(x), sa._dp(hist), 4, sa._ip(it)) == sa.SPARSH_ESTATE


def test_mbicg_is_refused_where_block_pcg_is(problem):
    rp, ci, v, n, B, X = problem
    m = sa.SPARSH_MBICG
    A = sa.sp_matrix_mg(rp, ci, v)
    for kind, order in (("sor", "symmetric"), ("sor", "forward"), ("chebyshev", "forward")):
        A.set_smoother(kind, 0, order)
        assert raw_solve_multi(A, m, 4, B, n, X, n) == sa.SPARSH_EINVAL, kind
        assert b"Jacobi" in sa.lib.sparsh_last_error()
    A.set_smoother("jacobi")
    assert raw_solve_multi(A, m, 4, B, n, X, n) == sa.SPARSH_ESTATE
    for cycle in ("w", "k"):
        A.set_cycle(cycle)
        assert raw_solve_multi(A, m, 4, B, n, X, n) == sa.SPARSH_EINVAL, cycle
        assert b"V-cycle" in sa.lib.sparsh_last_error()
    A.set_cycle("v")
    assert raw_solve_multi(A, m, 4, B, n, X, n) == sa.SPARSH_ESTATE
    F = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, precond_fp32=1), host_only=True)
    assert raw_solve_multi(F, m, 4, B, n, X, n) == sa.SPARSH_EINVAL
    assert b"precond_fp32" in sa.lib.sparsh_last_error()
    N = sa.sp_matrix_mg(*problems.poisson3d_neumann(6, 5, 4)).set_nullspace("constant")
    N.setup(sa.default_params(**QUIET), host_only=True)
    nn = N.nrow
    assert raw_solve_multi(N, m, 2, np.ones((nn, 2), order="F"), nn, np.zeros((nn, 2), order="F"), nn) == sa.SPARSH_EINVAL
    assert b"null space" in sa.lib.sparsh_last_error()
    group = sa.comm_group_create(2)
    try:
        P = sa.sp_matrix_mg(rp, ci, v)
        P.comm_init_group(group, 0)
        assert raw_solve_multi(P, m, 4, B, n, X, n) == sa.SPARSH_EINVAL
        assert b"partitioned" in sa.lib.sparsh_last_error()
        P.close()
    finally:
        sa.comm_group_destroy(group)
    with pytest.raises(sa.SparshError) as e:
        sa.sp_matrix_mg(rp, ci, v).solve_multi("mbicg", B[:, :4], X[:, :4].copy())
    assert e.value.code == sa.SPARSH_ESTATE


def test_mbicg_info_is_zero_before_a_solve(problem):
    rp, ci, v, n, _, _ = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    assert A.mbicg_info() == dict(iterations=0, bytes=0)
    A.setup(sa.default_params(**QUIET), host_only=True)
    assert A.mbicg_info() == dict(iterations=0, bytes=0)
    assert sa.lib.sparsh_mbicg_info(None, None, None) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_mbicg_info(A._h, None, None) == sa.SPARSH_OK


def test_hooks_refuse_bad_arguments_without_a_device(problem):
    rp, ci, v, n, _, _ = problem
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET), host_only=True)
    V = np.ones((5, 3))
    with pytest.raises(sa.SparshError) as e:
        A.op_dot2_multi(V, V, V, V)
    assert e.value.code == sa.SPARSH_ESTATE  # valid arguments, no device-side setup
    with pytest.raises(sa.SparshError) as e:
        A.op_dot2_multi(np.ones((5, 9)), V, V, V)
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.op_bicg_p_multi(1.0, 1.0, V, V, np.ones((0, 3)))
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.op_mbicg_finalize(7, 3, np.ones((3, 4)), None, mr.new_state(3), TOL)
    assert e.value.code == sa.SPARSH_EINVAL


def test_convection_diffusion_is_the_upwind_operator_of_the_bicgstab_test():
    n = 12
    I = sp.identity(n)
    T = sp.diags([-1.0 * np.ones(n - 1), 2.0 * np.ones(n), -1.0 * np.ones(n - 1)], [-1, 0, 1])
    Cx = sp.diags([-1.0 * np.ones(n - 1), 1.0 * np.ones(n)], [-1, 0])
    M = (sp.kron(I, T) + sp.kron(T, I) + 0.8 * sp.kron(I, Cx) + 0.3 * sp.kron(Cx, I)).tocsr()
    M.sort_indices()
    rp, ci, v = problems.convection_diffusion(n, n)
    assert rp.dtype == np.int32 and ci.dtype == np.int32 and v.dtype == np.float64
    assert np.array_equal(rp, M.indptr) and np.array_equal(ci, M.indices) and np.array_equal(v, M.data)
    # 3D, unequal sides, a third velocity: kron with x fastest, sorted columns
    nx, ny, nz, c = 5, 4, 3, (0.8, 0.3, 0.5)

    def lap(m):
        return sp.diags([-1.0 * np.ones(m - 1), 2.0 * np.ones(m), -1.0 * np.ones(m - 1)], [-1, 0, 1])

    def up(m):
        return sp.diags([-1.0 * np.ones(m - 1), 1.0 * np.ones(m)], [-1, 0])

    Ix, Iy, Iz = sp.identity(nx), sp.identity(ny), sp.identity(nz)
    M3 = (sp.kron(Iz, sp.kron(Iy, lap(nx) + c[0] * up(nx))) + sp.kron(Iz, sp.kron(lap(ny) + c[1] * up(ny), Ix))
          + sp.kron(sp.kron(lap(nz) + c[2] * up(nz), Iy), Ix)).tocsr()
    M3.sort_indices()
    rp, ci, v = problems.convection_diffusion(nx, ny, nz, *c)
    assert np.array_equal(rp, M3.indptr) and np.array_equal(ci, M3.indices)
    assert np.abs(v - M3.data).max() <= 4 * np.finfo(float).eps * np.abs(v).max()  # (the diagonal's four terms are added in another order)
    assert np.all(np.diff(ci)[np.diff(np.repeat(np.arange(len(rp) - 1), np.diff(rp))) == 0] > 0)
    G = sp.csr_matrix((v, ci, rp))
    assert abs(G - G.T).max() > 0.1


# ---------------------------------------------------------------------------- the restatement, anchored on the single-vector one

@pytest.fixture(scope="module")
def cd2():
    rp, ci, v = problems.convection_diffusion(12, 11)
    A = sp.csr_matrix((v, ci, rp))
    return A, spla.splu(A.tocsc())


@pytest.mark.parametrize("precond", ["identity", "lu"])
def test_one_column_of_the_restated_loop_is_the_single_vector_loop(cd2, precond):
    """The two restatements apply the same expressions and differ in the order their reductions add n = 132 terms.  A sum of n terms
    is within n eps of any other order relative to sum |terms|; with the identity the recurrences carry that over some 30
    iterations of a system of condition ~1e2: 1e-6 on the entries well above tol is far above that and far below the O(1) change
    an error in an expression makes (the bound test_one_column_follows_textbook_pcg applies to block CG)."""
    A, lu = cd2
    n = A.shape[0]
    b = np.random.default_rng(3).standard_normal(n)
    M1 = None if precond == "identity" else (lambda r: lu.solve(r))
    Mk = None if precond == "identity" else (lambda R: np.column_stack([lu.solve(R[:, c]) for c in range(R.shape[1])]))
    x, h = kr.bicg_loop(lambda u: A @ u, M1, b, np.zeros(n), TOL, cap=400)
    X, hs, its, st = mr.mbicg_loop(lambda U: A @ U, Mk, b[:, None], np.zeros((n, 1)), TOL, 400)
    print(precond, "iterations", len(h), its)
    assert st[0] == 0 and abs(int(its[0]) - len(h)) <= 1
    if precond == "lu":
        # an exact preconditioner: alpha = 1 and the half step leaves rounding noise, one iteration in both; the history entry is that
        # noise, so only its size is comparable
        assert len(h) == 1 and its[0] == 1 and h[0] <= TOL and hs[0][0] <= TOL
    else:
        m = min(len(h), its[0])
        big = h[:m] > 100 * TOL
        assert big.sum() >= 10
        rel = np.abs(hs[0][:m] - h[:m])[big] / h[:m][big]
        print(precond, "largest relative history difference", rel.max())
        assert rel.max() <= 1e-6
    assert np.linalg.norm(b - A @ X[:, 0]) <= 10 * TOL and np.linalg.norm(X[:, 0] - x) <= 1e-6 * np.linalg.norm(x)


def test_columns_of_the_restated_loop_do_not_interact_and_freeze(cd2):
    A, lu = cd2
    n = A.shape[0]
    rng = np.random.default_rng(4)
    B = np.column_stack([np.ones(n), rng.standard_normal(n), 1e-3 * rng.standard_normal(n), np.zeros(n), rng.standard_normal(n)])
    B[5, 4] = np.nan
    X, hs, its, st = mr.mbicg_loop(lambda U: A @ U, None, B, np.zeros((n, 5)), TOL, 400)
    assert list(st) == [0, 0, 0, 0, mr.STATUS_NUMERIC] and its[3] == 0 and its[4] == 0
    assert np.array_equal(X[:, 3], np.zeros(n)) and np.array_equal(X[:, 4], np.zeros(n))
    assert len(set(its[:3])) > 1
    for c in range(3):
        assert hs[c][-1] <= TOL and np.all(hs[c][:-1] > TOL)
        # alone at the same width the column takes the same steps bit for bit
        Xc, hc, ic, sc = mr.mbicg_loop(lambda U: A @ U, None, B[:, c:c + 1], np.zeros((n, 1)), TOL, 400, W=8)
        assert np.array_equal(Xc[:, 0], X[:, c]) and np.array_equal(hc[0], hs[c]) and ic[0] == its[c]
    # the cap (at the same width: the width cuts the partial sums)
    Xc, hc, ic, sc = mr.mbicg_loop(lambda U: A @ U, None, B[:, :3], np.zeros((n, 3)), TOL, 4, W=8)
    assert list(sc) == [-1, -1, -1] and list(ic) == [4, 4, 4] and all(np.array_equal(hc[c], hs[c][:4]) for c in range(3))


@pytest.mark.parametrize("nrhs", [1, 2, 3, 5, 8])
def test_a_frozen_column_is_untouched_by_every_restated_kernel(nrhs):
    rng = np.random.default_rng(nrhs)
    n = 300
    blocks = [rng.standard_normal((n, nrhs)) for _ in range(8)]
    coef = [rng.standard_normal(nrhs) for _ in range(3)]
    for frozen_col in range(nrhs):
        frozen = np.zeros(nrhs, dtype=np.int32)
        frozen[frozen_col] = 1
        bad = [np.array(c) for c in coef]
        for c in bad:
            c[frozen_col] = np.nan  # whatever a frozen column's scalars hold
        live = frozen == 0
        S_ = mr.bicg_s(bad[0], blocks[0], blocks[1], blocks[2], frozen)
        assert np.array_equal(S_[:, frozen_col], blocks[2][:, frozen_col])
        assert np.array_equal(S_[:, live], kr.bicg_s(coef[0], blocks[0], blocks[1])[:, live])
        Xn, Rn, q0, q1 = mr.bicg_xr(bad[0], bad[1], *blocks[:5], blocks[5], blocks[6], frozen)
        assert np.array_equal(Xn[:, frozen_col], blocks[5][:, frozen_col]) and np.array_equal(Rn[:, frozen_col], blocks[6][:, frozen_col])
        for c in np.flatnonzero(live):
            xs, rs, _, _ = kr.bicg_xr(coef[0][c], coef[1][c], *(b[:, c] for b in blocks[:5]), blocks[5][:, c])
            assert np.array_equal(Xn[:, c], xs) and np.array_equal(Rn[:, c], rs)
        P = mr.bicg_p(bad[2], bad[1], blocks[0], blocks[1], blocks[7], frozen)
        assert np.array_equal(P[:, frozen_col], blocks[7][:, frozen_col])
        assert np.array_equal(P[:, live], kr.bicg_p(coef[2], coef[1], blocks[0], blocks[1], blocks[7])[:, live])
        # the finalise: every code but "init" leaves a frozen column's scalars, count and status alone
        st = mr.new_state(nrhs)
        st["scal"][:] = rng.standard_normal(st["scal"].shape)
        st["frozen"][frozen_col], st["iters"][frozen_col], st["status"][frozen_col] = 1, 5, 1
        hist = np.full((nrhs, 4), -3.0)
        for code in ("alpha", "omega", "beta_res"):
            new, h = mr.finalize(code, q0, q1, st, TOL, hist, 2)
            assert np.array_equal(new["scal"][:, frozen_col], st["scal"][:, frozen_col])
            assert (new["frozen"][frozen_col], new["iters"][frozen_col], new["status"][frozen_col]) == (1, 5, 1)
            assert np.array_equal(h[frozen_col], hist[frozen_col])
            assert not live.any() or not np.array_equal(new["scal"][:, live], st["scal"][:, live])


def test_restated_partial_sums_add_up():
    """every term lands in exactly one partial: on integer-valued data every order gives the same sum"""
    rng = np.random.default_rng(9)
    for nrhs in (1, 2, 3, 4, 5, 8):
        W = mr.width(nrhs)
        for n in (1, 9, 63, 64, 65, 257, 4099, mr.GRID_MAX * mr.rows_per_pass(W) + 37):
            T = rng.integers(-8, 9, size=(n, nrhs)).astype(np.float64)
            p = mr.partials(T)
            assert p.shape == (nrhs, mr.grid(n, W))
            assert np.array_equal(mr.fin_sum(p), T.sum(axis=0)), (nrhs, n)
