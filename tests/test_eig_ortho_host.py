"""LOBPCG with an orthonormalised basis and guard vectors, the parts that need no GPU: the numpy restatement
of the loop against analytic eigenvalues and against the plain restatement, the clustered pencil the mode exists for on a CPU
hierarchy, the host Cholesky step (sparsh_debug_eig_chol) against numpy, against the restatement bit for bit and on its drop rule,
the guard vectors, and the setter, the getter and the guard= keyword without a device."""
import functools
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from eig_restatement import lobpcg
from eig_gen_restatement import lobpcg_gen
from eig_ortho_restatement import chol_ortho, lobpcg_ortho

QUIET = dict(print_setup=0, print_solve=0)
TOL = 1e-8
FEM_POINTS = 60000  # the clustered pencil of test_clustered_pencil...; test_gpu_eig_ortho.py solves the same one on the device
FEM_CAP = 300
OMEGA = 0.66667


def analytic(dims, k):
    lam = np.zeros(dims) + 2.0 * len(dims)
    for ax, d in enumerate(dims):
        shape = [1] * len(dims)
        shape[ax] = d
        lam = lam - 2.0 * np.cos(np.arange(1, d + 1) * np.pi / (d + 1)).reshape(shape)
    return np.sort(lam.ravel())[:k]


def scipy_csr(triple):
    rp, ci, v = triple
    n = len(rp) - 1
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


# ---------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("dims,k", [((12, 10, 9), 3), ((12, 10, 9), 8), ((40, 40), 6)])
def test_restatement_reaches_the_analytic_eigenvalues(dims, k):
    A = scipy_csr(problems.poisson3d(*dims) if len(dims) == 3 else problems.poisson2d(dims[0]))
    n = A.shape[0]
    lu = spla.splu(A.tocsc())
    X0 = np.random.default_rng(0).standard_normal((n, k))
    plain = lobpcg(lambda X: A @ X, lambda R: lu.solve(R), X0, tol=TOL, max_iters=200)
    out = lobpcg_ortho(lambda X: A @ X, lambda R: lu.solve(R), X0, tol=TOL, max_iters=200)
    assert not out["breakdown"] and out["converged"] and not out["status"].any()
    nit, nit_plain = out["hist"].shape[1] - 1, plain["hist"].shape[1] - 1
    print(f"{dims} k={k}: {nit} iterations, plain {nit_plain}, restarts {out['restarts']}, drops {out['dropped_w']} {out['dropped_p']}")
    assert nit <= nit_plain + max(2, 0.1 * nit_plain)
    ref = analytic(dims, k)
    assert np.all(np.diff(out["lam"]) >= 0)
    assert np.all(np.abs(out["lam"] - ref) <= TOL * ref), (out["lam"], ref)
    X = out["X"]
    assert np.max(np.abs(X.T @ X - np.eye(k))) <= 1e-12
    assert np.all(np.linalg.norm(A @ X - X * out["lam"], axis=0) <= TOL * out["lam"] + 1e-12 * 12.0)


class BlockCycle:
    """The scipy V-cycle restatement of test_gpu_nullspace.py on (n, k) blocks: heavy-edge pairwise aggregation (its hem), Galerkin
    products, weighted-Jacobi V(7,7) from a zero guess, a direct solve at 2 000 rows or fewer"""

    def __init__(self, A0, limit=2000):
        from test_gpu_nullspace import hem
        self.A, self.P = [A0.tocsr()], []
        while self.A[-1].shape[0] > limit:
            a = self.A[-1]
            a.sort_indices()
            p = hem(a, len(self.A) - 1)
            self.P.append(p)
            self.A.append((p.T @ a @ p).tocsr())
        self.D = [a.diagonal()[:, None] for a in self.A]
        self.lu = spla.splu(self.A[-1].tocsc())

    def __call__(self, b, l=0, nu=7):
        if l == len(self.A) - 1:
            return self.lu.solve(b)
        A, D = self.A[l], self.D[l]
        x = OMEGA * b / D
        for _ in range(nu - 1):
            x = x + OMEGA * (b - A @ x) / D
        x = x + self.P[l] @ self(self.P[l].T @ (b - A @ x), l + 1, nu)
        for _ in range(nu):
            x = x + OMEGA * (b - A @ x) / D
        return x


@functools.lru_cache(maxsize=None)
def fem():
    A, B = problems.fem_pencil(FEM_POINTS)
    As, Bs = scipy_csr(A), scipy_csr(B)
    return As, Bs, BlockCycle(As)


def test_clustered_pencil_converges_with_the_ortho_basis_and_not_with_the_plain_one():
    """fem_pencil(60000), k = 8, cap 300, tol 1e-8, seven levels of the scipy V-cycle (60000, 30230, 15221, 7750, 3970, 2065, 1074
    rows).  Measured on the CPU: the ortho restatement converges every column in 180 iterations with no restart and no drop, worst
    recomputed residual 0.73 of the bound; the plain restatement does not converge: it ends in a Rayleigh-Ritz breakdown after 20
    restarts (at 22 000 to 30 000 points it ends at the cap with 3 to 5 restarts and residuals 1e3 to 9e7 times the bound).  Without
    the step W <- W - P (BP)^T W the ortho restatement fails here too (cap, 1 restart, 12 dropped P columns, 1.4e7 times the bound)."""
    As, Bs, M = fem()
    k = 8
    X0 = np.random.default_rng(0).standard_normal((As.shape[0], k))
    out = lobpcg_ortho(lambda X: As @ X, M, X0, apply_B=lambda X: Bs @ X, tol=TOL, max_iters=FEM_CAP)
    assert not out["breakdown"]
    X, lam = out["X"], out["lam"]
    BX = Bs @ X
    worst = np.max(np.linalg.norm(As @ X - BX * lam, axis=0) / (TOL * np.abs(lam) * np.linalg.norm(BX, axis=0)))
    print(f"ortho: {len(M.A)} levels, {out['hist'].shape[1] - 1} iterations, restarts {out['restarts']}, drops {out['dropped_w']} "
          f"{out['dropped_p']}, worst residual / bound {worst:.3e}")
    assert out["converged"] and not out["status"].any() and out["restarts"] == 0
    assert worst <= 1.0 + 1e-3  # the carried residual met the rule; the recomputed one differs from it by rounding
    plain = lobpcg_gen(lambda X: As @ X, lambda X: Bs @ X, M, X0, tol=TOL, max_iters=FEM_CAP)
    if plain["breakdown"]:
        print(f"plain: breakdown after {plain['restarts']} restarts")
    else:
        Xp, lp = plain["X"], plain["lam"]
        BXp = Bs @ Xp
        wp = np.max(np.linalg.norm(As @ Xp - BXp * lp, axis=0) / (TOL * np.abs(lp) * np.linalg.norm(BXp, axis=0)))
        print(f"plain: {plain['hist'].shape[1] - 1} iterations, restarts {plain['restarts']}, active {plain['status'].tolist()}, "
              f"worst residual / bound {wp:.3e}")
        assert plain["status"].any()


# ---------------------------------------------------------------------------- the host Cholesky step

def random_gram(m, seed):
    V = np.random.default_rng(seed).standard_normal((40 + m, m)) * np.logspace(0, 3, m)
    return V.T @ V


def masks(m):
    return [np.array(p, dtype=np.int32) for p in itertools.product((0, 1), repeat=m)]


@pytest.mark.parametrize("m", range(1, 9))
def test_chol_matches_numpy_cholesky(m):
    G = random_gram(m, m)
    for mask in (masks(m) if m == 6 else [np.ones(m, dtype=np.int32)]):  # every mask pattern of one order
        T, mo = sa.eig_chol(G, mask)
        assert np.array_equal(mo, mask)
        idx = np.flatnonzero(mask)
        off = np.ones((m, m), dtype=bool)
        off[np.ix_(idx, idx)] = False
        assert not T[off].any()  # rows and columns of masked columns are zero
        if len(idx) == 0:
            continue
        Ts = T[np.ix_(idx, idx)]
        assert np.array_equal(Ts, np.triu(Ts))
        ref = np.linalg.inv(np.linalg.cholesky(G[np.ix_(idx, idx)])).T  # T = L^-T of the unscaled factor
        scale = np.sqrt(np.diag(G)[idx])
        assert np.max(np.abs(Ts - ref) * scale[:, None]) <= 1e-13 * max(1.0, np.max(np.abs(ref) * scale[:, None])), (m, mask)
        assert np.max(np.abs(Ts.T @ G[np.ix_(idx, idx)] @ Ts - np.eye(len(idx)))) <= 1e-10


@pytest.mark.parametrize("m", range(1, 9))
def test_chol_and_restatement_give_the_same_bits(m):
    rng = np.random.default_rng(50 + m)
    for trial in range(8):
        G = random_gram(m, 100 * m + trial)
        mask = (rng.random(m) < 0.75).astype(np.int32)
        if trial == 0:
            mask[:] = 1
        if trial == 1 and m > 1:
            G[:, m - 1] = G[:, 0]  # a duplicated column: a drop on both sides
            G[m - 1, m - 1] = G[0, 0]
        T, mo = sa.eig_chol(G, mask)
        Tr, mr = chol_ortho(G, mask)
        assert np.array_equal(T, Tr) and np.array_equal(mo, mr), (m, trial)


def test_chol_drop_rule():
    rng = np.random.default_rng(3)
    V = rng.standard_normal((30, 5))
    ones = np.ones(5, dtype=np.int32)

    def kept(G):
        T, mo = sa.eig_chol(G, ones)
        Tr, mr = chol_ortho(G, ones)
        assert np.array_equal(T, Tr) and np.array_equal(mo, mr)
        for c in np.flatnonzero(mo == 0):
            assert not T[:, c].any() and not T[c, :].any()
        idx = np.flatnonzero(mo)
        Ts = T[np.ix_(idx, idx)]
        assert np.max(np.abs(Ts.T @ G[np.ix_(idx, idx)] @ Ts - np.eye(len(idx)))) <= 1e-10
        return mo.tolist()

    D = V.copy()
    D[:, 3] = D[:, 1]  # a duplicated column: the later one goes
    assert kept(D.T @ D) == [1, 1, 1, 0, 1]
    Z = V.copy()
    Z[:, 2] = 0.0  # a zero column
    assert kept(Z.T @ Z) == [1, 1, 0, 1, 1]
    G = V.T @ V
    G[4, 4] = np.nan  # a NaN diagonal
    assert kept(G) == [1, 1, 1, 1, 0]
    G = V.T @ V
    G[0, 0] = np.inf
    assert kept(G) == [0, 1, 1, 1, 1]
    G = V.T @ V
    G[1, 1] = -1.0
    assert kept(G) == [1, 0, 1, 1, 1]


def test_chol_reads_the_upper_triangle_only():
    G = random_gram(6, 9)
    junk = G + np.tril(np.full((6, 6), np.nan), -1)
    mask = np.array([1, 1, 0, 1, 1, 1], dtype=np.int32)
    junk[2, :] = junk[:, 2] = np.nan  # nor the rows and columns outside the mask
    T, mo = sa.eig_chol(G, mask)
    Tj, mj = sa.eig_chol(junk, mask)
    assert np.array_equal(T, Tj) and np.array_equal(mo, mj) and np.array_equal(mo, mask)


def test_chol_bad_arguments():
    z = np.eye(8)
    i8 = np.ones(8, dtype=np.int32)
    DP, IP = sa.c_dbl_p, sa.c_int_p
    for m in (0, 9):
        assert sa.lib.sparsh_debug_eig_chol(m, z.ctypes.data_as(DP), i8.ctypes.data_as(IP), z.ctypes.data_as(DP), i8.ctypes.data_as(IP)) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_debug_eig_chol(2, None, None, None, None) == sa.SPARSH_EINVAL


# ---------------------------------------------------------------------------- guard vectors

@functools.lru_cache(maxsize=None)
def guard_problem():
    A = scipy_csr(problems.poisson3d(12, 10, 9))
    d = 1.0 / A.diagonal()
    return A, (lambda R: R * d[:, None]), np.random.default_rng(4).standard_normal((A.shape[0], 6))


def test_wanted_stops_when_the_lowest_columns_are_inactive():
    A, M, X0 = guard_problem()  # Jacobi as the preconditioner: slow enough for the columns to finish one after the other
    full = lobpcg_ortho(lambda X: A @ X, M, X0, tol=1e-6, max_iters=400)
    out = lobpcg_ortho(lambda X: A @ X, M, X0, tol=1e-6, max_iters=400, wanted=4)
    assert full["converged"] and out["converged"]
    nit = out["hist"].shape[1] - 1
    assert nit < full["hist"].shape[1] - 1
    bound = 1e-6 * np.abs(out["lam"])
    assert np.all(out["hist"][:4, -1] <= bound[:4])  # the wanted columns are inactive at the evaluation that ends the solve
    assert np.array_equal(out["hist"][:, :nit + 1], full["hist"][:, :nit + 1])  # and the loop up to there is the full one
    assert np.any(out["hist"][:4, nit - 1] > 1e-6 * np.abs(out["lam"][:4]) * (1.0 + 1e-3))  # and not one evaluation earlier
    # still-active guard columns come back as not converged
    assert out["status"][:4].tolist() == [0, 0, 0, 0]
    assert out["status"][4:].any()
    assert np.array_equal(out["status"][4:], (out["hist"][4:, -1] > bound[4:]).astype(int))


def test_wanted_zero_and_nev_behave_alike():
    A, M, X0 = guard_problem()
    a = lobpcg_ortho(lambda X: A @ X, M, X0[:, :4], tol=1e-6, max_iters=60, wanted=0)
    b = lobpcg_ortho(lambda X: A @ X, M, X0[:, :4], tol=1e-6, max_iters=60, wanted=4)
    assert np.array_equal(a["hist"], b["hist"]) and np.array_equal(a["X"], b["X"]) and np.array_equal(a["status"], b["status"])


# ---------------------------------------------------------------------------- the options without a device

@pytest.fixture()
def fresh():
    A = sa.sp_matrix_mg(*problems.poisson2d(12))
    yield A
    A.close()


def test_options_round_trip_without_a_device(fresh):
    A = fresh
    assert A.eig_options() == dict(basis="plain", wanted=0)
    assert A.eig_ortho_info() == dict(dropped_w=0, dropped_p=0, bytes=0)
    assert A.set_eig("ortho", wanted=5) is A
    assert A.eig_options() == dict(basis="ortho", wanted=5)
    A.setup(sa.default_params(**QUIET), host_only=True)  # the settings are the handle's: a setup keeps them
    assert A.eig_options() == dict(basis="ortho", wanted=5)
    A.set_eig("plain", wanted=8)
    assert A.eig_options() == dict(basis="plain", wanted=8)
    A.set_eig()
    assert A.eig_options() == dict(basis="plain", wanted=0)
    assert A.eig_ortho_info()["bytes"] == 0


@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_bad_options_are_einval_without_a_device(fresh, prepared):
    A = fresh
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    A.set_eig("ortho", wanted=2)
    for basis, wanted, word in ((2, 0, "basis"), (-1, 0, "basis"), (0, -1, "wanted"), (1, 9, "wanted")):
        with pytest.raises(sa.SparshError) as e:
            A.set_eig(basis, wanted)
        assert e.value.code == sa.SPARSH_EINVAL and word in str(e.value)
    assert A.eig_options() == dict(basis="ortho", wanted=2)  # a refused call changes nothing
    assert sa.lib.sparsh_set_eig_options(None, 0, 0) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_eig_options(None, None, None) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_eig_ortho_info(None, None, None, None) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_eig_options(A._h, None, None) == sa.SPARSH_OK


@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_wanted_above_nev_is_einval_in_the_solve(fresh, prepared):
    A = fresh
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    A.set_eig("plain", wanted=5)
    for call in (lambda: A.eigs(4), lambda: A.eigs_gen(3), lambda: A.eigs_con(4)):
        with pytest.raises(sa.SparshError) as e:
            call()
        assert e.value.code == sa.SPARSH_EINVAL and "wanted" in str(e.value)
    with pytest.raises(sa.SparshError) as e:
        A.eigs(5)  # wanted == nev is fine: what is missing now is the setup (or the device)
    assert e.value.code in (sa.SPARSH_ESTATE, sa.SPARSH_ENODEV)


def test_guard_keyword_restores_the_setting_also_when_the_solve_raises(fresh):
    A = fresh
    A.set_eig("ortho", wanted=2)
    with pytest.raises(sa.SparshError) as e:
        A.eigs(3, guard=2)  # no setup: the solve raises after wanted was set to 3
    assert e.value.code in (sa.SPARSH_ESTATE, sa.SPARSH_ENODEV)
    assert A.eig_options() == dict(basis="ortho", wanted=2)
    for call in (lambda: A.eigs_gen(3, guard=1), lambda: A.eigs_con(2, guard=3)):
        with pytest.raises(sa.SparshError):
            call()
        assert A.eig_options() == dict(basis="ortho", wanted=2)
    for k, g in ((5, 4), (8, 1), (0, 2), (3, -1)):
        with pytest.raises(ValueError):
            A.eigs(k, guard=g)
        assert A.eig_options() == dict(basis="ortho", wanted=2)
    for op in ("eig_transform", "eig_ortho_apply"):  # no device work before a setup
        with pytest.raises(sa.SparshError) as e:
            A.bench_op_multi(op, 0, nrhs=8)
        assert e.value.code == sa.SPARSH_ESTATE
