"""LOBPCG with an orthonormalised basis and guard vectors on the device: the four kernels of
eig_ortho_kernels.hip through their operator-level hooks, bit for bit against numpy in the stated order and against the host
Cholesky step; whole solves under set_eig("ortho") on the inputs of test_gpu_eig.py, against analytic eigenvalues and against the
numpy restatement driven by the handle's own hooks; a generalised and a constrained solve; the clustered pencil the mode exists for;
guard vectors; isolation from the plain loop and the linear solvers.  GPU box only."""
import functools
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import hist_tolerance
from eig_restatement import row_times
from eig_ortho_restatement import active_mask, chol_ortho, lobpcg_ortho, ortho_apply
from test_eig_ortho_host import FEM_CAP, FEM_POINTS

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
RAGGED = (1, 2, 63, 64, 65, 255, 257, 1080, 70001)  # below, at and above a wave, a pass of a workgroup, several workgroups
KS = (1, 2, 3, 5, 8)
TOL = 1e-8

INPUTS = {
    "p3_12_10_9": lambda: problems.poisson3d(12, 10, 9),
    "p3_8": lambda: problems.poisson3d(8),
    "p2_40": lambda: problems.poisson2d(40),
    "fem_3000": lambda: problems.fem_unstructured(3000),
}
GRIDS = {"p3_12_10_9": (12, 10, 9), "p3_8": (8, 8, 8), "p2_40": (40, 40)}
SOLVES = [("p3_12_10_9", 1, 0), ("p3_12_10_9", 3, 0), ("p3_12_10_9", 4, 0), ("p3_12_10_9", 8, 0), ("p3_8", 4, 0), ("p3_8", 7, 0),
          ("p2_40", 6, 0), ("fem_3000", 4, 300)]


@functools.lru_cache(maxsize=None)
def csr(name):
    return INPUTS[name]()


@functools.lru_cache(maxsize=None)
def handle(name):
    return sa.sp_matrix_mg(*csr(name)).setup(sa.default_params(**QUIET)).set_eig("ortho")


def scipy_csr(triple):
    rp, ci, v = triple
    return sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, len(rp) - 1))


def analytic(name, k):
    dims = GRIDS[name]
    lam = np.zeros(dims) + 2.0 * len(dims)
    for ax, d in enumerate(dims):
        shape = [1] * len(dims)
        shape[ax] = d
        lam = lam - 2.0 * np.cos(np.arange(1, d + 1) * np.pi / (d + 1)).reshape(shape)
    return np.sort(lam.ravel())[:k]


def masked_upper(rng, k, mask):
    """an upper-triangular T whose rows and columns of masked columns are zero, as the Cholesky kernel writes it"""
    T = np.triu(rng.standard_normal((k, k)))
    T[mask == 0, :] = 0.0
    T[:, mask == 0] = 0.0
    return T


# ---------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("k", KS)
def test_transform_is_bitwise_the_stated_order(k):
    A = handle("p3_8")
    rng = np.random.default_rng(60 + k)
    for n in RAGGED:
        mask = (rng.random(k) < 0.7).astype(np.int32)
        for T in (masked_upper(rng, k, np.ones(k, dtype=np.int32)), masked_upper(rng, k, mask), rng.standard_normal((k, k))):
            for nb in (1, 2, 3):  # X alone, a pair, the three blocks of the generalised solve: one launch, in place
                blocks = [rng.standard_normal((n, k)) for _ in range(nb)]
                got = A.op_eig_transform(blocks, T)  # (the hook refuses a padding column of the device block that is not zero)
                for b, g in zip(blocks, got):
                    assert np.array_equal(g, row_times(b, T)), (n, k, nb)


@pytest.mark.parametrize("k", KS)
def test_masked_subtraction_is_bitwise_the_stated_order(k):
    A = handle("p3_8")
    rng = np.random.default_rng(80 + k)
    for n in RAGGED:
        X, W0, Cm = rng.standard_normal((n, k)), rng.standard_normal((n, k)), rng.standard_normal((k, k))
        for mask in (np.ones(k, dtype=np.int32), np.zeros(k, dtype=np.int32), (rng.random(k) < 0.5).astype(np.int32)):
            want = ortho_apply(X, Cm, W0, mask)
            assert np.array_equal(A.op_eig_ortho_apply(X, Cm, mask, W0), want), (n, k, mask)
            assert np.array_equal(A.op_eig_ortho_apply(X, Cm, mask, W0, in_place=True), want), (n, k, mask, "in place")
        # a masked column comes back as exact +0.0 whatever it held
        mask = np.ones(k, dtype=np.int32)
        mask[k - 1] = 0
        Wn = W0.copy()
        Wn[:, k - 1] = np.where(np.arange(n) % 2 == 0, np.nan, -0.0)
        for in_place in (False, True):
            got = A.op_eig_ortho_apply(X, Cm, mask, Wn, in_place=in_place)
            assert np.array_equal(got[:, :k - 1], ortho_apply(X, Cm, W0, mask)[:, :k - 1])
            assert not got[:, k - 1].any() and not np.signbit(got[:, k - 1]).any()


def spd(rng, m):
    V = rng.standard_normal((40, m)) * np.logspace(0, 2, m)
    return V.T @ V


@pytest.mark.parametrize("W", (2, 4, 8))
def test_cholesky_kernel_matches_the_host_bit_for_bit(W):
    A = handle("p3_8")
    rng = np.random.default_rng(W)
    cases = []
    for mask in (itertools.product((0, 1), repeat=W) if W <= 4 else [tuple((rng.random(W) < 0.7).astype(int)) for _ in range(12)] + [(1,) * W]):
        cases.append((spd(rng, W), np.array(mask, dtype=np.int32)))
    ones = np.ones(W, dtype=np.int32)
    V = rng.standard_normal((30, W))
    D = V.copy()
    D[:, W - 1] = D[:, 0]
    cases.append((D.T @ D, ones))  # a duplicated column
    Z = V.copy()
    Z[:, W // 2] = 0.0
    cases.append((Z.T @ Z, ones))  # a zero column
    for bad in (np.nan, np.inf, -1.0):
        G = V.T @ V
        G[W - 1, W - 1] = bad
        cases.append((G, ones))
    G = V.T @ V + np.tril(np.full((W, W), np.nan), -1)  # the lower triangle is not read
    cases.append((G, ones))
    drops = 0
    for G, mask in cases:
        T, mo = A.op_eig_chol_small(G, mask)
        Th, mh = sa.eig_chol(G, mask)
        assert np.array_equal(T, Th) and np.array_equal(mo, mh), (W, mask)
        drops += int(np.count_nonzero(mask & (1 - mo)))
    assert drops >= 5


def test_mask_kernel_is_the_rule_of_step_two():
    A = handle("p3_8")
    rng = np.random.default_rng(11)
    tol = 1e-3
    for k in range(1, 9):
        X, AX, BX = rng.standard_normal((500, k)), rng.standard_normal((500, k)), rng.standard_normal((500, k))
        theta = rng.standard_normal(k) * 3.0
        theta[0] = 0.0  # a zero theta: the bound is 0, the column active unless its residual is 0
        _, rn = A.op_eig_residual(AX, X, theta)
        _, rg, bn = A.op_eig_residual_gen(AX, BX, theta)
        for scale in (1.0, 1e3, 1e6):  # all active, mixed, all inactive but the zero theta
            assert np.array_equal(A.op_eig_active_mask(theta, rn, tol * scale), active_mask(rn, theta, tol * scale)), (k, scale)
            assert np.array_equal(A.op_eig_active_mask(theta, rg, tol * scale, bn), active_mask(rg, theta, tol * scale, bn)), (k, scale)
        # a column exactly at the bound is inactive, one ulp above it active
        th = np.full(k, 2.0)
        at = np.full(k, tol * 2.0)
        assert not A.op_eig_active_mask(th, at, tol).any()
        assert A.op_eig_active_mask(th, np.nextafter(at, np.inf), tol).all()
        b = np.full(k, 0.75)
        at = (tol * np.abs(th)) * b
        assert not A.op_eig_active_mask(th, at, tol, b).any()
        assert A.op_eig_active_mask(th, np.nextafter(at, np.inf), tol, b).all()
        z = np.zeros(k)
        assert not A.op_eig_active_mask(z, z, tol).any() and not A.op_eig_active_mask(z, z, tol, b).any()


# ---------------------------------------------------------------------------- whole solves, the standard problem

@functools.lru_cache(maxsize=None)
def solved(name, k, max_iters):
    A = handle(name)
    out = A.eigs(k, tol=TOL, max_iters=max_iters)
    return out, A.last_eigs_rc, A.eig_info(), A.eig_ortho_info()


@functools.lru_cache(maxsize=None)
def restated(name, k, max_iters):
    """the ortho restatement with the handle's own block SpMV, block V-cycle and Gram launch (see test_gpu_eig.py::restated)"""
    A = handle(name)
    X0 = np.random.default_rng(0).standard_normal((A.nrow, k))
    return lobpcg_ortho(lambda X: A.op_spmv_dot_multi(0, X)[0], lambda R: A.op_precond_multi(R), X0, tol=TOL,
                        max_iters=max_iters or A.params.max_iter, gram=A.op_gram_multi)


def follows(hist, ref, k, what):
    assert not ref["breakdown"]
    nit, nit_ref = hist.shape[1] - 1, ref["hist"].shape[1] - 1
    m = min(nit, nit_ref) + 1
    err = np.abs(hist[:, :m] - ref["hist"][:, :m]) / ref["hist"][:, :m]
    tol = np.array([hist_tolerance(ref["hist"][c, :m]) for c in range(k)])
    print(f"{what}: {nit} iterations, restatement {nit_ref}; worst history deviation / tolerance {np.max(err / tol):.3e}")
    assert abs(nit - nit_ref) <= max(2, 0.1 * nit_ref)
    assert np.all(err <= tol), f"max history deviation / tolerance {np.max(err / tol):.3e} at {np.unravel_index(np.argmax(err / tol), err.shape)}"


@pytest.mark.parametrize("name,k,max_iters", SOLVES)
def test_ortho_solver_finds_the_lowest_eigenpairs(name, k, max_iters):
    (lam, X, iters, hist, status), rc, info, oinfo = solved(name, k, max_iters)
    M = scipy_csr(csr(name))
    assert rc == sa.SPARSH_OK and np.all(status == sa.SPARSH_OK)
    assert np.all(np.diff(lam) >= 0)
    if name in GRIDS:
        ref = analytic(name, k)
        assert np.all(np.abs(lam - ref) <= TOL * ref), (lam, ref)
    norm_inf = abs(M).sum(axis=1).max()
    res = np.linalg.norm(M @ X - X * lam, axis=0)
    orth = np.max(np.abs(X.T @ X - np.eye(k)))
    print(f"{name} k={k}: {hist.shape[1] - 1} iterations, iters {iters.tolist()}, max residual / (tol lam) "
          f"{np.max(res / (TOL * lam)):.3f}, orthonormality {orth:.2e}, restarts {info['restarts']}, drops {oinfo['dropped_w']} {oinfo['dropped_p']}")
    assert np.all(res <= TOL * lam + 1e-12 * norm_inf * np.linalg.norm(X, axis=0))
    assert orth <= 1e-12
    assert hist.shape[1] >= iters.max() + 1
    W = sa.multi_width(k) if hasattr(sa, "multi_width") else (2 if k <= 2 else 4 if k <= 4 else 8)
    assert oinfo["bytes"] == 8 * (3 * W + 2 * W * W)  # three masks and two W x W matrices


@pytest.mark.parametrize("name,k,max_iters", SOLVES)
def test_ortho_solver_follows_the_restatement(name, k, max_iters):
    (lam, X, iters, hist, status), *_ = solved(name, k, max_iters)
    follows(hist, restated(name, k, max_iters), k, f"{name} k={k}")


# ---------------------------------------------------------------------------- the generalised and the constrained problem

@functools.lru_cache(maxsize=None)
def pencil_handle():
    A, B = problems.fem_pencil(3000)
    H = sa.sp_matrix_mg(*A).setup(sa.default_params(**QUIET)).set_eig("ortho")
    H.set_eig_b(*B)
    return H, scipy_csr(A), scipy_csr(B)


def test_generalised_solve_in_ortho_mode():
    H, As, Bs = pencil_handle()
    k = 4
    lam, X, iters, hist, status = H.eigs_gen(k, tol=TOL, max_iters=300)
    assert H.last_eigs_rc == sa.SPARSH_OK and np.all(status == sa.SPARSH_OK)
    BX = Bs @ X
    res = np.linalg.norm(As @ X - BX * lam, axis=0)
    a_inf, b_inf = abs(As).sum(axis=1).max(), abs(Bs).sum(axis=1).max()
    assert np.all(np.diff(lam) >= 0)
    assert np.all(res <= TOL * lam * np.linalg.norm(BX, axis=0) + 1e-12 * (a_inf + lam * b_inf) * np.linalg.norm(X, axis=0))
    assert np.max(np.abs(X.T @ BX - np.eye(k))) <= 1e-12
    cond_b = np.linalg.cond(Bs.toarray())
    assert abs(lam[0] - 1.0) <= TOL * np.sqrt(cond_b)  # the constant vector: lambda_0 = 1
    X0 = np.random.default_rng(0).standard_normal((H.nrow, k))
    ref = lobpcg_ortho(lambda V: H.op_spmv_dot_multi(0, V)[0], lambda R: H.op_precond_multi(R), X0, apply_B=H.op_eig_b_multi, tol=TOL,
                       max_iters=300, gram=H.op_gram_multi)
    follows(hist, ref, k, "fem_pencil(3000) k=4")
    assert np.all(np.abs(lam - ref["lam"]) <= 10 * TOL * ref["lam"])


def test_constrained_solve_on_a_null_space_handle_in_ortho_mode():
    dims, k = (12, 10, 9), 3
    rp, ci, v = problems.poisson3d_neumann(*dims)
    N = sa.sp_matrix_mg(rp, ci, v)
    N.set_nullspace("constant")
    N.setup(sa.default_params(**QUIET)).set_eig("ortho")
    M = scipy_csr((rp, ci, v))
    n = M.shape[0]
    lam, X, iters, hist, status = N.eigs_con(k, tol=TOL)
    assert N.last_eigs_rc == sa.SPARSH_OK and np.all(status == sa.SPARSH_OK)
    full = np.zeros(dims)
    for ax, d in enumerate(dims):
        shape = [1] * 3
        shape[ax] = d
        full = full + (2.0 - 2.0 * np.cos(np.arange(d) * np.pi / d)).reshape(shape)
    ref = np.sort(full.ravel())[1:k + 1]  # the lowest nonzero eigenvalues of the Neumann Laplacian
    assert np.all(np.abs(lam - ref) <= TOL * ref), (lam, ref)
    res = np.linalg.norm(M @ X - X * lam, axis=0)
    assert np.all(res <= TOL * lam + 1e-12 * abs(M).sum(axis=1).max() * np.linalg.norm(X, axis=0))
    assert np.max(np.abs(X.T @ X - np.eye(k))) <= 1e-12
    # the drift of the constraint, within the bound of test_gpu_eig_con.py: ten times the restatement's or the rounding floor
    lu = spla.splu((M + 1e-2 * sp.identity(n)).tocsc())
    X0 = np.random.default_rng(0).standard_normal((n, k))
    r = lobpcg_ortho(lambda V: M @ V, lambda R: lu.solve(R), X0, Y=np.ones((n, 1)), tol=TOL, max_iters=300)
    assert not r["breakdown"] and not r["rank_deficient"]
    drift, drift_ref = np.abs(np.ones(n) @ X), np.abs(np.ones(n) @ r["X"])
    floor = n * 2.0 ** -53 * np.mean(np.abs(X), axis=0)
    print(f"drift {drift.max():.3e}, restatement {drift_ref.max():.3e}, floor {floor.max():.3e}")
    assert np.all(drift <= 10.0 * np.maximum(drift_ref, floor))
    assert N.eig_con_info()["ncon_total"] == 1 and N.eig_ortho_info()["bytes"] > 0
    N.close()


# ---------------------------------------------------------------------------- the clustered pencil

@functools.lru_cache(maxsize=None)
def clustered():
    A, B = problems.fem_pencil(FEM_POINTS)
    H = sa.sp_matrix_mg(*A).setup(sa.default_params(**QUIET))
    H.set_eig_b(*B)
    return H, scipy_csr(A), scipy_csr(B)


def worst_residual(As, Bs, lam, X):
    BX = Bs @ X
    return np.max(np.linalg.norm(As @ X - BX * lam, axis=0) / (TOL * np.abs(lam) * np.linalg.norm(BX, axis=0)))


def test_clustered_pencil_converges_in_ortho_mode():
    """fem_pencil(FEM_POINTS), k = 8, cap 300: SPARSH_OK with no restart under the ortho basis; the plain basis' outcome on the
    same handle is printed (profiles/eig_ortho_lobpcg.txt records it)."""
    H, As, Bs = clustered()
    H.set_eig("plain")
    lam, X, iters, hist, status = H.eigs_gen(8, tol=TOL, max_iters=FEM_CAP)
    print(f"plain: rc {H.last_eigs_rc}, {hist.shape[1] - 1} iterations, restarts {H.eig_info()['restarts']}, active "
          f"{(status != 0).astype(int).tolist()}, worst residual / bound {worst_residual(As, Bs, lam, X):.3e}")
    # (it failed on the device when profiles/eig_ortho_lobpcg.txt was taken: the cap, 8 restarts, 3.7e10 times the bound)
    assert H.last_eigs_rc == sa.SPARSH_ENOCONV
    H.set_eig("ortho")
    lam, X, iters, hist, status = H.eigs_gen(8, tol=TOL, max_iters=FEM_CAP)
    worst = worst_residual(As, Bs, lam, X)
    print(f"ortho: rc {H.last_eigs_rc}, {hist.shape[1] - 1} iterations, restarts {H.eig_info()['restarts']}, {H.eig_ortho_info()}, "
          f"worst residual / bound {worst:.3e}")
    assert H.last_eigs_rc == sa.SPARSH_OK and np.all(status == sa.SPARSH_OK)
    assert H.eig_info()["restarts"] == 0
    assert worst <= 1.0, worst
    assert np.max(np.abs(X.T @ (Bs @ X) - np.eye(8))) <= 1e-12


def test_guard_vectors_bring_four_pairs_home_under_the_cap():
    H, As, Bs = clustered()
    H.set_eig("ortho", wanted=0)
    lam, X, iters, hist, status = H.eigs_gen(4, tol=TOL, max_iters=FEM_CAP, guard=4)
    assert H.eig_options() == dict(basis="ortho", wanted=0)
    nit = hist.shape[1] - 1
    print(f"k = 4, guard 4: rc {H.last_eigs_rc}, {nit} iterations, worst residual / bound {worst_residual(As, Bs, lam, X):.3e}")
    assert H.last_eigs_rc == sa.SPARSH_OK and np.all(status == sa.SPARSH_OK)
    assert nit < FEM_CAP  # fewer than k = 4 without guards is allowed
    assert lam.shape == (4,) and X.shape == (H.nrow, 4) and hist.shape[0] == 4
    assert worst_residual(As, Bs, lam, X) <= 1.0
    lam0, X0_, it0, hist0, st0 = H.eigs_gen(4, tol=TOL, max_iters=FEM_CAP)
    print(f"k = 4 without guards: rc {H.last_eigs_rc}, {hist0.shape[1] - 1} iterations")
    assert nit < hist0.shape[1] - 1 or H.last_eigs_rc == sa.SPARSH_ENOCONV


def test_wanted_on_the_device_in_both_modes():
    A = handle("p3_12_10_9")
    try:
        for basis in ("plain", "ortho"):
            A.set_eig(basis, wanted=0)
            full = A.eigs(6, tol=TOL)
            A.set_eig(basis, wanted=3)
            lam, X, iters, hist, status = A.eigs(6, tol=TOL)
            nit = hist.shape[1] - 1
            assert A.last_eigs_rc == sa.SPARSH_OK
            assert nit <= full[3].shape[1] - 1
            assert np.array_equal(hist, full[3][:, :nit + 1])  # the same loop, ended earlier
            assert np.all(status[:3] == sa.SPARSH_OK)
            assert np.array_equal(status[3:] == sa.SPARSH_ENOCONV, hist[3:, -1] > TOL * np.abs(lam[3:]))
            ref = analytic("p3_12_10_9", 3)
            assert np.all(np.abs(lam[:3] - ref) <= TOL * ref)
            A.set_eig(basis, wanted=6)
            same = A.eigs(6, tol=TOL)
            assert all(np.array_equal(a, b) for a, b in zip(same, full))  # wanted = nev is wanted = 0
            A.set_eig(basis, wanted=7)
            with pytest.raises(sa.SparshError) as e:
                A.eigs(6, tol=TOL)
            assert e.value.code == sa.SPARSH_EINVAL
    finally:
        A.set_eig("ortho", wanted=0)


# ---------------------------------------------------------------------------- isolation

def test_isolated_from_the_plain_loop_and_the_linear_solvers():
    A_csr, B_csr = problems.fem_pencil(3000)
    H = sa.sp_matrix_mg(*A_csr).setup(sa.default_params(**QUIET))
    H.set_eig_b(*B_csr)
    n = H.nrow
    rng = np.random.default_rng(9)
    Bm = rng.standard_normal((n, 3))

    def plain_three():
        e = H.eigs(3, tol=TOL, max_iters=40)
        g = H.eigs_gen(3, tol=TOL, max_iters=40)
        Xm = np.zeros((n, 3))
        H.solve_multi("pcg", Bm, Xm)
        return list(e) + list(g) + [Xm], H.eig_info()["bytes"]

    before, bytes_before = plain_three()
    assert H.eig_ortho_info()["bytes"] == 0
    H.set_eig("ortho")
    o1 = H.eigs_gen(3, tol=TOL, max_iters=40)
    assert H.eig_ortho_info()["bytes"] == 8 * (3 * 4 + 2 * 16)
    assert H.eig_info()["bytes"] == bytes_before  # the mode's memory is counted on its own
    o2 = H.eigs_gen(3, tol=TOL, max_iters=40)
    assert all(np.array_equal(a, b) for a, b in zip(o1, o2))  # two ortho solves from one start block: the same bits
    t = H.bench_op_multi("eig_transform", 0, nrhs=4, reps=2)
    s = H.bench_op_multi("eig_ortho_apply", 0, nrhs=4, reps=2)
    assert t > 0.0 and s > 0.0
    H.set_eig("plain")
    assert H.eig_ortho_info()["bytes"] == 0  # a change of basis frees it
    with pytest.raises(sa.SparshError) as e:
        H.bench_op_multi("eig_transform", 0, nrhs=4, reps=2)
    assert e.value.code == sa.SPARSH_ESTATE
    after, bytes_after = plain_three()
    assert bytes_after == bytes_before
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    H.close()
