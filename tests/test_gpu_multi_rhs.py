"""A block of up to 8 right-hand sides in one AMG-PCG run against what the handle offers for one vector: the
block operators column by column against the single-vector entry points (bitwise), the block V-cycle against the Jacobi cycle
composed from those entry points (bitwise), independence of the columns, the head of block PCG against the numpy restatement, whole
block solves against single solves, and the life cycle of the block buffers.  GPU box only.

Where a level holds a row longer than one workgroup's LDS buffer (the dense-row grid) the single-vector SpMV, residual and Jacobi
kernels add that row's products in a tree; the block kernels add them in stored order, chunk by chunk, and are compared there with
the stored-order numpy restatement of the Chebyshev tests (ChebRef.rowsum) instead.
"""
import functools

import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import hist_tolerance, load_c0
from test_gpu_chebyshev import ChebRef
from test_gpu_gmres import assert_history, assert_solution
from test_gpu_precond_sites import pcg_ref
from test_gpu_sor import INPUTS as SOR_INPUTS

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
NRHS = (1, 2, 3, 4, 5, 8)  # every width (2, 4, 8), with and without padding columns
INPUTS = dict(SOR_INPUTS)
INPUTS["tiny"] = problems.poisson2d(3)  # 9 rows on a single level: fewer than one pass of a workgroup
KSTREAM = 2048  # kStreamNnz: products one workgroup's LDS buffer holds


@functools.lru_cache(maxsize=None)
def handle(name):
    return sa.sp_matrix_mg(*INPUTS[name]).setup(sa.default_params(**QUIET))


class Single:
    """The single-vector operators of a handle, column by column; on a level with a row longer than the LDS buffer the stored-order
    numpy restatement stands in for the row sums"""

    def __init__(self, A):
        self.A = A
        self.omega = A.params.omega
        self.ref = {}
        for l in range(A.nlevels):
            rp = A.level_csr(l)[0]
            if np.diff(rp).max() > KSTREAM:
                self.ref[l] = ChebRef(A, l)

    def spmv_dot(self, l, x):
        if l in self.ref:
            y = self.ref[l].rowsum(x)
            return y, float(x @ y)
        return self.A.op_spmv_dot(l, x)

    def residual(self, l, b, x):
        if l in self.ref:
            return 1.0 * b + (-1.0) * self.ref[l].rowsum(x)
        return self.A.op_residual(l, b, x)

    def jacobi(self, l, b, x, sweeps, zero=False):
        if l not in self.ref:
            return self.A.op_jacobi(l, b, x, sweeps, x_is_zero=zero)
        r = self.ref[l]
        x = np.array(x, dtype=np.float64)
        k = 0
        if zero and sweeps > 0:
            x, k = self.omega * b / r.diag, 1
        elif zero:
            x = np.zeros_like(b)
        for _ in range(k, sweeps):
            h = 1.0 * b + (-1.0) * r.rowsum(x)
            x = x + self.omega * h / r.diag
        return x

    def cycle(self, r, nu):
        """the Jacobi V(nu,nu) cycle from a zero guess in the order of Engine::vcycle_multi (composed_cycle of test_gpu_sor with Jacobi legs)"""
        A = self.A
        last = A.nlevels - 1
        if last == 0:
            return A.op_coarse(r)
        bs, xs = [r], []
        for l in range(last):
            xl = self.jacobi(l, bs[l], np.zeros(len(bs[l])), nu, zero=True)
            xs.append(xl)
            bs.append(A.op_restrict(l, self.residual(l, bs[l], xl)))
        xc = A.op_coarse(bs[last])
        for l in range(last, 0, -1):
            xc = self.jacobi(l - 1, bs[l - 1], A.op_prolong(l - 1, xc, xs[l - 1]), nu)
        return xc


@functools.lru_cache(maxsize=None)
def single(name):
    return Single(handle(name))


def columns(fn, *blocks):
    return np.column_stack([fn(*(b[:, c] for b in blocks)) for c in range(blocks[0].shape[1])])


@pytest.mark.parametrize("name", list(INPUTS))
def test_block_operators_are_bitwise_the_single_vector_operators(name):
    A, S = handle(name), single(name)
    rng = np.random.default_rng(21)
    last = A.nlevels - 1
    for l in range(A.nlevels):
        n = A.level_info(l)["nrow"]
        X, B = rng.standard_normal((n, 8)), rng.standard_normal((n, 8))
        ys = [S.spmv_dot(l, X[:, c]) for c in range(8)]
        want = dict(
            y=np.column_stack([y for y, _ in ys]), dot=np.array([d for _, d in ys]),
            r=columns(lambda b, x: S.residual(l, b, x), B, X),
            j1=columns(lambda b, x: S.jacobi(l, b, x, 1), B, X),
            j3=columns(lambda b, x: S.jacobi(l, b, x, 3), B, X),
            z3=columns(lambda b, x: S.jacobi(l, b, x, 3, zero=True), B, X),
            z1=columns(lambda b, x: S.jacobi(l, b, x, 1, zero=True), B, X))
        if l < last:
            nc = A.level_info(l + 1)["nrow"]
            XC = rng.standard_normal((nc, 8))
            want["bc"] = columns(lambda r: A.op_restrict(l, r), X)
            want["xf"] = columns(lambda xc, xf: A.op_prolong(l, xc, xf), XC, X)
        else:
            want["xl"] = columns(A.op_coarse, B)
        for k in NRHS:
            tag = (name, l, k)
            Y, dots = A.op_spmv_dot_multi(l, X[:, :k])
            assert np.array_equal(Y, want["y"][:, :k]), tag
            scale = np.abs(X[:, :k] * want["y"][:, :k]).sum(axis=0)
            err = np.abs(dots - want["dot"][:k])
            print(tag, "dots: largest error / sum |x_i s_i|", (err / scale).max())
            assert np.all(err <= 1e-13 * scale), tag
            assert np.array_equal(A.op_residual_multi(l, B[:, :k], X[:, :k]), want["r"][:, :k]), tag
            assert np.array_equal(A.op_jacobi_multi(l, B[:, :k], X[:, :k], 1), want["j1"][:, :k]), tag
            assert np.array_equal(A.op_jacobi_multi(l, B[:, :k], X[:, :k], 3), want["j3"][:, :k]), tag
            assert np.array_equal(A.op_jacobi_multi(l, B[:, :k], X[:, :k], 3, x_is_zero=True), want["z3"][:, :k]), tag
            assert np.array_equal(A.op_jacobi_multi(l, B[:, :k], X[:, :k], 1, x_is_zero=True), want["z1"][:, :k]), tag
            if l < last:
                assert np.array_equal(A.op_restrict_multi(l, X[:, :k]), want["bc"][:, :k]), tag
                assert np.array_equal(A.op_prolong_multi(l, XC[:, :k], X[:, :k]), want["xf"][:, :k]), tag
            else:
                assert np.array_equal(A.op_coarse_multi(B[:, :k]), want["xl"][:, :k]), tag


@pytest.mark.parametrize("name", list(INPUTS))
def test_block_cycle_is_bitwise_the_composed_jacobi_cycle(name):
    A, S = handle(name), single(name)
    nu = A.params.sweeps
    R = np.random.default_rng(22).standard_normal((A.nrow, 8))
    want = columns(lambda r: S.cycle(r, nu), R)
    for k in NRHS:
        Z = A.op_precond_multi(R[:, :k])
        assert np.array_equal(Z, want[:, :k]), (name, k, np.abs(Z - want[:, :k]).max())
    if name != "dense_row":  # (there op_precond adds the long row's products in a tree: compared with the restatement above only)
        for c in (0, 7):
            z = A.op_precond(R[:, c])
            diff = np.abs(want[:, c] - z).max()
            print(name, c, "difference from op_precond", diff, "of", np.abs(z).max())
            assert diff <= 1e-13 * np.abs(z).max()


def block_solve(A, B, X0=None):
    X = np.zeros_like(B) if X0 is None else np.array(X0)
    hists, iters, status, rc = A.solve_multi("pcg", B, X)
    return X, hists, iters, status, rc


@pytest.mark.parametrize("name", ["poisson3d", "fem_unstructured"])
def test_columns_do_not_interact(name):
    A = handle(name)
    rng = np.random.default_rng(23)
    B = rng.standard_normal((A.nrow, 5))
    B[:, 1] *= 1e-4
    B[:, 3] = B[:, 0]
    X, hists, iters, status, rc = block_solve(A, B)
    assert rc == 0 and np.all(status == 0)
    assert np.array_equal(X[:, 3], X[:, 0]) and np.array_equal(hists[3], hists[0]) and iters[3] == iters[0]
    # two runs of the same block
    X2, hists2, iters2, _, _ = block_solve(A, B)
    assert np.array_equal(X, X2) and np.array_equal(iters, iters2) and all(np.array_equal(a, b) for a, b in zip(hists, hists2))
    # permutations of the columns (the same width: the partial sums of a reduction are cut by the width, so its last bits are the width's)
    for perm in ([4, 2, 0, 3, 1], [1, 0, 3, 4, 2]):
        Xp, hp, ip, _, _ = block_solve(A, B[:, perm])
        assert np.array_equal(Xp, X[:, perm]), perm
        assert np.array_equal(ip, iters[perm]) and all(np.array_equal(hp[j], hists[c]) for j, c in enumerate(perm)), perm


@pytest.mark.parametrize("nrhs", [1, 3, 8])
def test_block_pcg_head_is_the_numpy_restatement(nrhs):
    A, S = handle("poisson3d"), single("poisson3d")
    A0 = A.level_scipy(0)
    nu = A.params.sweeps
    rng = np.random.default_rng(24)
    B = np.column_stack([np.ones(A.nrow)] + [rng.standard_normal(A.nrow) for _ in range(nrhs - 1)])
    tol = A.params.tol
    A.set_stopping(tol, max_iter=3)
    try:
        X, hists, iters, status, rc = block_solve(A, B)
    finally:
        A.set_stopping(tol, max_iter=sa.default_params().max_iter)
    assert rc == sa.SPARSH_ENOCONV and np.all(status == sa.SPARSH_ENOCONV) and np.all(iters == 3)
    for c in range(nrhs):
        want, href = pcg_ref(A0, lambda r: S.cycle(r, nu), B[:, c], 3)
        assert hists[c][-1] > tol
        assert_history(hists[c], href, np.linalg.norm(B[:, c]))
        assert_solution(X[:, c], want, 1e-9)


def rhs_block(n, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([np.ones(n), rng.standard_normal(n), 1e-3 * rng.standard_normal(n), np.zeros(n)])


@pytest.mark.parametrize("name", ["poisson3d", "c0", "fem_unstructured"])
@pytest.mark.parametrize("nonzero_x0", [False, True])
def test_block_solves_follow_single_solves(name, nonzero_x0):
    A = handle(name)
    n, tol = A.nrow, A.params.tol
    for seed in (31, 32, 33):  # the guard below: no single-solve history entry within 1e-3 of tol, else the next seed
        B = rhs_block(n, seed)
        X0 = np.zeros((n, 4))
        if nonzero_x0:
            X0[:, :3] = 0.1 * np.random.default_rng(seed + 100).standard_normal((n, 3))  # (the zero column keeps x0 = 0)
        singles = []
        for c in range(4):
            x = X0[:, c].copy()
            h, rc = A.solve("pcg", B[:, c], x)
            assert rc == 0
            singles.append((x, h))
        allh = np.concatenate([h for _, h in singles])
        if np.all(np.abs(allh / tol - 1.0) > 1e-3):
            break
    else:
        pytest.fail("every seed leaves a single-solve history entry within 1e-3 of tol")
    X, hists, iters, status, rc = block_solve(A, B, X0)
    assert rc == 0 and np.all(status == 0)
    print(name, "iterations", iters)
    for c in range(4):
        x, h = singles[c]
        assert iters[c] == len(h) and len(hists[c]) == len(h), (c, iters[c], len(h))
        if len(h):
            err = np.abs(hists[c] - h) / h
            print(name, c, "largest relative history difference", err.max())
            assert np.all(err <= hist_tolerance(h)), (c, err.max())
        assert np.abs(X[:, c] - x).max() <= 1e-9 * max(np.abs(x).max(), np.finfo(float).tiny), c
    assert iters[3] == 0 and len(hists[3]) == 0 and np.array_equal(X[:, 3], np.zeros(n))
    # a column that converged before the others keeps, bit for bit, the x it had when it froze: the run capped at that count
    first = int(iters[:3].min())
    assert first < int(iters[:3].max()), iters
    A.set_stopping(tol, max_iter=first)
    try:
        Xc, hc, ic, sc, rcc = block_solve(A, B, X0)
    finally:
        A.set_stopping(tol, max_iter=sa.default_params().max_iter)
    for c in np.flatnonzero(iters[:3] == first):
        assert sc[c] == 0 and ic[c] == first and np.array_equal(Xc[:, c], X[:, c]) and np.array_equal(hc[c], hists[c]), c
    for c in np.flatnonzero(iters[:3] > first):
        assert sc[c] == sa.SPARSH_ENOCONV and ic[c] == first and np.array_equal(hc[c], hists[c][:first]), c
    assert rcc == sa.SPARSH_ENOCONV


def test_check_every_does_not_change_a_column():
    rp, ci, v = INPUTS["poisson3d"]
    B = rhs_block(len(rp) - 1, 31)
    out = []
    for every in (1, 7):
        A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, check_every=every))
        out.append(block_solve(A, B))
        A.close()
    (X1, h1, i1, s1, _), (X7, h7, i7, s7, _) = out
    assert np.array_equal(X1, X7) and np.array_equal(i1, i7) and np.array_equal(s1, s7)
    assert all(np.array_equal(a, b) for a, b in zip(h1, h7))


def test_block_buffers_come_and_go_and_leave_the_single_path_alone():
    rp, ci, v, b = load_c0()
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
    assert A.multi_info() == dict(width=0, bytes=0)
    x0 = np.zeros(A.nrow)
    h0, rc = A.solve("pcg", b, x0)
    assert rc == 0 and A.multi_info() == dict(width=0, bytes=0)
    B = np.column_stack([b, 2.0 * b, -b])
    X, hists, iters, status, rc = block_solve(A, B)
    assert rc == 0
    info4 = A.multi_info()
    assert info4["width"] == 4 and info4["bytes"] > 4 * 8 * 4 * A.nrow  # at least x, x2, r of level 0 and the loop's four blocks
    x1 = np.zeros(A.nrow)
    h1, rc = A.solve("pcg", b, x1)
    assert rc == 0 and np.array_equal(h0, h1) and np.array_equal(x0, x1)
    block_solve(A, B[:, :2])
    info2 = A.multi_info()
    assert info2["width"] == 2 and 0 < info2["bytes"] < info4["bytes"]
    A.op_precond_multi(np.ones((A.nrow, 7)))
    assert A.multi_info()["width"] == 8 and A.multi_info()["bytes"] > info4["bytes"]
    A.setup(sa.default_params(**QUIET))
    assert A.multi_info() == dict(width=0, bytes=0)
    X2, hists2, iters2, _, rc = block_solve(A, B)
    assert rc == 0 and np.array_equal(X, X2) and np.array_equal(iters, iters2)


def test_refusals_on_the_device():
    rp, ci, v = INPUTS["poisson3d"]
    n = len(rp) - 1
    B, X = np.ones((n, 4)), np.zeros((n, 4))
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
    for kind, order in (("sor", "symmetric"), ("chebyshev", "forward")):
        A.set_smoother(kind, 0, order)
        for call in (lambda: A.solve_multi("pcg", B, X), lambda: A.op_precond_multi(B)):
            with pytest.raises(sa.SparshError) as e:
                call()
            assert e.value.code == sa.SPARSH_EINVAL, kind
    A.set_smoother("jacobi")
    assert block_solve(A, B)[4] == 0
    F = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, precond_fp32=1))
    with pytest.raises(sa.SparshError) as e:
        F.solve_multi("pcg", B, X)
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.solve_multi("pcg", np.ones((n, 9)), np.zeros((n, 9)))
    assert e.value.code == sa.SPARSH_EINVAL


def test_bench_op_multi_times_a_block_launch():
    A = handle("poisson3d")
    for op in ("spmv_dot", "jacobi_pingpong_resident"):
        for k in (2, 4, 8):
            t = A.bench_op_multi(op, 0, nrhs=k, reps=5)
            assert 0.0 < t < 1.0, (op, k, t)
