"""Constant null space (SPARSH_NULLSPACE_CONSTANT) on the device: the projection kernels, the pinned coarsest solve in its three
forms, and every solver on pure Neumann Poisson problems against a scipy restatement of the projected AMG-PCG.  GPU box only.

Bounds.  Means and dots: the first-order bound of any summation order, n u mean|terms| with u = 2^-53 for the mean (one rounding
per addition) and 2^-52 for the dot (a product and an addition per term) -- derived, not measured.  Histories: the rule of
test_gpu_parity.py (1e-6 relative while r_k >= 1e-6 r_0).  True residual: the 1.5 tol band of test_gpu_configs.py.  Error:
||x - xt|| <= ||r|| / lambda_min with lambda_min = 2 - 2 cos(pi / 24), the smallest nonzero eigenvalue along the longest axis."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
LIMITS = dict(limit_upper=300, limit_lower=100)
TOL = 1e-8
OMEGA = 0.66667
# The projection kernels take one pair of elements per thread and pass on a grid of at most 2048 workgroups of 256 threads: one grid
# stride is 2048 * 256 pairs = 1 048 576 elements.  524289 + 3 is the size at which launch_dot starts its second pass (one pass here);
# 1048577 is the first size with an element behind a full stride (offset 0: the odd tail; offset 1: the head in front of it), and
# 2 * 1048576 + 5 and 3 * 1048576 + 2 run the loop's second, third and the start of its fourth pass.
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 1000, 4097, 70001, 524289 + 3, 1048577, 2 * 1048576 + 5, 3 * 1048576 + 2]
GRIDS = [(12, 10, 9), (24, 20, 18)]
LAMBDA_MIN = 2.0 - 2.0 * math.cos(math.pi / 24.0)


@pytest.fixture(scope="module")
def hooks():
    """any ready handle: the projection hooks use its stream only"""
    A = sa.sp_matrix_mg(*problems.poisson3d(6)).setup(sa.default_params(**QUIET))
    yield A
    A.close()


# ------------------------------------------------------------------------------------------------ kernels

@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES + [1024, 65536, 1 << 20, 1 << 22])
def test_project_integer_data_is_exact(hooks, n, offset):
    """small integers: every partial sum is an integer below 2^53, so any order of additions gives the same sum; with a
    power-of-two n the mean is exact too and everything is bitwise numpy's"""
    rng = np.random.default_rng(n)
    x = rng.integers(-8, 9, n).astype(np.float64)
    r = rng.integers(-4, 5, n).astype(np.float64)
    if n & (n - 1) == 0:
        x[0] += n * 3 - x.sum()  # the mean is the integer 3
    m = x.sum() / n  # exact sum; one correctly rounded division, as on the device
    out, mean = hooks.op_project(x, offset)
    assert mean == m and np.array_equal(out, x - m)
    out, mean, dot = hooks.op_project_dot(x, r, offset)
    assert mean == m and np.array_equal(out, x - m)
    if n & (n - 1) == 0:
        assert dot == float(np.sum((x - m) * r))  # integers: exact
    # r on the other alignment than x
    out2, mean2, dot2 = hooks.op_project_dot(x, r, offset, 1 - offset)
    assert mean2 == m and np.array_equal(out2, out)
    if n & (n - 1) == 0:
        assert dot2 == dot


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_project_normal_data(hooks, n, offset):
    rng = np.random.default_rng(1000 + n)
    x = rng.standard_normal(n) + 0.25
    r = rng.standard_normal(n)
    out, mean, dot = hooks.op_project_dot(x, r, offset)
    assert abs(mean - math.fsum(x) / n) <= n * 2.0 ** -53 * np.mean(np.abs(x))
    assert np.array_equal(out, x - mean)
    terms = (x - mean) * r
    assert abs(dot - math.fsum(terms)) <= n * 2.0 ** -52 * np.mean(np.abs(terms))
    out_b, mean_b, dot_b = hooks.op_project_dot(x, r, offset)
    assert mean_b == mean and dot_b == dot and np.array_equal(out_b, out)  # no atomics: bitwise reproducible
    out_p, mean_p = hooks.op_project(x, offset)
    assert mean_p == mean and np.array_equal(out_p, out)  # the launch without the dot removes the same mean
    # r on the other alignment than x: the same vector, and a dot inside the same bound (r is then read as scalars, same order)
    out_r, mean_r, dot_r = hooks.op_project_dot(x, r, offset, 1 - offset)
    assert mean_r == mean and np.array_equal(out_r, out) and dot_r == dot


def test_project_hooks_refuse_bad_arguments(hooks):
    assert sa.lib.sparsh_op_project(hooks._h, 0, None, None) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_op_project_dot(hooks._h, 4, None, None, None, None) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_op_project_dev(hooks._h, -1, None, None, None, None) == sa.SPARSH_EINVAL


# ------------------------------------------------------------------------------------------------ coarsest solve

def pinned_csc(AL):
    n = AL.shape[0]
    keep = sp.diags(np.r_[np.ones(n - 1), 0.0])
    last = sp.csr_matrix(([1.0], ([n - 1], [n - 1])), shape=(n, n))
    return (keep @ AL @ keep + last).tocsc()


@pytest.mark.parametrize("form", ["dense", "nd", "bt"])
def test_coarse_solve_is_the_pinned_solve(form):
    rp, ci, v = problems.poisson3d_neumann(24, 20, 18)
    A = sa.sp_matrix_mg(rp, ci, v).set_nullspace("constant")
    kw = {}
    if form != "dense":
        kw["dense_limit"] = 100
        A.set_coarse_form(form)
    A.setup(sa.default_params(**QUIET, limit_upper=500, **kw))
    try:
        info = A.coarse_info()
        assert info["dense"] == (form == "dense")
        if form != "dense":
            assert info["form"] == ("nested_dissection" if form == "nd" else "block_tridiagonal")
        AL = A.level_scipy(A.nlevels - 1)
        n = AL.shape[0]
        assert A.nullspace_info()["pinned_row"] == n - 1
        lu = spla.splu(pinned_csc(AL))
        rng = np.random.default_rng(5)
        for b in (np.ones(n), rng.standard_normal(n)):
            x, xr = A.op_coarse(b), lu.solve(b)
            assert np.linalg.norm(x - xr) <= 1e-10 * np.linalg.norm(xr), form
            assert abs(x[n - 1] - b[n - 1]) <= 1e-10 * np.linalg.norm(xr)  # the unit row
    finally:
        A.close()


# ------------------------------------------------------------------------------------------------ the scipy restatement

def hem(A, level):
    """heavy-edge matching of the host setup, as in tools/cycle_model.py"""
    n = A.shape[0]
    rp, ci, v = A.indptr, A.indices, np.abs(A.data)
    agg = -np.ones(n, dtype=np.int64)
    nxt = 0
    for i in (range(n) if level % 2 == 0 else range(n - 1, -1, -1)):
        if agg[i] != -1:
            continue
        mate, best = -1, 0.0
        for j in range(rp[i], rp[i + 1]):
            c = ci[j]
            if c != i and agg[c] == -1 and v[j] > best:
                best, mate = v[j], c
        if mate >= 0:
            agg[i] = agg[mate] = nxt
            nxt += 1
    for i in range(n):
        if agg[i] == -1:
            agg[i] = nxt
            nxt += 1
    return sp.csr_matrix((np.ones(n), agg, np.arange(n + 1)), shape=(n, nxt))


class Model:
    """Galerkin hierarchy, weighted-Jacobi V(nu,nu) from a zero guess, pinned splu, PCG with the three projections"""

    def __init__(self, A0, limit_upper=300, limit_lower=100, max_levels=6):
        self.A, self.P = [A0.tocsr()], []
        while len(self.A) < max_levels and self.A[-1].shape[0] > limit_upper:
            a = self.A[-1]
            a.sort_indices()
            p = hem(a, len(self.A) - 1)
            self.P.append(p)
            self.A.append((p.T @ a @ p).tocsr())
            if self.A[-1].shape[0] < limit_lower:
                break
        self.D = [a.diagonal() for a in self.A]
        self.lu = spla.splu(pinned_csc(self.A[-1]))

    def cycle(self, l, b, nu):
        if l == len(self.A) - 1:
            return self.lu.solve(b)
        A, D = self.A[l], self.D[l]
        x = OMEGA * b / D
        for _ in range(nu - 1):
            x = x + OMEGA * (b - A @ x) / D
        x = x + self.P[l] @ self.cycle(l + 1, self.P[l].T @ (b - A @ x), nu)
        for _ in range(nu):
            x = x + OMEGA * (b - A @ x) / D
        return x

    def pcg(self, b, nu, cap=200):
        A = self.A[0]
        proj = lambda w: w - w.mean()  # noqa: E731
        b = proj(b)
        x = np.zeros_like(b)
        r = b - A @ x
        z = proj(self.cycle(0, r, nu))
        p, rho = z.copy(), z @ r
        hist = []
        while len(hist) < cap:
            q = A @ p
            alpha = rho / (p @ q)
            x += alpha * p
            r -= alpha * q
            hist.append(np.linalg.norm(r))
            if hist[-1] <= TOL:
                break
            z = proj(self.cycle(0, r, nu))
            rho_new = z @ r
            p = z + (rho_new / rho) * p
            rho = rho_new
        return proj(x), np.array(hist)


class Case:
    def __init__(self, dims):
        rp, ci, v = problems.poisson3d_neumann(*dims)
        self.n = len(rp) - 1
        self.S = sp.csr_matrix((v, ci, rp), shape=(self.n, self.n))
        self.A = sa.sp_matrix_mg(rp, ci, v).set_nullspace("constant").setup(sa.default_params(**QUIET, **LIMITS, tol=TOL))
        self.model = Model(self.S)
        xt = np.random.default_rng(sum(dims)).standard_normal(self.n)
        self.xt = xt - xt.mean()
        self.b = self.S @ self.xt
        self.model_runs = {}

    def model_pcg(self, nu):
        if nu not in self.model_runs:
            self.model_runs[nu] = self.model.pcg(self.b, nu)
        return self.model_runs[nu]

    def reset(self, nu=7):
        self.A.set_smoother("jacobi", nu).set_cycle("v")

    def check_solution(self, x, b, what):
        bp = b - b.mean()
        res = np.linalg.norm(bp - self.S @ x)
        err = np.abs(x - self.xt).max()
        print(f"{what}: true residual {res:.3e}, |mean x| {abs(x.mean()):.3e}, max error {err:.3e}")
        assert res <= 1.5 * TOL, what
        assert abs(x.mean()) <= self.n * 2.0 ** -52 * np.abs(x).max(), what
        assert err <= TOL / LAMBDA_MIN, what


@pytest.fixture(scope="module", params=GRIDS, ids=lambda d: "x".join(map(str, d)))
def case(request):
    c = Case(request.param)
    yield c
    c.A.close()


def history_rule(h, ho):
    k = min(len(h), len(ho))
    head = ho[:k] >= 1e-6 * ho[0]
    return np.all(np.abs(h[:k] - ho[:k])[head] <= 1e-6 * ho[:k][head])


def test_hierarchy_is_the_models(case):
    A, M = case.A, case.model
    assert [A.level_info(l)["nrow"] for l in range(A.nlevels)] == [a.shape[0] for a in M.A]
    assert A.level_info(A.nlevels - 1)["nrow"] == 270 and A.nullspace_info()["pinned_row"] == 269
    for l in range(A.nlevels - 1):
        assert abs(A.level_scipy(l, "P") - M.P[l]).max() == 0


@pytest.mark.parametrize("nu", [7, 2])
def test_pcg_follows_the_restatement(case, nu):
    case.reset(nu)
    xm, hm = case.model_pcg(nu)
    runs = []
    for shift in (0.0, 0.3):
        b = case.b + shift
        b_in = b.copy()
        x = np.zeros(case.n)
        h, rc = case.A.solve("pcg", b, x)
        print(f"nu = {nu}, b + {shift}: {len(h)} iterations (restatement {len(hm)}), last residuals {h[-1]:.3e} / {hm[-1]:.3e}")
        assert rc == sa.SPARSH_OK
        assert abs(len(h) - len(hm)) <= 1
        assert history_rule(h, hm)
        assert np.array_equal(b, b_in)
        case.check_solution(x, b, f"pcg nu={nu} shift={shift}")
        assert np.abs(x - xm).max() <= 2 * TOL / LAMBDA_MIN
        runs.append((h, x))
    (h0, x0), (h1, x1) = runs
    assert abs(len(h0) - len(h1)) <= 1 and history_rule(h1, h0)
    assert np.abs(x0 - x1).max() <= 2 * TOL / LAMBDA_MIN
    case.reset()


SMOOTHERS = [("jacobi", 0, "forward"), ("sor", 0, "symmetric"), ("chebyshev", 0, "forward")]


# (cg takes no preconditioner: one smoother is all there is to run)
SOLVES = [(m, s) for m in ("amg", "cg", "pcg", "pbicg", "pgmres", "fcg") for s in SMOOTHERS if m != "cg" or s[0] == "jacobi"]


@pytest.mark.parametrize("shift", [0.0, 0.3])
@pytest.mark.parametrize("method,smoother", SOLVES, ids=lambda v: v if isinstance(v, str) else v[0])
def test_every_solver_returns_the_mean_free_solution(case, method, smoother, shift):
    case.A.set_smoother(*smoother).set_cycle("v")
    b = case.b + shift
    b_in = b.copy()
    x = np.zeros(case.n)
    h, rc = case.A.solve(method, b, x)
    assert rc == sa.SPARSH_OK, (method, smoother, len(h))
    assert np.array_equal(b, b_in)
    case.check_solution(x, b, f"{method} {smoother[0]} shift={shift} ({len(h)} iterations)")
    case.reset()


@pytest.mark.parametrize("smoother", SMOOTHERS, ids=lambda s: s[0])
def test_fcg_on_the_k_cycle(case, smoother):
    case.A.set_smoother(*smoother).set_cycle("k", 2)
    for shift in (0.0, 0.3):
        b = case.b + shift
        x = np.full(case.n, 0.5)  # a guess that is all null space
        h, rc = case.A.solve("fcg", b, x)
        assert rc == sa.SPARSH_OK
        case.check_solution(x, b, f"fcg K/2 {smoother[0]} shift={shift} ({len(h)} iterations)")
    case.reset()


def test_precond_returns_the_projected_z(case):
    case.reset()
    r = case.b
    z = case.A.op_precond(r)
    zm = case.model.cycle(0, r, 7)
    zm = zm - zm.mean()
    assert abs(z.mean()) <= case.n * 2.0 ** -52 * np.abs(z).max()
    # one linear operator evaluated twice in fp64; the coarsest solves differ by the 1e-10 of test_coarse_solve_is_the_pinned_solve
    assert np.linalg.norm(z - zm) <= 1e-10 * np.linalg.norm(zm)


def test_stepwise_path_and_untouched_b(case):
    case.reset()
    A, n = case.A, case.n
    b = case.b + 0.3
    bd, xd = A.dev_alloc(n * 8), A.dev_alloc(n * 8)
    try:
        def run(stepper):
            A.h2d(bd, b)
            A.h2d(xd, np.zeros(n))
            out = stepper()
            x, b_back = np.empty(n), np.empty(n)
            A.d2h(x, xd)
            A.d2h(b_back, bd)
            assert np.array_equal(b_back, b)  # the caller's b is never written
            return out, x

        (h, iters, _, rc), x_solve = run(lambda: A.solve_dev("pcg", bd, xd))
        assert rc == sa.SPARSH_OK and iters == len(h)
        case.check_solution(x_solve, b, "solve_dev pcg")

        def one_call():
            A.krylov_init_dev("pcg", bd, xd)
            return A.krylov_step_dev(10000)

        (done, res), x_one = run(one_call)
        assert done == iters and res <= TOL
        assert np.array_equal(x_one, x_solve)  # the same launches
        assert np.array_equal(A.krylov_history(), h)

        def chunks():
            A.krylov_init_dev("pcg", bd, xd)
            total = calls = 0
            for _ in range(100):
                done, res = A.krylov_step_dev(4)  # every return projects x once more
                total += done
                calls += 1
                if res <= TOL:
                    break
            return total, calls, res

        (total, calls, res), x_chunks = run(chunks)
        assert total == iters and res <= TOL
        case.check_solution(x_chunks, b, "stepwise pcg in chunks of 4")
        # the same iterates up to the constants the extra projections remove, each at most the rounding of a mean
        assert np.abs(x_chunks - x_solve).max() <= calls * n * 2.0 ** -52 * np.abs(x_solve).max()

        # the stand-alone iteration on device vectors
        (hv, nv, _, rcv), x_v = run(lambda: A.solve_dev("amg", bd, xd))
        assert rcv == sa.SPARSH_OK and nv == len(hv)
        case.check_solution(x_v, b, "amg on device vectors")
    finally:
        A.dev_free(bd)
        A.dev_free(xd)


def test_use_graph_is_accepted_and_ignored():
    rp, ci, v = problems.poisson3d_neumann(12, 10, 9)
    S = sp.csr_matrix((v, ci, rp))
    xt = np.random.default_rng(3).standard_normal(S.shape[0])
    b = S @ (xt - xt.mean())
    res = []
    for g in (0, 1):
        A = sa.sp_matrix_mg(rp, ci, v).set_nullspace("constant").setup(sa.default_params(**QUIET, **LIMITS, use_graph=g))
        x = np.zeros_like(b)
        h, rc = A.solve("pcg", b, x)
        assert rc == sa.SPARSH_OK
        res.append((h, x))
        A.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------------ off means off

def test_off_means_off():
    rp, ci, v = problems.poisson3d(16)
    n = len(rp) - 1
    b = np.random.default_rng(11).standard_normal(n)

    def plain():
        A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
        assert A.nullspace_info()["kind"] == "none"
        x = np.zeros(n)
        h, rc = A.solve("pcg", b, x)
        A.close()
        assert rc == sa.SPARSH_OK
        return h, x

    h0, x0 = plain()
    rn, cn, vn = problems.poisson3d_neumann(12, 10, 9)
    N = sa.sp_matrix_mg(rn, cn, vn).set_nullspace("constant").setup(sa.default_params(**QUIET, **LIMITS))
    assert N.nullspace_info()["kind"] == "constant"
    xn = np.zeros(len(rn) - 1)
    _, rc = N.solve("pcg", np.arange(len(rn) - 1, dtype=np.float64), xn)
    assert rc == sa.SPARSH_OK
    h1, x1 = plain()
    assert np.array_equal(h0, h1) and np.array_equal(x0, x1)
    # a second setup of the same handle under NONE
    N.set_nullspace("none").setup(sa.default_params(**QUIET, **LIMITS))
    assert N.nullspace_info() == dict(kind="none", pinned_row=-1, row_defect=0.0, col_defect=0.0)
    N.close()
