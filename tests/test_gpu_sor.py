"""Multicolour SOR smoother on the device: op_sor against a numpy restatement of its arithmetic contract (bitwise), the two
launch paths against each other, the SOR V-cycle against one composed from the operator entry points, the solvers with SOR
against a CPU restatement, hipGraph replay, and the return to Jacobi on the same handle.  GPU box only.

numpy restatement of one sweep ("Multicolour SOR smoother"): per colour, the rows of that colour at once; the row
sums accumulate column by column over rows padded to one width (a padded slot leaves the sum untouched), so every row adds its
products one by one in stored order, each product rounded first -- every numpy elementwise operation is one IEEE rounding.
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import load_c0
from test_sor_host import unsymmetric_grid

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)


class SorRef:
    """numpy restatement of the SOR sweep of one level (colour classes taken from the handle, checked in test_sor_host)"""

    def __init__(self, A, level):
        rp, ci, v, _ = A.level_csr(level)
        n = len(rp) - 1
        lens = np.diff(rp)
        W = max(int(lens.max()), 1)
        k = np.arange(W)
        on = k[None, :] < lens[:, None]
        idx = np.where(on, rp[:-1, None] + k[None, :], 0)
        pc = np.where(on, ci[np.minimum(idx, len(ci) - 1)], 0)
        pv = np.where(on, v[np.minimum(idx, len(v) - 1)], 0.0)
        d = np.zeros(n)
        rows = np.repeat(np.arange(n), lens)
        first = np.flatnonzero(ci[: len(rows)] == rows)
        d[rows[first][::-1]] = v[first][::-1]  # the first diagonal entry of a row (extract_diagonal)
        _, _, color = A.level_colors(level)
        self.classes = []
        for c in range(1, int(color.max()) + 1):
            r = np.flatnonzero(color == c)
            self.classes.append((r, on[r], pc[r], pv[r], d[r]))
        self.n = n

    def sweep(self, b, x, sweeps, reverse, omega):
        x = np.array(x, dtype=np.float64)
        order = self.classes[::-1] if reverse else self.classes
        for _ in range(sweeps):
            for r, on, pc, pv, d in order:
                s = np.zeros(len(r))
                for k in range(on.shape[1]):
                    s = np.where(on[:, k], s + pv[:, k] * x[pc[:, k]], s)
                h = s - b[r]
                x[r] = x[r] - omega * h / d
        return x


def dense_row_grid(m=60):
    """5-point grid operator plus a dense first row and column (weak couplings, diagonal raised to stay dominant): row 0 holds
    m * m entries, more than one row block's LDS buffer (kStreamNnz = 2048), so the per-colour kernel parks it chunk by chunk"""
    import scipy.sparse as sp

    rp, ci, v = problems.poisson2d(m)
    n = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(n, n)).tolil()
    A[0, 1:] = -1e-3
    A[1:, 0] = -1e-3
    A[0, 0] = A[0, 0] + 1e-3 * n
    A = A.tocsr()
    A.sort_indices()
    assert np.diff(A.indptr).max() > 2048
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def inputs():
    rp, ci, v, _ = load_c0()
    yield "c0", (rp, ci, v)
    yield "poisson2d", problems.poisson2d(120)
    yield "poisson3d", problems.poisson3d(24)
    yield "fem_unstructured", problems.fem_unstructured(20000)
    yield "random_spd", problems.random_spd(6000)
    yield "unsymmetric", unsymmetric_grid()
    yield "dense_row", dense_row_grid()


INPUTS = dict(inputs())


def device_handle(rp, ci, v, **kw):
    return sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, **kw))


@pytest.mark.parametrize("name", list(INPUTS))
def test_op_sor_is_bitwise_the_numpy_restatement(name):
    A = device_handle(*INPUTS[name])
    omega = A.params.omega
    rng = np.random.default_rng(7)
    for l in range(A.nlevels):
        ref = SorRef(A, l)
        b = rng.standard_normal(ref.n)
        x = rng.standard_normal(ref.n)
        for sweeps in (1, 6):
            for reverse in (False, True):
                for zero in (False, True):
                    want = ref.sweep(b, np.zeros(ref.n) if zero else x, sweeps, reverse, omega)
                    got = A.op_sor(l, b, x, sweeps, reverse=reverse, x_is_zero=zero)
                    assert np.array_equal(got, want), (name, l, sweeps, reverse, zero, np.abs(got - want).max())


@pytest.mark.parametrize("name", ["c0", "poisson3d", "unsymmetric", "dense_row"])
def test_single_launch_legs_are_bitwise_the_per_colour_launches(name):
    A = device_handle(*INPUTS[name])
    rng = np.random.default_rng(3)
    for l in range(A.nlevels):
        n = A.level_info(l)["nrow"]
        b, x = rng.standard_normal(n), rng.standard_normal(n)
        for reverse in (False, True):
            A.set_sor_path(1)
            per_colour = A.op_sor(l, b, x, 6, reverse=reverse)
            A.set_sor_path(2)
            single = A.op_sor(l, b, x, 6, reverse=reverse)
            assert np.array_equal(per_colour, single), (l, reverse)
    # whole cycles under the three paths
    A.set_smoother("sor", 0, "symmetric")
    b = rng.standard_normal(A.nrow)
    out = []
    for path in (0, 1, 2):
        A.set_sor_path(path)
        x = np.zeros(A.nrow)
        A.vcycle(b, x, iterations=2)
        out.append(x)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


def composed_cycle(A, b, x, nu, symmetric):
    """One SOR V-cycle from the operator entry points (AMG_solve_SOR, src/AMG_phases.cpp:234-306)."""
    last = A.nlevels - 1
    bs, xs = [b], []
    for l in range(last):
        xl = A.op_sor(l, bs[l], x if l == 0 else np.zeros(len(bs[l])), nu, x_is_zero=l > 0)
        xs.append(xl)
        bs.append(A.op_restrict(l, A.op_residual(l, bs[l], xl)))
    xc = A.op_coarse(bs[last])
    for l in range(last, 0, -1):
        xc = A.op_sor(l - 1, bs[l - 1], A.op_prolong(l - 1, xc, xs[l - 1]), nu, reverse=symmetric)
    return xc


@pytest.mark.parametrize("name", ["c0", "poisson3d"])
@pytest.mark.parametrize("order", ["forward", "symmetric"])
def test_sor_vcycle_is_bitwise_the_composed_cycle(name, order):
    A = device_handle(*INPUTS[name])
    assert A.nlevels >= 3
    A.set_smoother("sor", 0, order)
    rng = np.random.default_rng(11)
    b = rng.standard_normal(A.nrow)
    x = rng.standard_normal(A.nrow)
    want = x.copy()
    for _ in range(2):
        want = composed_cycle(A, b, want, 6, order == "symmetric")
    got = x.copy()
    A.vcycle(b, got, iterations=2)
    assert np.array_equal(got, want)
    # a sweep count of one's own
    A.set_smoother("sor", 2, order)
    got = x.copy()
    A.vcycle(b, got, iterations=1)
    assert np.array_equal(got, composed_cycle(A, b, x, 2, order == "symmetric"))


class CpuSorCycle:
    """numpy / SciPy restatement of the SOR V-cycle (coarse level: sparse LU) for iteration counts"""

    def __init__(self, A, symmetric, nu=6):
        self.L = A.nlevels
        self.A = [A.level_scipy(l).tocsr() for l in range(self.L)]
        self.P = [A.level_scipy(l, "P").tocsr() for l in range(self.L - 1)]
        self.R = [P.T.tocsr() for P in self.P]
        self.sor = [SorRef(A, l) for l in range(self.L - 1)]
        self.lu = spla.splu(self.A[-1].tocsc())
        self.omega = A.params.omega
        self.sym, self.nu = symmetric, nu

    def __call__(self, b, x=None):
        bs, xs = [b], []
        for l in range(self.L - 1):
            xl = x.copy() if (l == 0 and x is not None) else np.zeros(len(bs[l]))
            xl = self.sor[l].sweep(bs[l], xl, self.nu, False, self.omega)
            xs.append(xl)
            bs.append(self.R[l] @ (bs[l] - self.A[l] @ xl))
        xc = self.lu.solve(bs[-1])
        for l in range(self.L - 1, 0, -1):
            xc = self.sor[l - 1].sweep(bs[l - 1], xs[l - 1] + self.P[l - 1] @ xc, self.nu, self.sym, self.omega)
        return xc


def cpu_iterations(method, A0, V, b, tol, cap=500):
    x = np.zeros(len(b))
    if method == "amg":
        it, r1 = 0, np.linalg.norm(b)
        while r1 > tol and it < cap:
            x = V(b, x)
            r1 = np.linalg.norm(b - A0 @ x)
            it += 1
        return it
    if method == "pcg":  # Solver_PCG_1
        r = b - A0 @ x
        z = V(r)
        p, rz, it, res = z.copy(), r @ z, 0, np.linalg.norm(r)
        while res > tol and it < cap:
            Ap = A0 @ p
            alpha = rz / (p @ Ap)
            x = x + alpha * p
            r = r - alpha * Ap
            z = V(r)
            zr = z @ r
            beta, rz = zr / rz, zr
            res = np.linalg.norm(r)
            p = z + beta * p
            it += 1
        return it
    # pbicg: Solver_PBiCG_1
    r0 = b - A0 @ x
    r, p, res, it = r0.copy(), r0.copy(), np.linalg.norm(r0), 0
    while res > tol and it < cap:
        p1 = V(p)
        Ap = A0 @ p1
        alpha1 = r @ r0
        alpha = alpha1 / (Ap @ r0)
        s = r - alpha * Ap
        s1 = V(s)
        As = A0 @ s1
        om = (As @ s) / (As @ As)
        x = x + alpha * p1 + om * s1
        r = s - om * As
        beta = (r @ r0) / alpha1 * (alpha / om)
        res = np.linalg.norm(r)
        p = r + beta * (p - om * Ap)
        it += 1
    return it


@pytest.mark.parametrize("name", ["c0", "poisson3d"])
@pytest.mark.parametrize("method,order", [("amg", "forward"), ("pbicg", "forward"), ("pbicg", "symmetric"), ("pcg", "symmetric")])
def test_solvers_with_sor_reach_tol(name, method, order):
    rp, ci, v = INPUTS[name]
    if name == "c0":
        b = load_c0()[3]
    else:
        b = np.ones(len(rp) - 1)
    A = device_handle(rp, ci, v)
    A.set_smoother("sor", 0, order)
    tol = A.params.tol
    x = np.zeros(A.nrow)
    hist, rc = A.solve(method, b, x)
    assert rc == 0 and hist[-1] <= tol
    A0 = A.level_scipy(0)
    true_res = np.linalg.norm(b - A0 @ x)
    if method == "pcg":
        assert true_res <= 1.001 * tol, true_res
    else:
        assert true_res <= 10 * tol, true_res
    want = cpu_iterations(method, A0, CpuSorCycle(A, order == "symmetric"), b, tol)
    assert abs(len(hist) - want) <= 1, (len(hist), want)


def test_pcg_with_forward_sor_is_refused_on_the_device():
    rp, ci, v = INPUTS["poisson3d"]
    A = device_handle(rp, ci, v)
    A.set_smoother("sor", 0, "forward")
    with pytest.raises(sa.SparshError) as e:
        A.solve("pcg", np.ones(A.nrow), np.zeros(A.nrow))
    assert e.value.code == sa.SPARSH_EINVAL


def test_graph_replay_of_sor_pcg_is_bitwise_the_eager_run():
    rp, ci, v = problems.poisson3d(30)
    n = len(rp) - 1
    b = np.ones(n)
    E = device_handle(rp, ci, v)
    E.set_smoother("sor", 0, "symmetric")
    x0 = np.zeros(n)
    h0, rc = E.solve("pcg", b, x0)
    assert rc == 0
    G = sa.sp_matrix_mg(rp, ci, v)
    G.set_smoother("sor", 0, "symmetric")  # chosen before the setup: layouts built there
    G.setup(sa.default_params(**QUIET, use_graph=1))
    assert G.level_sor_layout(0)["ncolors"] == 2
    for _ in range(2):
        x1 = np.zeros(n)
        h1, rc = G.solve("pcg", b, x1)
        assert rc == 0 and np.array_equal(h0, h1) and np.array_equal(x0, x1)


def test_jacobi_after_sor_is_bitwise_a_fresh_jacobi_handle():
    rp, ci, v, b = load_c0()
    F = device_handle(rp, ci, v)
    A = device_handle(rp, ci, v)
    A.set_smoother("sor", 0, "symmetric")  # chosen after the setup: layouts built at the first solve
    xs = np.zeros(A.nrow)
    hs, _ = A.solve("pcg", b, xs)
    for method in ("pcg", "amg", "pbicg"):
        A.set_smoother("jacobi")
        x1, x2 = np.zeros(A.nrow), np.zeros(A.nrow)
        h1, _ = A.solve(method, b, x1)
        h2, _ = F.solve(method, b, x2)
        assert np.array_equal(h1, h2) and np.array_equal(x1, x2), method
        A.set_smoother("sor", 0, "symmetric")
        h3, _ = A.solve("pcg", b, np.zeros(A.nrow))
        assert np.array_equal(h3, hs)


def test_smoother_change_inside_a_krylov_session():
    """krylov_init under Jacobi, then SOR: the steps check the smoother they now run (forward SOR is refused for PCG before
    anything is launched, the symmetric one builds its layouts first) and equal a session started under SOR"""
    rp, ci, v = problems.poisson3d(24)
    n = len(rp) - 1
    for graph in (0, 1):
        A = device_handle(rp, ci, v, use_graph=graph)
        bd, xd = A.dev_alloc(8 * n), A.dev_alloc(8 * n)
        A.h2d(bd, np.ones(n))
        A.dev_fill(xd, n, 0.0)
        A.krylov_init_dev("pcg", bd, xd)
        A.set_smoother("sor", 0, "forward")
        with pytest.raises(sa.SparshError) as e:
            A.krylov_step_dev(3)
        assert e.value.code == sa.SPARSH_EINVAL
        A.set_smoother("sor", 0, "symmetric")
        A.krylov_step_dev(3)  # layouts built here, at the first SOR step
        assert A.level_sor_layout(0)["ncolors"] == 2
        mixed = A.krylov_history()
        assert len(mixed) == 3 and np.all(np.isfinite(mixed))
        # the same session with the smoother set before the init: its first step differs only through z0 = V(r0)
        A.dev_fill(xd, n, 0.0)
        A.krylov_init_dev("pcg", bd, xd)
        A.krylov_step_dev(3)
        sor_only = A.krylov_history()
        B = device_handle(rp, ci, v, use_graph=graph)
        B.set_smoother("sor", 0, "symmetric")
        hb, _ = B.solve("pcg", np.ones(n), np.zeros(n))
        assert np.array_equal(sor_only, hb[:3])


@pytest.mark.parametrize("sweeps", [3, 0])
def test_jacobi_sweep_count_of_set_smoother_is_params_sweeps(sweeps):
    """set_smoother("jacobi", sweeps) after the setup: bitwise a handle set up with params.sweeps = sweeps (0: the setup's own)"""
    rp, ci, v, b = load_c0()
    A = device_handle(rp, ci, v)
    A.set_smoother("jacobi", sweeps)
    F = device_handle(rp, ci, v, sweeps=sweeps if sweeps > 0 else sa.default_params().sweeps)
    for method in ("pcg", "amg"):
        x1, x2 = np.zeros(A.nrow), np.zeros(A.nrow)
        h1, _ = A.solve(method, b, x1)
        h2, _ = F.solve(method, b, x2)
        assert np.array_equal(h1, h2) and np.array_equal(x1, x2), method
