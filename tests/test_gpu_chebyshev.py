"""Chebyshev polynomial smoother on the device: op_cheby against a numpy restatement of its arithmetic contract (bitwise) on every
kernel family, the Chebyshev V-cycle against one composed from the operator entry points, the fused dot of the last post-smoothing
step, the solvers, hipGraph replay, the return to Jacobi on the same handle, and the refusals.  GPU box only.

numpy restatement of step k of a leg (every numpy elementwise operation is one IEEE rounding):
    s_i = the row's products added one by one in stored order (SorRef's row-padded column-by-column sums)
    h = 1.0*b + (-1.0)*s ; t = (c2_k*h)/diag ; d = t (k = 0) or c1_k*d + t ; x = x + d
with the host coefficients theta = (lmax+lmin)/2, delta = (lmax-lmin)/2, sigma = theta/delta, rho_0 = 1/sigma, c1_0 = 0,
c2_0 = 1/theta, rho_k = 1/(2 sigma - rho_{k-1}), c1_k = rho_k rho_{k-1}, c2_k = 2 rho_k/delta.
"""
import threading

import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import load_c0
from test_gpu_sor import INPUTS, SorRef, device_handle

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
SYMMETRIC = ["c0", "poisson2d", "poisson3d", "fem_unstructured", "random_spd"]


def coefficients(lmax, ratio, degree):
    lmax, ratio = np.float64(lmax), np.float64(ratio)
    lmin = lmax / ratio
    theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = [np.float64(0.0)], [1.0 / theta]
    for _ in range(1, degree):
        rho_k = 1.0 / (2.0 * sigma - rho)
        c1.append(rho_k * rho)
        c2.append(2.0 * rho_k / delta)
        rho = rho_k
    return c1, c2


class ChebRef:
    """numpy restatement of a Chebyshev leg of one level on SorRef's padded rows (one block per colour class).  The column-by-column
    sums visit, at column k, only the rows that still hold an entry there (rows ordered by length): the same additions as under
    SorRef's mask, without 3 600 passes over every row of the dense-row grid."""

    def __init__(self, A, level):
        ref = SorRef(A, level)
        self.n = ref.n
        self.diag = np.zeros(self.n)
        self.blocks = []
        for r, on, pc, pv, d in ref.classes:
            self.diag[r] = d
            order = np.argsort(-on.sum(axis=1), kind="stable")
            self.blocks.append((r, order, on.sum(axis=0), pc, pv))

    def rowsum(self, x):
        s = np.zeros(self.n)
        for r, order, counts, pc, pv in self.blocks:
            sr = np.zeros(len(r))
            for k, c in enumerate(counts):
                if c == 0:
                    break
                a = order[:c]
                sr[a] = sr[a] + pv[a, k] * x[pc[a, k]]
            s[r] = sr
        return s

    def leg(self, b, x, degree, lmax, ratio=30.0):
        c1, c2 = coefficients(lmax, ratio, degree)
        x = np.array(x, dtype=np.float64)
        d = None
        for k in range(degree):
            h = 1.0 * b + (-1.0) * self.rowsum(x)
            t = (c2[k] * h) / self.diag
            d = t if k == 0 else c1[k] * d + t
            x = x + d
        return x


@pytest.mark.parametrize("name", list(INPUTS))
def test_op_cheby_is_bitwise_the_numpy_restatement(name):
    A = device_handle(*INPUTS[name])
    rng = np.random.default_rng(7)
    for l in range(A.nlevels):  # (the coarsest level too: the dense-row grid has no other)
        ref = ChebRef(A, l)
        b = rng.standard_normal(ref.n)
        x = rng.standard_normal(ref.n)
        for forced in (0.0, 2.75):
            A.set_chebyshev_lmax(l, forced)
            lmax = A.level_chebyshev(l)["lmax"]
            assert forced == 0.0 or lmax == forced
            for degree in (1, 2, 4, 7):
                for zero in (False, True):
                    want = ref.leg(b, np.zeros(ref.n) if zero else x, degree, lmax)
                    got = A.op_cheby(l, b, x, degree, x_is_zero=zero)
                    assert np.array_equal(got, want), (name, l, forced, degree, zero, np.abs(got - want).max())
    # another ratio, and degree 0 = nothing
    A.set_chebyshev(ratio=8.0)
    ref = ChebRef(A, 0)
    b, x = rng.standard_normal(ref.n), rng.standard_normal(ref.n)
    assert np.array_equal(A.op_cheby(0, b, x, 5), ref.leg(b, x, 5, A.level_chebyshev(0)["lmax"], 8.0))
    assert np.array_equal(A.op_cheby(0, b, x, 0), x)
    with pytest.raises(sa.SparshError) as e:
        A.op_cheby(A.nlevels, np.zeros(1), np.zeros(1), 2)
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.op_cheby(0, b, x, 17)
    assert e.value.code == sa.SPARSH_EINVAL


FAMILIES = [(0, 0), (0, 1), (0, 2), (0, 4), (1, 0), (1, 1), (2, 3), (3, 3)]


@pytest.mark.parametrize("name", ["poisson3d", "fem_unstructured", "poisson3d_42", "poisson3d_42_general"])
def test_every_kernel_family_gives_the_same_bits(name):
    """poisson3d(42): 74 088 rows, the smallest cube whose finest level takes the LDS-tiled table kernel (>= 65 536 rows) and, with
    the constant-slot folding off (the layout of a variable-coefficient operator: no stencil table), sdia_kernel instead of the
    sliced-ELL kernel small levels prefer.  The FEM input is ragged: it has the CSR-stream layouts only."""
    rp, ci, v = problems.poisson3d(42) if name.startswith("poisson3d_42") else INPUTS[name]
    A = sa.sp_matrix_mg(rp, ci, v)
    A.set_index_compression(2)
    if name.endswith("_general"):
        A.set_const_slots(False)
    A.setup(sa.default_params(**QUIET))
    rng = np.random.default_rng(5)
    ref = ChebRef(A, 0)
    b, x = rng.standard_normal(ref.n), rng.standard_normal(ref.n)
    lmax = A.level_chebyshev(0)["lmax"]
    want = {(deg, zero): ref.leg(b, np.zeros(ref.n) if zero else x, deg, lmax) for deg in (2, 5) for zero in (False, True)}
    coarse = {}
    kernels = set()
    for kind, vec in FAMILIES:
        for tile in (False, True):
            for alt in (1, 2):
                for nt, remap in ((-1, -1), (1, 16)):
                    if (tile and kind != 3) or (nt == 1 and alt == 2):
                        continue
                    A.set_kernel_config(kind, vec, nt, remap).set_tile(tile).set_alternate_sweeps(alt)
                    kernels.add((A.level_kernel(0), A.level_tile_rows(0) > 0))
                    for (deg, zero), w in want.items():
                        got = A.op_cheby(0, b, x, deg, x_is_zero=zero)
                        assert np.array_equal(got, w), (kind, vec, tile, alt, nt, deg, zero, np.abs(got - w).max())
                    for l in range(1, A.nlevels - 1):  # the coarser levels: every family against the first one
                        nl = A.level_info(l)["nrow"]
                        bl, xl = b[:nl], x[:nl]
                        got = A.op_cheby(l, bl, xl, 3)
                        assert np.array_equal(got, coarse.setdefault(l, got)), (l, kind, vec, tile, alt, nt)
    print(name, sorted(kernels))
    names = {k for k, _ in kernels}
    assert {"csr_block_kernel", "csr_wave_kernel", "csr_rowlane_kernel", "csr_rowlane16_kernel"} <= names, names
    if name.endswith("_general"):
        assert {"sell_kernel", "sdia_kernel"} <= names, names
    elif name != "fem_unstructured":
        assert {"sell_kernel", "sdia_tab_kernel"} <= names, names
    if name == "poisson3d_42":
        assert ("sdia_tab_kernel", True) in kernels, kernels


def composed_cycle(A, b, x, degree, x_is_zero=False):
    """One Chebyshev V-cycle from the operator entry points: the Jacobi cycle's order of operations"""
    last = A.nlevels - 1
    bs, xs = [b], []
    for l in range(last):
        zero = l > 0 or x_is_zero
        xl = A.op_cheby(l, bs[l], x if l == 0 else np.zeros(len(bs[l])), degree, x_is_zero=zero)
        xs.append(xl)
        bs.append(A.op_restrict(l, A.op_residual(l, bs[l], xl)))
    xc = A.op_coarse(bs[last])
    for l in range(last, 0, -1):
        xc = A.op_cheby(l - 1, bs[l - 1], A.op_prolong(l - 1, xc, xs[l - 1]), degree)
    return xc


@pytest.mark.parametrize("name", ["c0", "poisson3d", "unsymmetric"])
def test_cheby_vcycle_and_op_precond_are_bitwise_the_composed_cycle(name):
    A = device_handle(*INPUTS[name])
    assert A.nlevels >= (2 if name == "unsymmetric" else 3)  # (the unsymmetric grid coarsens to two levels)
    rng = np.random.default_rng(11)
    b = rng.standard_normal(A.nrow)
    x = rng.standard_normal(A.nrow)
    for degree in (0, 3):  # 0: the default of 4
        A.set_smoother("chebyshev", degree)
        m = degree or 4
        got = x.copy()
        A.vcycle(b, got, iterations=1)
        assert np.array_equal(got, composed_cycle(A, b, x, m)), degree
        assert np.array_equal(A.op_precond(b), composed_cycle(A, b, np.zeros(A.nrow), m, x_is_zero=True)), degree
    want = x.copy()
    for _ in range(2):
        want = composed_cycle(A, b, want, 3)
    got = x.copy()
    A.vcycle(b, got, iterations=2)
    assert np.array_equal(got, want)


def true_residual(A, b, x):
    return np.linalg.norm(b - A.level_scipy(0) @ x)


def test_fused_dot_of_the_last_post_smoothing_step():
    """OP_CHEBY_DOT has no switch of its own, so z.r is read off the iterate.  From x_0 = 0 the first PCG step leaves
    x_1 = alpha_0 z_0 with alpha_0 = (z_0.r_0) / (p_0.A p_0), z_0 = p_0 = M b: the numerator is the fused sum of the cycle's last
    post-smoothing step, the denominator the SpMV's fused sum, and z_0 is known bitwise from op_precond (the same cycle with a plain
    last step).  Both reductions are held to the project's 1e-12 against numpy, so alpha_0 to 2e-12 plus the few roundings of the
    quotient and of the fit: 2.5e-12.  Later steps: the iterate against the numpy recurrence with the device's preconditioner,
    to 1e-9 (rounding differences of the dots carried through four steps; a wrong z.r changes beta and the iterate in the
    leading digits)."""
    rp, ci, v = INPUTS["poisson3d"]
    A0 = None
    for degree in (4, 1):  # degree 1: the fused step is step 0 of its leg (no previous correction)
        A = device_handle(rp, ci, v)
        A.set_smoother("chebyshev", degree)
        n = A.nrow
        A0 = A.level_scipy(0)
        b = np.random.default_rng(3).standard_normal(n)
        bd, xd = A.dev_alloc(8 * n), A.dev_alloc(8 * n)
        A.h2d(bd, b)
        A.dev_fill(xd, n, 0.0)
        A.krylov_init_dev("pcg", bd, xd)
        A.krylov_step_dev(1)
        x1 = np.zeros(n)
        A.d2h(x1, xd)
        z0 = A.op_precond(b)
        alpha_dev = (x1 @ z0) / (z0 @ z0)
        alpha_np = (z0 @ b) / (z0 @ (A0 @ z0))
        print("degree", degree, "alpha_0 device", alpha_dev, "numpy", alpha_np, "relative", abs(alpha_dev - alpha_np) / abs(alpha_np))
        assert np.allclose(x1, alpha_dev * z0, rtol=1e-13, atol=1e-13 * np.abs(x1).max())  # x_1 is a multiple of z_0
        assert abs(alpha_dev - alpha_np) <= 2.5e-12 * abs(alpha_np)
        A.krylov_step_dev(3)
        xdev = np.zeros(n)
        A.d2h(xdev, xd)
        x, r = np.zeros(n), b.copy()
        z = A.op_precond(r)
        p, rz = z.copy(), r @ z
        for k in range(4):
            Ap = A0 @ p
            alpha = rz / (p @ Ap)
            x = x + alpha * p
            r = r - alpha * Ap
            z = A.op_precond(r)
            zr = z @ r
            beta, rz = zr / rz, zr
            p = z + beta * p
        err = np.linalg.norm(xdev - x) / np.linalg.norm(x)
        print("degree", degree, "iterate after 4 steps against the numpy recurrence", err)
        assert err <= 1e-9


@pytest.mark.parametrize("name", SYMMETRIC)
@pytest.mark.parametrize("method", ["amg", "pcg", "pbicg", "pgmres"])
def test_solvers_with_chebyshev_reach_tol(name, method):
    rp, ci, v = INPUTS[name]
    b = load_c0()[3] if name == "c0" else np.ones(len(rp) - 1)
    A = device_handle(rp, ci, v)
    A.set_smoother("chebyshev")
    tol = A.params.tol
    x = np.zeros(A.nrow)
    hist, rc = A.solve(method, b, x)
    res = true_residual(A, b, x)
    print(name, method, "iterations", len(hist), "true residual", res)
    assert rc == 0 and hist[-1] <= tol
    assert res <= (1.001 if method in ("pcg", "pgmres") else 10) * tol, res


def test_pgmres_with_chebyshev_on_the_unsymmetric_grid():
    rp, ci, v = INPUTS["unsymmetric"]
    A = device_handle(rp, ci, v)
    A.set_smoother("chebyshev")
    b = np.ones(A.nrow)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("pgmres", b, x)
    res = true_residual(A, b, x)
    print("unsymmetric pgmres iterations", len(hist), "true residual", res)
    assert rc == 0 and res <= 1.001 * A.params.tol


@pytest.mark.parametrize("name,model", [("poisson3d", (8, 11)), ("fem_unstructured", (60, 73))])
def test_pcg_iterations_are_no_more_than_with_as_many_jacobi_sweeps(name, model):
    rp, ci, v = INPUTS[name]
    b = np.ones(len(rp) - 1)
    A = device_handle(rp, ci, v, max_levels=6)
    A.set_smoother("chebyshev", 6)
    hc, rc = A.solve("pcg", b, np.zeros(A.nrow))
    assert rc == 0
    A.set_smoother("jacobi", sweeps=6)
    hj, rc = A.solve("pcg", b, np.zeros(A.nrow))
    assert rc == 0
    print(name, "PCG iterations: Chebyshev degree 6", len(hc), "Jacobi 6 sweeps", len(hj), "CPU model", model)
    assert len(hc) <= len(hj)


def test_graph_replay_of_chebyshev_pcg_is_bitwise_the_eager_run():
    rp, ci, v = problems.poisson3d(30)
    n = len(rp) - 1
    b = np.ones(n)
    E = device_handle(rp, ci, v)
    E.set_smoother("chebyshev")
    x0 = np.zeros(n)
    h0, rc = E.solve("pcg", b, x0)
    assert rc == 0
    G = sa.sp_matrix_mg(rp, ci, v)
    G.set_smoother("chebyshev")  # chosen before the setup: bounds and d vectors made there
    G.setup(sa.default_params(**QUIET, use_graph=1))
    for _ in range(2):
        x1 = np.zeros(n)
        h1, rc = G.solve("pcg", b, x1)
        assert rc == 0 and np.array_equal(h0, h1) and np.array_equal(x0, x1)
    # new coefficients: the captured iteration is dropped, not replayed
    G.set_chebyshev(ratio=10.0)
    E.set_chebyshev(ratio=10.0)
    x0, x1 = np.zeros(n), np.zeros(n)
    h0, _ = E.solve("pcg", b, x0)
    h1, _ = G.solve("pcg", b, x1)
    assert np.array_equal(h0, h1) and np.array_equal(x0, x1)


def test_jacobi_after_chebyshev_is_bitwise_a_fresh_jacobi_handle():
    rp, ci, v, b = load_c0()
    F = device_handle(rp, ci, v)
    A = device_handle(rp, ci, v)
    A.set_smoother("chebyshev")  # chosen after the setup: bounds and d vectors made at the first solve
    hs, _ = A.solve("pcg", b, np.zeros(A.nrow))
    for method in ("pcg", "amg", "pbicg"):
        A.set_smoother("jacobi")
        x1, x2 = np.zeros(A.nrow), np.zeros(A.nrow)
        h1, _ = A.solve(method, b, x1)
        h2, _ = F.solve(method, b, x2)
        assert np.array_equal(h1, h2) and np.array_equal(x1, x2), method
        A.set_smoother("chebyshev")
        h3, _ = A.solve("pcg", b, np.zeros(A.nrow))
        assert np.array_equal(h3, hs)


def test_smoother_change_inside_a_krylov_session():
    """krylov_init under Jacobi, then Chebyshev: the steps build the bounds and d vectors they now need and go on; a session started
    under Chebyshev equals the one-call solve"""
    rp, ci, v = problems.poisson3d(24)
    n = len(rp) - 1
    for graph in (0, 1):
        A = device_handle(rp, ci, v, use_graph=graph)
        bd, xd = A.dev_alloc(8 * n), A.dev_alloc(8 * n)
        A.h2d(bd, np.ones(n))
        A.dev_fill(xd, n, 0.0)
        A.krylov_init_dev("pcg", bd, xd)
        A.krylov_step_dev(2)
        A.set_smoother("chebyshev")
        A.krylov_step_dev(3)
        mixed = A.krylov_history()
        assert len(mixed) == 5 and np.all(np.isfinite(mixed)) and mixed[-1] < mixed[0]
        A.dev_fill(xd, n, 0.0)
        A.krylov_init_dev("pcg", bd, xd)
        A.krylov_step_dev(3)
        cheb_only = A.krylov_history()
        B = device_handle(rp, ci, v, use_graph=graph)
        B.set_smoother("chebyshev")
        hb, _ = B.solve("pcg", np.ones(n), np.zeros(n))
        assert np.array_equal(cheb_only, hb[:3])


def test_partitioned_handle_refuses_chebyshev():
    """two ranks on the in-process transport: refused when selected, before and after the setup; Jacobi goes on working"""
    rp, ci, v = problems.poisson3d(24)
    n = len(rp) - 1
    G = 2
    group = sa.comm_group_create(G)
    out, errs = [None] * G, []

    def work(r):
        try:
            A = sa.sp_matrix_mg(rp, ci, v)
            A.comm_init_group(group, r)
            codes = []
            for when in ("before", "after"):
                try:
                    A.set_smoother("chebyshev")
                    codes.append(0)
                except sa.SparshError as e:
                    codes.append(e.code)
                if when == "before":
                    A.setup(sa.default_params(**QUIET, replicate_rows=1000))
            lo, hi, rep = A.local_range(0)
            x = np.zeros(hi - lo)
            h, rc = A.solve("pcg", np.ones(hi - lo), x)
            out[r] = (codes, rep, rc)
            A.close()
        except Exception as e:  # noqa: BLE001
            errs.append((r, repr(e)))

    ts = [threading.Thread(target=work, args=(r,)) for r in range(G)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "a virtual rank hung"
    assert not errs, errs
    sa.comm_group_destroy(group)
    for codes, rep, rc in out:
        assert codes == [sa.SPARSH_EINVAL, sa.SPARSH_EINVAL] and not rep and rc == 0
    assert n == 13824


def test_second_setup_rebuilds_the_chebyshev_state():
    rp, ci, v = INPUTS["poisson3d"]
    b = np.ones(len(rp) - 1)
    A = sa.sp_matrix_mg(rp, ci, v)
    A.set_smoother("chebyshev", 5)
    runs = []
    for _ in range(3):
        A.setup(sa.default_params(**QUIET))
        x = np.zeros(A.nrow)
        h, rc = A.solve("pcg", b, x)
        assert rc == 0
        runs.append((h, x, [A.level_chebyshev(l) for l in range(A.nlevels - 1)]))
    for h, x, c in runs[1:]:
        assert np.array_equal(h, runs[0][0]) and np.array_equal(x, runs[0][1]) and c == runs[0][2]
    # a forced bound belongs to the setup it was given to
    A.set_chebyshev_lmax(0, 2.5)
    A.setup(sa.default_params(**QUIET))
    assert A.level_chebyshev(0) == runs[0][2][0]


def test_bench_op_runs_one_step_and_leaves_the_handle_clean():
    rp, ci, v = INPUTS["poisson3d"]
    A = device_handle(rp, ci, v)
    b = np.ones(A.nrow)
    x0 = np.zeros(A.nrow)
    h0, _ = A.solve("pcg", b, x0)
    for l in range(A.nlevels):
        assert A.bench_op("chebyshev_pingpong_resident", l, reps=3) > 0.0
    x1 = np.zeros(A.nrow)
    h1, _ = A.solve("pcg", b, x1)
    assert np.array_equal(h0, h1) and np.array_equal(x0, x1)
