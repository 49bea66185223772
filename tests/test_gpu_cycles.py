"""W- and K-cycles at chosen levels and flexible CG on the device: the K step against numpy, the W- and the
K-cycle against the recursion restated in Python from the operator entry points (bitwise), SPARSH_FCG against SPARSH_PCG and on the
K-cycle, the refusals and the handle's state.  GPU box only.

The recursion, with legs = the handle's smoother through op_jacobi / op_sor / op_cheby:
    cycle(l, b):        l last: coarse solve.  else x = pre-leg(b) ; b_c = R (b - A x) ; x += P solve_coarse(l + 1, b_c) ; x = post-leg(b, x)
    solve_coarse(l, b): plain level: cycle(l, b).   W: c = cycle(l, b) ; d = cycle(l, b - A c) ; c + d.
                        K: c = cycle(l, b) ; r = b - q A c ; d = cycle(l, r) ; k1 c + k2 d   (the K step: sparsh_op_kstep)
"""
import math
import threading

import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from test_gpu_sor import INPUTS, device_handle

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
DEEP = dict(limit_upper=300, limit_lower=150)  # 14 000 rows coarsen to the full six levels, so that strides 1 and 2 both recurse


def true_residual(A, b, x):
    return np.linalg.norm(b - A.level_scipy(0) @ x)


def tridiagonal(n):
    """tridiag(-1, 2, -1) of n rows"""
    rows = np.arange(n)
    cols = np.stack([rows - 1, rows, rows + 1], axis=1)
    vals = np.tile(np.array([-1.0, 2.0, -1.0]), (n, 1))
    keep = (cols >= 0) & (cols < n)
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return rp, cols[keep].astype(np.int32), vals[keep].astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- 1. the K step

def usable(v):
    return bool(np.isfinite(v) and v > 0.0)


def scalars_from_dots(rho1, alpha1, gamma, beta, alpha2):
    """q, rho2, k1, k2 of the contract from the five sums, every operation one rounding, with the two guards"""
    rho1, alpha1, gamma, beta, alpha2 = (np.float64(t) for t in (rho1, alpha1, gamma, beta, alpha2))
    if not usable(rho1):
        return np.float64(1.0), np.float64(0.0), np.float64(1.0), np.float64(1.0)
    q = alpha1 / rho1
    rho2 = beta - (gamma * gamma) / rho1
    if not usable(rho2):
        return q, rho2, q, np.float64(0.0)
    return q, rho2, q - (gamma * alpha2) / (rho1 * rho2), alpha2 / rho2


def close(a, b, rtol):
    return abs(a - b) <= rtol * abs(b) or (a == b)


def check_kstep(A, level, b, c, d, tag):
    n = len(b)
    zero = np.zeros(n)
    v = A.op_spmv(level, c)
    w = A.op_spmv(level, d)
    # d = 0: gamma = beta = alpha2 = 0, rho2 = 0 is not > 0, so k1 = q and k2 = 0 -- the device's own q
    r0, x0, s0 = A.op_kstep(level, b, c, zero)
    assert not np.isnan(r0).any() and not np.isnan(x0).any() and not np.isnan(s0).any(), tag
    q_dev = s0[6]
    assert s0[7] == 0.0 and np.array_equal(s0[2:5], np.zeros(3)), (tag, s0)
    assert np.array_equal(x0, q_dev * c + 0.0 * zero), tag  # x = q c
    r, x, s = A.op_kstep(level, b, c, d)
    r2, x2, s2 = A.op_kstep(level, b, c, d)
    assert np.array_equal(r, r2) and np.array_equal(x, x2) and np.array_equal(s, s2), tag  # run-to-run reproducible
    assert np.array_equal(r, r0) and np.array_equal(s[:2], s0[:2]), tag                   # the first half does not depend on d
    want = [math.fsum(c * v), math.fsum(c * b), math.fsum(d * v), math.fsum(d * w), math.fsum(d * r)]
    worst = max(abs(s[k] - want[k]) / abs(want[k]) if want[k] != 0.0 else abs(s[k]) for k in range(5))
    q, rho2, k1, k2 = scalars_from_dots(*s[:5])
    print(tag, "rows", n, "worst relative deviation of the five sums from fsum", worst, "scalars", s)
    for k in range(5):
        assert close(s[k], want[k], 1e-12), (tag, k, s[k], want[k])
    assert close(q_dev, q, 1e-14) and close(s[5], rho2, 1e-14) and close(s[6], k1, 1e-14) and close(s[7], k2, 1e-14), (tag, s, q, rho2, k1, k2)
    assert np.array_equal(r, b - q_dev * v), tag            # r_i = b_i - q v_i on the device's own q
    assert np.array_equal(x, s[6] * c + s[7] * d), tag      # x_i = k1 c_i + k2 d_i on the device's own k1, k2
    assert not np.isnan(r).any() and not np.isnan(x).any(), tag
    # c = 0: rho1 = 0 is not > 0, the W step: q = k1 = k2 = 1, r = b - A 0 = b, x = 0 + d
    rz, xz, sz = A.op_kstep(level, b, zero, d)
    assert sz[0] == 0.0 and sz[5] == 0.0 and sz[6] == 1.0 and sz[7] == 1.0, (tag, sz)
    assert np.array_equal(rz, b - 1.0 * A.op_spmv(level, zero)) and np.array_equal(xz, 1.0 * zero + 1.0 * d), tag
    assert not np.isnan(rz).any() and not np.isnan(xz).any() and not np.isnan(sz).any(), tag


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_kstep_on_single_level_handles(n):
    """sizes around the wave (64 lanes) and the workgroup (256 threads, two rows per thread and pass) of the reducing launches, odd
    and even tails; the handle is the tridiagonal matrix alone, its one level the "coarsest" """
    A = device_handle(*tridiagonal(n), max_levels=1)
    assert A.nlevels == 1
    rng = np.random.default_rng(100 + n)
    b, c, d = (rng.standard_normal(n) for _ in range(3))
    check_kstep(A, 0, b, c, d, f"tridiagonal({n})")


def test_kstep_across_workgroups():
    """4 100 rows: three workgroups of the reducing launches, the last one partly filled, and an even / odd tail"""
    for n in (4100, 4099):
        A = device_handle(*tridiagonal(n), max_levels=1)
        rng = np.random.default_rng(n)
        b, c, d = (rng.standard_normal(n) for _ in range(3))
        check_kstep(A, 0, b, c, d, f"tridiagonal({n})")


@pytest.mark.parametrize("name", ["c0", "poisson3d"])
def test_kstep_on_every_level(name):
    A = device_handle(*INPUTS[name], **DEEP)
    rng = np.random.default_rng(5)
    for l in range(A.nlevels):
        n = A.level_info(l)["nrow"]
        b, c, d = (rng.standard_normal(n) for _ in range(3))
        check_kstep(A, l, b, c, d, f"{name} level {l}")
    with pytest.raises(sa.SparshError) as e:
        A.op_kstep(A.nlevels, np.zeros(1), np.zeros(1), np.zeros(1))
    assert e.value.code == sa.SPARSH_EINVAL


# ---------------------------------------------------------------------------------------------------- 2. / 3. the recursive cycles

class Recursion:
    """cycle / solve_coarse of the contract from the operator entry points of a handle"""

    def __init__(self, A, kind, stride, smoother, count, symmetric=False):
        self.A, self.kind, self.stride = A, kind, stride
        self.smoother, self.count, self.symmetric = smoother, count, symmetric
        self.last = A.nlevels - 1
        self.steps = 0

    def wk(self, l):
        return self.kind != "v" and 1 <= l < self.last and l % self.stride == 0

    def leg(self, l, b, x, zero, post):
        if self.smoother == "jacobi":
            return self.A.op_jacobi(l, b, x, self.count, x_is_zero=zero)
        if self.smoother == "sor":
            return self.A.op_sor(l, b, x, self.count, reverse=post and self.symmetric, x_is_zero=zero)
        return self.A.op_cheby(l, b, x, self.count, x_is_zero=zero)

    def cycle(self, l, b, x=None):
        A = self.A
        if l == self.last:
            return A.op_coarse(b)
        zero = x is None
        x = self.leg(l, b, np.zeros(len(b)) if zero else x, zero, False)
        bc = A.op_restrict(l, A.op_residual(l, b, x))
        x = A.op_prolong(l, self.solve_coarse(l + 1, bc), x)
        return self.leg(l, b, x, False, True)

    def solve_coarse(self, l, b):
        if not self.wk(l):
            return self.cycle(l, b)
        A = self.A
        self.steps += 1
        c = self.cycle(l, b)
        if self.kind == "w":
            d = self.cycle(l, A.op_residual(l, b, c))
            return c + d
        r, _, _ = A.op_kstep(l, b, c, np.zeros(len(b)))  # d = 0: the first half of the step, r = b - q A c
        d = self.cycle(l, r)
        _, x, _ = A.op_kstep(l, b, c, d)
        return x


SMOOTHERS = [("jacobi", 2, "forward"), ("sor", 2, "forward"), ("sor", 2, "symmetric"), ("chebyshev", 3, "forward")]


@pytest.mark.parametrize("name", ["c0", "poisson3d", "unsymmetric"])
def test_w_cycle_is_bitwise_the_recursion(name):
    A = device_handle(*INPUTS[name], **DEEP)
    assert A.nlevels >= (2 if name == "unsymmetric" else 5), A.nlevels
    rng = np.random.default_rng(21)
    b, x = rng.standard_normal(A.nrow), rng.standard_normal(A.nrow)
    for smoother, count, order in (SMOOTHERS[0], SMOOTHERS[2], SMOOTHERS[3]):
        A.set_smoother(smoother, count, order)
        for stride in (1, 2):
            A.set_cycle("w", stride)
            ref = Recursion(A, "w", stride, smoother, count, order == "symmetric")
            got = x.copy()
            A.vcycle(b, got, iterations=1)
            assert np.array_equal(got, ref.cycle(0, b, x)), (smoother, stride)
            assert np.array_equal(A.op_precond(b), ref.cycle(0, b)), (smoother, stride)
            assert ref.steps == 2 * (2 ** A.cycle_info()["nlevels_wk"] - 1), (ref.steps, A.cycle_info())
            assert [ref.wk(l) for l in range(A.nlevels)] == [A.level_cycle(l)[0] for l in range(A.nlevels)]
    assert A.cycle_info()["bytes"] > 0


@pytest.mark.parametrize("name", ["c0", "poisson3d"])
def test_k_cycle_is_bitwise_the_recursion(name):
    A = device_handle(*INPUTS[name], **DEEP)
    assert A.nlevels >= 5, A.nlevels
    rng = np.random.default_rng(22)
    b, x = rng.standard_normal(A.nrow), rng.standard_normal(A.nrow)
    for smoother, count, order in (SMOOTHERS[0], SMOOTHERS[3]):
        A.set_smoother(smoother, count, order)
        for stride in (1, 2):
            A.set_cycle("k", stride)
            ref = Recursion(A, "k", stride, smoother, count)
            z = A.op_precond(b)
            assert np.array_equal(z, ref.cycle(0, b)), (smoother, stride)
            assert np.array_equal(z, A.op_precond(b))  # run to run
            got = x.copy()
            A.vcycle(b, got, iterations=1)
            assert np.array_equal(got, ref.cycle(0, b, x)), (smoother, stride)


# ------------------------------------------------------------------------------------------------------------------- 4. flexible CG

def test_fcg_with_the_v_cycle_follows_pcg():
    """FCG(1) is PCG in exact arithmetic under a fixed symmetric M: the histories agree to 1e-8 over their whole length (the band
    test_gpu_parity gives histories whose reductions are ordered differently; the CPU model deviates by 2e-12), the counts by at most 1"""
    rp, ci, v = INPUTS["poisson3d"]
    b = np.ones(len(rp) - 1)
    for smoother in ("jacobi", "chebyshev"):
        A = device_handle(rp, ci, v)
        A.set_smoother(smoother)
        xp, xf = np.zeros(A.nrow), np.zeros(A.nrow)
        hp, rcp = A.solve("pcg", b, xp)
        hf, rcf = A.solve("fcg", b, xf)
        m = min(len(hp), len(hf))
        dev = np.abs(hf[:m] - hp[:m]) / hp[:m]
        print(smoother, "pcg", len(hp), "fcg", len(hf), "largest relative deviation of the histories", dev.max())
        assert rcp == 0 and rcf == 0
        assert abs(len(hf) - len(hp)) <= 1
        assert dev.max() <= 1e-8
        assert true_residual(A, b, xf) <= 1.001 * A.params.tol


@pytest.fixture(scope="module")
def grid48():
    """poisson3d(48), b = 1, the default 6 levels, two Jacobi sweeps per leg; the V-cycle PCG count every comparison below is against"""
    rp, ci, v = problems.poisson3d(48)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, sweeps=2))
    assert A.nlevels == 6
    b = np.ones(A.nrow)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("pcg", b, x)
    assert rc == 0
    return A, b, len(hist)


def test_fcg_on_the_k_cycle_needs_fewer_iterations_than_pcg_on_the_v_cycle(grid48):
    A, b, n_v = grid48
    A.set_cycle("k", 3)
    try:
        x = np.zeros(A.nrow)
        hist, rc = A.solve("fcg", b, x)
        res = true_residual(A, b, x)
        print("poisson3d(48), sweeps 2: PCG + V", n_v, "iterations; FCG + K(stride 3)", len(hist), "(model: 20 and 16); true residual", res)
        assert rc == 0
        assert res <= 1.001 * A.params.tol
        assert len(hist) < n_v
    finally:
        A.set_cycle("v")


def test_w_cycle_under_pcg_pbicg_pgmres(grid48):
    A, b, n_v = grid48
    A.set_cycle("w", 2)
    try:
        counts = {}
        for method in ("pcg", "pbicg", "pgmres"):
            x = np.zeros(A.nrow)
            hist, rc = A.solve(method, b, x)
            res = true_residual(A, b, x)
            counts[method] = len(hist)
            print("poisson3d(48), sweeps 2, W(stride 2):", method, len(hist), "iterations, true residual", res)
            assert rc == 0 and hist[-1] <= A.params.tol
            assert res <= (1.001 if method != "pbicg" else 10) * A.params.tol
        print("PCG + V", n_v, "PCG + W(stride 2)", counts["pcg"], "(model: 20 and 16)")
        assert counts["pcg"] < n_v
    finally:
        A.set_cycle("v")


# ------------------------------------------------------------------------------------------------------------ 5. refusals and state

def refused(call):
    with pytest.raises(sa.SparshError) as e:
        call()
    assert e.value.code == sa.SPARSH_EINVAL, e.value
    return str(e.value)


def test_k_cycle_refusals_on_the_device():
    A = device_handle(*INPUTS["poisson3d"], **DEEP)
    b, x = np.ones(A.nrow), np.zeros(A.nrow)
    A.set_cycle("k", 2)
    for method in ("pcg", "pbicg", "pgmres"):
        assert "SPARSH_FCG" in refused(lambda: A.solve(method, b, x)), method
    assert np.array_equal(x, np.zeros(A.nrow))
    hist, rc = A.solve("fcg", b, x)
    assert rc == 0 and true_residual(A, b, x) <= 1.001 * A.params.tol
    x = np.zeros(A.nrow)
    hist, rc = A.solve("amg", b, x)  # the stand-alone iteration takes K
    assert rc == 0 and true_residual(A, b, x) <= 1.001 * A.params.tol
    # block solves
    assert "SPARSH_CYCLE_V" in refused(lambda: A.solve_multi("pcg", np.ones((A.nrow, 2)), np.zeros((A.nrow, 2))))
    A.set_cycle("w", 2)
    assert "SPARSH_CYCLE_V" in refused(lambda: A.solve_multi("pcg", np.ones((A.nrow, 2)), np.zeros((A.nrow, 2))))
    # the stepwise calls: not for SPARSH_FCG, and a K-cycle selected inside a PCG session is refused at the next step
    bd, xd = A.dev_alloc(8 * A.nrow), A.dev_alloc(8 * A.nrow)
    A.h2d(bd, b)
    A.dev_fill(xd, A.nrow, 0.0)
    refused(lambda: A.krylov_init_dev("fcg", bd, xd))
    A.krylov_init_dev("pcg", bd, xd)  # W: accepted
    A.krylov_step_dev(2)
    A.set_cycle("k", 2)
    assert "SPARSH_FCG" in refused(lambda: A.krylov_step_dev(1))
    A.dev_free(bd)
    A.dev_free(xd)


@pytest.mark.parametrize("kind", ["w", "k"])
def test_fp32_preconditioner_refuses_w_and_k(kind):
    A = device_handle(*INPUTS["poisson3d"], precond_fp32=1)
    b, x = np.ones(A.nrow), np.zeros(A.nrow)
    A.set_cycle(kind, 1)
    assert "precond_fp32" in refused(lambda: A.solve("fcg", b, x))
    assert "precond_fp32" in refused(lambda: A.op_precond(b))
    A.set_cycle("v")
    hist, rc = A.solve("fcg", b, x)  # FCG takes the fp32 preconditioner under the V-cycle
    assert rc == 0 and true_residual(A, b, x) <= 1.001 * A.params.tol


def test_partitioned_handle_refuses_w_and_k():
    """two ranks on the in-process transport: W and K are refused at the solve, before any collective step; the V-cycle goes on working"""
    rp, ci, v = problems.poisson3d(24)
    G = 2
    group = sa.comm_group_create(G)
    out, errs = [None] * G, []

    def work(r):
        try:
            A = sa.sp_matrix_mg(rp, ci, v)
            A.comm_init_group(group, r)
            A.setup(sa.default_params(**QUIET, replicate_rows=1000))
            lo, hi, rep = A.local_range(0)
            codes = []
            for kind, method in (("w", "pcg"), ("k", "fcg"), ("w", "pbicg"), ("v", "fcg")):
                A.set_cycle(kind, 1)
                try:
                    A.solve(method, np.ones(hi - lo), np.zeros(hi - lo))
                    codes.append(0)
                except sa.SparshError as e:
                    codes.append(e.code)
            A.set_cycle("v")
            h, rc = A.solve("pcg", np.ones(hi - lo), np.zeros(hi - lo))
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
        assert codes == [sa.SPARSH_EINVAL] * 4 and not rep and rc == 0


def test_v_after_k_is_bitwise_a_fresh_handle():
    rp, ci, v = INPUTS["poisson3d"]
    b = np.ones(len(rp) - 1)
    fresh = device_handle(rp, ci, v, **DEEP)
    x0 = np.zeros(fresh.nrow)
    h0, _ = fresh.solve("pcg", b, x0)
    c0 = np.random.default_rng(1).standard_normal(fresh.nrow)
    fresh.vcycle(b, c0, iterations=2)
    A = device_handle(rp, ci, v, **DEEP)
    for kind in ("k", "w"):
        A.set_cycle(kind, 1)
        A.solve("fcg", b, np.zeros(A.nrow))
        A.set_cycle("v")
        x1 = np.zeros(A.nrow)
        h1, _ = A.solve("pcg", b, x1)
        assert np.array_equal(h1, h0) and np.array_equal(x1, x0), kind
        c1 = np.random.default_rng(1).standard_normal(A.nrow)
        A.vcycle(b, c1, iterations=2)
        assert np.array_equal(c1, c0), kind


def test_buffers_are_rebuilt_by_a_second_setup_and_a_smoother_change_is_honoured():
    rp, ci, v = INPUTS["poisson3d"]
    A = device_handle(rp, ci, v, **DEEP)
    rng = np.random.default_rng(8)
    b = rng.standard_normal(A.nrow)
    A.set_cycle("k", 2)
    assert A.cycle_info()["bytes"] == 0  # nothing until first use
    A.set_smoother("jacobi", 2)
    z1 = A.op_precond(b)
    held = A.cycle_info()["bytes"]
    rows = sum(A.level_info(l)["nrow"] for l in range(A.nlevels) if A.level_cycle(l)[0])
    assert held >= 3 * 8 * rows and held <= 3 * 8 * rows + 8 * (3 * 512 + 16 * (A.nlevels + 1)), (held, rows)
    assert np.array_equal(z1, Recursion(A, "k", 2, "jacobi", 2).cycle(0, b))
    A.set_smoother("chebyshev", 3)  # between two applications: the next one smooths with it
    z2 = A.op_precond(b)
    assert np.array_equal(z2, Recursion(A, "k", 2, "chebyshev", 3).cycle(0, b)) and not np.array_equal(z1, z2)
    assert A.cycle_info()["bytes"] == held
    A.setup(sa.default_params(**QUIET, **DEEP))  # the second setup frees the buffers with the hierarchy
    info = A.cycle_info()
    assert info["bytes"] == 0 and info["kind"] == "k" and info["stride"] == 2
    assert np.array_equal(A.op_precond(b), z2)  # (the smoother and the cycle of the handle stand)
    assert A.cycle_info()["bytes"] == held
    A.set_cycle("w", 2)  # W needs no third vector: nothing more is allocated
    A.op_precond(b)
    assert A.cycle_info()["bytes"] == held
