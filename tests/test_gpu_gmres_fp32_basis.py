"""Restarted GMRES with the basis stored as float (sparsh_set_gmres_basis(SPARSH_BASIS_FP32)) against a numpy
restatement of the same algorithm: fp64 arithmetic, the device's own preconditioner (op_precond) and level-0 operator (op_spmv),
and astype(np.float32) at exactly the points where the device rounds -- every v_k as it is stored; the orthogonalisation, the
Hessenberg column, V y and the input of M / A all use the stored vectors.  Device and restatement differ in the order of the
additions inside a dot product only, which can flip the last bit of a stored float.  GPU box only.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from test_gpu_gmres import INPUTS as BASE_INPUTS, QUIET, TOL, true_residual

pytestmark = pytest.mark.gpu

# Largest relative difference between the device's history and the restatement's over the entries above 1e-6 r0, measured on one
# MI355X per input and restart length (all of them in DESIGN.md section 5d).  Restart 30: 1.7e-15 at the most.  Restart 5, where
# the reduction orders meet again in every cycle's true residual: c0 7.9e-11, poisson3d 2.1e-11, convdiff 2.1e-10, poisson3d(7, 7, 6)
# without preconditioner 6.7e-11 and, the loosest of all, poisson2d(9) without preconditioner 7.02e-8 (78 iterations, 16 cycles).
# No bound can be derived in advance -- a flipped last bit of a stored float moves the continuation of the history -- so the
# assertion is ten times the loosest measured value, the margin for other reduction orders on another box, for every input.
HIST_RTOL = 10 * 7.02e-8


def small_inputs():
    ones = lambda t: t + (np.ones(len(t[0]) - 1),)
    yield "poisson2d_37", ones(problems.poisson2d(37))    # 1369 rows: odd, n % 4 = 1
    yield "poisson3d_776", ones(problems.poisson3d(7, 7, 6))  # 294 rows: n % 4 = 2, less than one workgroup's span
    yield "poisson2d_9", ones(problems.poisson2d(9))      # 81 rows: n % 4 = 1, less than one workgroup


INPUTS = dict(BASE_INPUTS, **dict(small_inputs()))


def device_handle(name, basis="fp32", **kw):
    rp, ci, v, b = INPUTS[name]
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, **kw))
    if basis is not None:
        A.set_gmres(basis=basis)
    return A, b


def gmres_ref_f32(spmv, M, b, x0, m, tol=TOL, cap=100000):
    """(x, history, initial true residual) of right-preconditioned GMRES(m) with the basis stored as float; M = None: none"""
    if M is None:
        M = lambda v: v
    n = len(b)
    x = np.array(x0, dtype=np.float64)
    hist, it, r0 = [], 0, None
    while True:
        r = b - spmv(x)
        beta = np.linalg.norm(r)
        if r0 is None:
            r0 = beta
        if beta <= tol or it >= cap:
            break
        V = np.zeros((m + 1, n), dtype=np.float32)
        V[0] = (r / beta).astype(np.float32)
        g = np.zeros(m + 1)
        g[0] = beta
        R = np.zeros((m, m))
        cs, sn = np.zeros(m), np.zeros(m)
        k = 0
        for j in range(m):
            if it >= cap:
                break
            Vj = V[: j + 1].astype(np.float64)  # the vectors as stored
            w = spmv(M(Vj[j]))
            h = Vj @ w
            w = w - Vj.T @ h
            c = Vj @ w
            w = w - Vj.T @ c
            col = np.append(h + c, np.linalg.norm(w))
            V[j + 1] = (w / col[j + 1]).astype(np.float32) if col[j + 1] > 0 else 0.0
            for i in range(j):
                col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], cs[i] * col[i + 1] - sn[i] * col[i]
            d = np.hypot(col[j], col[j + 1])
            cs[j], sn[j] = (col[j] / d, col[j + 1] / d) if d != 0 else (1.0, 0.0)
            R[: j + 1, j] = col[: j + 1]
            R[j, j] = cs[j] * col[j] + sn[j] * col[j + 1]
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            hist.append(abs(g[j + 1]))
            it += 1
            k = j + 1
            if abs(g[j + 1]) <= tol:
                break
        y = sla.solve_triangular(R[:k, :k], g[:k])
        x = x + M(V[:k].astype(np.float64).T @ y)
    return x, np.array(hist), r0


def history_difference(hist, ref, r0):
    """largest relative difference over the common entries above 1e-6 r0"""
    k = min(len(hist), len(ref))
    keep = ref[:k] >= 1e-6 * r0
    if not keep.any():
        return 0.0
    return float((np.abs(hist[:k] - ref[:k]) / ref[:k])[keep].max())


CASES = [(name, "pgmres") for name in ("c0", "poisson3d", "convdiff", "unsymmetric", "poisson2d_37", "poisson3d_776", "poisson2d_9")]
CASES += [("poisson3d_776", "gmres"), ("poisson2d_9", "gmres")]


@pytest.mark.parametrize("restart", [30, 5])
@pytest.mark.parametrize("name,method", CASES)
def test_history_is_the_numpy_restatement(name, method, restart):
    A, b = device_handle(name)
    A.set_gmres(restart)
    assert A.gmres_info() == dict(restart=restart, basis_bytes=0, basis="fp32")
    spmv = lambda v: A.op_spmv(0, v)
    _, href, r0 = gmres_ref_f32(spmv, A.op_precond if method == "pgmres" else None, b, np.zeros(A.nrow), restart)
    x = np.zeros(A.nrow)
    hist, rc = A.solve(method, b, x)
    diff = history_difference(hist, href, r0)
    print(f"{name} {method} restart {restart}: iterations {len(hist)} reference {len(href)} largest relative history difference {diff:.3e}")
    assert rc == 0
    assert abs(len(hist) - len(href)) <= 1, (len(hist), len(href))
    assert true_residual(A.level_scipy(0), b, x) <= 1.001 * TOL
    assert diff <= HIST_RTOL, diff


def test_fp64_basis_is_untouched():
    """fp64 set explicitly, never set, and set after an fp32 solve on the same handle: bitwise the same histories and solutions"""
    out = []
    for name in ("convdiff", "poisson2d_37"):
        for basis in (None, "fp64", "fp32"):
            A, b = device_handle(name, basis=basis)
            x = np.zeros(A.nrow)
            if basis == "fp32":
                h32, rc = A.solve("pgmres", b, x)
                assert rc == 0 and A.gmres_info()["basis_bytes"] > 0
                A.set_gmres(30, basis="fp64")
                assert A.gmres_info() == dict(restart=30, basis_bytes=0)  # the float basis is gone
                x = np.zeros(A.nrow)
            hist, rc = A.solve("pgmres", b, x)
            assert rc == 0 and A.gmres_basis() == "fp64"
            out.append((hist, x, A.gmres_info()["basis_bytes"]))
        (h0, x0, n0), (h1, x1, n1), (h2, x2, n2) = out[-3:]
        assert np.array_equal(h0, h1) and np.array_equal(x0, x1) and n0 == n1
        assert np.array_equal(h0, h2) and np.array_equal(x0, x2) and n0 == n2
        assert not np.array_equal(h0[: len(h32)], h32[: len(h0)])  # (the float basis did run: its history is another one)


def test_determinism():
    A, b = device_handle("c0")
    x1, x2 = np.zeros(A.nrow), np.zeros(A.nrow)
    h1, rc1 = A.solve("pgmres", b, x1)
    held = A.gmres_info()["basis_bytes"]
    h2, rc2 = A.solve("pgmres", b, x2)
    assert rc1 == 0 and rc2 == 0
    assert np.array_equal(h1, h2) and np.array_equal(x1, x2)
    assert A.gmres_info()["basis_bytes"] == held  # the basis stays between solves
    A.set_gmres(30, basis="fp32")  # unchanged: it stays
    assert A.gmres_info()["basis_bytes"] == held


def gs_grid(n):
    return min(max((n + 511) // 512, 1), 2048)


@pytest.mark.parametrize("name", ["poisson3d", "poisson2d_37"])
def test_memory(name):
    """(m + 1) vectors of n rounded up to 4 floats, (m + 1) * gs_grid(n) partial sums, one fp64 vector of n
    rounded up to 4 doubles"""
    m = 30
    held = {}
    for basis in ("fp32", "fp64"):
        A, b = device_handle(name, basis=basis)
        _, rc = A.solve("pgmres", b, np.zeros(A.nrow))
        assert rc == 0
        held[basis] = A.gmres_info()["basis_bytes"]
    n = A.nrow
    part = (m + 1) * gs_grid(n) * 8
    stride4, stride2 = (n + 3) // 4 * 4, (n + 1) // 2 * 2
    print(name, "bytes held", held, "ratio", held["fp32"] / held["fp64"])
    assert held["fp32"] == (m + 1) * stride4 * 4 + part + stride4 * 8
    assert held["fp64"] == (m + 1) * stride2 * 8 + part
    if name == "poisson3d":
        assert held["fp32"] < 0.6 * held["fp64"]


def test_long_run_across_many_restarts():
    """fem_unstructured(20000), restart 30: several restart cycles, so only convergence and the iteration count are compared, and the
    restatement is the reference for the count.  Measured on the MI355X: 160 iterations with the float basis, the restatement 160
    (the fp64 basis: 160)."""
    A, b = device_handle("fem")
    spmv = lambda v: A.op_spmv(0, v)
    _, href, _ = gmres_ref_f32(spmv, A.op_precond, b, np.zeros(A.nrow), 30)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("pgmres", b, x)
    print("fem: iterations", len(hist), "reference", len(href))
    assert rc == 0
    assert true_residual(A.level_scipy(0), b, x) <= 1.001 * TOL
    assert abs(len(hist) - len(href)) <= 1, (len(hist), len(href))


def test_lucky_breakdown():
    """The eigenvector is no float vector: v_0 as stored carries 6e-8 of other eigenvectors, no h_{j+1} vanishes, and GMRES(10)
    without a preconditioner works that remainder off -- 104 iterations on the MI355X where the fp64 basis takes 4.  Finite, rc 0."""
    m = 40
    rp, ci, v = problems.poisson2d(m)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
    s = np.sin(np.pi * np.arange(1, m + 1) / (m + 1))
    b = np.outer(s, s).ravel()  # the lowest eigenvector: the Krylov space is exhausted after one step
    A.set_gmres(10, basis="fp32")
    A.set_stopping(TOL, 0, 4)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("gmres", b, x)
    print("history", hist)
    assert rc == 0 and np.all(np.isfinite(x)) and np.all(np.isfinite(hist))
    assert true_residual(A.level_scipy(0), b, x) <= 1.001 * TOL


@pytest.mark.parametrize("precond", ["sor_forward", "fp32"])
def test_other_preconditioners(precond):
    A, b = device_handle("poisson3d", **(dict(precond_fp32=1) if precond == "fp32" else {}))
    if precond != "fp32":
        A.set_smoother("sor", 0, precond[4:])
    spmv = lambda v: A.op_spmv(0, v)
    _, href, _ = gmres_ref_f32(spmv, A.op_precond, b, np.zeros(A.nrow), 30)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("pgmres", b, x)
    print(precond, "iterations", len(hist), "reference", len(href))
    assert rc == 0
    assert true_residual(A.level_scipy(0), b, x) <= 1.001 * TOL
    assert abs(len(hist) - len(href)) <= 1, (len(hist), len(href))


def test_bench_ops_follow_the_precision_of_the_handle():
    A, _ = device_handle("poisson2d_37")
    assert A.bench_op("gmres_orth_fp32_basis", 0, 2) > 0
    assert A.gmres_info()["basis_bytes"] > 0
    with pytest.raises(sa.SparshError) as e:
        A.bench_op("gmres_orth", 0, 2)
    assert e.value.code == sa.SPARSH_ESTATE
    A.set_gmres(basis="fp64")
    assert A.bench_op("gmres_orth", 0, 2) > 0
    with pytest.raises(sa.SparshError) as e:
        A.bench_op("gmres_orth_fp32_basis", 0, 2)
    assert e.value.code == sa.SPARSH_ESTATE
    with pytest.raises(sa.SparshError) as e:
        A.bench_op("gmres_orth_fp32_basis", 1, 2)
    assert e.value.code == sa.SPARSH_EINVAL
