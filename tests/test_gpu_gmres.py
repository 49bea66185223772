"""Restarted GMRES on the device (SPARSH_GMRES, SPARSH_PGMRES) against a numpy restatement of the same algorithm that applies
the device's own preconditioner (op_precond) and the level-0 operator as SciPy holds it.  GPU box only.

The restatement: right preconditioning, classical Gram-Schmidt twice, Givens rotations, the recurrence
residual |g_{j+1}| as history entry, a true residual at the start of every restart cycle.  It differs from the device in the
order of the additions inside a dot product only.
"""
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import ROOT, hist_tolerance, load_c0
from test_gpu_sor import composed_cycle
from test_sor_host import unsymmetric_grid

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
LIB_DIR = os.path.join(ROOT, "sparsh_amg_amd")
TOL = 1e-8


def convdiff(m=96):
    """5-point diffusion plus first-order upwind convection from the south-west: poisson2d(m) with 0.6 subtracted from every west
    and south entry and 1.2 added to every diagonal entry"""
    rp, ci, v = problems.poisson2d(m)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    v = v.copy()
    v[(ci == rows - 1) | (ci == rows - m)] -= 0.6
    v[ci == rows] += 1.2
    return rp, ci, v


def inputs():
    rp, ci, v, b = load_c0()
    yield "c0", (rp, ci, v, b)
    for name, (rp, ci, v) in (("poisson3d", problems.poisson3d(24)), ("unsymmetric", unsymmetric_grid()), ("convdiff", convdiff()),
                              ("fem", problems.fem_unstructured(20000))):
        yield name, (rp, ci, v, np.ones(len(rp) - 1))


INPUTS = dict(inputs())


def device_handle(name, **kw):
    rp, ci, v, b = INPUTS[name]
    return sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, **kw)), b


def gmres_ref(A0, M, b, x0, m, tol=TOL, cap=100000):
    """(x, history, initial true residual) of right-preconditioned GMRES(m); M = None: no preconditioner"""
    if M is None:
        M = lambda v: v
    n = len(b)
    x = np.array(x0, dtype=np.float64)
    hist, it, r0 = [], 0, None
    while True:
        r = b - A0 @ x
        beta = np.linalg.norm(r)
        if r0 is None:
            r0 = beta
        if beta <= tol or it >= cap:
            break
        V = np.zeros((m + 1, n))
        V[0] = r / beta
        g = np.zeros(m + 1)
        g[0] = beta
        R = np.zeros((m, m))
        cs, sn = np.zeros(m), np.zeros(m)
        k = 0
        for j in range(m):
            if it >= cap:
                break
            w = A0 @ M(V[j])
            Vj = V[: j + 1]
            h = Vj @ w
            w = w - Vj.T @ h
            c = Vj @ w
            w = w - Vj.T @ c
            col = np.append(h + c, np.linalg.norm(w))
            V[j + 1] = w / col[j + 1] if col[j + 1] > 0 else 0.0
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
        x = x + M(V[:k].T @ y)
    return x, np.array(hist), r0


def assert_history(hist, ref, r0):
    assert len(hist) == len(ref), (len(hist), len(ref))
    print("history:", len(hist), "entries")
    if len(ref) == 0:
        return
    tol = hist_tolerance(np.concatenate([[r0], ref]))[1:]  # the rule of conftest.hist_tolerance, seeded with the initial true residual
    err = np.abs(hist - ref) / ref
    print("largest relative history difference", err.max())
    assert np.all(err <= tol), f"max rel err {err.max():.3e} at {err.argmax()}"


def assert_solution(x, ref, rtol):
    err = np.abs(x - ref).max()
    print("solution difference", err, "of", np.abs(ref).max())
    assert err <= rtol * np.abs(ref).max(), err


def true_residual(A0, b, x):
    res = np.linalg.norm(b - A0 @ x)
    print("true residual", res)
    return res


@pytest.mark.parametrize("name", ["c0", "poisson3d", "unsymmetric", "convdiff"])
@pytest.mark.parametrize("restart,random_x0", [(30, False), (5, False), (5, True)])
def test_pgmres_history_is_the_numpy_restatement(name, restart, random_x0):
    A, b = device_handle(name)
    A.set_gmres(restart)
    A0 = A.level_scipy(0)
    x0 = np.random.default_rng(5).standard_normal(A.nrow) if random_x0 else np.zeros(A.nrow)
    want, href, r0 = gmres_ref(A0, A.op_precond, b, x0, restart)
    x = x0.copy()
    hist, rc = A.solve("pgmres", b, x)
    assert rc == 0
    assert_history(hist, href, r0)
    assert true_residual(A0, b, x) <= 1.001 * TOL
    assert_solution(x, want, 1e-6)


@pytest.mark.parametrize("name", ["poisson3d", "convdiff"])
def test_unpreconditioned_head(name):
    A, b = device_handle(name)
    A.set_gmres(10)
    A.set_stopping(TOL, max_iter=25)
    A0 = A.level_scipy(0)
    want, href, _ = gmres_ref(A0, None, b, np.zeros(A.nrow), 10, cap=25)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("gmres", b, x)
    assert rc == sa.SPARSH_ENOCONV and len(hist) == 25 and len(href) == 25
    err = np.abs(hist - href) / href
    print("largest relative history difference", err.max())
    assert np.all(err <= 1e-6)
    assert_solution(x, want, 1e-9)


@pytest.mark.parametrize("precond", ["sor_forward", "sor_symmetric", "fp32"])
def test_pgmres_takes_any_preconditioner_of_the_handle(precond):
    A, b = device_handle("poisson3d", **(dict(precond_fp32=1) if precond == "fp32" else {}))
    if precond != "fp32":
        A.set_smoother("sor", 0, precond[4:])
    A0 = A.level_scipy(0)
    _, href, _ = gmres_ref(A0, A.op_precond, b, np.zeros(A.nrow), 30)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("pgmres", b, x)
    print(precond, "iterations", len(hist), "reference", len(href))
    assert rc == 0
    assert true_residual(A0, b, x) <= 1.001 * TOL
    assert len(hist) == len(href)
    if precond == "sor_forward":
        with pytest.raises(sa.SparshError) as e:
            A.solve("pcg", b, np.zeros(A.nrow))
        assert e.value.code == sa.SPARSH_EINVAL


def test_op_precond_is_the_cycle_of_the_handle():
    A, _ = device_handle("poisson3d")
    r = np.random.default_rng(2).standard_normal(A.nrow)
    x = np.zeros(A.nrow)
    A.vcycle(r, x, iterations=1)
    z = A.op_precond(r)
    print("Jacobi: difference from vcycle", np.abs(z - x).max())
    assert np.abs(z - x).max() <= 1e-13 * np.abs(x).max()
    for order in ("forward", "symmetric"):
        A.set_smoother("sor", 0, order)
        assert np.array_equal(A.op_precond(r), composed_cycle(A, r, np.zeros(A.nrow), 6, order == "symmetric")), order
    F, _ = device_handle("poisson3d", precond_fp32=1)
    assert np.array_equal(F.op_precond(r), F.op_precond_f32(r))


def test_pgmres_converges_where_pcg_does_not():
    A, b = device_handle("convdiff")
    A.set_stopping(TOL, max_iter=200)
    hist, rc = A.solve("pcg", b, np.zeros(A.nrow), allow=(sa.SPARSH_ENUMERIC,))
    finite = hist[np.isfinite(hist)]
    print("pcg: rc", rc, "first", hist[0], "last finite", finite[-1], "entries", len(hist))
    assert rc in (sa.SPARSH_ENOCONV, sa.SPARSH_ENUMERIC)
    assert finite[-1] > hist[0]
    x = np.zeros(A.nrow)
    hist, rc = A.solve("pgmres", b, x)
    print("pgmres iterations", len(hist))
    assert rc == 0 and len(hist) <= 19
    assert true_residual(A.level_scipy(0), b, x) <= 1.001 * TOL


def test_pgmres_on_the_unstructured_mesh():
    """fem_unstructured(20000), restart 30: several restart cycles, so only convergence and the iteration count are compared.
    Measured on the MI355X: 160 iterations, the numpy restatement with the device's op_precond 160."""
    A, b = device_handle("fem")
    A0 = A.level_scipy(0)
    _, href, _ = gmres_ref(A0, A.op_precond, b, np.zeros(A.nrow), 30)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("pgmres", b, x)
    print("fem: iterations", len(hist), "reference", len(href))
    assert rc == 0
    assert true_residual(A0, b, x) <= 1.001 * TOL
    assert abs(len(hist) - len(href)) <= 0.1 * len(href), (len(hist), len(href))


def test_determinism_and_independence():
    A, b = device_handle("c0")
    n = A.nrow
    assert A.gmres_info() == dict(restart=30, basis_bytes=0)
    xp0 = np.zeros(n)
    hp0, _ = A.solve("pcg", b, xp0)
    assert A.gmres_info()["basis_bytes"] == 0
    x1, x2 = np.zeros(n), np.zeros(n)
    h1, rc1 = A.solve("pgmres", b, x1)
    h2, rc2 = A.solve("pgmres", b, x2)
    assert rc1 == 0 and rc2 == 0
    assert np.array_equal(h1, h2) and np.array_equal(x1, x2)
    held = A.gmres_info()["basis_bytes"]
    print("basis bytes", held, "n", n)
    assert 31 * 8 * n <= held < 33 * 8 * n
    xp1 = np.zeros(n)
    hp1, _ = A.solve("pcg", b, xp1)
    assert np.array_equal(hp0, hp1) and np.array_equal(xp0, xp1)
    A.set_gmres(7)
    assert A.gmres_info() == dict(restart=7, basis_bytes=0)
    x3 = np.zeros(n)
    _, rc3 = A.solve("pgmres", b, x3)
    held = A.gmres_info()["basis_bytes"]
    assert rc3 == 0 and 8 * 8 * n <= held < 10 * 8 * n
    A.set_gmres(7)  # unchanged length: the basis stays
    assert A.gmres_info()["basis_bytes"] == held
    A.set_gmres(0)
    assert A.gmres_info() == dict(restart=30, basis_bytes=0)


def test_lucky_breakdown_and_overshoot():
    m = 40
    rp, ci, v = problems.poisson2d(m)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
    s = np.sin(np.pi * np.arange(1, m + 1) / (m + 1))
    b = np.outer(s, s).ravel()  # the lowest eigenvector: the Krylov space is exhausted after one step
    A.set_gmres(10)
    A.set_stopping(TOL, 0, 4)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("gmres", b, x)
    print("history", hist)
    assert rc == 0 and np.all(np.isfinite(x)) and np.all(np.isfinite(hist))
    assert len(hist) <= 4
    assert true_residual(A.level_scipy(0), b, x) <= 1.001 * TOL


@pytest.mark.parametrize("method", ["pgmres", "gmres"])
def test_stopping_rule(method):
    A, b = device_handle("c0")
    A.set_stopping(TOL, max_iter=3)
    want, href, _ = gmres_ref(A.level_scipy(0), A.op_precond if method == "pgmres" else None, b, np.zeros(A.nrow), 30, cap=3)
    x = np.zeros(A.nrow)
    hist, rc = A.solve(method, b, x)
    assert rc == sa.SPARSH_ENOCONV and len(hist) == 3 and len(href) == 3
    assert_solution(x, want, 1e-9)


def test_cpp_gmres_entry_points(c0_files, tmp_path):
    """Solver_PGMRES_1 / Solver_GMRES_1 of the drop-in layer on the bundled matrix files"""
    mf, rf = c0_files
    exe = tmp_path / "gmres_objects"
    cmd = ["g++", "-std=c++17", "-O1", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "cpp", "gmres_objects.cpp"),
           "-o", str(exe), f"-L{LIB_DIR}", "-lsparsh_amg", f"-Wl,-rpath,{LIB_DIR}", "-L/opt/rocm/lib", "-L/opt/rocm/lib/llvm/lib",
           "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib/llvm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), mf, rf], capture_output=True, text=True, timeout=300)
    print(r.stdout[-600:])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
