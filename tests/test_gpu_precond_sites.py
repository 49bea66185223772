"""The places where SPARSH_PCG and SPARSH_PBICG apply the preconditioner (pcg_init, pcg_body, both applications in bicg) against a
numpy restatement of Solver_PCG_1 / Solver_PBiCG_1 that applies the device's own op_precond and the level-0 operator as SciPy
holds it, under every preconditioner a handle can have.  GPU box only.

Three iterations from x0 = 0 on poisson3d(24), the smallest problem whose hierarchy has box-grid levels (the Jacobi cycle takes its
fused paths, the zero-guess sweep written by the CG update included): pcg_init's application, pcg_body's twice, bicg's two three
times each.  The restatement differs from the device in the order of the additions inside a dot product, and under Jacobi by the
1e-13 between the fused cycle and op_precond that test_op_precond_is_the_cycle_of_the_handle allows.
"""
import functools

import numpy as np
import pytest

import sparsh_amg_amd as sa
from test_gpu_gmres import TOL, assert_history, assert_solution, device_handle

pytestmark = pytest.mark.gpu

K = 3  # iterations of every run
CONFIGS = {  # name -> (setup parameters, smoother selection or None)
    "jacobi": ({}, None),
    "jacobi_fp32": (dict(precond_fp32=1), None),
    "sor_symmetric": ({}, ("sor", 0, "symmetric")),
    "sor_forward": ({}, ("sor", 0, "forward")),
    "chebyshev": ({}, ("chebyshev", 0, "forward")),
}
PCG_CONFIGS = [c for c in CONFIGS if c != "sor_forward"]  # SPARSH_PCG refuses the unsymmetric preconditioner


@functools.lru_cache(maxsize=None)
def handle(config, use_graph=0):
    params, smoother = CONFIGS[config]
    A, b = device_handle("poisson3d", use_graph=use_graph, **params)
    if smoother:
        A.set_smoother(*smoother)
    A.set_stopping(TOL, max_iter=K)
    return A, b


def pcg_ref(A0, M, b, k):
    """(x, history) of k iterations of Solver_PCG_1 from x = 0, in the order of Engine::pcg_init / Engine::pcg_body"""
    x = np.zeros(len(b))
    r = b - A0 @ x
    z = M(r)
    rz, p, hist = z @ r, z.copy(), []
    for _ in range(k):
        Ap = A0 @ p
        alpha = rz / (p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        z = M(r)
        zr = z @ r
        beta, rz = zr / rz, zr
        hist.append(np.linalg.norm(r))
        p = z + beta * p
    return x, np.array(hist)


def pbicg_ref(A0, M, b, k):
    """(x, history) of k iterations of Solver_PBiCG_1 from x = 0, in the order of Engine::bicg"""
    x = np.zeros(len(b))
    r0 = b - A0 @ x
    r, p, hist = r0.copy(), r0.copy(), []
    for _ in range(k):
        p1 = M(p)
        Ap = A0 @ p1
        alpha1 = r @ r0
        alpha = alpha1 / (Ap @ r0)
        s = r - alpha * Ap
        s1 = M(s)
        As = A0 @ s1
        omega = (As @ s) / (As @ As)
        x = x + alpha * p1 + omega * s1
        r = s - omega * As
        beta = (r @ r0) / alpha1 * (alpha / omega)
        hist.append(np.linalg.norm(r))
        p = r + beta * (p - omega * Ap)
    return x, np.array(hist)


def run(A, method, b):
    x = np.zeros(A.nrow)
    hist, rc = A.solve(method, b, x)
    assert rc == sa.SPARSH_ENOCONV and len(hist) == K, (rc, len(hist))
    assert hist[-1] > TOL  # K iterations do not converge: every one of them ran
    return x, hist


@pytest.mark.parametrize("method,config", [("pcg", c) for c in PCG_CONFIGS] + [("pbicg", c) for c in CONFIGS])
def test_krylov_head_is_the_numpy_restatement_with_op_precond(method, config):
    A, b = handle(config)
    want, href = (pcg_ref if method == "pcg" else pbicg_ref)(A.level_scipy(0), A.op_precond, b, K)
    x, hist = run(A, method, b)
    print(method, config, "history", hist)
    assert_history(hist, href, np.linalg.norm(b))
    assert_solution(x, want, 1e-9)


@pytest.mark.parametrize("config", PCG_CONFIGS)
def test_graph_replay_of_the_pcg_head_is_bitwise_the_eager_run(config):
    (E, b), (G, _) = handle(config, 0), handle(config, 1)
    x0, h0 = run(E, "pcg", b)
    x1, h1 = run(G, "pcg", b)
    print(config, "history", h0)
    assert np.array_equal(h0, h1) and np.array_equal(x0, x1)
