"""What every single-vector Krylov loop does around its iterations, on the system of the loop tests in test_gpu_krylov_ops.py: the
copy of the residual history into a buffer shorter than the run, the start and the end under a constant null space, the lines of
print_solve (one per residual read, numbered as the loop numbers them) and the iteration cap of GMRES between two reads."""
import ctypes

import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from test_gpu_krylov_ops import same_bits
from test_gpu_nullspace import GRIDS, Case

pytestmark = pytest.mark.gpu
TOL = 1e-8
RESTART = 5
METHODS = ["cg", "pcg", "bicg", "pbicg", "fcg", "gmres", "pgmres"]


def poisson_handle(**params):
    rp, ci, v = problems.poisson3d(30)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(print_setup=0, **params))
    A.set_gmres(RESTART)
    return A, np.ones(len(rp) - 1)


@pytest.fixture(scope="module")
def quiet():
    A, b = poisson_handle(print_solve=0)
    yield A, b
    A.close()


@pytest.fixture(scope="module")
def talking():
    A, b = poisson_handle(print_solve=1)
    yield A, b, {}  # method -> iterations to convergence under check_every = 1
    A.close()


@pytest.fixture(scope="module")
def neumann():
    c = Case(GRIDS[0])
    c.A.set_gmres(RESTART)
    yield c
    c.A.close()


def solve_dev(A, b, method, hist_cap=None):
    """(history as returned, iteration count, return code, x) of one solve_dev from x = 0"""
    n = A.nrow
    bd, xd = A.dev_alloc(8 * n), A.dev_alloc(8 * n)
    try:
        A.h2d(bd, b)
        A.h2d(xd, np.zeros(n))
        hist, iters, _, rc = A.solve_dev(method, bd, xd) if hist_cap is None else A.solve_dev(method, bd, xd, hist_cap=hist_cap)
        x = np.zeros(n)
        A.d2h(x, xd)
    finally:
        A.dev_free(bd)
        A.dev_free(xd)
    return hist, iters, rc, x


@pytest.fixture(scope="module")
def full_runs(quiet):
    """method -> the converged run with check_every = 1 and the default history buffer; computed once, never written"""
    A, b = quiet
    A.set_stopping(TOL, 100000, 1)
    return {m: solve_dev(A, b, m) for m in METHODS}


@pytest.mark.parametrize("method", METHODS)
def test_short_history_buffer(quiet, full_runs, method):
    """A history buffer of three entries takes the first three residuals and changes nothing else."""
    A, b = quiet
    hist, iters, rc, x = full_runs[method]
    assert rc == sa.SPARSH_OK and iters == len(hist) > 3 and hist[-1] <= TOL
    A.set_stopping(TOL, 100000, 1)
    h3, iters3, rc3, x3 = solve_dev(A, b, method, hist_cap=3)
    print(method, "iterations", iters, "with three history entries", iters3, h3)
    assert iters3 == iters and rc3 == rc
    assert len(h3) == 3 and same_bits(h3, hist[:3])
    assert same_bits(x3, x)


@pytest.mark.parametrize("method", METHODS)
def test_null_space_start_and_finish(neumann, method):
    """Singular pure-Neumann system: the returned x is mean-free (the bound of tests/test_gpu_nullspace.py) and the history does
    not depend on how often the host reads it."""
    c = neumann
    runs = {}
    try:
        for k in (1, 4):
            c.A.set_stopping(TOL, 100000, k)
            x = np.zeros(c.n)
            h, rc = c.A.solve(method, c.b, x)
            print(f"{method} check_every {k}: {len(h)} iterations, rc {rc}, |mean x| {abs(x.mean()):.3e}, max |x| {np.abs(x).max():.3e}")
            assert rc == sa.SPARSH_OK
            assert abs(x.mean()) <= c.n * 2.0 ** -52 * np.abs(x).max()
            runs[k] = h
    finally:
        c.A.set_stopping(TOL, 100000, 1)
    m1 = len(runs[1])
    assert len(runs[4]) >= m1 and same_bits(runs[4][:m1], runs[1])


def printed_solve(A, b, method, capfd, check_every, max_iter):
    """(history, return code, [(number, residual text)] of the lines the solve printed)"""
    libc = ctypes.CDLL(None)  # the library prints with printf, block-buffered into the capture's pipe
    libc.fflush(None)
    capfd.readouterr()
    A.set_stopping(TOL, max_iter, check_every)
    hist, rc = A.solve(method, b, np.zeros(A.nrow))
    libc.fflush(None)
    lines = [ln.split("\t") for ln in capfd.readouterr().out.splitlines()]
    assert all(len(ln) == 2 for ln in lines), lines
    return hist, rc, [(int(num), text) for num, text in lines]


@pytest.mark.parametrize("check_every", [1, 3])
@pytest.mark.parametrize("method", ["pcg", "pbicg", "fcg", "pgmres"])
def test_print_solve_lines(talking, capfd, method, check_every):
    """One line per residual read: at the iterations k, 2k, ... and at the iteration cap, numbered by the iteration (BiCGStab: one
    less), with the residual as %g of the history entry that was read."""
    A, b, counts = talking
    k = check_every
    try:
        if method not in counts:
            counts[method] = len(printed_solve(A, b, method, capfd, 1, 100000)[0])
        m1 = counts[method]
        hist, rc, lines = printed_solve(A, b, method, capfd, k, 100000)
        assert rc == sa.SPARSH_OK and len(hist) >= m1 >= 7  # (so that the cap below lies behind the first read of check_every = 3)
        if method != "pgmres":  # (a GMRES cycle may end, and its true residual stop the solve, between two reads)
            assert len(hist) % k == 0
        cap = m1 - 2 if (m1 - 2) % 3 else m1 - 3  # no multiple of 3, before convergence
        hist_c, rc_c, lines_c = printed_solve(A, b, method, capfd, k, cap)
        assert rc_c == sa.SPARSH_ENOCONV and len(hist_c) == cap and cap % 3 != 0
    finally:
        A.set_stopping(TOL, 100000, 1)
    shift = 1 if method == "pbicg" else 0
    for what, h, got, last in (("to convergence", hist, lines, None), ("capped", hist_c, lines_c, cap)):
        reads = list(range(k, len(h) + 1, k))
        if last is not None and reads[-1] != last:
            reads.append(last)
        print(method, "check_every", k, what, "reads at", reads, "printed", got)
        assert got == [(it - shift, "%g" % h[it - 1]) for it in reads], what


@pytest.mark.parametrize("method", ["gmres", "pgmres"])
def test_gmres_iteration_cap_between_reads(quiet, full_runs, method):
    """An iteration cap that is no multiple of check_every: SPARSH_ENOCONV after exactly `cap` iterations, as the other loops do
    (test_loops_under_check_every)."""
    A, b = quiet
    h1 = full_runs[method][0]
    m1 = len(h1)
    cap = m1 - 2 if (m1 - 2) % 4 else m1 - 3
    try:
        out = {}
        for k in (1, 4):
            A.set_stopping(TOL, cap, k)
            out[k] = solve_dev(A, b, method)
    finally:
        A.set_stopping(TOL, 100000, 1)
    (hc1, it1, rc1, xc1), (hc4, it4, rc4, xc4) = out[1], out[4]
    print(method, "converges in", m1, "cap", cap, "iterations", it1, it4, "codes", rc1, rc4)
    assert cap % 4 != 0 and rc1 == rc4 == sa.SPARSH_ENOCONV
    assert it1 == it4 == cap and len(hc1) == len(hc4) == cap
    assert same_bits(hc1, hc4) and same_bits(xc1, xc4) and same_bits(hc1, h1[:cap])
