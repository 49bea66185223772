"""What the block solvers ("pcg", "bcg", "mbicg" of solve_multi) and the eigensolver do around their iterations: the copy of the
residual histories into a buffer shorter than the run, the lines of print_solve (one per flag read), the `seconds` of
solve_multi_dev, and the device bytes their reserves hold.

The operators are the 7-point Laplacian (pcg, bcg) and the upwind convection-diffusion operator (mbicg) on a 12^3 grid.  At 1 728
rows the default coarsening limits leave a single level, whose cycle is the direct solve and whose loops are done after one
iteration; the handles take the limits of tests/test_gpu_bcg.py, which give several levels and runs of 6 iterations and more (every
test asserts that first, so that no cap and no short buffer passes vacuously)."""
import ctypes
import time

import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from test_gpu_krylov_ops import same_bits

pytestmark = pytest.mark.gpu
LIMITS = dict(limit_upper=300, limit_lower=100)  # several levels at 1 728 rows (tests/test_gpu_bcg.py)
# sparsh_params' default, the tolerance of the other block tests, where it gives 6 iterations; block BiCGStab is done after 5
TOL = dict(pcg=1e-8, bcg=1e-8, mbicg=1e-10)
METHODS = ["pcg", "bcg", "mbicg"]
OPERATOR = dict(pcg="poisson", bcg="poisson", mbicg="cd")
N, NRHS = 12 ** 3, 4


def make_handles(**params):
    ops = dict(poisson=problems.poisson3d(12), cd=problems.convection_diffusion(12, 12, 12))
    return {name: sa.sp_matrix_mg(*op).setup(sa.default_params(print_setup=0, **LIMITS, **params)) for name, op in ops.items()}


@pytest.fixture(scope="module")
def quiet():
    H = make_handles(print_solve=0)
    yield H
    for A in H.values():
        A.close()


@pytest.fixture(scope="module")
def talking():
    H = make_handles(print_solve=1)
    yield H
    for A in H.values():
        A.close()


@pytest.fixture(scope="module")
def rhs():
    B = np.random.default_rng(31).standard_normal((N, NRHS))
    B.setflags(write=False)
    return B


def stopping(A, method, max_iter=0, check_every=1):
    A.set_stopping(TOL[method], max_iter or sa.default_params().max_iter, check_every)


def block_solve(A, method, B, **kw):
    """(X, histories, iters, status, rc) of one solve_multi from X = 0"""
    X = np.zeros_like(B)
    hists, iters, status, rc = A.solve_multi(method, B, X, **kw)
    return X, hists, iters, status, rc


@pytest.fixture(scope="module")
def full_runs(quiet, rhs):
    """method -> the converged run with check_every = 1 and the default history buffer; computed once, never written"""
    out = {}
    for m in METHODS:
        stopping(quiet[OPERATOR[m]], m)
        out[m] = block_solve(quiet[OPERATOR[m]], m, rhs)
    return out


def long_enough(method, run):
    """the precondition of every test here: a converged run of at least 6 iterations in every column"""
    X, hists, iters, status, rc = run
    assert rc == sa.SPARSH_OK and np.all(status == sa.SPARSH_OK), (rc, status)
    assert len(iters) == NRHS and np.all(iters >= 6), iters
    assert all(len(h) == it and h[-1] <= TOL[method] for h, it in zip(hists, iters))
    return int(iters.max())


@pytest.mark.parametrize("method", METHODS)
def test_short_history_buffer(quiet, rhs, full_runs, method):
    """A history buffer of three entries per column takes the first three residuals of every column and changes nothing else; a
    buffer of none takes none."""
    A = quiet[OPERATOR[method]]
    X, hists, iters, status, rc = full_runs[method]
    long_enough(method, full_runs[method])
    stopping(A, method)
    X3, h3, it3, st3, rc3 = block_solve(A, method, rhs, hist_cap=3)
    print(method, "iterations", iters, "with three history entries", it3, h3)
    assert rc3 == rc and np.array_equal(it3, iters) and np.array_equal(st3, status)
    for c in range(NRHS):
        assert len(h3[c]) == 3 and same_bits(h3[c], hists[c][:3]), c
    assert same_bits(X3, X)
    X0, h0, it0, st0, rc0 = block_solve(A, method, rhs, hist_cap=0)
    assert rc0 == rc and np.array_equal(it0, iters) and np.array_equal(st0, status)
    assert all(len(h) == 0 for h in h0) and same_bits(X0, X)


def printed_solve(A, method, B, capfd, check_every, max_iter=0):
    """(iters, return code, [(number, text)] of the lines the solve printed)"""
    libc = ctypes.CDLL(None)  # the library prints with printf, block-buffered into the capture's pipe
    libc.fflush(None)
    capfd.readouterr()
    stopping(A, method, max_iter, check_every)
    try:
        _, _, iters, _, rc = block_solve(A, method, B)
    finally:
        stopping(A, method)
    libc.fflush(None)
    lines = [ln.split("\t") for ln in capfd.readouterr().out.splitlines()]
    assert all(len(ln) == 2 for ln in lines), lines
    return iters, rc, [(int(num), text) for num, text in lines]


def assert_line_texts(method, lines, iters=None):
    """"<m> of 4 columns running" (iters given: m = the columns that stop after that read) or "rank <r> of 4", 0 <= m, r <= 4"""
    for it, text in lines:
        words = text.split(" ")
        if method == "bcg":
            assert words[0] == "rank" and words[2:] == ["of", "4"] and words[1] == str(int(words[1])) and 0 <= int(words[1]) <= 4, text
        else:
            assert words[1:] == ["of", "4", "columns", "running"] and words[0] == str(int(words[0])) and 0 <= int(words[0]) <= 4, text
            if iters is not None:
                assert int(words[0]) == int(np.count_nonzero(iters > it)), (it, text, iters)


@pytest.mark.parametrize("check_every", [1, 3])
@pytest.mark.parametrize("method", METHODS)
def test_print_solve_lines(talking, rhs, full_runs, capfd, method, check_every):
    """One line per flag read: after the iterations k, 2k, ... up to the first read that finds every column done, and under an
    iteration cap one more at the cap when that is no multiple of k."""
    A = talking[OPERATOR[method]]
    k = check_every
    m1 = long_enough(method, full_runs[method])
    iters, rc, lines = printed_solve(A, method, rhs, capfd, k)
    print(method, "check_every", k, "full run", m1, "iterations", iters, "printed", lines)
    assert rc == sa.SPARSH_OK
    if method != "bcg":  # (a frozen column stops counting; block CG's columns share one count, which the device stops at `done`)
        assert np.array_equal(iters, full_runs[method][2])
    last = -(-m1 // k) * k  # the first read at or after the last column's stop
    assert [it for it, _ in lines] == list(range(k, last + 1, k))
    assert_line_texts(method, lines, None if method == "bcg" else full_runs[method][2])
    for cap in (4, 5):
        iters_c, rc_c, lines_c = printed_solve(A, method, rhs, capfd, k, cap)
        print(method, "check_every", k, "cap", cap, "iterations", iters_c, "printed", lines_c)
        reads = list(range(k, cap + 1, k))
        if reads[-1:] != [cap]:
            reads.append(cap)
        assert rc_c == sa.SPARSH_ENOCONV and np.all(iters_c == cap)
        assert [it for it, _ in lines_c] == reads
        assert_line_texts(method, lines_c)
        if (cap, k) == (4, 3):
            assert [it for it, _ in lines_c] == [3, 4]


def solve_multi_dev(A, method, B, max_iters=0):
    """(X, iters, rc, seconds as the call reports them, wall seconds around the call) of one solve_multi_dev from X = 0"""
    n, nrhs = B.shape
    bd, xd = A.dev_alloc(8 * n * nrhs), A.dev_alloc(8 * n * nrhs)
    try:
        A.h2d(bd, np.ascontiguousarray(B.T))  # column-major: column c at bd + 8 n c
        A.dev_fill(xd, n * nrhs, 0.0)
        A.sync()
        t0 = time.perf_counter()
        _, iters, _, sec, rc = A.solve_multi_dev(method, nrhs, bd, n, xd, n, max_iters=max_iters)
        wall = time.perf_counter() - t0
        Xt = np.zeros((nrhs, n))
        A.d2h(Xt, xd)
    finally:
        A.dev_free(bd)
        A.dev_free(xd)
    return Xt.T, iters, rc, sec, wall


@pytest.mark.parametrize("method", METHODS)
def test_seconds_of_solve_multi_dev(quiet, rhs, full_runs, method):
    """The HIP-event time of the call: finite, positive and no longer than the wall time around it, converged or capped; the
    device entry point computes what solve_multi computes."""
    A = quiet[OPERATOR[method]]
    X, _, iters, _, _ = full_runs[method]
    long_enough(method, full_runs[method])
    stopping(A, method)
    for cap, want_rc in ((0, sa.SPARSH_OK), (4, sa.SPARSH_ENOCONV)):
        Xd, it, rc, sec, wall = solve_multi_dev(A, method, rhs, max_iters=cap)
        print(method, "cap", cap, "iterations", it, "rc", rc, "seconds", sec, "wall", wall)
        assert rc == want_rc
        assert np.isfinite(sec) and 0.0 < sec <= wall
        if cap == 0:
            assert np.array_equal(it, iters) and same_bits(Xd, X)
        else:
            assert np.all(it == cap)


# ---------------------------------------------------------------------------- device bytes of the reserves

K_MULTI_MAX, K_EIG_PAIRS, K_EIG_MAX_GRID = 8, 12, 512  # kMultiMax, kEigPairs, kEigMaxGrid of kernels.hpp
MB_COUNT, BF_COUNT = 9, 16                              # scalars per column of block BiCGStab, flags of block CG
FLAG_DOUBLES = (3 * K_MULTI_MAX + 1) // 2               # frozen, iters, status as ints, in doubles


def mbicg_bytes(n, W):
    """mbicg_reserve: R0, S, AS, P1, the per-column scalars and the flags"""
    return 8 * (4 * n * W + MB_COUNT * K_MULTI_MAX + FLAG_DOUBLES)


def bcg_bytes(W):
    """bcg_reserve: [G, C1, C2], [alpha, beta], the Gram launch's partial sums, the factor, d, res and the flags"""
    return 8 * (3 * W * W + 2 * W * W + 2 * W * W * K_EIG_MAX_GRID + K_MULTI_MAX * K_MULTI_MAX + 2 * K_MULTI_MAX + BF_COUNT // 2)


def eig_bytes(n, W):
    """eig_reserve: seven blocks, the partial sums of the Gram and residual launches, G with the norms, the coefficients"""
    return 8 * (7 * n * W + (K_EIG_PAIRS * W * W + W) * K_EIG_MAX_GRID + 2 * 9 * W * W + W + 3 * W * W + W)


# multi_reserve's count needs the rows and the row-block counts of every level: recorded once at the commit before the block solvers
# were given one shared allocator (f6ebb43), on the two hierarchies of this file
MULTI_BYTES_AT_PARENT = dict(poisson={4: 7244448, 2: 6954144}, cd={4: 7244448, 2: 6954144})


def test_reserved_bytes(rhs):
    H = make_handles(print_solve=0)
    try:
        for W in (4, 2):
            for m in METHODS:
                stopping(H[OPERATOR[m]], m)
                assert block_solve(H[OPERATOR[m]], m, rhs[:, :W])[4] == sa.SPARSH_OK
            got = dict(multi_poisson=H["poisson"].multi_info(), multi_cd=H["cd"].multi_info(), bcg=H["poisson"].bcg_info()["bytes"],
                       mbicg=H["cd"].mbicg_info()["bytes"])
            print("width", W, got)
            assert got["mbicg"] == mbicg_bytes(N, W) and got["bcg"] == bcg_bytes(W)
            assert got["multi_poisson"] == dict(width=W, bytes=MULTI_BYTES_AT_PARENT["poisson"][W])
            assert got["multi_cd"] == dict(width=W, bytes=MULTI_BYTES_AT_PARENT["cd"][W])
            assert H["cd"].bcg_info()["bytes"] == 0 and H["poisson"].mbicg_info()["bytes"] == 0
        H["poisson"].eigs(4)
        info = H["poisson"].eig_info()
        print("eigs(4)", info, H["poisson"].multi_info())
        assert info["width"] == 4 and info["bytes"] == eig_bytes(N, 4)
        assert H["poisson"].multi_info() == dict(width=4, bytes=MULTI_BYTES_AT_PARENT["poisson"][4])  # the cycle's blocks, at the eigensolver's width
        assert H["poisson"].bcg_info()["bytes"] == 0  # ... and the change of width released block CG's arrays with them
    finally:
        for A in H.values():
            A.close()
