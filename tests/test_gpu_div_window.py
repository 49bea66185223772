"""The box-grid kernels' division by the constant diagonal (div_const) on both sides of its exponent window.

Inside the window (|E - 1023| <= 256 for the biased exponent E of the numerator) div_const is three instructions on a reciprocal
refined once per thread; a wave with one numerator outside it takes the plain division.  Both must give the plain division's bits.
On a 12^3 Poisson box (the smallest on which a tile has interior lines, ring lines, a first, a last and a short last chunk at once;
the hierarchy is cut at 200 rows so that it has box levels at all) every box level runs under forced plans of 256, 512 and 1024
threads with Q = 2 and Q = 4, fewer lines per tile than the level has and 5 planes per chunk, on standard-normal x and b scaled by
2^s: at s = 0 and 250 the numerators omega h and omega b lie inside the window, at -250 and 262 one of its edges runs through the
vector, at -262, +-300 and +-600 all lie outside; then s = 0 with every 7th entry of b zero, and s = 0 with one entry of b 2^300
times larger (one wave of a workgroup on the other branch).  op_jacobi (2, 4, 7 sweeps from x; 3, 4, 7 from a zero guess; 1 and 3
through the marching kernel), op_jacobi_dot and op_residual_restrict are compared bit for bit with the CPU oracle on the level's own
CSR; the oracle's results are finite at every scale (asserted).  On that box a tile's region is smaller than a workgroup, so every
thread owns one live point at most; a second box, 40 x 24 x 7, runs its finest level under the smallest tiles whose region has more
points than the workgroup has threads -- (TY + 4) nx = 280, 520 and 1040 for 256, 512 and 1024 threads -- so that the second point of
a thread (q = 1) is live under every thread count and meets the same numerators.  The helpers are those of test_gpu_box_threads.py.  GPU box only.
"""
import numpy as np
import pytest

import oracle
import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
WINDOW = 256  # kDivWindow of csrc/kernels.hip
# The numerators omega h and omega b of standard-normal vectors span about 2^-8 .. 2^5, and the window is 2^-256 <= |a| < 2^257: at 2^250 all
# of them are inside, at 2^262 only those below 2^-5 (the upper edge runs through the vector), at 2^-250 all but those below 2^-6 (the lower
# edge does), at 2^-262 none
SCALES = (0, 250, -250, 262, -262, 300, -300, 600, -600)
assert 250 < WINDOW < 262
DOUBLE_FROM_X, DOUBLE_FROM_ZERO, MARCHING = (2, 4, 7), (3, 4, 7), (1, 3)


def _csr(A, l, which="A"):
    rp, ci, v, ncol = A.level_csr(l, which)
    return oracle.Csr(rp, ci, v, ncol=ncol)


def _dot_ok(got, x, y):
    """A fused dot against the long-double sum of its terms, to 1e-12 of the sum of their magnitudes (as test_blas1)."""
    t = np.asarray(x, dtype=np.longdouble) * np.asarray(y, dtype=np.longdouble)
    return abs(np.longdouble(got) - t.sum()) <= 1e-12 * np.abs(t).sum()


def _cases(n, rng):
    """name -> (x, b, the dot y . b is representable in fp64)."""
    x, b = rng.standard_normal(n), rng.standard_normal(n)
    out = {}
    for s in SCALES:  # x is scaled with b, so that h = b - A x keeps the magnitude
        out[f"2^{s}"] = (np.ldexp(x, s), np.ldexp(b, s), abs(2 * s) < 1000)
    bz = b.copy()
    bz[::7] = 0.0
    out["zeros in b"] = (x, bz, True)
    b1 = b.copy()
    r = (2 * n) // 3 + 1  # a row of the last third: its wave alone leaves the window in the first sweep
    b1[r] = np.ldexp(b1[r], 300)
    out["one row 2^300"] = (x, b1, True)
    return out


class _Ref:
    """What the oracle gives on level l for one case; independent of the launch plan, so computed once and left alone."""

    def __init__(self, Ol, P, Oc, x, b, paired):
        zero = np.zeros(len(b))
        self.x, self.b = x, b
        self.jac = {s: oracle.jacobi(Ol, b, x, s - 1) for s in set(DOUBLE_FROM_X + MARCHING)}
        self.jz = {s: oracle.jacobi(Ol, b, zero, s - 1) for s in DOUBLE_FROM_ZERO}
        self.restrict = None
        if paired:
            bc = oracle.transfer_residual(P, oracle.store_residual(Ol, b, x))
            self.restrict = (bc, oracle.jacobi(Oc, bc, np.zeros(len(bc)), 0))

    def vectors(self):
        return list(self.jac.values()) + list(self.jz.values()) + (list(self.restrict) if self.restrict else [])


def _level_refs(A, l, rng):
    n = A.level_info(l)["nrow"]
    grid = tuple(A.level_double_sweep(l)["grid"])
    paired = A.level_paired(l) == 1 and grid[0] % 2 == 0  # row pairs on an even line: the marching kernel's RESID_PAIRX epilogue
    Ol = _csr(A, l)
    P, Oc = (_csr(A, l, "P"), _csr(A, l + 1)) if paired else (None, None)
    refs = {}
    for name, (x, b, dot_fits) in _cases(n, rng).items():
        ref = _Ref(Ol, P, Oc, x, b, paired)
        ref.dot_fits = dot_fits
        for v in ref.vectors():  # a case in which the oracle itself overflows would prove nothing
            assert np.all(np.isfinite(v)), (l, name)
        refs[name] = ref
    return refs


@pytest.fixture(scope="module")
def hierarchy():
    rp, ci, v = problems.poisson3d(12)
    A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET, limit_upper=200, limit_lower=100))
    boxes = [l for l in range(A.nlevels - 1) if A.level_double_sweep(l)["on"] and A.level_marching_ops(l)["on"]]
    assert len(boxes) >= 2 and boxes[0] == 0, [A.level_double_sweep(l) for l in range(A.nlevels)]
    assert A.level_double_sweep(0)["grid"] == [12, 12, 12]
    rng = np.random.default_rng(211)
    refs = {l: _level_refs(A, l, rng) for l in boxes}
    assert any(r["2^0"].restrict for r in refs.values())  # the pair restriction ran somewhere
    yield A, boxes, refs
    A.close()


def _check_level(A, l, refs, threads, plan2, plan1):
    """Level l under (Q, TY, CZ) plan2 for the double sweep and plan1 for the marching kernel, both on `threads` threads: every case of refs."""
    A.set_box_plan(l, 2, *plan2, threads=threads).set_box_plan(l, 1, *plan1, threads=threads)
    assert A.level_box_threads(l) == (threads, threads)
    for name, ref in refs.items():
        tag = (l, threads, plan2, plan1, name)
        n = len(ref.b)
        for s in DOUBLE_FROM_X:
            assert np.array_equal(A.op_jacobi(l, ref.b, ref.x, s), ref.jac[s]), (tag, "jacobi", s)
        for s in DOUBLE_FROM_ZERO:
            assert np.array_equal(A.op_jacobi(l, ref.b, np.zeros(n), s, x_is_zero=True), ref.jz[s]), (tag, "jacobi from zero", s)
        for s in MARCHING:
            assert np.array_equal(A.op_jacobi(l, ref.b, ref.x, s), ref.jac[s]), (tag, "jacobi, marching kernel", s)
        y, d = A.op_jacobi_dot(l, ref.b, ref.x)
        assert np.array_equal(y, ref.jac[1]), (tag, "jacobi_dot")
        if ref.dot_fits:  # (2^+-600: the products y_i b_i leave fp64's range, the sweep's result does not)
            assert _dot_ok(d, ref.jac[1], ref.b), (tag, "jacobi_dot: dot")
        if ref.restrict:
            bc, xc = A.op_residual_restrict(l, ref.b, ref.x)
            assert np.array_equal(bc, ref.restrict[0]) and np.array_equal(xc, ref.restrict[1]), (tag, "residual_restrict")
    A.set_box_plan(l, 2).set_box_plan(l, 1)  # back to the planner's plans
    return len(refs)


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_div_window_bitwise(hierarchy, threads):
    """Every box level of the 12^3 hierarchy: fewer lines per tile than the level has (a ring, interior lines, a short last tile), 5 planes
    per chunk (a short last chunk), Q = 2 and Q = 4."""
    A, boxes, refs = hierarchy
    ran = 0
    for l in boxes:
        nx, ny, nz = A.level_double_sweep(l)["grid"]
        for q in (2, 4):
            plan = (q, min(5, ny - 1), min(5, nz))
            ran += _check_level(A, l, refs[l], threads, plan, plan)
    assert ran == len(boxes) * 2 * (len(SCALES) + 2)


WIDE = (40, 24, 7)


@pytest.fixture(scope="module")
def wide():
    rp, ci, v = problems.poisson3d(*WIDE)
    A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET))
    assert A.nlevels >= 2 and A.level_double_sweep(0)["on"] and A.level_marching_ops(0)["on"]
    assert tuple(A.level_double_sweep(0)["grid"]) == WIDE
    refs = _level_refs(A, 0, np.random.default_rng(223))  # (with the pair restriction only if this box pairs rows along x)
    yield A, refs
    A.close()


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_div_window_second_point_live(wide, threads):
    """40 x 24 x 7, finest level: the smallest tile whose region has more points than the workgroup has threads (280, 520, 1040), so that
    threads own a live second point (q = 1) at Q = 2 and Q = 4 and the region ends inside a wave; 5 planes per chunk of 7."""
    A, refs = wide
    nx, ny, nz = WIDE
    lines = threads // nx + 1  # lines of a region of just above `threads` points
    assert threads < lines * nx <= 2 * threads and lines - 4 < ny and lines - 2 <= ny
    for q in (2, 4):
        assert _check_level(A, 0, refs, threads, (q, lines - 4, 5), (q, lines - 2, 5)) == len(SCALES) + 2
