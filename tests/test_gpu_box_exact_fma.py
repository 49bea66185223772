"""The box-grid kernels' exact-FMA instances (sparsh_set_box_exact_fma): on levels whose six off-diagonal stencil constants are all 0 or
+-2^k, k >= 0, the off-diagonal terms of every stencil sum are one FMA each.  c x is then exact, so the results must be the unfused
code's -- and the CPU oracle's -- bit for bit wherever those are finite.

Boxes and plans are those of test_gpu_div_window.py (its helpers, and _stencil7 of test_gpu_box_threads.py): the 12^3 box with the
hierarchy cut at 200 rows (ring lines, first / last / short chunks on every box level) and the 40 x 24 x 7 box under the smallest tiles
that give a thread a live second point, under forced plans of 256, 512 and 1024 threads with Q = 2 and Q = 4.  Operators: the Poisson
stencil (-1), twice it (-2, diagonal 12), a non-symmetric stencil (-1, +2, -4, -1, -2, +4 around 16: diagonally dominant) -- these
qualify -- and, not qualifying (the flag must read false, the results still be the oracle's): half the Poisson stencil (-0.5) and one
with a 3.0.  Vectors: standard-normal x and b times 2^s, s = 0, +-600, +-900 and -1040 (a denormal iterate), and b with every 7th
entry zero.  A scale at which the oracle itself leaves fp64's range is dropped for that operator (at most one, never 0 or +-600).
op_jacobi (2, 4, 7 sweeps from x; 3, 4, 7 from zero; 1 and 3 through the marching kernel), op_jacobi_dot and op_residual_restrict:
mode 1 against the oracle, mode 0 against mode 1 on the same handle, the fused dot to 1e-12.  Then a 20-iteration PCG history on
poisson3d(24), mode 0 against mode 1.  GPU box only.
"""
import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from test_gpu_box_threads import _stencil7
from test_gpu_div_window import DOUBLE_FROM_X, DOUBLE_FROM_ZERO, MARCHING, QUIET, WIDE, _Ref, _csr, _dot_ok

pytestmark = pytest.mark.gpu

SCALES = (0, 600, -600, 900, -900, -1040)
NEVER_DROPPED = (0, 600, -600)
THREADS = (256, 512, 1024)
POISSON = (-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0)
# name -> (the seven constants, the rule holds)
OPERATORS = {
    "poisson": (POISSON, True),
    "poisson x 2": (tuple(2.0 * c for c in POISSON), True),
    "non-symmetric": ((-1.0, 2.0, -4.0, 16.0, -1.0, -2.0, 4.0), True),
    "poisson x 0.5": (tuple(0.5 * c for c in POISSON), False),
    "one 3.0": ((-1.0, -1.0, -3.0, 9.0, -1.0, -1.0, -1.0), False),
}


def _cases(n, rng):
    """name -> (x, b, scale or None, the dot y . b is representable in fp64)."""
    x, b = rng.standard_normal(n), rng.standard_normal(n)
    out = {}
    for s in SCALES:  # x is scaled with b, so that h = b - A x keeps the magnitude
        out[f"2^{s}"] = (np.ldexp(x, s), np.ldexp(b, s), s, abs(2 * s) < 1000)
    bz = b.copy()
    bz[::7] = 0.0
    out["zeros in b"] = (x, bz, None, True)
    return out


def _level_refs(A, l, rng, dropped):
    """The oracle's results on level l for every case whose results are finite; the scales dropped go to `dropped`."""
    n = A.level_info(l)["nrow"]
    grid = tuple(A.level_double_sweep(l)["grid"])
    paired = A.level_paired(l) == 1 and grid[0] % 2 == 0  # row pairs on an even line: the marching kernel's RESID_PAIRX epilogue
    Ol = _csr(A, l)
    P, Oc = (_csr(A, l, "P"), _csr(A, l + 1)) if paired else (None, None)
    refs = {}
    for name, (x, b, scale, dot_fits) in _cases(n, rng).items():
        with np.errstate(all="ignore"):
            ref = _Ref(Ol, P, Oc, x, b, paired)
        ref.dot_fits = dot_fits
        if not all(np.all(np.isfinite(v)) for v in ref.vectors()):  # a case in which the oracle itself overflows would prove nothing
            assert scale is not None and scale not in NEVER_DROPPED, (l, name)
            dropped.add(scale)
            continue
        if scale == -1040:
            assert np.abs(ref.x).max() < 2.0 ** -1022  # the iterate is denormal
        refs[name] = ref
    return refs


def _handle(c, dims, **params):
    rp, ci, v = _stencil7(*dims, c)
    return sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET, **params))


def _box_levels(A):
    return [l for l in range(A.nlevels - 1) if A.level_double_sweep(l)["on"] and A.level_marching_ops(l)["on"]]


@pytest.fixture(scope="module", params=list(OPERATORS))
def cube(request):
    """12^3, hierarchy cut at 200 rows: (handle, box levels, level -> refs, whether the operator qualifies)."""
    c, qualifies = OPERATORS[request.param]
    A = _handle(c, (12, 12, 12), limit_upper=200, limit_lower=100)
    boxes = _box_levels(A)
    assert boxes and boxes[0] == 0 and A.level_double_sweep(0)["grid"] == [12, 12, 12], [A.level_double_sweep(l) for l in range(A.nlevels)]
    if request.param == "poisson":
        assert len(boxes) >= 2
    rng = np.random.default_rng(311)
    dropped = set()
    refs = {l: _level_refs(A, l, rng, dropped) for l in boxes}
    assert len(dropped) <= 1, dropped
    yield A, boxes, refs, qualifies
    A.close()


@pytest.fixture(scope="module", params=list(OPERATORS))
def wide(request):
    c, qualifies = OPERATORS[request.param]
    A = _handle(c, WIDE)
    assert A.nlevels >= 2 and A.level_double_sweep(0)["on"] and A.level_marching_ops(0)["on"]
    assert tuple(A.level_double_sweep(0)["grid"]) == WIDE
    dropped = set()
    refs = _level_refs(A, 0, np.random.default_rng(323), dropped)
    assert len(dropped) <= 1, dropped
    yield A, refs, qualifies
    A.close()


def _run(A, l, ref):
    """Every op of the checks on one case: name -> result."""
    n = len(ref.b)
    out = {}
    for s in DOUBLE_FROM_X + MARCHING:
        out["jacobi", s] = A.op_jacobi(l, ref.b, ref.x, s)
    for s in DOUBLE_FROM_ZERO:
        out["jacobi from zero", s] = A.op_jacobi(l, ref.b, np.zeros(n), s, x_is_zero=True)
    out["jacobi_dot"], out["dot"] = A.op_jacobi_dot(l, ref.b, ref.x)
    if ref.restrict:
        out["restrict bc"], out["restrict xc"] = A.op_residual_restrict(l, ref.b, ref.x)
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _check_level(A, l, refs, qualifies, threads, plan2, plan1):
    """Level l under (Q, TY, CZ) plan2 for the double sweep and plan1 for the marching kernel, both on `threads` threads: every case of refs,
    mode 1 against the oracle and mode 0 against mode 1."""
    A.set_box_plan(l, 2, *plan2, threads=threads).set_box_plan(l, 1, *plan1, threads=threads)
    assert A.level_box_threads(l) == (threads, threads)
    for name, ref in refs.items():
        tag = (l, threads, plan2, plan1, name)
        A.set_box_exact_fma(1)
        assert A.level_box_exact_fma(l) is qualifies, tag
        on = _run(A, l, ref)
        A.set_box_exact_fma(0)
        assert A.level_box_exact_fma(l) is False, tag
        off = _run(A, l, ref)
        A.set_box_exact_fma(1)
        for s in DOUBLE_FROM_X + MARCHING:
            assert np.array_equal(on["jacobi", s], ref.jac[s]), (tag, "jacobi", s)
        for s in DOUBLE_FROM_ZERO:
            assert np.array_equal(on["jacobi from zero", s], ref.jz[s]), (tag, "jacobi from zero", s)
        assert np.array_equal(on["jacobi_dot"], ref.jac[1]), (tag, "jacobi_dot")
        if ref.dot_fits:  # (otherwise the products y_i b_i leave fp64's range, the sweep's result does not)
            assert _dot_ok(on["dot"], ref.jac[1], ref.b) and _dot_ok(off["dot"], ref.jac[1], ref.b), (tag, "jacobi_dot: dot")
        if ref.restrict:
            assert np.array_equal(on["restrict bc"], ref.restrict[0]) and np.array_equal(on["restrict xc"], ref.restrict[1]), (tag, "residual_restrict")
        for key in on:  # the two modes: the same bits, zero signs included (the dot: the same terms in the same order)
            assert _same_bits(on[key], off[key]), (tag, "mode 0 against mode 1", key)
    A.set_box_plan(l, 2).set_box_plan(l, 1)  # back to the planner's plans
    return len(refs)


@pytest.mark.parametrize("threads", THREADS)
def test_exact_fma_bitwise(cube, threads):
    """Every box level of the 12^3 hierarchy: fewer lines per tile than the level has (a ring, interior lines, a short last tile), 5 planes
    per chunk (a short last chunk), Q = 2 and Q = 4."""
    A, boxes, refs, qualifies = cube
    ran = 0
    for l in boxes:
        nx, ny, nz = A.level_double_sweep(l)["grid"]
        for q in (2, 4):
            plan = (q, min(5, ny - 1), min(5, nz))
            ran += _check_level(A, l, refs[l], qualifies if l == 0 else A.level_box_exact_fma(l), threads, plan, plan)
    assert ran >= len(boxes) * 2 * len(SCALES)  # (at most one scale dropped, the zeros case never)


def test_exact_fma_rule_on_the_coarse_levels(cube):
    """The finest level's flag is the operator's; below it pairwise aggregation of the Poisson stencils multiplies edge counts: powers of
    two times the fine constant, so twice and once the Poisson stencil qualify on every box level and half of it on none whose constants
    stay below 1."""
    A, boxes, refs, qualifies = cube
    assert A.level_box_exact_fma(0) is qualifies
    for l in boxes:
        rp, ci, v, _ = A.level_csr(l, "A")
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        off = np.unique(v[ci != rows])
        m, e = np.frexp(np.abs(off))
        want = bool(np.all((off == 0.0) | ((m == 0.5) & (e >= 1))))
        assert A.level_box_exact_fma(l) is want, (l, off)


@pytest.mark.parametrize("threads", THREADS)
def test_exact_fma_second_point_live(wide, threads):
    """40 x 24 x 7, finest level: the smallest tile whose region has more points than the workgroup has threads (280, 520, 1040), so that
    threads own a live second point (q = 1) at Q = 2 and Q = 4 and the region ends inside a wave; 5 planes per chunk of 7."""
    A, refs, qualifies = wide
    nx, ny, nz = WIDE
    lines = threads // nx + 1  # lines of a region of just above `threads` points
    assert threads < lines * nx <= 2 * threads and lines - 4 < ny and lines - 2 <= ny
    for q in (2, 4):
        assert _check_level(A, 0, refs, qualifies, threads, (q, lines - 4, 5), (q, lines - 2, 5)) >= len(SCALES)


def test_pcg_history_is_the_same_in_both_modes():
    """poisson3d(24) with the box kernels forced on: 20 PCG iterations (a tolerance out of reach) give the same residual history and the
    same iterate, bit for bit, with and without the exact-FMA instances."""
    rp, ci, v = problems.poisson3d(24)
    n = len(rp) - 1
    A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET, max_iter=20, tol=1e-300))
    assert A.level_double_sweep(0)["on"] and A.level_marching_ops(0)["on"] and A.level_box_exact_fma(0)
    b = np.random.default_rng(331).standard_normal(n)
    got = {}
    for mode in (1, 0, 1):
        A.set_box_exact_fma(mode)
        assert A.level_box_exact_fma(0) is bool(mode)
        x = np.zeros(n)
        hist, rc = A.solve("pcg", b, x)
        assert len(hist) >= 20 and hist[10] < 1e-3 * hist[0], (mode, rc, hist)
        if mode in got:
            assert _same_bits(got[mode][0], hist) and _same_bits(got[mode][1], x)  # (and a second run in mode 1 repeats the first)
        got[mode] = (hist, x)
    assert _same_bits(got[0][0], got[1][0]), np.flatnonzero(got[0][0] != got[1][0])
    assert _same_bits(got[0][1], got[1][1])
    A.close()
