"""The rule under which the box-grid kernels fuse the off-diagonal terms of their stencil sums (box_exact_offdiag, csrc/box_plan.cpp),
and the arithmetic claim behind it.  CPU only.

Rule: each of the six off-diagonal constants is 0.0 or finite with |c| = 2^k, k >= 0; the diagonal is not looked at.  Claim: for such
c the product c x is exact whenever it is finite, so sum + c x -- two IEEE operations -- rounds the exact value sum + c x once, which is
what fma(c, x, sum) does by definition: the two agree bit for bit wherever the unfused result is finite.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

DENORMAL = 5e-324 * 12345  # far below 2^-1022


def _stencil(off, diag=100.0):
    c = np.empty(7)
    c[[0, 1, 2, 4, 5, 6]] = off
    c[3] = diag
    return c


@pytest.mark.parametrize("value,expect", [
    (1.0, True), (-1.0, True), (2.0, True), (-2.0, True), (4.0, True), (-4.0, True), (2.0 ** 60, True), (-(2.0 ** 60), True), (0.0, True),
    (-0.0, True), (2.0 ** 1023, True),
    (0.5, False), (-0.5, False), (3.0, False), (6.0, False), (-1.5, False), (math.inf, False), (-math.inf, False), (math.nan, False),
    (DENORMAL, False), (-DENORMAL, False), (2.0 ** -1022, False), (1.0 + 2.0 ** -52, False),
])
def test_rule_on_one_value(value, expect):
    """The value in every off-diagonal position of an otherwise qualifying stencil, one position at a time and in all six."""
    assert sa.box_exact_offdiag(_stencil([value] * 6)) is expect
    for pos in range(6):
        off = [-1.0] * 6
        off[pos] = value
        assert sa.box_exact_offdiag(_stencil(off)) is expect, pos


def test_rule_mixed_signs_and_the_diagonal():
    assert sa.box_exact_offdiag(_stencil([-1.0, 2.0, -4.0, -1.0, -2.0, 4.0], 15.0))
    assert sa.box_exact_offdiag(_stencil([-1.0, 0.0, -4.0, 2.0 ** 60, -2.0, 0.0], 15.0))
    assert not sa.box_exact_offdiag(_stencil([-1.0, 2.0, -4.0, -1.0, -2.0, 3.0], 15.0))
    # the diagonal is not looked at
    for d in (6.0, 10.0, 0.5, 3.0, math.inf, math.nan, DENORMAL, 0.0):
        assert sa.box_exact_offdiag(_stencil([-1.0] * 6, d)), d
        assert not sa.box_exact_offdiag(_stencil([-0.5] * 6, d)), d
    with pytest.raises(ValueError):
        sa.box_exact_offdiag(np.ones(6))


def _box_stencil(rp, ci, v):
    """The seven constants (-plane, -line, -1, 0, +1, +line, +plane) of a CSR matrix that is one constant-coefficient 7-point stencil on
    a box in lexicographic order, else None."""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    off = ci.astype(np.int64) - rows
    offs = np.unique(off)
    if len(offs) != 7 or not np.array_equal(offs, -offs[::-1]) or offs[4] != 1:
        return None
    L, P = int(offs[5]), int(offs[6])
    if L < 2 or P % L or n % P:
        return None
    c = np.empty(7)
    for u, o in enumerate(offs):
        vals = np.unique(v[off == o])
        if len(vals) != 1:
            return None
        c[u] = vals[0]
    return c, (L, P // L, n // P)


def test_benchmark_hierarchy_qualifies_on_every_box_level():
    """The benchmark's operator at 24^3 through the host setup: every level that is a box grid carries off-diagonal constants -1, -2
    or -4 (edge counts between aggregates of a uniform grid: products of the aggregates' extents) and so satisfies the rule."""
    rp, ci, v = problems.poisson3d(24)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(print_setup=0), host_only=True)
    boxes = 0
    for l in range(A.nlevels):
        lrp, lci, lv, _ = A.level_csr(l, "A")
        st = _box_stencil(lrp, lci, lv)
        if st is None:
            print(f"level {l}: {len(lrp) - 1} rows, not one constant 7-point stencil on a box")
            continue
        c, grid = st
        print(f"level {l}: box {grid}, constants {c.tolist()}")
        boxes += 1
        off = c[[0, 1, 2, 4, 5, 6]]
        assert set(off.tolist()) <= {-1.0, -2.0, -4.0}, (l, c)
        assert sa.box_exact_offdiag(c), (l, c)
        if l == 0:
            assert grid == (24, 24, 24) and np.array_equal(c, [-1, -1, -1, 6, -1, -1, -1])
        if l == 1:  # one pairing: -1 along the paired axis, -2 across it, diagonal 6 + 6 - 2
            assert sorted(off.tolist()) == [-2.0, -2.0, -2.0, -2.0, -1.0, -1.0] and c[3] == 10.0, c
    assert boxes >= 2
    A.close()


def _patterns(rng, n):
    """n pairs (x, sum) of fp64 bit patterns: a third uniform over all patterns (every exponent, NaNs and infinities included), a third
    with x within 2^+-70 of sum (the additions that round), a third of that with one or both operands denormal or near the overflow edge."""
    bits = rng.integers(0, 2 ** 64, size=2 * n, dtype=np.uint64)
    x, s = bits[:n].copy(), bits[n:].copy()
    k = n // 3
    sexp = (s[k:] >> np.uint64(52)) & np.uint64(0x7ff)
    near = np.clip(sexp.astype(np.int64) + rng.integers(-70, 71, size=n - k), 0, 2046).astype(np.uint64)
    x[k:] = (x[k:] & np.uint64(0x800fffffffffffff)) | (near << np.uint64(52))
    m = 2 * k
    third = (n - m) // 3
    x[m:m + third] &= np.uint64(0x800fffffffffffff)                      # x denormal
    s[m + third:m + 2 * third] &= np.uint64(0x800fffffffffffff)          # sum denormal
    x[m + third:m + 2 * third] &= np.uint64(0x803fffffffffffff)          # ... and x within 4 binades of it
    top = np.uint64(0x7fd) << np.uint64(52)
    x[m + 2 * third:] = (x[m + 2 * third:] & np.uint64(0x800fffffffffffff)) | (np.uint64(0x7f0) << np.uint64(52))  # c x near / past overflow
    s[m + 2 * third:] = (s[m + 2 * third:] & np.uint64(0x800fffffffffffff)) | top
    return x.view(np.float64), s.view(np.float64)


def _round_exact(c, x, s):
    """sum + c x computed exactly and rounded once, to nearest even (float() of a Fraction is correctly rounded)."""
    return float(Fraction(s) + Fraction(c) * Fraction(x))


@pytest.mark.parametrize("mag", [1.0, 2.0, 4.0, 2.0 ** 10])
def test_unfused_sum_is_the_correctly_rounded_exact_value(mag):
    """10^6 patterns per coefficient.  On all of them: where c x is finite, (c x) / c gives back x's bits -- the product was not rounded
    (a rounded or flushed product cannot map back to x) -- so the IEEE addition that follows rounds the exact sum + c x once.  On a
    sample, independently: the unfused result equals the exact rational value rounded once, and math.fma's where Python has it."""
    rng = np.random.default_rng(int(mag))
    x, s = _patterns(rng, 1_000_000)
    assert (np.abs(x[np.isfinite(x)]) < 2.0 ** -1022).sum() > 50_000  # the denormals are there
    for c in (mag, -mag):
        with np.errstate(all="ignore"):
            p = c * x
            unfused = s + p
            back = p / c
        fin = np.isfinite(unfused)
        assert fin.sum() > 500_000
        assert np.all(np.isfinite(p[fin]))
        assert np.array_equal(back[fin].view(np.uint64), x[fin].view(np.uint64))
        idx = np.flatnonzero(fin)
        sample = idx[::len(idx) // 6000]  # every group of _patterns in proportion
        for i in sample:
            want = _round_exact(c, float(x[i]), float(s[i]))
            got = float(unfused[i])
            assert got == want, (c, x[i], s[i], got, want)
            if hasattr(math, "fma"):
                f = math.fma(c, float(x[i]), float(s[i]))
                assert np.float64(f).view(np.uint64) == np.float64(got).view(np.uint64), (c, x[i], s[i])


def test_a_coefficient_below_one_is_not_exact():
    """Why 0.5 does not qualify: its product with the smallest denormal is rounded (to zero), and the fused and unfused sums differ."""
    x, s = 5e-324, 5e-324
    assert 0.5 * x == 0.0
    assert s + 0.5 * x == 5e-324
    assert _round_exact(0.5, x, s) == 1e-323  # 1.5 denormal steps round to the even neighbour: 2 steps
