"""The eight kernels of the opt-in float V-cycle (precond_fp32 = 1), one step at a time and bit for bit.  GPU box only.

sdia_f32_kernel / csr_f32_kernel (sweep and residual), csr_rows_f32_kernel (restriction, and prolongation through a general P),
prolong_agg_f32_kernel, jacobi_zero_f32_kernel, gemv_f32_kernel, cvt_d2f_kernel and cvt_f2d_dot_kernel are reached through
sparsh_op_*_f32, which call the engine functions Engine::vcycle_f32 is made of.  The reference is F32Ref of test_fp32_ops_host.py:
numpy float32, every product, sum and quotient rounded once and in the kernels' order -- what the device computes too, since the
library is built without contraction, the float division is the IEEE sequence and float denormals are kept.  The same class run
in float64 equals the CPU oracle bit for bit (test_fp32_ops_host.py), and the inputs reach every tail of the slot loop, both
layouts, ragged last slices and coarsest levels of fewer than 64 rows (ibid.).  Every comparison is exact unless it says otherwise.
"""
import functools
import math

import numpy as np
import pytest

import sparsh_amg_amd as sa
from test_fp32_ops_host import CASES, IDS, F32Ref, case_params, host_handle, matrix, predict_layout, vectors

pytestmark = pytest.mark.gpu

FACTORED = [("poisson3d", "hem", "nd"), ("poisson2d", "beck", "bt"), ("banded19_s9", "beck", "nd")]  # coarsest levels of 156, 265, 275 rows
FACTORED_IDS = [f"{n}-{c}-{f}" for n, c, f in FACTORED]


def handle(name, coarsening, form=None):
    """device handle with the float hierarchy; form: the coarsest level factored on the device (dense_limit below its rows)"""
    return _handle(name, coarsening, form)


@functools.lru_cache(maxsize=None)
def _handle(name, coarsening, form):
    A = sa.sp_matrix_mg(*matrix(name))
    if form:
        A.set_coarse_form(form)
    return A.setup(case_params(coarsening, precond_fp32=1, **(dict(dense_limit=100) if form else {})))


@functools.lru_cache(maxsize=None)
def reference(name, coarsening):
    return F32Ref(host_handle(name, coarsening), np.float32)


def same_bits(a, b):
    """bit patterns, so that -0.0 / 0.0 and the infinities count too"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                                                                         b.view(np.uint32 if b.dtype == np.float32 else np.uint64))


@pytest.mark.parametrize("name,coarsening", CASES, ids=IDS)
def test_level_steps_are_bitwise_the_float_restatement(name, coarsening):
    A, ref = handle(name, coarsening), reference(name, coarsening)
    H = host_handle(name, coarsening)
    assert A.nlevels == H.nlevels == ref.nlevels
    assert A.level_f32_layout(A.nlevels - 1) is None
    for l in range(A.nlevels - 1):
        n, nc = ref.n[l], ref.n[l + 1]
        assert A.level_info(l)["nrow"] == n
        assert A.level_f32_layout(l) == predict_layout(H, l)[0], (name, coarsening, l)
        for k, (b, x) in enumerate(vectors(n, np.float32, 200 + l)):
            tag = (name, coarsening, l, A.level_f32_layout(l), k)
            xc = vectors(nc, np.float32, 300 + l)[k][1]
            assert np.array_equal(A.op_residual_f32(l, b, x), ref.residual(l, b, x)), tag
            for sweeps in (1, 2, 3):
                assert np.array_equal(A.op_jacobi_f32(l, b, x, sweeps), ref.jacobi(l, b, x, sweeps)), tag + (sweeps,)
            assert np.array_equal(A.op_jacobi_f32(l, b, x, 1, x_is_zero=True), ref.zero_sweep(l, b)), tag
            assert np.array_equal(A.op_jacobi_f32(l, b, x, 3, x_is_zero=True), ref.jacobi(l, b, None, 3, x_is_zero=True)), tag
            assert np.array_equal(A.op_restrict_f32(l, x), ref.restrict(l, x)), tag
            assert np.array_equal(A.op_prolong_f32(l, xc, x), ref.prolong(l, xc, x)), tag
        assert same_bits(A.op_jacobi_f32(l, b, x, 0), x) and same_bits(A.op_jacobi_f32(l, b, x, 0, x_is_zero=True), np.zeros_like(x))
    with pytest.raises(sa.SparshError) as e:
        A.op_jacobi_f32(0, b[:1], x[:1], -1)
    assert e.value.code == sa.SPARSH_EINVAL


@pytest.mark.parametrize("name,coarsening", CASES, ids=IDS)
def test_coarse_gemv_is_bitwise_lane_sums_and_shuffle_tree(name, coarsening):
    """gemv_f32_kernel on coarsest levels of 16 .. 289 rows: fewer columns than lanes (16, 23, 50, 58, 59), a ragged last pass"""
    A, ref = handle(name, coarsening), reference(name, coarsening)
    n = ref.n[-1]
    assert A.coarse_info()["dense"] and ref.inv.shape == (n, n)
    for k, (b, _) in enumerate(vectors(n, np.float32, 400)):
        got, want = A.op_coarse_f32(b), ref.gemv(b)
        assert np.array_equal(got, want), (name, coarsening, n, k, np.abs(got - want).max())


@pytest.mark.parametrize("name,coarsening,form", FACTORED, ids=FACTORED_IDS)
def test_factored_coarse_solve_is_the_fp64_solve_between_two_conversions(name, coarsening, form):
    A = handle(name, coarsening, form)
    info = A.coarse_info()
    assert not info["dense"] and info["form"] == ("nested_dissection" if form == "nd" else "block_tridiagonal")
    n = info["rows"]
    assert n == reference(name, coarsening).n[-1]
    for k, (b, _) in enumerate(vectors(n, np.float32, 500)):
        with np.errstate(over="ignore", under="ignore"):
            want = A.op_coarse(b.astype(np.float64)).astype(np.float32)
        assert np.array_equal(A.op_coarse_f32(b), want), (name, form, k)


# ---------------------------------------------------------------------------------------------------------------- conversions
def tie_cases(rng, count):
    """doubles exactly half way between two neighbouring floats, and the float round-to-nearest-even picks (the even bit pattern)"""
    lo = rng.integers(0x00800000, 0x7F000000, size=count, dtype=np.uint32)  # normal, finite, well below the largest
    lo[::2] &= ~np.uint32(1)   # lower neighbour even: the tie goes down
    lo[1::2] |= np.uint32(1)   # lower neighbour odd: the tie goes up
    hi = lo + np.uint32(1)
    mid = (lo.view(np.float32).astype(np.float64) + hi.view(np.float32).astype(np.float64)) / 2.0
    want = np.where(lo & 1, hi, lo).astype(np.uint32)
    sign = rng.random(count) < 0.5
    return np.where(sign, -mid, mid), np.where(sign, want | np.uint32(0x80000000), want).astype(np.uint32)


FLT_MAX = float(np.finfo(np.float32).max)
# value, bit pattern of (float)value
SPECIAL = [(1e39, 0x7F800000), (-1e39, 0xFF800000), (1e-40, int(np.float32(1e-40).view(np.uint32))), (-1e-40, int(np.float32(-1e-40).view(np.uint32))),
           (1e-46, 0x00000000), (-1e-46, 0x80000000), (0.0, 0x00000000), (-0.0, 0x80000000),
           (FLT_MAX, 0x7F7FFFFF), ((FLT_MAX + 2.0 ** 128) / 2.0, 0x7F800000),             # the tie above the largest float goes to infinity
           (float(np.nextafter((FLT_MAX + 2.0 ** 128) / 2.0, 0.0)), 0x7F7FFFFF),
           (2.0 ** -149, 0x00000001), (2.0 ** -150, 0x00000000), (1.5 * 2.0 ** -149, 0x00000002),  # denormal ties: to the even neighbour
           (float(np.nextafter(2.0 ** -150, 1.0)), 0x00000001), (2.0 ** -126, 0x00800000),
           (float(np.nextafter(2.0 ** -126, 0.0)), 0x00800000), (1.0 + 2.0 ** -24, 0x3F800000), (1.0 + 3 * 2.0 ** -24, 0x3F800002)]
CVT_SIZES = [1, 255, 256, 257, 1025, 100003]


def conversion_data(n, seed):
    """n doubles with the ties and special values at random places, and the bit patterns of their floats"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, size=n)
    want = x.astype(np.float32).view(np.uint32).copy()
    tv, tw = tie_cases(rng, 64)
    sv = np.concatenate([[v for v, _ in SPECIAL], tv])
    sw = np.concatenate([np.array([w for _, w in SPECIAL], dtype=np.uint32), tw])
    m = min(n, len(sv))
    pick = rng.permutation(len(sv))[:m] if n < len(sv) else np.arange(len(sv))
    at = rng.choice(n, size=m, replace=False)
    x[at], want[at] = sv[pick], sw[pick]
    return x, want


@pytest.mark.parametrize("n", CVT_SIZES)
def test_cvt_d2f_rounds_to_nearest_even_overflows_and_keeps_denormals_and_signs(n):
    A = handle("poisson2d", "hem")
    for seed in range(4 if n < 300 else 1):  # (the short ones draw other special values each time)
        x, want = conversion_data(n, 1000 * n + seed)
        got = A.op_cvt_f32(x)
        assert got.dtype == np.float32
        bad = np.nonzero(got.view(np.uint32) != want)[0]
        assert len(bad) == 0, (n, seed, [(x[i].hex(), hex(got.view(np.uint32)[i]), hex(want[i])) for i in bad[:5]])
        with np.errstate(over="ignore", under="ignore"):
            assert same_bits(got, x.astype(np.float32))  # (numpy's own conversion says the same)


@pytest.mark.parametrize("n", CVT_SIZES)
def test_cvt_f2d_dot_widens_exactly_and_sums_to_rounding(n):
    A = handle("poisson2d", "hem")
    x, want = conversion_data(n, 77 * n)
    z32 = want.view(np.float32)
    rng = np.random.default_rng(n)
    r = rng.standard_normal(n)
    z, _ = A.op_cvt_f2d_dot(z32, r)  # (infinities among z32: the sum is not a number, the widening is still exact)
    assert same_bits(z, z32.astype(np.float64))
    z32 = np.where(np.isfinite(z32), z32, np.float32(1.0))
    z, dot = A.op_cvt_f2d_dot(z32, r)
    assert same_bits(z, z32.astype(np.float64))
    exact = math.fsum(float(a) * float(b) for a, b in zip(z, r))  # (each product rounded, as the kernel's: the bound covers it)
    scale = float(np.abs(z * r).sum())
    print(n, "dot: error / sum |z_i r_i| =", abs(dot - exact) / scale if scale else 0.0)
    assert abs(dot - exact) <= 1e-13 * scale


# ---------------------------------------------------------------------------------------------------------------- the whole cycle
def composed_cycle(A, r, nu):
    """Engine::vcycle_f32 from the operator entry points, in its order (Single.cycle of test_gpu_multi_rhs.py); returns (z, z . r)"""
    last = A.nlevels - 1
    bs, xs = [A.op_cvt_f32(r)], []
    for l in range(last):
        xs.append(A.op_jacobi_f32(l, bs[l], np.zeros_like(bs[l]), nu, x_is_zero=True))
        bs.append(A.op_restrict_f32(l, A.op_residual_f32(l, bs[l], xs[l])))
    xc = A.op_coarse_f32(bs[last])
    for l in range(last, 0, -1):
        xc = A.op_jacobi_f32(l - 1, bs[l - 1], A.op_prolong_f32(l - 1, xc, xs[l - 1]), nu)
    return A.op_cvt_f2d_dot(xc, r)


@pytest.mark.parametrize("form", [None, "nd"], ids=["dense", "factored"])
@pytest.mark.parametrize("coarsening", ["hem", "beck"])
def test_op_precond_f32_is_bitwise_the_composed_cycle(coarsening, form):
    name = "poisson3d" if form is None or coarsening == "hem" else "poisson2d"  # (Beck leaves poisson3d 59 rows: nothing to factor)
    A = handle(name, coarsening, form)
    assert A.coarse_info()["dense"] == (form is None)
    ref = reference(name, coarsening)
    rng = np.random.default_rng(31)
    r = rng.standard_normal(A.nrow)
    try:
        for nu in (1, 2, 7):
            A.set_smoother("jacobi", nu)
            z = A.op_precond_f32(r)
            want, dot = composed_cycle(A, r, nu)
            assert same_bits(z, want), (coarsening, form, nu, np.abs(z - want).max())
            assert same_bits(A.op_precond_f32(r), z), (coarsening, form, nu)  # (an odd number of x / x2 swaps persists across the calls)
            assert same_bits(A.op_precond(r), z)                              # what the Krylov loops apply
            assert abs(dot - math.fsum(z * r)) <= 1e-13 * float(np.abs(z * r).sum())
            if form is None:  # the restatement alone, from cvt to cvt
                with np.errstate(over="ignore", under="ignore"):
                    assert same_bits(z, ref.cycle(r.astype(np.float32), nu).astype(np.float64)), (coarsening, nu)
    finally:
        A.set_smoother("jacobi", 0)


# ---------------------------------------------------------------------------------------------------------------- solves
def test_solves_with_the_float_cycle_over_a_general_prolongator():
    """Beck's coarsening under precond_fp32: csr_rows_f32_kernel as prolongation and as restriction through rows of 4-6 entries inside
    AMG-PCG and AMG-BiCGStab.  Same promises as test_fp32_preconditioner_mode (tests/test_gpu_configs.py): return code 0, true residual
    within 5e-8, at most 3 iterations more than with the fp64 cycle.  Measured on the MI355X (fp32 / fp64 cycle): pcg 6 / 6 iterations,
    pbicg 3 / 3, true residuals 1.1e-9 and 3.7e-9 -- no excess at all, so the +3 of that test is kept as the margin."""
    import scipy.sparse as sp

    rp, ci, v = matrix("poisson3d")
    n = len(rp) - 1
    S = sp.csr_matrix((v, ci, rp), shape=(n, n))
    b = np.ones(n)
    A32 = handle("poisson3d", "beck")
    A64 = sa.sp_matrix_mg(rp, ci, v).setup(case_params("beck"))
    assert max(np.diff(A32.level_csr(l, "R")[0]).max() for l in range(A32.nlevels - 1)) >= 4
    try:
        for method in ("pcg", "pbicg"):
            x32, x64 = np.zeros(n), np.zeros(n)
            h32, rc32 = A32.solve(method, b, x32)
            h64, rc64 = A64.solve(method, b, x64)
            res = np.linalg.norm(b - S @ x32)
            print(method, "iterations fp32 / fp64 cycle:", len(h32), "/", len(h64), "true residual:", res)
            assert rc32 == 0 and rc64 == 0, method
            assert res <= 5e-8, (method, res)
            assert len(h32) <= len(h64) + 3, (method, len(h32), len(h64))
            assert np.linalg.norm(x32 - x64) <= 1e-7 * np.linalg.norm(x64), method
    finally:
        A64.close()


def test_refusals_on_the_device():
    rp, ci, v = matrix("poisson2d")
    plain = sa.sp_matrix_mg(rp, ci, v).setup(case_params("hem"))  # no precond_fp32
    try:
        f = np.zeros(plain.nrow, dtype=np.float32)
        calls = [lambda: plain.level_f32_layout(0), lambda: plain.op_jacobi_f32(0, f, f, 1), lambda: plain.op_residual_f32(0, f, f),
                 lambda: plain.op_restrict_f32(0, f), lambda: plain.op_prolong_f32(0, f[:plain.level_info(1)["nrow"]], f),
                 lambda: plain.op_coarse_f32(f[:plain.level_info(plain.nlevels - 1)["nrow"]]), lambda: plain.op_cvt_f32(np.zeros(3)),
                 lambda: plain.op_cvt_f2d_dot(f[:3], np.zeros(3))]
        for call in calls:
            with pytest.raises(sa.SparshError) as e:
                call()
            assert e.value.code == sa.SPARSH_ESTATE and "fp32 preconditioner hierarchy was not built" in str(e.value)
    finally:
        plain.close()
    A = handle("poisson2d", "hem")
    f = np.zeros(A.nrow, dtype=np.float32)
    for level, what in ((-1, "level out of range"), (A.nlevels, "level out of range"), (A.nlevels - 1, "coarsest level has no float operator")):
        for call in (lambda: A.op_jacobi_f32(level, f, f, 1), lambda: A.op_residual_f32(level, f, f),
                     lambda: sa._check(sa.lib.sparsh_op_restrict_f32(A._h, level, sa._fp(f), sa._fp(f.copy()))),
                     lambda: sa._check(sa.lib.sparsh_op_prolong_f32(A._h, level, sa._fp(f), sa._fp(f.copy())))):
            with pytest.raises(sa.SparshError) as e:
                call()
            assert e.value.code == sa.SPARSH_EINVAL and what in str(e.value), (level, str(e.value))
    with pytest.raises(sa.SparshError) as e:
        A.op_cvt_f32(np.zeros(0))
    assert e.value.code == sa.SPARSH_EINVAL
