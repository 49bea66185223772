"""The single-vector Krylov kernels at the end of kernels.hip and finalize_kernel, one launch at a time against the numpy restatement
(tests/krylov_ops_restatement.py, anchored on the oracle by tests/test_krylov_ops_host.py): stored vectors and partial sums bit for
bit, nothing written behind the end, every finalize code, both reduction batches of fin_strided_sum, the history slot under the
device counter, modes 1 + 2 -- and the loops built from them under check_every > 1 and under the benchmark's stepping protocol."""
import math

import numpy as np
import pytest

import krylov_ops_restatement as kr
import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import load_c0

pytestmark = pytest.mark.gpu
QUIET = dict(print_setup=0, print_solve=0)
TOL = 1e-8

# 1 048 576 is the last n below the grid's cap of 2048 workgroups; from there on every thread takes more than two terms
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 123457, 1048576, 1048577, 3145733]
NBLKS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 4096, 20479, 20480, 20481, 39366, 40961]
NBLK_PAIRS = [(391, 2048), (39366, 2048), (1, 1025)]  # (nblk of z.r from the cycle's last launch, nblk1 of r.r from the update)
S = kr.S


@pytest.fixture(scope="module")
def A():
    rp, ci, v = problems.poisson2d(30)
    return sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))


def same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# Distance allowed between a square root stored by finalize_kernel and math.sqrt of the same argument.  Measured on an MI355X by
# test_finalize_codes (see its docstring): 0 ulp everywhere, so square roots are held to equality like everything else.
SQRT_ULPS = 0


def ulps(a, b):
    a, b = np.float64(a), np.float64(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if (np.isnan(a) and np.isnan(b)) else 1 << 62
    return abs(int(a.view(np.int64)) - int(b.view(np.int64)))


def near(a, b):
    """arrays that may hold square roots: every element within SQRT_ULPS of the restatement (0: the same bits)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and all(ulps(u, v) <= SQRT_ULPS for u, v in zip(a, b))


def clean(res):
    """nothing written behind the logical end of any array the launch wrote"""
    return all(np.all(t == sa.OP_SENTINEL) for t in res["tails"].values())


def normal(n, count, seed):
    rng = np.random.default_rng([n, seed])
    return [rng.standard_normal(n) for _ in range(count)]


def integers(n, count, seed, lim=50):
    rng = np.random.default_rng([n, seed])
    return [rng.integers(-lim, lim + 1, n).astype(np.float64) for _ in range(count)]


# ---------------------------------------------------------------------------------------------------------------- vector kernels

@pytest.mark.parametrize("n", SIZES)
def test_dot2(A, n):
    a, b, c, d = normal(n, 4, 1)
    res = A.op_dot2(a, b, c, d)
    p0, p1 = kr.dot2(a, b, c, d)
    assert res["nblk"] == kr.ew_grid(n) and clean(res)
    assert same_bits(res["p0"], p0) and same_bits(res["p1"], p1)
    res = A.op_dot2(a, b, a, a)  # BiCGStab's As.s and As.As: one device vector three times
    p0, p1 = kr.dot2(a, b, a, a)
    assert res["nblk"] == kr.ew_grid(n) and clean(res) and same_bits(res["p0"], p0) and same_bits(res["p1"], p1)


@pytest.mark.parametrize("n", SIZES)
def test_cg_update(A, n):
    p, Ap, x, r = normal(n, 4, 2)
    alpha = 0.37251846
    for with_x in (True, False):
        res = A.op_cg_update(alpha, p, Ap, x if with_x else None, r)
        xn, rn, part = kr.cg_update(alpha, -alpha, p, Ap, x if with_x else None, r)
        assert res["nblk"] == kr.ew_grid(n) and clean(res)
        assert same_bits(res["r"], rn) and same_bits(res["partial"], part)
        assert same_bits(res["x"], xn) if with_x else res["x"] is None
    # the pair (alpha, nalpha) goes in as given: any nalpha, not a negation made on the way
    res = A.op_cg_update(alpha, p, Ap, x, r, nalpha=-0.6180339)
    xn, rn, part = kr.cg_update(alpha, -0.6180339, p, Ap, x, r)
    assert same_bits(res["x"], xn) and same_bits(res["r"], rn) and same_bits(res["partial"], part)


@pytest.mark.parametrize("n", SIZES)
def test_cg_update_zero(A, n):
    """cg_update_zero_kernel<NT>: a diagonal array or the constant, nt 0 and 1, with and without x -- against the restatement, and
    the four variants of one diagonal against each other."""
    p, Ap, x, r, d = normal(n, 5, 3)
    d = 2.0 + np.abs(d)
    alpha, omega, dconst = 0.81330514, 0.66667, 6.0
    for diag in (d, None, np.full(n, dconst)):
        xn, rn, z0, part = kr.cg_update_zero(alpha, -alpha, p, Ap, x, r, diag, dconst, omega)
        for nt in (False, True):
            for with_x in (True, False):
                res = A.op_cg_update(alpha, p, Ap, x if with_x else None, r, zero=True, d=diag, dconst=dconst, omega=omega, nt=nt)
                assert res["nblk"] == kr.ew_grid(n) and clean(res), (nt, with_x)
                assert same_bits(res["r"], rn) and same_bits(res["z0"], z0) and same_bits(res["partial"], part), (nt, with_x)
                assert same_bits(res["x"], xn) if with_x else res["x"] is None
    # (the constant as an array and as dconst were both compared with their own restatement; these are the same numbers)
    assert same_bits(kr.cg_update_zero(alpha, -alpha, p, Ap, x, r, None, dconst, omega)[2],
                     kr.cg_update_zero(alpha, -alpha, p, Ap, x, r, np.full(n, dconst), dconst, omega)[2])
    # the plain kernel leaves the same x, r and partial sums
    res = A.op_cg_update(alpha, p, Ap, x, r)
    assert same_bits(res["x"], xn) and same_bits(res["r"], rn) and same_bits(res["partial"], part)


@pytest.mark.parametrize("n", SIZES)
def test_p_and_xp_update(A, n):
    p, Ap, x, r = normal(n, 4, 4)
    alpha, beta = 0.45017332, 0.2718281
    # CG: z is r, the vector the update left
    upd = A.op_cg_update(alpha, p, Ap, x, r)
    z = upd["r"]
    pu = A.op_p_update(beta, z, p)
    assert clean(pu) and same_bits(pu["p"], kr.p_update(beta, z, p))
    # PCG with the deferred x: xp_update gives the x and p of cg_update-with-x followed by p_update
    z = normal(n, 1, 5)[0]
    xp = A.op_xp_update(alpha, beta, z, p, x)
    xn, pn = kr.xp_update(alpha, beta, z, p, x)
    assert clean(xp) and same_bits(xp["x"], xn) and same_bits(xp["p"], pn)
    pu = A.op_p_update(beta, z, p)
    assert same_bits(xp["x"], upd["x"]) and same_bits(xp["p"], pu["p"])


@pytest.mark.parametrize("n", SIZES)
def test_bicg_kernels(A, n):
    r, Ap, p1, s1, As, r0, x, p = normal(n, 8, 6)
    alpha, omega1, beta = 0.3141592, 0.7071067, 1.4142135
    s = A.op_bicg_s(alpha, r, Ap)
    assert clean(s) and same_bits(s["s"], kr.bicg_s(alpha, r, Ap))
    s = s["s"]
    xr = A.op_bicg_xr(alpha, omega1, p1, s1, s, As, r0, x, r)
    xn, rn, q0, q1 = kr.bicg_xr(alpha, omega1, p1, s1, s, As, r0, x)
    assert xr["nblk"] == kr.ew_grid(n) and clean(xr)
    assert same_bits(xr["x"], xn) and same_bits(xr["r"], rn) and same_bits(xr["q0"], q0) and same_bits(xr["q1"], q1)
    # without a preconditioner p1 is p and s1 is s: one device vector each
    xr = A.op_bicg_xr(alpha, omega1, p, s, s, As, r0, x, r)
    xn, rn, q0, q1 = kr.bicg_xr(alpha, omega1, p, s, s, As, r0, x)
    assert clean(xr) and same_bits(xr["x"], xn) and same_bits(xr["r"], rn) and same_bits(xr["q0"], q0) and same_bits(xr["q1"], q1)
    pn = A.op_bicg_p(beta, omega1, rn, Ap, p)
    assert clean(pn) and same_bits(pn["p"], kr.bicg_p(beta, omega1, rn, Ap, p))


@pytest.mark.parametrize("n", [1000, 123457, 3145733])
def test_integer_data(A, n):
    """Integer-valued data of mixed sign, integer coefficients: every product and sum is exact, so each partial sum is math.fsum over
    the elements its workgroup owns -- whatever the order -- and the kernels must still agree with the restatement."""
    p, Ap, x, r, z, r0 = integers(n, 6, 7)
    g = kr.ew_grid(n)
    owner = (np.arange(n) // kr.K_BLOCK) % g
    some = sorted({0, 1 % g, g // 2, g - 1})

    def exact(part, terms):
        return all(part[w] == math.fsum(terms[owner == w]) for w in some) and math.fsum(part) == math.fsum(terms)

    res = A.op_dot2(p, Ap, x, x)
    assert clean(res) and exact(res["p0"], p * Ap) and exact(res["p1"], x * x)
    assert same_bits(res["p0"], kr.dot2(p, Ap, x, x)[0])
    res = A.op_cg_update(3.0, p, Ap, x, r)
    assert clean(res) and np.array_equal(res["x"], x + 3.0 * p) and np.array_equal(res["r"], r - 3.0 * Ap)
    assert exact(res["partial"], res["r"] * res["r"]) and same_bits(res["partial"], kr.cg_update(3.0, -3.0, p, Ap, x, r)[2])
    d = 1.0 + np.abs(z)
    resz = A.op_cg_update(3.0, p, Ap, None, r, zero=True, d=d, omega=2.0, nt=True)
    assert clean(resz) and np.array_equal(resz["r"], res["r"]) and same_bits(resz["z0"], (2.0 * res["r"]) / d)
    assert exact(resz["partial"], res["r"] * res["r"])
    assert np.array_equal(A.op_p_update(-2.0, z, p)["p"], z - 2.0 * p)
    res = A.op_xp_update(3.0, -2.0, z, p, x)
    assert clean(res) and np.array_equal(res["x"], x + 3.0 * p) and np.array_equal(res["p"], z - 2.0 * p)
    s = A.op_bicg_s(3.0, r, Ap)
    assert clean(s) and np.array_equal(s["s"], r - 3.0 * Ap)
    res = A.op_bicg_xr(3.0, -2.0, p, z, s["s"], Ap, r0, x, r)
    rn = s["s"] + 2.0 * Ap
    assert clean(res) and np.array_equal(res["x"], x + 3.0 * p - 2.0 * z) and np.array_equal(res["r"], rn)
    assert exact(res["q0"], rn * r0) and exact(res["q1"], rn * rn)
    res = A.op_bicg_p(-2.0, 3.0, r, Ap, p)
    assert clean(res) and np.array_equal(res["p"], r - 2.0 * (p - 3.0 * Ap))


# ---------------------------------------------------------------------------------------------------------------- finalize: sums

def random_block(seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, kr.S_COUNT)


def check_sums(A, p0, p1, exact):
    """FIN_STORE into a slot and FIN_PCG_BETA_RES on (p0, p1): the restatement bit for bit; exact: the sums are math.fsum"""
    base = random_block(len(p0))
    res = A.op_finalize(kr.FIN_STORE, p0, None, base, S["TMP"])
    ref, _, _ = kr.finalize(kr.FIN_STORE, p0, None, base, S["TMP"])
    assert same_bits(res["scal"], ref) and res["counter"] == 0
    if exact:
        assert res["scal"][S["TMP"]] == math.fsum(p0)
    hist = np.full(3, -1.0)
    res = A.op_finalize(kr.FIN_PCG_BETA_RES, p0, p1, base, 0, hist=hist, it=1)
    ref, h, _ = kr.finalize(kr.FIN_PCG_BETA_RES, p0, p1, base, 0, hist, 1)
    rest = [k for k in range(kr.S_COUNT) if k != S["RES"]]
    assert clean(res) and same_bits(res["scal"][rest], ref[rest]) and near(res["scal"][S["RES"]], ref[S["RES"]])
    assert same_bits(res["hist"][1], res["scal"][S["RES"]]) and same_bits(res["hist"][[0, 2]], hist[[0, 2]])
    if exact:
        assert res["scal"][S["ZR"]] == math.fsum(p0) and near(res["scal"][S["RES"]], math.sqrt(math.fsum(p1)))


@pytest.mark.parametrize("nblk", NBLKS)
def test_finalize_sums(A, nblk):
    """fin_strided_sum<20>: counts that leave the 20-wide batch partly empty (<= 1024: only u = 0 in range), fill it exactly
    (20 480), start a second round (20 481, 39 366 = the 216^3 benchmark, 40 961 = a third)"""
    rng = np.random.default_rng(nblk)
    ints = rng.integers(-10 ** 6, 10 ** 6 + 1, nblk).astype(np.float64)
    squares = rng.integers(0, 10 ** 6, nblk).astype(np.float64)  # (r.r partials are sums of squares: not negative)
    check_sums(A, ints, squares, exact=True)
    check_sums(A, rng.standard_normal(nblk), rng.standard_normal(nblk) ** 2, exact=False)


@pytest.mark.parametrize("nblk,nblk1", NBLK_PAIRS)
def test_finalize_sums_of_two_lengths(A, nblk, nblk1):
    """FIN_PCG_BETA_RES with z.r from the cycle's last launch and r.r from the update: two counts"""
    rng = np.random.default_rng([nblk, nblk1])
    check_sums(A, rng.integers(-10 ** 6, 10 ** 6 + 1, nblk).astype(np.float64), rng.integers(0, 10 ** 6, nblk1).astype(np.float64), exact=True)
    check_sums(A, rng.standard_normal(nblk), rng.standard_normal(nblk1) ** 2, exact=False)
    # a marked element at the end of the longer array must count: the second sum runs to its own length
    p0, p1 = np.ones(nblk), np.zeros(nblk1)
    p1[-1] = 9.0
    res = A.op_finalize(kr.FIN_PCG_BETA_RES, p0, p1, random_block(1), 0)
    assert res["scal"][S["ZR"]] == float(nblk) and res["scal"][S["RES"]] == 3.0


@pytest.mark.parametrize("nblk", [1, 1025, 39366])
def test_finalize_modes_1_and_2(A, nblk):
    """multi-GPU path without the all-reduce: mode 1 leaves the sums in S_SUM0 / S_SUM1 and nothing else, mode 2 applies the code to
    them -- together the scalar block and the history of mode 0, bit for bit, for every code"""
    rng = np.random.default_rng(nblk)
    p0, p1 = rng.standard_normal(nblk), rng.standard_normal(max(1, nblk // 2)) ** 2
    keep = [k for k in range(kr.S_COUNT) if kr.SLOTS[k] not in ("SUM0", "SUM1")]
    for code in range(11):
        base = random_block(100 + code)
        hist = np.full(4, -1.0)
        m0 = A.op_finalize(code, p0, p1, base, S["TMP"], hist=hist, it=2)
        m1 = A.op_finalize(code, p0, p1, base, S["TMP"], mode=1, hist=hist, it=-1, counter=1)
        ref1, _, _ = kr.finalize(code, p0, p1, base, S["TMP"], hist, -1, 1, mode=1)
        assert same_bits(m1["scal"], ref1) and same_bits(m1["scal"][keep], base[keep]), kr.FIN_NAMES[code]
        assert same_bits(m1["hist"], hist) and m1["counter"] == 1 and clean(m1)  # mode 1 takes no slot
        assert m1["scal"][S["SUM0"]] == kr.fin_sum(p0) and m1["scal"][S["SUM1"]] == kr.fin_sum(p1)
        m2 = A.op_finalize(code, None, None, m1["scal"], S["TMP"], mode=2, hist=hist, it=2)
        assert same_bits(m2["scal"][keep], m0["scal"][keep]) and same_bits(m2["hist"], m0["hist"]) and clean(m2), kr.FIN_NAMES[code]
        ref2, h2, _ = kr.finalize(code, None, None, ref1, S["TMP"], hist, 2, 0, mode=2)
        assert near(m2["scal"], ref2) and near(m2["hist"], h2)


# ---------------------------------------------------------------------------------------------------------------- finalize: codes

def check_code(A, code, p0, p1, base, slot, worst):
    """One launch of `code`: slots made of sums, products, quotients and negation equal the restatement bit for bit; slots the code
    does not write are unchanged; square roots are held against math.sqrt of the restated argument, the distance kept in worst[0]."""
    hist = np.full(4, -1.0)
    res = A.op_finalize(code, p0, p1, base, slot, hist=hist, it=2)
    ref, href, _ = kr.finalize(code, p0, p1, base, slot, hist, 2)
    exact, roots = (list(names) for names in kr.FIN_WRITES[code])
    exact_idx = [S[s] for s in exact] + ([slot] if code == kr.FIN_STORE else [])
    root_idx = [S[s] for s in roots] + ([slot] if code == kr.FIN_SQRT else [])
    untouched = [k for k in range(kr.S_COUNT) if k not in exact_idx + root_idx]
    name = kr.FIN_NAMES[code]
    assert clean(res) and res["counter"] == 0, name
    assert same_bits(res["scal"][untouched], base[untouched]), name
    assert same_bits(res["scal"][exact_idx], ref[exact_idx]), (name, res["scal"][exact_idx], ref[exact_idx])
    for k in root_idx:
        worst[0] = max(worst[0], ulps(res["scal"][k], ref[k]))
    if code in kr.HIST_CODES:
        assert len(root_idx) == 1 and same_bits(res["hist"][2], res["scal"][root_idx[0]]), name  # the history holds the stored root
        assert same_bits(np.delete(res["hist"], 2), np.delete(hist, 2)), name
    else:
        assert same_bits(res["hist"], hist), name
    return res["scal"]


def test_finalize_codes(A):
    """The eleven codes on scalar blocks prefilled with random positive values, partial sums of several counts and of both signs.
    Square roots: sqrt() on the device against math.sqrt of the same argument.  The largest distance is printed; measured on an
    MI355X over the 165 launches here, the breakdown inputs and every root of the sum tests: 0 ulp (the device's fp64 sqrt is
    correctly rounded), so what is asserted is equality (SQRT_ULPS = 0), not the 1 ulp a merely accurate sqrt would need."""
    worst = [0]
    for code in range(11):
        for trial, nblk in enumerate((1, 7, 391, 2048, 39366)):
            for sign in (1.0, -1.0, 0.0):
                rng = np.random.default_rng([code, trial])
                p0 = rng.standard_normal(nblk) ** 2
                if sign < 0.0:
                    p0 = -p0  # (a negative sum: FIN_SQRT and FIN_CG_BETA then take the root of a negative number)
                elif sign == 0.0:
                    p0 = rng.standard_normal(nblk)
                p1 = rng.standard_normal(max(1, nblk // 2)) ** 2
                check_code(A, code, p0, p1, random_block([code, trial]), S["TMP"] if code <= kr.FIN_SQRT else 0, worst)
    print("largest distance of a device square root from math.sqrt:", worst[0], "ulp")
    assert worst[0] <= SQRT_ULPS


def test_finalize_breakdowns(A):
    """The branches a solve meets only by chance, as plain arithmetic on a scalar block"""
    base = random_block(5)
    ones, zeros = np.ones(3), np.zeros(3)
    worst = [0]
    # BiCGStab's lucky breakdown: As.As = 0 gives omega1 = 0, not 0 / 0
    sc = check_code(A, kr.FIN_BICG_OMEGA, zeros, zeros, base, 0, worst)
    assert sc[S["OMEGA1"]] == 0.0 and not np.signbit(sc[S["OMEGA1"]]) and sc[S["ASS"]] == 0.0 and sc[S["ASAS"]] == 0.0
    sc = check_code(A, kr.FIN_BICG_OMEGA, ones, zeros, base, 0, worst)
    assert sc[S["OMEGA1"]] == 0.0
    # alpha with a zero denominator: the IEEE quotient, and nalpha its negation
    for code, num in ((kr.FIN_PCG_ALPHA, "RZ"), (kr.FIN_CG_ALPHA, "RR")):
        sc = check_code(A, code, zeros, None, base, 0, worst)
        assert sc[S["ALPHA"]] == math.inf and sc[S["NALPHA"]] == -math.inf
        neg = base.copy()
        neg[S[num]] = -1.5
        sc = check_code(A, code, zeros, None, neg, 0, worst)
        assert sc[S["ALPHA"]] == -math.inf and sc[S["NALPHA"]] == math.inf
        nul = base.copy()
        nul[S[num]] = 0.0
        sc = check_code(A, code, zeros, None, nul, 0, worst)
        assert math.isnan(sc[S["ALPHA"]]) and math.isnan(sc[S["NALPHA"]]) and sc[S["PAP"]] == 0.0
    # beta of BiCGStab after omega1 = 0: r.r0 / alpha1 * (alpha / 0)
    om0 = base.copy()
    om0[S["OMEGA1"]] = 0.0
    sc = check_code(A, kr.FIN_BICG_BETA, ones, ones, om0, 0, worst)
    assert sc[S["BETA"]] == math.inf and sc[S["RES"]] == math.sqrt(3.0)
    sc = check_code(A, kr.FIN_BICG_BETA, zeros, ones, om0, 0, worst)
    assert math.isnan(sc[S["BETA"]])
    # CG's residual sqrt(rr * beta) with rr = 0: 0 / 0
    rr0 = base.copy()
    rr0[S["RR"]] = 0.0
    sc = check_code(A, kr.FIN_CG_BETA, zeros, None, rr0, 0, worst)
    assert math.isnan(sc[S["BETA"]]) and math.isnan(sc[S["RES"]]) and sc[S["RR"]] == 0.0
    sc = check_code(A, kr.FIN_CG_BETA, zeros, None, base, 0, worst)
    assert sc[S["BETA"]] == 0.0 and sc[S["RES"]] == 0.0
    # a NaN partial reaches the history (and the loops' NaN test) through every code that stores a residual
    nan = np.array([1.0, math.nan, 2.0])
    for code in kr.HIST_CODES:
        p0, p1 = (nan, None) if code in (kr.FIN_SQRT, kr.FIN_CG_BETA) else (ones, nan)
        res = A.op_finalize(code, p0, p1, base, S["RES"], hist=np.zeros(2), it=1)
        assert math.isnan(res["hist"][1]) and res["hist"][0] == 0.0 and math.isnan(res["scal"][S["RES"]]), kr.FIN_NAMES[code]
    assert worst[0] <= SQRT_ULPS


# ---------------------------------------------------------------------------------------------------------------- history slot

def test_history_slot(A):
    base = random_block(9)
    cap = 8
    blank = np.full(cap, -1.0)
    p = np.array([4.0, 12.0])  # sum 16, root 4

    def slots(res):
        return [k for k in range(len(res["hist"])) if res["hist"][k] != -1.0]

    for it, want in ((0, 0), (5, 5), (cap - 1, cap - 1), (cap, cap - 1), (cap + 100, cap - 1), (1 << 30, cap - 1)):
        for code, p0, p1 in ((kr.FIN_SQRT, p, None), (kr.FIN_PCG_BETA_RES, p, p), (kr.FIN_CG_BETA, p, None), (kr.FIN_BICG_BETA, p, p)):
            res = A.op_finalize(code, p0, p1, base, S["RES"], hist=blank, it=it, counter=3)
            assert slots(res) == [want] and clean(res) and res["counter"] == 3, (it, kr.FIN_NAMES[code])  # an explicit slot: no counter
            assert near(res["hist"], kr.finalize(code, p0, p1, base, S["RES"], blank, it, 3)[1])
    # graph replay: frozen arguments, the slot comes from the device counter; six launches into four slots
    vals = np.array([1.0, 4.0, 9.0, 16.0, 25.0, 36.0])
    res = A.op_finalize(kr.FIN_SQRT, vals[:1], None, base, S["RES"], hist=np.full(4, -1.0), it=-1, counter=0, repeat=6)
    assert res["counter"] == 6 and clean(res) and np.array_equal(res["hist"], [1.0, 1.0, 1.0, 1.0])
    # six different values from six launches of one call: in mode 2 FIN_SQRT into S_SUM0 takes the root of what the launch before
    # it left there -- 2^32 -> 65536, 256, 16, 4, 2, sqrt(2) go to slots 0, 1, 2, 3, 3, 3
    chain = base.copy()
    chain[S["SUM0"]] = 2.0 ** 32
    res = A.op_finalize(kr.FIN_SQRT, None, None, chain, S["SUM0"], mode=2, hist=np.full(4, -1.0), it=-1, counter=0, repeat=6)
    assert res["counter"] == 6 and clean(res) and np.array_equal(res["hist"], [65536.0, 256.0, 16.0, math.sqrt(2.0)])
    assert res["scal"][S["SUM0"]] == math.sqrt(2.0)
    assert same_bits(np.delete(res["scal"], S["SUM0"]), np.delete(chain, S["SUM0"]))
    hist, ctr, sc = np.full(4, -1.0), 0, base
    seen = []
    for k in range(6):  # one launch per value, the counter carried over as the device keeps it
        res = A.op_finalize(kr.FIN_PCG_BETA_RES, vals[:1], vals[k: k + 1], sc, 0, hist=hist, it=-1, counter=ctr)
        ref = kr.finalize(kr.FIN_PCG_BETA_RES, vals[:1], vals[k: k + 1], sc, 0, hist, -1, ctr)
        assert near(res["scal"], ref[0]) and near(res["hist"], ref[1]) and res["counter"] == ref[2] == k + 1 and clean(res)
        hist, ctr, sc = res["hist"], res["counter"], res["scal"]
        seen.append(hist.copy())
    assert np.array_equal(seen[3], [1.0, 2.0, 3.0, 4.0]) and np.array_equal(seen[4], [1.0, 2.0, 3.0, 5.0])
    assert np.array_equal(seen[5], [1.0, 2.0, 3.0, 6.0])  # slots 0, 1, 2, 3, 3, 3: the last value stands in slot 3
    # a counter starting at 7, as after the copy of the host's count in pcg_steps, writes slot 7
    res = A.op_finalize(kr.FIN_PCG_BETA_RES, p, p, base, 0, hist=blank, it=-1, counter=7, repeat=1)
    assert slots(res) == [7] and res["hist"][7] == 4.0 and res["counter"] == 8
    res = A.op_finalize(kr.FIN_CG_BETA, p, None, base, 0, hist=np.full(12, -1.0), it=-1, counter=7, repeat=3)
    assert slots(res) == [7, 8, 9] and res["counter"] == 10
    # codes that store no residual, and launches without a history, leave the counter alone
    for code in range(11):
        res = A.op_finalize(code, p, p, base, S["TMP"], hist=None, it=-1, counter=5, repeat=2)
        assert res["counter"] == 5, kr.FIN_NAMES[code]
        if code not in kr.HIST_CODES:
            res = A.op_finalize(code, p, p, base, S["TMP"], hist=blank, it=-1, counter=5, repeat=2)
            assert res["counter"] == 5 and same_bits(res["hist"], blank) and clean(res), kr.FIN_NAMES[code]


# ---------------------------------------------------------------------------------------------------------------- loops

@pytest.fixture(scope="module")
def systems():
    out = {}
    rp, ci, v = problems.poisson3d(30)
    out["poisson3d"] = (sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET)), np.ones(len(rp) - 1))
    rp, ci, v, b = load_c0()
    out["c0"] = (sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET)), b)
    return out


def solve_with(A, b, method, check_every, max_iter=0):
    A.set_stopping(TOL, max_iter, check_every)
    x = np.zeros(A.nrow)
    hist, rc = A.solve(method, b, x)
    return hist, rc, x


@pytest.mark.parametrize("name", ["poisson3d", "c0"])
@pytest.mark.parametrize("method", ["pcg", "cg", "pbicg", "fcg"])
def test_loops_under_check_every(systems, name, method):
    """Reading the residual every k iterations changes nothing that is stored: the history up to the count of check_every = 1 is the
    same bits, the loop ends at the first multiple of k from there, with the same return code and an x that meets the bound of the
    solver tests.  (tests/test_krylov_ops_host.py: the recurrences of these inputs stay finite over the extra iterations.)"""
    A, b = systems[name]
    S0 = A.level_scipy(0)
    try:
        h1, rc1, x1 = solve_with(A, b, method, 1, 100000)
        m1 = len(h1)
        assert rc1 == 0 and h1[-1] <= TOL and np.all(h1[:-1] > TOL)
        for k in (4, 7):
            hk, rck, xk = solve_with(A, b, method, k, 100000)
            want = -(-m1 // k) * k
            print(name, method, "check_every", k, "iterations", len(hk), "against", m1, "past convergence", hk[m1 - 1:])
            assert len(hk) == want and want - m1 <= 6
            assert same_bits(hk[:m1], h1)
            assert rck == rc1
            assert np.all(np.isfinite(hk)) and np.all(hk[m1:] <= TOL)
            assert np.linalg.norm(b - S0 @ xk) <= 1.0001e-8
            if want == m1:
                assert same_bits(xk, x1)
        # the iteration cap first: it is a check of its own
        cap = m1 - 2 if (m1 - 2) % 4 else m1 - 3
        hc1, rcc1, xc1 = solve_with(A, b, method, 1, cap)
        hc4, rcc4, xc4 = solve_with(A, b, method, 4, cap)
        assert cap % 4 != 0 and len(hc1) == len(hc4) == cap and rcc1 == rcc4 == sa.SPARSH_ENOCONV
        assert same_bits(hc1, hc4) and same_bits(xc1, xc4) and same_bits(hc1, h1[:cap])
    finally:
        A.set_stopping(TOL, 100000, 1)


def test_gmres_under_check_every(systems):
    """sparsh_amg.h on GMRES: the host reads one history entry every check_every iterations, so up to check_every - 1 steps may run
    past convergence; a cycle still ends after `restart` steps, and its true residual is the stopping test.  Restart 5 with
    check_every 4: the checkpoints 4, 8, 12, ... straddle the cycle ends 5, 10, 15, ..."""
    A, b = systems["poisson3d"]
    S0 = A.level_scipy(0)
    try:
        A.set_gmres(5)
        h1, rc1, x1 = solve_with(A, b, "pgmres", 1, 100000)
        m1 = len(h1)
        h4, rc4, x4 = solve_with(A, b, "pgmres", 4, 100000)
        print("pgmres(5) iterations", m1, "with check_every = 4:", len(h4), "history", h4)
        assert rc1 == 0 and rc4 == 0 and m1 > 5  # more than one cycle
        assert h1[-1] <= TOL and np.all(h1[:-1] > TOL)
        # the loop under check_every = 4 leaves its cycle at the first checkpoint or cycle end from m1 on
        want = min(-(-m1 // 4) * 4, -(-m1 // 5) * 5)
        assert len(h4) == want and want - m1 <= 3
        assert same_bits(h4[:m1], h1)
        assert np.all(np.isfinite(h4)) and np.all(np.diff(h4[(m1 - 1) // 5 * 5:]) <= 0.0)  # within a cycle |g_{j+1}| cannot grow
        assert np.linalg.norm(b - S0 @ x4) <= 1.0001e-8 and np.linalg.norm(b - S0 @ x1) <= 1.0001e-8
    finally:
        A.set_gmres(0)
        A.set_stopping(TOL, 100000, 1)


def test_benchmark_protocol_is_independent_of_check_every():
    """What bench.py runs: tol = 0, check_every = 1 << 30, krylov_init_dev("pcg") and krylov_step_dev in pieces -- here 5, 1 and 42,
    launched eagerly and replayed from the captured graph -- against the same on handles that read the residual every iteration.
    History and x: the same bits in all four runs, and every call takes the steps it was asked for."""
    rp, ci, v = problems.poisson3d(30)
    n = len(rp) - 1
    b = np.ones(n)
    runs = {}
    for check_every in (1 << 30, 1):
        for graph in (0, 1):
            H = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, tol=0.0, check_every=check_every, use_graph=graph))
            bd, xd = H.dev_alloc(8 * n), H.dev_alloc(8 * n)
            try:
                H.h2d(bd, b)
                H.h2d(xd, np.zeros(n))
                H.krylov_init_dev("pcg", bd, xd)
                for piece in (5, 1, 42):
                    done, _ = H.krylov_step_dev(piece)
                    assert done == piece, (check_every, graph, piece, done)
                hist = H.krylov_history()
                x = np.zeros(n)
                H.d2h(x, xd)
            finally:
                H.dev_free(bd)
                H.dev_free(xd)
                H.close()
            assert len(hist) == 48 and np.all(np.isfinite(hist)) and np.all(np.isfinite(x))
            runs[(check_every, graph)] = (hist, x)
    h0, x0 = runs[(1, 0)]
    assert h0[11] <= TOL < h0[3]  # (the run goes far past convergence, as the benchmark's does)
    for key, (hist, x) in runs.items():
        assert same_bits(hist, h0) and same_bits(x, x0), key
