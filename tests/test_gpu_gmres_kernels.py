"""The kernels of restarted GMRES (krylov_kernels.hip) one by one, through the sparsh_op_gs_* / sparsh_op_gmres_small hooks, against
plain numpy written out in this file, and the whole-solve cases that the kernel tests do not replace.  GPU box only.

Two kinds of data.  "exact": every entry of V, w and h is an integer in [-8, 8] divided by 16, so every product and every partial
sum is exactly representable in fp64 whatever the order of the additions (and every value is a float): all outputs, reductions
included, are compared with np.array_equal.  "normal": standard_normal entries (rounded to float32 first under a float basis);
stored vectors are compared bitwise -- the device rounds the product and the subtraction separately, as numpy does -- and
reductions against a longdouble dot to 1e-13 * sum |v_i| |w_i|, the figure of test_blas1.

Shapes: kBlock = 256 rows per workgroup step of a double basis, gs_grid(n) changes every 512 rows, a float basis takes 4 rows per
thread (2 when 9..16 vectors are in a launch), a launch holds kGsMaxK = 16 vectors and picks its template at 4 / 8 / 16.
"""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from test_gpu_gmres import QUIET, TOL, gmres_ref, true_residual
from test_gpu_gmres_fp32_basis import gmres_ref_f32

pytestmark = pytest.mark.gpu

LD = np.longdouble
BASES = ["fp64", "fp32"]
KINDS = ["exact", "normal"]
NS = (1, 2, 3, 4, 5, 7, 255, 256, 257, 511, 512, 513, 1024, 1025, 1027, 2049, 4099)
NV_AT_EVERY_N = (3, 8, 16, 17)
NVS = (1, 3, 4, 5, 8, 9, 15, 16, 17, 24, 32, 33, 48, 49, 63, 64)
N_AT_EVERY_NV = (3, 258, 1027)
ALL_N = tuple(sorted(set(NS) | set(N_AT_EVERY_NV)))
NV_MAX = 65
SENTINEL = -7.25
SUM_RTOL = 1e-13


def nvs_at(n, extra=()):
    return sorted(set(NV_AT_EVERY_N) | (set(NVS) | set(extra) if n in N_AT_EVERY_NV else set()))


@pytest.fixture(scope="module")
def dev():
    """any ready single-GPU handle: the hooks use its stream and allocator only"""
    rp, ci, v = problems.poisson2d(8)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
    yield A
    A.close()


@functools.lru_cache(maxsize=None)
def data(kind, basis, n, nv=NV_MAX):
    """(V[nv][n], w[n], h[nv]), read-only and shared by every test of this shape"""
    rng = np.random.default_rng(1000 * n + nv)
    if kind == "exact":
        V, w, h = (rng.integers(-8, 9, size=s) / 16.0 for s in ((nv, n), n, nv))
    else:
        V, w, h = (rng.standard_normal(s) for s in ((nv, n), n, nv))
        if basis == "fp32":
            V, w, h = (a.astype(np.float32).astype(np.float64) for a in (V, w, h))
    for a in (V, w, h):
        a.setflags(write=False)
    return V, w, h


def stored(V, basis):
    """the basis as the device holds it, widened back"""
    return V.astype(np.float32).astype(np.float64) if basis == "fp32" else V


def check_sums(got, V, w, kind, what):
    """got[k] against V[k] . w"""
    if kind == "exact":
        want = (V * w).sum(axis=1)
        assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])
        return
    want = (V.astype(LD) * w.astype(LD)).sum(axis=1)
    bound = SUM_RTOL * (np.abs(V) * np.abs(w)).sum(axis=1)
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    assert np.all(err <= bound), (what, int((err / bound).argmax()), float((err / bound).max()))


def check_ww(got, w, kind, what):
    check_sums(np.array([got]), w[None, :], w, kind, what + " w.w")


def update_ref(V, h, w_in):
    s = np.zeros(V.shape[1]) if w_in is None else w_in.copy()
    for k in range(len(h)):
        s = s - h[k] * V[k]  # two roundings, k ascending
    return s


def expected_tail(n, basis):
    return (-n) % 4 if basis == "fp32" else n % 2


# ---- gs_dot + gs_finalize

@pytest.mark.parametrize("n", ALL_N)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("basis", BASES)
def test_gs_dot(dev, basis, kind, n):
    Vall, w, _ = data(kind, basis, n)
    for nv in nvs_at(n, extra=(NV_MAX,)):
        V = Vall[:nv]
        for want_ww in (False, True):
            sums, ww = dev.op_gs_dot(V, w, basis, ww=want_ww)
            what = f"gs_dot {basis} {kind} n={n} nv={nv} ww={want_ww}"
            check_sums(sums, stored(V, basis), w, kind, what)
            if want_ww:
                check_ww(ww, w, kind, what)
            else:
                assert ww is None


# ---- gs_update (+ gs_finalize)

def run_update(dev, basis, kind, n, nv, mode, dots, ww):
    Vall, w, hall = data(kind, basis, n)
    V, h = Vall[:nv], hall[:nv]
    w_in = None if mode == "null" else w
    out, d, s, tail = dev.op_gs_update(V, h, w_in, basis, in_place=mode == "in_place", dots=dots, ww=ww, sentinel=SENTINEL)
    what = f"gs_update {basis} {kind} n={n} nv={nv} {mode} dots={dots} ww={ww}"
    Vs = stored(V, basis)
    want = update_ref(Vs, h, w_in)
    assert np.array_equal(out, want), (what, np.flatnonzero(out != want)[:8])
    assert len(tail) == expected_tail(n, basis) and np.all(tail == SENTINEL), (what, tail)
    if dots:
        check_sums(d, Vs, want, kind, what)
    else:
        assert d is None
    if ww:
        check_ww(s, want, kind, what)
    else:
        assert s is None


@pytest.mark.parametrize("n", ALL_N)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("basis", BASES)
def test_gs_update_shapes(dev, basis, kind, n):
    """the first update of a step (in place, with the sums of the second pass), the second (in place, w.w only), and both at once"""
    for nv in nvs_at(n):
        run_update(dev, basis, kind, n, nv, "in_place", True, False)
        run_update(dev, basis, kind, n, nv, "in_place", False, True)
        run_update(dev, basis, kind, n, nv, "in_place", True, True)  # (w.w in the k == nv slot, also where nv == K)


@pytest.mark.parametrize("ww", [False, True], ids=["noww", "ww"])
@pytest.mark.parametrize("dots", [False, True], ids=["nodots", "dots"])
@pytest.mark.parametrize("mode", ["null", "in_place", "two_vectors"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("basis", BASES)
def test_gs_update_argument_combinations(dev, basis, kind, mode, dots, ww):
    """n = 6 (one partly filled group of 4 rows, n = 2 mod 4) and n = 1027 (three workgroups, n = 3 mod 4)"""
    for n in (6, 1027):
        for nv in (3, 16, 17, 33):
            run_update(dev, basis, kind, n, nv, mode, dots, ww)


@pytest.mark.parametrize("basis", BASES)
def test_large_n(dev, basis):
    """n = 1 310 723 = 2.5 * 2048 * 256 + 3: three grid-stride steps of the 2048 workgroups of a double basis, n = 3 (mod 4)"""
    n, nv = 1310723, 5
    V, w, h = data("normal", basis, n, nv)
    Vs = stored(V, basis)
    sums, ww = dev.op_gs_dot(V, w, basis, ww=True)
    check_sums(sums, Vs, w, "normal", "gs_dot")
    check_ww(ww, w, "normal", "gs_dot")
    out, d, s, tail = dev.op_gs_update(V, h, w, basis, in_place=True, dots=True, ww=True, sentinel=SENTINEL)
    want = update_ref(Vs, h, w)
    assert np.array_equal(out, want), np.flatnonzero(out != want)[:8]
    assert len(tail) == expected_tail(n, basis) and np.all(tail == SENTINEL), tail
    check_sums(d, Vs, want, "normal", "gs_update")
    check_ww(s, want, "normal", "gs_update")


# ---- gs_scale



@pytest.mark.parametrize("d", [2.5, 1e-300, 0.0, -1.0, float("nan")])
@pytest.mark.parametrize("basis", BASES)
def test_gs_scale(dev, basis, d):
    """v = w / d, rounded once to float under a float basis (1e-300: every quotient overflows the float to +-inf); d not > 0: zeros
    and no division.  The padding of the float vector stays zero."""
    for n in NS:
        w = data("normal", basis, n)[1]
        with np.errstate(over="ignore"):
            want = w / d if d > 0 else np.zeros(n)
            want32 = want.astype(np.float32).astype(np.float64)
        if basis == "fp64":
            v = dev.op_gs_scale(w, d, basis)
            assert np.array_equal(v, want), (n, d)
            continue
        v, vd, tail = dev.op_gs_scale(w, d, basis)
        assert np.array_equal(v, want32), (n, d)
        assert np.array_equal(vd, want32), (n, d)
        assert len(tail) == expected_tail(n, basis) and np.all(tail == 0.0) and not np.any(np.signbit(tail)), (n, d, tail)


# ---- gmres_step + gmres_solve

def small_problem(m, nblk, seed=0):
    """Coefficient columns of a Hessenberg matrix 4 I + uniform(-1, 1): column j is split into the two Gram-Schmidt passes
    (hcol + ccol, the second three orders of magnitude smaller); the subdiagonal entry is sqrt(sum of ww_partial[j]), the partial
    sums being non-negative multiples of 2^-10 whose sum (< 1) is exact in any order."""
    rng = np.random.default_rng(100 * m + nblk + seed)
    hcols, ccols = [], []
    for j in range(m):
        col = rng.uniform(-1.0, 1.0, j + 1)
        col[j] += 4.0
        c = 1e-3 * rng.uniform(-1.0, 1.0, j + 1)
        hcols.append(col - c)
        ccols.append(c)
    ww = rng.integers(0, 1024 // nblk + 1, size=(m, nblk)) / 1024.0
    beta = 1.0 + rng.uniform()
    return hcols, ccols, ww, beta


def small_ref(hcols, ccols, ww, beta, k, T=LD):
    """the Givens recurrence of gmres_step_kernel and the back-substitution of gmres_solve_kernel in type T"""
    m = len(hcols)
    R, cs, sn, g, hist = np.zeros((m, m), T), np.zeros(m, T), np.zeros(m, T), np.zeros(m + 1, T), np.zeros(m, T)
    with np.errstate(invalid="ignore"):
        for j in range(m):
            col = np.zeros(j + 2, T)
            col[: j + 1] = (np.asarray(hcols[j]) + np.asarray(ccols[j])).astype(T)  # (the fp64 sum the device forms)
            hn = np.sqrt(T(ww[j].sum()))
            for i in range(j):
                a, b = col[i], col[i + 1]
                col[i] = cs[i] * a + sn[i] * b
                col[i + 1] = cs[i] * b - sn[i] * a
            a = col[j]
            d = np.sqrt(a * a + hn * hn)
            c, z = (a / d, hn / d) if d != 0 else (T(1), T(0))
            col[j] = c * a + z * hn
            cs[j], sn[j] = c, z
            gj = T(beta) if j == 0 else g[j]
            g[j] = c * gj
            g[j + 1] = -z * gj
            hist[j] = abs(g[j + 1])
            R[: j + 1, j] = col[: j + 1]
        y = np.zeros(k, T)
        for i in range(k - 1, -1, -1):
            t = (R[i, i + 1:k] * y[i + 1:]).sum()
            y[i] = (g[i] - t) / R[i, i] if R[i, i] != 0 else T(0)
    return dict(hist=hist, R=R, cs=cs, sn=sn, g=g, ny=-y)


EPS = 2.0 ** -52


def check_small(got, ref, m, k, cond):
    """column j of R, cs, sn, g, hist: 4 (j + 2) eps of the largest magnitude in that column / in g -- j rotations of two products
    and a sum each on column j, one more on g; ny: 64 k eps cond(R) max|y| for the back-substitution on a rotated R"""
    gmax = float(np.abs(ref["g"]).max())
    for j in range(m):
        tol = 4 * (j + 2) * EPS
        rcol = ref["R"][: j + 1, j]
        err = np.abs(got["R"][: j + 1, j].astype(LD) - rcol).max()
        assert err <= tol * np.abs(rcol).max(), ("R", j, float(err))
        rot = max(abs(ref["cs"][j]), abs(ref["sn"][j]))
        assert abs(got["cs"][j] - ref["cs"][j]) <= tol * rot, ("cs", j)
        assert abs(got["sn"][j] - ref["sn"][j]) <= tol * rot, ("sn", j)
        assert abs(got["g"][j] - ref["g"][j]) <= tol * gmax, ("g", j)
        assert abs(got["hist"][j] - ref["hist"][j]) <= tol * gmax, ("hist", j)
    assert abs(got["g"][m] - ref["g"][m]) <= 4 * (m + 1) * EPS * gmax, ("g", m)
    assert np.all(np.tril(got["R"], -1) == 0.0)
    yerr = np.abs(got["ny"].astype(LD) - ref["ny"]).max()
    ymax = np.abs(ref["ny"]).max()
    print(f"m={m} k={k}: largest y error {float(yerr):.3e} of max|y| {float(ymax):.3e}, bound {64 * k * EPS * cond * float(ymax):.3e}")
    assert yerr <= 64 * k * EPS * cond * ymax


@pytest.mark.parametrize("nblk", [1, 5, 300])
@pytest.mark.parametrize("m,k", [(1, 1), (2, 2), (5, 5), (17, 17), (64, 64), (64, 40)])
def test_gmres_small(dev, m, k, nblk):
    """The Hessenberg matrices of small_problem were meant to keep cond(R) below 10.  They do up to k = 40 (1 .. 3.6 up to m = 17,
    6.5 .. 8.2 at k = 40) and not at m = k = 64, where cond(R) is 11 .. 14.4.  The bound on y carries the computed cond(R) as a
    factor, so it is not widened by this; the value is printed."""
    hcols, ccols, ww, beta = small_problem(m, nblk)
    got = dev.op_gmres_small(hcols, ccols, ww, beta, k)
    ref = small_ref(hcols, ccols, ww, beta, k)
    cond = np.linalg.cond(ref["R"][:k, :k].astype(np.float64))
    print(f"m={m} k={k} nblk={nblk}: cond(R) = {cond:.3f}")
    check_small(got, ref, m, k, cond)
    # not asserted: bitwise agreement with the same recurrence in float64 would need a correctly rounded device sqrt
    r64 = small_ref(hcols, ccols, ww, beta, k, np.float64)
    print("step outputs equal the float64 restatement bit for bit:",
          {name: bool(np.array_equal(got[name], r64[name])) for name in ("hist", "R", "cs", "sn", "g")})


def test_gmres_small_zero_column(dev):
    """a step whose column and w.w are all zero (a step taken after a lucky breakdown): rotation (1, 0), zero pivot, y_j = 0"""
    m, j0 = 5, 2
    hcols, ccols, ww, beta = small_problem(m, 5)
    hcols[j0], ccols[j0], ww[j0] = np.zeros(j0 + 1), np.zeros(j0 + 1), 0.0
    got = dev.op_gmres_small(hcols, ccols, ww, beta, m)
    assert all(np.all(np.isfinite(a)) for a in got.values())
    assert got["cs"][j0] == 1.0 and got["sn"][j0] == 0.0 and got["R"][j0, j0] == 0.0 and got["ny"][j0] == 0.0
    assert got["hist"][j0] == 0.0
    ref = small_ref(hcols, ccols, ww, beta, m)
    for name in got:
        assert np.abs(got[name].astype(LD) - ref[name]).max() <= 64 * m * EPS * max(1.0, float(np.abs(ref[name]).max())), name


def test_gmres_small_nan_reaches_the_history(dev):
    m, j0 = 5, 3
    hcols, ccols, ww, beta = small_problem(m, 5)
    hcols[j0] = hcols[j0].copy()
    hcols[j0][1] = np.nan
    got = dev.op_gmres_small(hcols, ccols, ww, beta, m)
    ref = small_ref(hcols, ccols, ww, beta, m)
    assert np.all(np.isfinite(got["hist"][:j0])) and np.all(np.isnan(got["hist"][j0:]))
    assert np.abs(got["hist"][:j0].astype(LD) - ref["hist"][:j0]).max() <= 4 * (j0 + 2) * EPS * float(np.abs(ref["g"][:j0]).max())


# ---- whole solves that the kernel tests do not replace

def longdouble_dot(a, c):
    return np.float64((a.astype(LD) * c.astype(LD)).sum())


def gmres_ref_dots(spmv, b, x0, m, cap, f32, dot=longdouble_dot):
    """gmres_ref / gmres_ref_f32 without preconditioner with every dot product and norm taken by `dot`: the restatement with
    another summation, which measures how far the summation moves the solution"""
    n = len(b)
    x = np.array(x0, dtype=np.float64)
    hist, it = [], 0
    while it < cap:
        r = b - spmv(x)
        beta = np.sqrt(dot(r, r))
        V = np.zeros((m + 1, n))
        V[0] = r / beta
        if f32:
            V[0] = V[0].astype(np.float32)
        g = np.zeros(m + 1)
        g[0] = beta
        R = np.zeros((m, m))
        cs, sn = np.zeros(m), np.zeros(m)
        k = 0
        for j in range(m):
            if it >= cap:
                break
            w = spmv(V[j])
            h = np.array([dot(V[i], w) for i in range(j + 1)])
            w = w - V[: j + 1].T @ h
            c = np.array([dot(V[i], w) for i in range(j + 1)])
            w = w - V[: j + 1].T @ c
            col = np.append(h + c, np.sqrt(dot(w, w)))
            V[j + 1] = w / col[j + 1]
            if f32:
                V[j + 1] = V[j + 1].astype(np.float32)
            for i in range(j):
                col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], cs[i] * col[i + 1] - sn[i] * col[i]
            d = np.hypot(col[j], col[j + 1])
            cs[j], sn[j] = col[j] / d, col[j + 1] / d
            R[: j + 1, j] = col[: j + 1]
            R[j, j] = cs[j] * col[j] + sn[j] * col[j + 1]
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            hist.append(abs(g[j + 1]))
            it += 1
            k = j + 1
        x = x + V[:k].T @ sla.solve_triangular(R[:k, :k], g[:k])
    return x, np.array(hist)


def restatement(A0, b, x0, restart, cap, basis):
    """(x, history, summation sensitivity) of unpreconditioned GMRES(restart), `cap` steps from x0: gmres_ref / gmres_ref_f32, and
    the largest difference of its solution, relative to max|x|, from the same restatement with longdouble dot products.  Device
    and restatement differ in the order of the additions inside a dot product only; ten times the sensitivity is the solution bound,
    the factor covering the device's tree order."""
    spmv = lambda u: A0 @ u
    if basis == "fp32":
        want, href, _ = gmres_ref_f32(spmv, None, b, x0, restart, cap=cap)
    else:
        want, href, _ = gmres_ref(A0, None, b, x0, restart, cap=cap)
    xl, _ = gmres_ref_dots(spmv, b, x0, restart, cap, basis == "fp32")
    sens = np.abs(want - xl).max() / np.abs(want).max()
    print(f"restart {restart}, {cap} steps, {basis}: summation sensitivity of the restatement {sens:.3e}")
    return want, href, sens


def long_restart_handle(restart, basis, max_iter):
    rp, ci, v = problems.poisson2d(48)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
    A.set_gmres(restart, basis=basis)
    A.set_stopping(TOL, max_iter=max_iter)
    return A, A.level_scipy(0), np.ones(A.nrow)


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("restart,max_iter", [(64, 64), (33, 33), (33, 66)])
def test_full_cycles_of_long_restarts(basis, restart, max_iter):
    """Unpreconditioned GMRES on poisson2d(48), b = ones.  Restart 64 with 64 iterations: one complete cycle of the largest restart
    length, every multi-launch chunk from one vector to four whole chunks, gmres_step at j = 63 and a 64-lane solve (SciPy's GMRES
    needs 162 steps on this system, so the cycle cannot end early).  Restart 33: one and two cycles whose last step has a chunk of
    one vector.  Every history entry within 1e-6 relative (the figure of test_unpreconditioned_head); the solution within ten times
    the summation sensitivity, which `restatement` measures anew in every run.  Measured on the CPU, of max|x|: restart 64 3.46e-15
    with a double basis and 3.44e-14 with a float one; restart 33, one cycle 4.5e-15 and 3.2e-14, two cycles 1.13e-15 and 1.18e-12.

    Two cycles with a float basis: the history only.  There the device differs from the restatement by 1.16e-9 of max|x| (history
    2.6e-7), a hundred times the bound that 1.18e-12 gives.  b - A x cancels two digits at the cycle start, so solutions that
    differ by 3e-14 max|x| after the first cycle round some of the 2304 floats of v_0 differently, and the second cycle then runs in
    another Krylov space.  test_second_cycle_of_a_float_basis shows that this is all there is to it: from the device's own x after
    the first cycle the restatement meets the device's second cycle at the tight bound."""
    A, A0, b = long_restart_handle(restart, basis, max_iter)
    want, href, sens = restatement(A0, b, np.zeros(A.nrow), restart, max_iter, basis)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("gmres", b, x)
    assert rc == sa.SPARSH_ENOCONV and len(hist) == max_iter and len(href) == max_iter
    err = np.abs(hist - href) / href
    print("largest relative history difference", err.max(), "at", err.argmax())
    assert np.all(err <= 1e-6)
    xerr = np.abs(x - want).max() / np.abs(want).max()
    print("solution difference relative to max|x|", xerr, "bound", 10 * sens)
    if (basis, max_iter) != ("fp32", 2 * restart):
        assert xerr <= 10 * sens


def test_second_cycle_of_a_float_basis():
    """Restart 33, float basis, 66 steps: the second cycle against the restatement started from the x the device itself holds
    after the first (a solve stopped at 33 steps returns it).  Both then round the same v_0, and the 33 history entries and the
    solution are held to the bounds of a single cycle."""
    restart = 33
    A, A0, b = long_restart_handle(restart, "fp32", restart)
    x1 = np.zeros(A.nrow)
    h1, rc = A.solve("gmres", b, x1)
    assert rc == sa.SPARSH_ENOCONV and len(h1) == restart
    A.set_stopping(TOL, max_iter=2 * restart)
    x = np.zeros(A.nrow)
    hist, rc = A.solve("gmres", b, x)
    assert rc == sa.SPARSH_ENOCONV and len(hist) == 2 * restart
    assert np.array_equal(hist[:restart], h1)  # the same first cycle, so x1 is where the second one starts
    want, href, sens = restatement(A0, b, x1, restart, restart, "fp32")
    err = np.abs(hist[restart:] - href) / href
    print("second cycle: largest relative history difference", err.max(), "at", err.argmax())
    assert np.all(err <= 1e-6)
    xerr = np.abs(x - want).max() / np.abs(want).max()
    print("second cycle: solution difference relative to max|x|", xerr, "bound", 10 * sens)
    assert xerr <= 10 * sens


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_tiny_systems(n, basis):
    """1-D Laplacian of n rows (a single level), restart 30: the Krylov space is exhausted before the cycle ends, the kernels run
    with n below one group of rows"""
    M = sp.csr_matrix(2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1))
    M.sort_indices()
    A = sa.sp_matrix_mg(M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data).setup(sa.default_params(**QUIET))
    assert A.nlevels == 1
    A.set_gmres(30, basis=basis)
    b = 1.0 + np.arange(n) ** 2
    x = np.zeros(n)
    hist, rc = A.solve("gmres", b, x)
    print(f"n={n} {basis}: history", hist)
    assert rc == 0
    assert np.all(np.isfinite(hist)) and np.all(np.isfinite(x))
    assert true_residual(M, b, x) <= 1.001 * TOL
