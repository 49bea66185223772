"""The restatement of the single-vector Krylov kernels and of finalize_kernel (tests/krylov_ops_restatement.py) anchored on the CPU:
loops composed from it reproduce the oracle's solvers, its sums are exact where exact sums exist, and the hooks that run the
kernels refuse bad arguments before any device is asked for.  tests/test_gpu_krylov_ops.py compares the kernels with it bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import krylov_ops_restatement as kr
import oracle
import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import hist_tolerance, load_c0

TOL = 1e-8  # tol of the oracle's default parameters, and the constant in its CG loop
OVERSHOOT = 6  # iterations check_every = 7 can run past the one that meets tol


# The two anchoring matrices have 144 and 300 rows.  Under the default coarsening limits (4000 / 2000 rows) neither is coarsened: M is
# the exact inverse, every preconditioned loop ends after one iteration, and its only history entry is rounding noise (4e-14 against
# ||b|| = 12), which two orders of summation reproduce to no digit at all.  So the oracle and the composed loops get limits that make
# real hierarchies (144 / 72 / 36 and 300 / 160 / 85 / 46 rows), and b is a fixed standard-normal vector, not the constant one -- on
# poisson2d(12) CG on the constant vector terminates finitely after 20 steps, again at rounding level.
SMALL = dict(limit_upper=60, limit_lower=30)


def _case(name):
    if name == "c0":
        rp, ci, v, b = load_c0()
    elif name == "poisson3d":
        rp, ci, v = problems.poisson3d(30)
        b = np.ones(len(rp) - 1)
    else:
        rp, ci, v = problems.poisson2d(12) if name == "poisson2d" else problems.random_spd(300, 9)
        b = np.random.default_rng(7).standard_normal(len(rp) - 1)
    return oracle.Csr(rp, ci, v), b


def _operators(O, **prm):
    H = oracle.Hierarchy(O, oracle.params(**prm))
    return (lambda v: oracle.spmv(O, v)), (lambda r: H.solve(r, np.zeros_like(r), iterations=1)[0]), H


def _hist_ok(h, ref):
    assert len(h) == len(ref), (len(h), len(ref))
    err = np.abs(h - ref) / ref
    assert np.all(err <= hist_tolerance(ref)), f"max rel err {err.max():.3e} at {err.argmax()}"


@pytest.mark.parametrize("name", ["poisson2d", "random_spd"])
@pytest.mark.parametrize("method", ["pcg", "pbicg", "cg"])
def test_composed_loops_reproduce_the_oracle(name, method):
    """One PCG, one BiCGStab and one CG loop made of the restated kernels and finalize codes (A p from the oracle's SpMV, M r from
    its cycle) give the oracle's history within hist_tolerance and its x to 1e-8."""
    O, b = _case(name)
    spmv, precond, H = _operators(O, **SMALL)
    xo, ho = oracle.solve(method, O, b, prm=oracle.params(**SMALL))
    assert H.nlevels >= 3 and len(ho) >= 2
    x0 = np.zeros(len(b))
    if method == "pcg":
        x, h = kr.pcg_loop(spmv, precond, b, x0, TOL)
        x2, h2 = kr.pcg_loop(spmv, precond, b, x0, TOL, defer_x=False)
        assert np.array_equal(h, h2) and np.array_equal(x, x2)  # x += alpha p at either place: the same bits
    elif method == "cg":
        x, h = kr.pcg_loop(spmv, None, b, x0, TOL)
    else:
        x, h = kr.bicg_loop(spmv, precond, b, x0, TOL, cap=1000)
    _hist_ok(h, ho)
    assert np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)


@pytest.mark.parametrize("name", ["poisson3d", "c0"])
def test_histories_stay_finite_past_convergence(name):
    """The inputs of the GPU check_every tests: every loop's recurrences stay finite for the 6 iterations that check_every = 7 can
    run past convergence at tol 1e-8 (a 0/0 there would be a property of the input, not of the loop)."""
    O, b = _case(name)
    spmv, precond, _H = _operators(O)
    x0 = np.zeros(len(b))
    for method, run in (("pcg", lambda: kr.pcg_loop(spmv, precond, b, x0, TOL, extra=OVERSHOOT)),
                        ("cg", lambda: kr.pcg_loop(spmv, None, b, x0, TOL, extra=OVERSHOOT)),
                        ("pbicg", lambda: kr.bicg_loop(spmv, precond, b, x0, TOL, cap=1000, extra=OVERSHOOT)),
                        ("fcg", lambda: kr.fcg_loop(spmv, precond, b, x0, TOL, cap=1000, extra=OVERSHOOT))):
        x, h = run()
        m1 = len(h) - OVERSHOOT
        print(name, method, "iterations", m1, "residuals past convergence", h[m1 - 1:])
        assert m1 >= 1 and h[m1 - 1] <= TOL and np.all(h[: m1 - 1] > TOL)
        assert np.all(np.isfinite(h)) and np.all(np.isfinite(x)), (method, h[m1:])
        assert np.all(h[m1:] <= 10 * TOL), (method, h[m1:])  # and the extra steps do not leave the converged state


def _integers(rng, n, lim=1000):
    return rng.integers(-lim, lim + 1, n).astype(np.float64)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 123457, 1048577])
def test_partial_sums_are_exact_on_integers(n):
    """On integer-valued terms of mixed sign every order of addition is exact: the restated partial sums are math.fsum over the
    elements the workgroup owns, whatever the tree."""
    rng = np.random.default_rng(n)
    t = _integers(rng, n)
    g = kr.ew_grid(n)
    assert g == min(2048, max(1, -(-n // 512)))
    part = kr.partials(t)
    assert part.shape == (g,)
    owner = (np.arange(n) // kr.K_BLOCK) % g
    sel = range(g) if g <= 8 else (0, 1, g // 2, g - 2, g - 1)
    for w in sel:
        assert part[w] == math.fsum(t[owner == w]), w
    assert math.fsum(part) == math.fsum(t)


@pytest.mark.parametrize("nblk", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 4096, 20479, 20480, 20481, 39366, 40961])
def test_finalize_sums_are_exact_on_integers(nblk):
    rng = np.random.default_rng(nblk)
    p = _integers(rng, nblk, 10 ** 6)
    assert kr.fin_sum(p) == math.fsum(p)
    q = _integers(rng, max(1, nblk // 3), 10 ** 6)
    sc, h, ctr = kr.finalize(kr.FIN_PCG_BETA_RES, p, q * q, np.ones(kr.S_COUNT), 0, np.zeros(3), 7, 5)
    assert sc[kr.S["ZR"]] == math.fsum(p) and sc[kr.S["RZ"]] == math.fsum(p) and sc[kr.S["BETA"]] == math.fsum(p)
    assert sc[kr.S["RES"]] == math.sqrt(math.fsum(q * q)) and h[2] == sc[kr.S["RES"]] and not h[:2].any() and ctr == 5


def test_restated_reduction_is_the_halving_tree():
    """The tree is not a left-to-right sum: on data where the two differ in the last bits the restatement follows the tree as
    written out here by hand for one wave and one workgroup."""
    def block(acc):  # 256 per-thread sums -> the workgroup's sum, scalar by scalar
        total = 0.0
        for w in range(len(acc) // 64):
            lane = [float(a) for a in acc[64 * w: 64 * w + 64]]
            off = 32
            while off:
                lane = [lane[l] + lane[l + off] for l in range(off)]
                off //= 2
            total = total + lane[0]
        return total

    rng = np.random.default_rng(3)
    v = rng.standard_normal(256)
    assert kr.partials(v)[0] == block(v)
    left_to_right = 0.0
    for e in v:
        left_to_right += e
    assert block(v) != left_to_right  # (this seed: the orders do differ, so the GPU comparison can tell them apart)
    # n = 600: two workgroups; workgroup 0 owns [0, 256) and [512, 600), its thread t adds u[t], then u[512 + t]
    u = rng.standard_normal(600)
    assert kr.ew_grid(600) == 2
    acc0 = [(0.0 + u[t]) + (u[512 + t] if t < 88 else 0.0) for t in range(256)]
    acc1 = [0.0 + u[256 + t] for t in range(256)]
    assert list(kr.partials(u)) == [block(acc0), block(acc1)]
    # finalize: thread t of 1024 adds p[t], p[t + 1024], p[t + 2048]; sixteen waves
    p = rng.standard_normal(2500)
    accf = [((0.0 + p[t]) + p[t + 1024]) + (p[t + 2048] if t < 452 else 0.0) for t in range(1024)]
    assert kr.fin_sum(p) == block(accf)


def test_finalize_codes_on_a_worked_block():
    """Every code once on small integers, against values worked out by hand; breakdown branches included."""
    S = kr.S
    base = np.arange(1.5, kr.S_COUNT + 1.5)  # slot k holds k + 1.5
    p0, p1 = np.array([3.0, 5.0]), np.array([4.0, 12.0])  # sums 8 and 16
    hist = np.full(4, -1.0)

    def run(code, **kw):
        return kr.finalize(code, p0, kw.pop("p1", p1), base, kw.pop("slot", S["TMP"]), hist, kw.pop("it", 1), 0, **kw)

    def changed(sc):
        return {kr.SLOTS[k]: sc[k] for k in range(kr.S_COUNT) if sc[k] != base[k]}

    sc, h, _ = run(kr.FIN_STORE)
    assert changed(sc) == {"TMP": 8.0} and np.array_equal(h, hist)
    sc, h, _ = run(kr.FIN_SQRT, p1=None, slot=S["RES"])
    assert changed(sc) == {"RES": math.sqrt(8.0)} and h[1] == math.sqrt(8.0)
    sc, h, _ = run(kr.FIN_PCG_ALPHA)
    assert changed(sc) == {"PAP": 8.0, "ALPHA": 1.5 / 8.0, "NALPHA": -1.5 / 8.0}
    sc, h, _ = run(kr.FIN_CG_ALPHA)
    assert changed(sc) == {"PAP": 8.0, "ALPHA": 6.5 / 8.0, "NALPHA": -6.5 / 8.0}
    sc, h, _ = run(kr.FIN_PCG_BETA)
    assert changed(sc) == {"ZR": 8.0, "BETA": 8.0 / 1.5, "RZ": 8.0} and np.array_equal(h, hist)
    sc, h, _ = run(kr.FIN_PCG_BETA_RES)
    assert changed(sc) == {"ZR": 8.0, "BETA": 8.0 / 1.5, "RZ": 8.0, "RES": 4.0} and h[1] == 4.0
    sc, h, _ = run(kr.FIN_CG_BETA)
    assert changed(sc) == {"BETA": 8.0 / 6.5, "RES": math.sqrt(6.5 * (8.0 / 6.5)), "RR": 8.0} and h[1] == sc[S["RES"]]
    sc, h, _ = run(kr.FIN_BICG_ALPHA)
    assert changed(sc) == {"ALPHA1": 8.0, "APR0": 16.0, "ALPHA": 0.5}
    sc, h, _ = run(kr.FIN_BICG_OMEGA)
    assert changed(sc) == {"ASS": 8.0, "ASAS": 16.0, "OMEGA1": 0.5}
    sc, h, _ = run(kr.FIN_BICG_BETA)
    assert changed(sc) == {"BETA": (8.0 / 9.5) * (3.5 / 13.5), "RR0": 8.0, "RES": 4.0} and h[1] == 4.0
    sc, h, _ = run(kr.FIN_FCG_BETA)
    assert changed(sc) == {"ZR": 8.0, "RZ": 8.0, "BETA": -16.0 / 2.5}
    # breakdowns: plain IEEE arithmetic
    z = np.zeros(2)
    sc, _, _ = kr.finalize(kr.FIN_BICG_OMEGA, p0, z, base)
    assert sc[S["OMEGA1"]] == 0.0 and sc[S["ASAS"]] == 0.0
    sc, _, _ = kr.finalize(kr.FIN_PCG_ALPHA, z, None, base)
    assert sc[S["ALPHA"]] == math.inf and sc[S["NALPHA"]] == -math.inf
    zero_rz = base.copy()
    zero_rz[S["RZ"]] = 0.0
    sc, _, _ = kr.finalize(kr.FIN_PCG_ALPHA, z, None, zero_rz)
    assert math.isnan(sc[S["ALPHA"]]) and math.isnan(sc[S["NALPHA"]])
    sc, h, _ = kr.finalize(kr.FIN_SQRT, np.array([1.0, math.nan]), None, base, S["RES"], hist, 0)
    assert math.isnan(h[0]) and math.isnan(sc[S["RES"]])
    # the slot: explicit, clamped, or from the counter -- which only a code that stores a residual advances
    assert kr.finalize(kr.FIN_SQRT, p1, None, base, S["RES"], hist, 9)[1][3] == 4.0
    sc, h, ctr = kr.finalize(kr.FIN_SQRT, p1, None, base, S["RES"], hist, -1, 2)
    assert h[2] == 4.0 and ctr == 3
    assert kr.finalize(kr.FIN_STORE, p1, None, base, S["TMP"], hist, -1, 2)[2] == 2
    assert kr.finalize(kr.FIN_SQRT, p1, None, base, S["RES"], None, -1, 2)[2] == 2
    # modes 1 and 2 together are mode 0
    for code in range(11):
        m1 = kr.finalize(code, p0, p1, base, S["TMP"], hist, 1, 0, mode=1)
        assert {kr.SLOTS[k] for k in range(kr.S_COUNT) if m1[0][k] != base[k]} == {"SUM0", "SUM1"}
        m2 = kr.finalize(code, None, None, m1[0], S["TMP"], hist, 1, 0, mode=2)
        m0 = kr.finalize(code, p0, p1, base, S["TMP"], hist, 1, 0)
        keep = [k for k in range(kr.S_COUNT) if kr.SLOTS[k] not in ("SUM0", "SUM1")]
        assert np.array_equal(m2[0][keep], m0[0][keep]) and np.array_equal(m2[1], m0[1])


def test_krylov_op_hooks_reject_bad_arguments():
    """sparsh_op_dot2 ... sparsh_op_finalize: a bad argument is SPARSH_EINVAL before any device is asked for"""
    rp, ci, v = problems.poisson2d(8)
    A = sa.sp_matrix_mg(rp, ci, v)
    A.setup(sa.default_params(print_setup=0), host_only=True)
    dp = C.POINTER(C.c_double)
    bufs = [np.zeros(sa.OP_PARTIALS + sa.OP_PAD) for _ in range(4)]
    p, q, s, t = (b.ctypes.data_as(dp) for b in bufs)
    nb, ctr = C.c_int(), C.c_int(0)
    L, h = sa.lib, A._h
    vec = {
        "dot2": lambda h, n: L.sparsh_op_dot2(h, n, p, p, q, q, s, t, C.byref(nb)),
        "cg_update": lambda h, n: L.sparsh_op_cg_update(h, n, 0.5, -0.5, p, q, None, s, t, C.byref(nb), 0, None, 1.0, 1.0, 0, None),
        "p_update": lambda h, n: L.sparsh_op_p_update(h, n, 0.5, p, q),
        "xp_update": lambda h, n: L.sparsh_op_xp_update(h, n, 0.5, 0.5, p, q, s),
        "bicg_s": lambda h, n: L.sparsh_op_bicg_s(h, n, 0.5, p, q, s),
        "bicg_xr": lambda h, n: L.sparsh_op_bicg_xr(h, n, 0.5, 0.5, p, p, p, p, p, q, s, t, bufs[0][8:].ctypes.data_as(dp), C.byref(nb)),
        "bicg_p": lambda h, n: L.sparsh_op_bicg_p(h, n, 0.5, 0.5, p, q, s),
    }
    for name, call in vec.items():
        assert call(None, 4) == sa.SPARSH_EINVAL, name
        assert b"null handle" in L.sparsh_last_error()
        for n in (0, -5):
            assert call(h, n) == sa.SPARSH_EINVAL, name
            assert b"n <= 0" in L.sparsh_last_error()
        assert call(h, 4) == sa.SPARSH_ESTATE, name  # good arguments, no device setup: a state error
    assert L.sparsh_op_dot2(h, 4, p, None, q, q, s, t, C.byref(nb)) == sa.SPARSH_EINVAL
    assert L.sparsh_op_dot2(h, 4, p, p, q, q, s, s, C.byref(nb)) == sa.SPARSH_EINVAL  # one array for both results
    assert L.sparsh_op_p_update(h, 4, 0.5, None, q) == sa.SPARSH_EINVAL
    assert L.sparsh_op_xp_update(h, 4, 0.5, 0.5, p, q, None) == sa.SPARSH_EINVAL
    assert L.sparsh_op_bicg_s(h, 4, 0.5, p, q, None) == sa.SPARSH_EINVAL
    assert L.sparsh_op_bicg_p(h, 4, 0.5, 0.5, p, None, s) == sa.SPARSH_EINVAL
    cgu = lambda r, zero, nt, z0: L.sparsh_op_cg_update(h, 4, 0.5, -0.5, p, q, None, r, t, C.byref(nb), zero, None, 1.0, 1.0, nt, z0)
    assert cgu(None, 0, 0, None) == sa.SPARSH_EINVAL
    assert cgu(s, 2, 0, None) == sa.SPARSH_EINVAL
    assert cgu(s, 0, 3, None) == sa.SPARSH_EINVAL
    assert cgu(s, 1, 0, None) == sa.SPARSH_EINVAL and b"z0" in L.sparsh_last_error()
    assert cgu(s, 1, 0, s) == sa.SPARSH_EINVAL
    fin = lambda h=h, code=1, mode=0, p0=p, nblk=4, p1=None, nblk1=0, scal=q, slot=0, hist=s, cap=4, it=0, ctr=ctr, repeat=1: \
        L.sparsh_op_finalize(h, code, mode, p0, nblk, p1, nblk1, scal, slot, hist, cap, it, None if ctr is None else C.byref(ctr), repeat)
    assert fin(h=None) == sa.SPARSH_EINVAL and b"null handle" in L.sparsh_last_error()
    bad = [dict(code=-1), dict(code=11), dict(mode=-1), dict(mode=3), dict(p0=None), dict(scal=None), dict(ctr=None), dict(nblk=0),
           dict(p1=t, nblk1=0), dict(slot=-1), dict(slot=sa.OP_SCALARS), dict(cap=0), dict(ctr=C.c_int(-1)), dict(repeat=0),
           dict(repeat=65)]
    for kw in bad:
        assert fin(**kw) == sa.SPARSH_EINVAL, kw
    for kw in (dict(), dict(mode=2, p0=None), dict(hist=None, cap=0), dict(p1=t, nblk1=3, code=9, it=-1, repeat=64)):
        assert fin(**kw) == sa.SPARSH_ESTATE, kw
    with pytest.raises(sa.SparshError) as e:
        A.op_dot2(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4))
    assert e.value.code == sa.SPARSH_ESTATE
