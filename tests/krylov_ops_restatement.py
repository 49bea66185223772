"""numpy restatement of the single-vector Krylov kernels at the end of kernels.hip -- dot2, cg_update, cg_update_zero, p_update,
xp_update, bicg_s, bicg_xr, bicg_p -- and of finalize_kernel with its eleven codes, in the kernels' own order of operations, so that
a GPU result can be compared bit for bit.  The library is built with -ffp-contract=off: every product and every sum below is
rounded on its own, which is what numpy's elementwise operations do.

Order of a reducing elementwise launch: the grid is ew_grid(n) workgroups of 256 threads; thread t of workgroup w starts from 0.0
and adds its terms i = 256 w + t, + 256 g, ... in that order; a wave's 64 values are added by the __shfl_down halving tree as lane 0
sees it (v[l] + v[l + off], off = 32, 16, ..., 1); the four wave sums are added to 0.0 in wave order.  finalize_kernel: thread t of
1024 adds p[t], p[t + 1024], ... in order, the same tree per wave, the sixteen wave sums added to 0.0 in order, then the code's
scalar arithmetic.  (A thread's running sum starts at +0.0 and can never become -0.0, so the terms past the end that the vectorised
form below adds as +0.0 change nothing.)"""
import math

import numpy as np

K_BLOCK = 256        # kBlock
EW_GRID_MAX = 2048   # kEwGridMax
FIN_BLOCK = 1024     # kFinBlock

SLOTS = ("RZ", "PAP", "ALPHA", "NALPHA", "BETA", "RR", "RES", "ZR", "ALPHA1", "APR0", "ASS", "ASAS", "OMEGA1", "RR0", "TMP", "SUM0", "SUM1",
         "MEAN")
S = {name: k for k, name in enumerate(SLOTS)}  # enum Slot of kernels.hpp
S_COUNT = len(SLOTS)

FIN_STORE, FIN_SQRT, FIN_PCG_ALPHA, FIN_PCG_BETA, FIN_CG_BETA, FIN_CG_ALPHA, FIN_BICG_ALPHA, FIN_BICG_OMEGA, FIN_BICG_BETA, \
    FIN_PCG_BETA_RES, FIN_FCG_BETA = range(11)  # enum Fin of kernels.hpp
FIN_NAMES = ("STORE", "SQRT", "PCG_ALPHA", "PCG_BETA", "CG_BETA", "CG_ALPHA", "BICG_ALPHA", "BICG_OMEGA", "BICG_BETA", "PCG_BETA_RES",
             "FCG_BETA")
HIST_CODES = (FIN_SQRT, FIN_CG_BETA, FIN_BICG_BETA, FIN_PCG_BETA_RES)  # the codes that store a residual in the history
# what each code writes: (slots that come from sums, products, quotients or negation; slots that hold a square root)
FIN_WRITES = {
    FIN_STORE: ((), ()),  # + slot_a, exact
    FIN_SQRT: ((), ()),   # + slot_a, a square root
    FIN_PCG_ALPHA: (("PAP", "ALPHA", "NALPHA"), ()),
    FIN_PCG_BETA: (("ZR", "BETA", "RZ"), ()),
    FIN_CG_BETA: (("BETA", "RR"), ("RES",)),
    FIN_CG_ALPHA: (("PAP", "ALPHA", "NALPHA"), ()),
    FIN_BICG_ALPHA: (("ALPHA1", "APR0", "ALPHA"), ()),
    FIN_BICG_OMEGA: (("ASS", "ASAS", "OMEGA1"), ()),
    FIN_BICG_BETA: (("BETA", "RR0"), ("RES",)),
    FIN_PCG_BETA_RES: (("ZR", "BETA", "RZ"), ("RES",)),
    FIN_FCG_BETA: (("ZR", "RZ", "BETA"), ()),
}


def ew_grid(n):
    return min(EW_GRID_MAX, max(1, (n + 2 * K_BLOCK - 1) // (2 * K_BLOCK)))


def _wave_tree(v):
    """v[..., 64] -> the sum lane 0 holds after the __shfl_down halving tree"""
    off = 32
    while off > 0:
        v = v[..., :off] + v[..., off:2 * off]
        off >>= 1
    return v[..., 0]


def _strided_block_sums(terms, grid, block):
    """per-workgroup sums of `terms` under a grid-stride loop of grid x block threads, reduced as block_sum does"""
    n = len(terms)
    stride = grid * block
    rounds = max(1, (n + stride - 1) // stride)
    t = np.zeros(rounds * stride)
    t[:n] = terms
    t = t.reshape(rounds, stride)
    acc = np.zeros(stride)
    for k in range(rounds):
        acc = acc + t[k]
    waves = _wave_tree(acc.reshape(grid, block // 64, 64))
    s = np.zeros(grid)
    for w in range(block // 64):
        s = s + waves[:, w]
    return s


def partials(terms):
    """the ew_grid(n) partial sums a reducing elementwise launch stores for the per-element terms `terms`"""
    return _strided_block_sums(np.asarray(terms, dtype=np.float64), ew_grid(len(terms)), K_BLOCK)


def fin_sum(p):
    """the sum finalize_kernel forms of the partial sums p (any count >= 1)"""
    return float(_strided_block_sums(np.asarray(p, dtype=np.float64), 1, FIN_BLOCK)[0])


# ---- the vector kernels: every function returns new arrays

def dot2(a, b, c, d):
    return partials(a * b), partials(c * d)


def cg_update(alpha, nalpha, p, Ap, x, r):
    """(x or None, r, partial sums of r.r)"""
    xn = None if x is None else x + alpha * p
    rn = r + nalpha * Ap
    return xn, rn, partials(rn * rn)


def cg_update_zero(alpha, nalpha, p, Ap, x, r, d, dconst, omega):
    """(x or None, r, z0, partial sums of r.r); d None: the constant diagonal dconst"""
    xn, rn, part = cg_update(alpha, nalpha, p, Ap, x, r)
    return xn, rn, (omega * rn) / (dconst if d is None else d), part


def p_update(beta, z, p):
    return 1.0 * z + beta * p


def xp_update(alpha, beta, z, p, x):
    """(x, p)"""
    return x + alpha * p, 1.0 * z + beta * p


def bicg_s(alpha, r, Ap):
    return r - alpha * Ap


def bicg_xr(alpha, omega1, p1, s1, s, As, r0, x):
    """(x, r, partial sums of r.r0, partial sums of r.r)"""
    xn = (x + alpha * p1) + omega1 * s1
    rn = s - omega1 * As
    return xn, rn, partials(rn * r0), partials(rn * rn)


def bicg_p(beta, omega1, r, Ap, p):
    return r + beta * (p - omega1 * Ap)


# ---- finalize_kernel

def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan  # (sqrt(-0.0) = -0.0 as on the device)


def finalize(code, p0, p1=None, scal=None, slot=0, hist=None, it=0, counter=0, mode=0):
    """One launch: (scalar block, history or None, counter), all new.  mode 1 leaves the sums in SUM0 / SUM1, mode 2 takes them from
    there; hist_cap is len(hist); it < 0 takes the history slot from the counter."""
    f = np.float64
    sc = np.zeros(S_COUNT) if scal is None else np.array(scal, dtype=np.float64)
    h = None if hist is None else np.array(hist, dtype=np.float64)
    if mode != 2:
        s0 = f(fin_sum(p0))
        s1 = f(fin_sum(p1)) if p1 is not None else f(0.0)
        if mode == 1:
            sc[S["SUM0"]], sc[S["SUM1"]] = s0, s1
            return sc, h, counter
    else:
        s0, s1 = f(sc[S["SUM0"]]), f(sc[S["SUM1"]])
    hslot = it
    if h is not None and code in HIST_CODES and it < 0:
        hslot = counter
        counter += 1
    if h is not None and hslot >= len(h):
        hslot = len(h) - 1
    g = lambda name: f(sc[S[name]])

    def put(name, v):
        sc[S[name]] = v

    with np.errstate(all="ignore"):
        if code == FIN_STORE:
            sc[slot] = s0
        elif code == FIN_SQRT:
            v = _sqrt(s0)
            sc[slot] = v
            if h is not None:
                h[hslot] = v
        elif code in (FIN_PCG_ALPHA, FIN_CG_ALPHA):
            put("PAP", s0)
            alpha = g("RZ" if code == FIN_PCG_ALPHA else "RR") / s0
            put("ALPHA", alpha)
            put("NALPHA", -alpha)
        elif code in (FIN_PCG_BETA, FIN_PCG_BETA_RES):
            put("ZR", s0)
            put("BETA", s0 / g("RZ"))
            put("RZ", s0)
            if code == FIN_PCG_BETA_RES:
                v = _sqrt(s1)
                put("RES", v)
                if h is not None:
                    h[hslot] = v
        elif code == FIN_CG_BETA:
            s = g("RR")
            beta = s0 / s
            put("BETA", beta)
            res = _sqrt(s * beta)
            put("RES", res)
            put("RR", s0)
            if h is not None:
                h[hslot] = res
        elif code == FIN_BICG_ALPHA:
            put("ALPHA1", s0)
            put("APR0", s1)
            put("ALPHA", s0 / s1)
        elif code == FIN_BICG_OMEGA:
            put("ASS", s0)
            put("ASAS", s1)
            put("OMEGA1", f(0.0) if s1 == 0.0 else s0 / s1)
        elif code == FIN_BICG_BETA:
            beta = s0 / g("ALPHA1")
            beta = beta * (g("ALPHA") / g("OMEGA1"))
            put("BETA", beta)
            put("RR0", s0)
            res = _sqrt(s1)
            put("RES", res)
            if h is not None:
                h[hslot] = res
        elif code == FIN_FCG_BETA:
            put("ZR", s0)
            put("RZ", s0)
            put("BETA", -s1 / g("PAP"))
        else:
            raise ValueError(code)
    return sc, h, counter


# ---- the loops of engine.cpp composed from the pieces above.  spmv(v) = A v; precond(v) = M v (None: the identity).  They run
# `iters` iterations regardless of the residual, or (iters None) until the stored residual is <= tol, as check_every = 1 does.

# extra > 0 goes on for that many iterations past the one that would have ended the loop (what check_every > 1 can do); the history
# then holds `extra` entries more than check_every = 1 stores.

class _Stop:
    def __init__(self, tol, iters, cap, extra):
        self.tol, self.iters, self.cap, self.extra, self.m1 = tol, iters, cap, extra, None

    def go(self, res, count):
        if self.iters is not None:
            return count < self.iters
        if self.m1 is None and not (res > self.tol and count < self.cap):
            self.m1 = count
        return self.m1 is None or count < self.m1 + self.extra


def pcg_loop(spmv, precond, b, x0, tol, iters=None, cap=1 << 30, defer_x=True, extra=0):
    """Engine::pcg_init + pcg_body, precond None: the CG loop.  (x, history)"""
    stop = _Stop(tol, iters, min(cap, len(b)), extra)
    x = np.array(x0, dtype=np.float64)
    r = b - spmv(x)
    sc = np.zeros(S_COUNT)
    rr = partials(r * r)
    if precond is None:
        sc, _, _ = finalize(FIN_STORE, rr, None, sc, S["RR"])
    sc, _, _ = finalize(FIN_SQRT, rr, None, sc, S["RES"])
    z = r
    if precond is not None:
        z = precond(r)
        sc, _, _ = finalize(FIN_STORE, partials(z * r), None, sc, S["RZ"])
    p = z.copy()
    hist = []
    one = np.zeros(1)
    while stop.go(sc[S["RES"]] if not hist else hist[-1], len(hist)):
        Ap = spmv(p)
        sc, _, _ = finalize(FIN_PCG_ALPHA if precond is not None else FIN_CG_ALPHA, partials(p * Ap), None, sc)
        alpha, nalpha = sc[S["ALPHA"]], sc[S["NALPHA"]]
        if precond is not None:
            xn, r, part1 = cg_update(alpha, nalpha, p, Ap, None if defer_x else x, r)
            z = precond(r)
            sc, h, _ = finalize(FIN_PCG_BETA_RES, partials(z * r), part1, sc, 0, one, 0)
            if defer_x:
                x, p = xp_update(alpha, sc[S["BETA"]], z, p, x)
            else:
                x, p = xn, p_update(sc[S["BETA"]], z, p)
        else:
            x, r, part0 = cg_update(alpha, nalpha, p, Ap, x, r)
            sc, h, _ = finalize(FIN_CG_BETA, part0, None, sc, 0, one, 0)
            p = p_update(sc[S["BETA"]], r, p)
        hist.append(h[0])
    return x, np.array(hist)


def bicg_loop(spmv, precond, b, x0, tol, iters=None, cap=1 << 30, extra=0):
    """Engine::bicg, precond None: BiCGStab without a preconditioner.  (x, history)"""
    stop = _Stop(tol, iters, cap, extra)
    x = np.array(x0, dtype=np.float64)
    r0 = b - spmv(x)
    r, p = r0.copy(), r0.copy()
    sc, _, _ = finalize(FIN_SQRT, partials(r0 * r0), None, None, S["RES"])
    hist = []
    one = np.zeros(1)
    while stop.go(sc[S["RES"]] if not hist else hist[-1], len(hist)):
        p1 = p if precond is None else precond(p)
        Ap = spmv(p1)
        sc, _, _ = finalize(FIN_BICG_ALPHA, *dot2(r, r0, Ap, r0), sc)
        s = bicg_s(sc[S["ALPHA"]], r, Ap)
        s1 = s if precond is None else precond(s)
        As = spmv(s1)
        sc, _, _ = finalize(FIN_BICG_OMEGA, *dot2(As, s, As, As), sc)
        x, r, q0, q1 = bicg_xr(sc[S["ALPHA"]], sc[S["OMEGA1"]], p1, s1, s, As, r0, x)
        sc, h, _ = finalize(FIN_BICG_BETA, q0, q1, sc, 0, one, 0)
        p = bicg_p(sc[S["BETA"]], sc[S["OMEGA1"]], r, Ap, p)
        hist.append(h[0])
    return x, np.array(hist)


def fcg_loop(spmv, precond, b, x0, tol, iters=None, cap=1 << 30, extra=0):
    """Engine::fcg.  (x, history)"""
    stop = _Stop(tol, iters, cap, extra)
    x = np.array(x0, dtype=np.float64)
    r = b - spmv(x)
    sc, _, _ = finalize(FIN_SQRT, partials(r * r), None, None, S["RES"])
    z = precond(r)
    sc, _, _ = finalize(FIN_STORE, partials(z * r), None, sc, S["RZ"])
    p = z.copy()
    hist = []
    one = np.zeros(1)
    while stop.go(sc[S["RES"]] if not hist else hist[-1], len(hist)):
        Ap = spmv(p)
        sc, _, _ = finalize(FIN_PCG_ALPHA, partials(p * Ap), None, sc)
        x, r, part1 = cg_update(sc[S["ALPHA"]], sc[S["NALPHA"]], p, Ap, x, r)
        sc, h, _ = finalize(FIN_SQRT, part1, None, sc, S["RES"], one, 0)
        z = precond(r)
        sc, _, _ = finalize(FIN_FCG_BETA, *dot2(z, r, z, Ap), sc)
        p = p_update(sc[S["BETA"]], z, p)
        hist.append(h[0])
    return x, np.array(hist)
