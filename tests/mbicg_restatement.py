"""numpy restatement of block BiCGStab: the kernels of mbicg_kernels.hip -- dot2_multi, bicg_s_multi,
bicg_xr_multi, bicg_p_multi and the finalise with its four codes -- and Engine::solve_mbicg_dev composed from them, in the kernels'
own order of operations, so that a GPU result can be compared bit for bit.  Blocks are arrays of shape (n, nrhs); per column the
expressions are those of krylov_ops_restatement (bicg_s, bicg_xr, bicg_p, FIN_BICG_ALPHA / OMEGA / BETA), parentheses included.

Order of a reducing launch: per column that of the single-vector kernels, whatever the width -- a lane owns a whole row of the
block, so column c's terms are added as krylov_ops_restatement.partials adds a vector's (ew_grid(n) workgroups of 256 threads, thread
t of workgroup w adds the rows 256 w + t, + 256 g, ... from 0.0, the shuffle tree per wave, the four waves in order), and the finalise
adds a column's partials as finalize_kernel does (krylov_ops_restatement.fin_sum).  The launches without a reduction keep a lane on
two neighbouring columns of one row, 512 / W rows per pass and workgroup; their grid rule is elementwise_grid."""
import math

import numpy as np

import krylov_ops_restatement as kr

K_BLOCK = 256     # kBlock
GRID_MAX = 2048   # kMultiGridMax
SLOTS = ("ALPHA1", "APR0", "ALPHA", "ASS", "ASAS", "OMEGA1", "BETA", "RR0", "RES")  # enum MbicgSlot
S = {name: k for k, name in enumerate(SLOTS)}
STATUS_NUMERIC = 1  # kMultiStatusNumeric


def width(nrhs):
    return 2 if nrhs <= 2 else (4 if nrhs <= 4 else 8)


def rows_per_pass(W):
    """rows one workgroup of an S or P launch covers per pass"""
    return 2 * K_BLOCK // W


def elementwise_grid(n, W):
    """mbicg_grid: workgroups of an S or P launch"""
    return min(GRID_MAX, max(1, -(-n // rows_per_pass(W))))


def grid(n, W=None):
    """mbicg_reduce_grid: workgroups of a reducing launch = partial sums per column"""
    return kr.ew_grid(n)


def partials(terms, W=None):
    """terms (n, nrhs) -> (nrhs, grid(n)): the partial sums a reducing launch stores for the per-element terms (W plays no part)"""
    terms = np.asarray(terms, dtype=np.float64)
    return np.stack([kr.partials(terms[:, c]) for c in range(terms.shape[1])])


def fin_sum(p):
    """p (nrhs, m) -> (nrhs,): the sums the finalise forms of every column's partials"""
    return np.array([kr.fin_sum(row) for row in np.asarray(p, dtype=np.float64)])


# ---- the vector kernels: every function returns new arrays; a frozen column comes back as it went in

def _live(frozen, k):
    return np.ones(k, dtype=bool) if frozen is None else np.asarray(frozen) == 0


def dot2(a, b, c, d, W=None):
    return partials(a * b, W), partials(c * d, W)


def bicg_s(alpha, R, AP, S, frozen=None):
    live = _live(frozen, R.shape[1])
    with np.errstate(all="ignore"):
        return np.where(live, R - alpha * AP, S)


def bicg_xr(alpha, omega, P1, S1, S_, AS, R0, X, R, frozen=None, W=None):
    """(X, R, partial sums of R.R0, partial sums of R.R)"""
    live = _live(frozen, R.shape[1])
    with np.errstate(all="ignore"):
        Xn = np.where(live, (X + alpha * P1) + omega * S1, X)
        Rn = np.where(live, S_ - omega * AS, R)
        return Xn, Rn, partials(Rn * R0, W), partials(Rn * Rn, W)


def bicg_p(beta, omega, R, AP, P, frozen=None):
    live = _live(frozen, R.shape[1])
    with np.errstate(all="ignore"):
        return np.where(live, R + beta * (P - omega * AP), P)


# ---- the finalise

def new_state(nrhs):
    return dict(scal=np.zeros((len(SLOTS), nrhs)), frozen=np.zeros(nrhs, dtype=np.int32), iters=np.zeros(nrhs, dtype=np.int32),
                status=np.zeros(nrhs, dtype=np.int32))


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan  # (sqrt(-0.0) = -0.0 as on the device)


def finalize(code, part0, part1, state, tol, hist=None, it=0):
    """One launch on the nrhs columns in use: (state, hist), both new.  hist: (nrhs, hist_cap) or None."""
    st = {k: np.array(v) for k, v in state.items()}
    sc = st["scal"]
    h = None if hist is None else np.array(hist, dtype=np.float64)
    s0 = fin_sum(part0)
    s1 = fin_sum(part1) if part1 is not None else np.zeros(len(s0))
    f = np.float64

    def freeze_on(c, res, iters):
        if res <= tol or res != res:
            st["frozen"][c], st["iters"][c], st["status"][c] = 1, iters, 0 if res == res else STATUS_NUMERIC

    with np.errstate(all="ignore"):
        for c in range(len(s0)):
            a, b = f(s0[c]), f(s1[c])
            if code == "init":
                sc[:, c] = 0.0
                res = _sqrt(a)
                sc[S["RES"], c] = res
                st["frozen"][c] = st["iters"][c] = st["status"][c] = 0
                freeze_on(c, res, 0)
                continue
            if st["frozen"][c]:
                continue
            if code == "alpha":
                sc[S["ALPHA1"], c], sc[S["APR0"], c], sc[S["ALPHA"], c] = a, b, a / b
            elif code == "omega":
                sc[S["ASS"], c], sc[S["ASAS"], c] = a, b
                sc[S["OMEGA1"], c] = f(0.0) if b == 0.0 else a / b
            elif code == "beta_res":
                beta = a / f(sc[S["ALPHA1"], c])
                beta = beta * (f(sc[S["ALPHA"], c]) / f(sc[S["OMEGA1"], c]))
                sc[S["BETA"], c], sc[S["RR0"], c] = beta, a
                res = _sqrt(b)
                sc[S["RES"], c] = res
                if h is not None and it < h.shape[1]:
                    h[c, it] = res
                st["iters"][c] = it + 1
                freeze_on(c, res, it + 1)
            else:
                raise ValueError(code)
    return st, h


# ---- Engine::solve_mbicg_dev.  spmv(V) = A V and precond(V) = M V act on blocks column by column (precond None: the identity).

def mbicg_loop(spmv, precond, B, X0, tol, max_iters, W=None, init_partials=None):
    """(X, histories, iters, status) with status 0 converged, STATUS_NUMERIC, or -1 for a column still running at the cap.
    init_partials(terms): the partial sums of the launch that forms ||r0||^2 (the block PCG's dot launch, whose order is not the
    one of partials(); the default takes partials())."""
    B = np.asarray(B, dtype=np.float64)
    n, k = B.shape
    W = W or width(k)
    M = (lambda V: V) if precond is None else precond
    X = np.array(X0, dtype=np.float64)
    with np.errstate(all="ignore"):
        R0 = B - spmv(X)
        R, P = R0.copy(), R0.copy()
        Sb = np.zeros_like(R0)
        st, _ = finalize("init", (init_partials or (lambda t: partials(t, W)))(R0 * R0), None, new_state(k), tol)
        hist = np.zeros((k, max(max_iters, 1)))
        it = 0
        while not st["frozen"].all() and it < max_iters:
            P1 = M(P)
            AP = spmv(P1)
            st, _ = finalize("alpha", *dot2(R, R0, AP, R0, W), st, tol)
            Sb = bicg_s(st["scal"][S["ALPHA"]], R, AP, Sb, st["frozen"])
            S1 = M(Sb)
            AS = spmv(S1)
            st, _ = finalize("omega", *dot2(AS, Sb, AS, AS, W), st, tol)
            X, R, q0, q1 = bicg_xr(st["scal"][S["ALPHA"]], st["scal"][S["OMEGA1"]], P1, S1, Sb, AS, R0, X, R, st["frozen"], W)
            st, hist = finalize("beta_res", q0, q1, st, tol, hist, it)
            P = bicg_p(st["scal"][S["BETA"]], st["scal"][S["OMEGA1"]], R, AP, P, st["frozen"])
            it += 1
    status = np.where(st["frozen"] == 0, -1, st["status"])
    return X, [hist[c, : st["iters"][c]].copy() for c in range(k)], st["iters"].copy(), status
