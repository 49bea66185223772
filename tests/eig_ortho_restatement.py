"""numpy restatement of the LOBPCG loop under SPARSH_EIG_BASIS_ORTHO (include/sparsh_amg.h, sparsh_set_eig_options; DESIGN.md section
5i): the loop of eig_restatement.py / eig_gen_restatement.py / eig_con_restatement.py with W made B-orthogonal to X and to P and
B-orthonormalised by two passes of Cholesky-QR, P B-orthonormalised on its active columns, the masks that go with both, the drops
and the guard vectors (`wanted`).  The operators, the preconditioner and the Gram product are callables on (n, k) blocks.  A helper
of test_eig_ortho_host.py and test_gpu_eig_ortho.py, not collected by pytest."""
import math

import numpy as np

from eig_restatement import BREAKDOWN_PIVOT, row_times, small_eig
from eig_gen_restatement import gram_blocks_gen, update_gen
from eig_con_restatement import Projector


def chol_ortho(G, mask_in):
    """The small step of one orthonormalisation: (T, mask_out) with V T B-orthonormal on the kept columns for G = V^T (B V).  Only the
    upper triangle of G (order m <= 8) is read, and only the rows and columns i with mask_in[i].  The library's eig_chol, operation by
    operation: D = diag(G)^-1/2, the Cholesky factor of D G D row by row over the kept columns (sums over p ascending, one rounding per
    product and per sum), T = D L^-T by a backward substitution per column.  An active column whose diagonal is not finite and
    positive, or whose pivot is below the 1e-7 of step 5, is dropped: column of T zero, mask_out[i] = 0."""
    Gl = np.asarray(G, dtype=np.float64).tolist()
    m = len(Gl)
    d, L = [0.0] * m, [[0.0] * m for _ in range(m)]
    kept = []
    for i in range(m):
        if not mask_in[i]:
            continue
        g = Gl[i][i]
        if not (g > 0.0 and math.isfinite(g)):
            continue
        d[i] = 1.0 / math.sqrt(g)
        for j in kept:
            s = d[i] * Gl[j][i] * d[j]  # (j < i: the upper triangle)
            for p in kept:
                if p < j:
                    s -= L[i][p] * L[j][p]
            L[i][j] = s / L[j][j]
        s = d[i] * g * d[i]
        for p in kept:
            s -= L[i][p] * L[i][p]
        piv = math.sqrt(s) if s > 0.0 else 0.0
        if not piv >= BREAKDOWN_PIVOT:  # (a NaN lands here too)
            continue
        L[i][i] = piv
        kept.append(i)
    T, mask_out = np.zeros((m, m)), np.zeros(m, dtype=np.int32)
    for j in kept:
        mask_out[j] = 1
        z = [0.0] * m
        for i in reversed([q for q in kept if q <= j]):
            s = 1.0 if i == j else 0.0
            for p in kept:
                if i < p <= j:
                    s -= L[p][i] * z[p]
            z[i] = s / L[i][i]
            T[i, j] = d[i] * z[i]
    return T, mask_out


def transform(V, T):
    """V T, row by row: sum_c V[:, c] T[c, :], c ascending from the product of c = 0, every product and sum rounded on its own"""
    return row_times(V, T)


def ortho_apply(X, C, W0, mask):
    """W = W0 - X C on the columns of the mask (the sum over j ascending from the product of j = 0, one subtraction at the end),
    exact zeros elsewhere"""
    return np.where(np.asarray(mask, dtype=bool)[None, :], W0 - row_times(X, C), 0.0)


def active_mask(rn, theta, tol, bn=None):
    """the rule of step 2 on the norms of the residual kernel; bn: ||B x_c|| of the generalised form"""
    bound = tol * np.abs(theta)
    return (rn > (bound if bn is None else bound * bn)).astype(np.int32)


def lobpcg_ortho(apply_A, apply_M, X0, apply_B=None, Y=None, tol=1e-8, max_iters=1000, gram=None, wanted=0, trace=None):
    """Steps 1-6 under SPARSH_EIG_BASIS_ORTHO.  apply_B None: the standard problem (BX is X).  Y: constraints (None: none); the
    projection is that of eig_con_restatement.  wanted: 0 or k for all columns, else the solve ends once the columns below it are
    inactive.  trace: called as trace(it, rn, theta, active, out) at every evaluation of the residual.  Returns a dict: lam, X, iters[c], hist (k, evaluations), status[c] (0 inactive at the end, 1 still active), restarts,
    dropped_w, dropped_p, breakdown, converged."""
    gram = gram or (lambda U, V: U.T @ V)
    gen = apply_B is not None
    B = apply_B if gen else (lambda V: V)
    X = np.array(X0, dtype=np.float64)
    n, k = X.shape
    need = wanted if 0 < wanted < k else k
    out = dict(breakdown=False, restarts=0, dropped_w=0, dropped_p=0, rank_deficient=False)
    Pi = None
    if Y is not None and np.shape(Y)[1] > 0:
        Y = np.array(Y, dtype=np.float64)
        Pi = Projector(Y, B(Y), gram)
        if Pi.bad:
            return dict(out, rank_deficient=True)
        X = Pi(X)
    AX, BX = apply_A(X), B(X)
    bad, theta, Cm = small_eig(*gram_blocks_gen(gram, X, AX, BX, k, 1), k)
    if bad:
        return dict(out, breakdown=True)
    X, AX = row_times(X, Cm), row_times(AX, Cm)
    BX = row_times(BX, Cm) if gen else X
    P, AP, BP = np.zeros_like(X), np.zeros_like(X), np.zeros_like(X)
    have_p = False
    iters, hist = np.zeros(k, dtype=int), []
    it, converged = 0, False
    while True:
        R = AX - BX * theta
        rn = np.sqrt(np.sum(R * R, axis=0))
        hist.append(rn)
        active = active_mask(rn, theta, tol, np.sqrt(np.sum(BX * BX, axis=0)) if gen else None)
        if trace is not None:
            trace(it, rn, theta, active, out)
        if not active[:need].any():
            converged = True
            break
        if it >= max_iters:
            break
        pmask = np.zeros(k, dtype=np.int32)
        if have_p:
            T, pmask = chol_ortho(gram(P, BP if gen else P), active)
            P, AP = transform(P, T), transform(AP, T)
            if gen:
                BP = transform(BP, T)
            out["dropped_p"] += int(np.count_nonzero(active & (1 - pmask)))
        W0 = apply_M(R)
        if Pi is not None:
            W0 = Pi(W0)
        W = ortho_apply(X, gram(BX, W0), W0, active)
        if have_p:  # against the orthonormalised P as well (its dropped and inactive columns are zero)
            W = ortho_apply(P, gram(BP if gen else P, W), W, active)
        BW = B(W) if gen else W
        wmask = active
        for _ in range(2):  # Cholesky-QR twice; B W follows W by the same transform
            T, wmask = chol_ortho(gram(W, BW), wmask)
            W = transform(W, T)
            BW = transform(BW, T) if gen else W
        out["dropped_w"] += int(np.count_nonzero(active & (1 - wmask)))
        AW = apply_A(W)
        S, AS, BS = np.hstack([X, W, P]), np.hstack([AX, AW, AP]), np.hstack([BX, BW, BP if gen else P])
        GA, GB = gram_blocks_gen(gram, S, AS, BS, k, 3)
        idx_xw = np.concatenate([np.arange(k), k + np.flatnonzero(wmask)])
        idx = np.concatenate([idx_xw, 2 * k + np.flatnonzero(pmask)])
        bad, th, Cm = small_eig(GA[np.ix_(idx, idx)], GB[np.ix_(idx, idx)], k)
        if bad:
            out["restarts"] += 1
            if len(idx) == len(idx_xw):
                return dict(out, breakdown=True)
            idx = idx_xw
            bad, th, Cm = small_eig(GA[np.ix_(idx, idx)], GB[np.ix_(idx, idx)], k)
            if bad:
                return dict(out, breakdown=True)
        full = np.zeros((3 * k, k))
        full[idx, :] = Cm
        X, P, AX, AP, BXn, BP = update_gen(X, W, P, AX, AW, AP, BX, BW, BP if gen else P, full[:k], full[k:2 * k], full[2 * k:])
        BX = BXn if gen else X
        theta = th
        iters += active
        have_p = True
        it += 1
    return dict(out, lam=theta, X=X, iters=iters, hist=np.array(hist).T, status=np.asarray(active, dtype=int), converged=converged)
