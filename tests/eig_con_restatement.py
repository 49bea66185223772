"""numpy restatement of the constrained LOBPCG eigensolver (include/sparsh_amg.h, sparsh_eigs_con): the loop of
eig_restatement.py / eig_gen_restatement.py with the projection Pi V = V - Y G^-1 (BY)^T V applied at the same two places, to the
start block and to the preconditioned residuals.  A helper of test_eig_con_host.py and test_gpu_eig_con.py, not collected by pytest."""
import math

import numpy as np

from eig_restatement import BREAKDOWN_PIVOT, mirror_upper, row_times, small_eig
from eig_gen_restatement import gram_blocks_gen, residual_gen, update_gen

DUMBBELL = (4, 3)  # problems.dumbbell_laplacian(a, bridge) of both test files: test_eig_con_host.py checks its Fiedler vector on the CPU


def spd_inverse(G):
    """(breakdown, Ginv): the library's eig_spd_inverse: scaling by diag(G)^-1/2, Cholesky with the breakdown rule of step 5, two
    triangular solves per column, symmetrised"""
    G = mirror_upper(np.asarray(G, dtype=np.float64))
    m = G.shape[0]
    g = np.diag(G)
    if not (np.all(np.isfinite(g)) and np.all(g > 0.0)):
        return 1, None
    d = 1.0 / np.sqrt(g)
    B = d[:, None] * G * d[None, :]
    L = np.zeros((m, m))
    for j in range(m):
        col = B[j:, j].copy()
        for p in range(j):
            col = col - L[j:, p] * L[j, p]
        piv = math.sqrt(col[0]) if col[0] > 0.0 else 0.0
        if not piv >= BREAKDOWN_PIVOT:
            return 1, None
        L[j, j] = piv
        L[j + 1:, j] = col[1:] / piv
    Z = np.eye(m)
    for i in range(m):  # L Z' = I
        s = Z[i, :].copy()
        for p in range(i):
            s = s - L[i, p] * Z[p, :]
        Z[i, :] = s / L[i, i]
    for i in range(m - 1, -1, -1):  # L^T Z = Z'
        s = Z[i, :].copy()
        for p in range(i + 1, m):
            s = s - L[p, i] * Z[p, :]
        Z[i, :] = s / L[i, i]
    return 0, d[:, None] * (0.5 * (Z + Z.T)) * d[None, :]


def coefficients(Ginv, C):
    """coef = Ginv C, coef_jc = sum_i Ginv_ji C_ic with i ascending from the product of i = 0, every product and sum rounded on its own"""
    acc = None
    for i in range(Ginv.shape[1]):
        t = Ginv[:, i:i + 1] * C[i:i + 1, :]
        acc = t if acc is None else acc + t
    return acc


def apply_projection(Y, Ginv, C, V):
    """the projection kernel given C = (BY)^T V: V - sum_j Y[:, j] coef[j, :], j ascending from the product of j = 0, one subtraction"""
    return V - row_times(Y, coefficients(Ginv, C))


class Projector:
    """Pi of one solve: Y (n, mt), BY = B Y, G = Y^T (BY) inverted once; gram(U, V) = U^T V (None: numpy)"""

    def __init__(self, Y, BY=None, gram=None):
        self.gram = gram or (lambda U, V: U.T @ V)
        self.Y = np.array(Y, dtype=np.float64)
        self.BY = self.Y if BY is None else np.array(BY, dtype=np.float64)
        self.bad, self.Ginv = spd_inverse(self.gram(self.Y, self.BY))

    def __call__(self, V):
        return apply_projection(self.Y, self.Ginv, self.gram(self.BY, V), V)


def lobpcg_con(apply_A, apply_M, X0, Y, apply_B=None, tol=1e-8, max_iters=1000, gram=None):
    """The constrained loop: the lowest pairs of A x = lam B x (apply_B None: B = I) with (B y_j)^T x = 0 for the columns of Y.  Returns
    the dict of eig_gen_restatement.lobpcg_gen, with rank_deficient=True (and nothing else) when Y^T B Y fails the Cholesky test."""
    gram = gram or (lambda U, V: U.T @ V)
    apply_B = apply_B or (lambda V: V)
    Y = np.array(Y, dtype=np.float64)
    Pi = Projector(Y, apply_B(Y), gram)
    out = dict(breakdown=False, restarts=0, rank_deficient=bool(Pi.bad))
    if Pi.bad:
        return out
    X = Pi(np.array(X0, dtype=np.float64))  # step 1: X <- Pi X before AX and BX
    n, k = X.shape
    AX, BX = apply_A(X), apply_B(X)
    bad, theta, Cm = small_eig(*gram_blocks_gen(gram, X, AX, BX, k, 1), k)
    if bad:
        return dict(out, breakdown=True)
    X, AX, BX = row_times(X, Cm), row_times(AX, Cm), row_times(BX, Cm)
    P, AP, BP = np.zeros_like(X), np.zeros_like(X), np.zeros_like(X)
    have_p = False
    iters, hist = np.zeros(k, dtype=int), []
    it = 0
    while True:
        R, rn, bn = residual_gen(AX, BX, theta)
        hist.append(rn)
        active = rn > tol * np.abs(theta) * bn
        if not active.any() or it >= max_iters:
            break
        W = Pi(apply_M(R))  # step 3: W <- Pi (M R) before AW and BW
        AW, BW = apply_A(W), apply_B(W)
        S, AS, BS = np.hstack([X, W, P]), np.hstack([AX, AW, AP]), np.hstack([BX, BW, BP])
        GA, GB = gram_blocks_gen(gram, S, AS, BS, k, 3)
        act = np.flatnonzero(active)
        idx_xw = np.concatenate([np.arange(k), k + act])
        idx = np.concatenate([idx_xw, 2 * k + act]) if have_p else idx_xw
        bad, th, Cm = small_eig(GA[np.ix_(idx, idx)], GB[np.ix_(idx, idx)], k)
        if bad:
            out["restarts"] += 1
            if not have_p:
                return dict(out, breakdown=True)
            idx = idx_xw
            bad, th, Cm = small_eig(GA[np.ix_(idx, idx)], GB[np.ix_(idx, idx)], k)
            if bad:
                return dict(out, breakdown=True)
        full = np.zeros((3 * k, k))
        full[idx, :] = Cm
        X, P, AX, AP, BX, BP = update_gen(X, W, P, AX, AW, AP, BX, BW, BP, full[:k], full[k:2 * k], full[2 * k:])
        theta = th
        iters += active
        have_p = True
        it += 1
    return dict(out, lam=theta, X=X, iters=iters, hist=np.array(hist).T, status=active.astype(int))
