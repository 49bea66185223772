"""numpy restatement of the LOBPCG eigensolver (include/sparsh_amg.h, steps 1-6), with the operator and the
preconditioner passed in as callables on (n, k) blocks.  A helper of test_eig_host.py and test_gpu_eig.py, not collected by pytest."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
BREAKDOWN_PIVOT = 1e-7


def mirror_upper(G):
    """the matrix the solver sees: the upper triangle, mirrored"""
    return np.triu(G) + np.triu(G, 1).T


def small_eig(GA, GB, k):
    """Step 5 on a compacted pencil: (breakdown, theta[k], C (m, k)).  Every sum runs in the order of the library's eig_small (sums
    over p ascending, one rounding per product and per sum), vectorised only across entries that do not depend on each other: on a
    host without contracted multiply-adds the two give the same bits."""
    GA, GB = mirror_upper(np.asarray(GA, dtype=np.float64)), mirror_upper(np.asarray(GB, dtype=np.float64))
    m = GA.shape[0]
    g = np.diag(GB)
    if not (np.all(np.isfinite(g)) and np.all(g > 0.0)):
        return 1, None, None
    d = 1.0 / np.sqrt(g)
    B = d[:, None] * GB * d[None, :]
    L = np.zeros((m, m))
    for j in range(m):  # Cholesky factor of D GB D
        col = B[j:, j].copy()
        for p in range(j):
            col = col - L[j:, p] * L[j, p]
        piv = math.sqrt(col[0]) if col[0] > 0.0 else 0.0
        if not piv >= BREAKDOWN_PIVOT:
            return 1, None, None
        L[j, j] = piv
        L[j + 1:, j] = col[1:] / piv
    T = d[:, None] * GA * d[None, :]
    for i in range(m):  # T <- L^-1 T
        s = T[i, :].copy()
        for p in range(i):
            s = s - L[i, p] * T[p, :]
        T[i, :] = s / L[i, i]
    for j in range(m):  # T <- T L^-T
        s = T[:, j].copy()
        for p in range(j):
            s = s - L[j, p] * T[:, p]
        T[:, j] = s / L[j, j]
    T = 0.5 * (T + T.T)
    Y = np.eye(m)
    for _ in range(64):  # cyclic Jacobi until the off-diagonal norm is at most eps ||T||_F
        off = diag = 0.0
        for i in range(m):
            diag += T[i, i] * T[i, i]
            for j in range(i + 1, m):
                off += 2.0 * T[i, j] * T[i, j]
        if not math.isfinite(off + diag):
            return 1, None, None
        if math.sqrt(off) <= EPS * math.sqrt(off + diag):
            break
        for p in range(m):
            for q in range(p + 1, m):
                apq = T[p, q]
                if apq == 0.0:
                    continue
                tau = (T[q, q] - T[p, p]) / (2.0 * apq)
                t = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + math.sqrt(1.0 + tau * tau))
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = t * c
                a, b = T[:, p].copy(), T[:, q].copy()
                T[:, p], T[:, q] = c * a - s * b, s * a + c * b
                a, b = T[p, :].copy(), T[q, :].copy()
                T[p, :], T[q, :] = c * a - s * b, s * a + c * b
                T[p, q] = T[q, p] = 0.0
                a, b = Y[:, p].copy(), Y[:, q].copy()
                Y[:, p], Y[:, q] = c * a - s * b, s * a + c * b
    order = np.argsort(np.diag(T), kind="stable")[:k]
    Z = np.zeros((m, k))
    for i in range(m - 1, -1, -1):  # L^T Z = Y[:, order]
        s = Y[i, order].copy()
        for p in range(i + 1, m):
            s = s - L[p, i] * Z[p, :]
        Z[i, :] = s / L[i, i]
    return 0, np.diag(T)[order].copy(), d[:, None] * Z


def row_times(B, Cm, acc=None):
    """sum_c B[:, c] Cm[c, :], c ascending, every product and sum rounded on its own; acc: the running sum this one continues"""
    for c in range(B.shape[1]):
        t = B[:, c:c + 1] * Cm[c:c + 1, :]
        acc = t if acc is None else acc + t
    return acc


def update(X, W, P, AX, AW, AP, Cx, Cw, Cp):
    """Step 6: (X', P', AX', AP')."""
    Pn = row_times(P, Cp, row_times(W, Cw))
    APn = row_times(AP, Cp, row_times(AW, Cw))
    return row_times(X, Cx) + Pn, Pn, row_times(AX, Cx) + APn, APn


def gram_blocks(gram, S, AS, k, nblocks):
    """(S^T A S, S^T S) from the upper block triangle of k x k blocks, as the solver forms them; gram(U, V) = U^T V"""
    m = nblocks * k
    GA, GB = np.zeros((m, m)), np.zeros((m, m))
    for bi in range(nblocks):
        for bj in range(bi, nblocks):
            r, c = slice(bi * k, (bi + 1) * k), slice(bj * k, (bj + 1) * k)
            GB[r, c] = gram(S[:, r], S[:, c])
            GA[r, c] = gram(S[:, r], AS[:, c])
    return mirror_upper(GA), mirror_upper(GB)


def lobpcg(apply_A, apply_M, X0, tol=1e-8, max_iters=1000, gram=None):
    """Steps 1-6; gram(U, V) = U^T V of two (n, k) blocks (None: numpy).  Returns a dict: lam, X, iters[c], hist (k, evaluations),
    status[c] (0 converged, 1 not), restarts, breakdown."""
    gram = gram or (lambda U, V: U.T @ V)
    X = np.array(X0, dtype=np.float64)
    n, k = X.shape
    out = dict(breakdown=False, restarts=0)
    AX = apply_A(X)
    bad, theta, Cm = small_eig(*gram_blocks(gram, X, AX, k, 1), k)
    if bad:
        return dict(out, breakdown=True)
    X, AX = row_times(X, Cm), row_times(AX, Cm)
    P, AP = np.zeros_like(X), np.zeros_like(X)
    have_p = False
    iters, hist = np.zeros(k, dtype=int), []
    it = 0
    while True:
        R = AX - X * theta
        rn = np.sqrt(np.sum(R * R, axis=0))
        hist.append(rn)
        active = rn > tol * np.abs(theta)
        if not active.any() or it >= max_iters:
            break
        W = apply_M(R)
        AW = apply_A(W)
        S, AS = np.hstack([X, W, P]), np.hstack([AX, AW, AP])
        GA, GB = gram_blocks(gram, S, AS, k, 3)
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
        X, P, AX, AP = update(X, W, P, AX, AW, AP, full[:k], full[k:2 * k], full[2 * k:])
        theta = th
        iters += active
        have_p = True
        it += 1
    return dict(out, lam=theta, X=X, iters=iters, hist=np.array(hist).T, status=active.astype(int))
