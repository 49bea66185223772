"""Numpy restatement of block CG in the orders the library uses: the small solve with dropped directions, the
two block updates and the coupled loop.  Shared by the host and the GPU tests; imports nothing from the library.

Every product and every sum is rounded on its own; sums over the columns of a block run with c ascending from the product of c = 0.
"""
import numpy as np

PIVOT = 1e-14  # a pivot d_j <= PIVOT * g_jj drops direction j


def small(G, C, sign=1.0):
    """coef = sign * pinv(G) C by LDL^T of G (upper triangle read) without square roots and with dropped directions.  G and C are
    k x k.  Returns (coef, keep, rank); the rows of dropped directions are zero.  Python floats are IEEE doubles: only + - * / ."""
    G, C = np.asarray(G, dtype=np.float64), np.asarray(C, dtype=np.float64)
    k = G.shape[0]
    g = lambda i, j: float(G[min(i, j), max(i, j)])  # noqa: E731
    L = [[0.0] * k for _ in range(k)]
    d = [0.0] * k
    keep = [False] * k
    for j in range(k):
        acc = 0.0
        for m in range(j):
            if keep[m]:
                acc += (L[j][m] * L[j][m]) * d[m]
        d[j] = g(j, j) - acc
        keep[j] = g(j, j) > 0.0 and d[j] > PIVOT * g(j, j)
        if not keep[j]:
            continue
        for i in range(j + 1, k):
            s = 0.0
            for m in range(j):
                if keep[m]:
                    s += (L[i][m] * L[j][m]) * d[m]
            L[i][j] = (g(i, j) - s) / d[j]
    coef = np.zeros((k, k))
    for c in range(k):
        y = [0.0] * k
        for i in range(k):
            if keep[i]:
                s = 0.0
                for m in range(i):
                    if keep[m]:
                        s += L[i][m] * y[m]
                y[i] = float(C[i, c]) - s
        for i in range(k):
            if keep[i]:
                y[i] = y[i] / d[i]
        for i in range(k - 1, -1, -1):
            if keep[i]:
                s = 0.0
                for m in range(i + 1, k):
                    if keep[m]:
                        s += L[m][i] * y[m]
                y[i] = y[i] - s
        for i in range(k):
            coef[i, c] = sign * y[i] if keep[i] else 0.0
    return coef, np.array(keep, dtype=np.int32), int(sum(keep))


def times(Bk, coef):
    """Bk coef with the sum over c ascending from the product of c = 0"""
    T = Bk[:, 0:1] * coef[0:1, :]
    for c in range(1, Bk.shape[1]):
        T = T + Bk[:, c:c + 1] * coef[c:c + 1, :]
    return T


def update(X, R, P, Q, alpha):
    """(X + P alpha, R - Q alpha)"""
    return X + times(P, alpha), R - times(Q, alpha)


def direction(Z, P, beta):
    """Z + P beta"""
    return Z + times(P, beta)


def gram(U, V, chunk=0):
    """U^T V with the sum over the rows ascending (chunk = 0) or in chunks of `chunk` rows whose sums are added ascending"""
    prod = U[:, :, None] * V[:, None, :]
    if chunk <= 0:
        return prod.sum(axis=0)  # a reduction over the leading axis adds row after row
    parts = [prod[i:i + chunk].sum(axis=0) for i in range(0, len(prod), chunk)]
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


def norms(R, chunk=0):
    return np.sqrt(np.diagonal(gram(R, R, chunk)))


def bcg(apply_A, apply_M, B, X0, tol, cap, chunk=0):
    """Block CG on the n x k block B from X0.  apply_A and apply_M map blocks to blocks.  Returns (X, hist, info): hist[it, c] is
    column c's recurrence residual after iteration it + 1; info has iterations, min_rank, dropped, ranks and status ("ok", "noconv"
    at the cap, "numeric" on a NaN or on rank 0)."""
    B = np.asarray(B, dtype=np.float64)
    X = np.array(X0, dtype=np.float64)
    k = B.shape[1]
    R = B - apply_A(X)
    rn = norms(R, chunk)
    hist, ranks = [], []
    info = dict(iterations=0, min_rank=k, dropped=0, ranks=ranks, status="noconv")

    def finish(status):
        info.update(status=status, iterations=len(hist), min_rank=min(ranks + [k]), dropped=sum(k - r for r in ranks))
        return X, np.array(hist).reshape(len(hist), k), info

    if np.isnan(rn).any():
        return finish("numeric")
    if np.all(rn <= tol):
        return finish("ok")
    Z = apply_M(R)
    P = Z.copy()
    while len(hist) < cap:
        Q = apply_A(P)
        G, C1 = gram(P, Q, chunk), gram(P, R, chunk)
        alpha, _, rank = small(G, C1, 1.0)
        ranks.append(rank)
        if rank == 0:
            return finish("numeric")
        X, R = update(X, R, P, Q, alpha)
        rn = norms(R, chunk)
        hist.append(rn)
        if np.isnan(rn).any():
            return finish("numeric")
        if np.all(rn <= tol):
            return finish("ok")
        Z = apply_M(R)
        beta, _, _ = small(G, gram(Q, Z, chunk), -1.0)
        P = direction(Z, P, beta)
    return finish("noconv")


def pcg(apply_A, apply_M, b, x0, tol, cap):
    """textbook preconditioned CG on one vector: (x, hist)"""
    x = np.array(x0, dtype=np.float64)
    r = b - apply_A(x)
    hist = []
    if np.linalg.norm(r) <= tol:
        return x, np.array(hist)
    z = apply_M(r)
    p, rho = z.copy(), z @ r
    while len(hist) < cap:
        q = apply_A(p)
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        hist.append(np.linalg.norm(r))
        if hist[-1] <= tol:
            break
        z = apply_M(r)
        rho_new = z @ r
        p = z + (rho_new / rho) * p
        rho = rho_new
    return x, np.array(hist)


# ---------------------------------------------------------------------------- inputs of the small solve, shared by both test files

def spd(k, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((k, k))
    S = M @ M.T
    return 0.5 * (S + S.T) + k * np.eye(k)


def small_cases():
    """(name, G, C, expected keep mask): well-conditioned SPD matrices of every order, and the degenerate blocks"""
    out = []
    for k in range(1, 9):
        out.append((f"spd{k}", spd(k, k), np.random.default_rng(100 + k).standard_normal((k, k)), [1] * k))
    G = spd(6, 11)
    G[3, :], G[:, 3] = G[1, :].copy(), G[:, 1].copy()
    G[3, 3] = G[1, 1]
    G[1, 3] = G[3, 1] = G[1, 1]
    out.append(("duplicate", G, np.random.default_rng(111).standard_normal((6, 6)), [1, 1, 1, 0, 1, 1]))
    G = spd(5, 12)
    G[2, :] = 0.0
    G[:, 2] = 0.0
    out.append(("zero", G, np.random.default_rng(112).standard_normal((5, 5)), [1, 1, 0, 1, 1]))
    w = np.array([1.0, -2.0, 0.5, 3.0, 1.5, -0.75, 2.0, 1.0])
    out.append(("rank1", 3.7 * np.outer(w, w), np.random.default_rng(113).standard_normal((8, 8)), [1, 0, 0, 0, 0, 0, 0, 0]))
    # d_1 = (0.25 + delta) - 0.5 * 0.5 * 1 = delta exactly; the rule compares it with 1e-14 * (0.25 + delta) ~ 2.5e-15
    for name, delta, kept in (("below_pivot", 2.0 ** -49, 0), ("above_pivot", 2.0 ** -48, 1)):
        out.append((name, np.array([[1.0, 0.5], [0.5, 0.25 + delta]]), np.array([[1.0, 2.0], [3.0, 4.0]]), [1, kept]))
    out.append(("all_zero", np.zeros((3, 3)), np.ones((3, 3)), [0, 0, 0]))
    out.append(("negative", np.array([[-1.0, 0.0], [0.0, 2.0]]), np.ones((2, 2)), [0, 1]))
    out.append(("nan", np.array([[np.nan, 1.0], [1.0, 2.0]]), np.ones((2, 2)), [0, 1]))
    return out


def degenerate_block(B):
    """B (n x 8, independent columns) with a duplicate (column 5 = column 1), a zero (column 3) and a dependent column (6 = 0.5 * column 0
    - 2 * column 2): rank 5"""
    B = np.array(B, dtype=np.float64)
    B[:, 5] = B[:, 1]
    B[:, 3] = 0.0
    B[:, 6] = 0.5 * B[:, 0] - 2.0 * B[:, 2]
    return B
