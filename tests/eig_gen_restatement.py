"""numpy restatement of the generalised LOBPCG eigensolver A x = lambda B x (include/sparsh_amg.h, sparsh_eigs_gen; DESIGN.md section
5i), with both operators and the preconditioner passed in as callables on (n, k) blocks.  The small eigenproblem, the order of the
update's sums and the mirroring are those of eig_restatement.py.  A helper of test_eig_gen_host.py and test_gpu_eig_gen.py, not
collected by pytest."""
import numpy as np

from eig_restatement import mirror_upper, row_times, small_eig


def residual_gen(AX, BX, theta):
    """Step 2: (R, rn, bn) with R = AX - BX * theta, the product and the subtraction rounded separately."""
    R = AX - BX * theta
    return R, np.sqrt(np.sum(R * R, axis=0)), np.sqrt(np.sum(BX * BX, axis=0))


def update_gen(X, W, P, AX, AW, AP, BX, BW, BP, Cx, Cw, Cp):
    """Step 6: (X', P', AX', AP', BX', BP'), the same coefficients on S, A S and B S."""
    Pn = row_times(P, Cp, row_times(W, Cw))
    APn = row_times(AP, Cp, row_times(AW, Cw))
    BPn = row_times(BP, Cp, row_times(BW, Cw))
    return row_times(X, Cx) + Pn, Pn, row_times(AX, Cx) + APn, APn, row_times(BX, Cx) + BPn, BPn


def gram_blocks_gen(gram, S, AS, BS, k, nblocks):
    """(S^T A S, S^T B S) from the upper block triangle of k x k blocks, the pairs (S_i, AS_j) and (S_i, BS_j); gram(U, V) = U^T V"""
    m = nblocks * k
    GA, GB = np.zeros((m, m)), np.zeros((m, m))
    for bi in range(nblocks):
        for bj in range(bi, nblocks):
            r, c = slice(bi * k, (bi + 1) * k), slice(bj * k, (bj + 1) * k)
            GB[r, c] = gram(S[:, r], BS[:, c])
            GA[r, c] = gram(S[:, r], AS[:, c])
    return mirror_upper(GA), mirror_upper(GB)


def lobpcg_gen(apply_A, apply_B, apply_M, X0, tol=1e-8, max_iters=1000, gram=None):
    """Steps 1-6 for the pencil (A, B); gram(U, V) = U^T V of two (n, k) blocks (None: numpy).  Returns a dict: lam, X, iters[c], hist
    (k, evaluations) of ||A x_c - lam_c B x_c||, status[c] (0 converged, 1 not), restarts, breakdown."""
    gram = gram or (lambda U, V: U.T @ V)
    X = np.array(X0, dtype=np.float64)
    n, k = X.shape
    out = dict(breakdown=False, restarts=0)
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
        W = apply_M(R)
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


# ---------------------------------------------------------------------------- the pencils both test files solve

def diag_b(n):
    """B = diag(1 + (i mod 7) / 3) as a CSR triple"""
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), 1.0 + (np.arange(n) % 7) / 3.0


def pencil_p3_diag():
    from sparsh_amg_amd import problems
    A = problems.poisson3d(12, 10, 9)
    return A, diag_b(len(A[0]) - 1)


def pencil_fem():
    from sparsh_amg_amd import problems
    return problems.fem_pencil(3000)


# name -> (pencil, hierarchy parameters); the levels the coarsening then builds: 5, 4 and 1
PENCILS = {
    "p3_diag": (pencil_p3_diag, dict(limit_upper=100, limit_lower=50)),
    "fem_ml": (pencil_fem, dict(limit_upper=400, limit_lower=200)),
    "fem_1l": (pencil_fem, dict()),
}
# (pencil, k): the whole solves of the GPU suite; test_eig_gen_host.py holds each to half the iteration cap with the oracle's cycle
SOLVES = [("p3_diag", 1), ("p3_diag", 3), ("p3_diag", 8), ("fem_ml", 4), ("fem_ml", 8), ("fem_1l", 8)]
CAP = 300
TOL = 1e-8


def dense_reference(A, B, k):
    """(the k + 1 lowest eigenvalues of the dense pencil, cond_2(B), ||A||_inf, ||B||_inf) from CSR triples"""
    import scipy.linalg
    import scipy.sparse as sp
    n = len(A[0]) - 1
    Ad = sp.csr_matrix((A[2], A[1], A[0]), shape=(n, n)).toarray()
    Bd = sp.csr_matrix((B[2], B[1], B[0]), shape=(n, n)).toarray()
    lam = scipy.linalg.eigh(Ad, Bd, eigvals_only=True, subset_by_index=[0, k])
    wb = scipy.linalg.eigvalsh(Bd)
    return lam, wb[-1] / wb[0], np.abs(Ad).sum(axis=1).max(), np.abs(Bd).sum(axis=1).max()


def check_solution(name, k, lam, X, A, B, ref):
    """the asserts of a whole solve at TOL: ascending, eigenvalues within the first-order bound tol lam sqrt(cond_2(B)) of the dense
    pencil's, true residuals within the stopping rule plus the rounding floor of forming them, B-orthonormal vectors.  Returns the
    figures (worst eigenvalue error / bound, worst residual / bound, B-orthonormality)."""
    import scipy.sparse as sp
    n = len(A[0]) - 1
    As, Bs = sp.csr_matrix((A[2], A[1], A[0]), shape=(n, n)), sp.csr_matrix((B[2], B[1], B[0]), shape=(n, n))
    lam_ref, cond_b, a_inf, b_inf = ref
    lam_ref = lam_ref[:k]
    assert np.all(np.diff(lam) >= 0)
    bound = TOL * lam_ref * np.sqrt(cond_b)
    e_lam = np.max(np.abs(lam - lam_ref) / bound)
    BX = Bs @ X
    res = np.linalg.norm(As @ X - BX * lam, axis=0)
    res_bound = TOL * lam * np.linalg.norm(BX, axis=0) + 1e-12 * (a_inf + lam * b_inf) * np.linalg.norm(X, axis=0)
    e_res = np.max(res / res_bound)
    orth = np.max(np.abs(X.T @ BX - np.eye(k)))
    print(f"{name} k={k}: eigenvalue error / bound {e_lam:.3e}, residual / bound {e_res:.3e}, B-orthonormality {orth:.2e}")
    assert e_lam <= 1.0, (lam, lam_ref)
    assert e_res <= 1.0
    assert orth <= 1e-12
    if name.startswith("fem"):
        assert abs(lam[0] - 1.0) <= TOL * np.sqrt(cond_b)  # the constant vector: lambda_0 = 1
    return e_lam, e_res, orth
