"""Operators whose coarse factorisation has to interchange rows, and a numpy restatement of the device's Gauss-Jordan inversion.

The grids of the suite are diagonally dominant: partial pivoting always takes the diagonal row there, so the row interchange, the
source-row redirection s = (i == p ? k : i), the tie rule and the final column un-permutation of the inversion kernels
(csrc/nd_kernels.hip, csrc/coarse_kernels.hip) never run.  These inputs make them run.  Everything here is plain numpy: the CPU
tests (test_host_setup.py) fix what the inputs do before test_gpu_coarse_pivoting.py compares the device against them.
"""
import numpy as np

CLIQUE_SIZES = (1, 2, 63, 64, 65, 79, 80, 81, 82, 128, 129, 257)  # the LDS limit (80 | 81), a wave (63, 64, 65), rows that are no
#                                                                   multiple of 8 per workgroup, a second trip of 256 columns (257)
HADAMARD_SIZES = (64, 128, 256)
LDS_LIMIT = 80  # csrc/nd_solver.hpp kNdTinyPivot


def gauss_jordan_inverse(M):
    """The documented algorithm of the device inverters in fp64, every product and difference rounded on its own:
    step k: p = argmax_{i >= k} |M[i][k]| (lowest index on ties), rows k and p interchanged, row k scaled by 1 / pivot with
    M[k][k] = 1 / pivot, every other row i: M[i][j] -= f_i M[k][j], M[i][k] = -f_i / pivot; at the end the columns are swapped back
    in reverse pivot order.  Returns (inverse, interchanges, singular)."""
    M = np.array(M, dtype=np.float64)
    n = M.shape[0]
    piv = np.zeros(n, dtype=np.int64)
    singular = False
    with np.errstate(all="ignore"):
        for k in range(n):
            p = k + int(np.argmax(np.abs(M[k:, k])))  # argmax returns the first maximum
            piv[k] = p
            if not abs(M[p, k]) > 0.0:
                singular = True
            if p != k:
                M[[k, p]] = M[[p, k]]
            rpiv = 1.0 / M[k, k]
            prow = M[k] * rpiv
            prow[k] = rpiv
            f = M[:, k].copy()
            M = M - f[:, None] * prow[None, :]
            M[:, k] = -f * rpiv
            M[k] = prow
    cm = np.arange(n)
    for k in range(n - 1, -1, -1):
        cm[k], cm[piv[k]] = cm[piv[k]], cm[k]
    return M[:, cm], int(np.count_nonzero(piv != np.arange(n))), singular


def block_diagonal_csr(blocks):
    """CSR (int32 rowptr, int32 colindex, fp64 values) of a block-diagonal matrix, every entry of every block stored."""
    rp, ci, v = [0], [], []
    r0 = 0
    for Bk in blocks:
        s = Bk.shape[0]
        for i in range(s):
            ci.append(np.arange(r0, r0 + s))
            v.append(Bk[i])
            rp.append(rp[-1] + s)
        r0 += s
    return np.asarray(rp, dtype=np.int32), np.concatenate(ci).astype(np.int32), np.concatenate(v).astype(np.float64)


def integer_vector(n, seed):
    """Nonzero integers in [-9, 9]: products with integer or power-of-two-scaled matrices are exact in fp64."""
    x = np.random.default_rng(seed).integers(-9, 10, n).astype(np.float64)
    x[x == 0.0] = 1.0
    return x


def clique_blocks(sizes=CLIQUE_SIZES, seed=11):
    """Dense blocks of random integers in [-9, 9] with zeros replaced by 1: most steps interchange, exact ties are frequent."""
    rng = np.random.default_rng(seed)
    out = []
    for s in sizes:
        Bk = rng.integers(-9, 10, (s, s)).astype(np.float64)
        Bk[Bk == 0.0] = 1.0
        out.append(Bk)
    return out


def hadamard_blocks(sizes=HADAMARD_SIZES, seed=5):
    """Sylvester Hadamard matrices with shuffled rows, A = H[perm].  Every intermediate of the pivoted Gauss-Jordan is a dyadic
    rational, so the inversion is exact in fp64 whatever the rounding of single operations.  Returns (blocks, perms)."""
    rng = np.random.default_rng(seed)
    blocks, perms = [], []
    for s in sizes:
        H = np.ones((1, 1))
        while H.shape[0] < s:
            H = np.block([[H, H], [H, -H]])
        perm = rng.permutation(s)
        blocks.append(H[perm])
        perms.append(perm)
    return blocks, perms


def hadamard_exact_inverse(block, perm):
    """A = H[perm]  =>  A^-1 = (H^T / n)[:, perm]   (H H^T = n I)."""
    n = block.shape[0]
    H = np.empty_like(block)
    H[perm] = block
    return (H.T / n)[:, perm]


def singular_clique(m):
    """All ones, 2 on the diagonal, row 1 a copy of row 0: step 0 takes row 0 on the tie and leaves row 1 exactly zero in every
    remaining column; a zero row stays zero, so the last step meets a pivot of exactly 0."""
    S = np.ones((m, m)) + np.eye(m)
    S[1] = S[0]
    return S


def scale_rows(rp, ci, v, seed=3, factor=8.0):
    """A seeded third of the rows multiplied by a power of two: S A x_true stays exact for integer x_true, and x_true unchanged."""
    n = len(rp) - 1
    s = np.where(np.random.default_rng(seed).random(n) < 1.0 / 3.0, factor, 1.0)
    return rp, ci, np.asarray(v, dtype=np.float64) * np.repeat(s, np.diff(rp))


def lu_row_swaps(A):
    """Row interchanges of a dense partial-pivot LU of the whole matrix (lowest index on ties)."""
    M = np.array(A, dtype=np.float64)
    n = M.shape[0]
    swaps = 0
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
            swaps += 1
        M[k + 1:, k] /= M[k, k]
        M[k + 1:, k + 1:] -= np.outer(M[k + 1:, k], M[k, k + 1:])
    return swaps
