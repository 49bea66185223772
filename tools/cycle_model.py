"""CPU model of the cycles of DESIGN.md section 5g: iteration counts of PCG / flexible CG under the V-, W- and K-cycle on the pairwise
aggregation hierarchy, in scipy.  Model counts, not device measurements.

    python tools/cycle_model.py [--grids 32,64] [--strides 3] [--seed 0]

Restated here: the heavy-edge matching of the host setup (rows walked forwards on even levels and backwards on odd ones; an
unmatched row joins its unmatched neighbour of the largest |a_ij|, the first one on ties; leftovers stay alone), the Galerkin
products P^T A P with the piecewise-constant P, weighted Jacobi legs (omega = 0.66667) and the cycles of the contract:
    cycle(l, b):        l last: direct solve.  else x = nu sweeps from 0 ; x += P solve_coarse(l + 1, P^T (b - A x)) ; nu sweeps
    solve_coarse(l, b): plain level: cycle(l, b).   W: c = cycle(l, b) ; d = cycle(l, b - A c) ; c + d.
                        K: two steps of flexible CG preconditioned by cycle(l, .), with the guards of the header.
The hierarchy coarsens while a level has more than 500 rows, to at most 10 levels.  System: 7-point Poisson, random right-hand
side, zero guess, stop at ||r|| <= 1e-8 ||b||.
"""
import argparse

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

OMEGA = 0.66667


def poisson3d(n):
    e = np.ones(n)
    t = sp.diags([-e[:-1], 2 * e, -e[:-1]], [-1, 0, 1])
    i = sp.identity(n)
    return (sp.kron(sp.kron(t, i), i) + sp.kron(sp.kron(i, t), i) + sp.kron(sp.kron(i, i), t)).tocsr()


def hem(A, level):
    n = A.shape[0]
    rp, ci, v = A.indptr, A.indices, np.abs(A.data)
    agg = -np.ones(n, dtype=np.int64)
    nxt = 0
    order = range(n) if level % 2 == 0 else range(n - 1, -1, -1)
    for i in order:
        if agg[i] != -1:
            continue
        mate, best = -1, 0.0
        for j in range(rp[i], rp[i + 1]):
            c = ci[j]
            if c != i and agg[c] == -1 and v[j] > best:
                best, mate = v[j], c
        if mate >= 0:
            agg[i] = agg[mate] = nxt
            nxt += 1
    for i in range(n):
        if agg[i] == -1:
            agg[i] = nxt
            nxt += 1
    return sp.csr_matrix((np.ones(n), agg, np.arange(n + 1)), shape=(n, nxt))


class Hierarchy:
    def __init__(self, A, max_levels=10, stop_rows=500):
        self.A, self.P = [A.tocsr()], []
        while len(self.A) < max_levels and self.A[-1].shape[0] > stop_rows:
            a = self.A[-1]
            a.sort_indices()
            p = hem(a, len(self.A) - 1)
            self.P.append(p)
            self.A.append((p.T @ a @ p).tocsr())
        self.D = [a.diagonal() for a in self.A]
        self.lu = spla.splu(self.A[-1].tocsc())
        self.last = len(self.A) - 1
        self.visits = 0

    def leg(self, l, b, x, nu):
        for _ in range(nu):
            x = OMEGA * b / self.D[l] if x is None else x + OMEGA * (b - self.A[l] @ x) / self.D[l]
        return np.zeros_like(b) if x is None else x

    def cycle(self, l, b, kind, stride, nu):
        self.visits += 1
        if l == self.last:
            return self.lu.solve(b)
        x = self.leg(l, b, None, nu)
        x = x + self.P[l] @ self.solve_coarse(l + 1, self.P[l].T @ (b - self.A[l] @ x), kind, stride, nu)
        return self.leg(l, b, x, nu)

    def solve_coarse(self, l, b, kind, stride, nu):
        if kind == "v" or not (1 <= l < self.last and l % stride == 0):
            return self.cycle(l, b, kind, stride, nu)
        c = self.cycle(l, b, kind, stride, nu)
        if kind == "w":
            return c + self.cycle(l, b - self.A[l] @ c, kind, stride, nu)
        v = self.A[l] @ c
        rho1, alpha1 = c @ v, c @ b
        ok1 = np.isfinite(rho1) and rho1 > 0
        q = alpha1 / rho1 if ok1 else 1.0
        r = b - q * v
        d = self.cycle(l, r, kind, stride, nu)
        if not ok1:
            return c + d
        w = self.A[l] @ d
        gamma, beta, alpha2 = d @ v, d @ w, d @ r
        rho2 = beta - gamma * gamma / rho1
        if not (np.isfinite(rho2) and rho2 > 0):
            return q * c
        return (q - gamma * alpha2 / (rho1 * rho2)) * c + (alpha2 / rho2) * d


def solve(H, b, kind, stride, nu, flexible, rtol=1e-8, cap=200):
    A = H.A[0]
    M = lambda r: H.cycle(0, r, kind, stride, nu)  # noqa: E731
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    p, rho = z.copy(), z @ r
    stop = rtol * np.linalg.norm(b)
    for k in range(1, cap + 1):
        q = A @ p
        sigma = p @ q
        alpha = rho / sigma
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= stop:
            return k
        z = M(r)
        rho_new = z @ r
        beta = -(z @ q) / sigma if flexible else rho_new / rho
        rho = rho_new
        p = z + beta * p
    return cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="32,64")
    ap.add_argument("--strides", default="3")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    for g in (int(t) for t in args.grids.split(",")):
        H = Hierarchy(poisson3d(g))
        b = np.random.default_rng(args.seed).standard_normal(g ** 3)
        row = {f"V({nu},{nu}) PCG": solve(H, b, "v", 1, nu, False) for nu in (7, 2, 1)}
        for s in (int(t) for t in args.strides.split(",")):
            for nu in (2, 1):
                row[f"K/{s} nu={nu} FCG"] = solve(H, b, "k", s, nu, True)
            row[f"W/{s} nu=2 PCG"] = solve(H, b, "w", s, 2, False)
            H.visits = 0
            H.cycle(0, b, "k", s, 2)
            row[f"K/{s} level visits"] = H.visits
        print(f"{g}^3 ({len(H.A)} levels, rows {[a.shape[0] for a in H.A]}):", row, flush=True)


if __name__ == "__main__":
    main()
