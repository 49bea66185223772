"""V-cycle PCG against the W-cycle under PCG and the K-cycle under flexible CG: iterations, ms to tol and launches per iteration.

    python tools/cycle_ab.py [--problems p216,p216_noconst,fem] [--reps 2] [--tol 1e-8] [--out FILE]

Problems: p216 = 7-point Poisson on 216^3 in the box-grid default layout, p216_noconst = the same operator in the general-values
layout (constant-slot folding off: what a variable-coefficient operator gets), fem = the unstructured FEM stand-in.  Configurations:
PCG with V(7,7) (the default), V(2,2) and V(1,1); FCG with the K-cycle and PCG with the W-cycle at strides 2, 3 and 4 for
nu = 1, 2, 3 Jacobi sweeps per leg.  One handle per problem; the configurations alternate in one process, one warm-up round and then
--reps timed rounds; times are HIP-event times of whole solves on device vectors (sparsh_solve_dev), best of the rounds.

Launches per iteration are counted from the hierarchy, not measured: the recursive cycle issues, per visit of a smoothed level, nu
launches per leg, residual, restriction and prolongation; per coarse solve what the direct solver reports; per W step 2 and per K step
8 (two SpMVs and six of its own); the Krylov loop 5 (PCG) or 7 (FCG).  The V-cycle's Jacobi path fuses launches on top of that (double
and triple sweeps, residual + restriction, sweep + prolongation), so its figure is an upper bound.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sparsh_amg_amd as sa  # noqa: E402
from sparsh_amg_amd import problems  # noqa: E402


def load(name):
    if name.startswith("p216"):
        return problems.poisson3d(216)
    if name.startswith("p"):  # p48, p100 ...: smaller cubes for a quick look
        return problems.poisson3d(int(name[1:].split("_")[0]))
    if name == "fem":
        return problems.fem_unstructured()
    raise ValueError(name)


def launches_per_iteration(A, kind, stride, nu, method):
    L = A.nlevels
    ci = A.coarse_info()
    coarse = 1 if ci["dense"] else max(ci["nd_launches_per_solve"], 1)
    last = L - 1
    total, visits = 0, 1
    for l in range(L):
        wk = kind != "v" and 1 <= l < last and l % stride == 0
        if wk:
            total += visits * (2 if kind == "w" else 8)
            visits *= 2
        total += visits * (coarse if l == last else 2 * nu + 3)
    return total + (7 if method == "fcg" else 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="p216,p216_noconst,fem")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    configs = [("pcg", "v", 3, 7), ("pcg", "v", 3, 2), ("pcg", "v", 3, 1)]
    for nu in (1, 2, 3):
        for stride in (2, 3, 4):
            configs.append(("fcg", "k", stride, nu))
            configs.append(("pcg", "w", stride, nu))
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    for name in args.problems.split(","):
        rp, ci, v = load(name)
        n = len(rp) - 1
        A = sa.sp_matrix_mg(rp, ci, v)
        if name.endswith("_noconst"):
            A.set_const_slots(False)
        A.setup(sa.default_params(print_setup=0, print_solve=0, tol=args.tol))
        rows = [A.level_info(l)["nrow"] for l in range(A.nlevels)]
        emit(f"# {name}: {n} rows, {A.nlevels} levels {rows}, level 0 kernel {A.level_kernel(0)}, setup {A.setup_seconds:.1f} s")
        bd, xd = A.dev_alloc(8 * n), A.dev_alloc(8 * n)
        A.h2d(bd, np.ones(n))
        runs = {c: [] for c in configs}
        for k in range(args.reps + 1):  # first round: warm-up
            for c in configs:
                method, kind, stride, nu = c
                A.set_smoother("jacobi", nu)
                A.set_cycle(kind, stride)
                A.dev_fill(xd, n, 0.0)
                h, it, sec, rc = A.solve_dev(method, bd, xd)
                if k > 0:
                    runs[c].append((it, sec, rc, float(h[-1]) if len(h) else float("nan")))
        emit(f"{'problem':14s} {'method':6s} {'cycle':5s} {'stride':>6s} {'nu':>3s} {'iters':>6s} {'rc':>3s} {'best ms':>9s} {'ms/iter':>8s} {'launches/iter':>14s} {'visits':>7s}  all ms")
        for c in configs:
            method, kind, stride, nu = c
            A.set_cycle(kind, stride)
            visits = A.cycle_info()["level_visits"]
            it, _, rc, _ = runs[c][0]
            secs = [s for _, s, _, _ in runs[c]]
            best = min(secs) * 1e3
            lp = launches_per_iteration(A, kind, stride, nu, method)
            emit(f"{name:14s} {method:6s} {kind:5s} {stride if kind != 'v' else '-':>6} {nu:3d} {it:6d} {rc:3d} {best:9.2f} {best / max(it, 1):8.3f} {lp:14d} {visits:7d}  "
                 + " ".join(f"{s * 1e3:.2f}" for s in secs))
            rec = {"problem": name, "method": method, "cycle": kind, "stride": stride, "nu": nu, "iterations": it, "rc": rc, "best_ms": round(best, 3),
                   "launches_per_iteration": lp, "level_visits": visits}
            lines.append("JSON " + json.dumps(rec))
        A.set_cycle("v")
        A.set_smoother("jacobi")
        A.dev_free(bd)
        A.dev_free(xd)
        A.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
