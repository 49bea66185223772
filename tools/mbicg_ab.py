"""Block BiCGStab against as many single "pbicg" solves on the same right-hand sides: what reading the hierarchy once for all columns
buys on an unsymmetric system.

    python tools/mbicg_ab.py [--problems cd216_csr,fem,cd216] [--widths 2,4,8] [--tol 1e-8] [--reps 3] [--out FILE]

Per problem one handle and, per width W, in one process: a warm-up round, then `reps` alternations of solve_multi_dev("mbicg") on W
right-hand sides and W solve_dev("pbicg") calls on the same columns one after the other (seeded normal vectors, the first W columns of
one block for every W), HIP-event times of the whole calls; the singles' time is the sum of their W calls.  The block's iteration
count is that of its slowest column: the loop runs until every column is frozen.  One side counts as faster when its slowest repeat
beats the other's fastest, i.e. by more than the spread of the runs.  A solve that does not end SPARSH_OK ends its width: the record
then holds "failed" (which side, the return code, the per-column status and counts) and no times.

cdN is the upwind convection-diffusion operator on an N^3 grid, cdN_csr the same under set_kernel_config(kind=0), the CSR-stream
path whose arrays the block kernels read (without it the single solves take whatever path the handle picks for a constant-coefficient
box grid); fem is the unstructured FEM stand-in at 525 825 rows.  One JSON line per problem and width.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sparsh_amg_amd as sa  # noqa: E402
from sparsh_amg_amd import problems  # noqa: E402


def load(name):
    if name.startswith("cd") and name[2:].split("_")[0].isdigit():  # cdN / cdN_csr
        m = int(name[2:].split("_")[0])
        return problems.convection_diffusion(m, m, m)
    if name == "fem":
        return problems.fem_unstructured()
    if name.startswith("fem"):  # femN: a smaller stand-in (dry runs)
        return problems.fem_unstructured(int(name[3:]))
    raise ValueError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="cd216_csr,fem,cd216")
    ap.add_argument("--widths", default="2,4,8")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    widths = [int(w) for w in args.widths.split(",")]
    for name in args.problems.split(","):
        rp, ci, v = load(name)
        n, nnz = len(rp) - 1, int(rp[-1])
        A = sa.sp_matrix_mg(rp, ci, v)
        if name.endswith("_csr"):
            A.set_kernel_config(kind=0)
        A.setup(sa.default_params(print_setup=0, print_solve=0, tol=args.tol))
        B = np.random.default_rng(5).standard_normal((n, max(widths)))
        bd, xd = A.dev_alloc(8 * n * max(widths)), A.dev_alloc(8 * n * max(widths))
        A.h2d(bd, np.ascontiguousarray(B.T))  # row c of B.T is column c of B: column c at bd + 8 n c
        col = lambda p, c: C.c_void_p(p.value + 8 * n * c)  # noqa: E731
        for W in widths:
            rec = {"problem": name, "rows": n, "nnz": nnz, "levels": A.nlevels, "W": W}
            ms = {"mbicg": [], "singles": []}
            its = {}
            failed = None  # a solve that does not end SPARSH_OK ends the width: its record says which and how
            for k in range(args.reps + 1):  # first round: warm-up
                A.dev_fill(xd, n * W, 0.0)
                _, it, status, sec, rc = A.solve_multi_dev("mbicg", W, bd, n, xd, n)
                if rc != 0:
                    failed = {"side": "mbicg", "rc": int(rc), "status": [int(v) for v in status], "iterations": [int(i) for i in it]}
                    break
                if k > 0:
                    ms["mbicg"].append(sec * 1e3)
                    its["mbicg"] = [int(i) for i in it]
                A.dev_fill(xd, n * W, 0.0)
                total, counts = 0.0, []
                for c in range(W):
                    try:
                        _, cnt, sec, rc = A.solve_dev("pbicg", col(bd, c), col(xd, c))
                    except sa.SparshError as e:  # (a NaN residual raises)
                        cnt, sec, rc = -1, 0.0, e.code
                    if rc != 0:
                        failed = {"side": "singles", "column": c, "rc": int(rc), "iterations": int(cnt)}
                        break
                    total += sec
                    counts.append(cnt)
                if failed:
                    break
                if k > 0:
                    ms["singles"].append(total * 1e3)
                    its["singles"] = counts
            if failed:
                rec["failed"] = failed
                print(json.dumps(rec), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(rec) + "\n")
                continue
            for side in ("mbicg", "singles"):
                t = ms[side]
                rec[f"{side}_iterations"] = its[side]
                rec[f"{side}_ms"] = [round(x, 3) for x in t]
                rec[f"{side}_spread_ms"] = round(max(t) - min(t), 3)
            rec["mbicg_ms_per_iteration"] = round(float(np.median(ms["mbicg"])) / max(its["mbicg"]), 4)
            rec["singles_ms_per_iteration"] = round(float(np.median(ms["singles"])) / sum(its["singles"]), 4)
            rec["speedup_median"] = round(float(np.median(ms["singles"]) / np.median(ms["mbicg"])), 3)
            rec["mbicg_faster_beyond_spread"] = bool(max(ms["mbicg"]) < min(ms["singles"]))
            rec["singles_faster_beyond_spread"] = bool(max(ms["singles"]) < min(ms["mbicg"]))
            rec["mbicg_info"] = A.mbicg_info()
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
        A.close()


if __name__ == "__main__":
    main()
