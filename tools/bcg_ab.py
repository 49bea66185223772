"""Block CG against block PCG on the same block of right-hand sides: what the coupled search space buys in iterations and what an
iteration of it costs.

    python tools/bcg_ab.py [--problems fem,p216_csr] [--widths 2,4,8] [--tol 1e-8] [--reps 3] [--out FILE]

Per problem one handle and, per width W, in one process: a warm-up round, then `reps` alternations of solve_multi_dev("bcg") and
solve_multi_dev("pcg") on the same W right-hand sides (seeded normal vectors, the first W columns of one block for every W), HIP-event
times of the whole calls.  Block PCG's iteration count is that of its slowest column: the loop runs until every column is frozen.
Block CG counts as faster when its slowest repeat beats block PCG's fastest, i.e. by more than the spread of the runs.

fem is the unstructured FEM stand-in at 525 825 rows; p216_csr is 216^3 under set_kernel_config(kind=0), the CSR-stream path whose
arrays the block kernels read.  One JSON line per problem and width.
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
    if name.startswith("p") and name[1:].split("_")[0].isdigit():  # pN / pN_csr: a box grid
        return problems.poisson3d(int(name[1:].split("_")[0]))
    if name == "fem":
        return problems.fem_unstructured()
    if name.startswith("fem"):  # femN: a smaller stand-in (dry runs)
        return problems.fem_unstructured(int(name[3:]))
    raise ValueError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="fem,p216_csr")
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
        for W in widths:
            rec = {"problem": name, "rows": n, "nnz": nnz, "levels": A.nlevels, "W": W}
            ms = {"bcg": [], "pcg": []}
            its = {}
            for k in range(args.reps + 1):  # first round: warm-up
                for method in ("bcg", "pcg"):
                    A.dev_fill(xd, n * W, 0.0)
                    _, it, status, sec, rc = A.solve_multi_dev(method, W, bd, n, xd, n)
                    assert rc == 0 and np.all(status == 0), (method, rc, status)
                    if k > 0:
                        ms[method].append(sec * 1e3)
                        its[method] = int(it.max())
            for method in ("bcg", "pcg"):
                t = ms[method]
                rec[f"{method}_iterations"] = its[method]
                rec[f"{method}_ms"] = [round(x, 3) for x in t]
                rec[f"{method}_ms_per_iteration"] = round(float(np.median(t)) / its[method], 4)
                rec[f"{method}_spread_ms"] = round(max(t) - min(t), 3)
            rec["iteration_ratio"] = round(its["bcg"] / its["pcg"], 3)
            rec["cost_per_iteration_ratio"] = round(rec["bcg_ms_per_iteration"] / rec["pcg_ms_per_iteration"], 3)
            rec["speedup_median"] = round(float(np.median(ms["pcg"]) / np.median(ms["bcg"])), 3)
            rec["bcg_faster_beyond_spread"] = bool(max(ms["bcg"]) < min(ms["pcg"]))
            rec["pcg_faster_beyond_spread"] = bool(max(ms["pcg"]) < min(ms["bcg"]))
            rec["bcg_info"] = A.bcg_info()
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
        A.close()


if __name__ == "__main__":
    main()
