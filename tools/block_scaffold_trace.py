#!/usr/bin/env python3
"""The stream work of the block path, for comparing two builds launch by launch (profiles/block_scaffold_trace.txt).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/block_scaffold_trace.py
    python tools/block_scaffold_trace.py names DIR/.../*_kernel_trace.csv > names.txt

Without arguments: one width-4 solve each of "pcg", "bcg" (7-point Laplacian on 12^3) and "mbicg" (upwind convection-diffusion on
12^3), then one eigs(4) on the Laplacian, under the coarsening limits of tests/test_gpu_block_exits.py (several levels at 1 728 rows)
and seeded inputs.  `names`: the kernel names of such a trace in dispatch order, one per line; two builds issue the same stream work
when `diff` of their lists is empty."""
import csv
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run():
    import numpy as np

    import sparsh_amg_amd as sa
    from sparsh_amg_amd import problems

    prm = dict(print_setup=0, print_solve=0, limit_upper=300, limit_lower=100)
    for op, methods in ((problems.poisson3d(12), ("pcg", "bcg")), (problems.convection_diffusion(12, 12, 12), ("mbicg",))):
        A = sa.sp_matrix_mg(*op).setup(sa.default_params(**prm))
        B = np.random.default_rng(31).standard_normal((A.nrow, 4))
        for m in methods:
            _, iters, _, rc = A.solve_multi(m, B, np.zeros_like(B))
            print(m, "iterations", list(iters), "rc", rc)
        if "pcg" in methods:
            lam, _, iters, _, _ = A.eigs(4)
            print("eigs", list(lam), "iterations", list(iters), "rc", A.last_eigs_rc)
        A.close()


def names(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]) if r.get("Dispatch_Id") else int(r["Start_Timestamp"]))
    for r in rows:
        print(r["Kernel_Name"])


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "names":
        names(sys.argv[2])
    else:
        run()
