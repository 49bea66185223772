"""Jacobi against multicolour SOR (symmetric, inside PCG): iterations to tol, ms per iteration and time to solution, plus the
SOR layout's byte model, per-sweep timings of both SOR launch paths per level and the launches of one cycle.

    python tools/smoother_ab.py [--problems p216,p216_noconst,p216_csr,fem,c0] [--tol 1e-8] [--reps 3] [--out FILE]
    python tools/smoother_ab.py --sweep-only [--problems p216] [--reps 200]   # level-0 SOR sweeps alone (run under rocprofv3)

One handle per problem; the smoother is switched on it between timed solves (sparsh_set_smoother; the SOR layouts are built at
the first SOR solve).  Times are HIP-event times of whole solves on device vectors (sparsh_solve_dev), best of --reps after
one warm-up solve.  One JSON line per problem.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sparsh_amg_amd as sa  # noqa: E402
from sparsh_amg_amd import problems  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def load(name):
    if name.startswith("p216"):
        return problems.poisson3d(216), np.ones(216 ** 3)
    if name == "fem":
        rp, ci, v = problems.fem_unstructured()
        return (rp, ci, v), np.ones(len(rp) - 1)
    if name == "c0":
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
        from conftest import load_c0

        rp, ci, v, b = load_c0()
        return (rp, ci, v), b
    raise ValueError(name)


def configure(A, name):
    if name == "p216_noconst":
        A.set_const_slots(False)  # read at setup: the layout of a variable-coefficient operator
    if name == "p216_csr":
        A.set_kernel_config(kind=0)


def sweep_bytes(A, level):
    """Bytes one SOR sweep of `level` moves under the per-colour launches, from the layout: per colour the compacted CSR
    (12 B per entry, rowptr + row id + diagonal 16 B per row), b (8 B per row), x_i written (8 B per row) and every distinct
    x entry the colour gathers read once (8 B)."""
    rp, ci, _, _ = A.level_csr(level)
    nc, _, color = A.level_colors(level)
    lens = np.diff(rp)
    row_of = np.repeat(color, lens)
    total = 0
    for c in range(1, nc + 1):
        rows_c = int(np.sum(color == c))
        cols = ci[row_of == c]
        total += 12 * len(cols) + 16 * rows_c + 4 + 8 * rows_c + 8 * rows_c + 8 * len(np.unique(cols))
    return total


def timed_solve(A, bd, xd, n, reps):
    best, hist = None, None
    for k in range(reps + 1):  # first: warm-up
        A.dev_fill(xd, n, 0.0)
        h, it, sec, rc = A.solve_dev("pcg", bd, xd)
        assert rc == 0, rc
        if k > 0 and (best is None or sec < best):
            best, hist = sec, h
    return best, len(hist)


def cycle_launches(A, single):
    """launches of one SOR V-cycle from a zero guess (PCG preconditioner), the coarsest solve counted as one"""
    L = A.nlevels
    total = 1  # coarsest solve
    smooth = 0
    for l in range(L - 1):
        info = A.level_sor_layout(l)
        per_leg = 1 if (single and info["single_launch"]) else info["ncolors"] * 6
        smooth += 2 * per_leg
        total += 1 + 1 + 1 + 1  # zero fill, residual, restriction, prolongation
    return total + smooth + 1, smooth  # + the dot product of z.r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="p216,p216_noconst,p216_csr,fem,c0")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep-only", action="store_true")
    ap.add_argument("--levels-max-nnz", type=int, default=4_000_000, help="time the single-launch path on levels up to this nnz")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for name in args.problems.split(","):
        (rp, ci, v), b = load(name)
        n = len(rp) - 1
        A = sa.sp_matrix_mg(rp, ci, v)
        configure(A, name)
        A.setup(sa.default_params(print_setup=0, print_solve=0, tol=args.tol))
        if args.sweep_only:
            A.set_smoother("sor", 0, "symmetric")
            A.op_sor(0, np.zeros(n), np.zeros(n), 1)  # builds the layouts
            sec = A.bench_op("sor", 0, args.reps)
            print(json.dumps({"problem": name, "level0_sor_sweep_us": round(sec * 1e6, 2)}), flush=True)
            A.close()
            continue
        bd, xd = A.dev_alloc(8 * n), A.dev_alloc(8 * n)
        A.h2d(bd, b)
        rec = {"problem": name, "rows": n, "nnz": int(rp[-1]), "levels": A.nlevels, "level0_kernel": A.level_kernel(0)}
        for sm in ("jacobi", "sor"):
            A.set_smoother(sm, 0, "symmetric")
            sec, it = timed_solve(A, bd, xd, n, args.reps)
            rec[sm] = {"iterations": it, "ms_per_iteration": round(sec * 1e3 / it, 4), "time_to_solution_ms": round(sec * 1e3, 3)}
            print(name, sm, rec[sm], flush=True)
        rec["sor_over_jacobi_time"] = round(rec["sor"]["time_to_solution_ms"] / rec["jacobi"]["time_to_solution_ms"], 3)
        # per level: colours, layout bytes, one sweep under each launch path (bench_op "sor" = one sweep as a leg issues it; on the
        # coarsest level, which the cycle solves directly, it builds that level's layout for the measurement alone)
        lev = []
        for l in range(A.nlevels):
            li = A.level_info(l)
            row = {"level": l, "rows": li["nrow"], "nnz": li["nnz"], "smoothed": l + 1 < A.nlevels}
            A.set_sor_path(1)
            row["per_colour_us"] = round(A.bench_op("sor", l, 20) * 1e6, 2)
            if li["nnz"] <= args.levels_max_nnz:
                A.set_sor_path(2)
                row["single_launch_us"] = round(A.bench_op("sor", l, 20) * 1e6, 2)
            A.set_sor_path(0)
            info = A.level_sor_layout(l)
            row.update(ncolors=info["ncolors"], layout_bytes=info["bytes"], single_by_policy=info["single_launch"])
            lev.append(row)
            print(row, flush=True)
        rec["levels_sor"] = lev
        rec["sor_layout_bytes"] = int(sum(r["layout_bytes"] for r in lev if r["smoothed"]))  # what a solve holds
        bts = sweep_bytes(A, 0)
        us = lev[0]["per_colour_us"]
        rec["level0_sweep_model_bytes"] = int(bts)
        rec["level0_sweep_event_us"] = us
        rec["level0_sweep_fraction_of_8TBps"] = round(bts / (us * 1e-6) / HBM_BYTES_PER_S, 3)
        rec["launches_per_cycle"] = {"with_single_launch": cycle_launches(A, True), "per_colour_only": cycle_launches(A, False)}
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        A.close()


if __name__ == "__main__":
    main()
