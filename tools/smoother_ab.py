"""Jacobi against multicolour SOR (symmetric, inside PCG): iterations to tol, ms per iteration and time to solution, plus the
SOR layout's byte model, per-sweep timings of both SOR launch paths per level and the launches of one cycle.

    python tools/smoother_ab.py [--problems p216,p216_noconst,p216_csr,fem,c0] [--tol 1e-8] [--reps 3] [--out FILE]
    python tools/smoother_ab.py --sweep-only [--problems p216] [--reps 200]   # level-0 SOR sweeps alone (run under rocprofv3)
    python tools/smoother_ab.py --chebyshev [--problems p216_noconst,p216_csr,fem,p216] [--reps 3] [--out FILE]

--chebyshev: Jacobi (the default sweep count) against the Chebyshev smoother of degree 4 and 6 inside PCG, the solves alternating
in one process after a warm-up; one Chebyshev step against one Jacobi sweep on the finest level's resident buffers (bench_op 17
against 10, alternating repeats) beside the byte model's expectation (+16 B per row: the correction vector read and written); and
the host time of the spectral-bound estimate beside the setup's.

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


def jacobi_sweep_bytes(A, level):
    """bytes one Jacobi sweep of the level streams under the kernel it launches (the layout models of csr_placement)"""
    li = A.level_info(level)
    n, nnz = li["nrow"], li["nnz"]
    k = A.level_kernel(level)
    if k == "sdia_tab_kernel":
        return 24 * n + 68 * ((n + 63) // 64)
    if k == "sdia_kernel":
        return 8 * nnz + 24 * n + 24 * ((n + 63) // 64) * 8
    if k == "sell_kernel":
        return 12 * nnz + 28 * n
    return (10 if k == "csr_rowlane16_kernel" else 12) * nnz + 36 * n


def chebyshev_ab(A, name, b, args):
    import time

    n = A.nrow
    rec = {"problem": name, "rows": n, "levels": A.nlevels, "level0_kernel": A.level_kernel(0), "setup_seconds": round(A.setup_seconds(), 3)}
    t0 = time.perf_counter()
    bounds = [A.level_chebyshev(l) for l in range(A.nlevels - 1)]
    rec["bounds_seconds"] = round(time.perf_counter() - t0, 3)
    rec["bounds"] = [{k: round(v, 5) for k, v in c.items()} for c in bounds]
    # one step against one sweep on the finest level, alternating
    A.set_smoother("chebyshev", 4)
    A.op_precond(np.zeros(n))  # d vectors
    t10, t17 = [], []
    for _ in range(5):
        t10.append(A.bench_op(10, 0, 50) * 1e6)
        t17.append(A.bench_op(17, 0, 50) * 1e6)
    jb = jacobi_sweep_bytes(A, 0)
    rec["level0_jacobi_sweep_us"] = [round(t, 2) for t in t10]
    rec["level0_chebyshev_step_us"] = [round(t, 2) for t in t17]
    rec["step_over_sweep_measured"] = round(float(np.median(t17) / np.median(t10)), 4)
    rec["step_over_sweep_byte_model"] = round((jb + 16 * n) / jb, 4)
    rec["jacobi_sweep_model_bytes"] = int(jb)
    print(rec, flush=True)
    bd, xd = A.dev_alloc(8 * n), A.dev_alloc(8 * n)
    A.h2d(bd, b)
    configs = [("jacobi", 0), ("chebyshev", 4), ("chebyshev", 6)]
    runs = {c: [] for c in configs}
    for k in range(args.reps + 1):  # first round: warm-up
        for c in configs:
            A.set_smoother(c[0], c[1])
            A.dev_fill(xd, n, 0.0)
            h, it, sec, rc = A.solve_dev("pcg", bd, xd)
            assert rc == 0, (c, rc)
            if k > 0:
                runs[c].append((len(h), sec))
    for c in configs:
        its = runs[c][0][0]
        secs = [s for _, s in runs[c]]
        rec[f"{c[0]}_{c[1]}"] = {"iterations": its, "time_to_solution_ms": [round(s * 1e3, 3) for s in secs],
                                 "best_ms": round(min(secs) * 1e3, 3), "ms_per_iteration": round(min(secs) * 1e3 / its, 4)}
        print(name, c, rec[f"{c[0]}_{c[1]}"], flush=True)
    A.set_smoother("jacobi")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="p216,p216_noconst,p216_csr,fem,c0")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep-only", action="store_true")
    ap.add_argument("--chebyshev", action="store_true")
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
        if args.chebyshev:
            rec = chebyshev_ab(A, name, b, args)
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
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
