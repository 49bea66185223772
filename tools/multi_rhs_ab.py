"""A block of W right-hand sides in one AMG-PCG run against what the handle offers otherwise for W systems: W single solves.

    python tools/multi_rhs_ab.py [--problems p216_csr,p216,fem] [--widths 2,4,8] [--tol 1e-8] [--reps 3] [--out FILE]

Per problem one handle and, per width W, in one process and alternating (after one warm-up round):
  * sparsh_solve_multi_dev of W right-hand sides against W sparsh_solve_dev("pcg") runs of the same right-hand sides, HIP-event
    times of the whole calls; the block counts as faster when its slowest repeat beats the fastest sum of the W single solves, i.e.
    by more than the spread of the single-solve runs of the same call;
  * one block Jacobi sweep on the finest level's resident block buffers (bench_op_multi 1) against one single-vector sweep
    (bench_op 10), as time per vector;
  * beside each measured ratio the byte model's: a sweep over W interleaved vectors streams 12 nnz + (12 + 24 W) n bytes (rowptr and
    the diagonal once, b, x and y once per column), so W single sweeps cost W (12 nnz + 36 n) / (12 nnz + (12 + 24 W) n) times the block's.

Right-hand sides: ones, then seeded normal vectors.  p216_csr is 216^3 under set_kernel_config(kind=0), the CSR-stream path whose
arrays the block kernels read; p216 the defaults (matrix-free box path); fem the unstructured FEM stand-in at 525 825 rows.
One JSON line per problem and width.
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
        return problems.poisson3d(216)
    if name.startswith("p") and name[1:].split("_")[0].isdigit():  # pN / pN_csr: a smaller box (dry runs)
        return problems.poisson3d(int(name[1:].split("_")[0]))
    if name == "fem":
        return problems.fem_unstructured()
    raise ValueError(name)


def model_ratio(n, nnz, W):
    return W * (12.0 * nnz + 36.0 * n) / (12.0 * nnz + (12.0 + 24.0 * W) * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="p216_csr,p216,fem")
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
        rng = np.random.default_rng(5)
        B = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(max(widths) - 1)])
        bd, xd = A.dev_alloc(8 * n * max(widths)), A.dev_alloc(8 * n * max(widths))
        A.h2d(bd, np.asfortranarray(B))  # column c at bd + 8 n c
        col = lambda p, c: type(p)(p.value + 8 * n * c)  # noqa: E731
        for W in widths:
            rec = {"problem": name, "rows": n, "nnz": nnz, "levels": A.nlevels, "level0_kernel": A.level_kernel(0), "W": W,
                   "byte_model_ratio": round(model_ratio(n, nnz, W), 3)}
            block, singles, its_b, its_s = [], [], None, None
            for k in range(args.reps + 1):  # first round: warm-up
                A.dev_fill(xd, n * W, 0.0)
                _, its, status, sec, rc = A.solve_multi_dev("pcg", W, bd, n, xd, n)
                assert rc == 0 and np.all(status == 0), (rc, status)
                total, counts = 0.0, []
                A.dev_fill(xd, n * W, 0.0)
                for c in range(W):
                    h, it, s, rc = A.solve_dev("pcg", col(bd, c), col(xd, c))
                    assert rc == 0, rc
                    total += s
                    counts.append(len(h))
                if k > 0:
                    block.append(sec)
                    singles.append(total)
                    its_b, its_s = [int(i) for i in its], counts
            rec["block_ms"] = [round(s * 1e3, 3) for s in block]
            rec["singles_ms"] = [round(s * 1e3, 3) for s in singles]
            rec["iterations_block"], rec["iterations_singles"] = its_b, its_s
            rec["speedup_median"] = round(float(np.median(singles) / np.median(block)), 3)
            rec["singles_spread_ms"] = round((max(singles) - min(singles)) * 1e3, 3)
            rec["block_faster_beyond_spread"] = bool(max(block) < min(singles))
            # one sweep on the finest level: the block's against a single vector's, alternating
            tb, ts = [], []
            for _ in range(5):
                tb.append(A.bench_op_multi(1, 0, nrhs=W, reps=30) * 1e6)
                ts.append(A.bench_op(10, 0, 30) * 1e6)
            rec["block_sweep_us"] = [round(t, 2) for t in tb]
            rec["single_sweep_us"] = [round(t, 2) for t in ts]
            rec["sweep_ratio_per_vector"] = round(float(W * np.median(ts) / np.median(tb)), 3)
            bts = 12.0 * nnz + (12.0 + 24.0 * W) * n
            rec["block_sweep_model_bytes"] = int(bts)
            rec["block_sweep_fraction_of_8TBps"] = round(bts / (float(np.median(tb)) * 1e-6) / HBM_BYTES_PER_S, 3)
            rec["multi_info"] = A.multi_info()
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
        A.close()


if __name__ == "__main__":
    main()
