"""The LOBPCG eigensolver on the large inputs: iterations, ms per iteration, the eigensolver's own launches
beside the block path's, and the rate of the new kernels against the copy rate DESIGN.md uses.

    python tools/eig_ab.py [--out profiles/eig_lobpcg.txt] [--reps 20] [--step-seconds 420]

Cases: poisson3d(216) with k = 4 and k = 8 under set_kernel_config(kind=0), fem_unstructured() with k = 4.  Every case runs in a
process of its own under `timeout`; the first case that fails stops the rest.  Per case one JSON line:
  iterations, ms_per_iteration                   one timed eigs_dev call (HIP-event time) after a warm-up call
  gram_us, update_us                             sparsh_bench_op_multi ops 2 and 3 on the solver's resident blocks
  spmv_dot_us, jacobi_us                         ops 0 and 1 on level 0 of the block path, for scale
  gram_TBps, update_TBps, *_of_copy_rate         24 and 10 block passes of 8 n W bytes over the measured time, against 6.29 TB/s
  eig_kernels_share                              (gram + update + residual estimate) / ms_per_iteration, the residual taken as 3 / 10
                                                 of the update (3 block passes against 10)
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

COPY_BYTES_PER_S = 6.29e12  # the device-to-device copy rate DESIGN.md measures kernels against
CASES = ["p216:4", "p216:8", "fem:4"]


def run_case(case, reps):
    import sparsh_amg_amd as sa
    from sparsh_amg_amd import problems

    name, k = case.split(":")
    k = int(k)
    rp, ci, v = problems.poisson3d(216) if name == "p216" else problems.fem_unstructured()
    n = len(rp) - 1
    A = sa.sp_matrix_mg(rp, ci, v)
    if name == "p216":
        A.set_kernel_config(kind=0)
    A.setup(sa.default_params(print_setup=0, print_solve=0))
    W = 2 if k <= 2 else (4 if k <= 4 else 8)
    X0 = np.ascontiguousarray(np.random.default_rng(0).standard_normal((n, k)).T)  # (k, n) row-major = column-major (n, k)
    xd = A.dev_alloc(8 * n * k)
    rec = {"case": case, "rows": n, "nnz": int(rp[-1]), "k": k, "width": W, "levels": A.nlevels}
    for _ in range(2):  # the first call reserves the blocks
        A.h2d(xd, X0)
        lam, iters, hist, status, sec, rc = A.eigs_dev(k, xd, n, max_iters=300)
    its = hist.shape[1] - 1
    rec.update(rc=int(rc), iterations=its, seconds=round(sec, 4), ms_per_iteration=round(sec * 1e3 / max(its, 1), 4),
               lam=[float(x) for x in lam], restarts=A.eig_info()["restarts"], eig_bytes=A.eig_info()["bytes"])
    t = {op: A.bench_op_multi(op, 0, nrhs=k, reps=reps) for op in ("eig_gram", "eig_update", "spmv_dot", "jacobi_pingpong_resident")}
    block = 8.0 * n * W
    rec.update(gram_us=round(t["eig_gram"] * 1e6, 2), update_us=round(t["eig_update"] * 1e6, 2),
               spmv_dot_us=round(t["spmv_dot"] * 1e6, 2), jacobi_us=round(t["jacobi_pingpong_resident"] * 1e6, 2))
    rec["gram_TBps"] = round(24 * block / t["eig_gram"] / 1e12, 3)
    rec["update_TBps"] = round(10 * block / t["eig_update"] / 1e12, 3)
    rec["gram_of_copy_rate"] = round(24 * block / t["eig_gram"] / COPY_BYTES_PER_S, 3)
    rec["update_of_copy_rate"] = round(10 * block / t["eig_update"] / COPY_BYTES_PER_S, 3)
    rec["eig_kernels_share"] = round((t["eig_gram"] + 1.3 * t["eig_update"]) / (sec / max(its, 1)), 3)
    A.dev_free(xd)
    A.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="run one case in this process (used by the driver)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-seconds", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eig_lobpcg.txt"))
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.reps)
        return 0
    lines = []
    for case in CASES:  # the driver itself never opens the GPU
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print(f"{case}: exit status {p.returncode}; the remaining cases are not run", flush=True)
            return p.returncode
        lines += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    with open(args.out, "w") as f:
        f.write("# tools/eig_ab.py: LOBPCG on the block path, one JSON line per case (see the tool's docstring for the fields)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
