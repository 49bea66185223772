"""The LOBPCG eigensolver on the large inputs: iterations, ms per iteration, the eigensolver's own launches
beside the block path's, and the rate of the new kernels against the copy rate DESIGN.md uses.

    python tools/eig_ab.py [--out profiles/eig_lobpcg.txt] [--reps 20] [--step-seconds 420] [--max-iters 300]
    python tools/eig_ab.py --generalised [--out profiles/eig_gen_lobpcg.txt]
    python tools/eig_ab.py --constrained [--out profiles/eig_con_lobpcg.txt]
    python tools/eig_ab.py --ortho [--guard 4] [--out profiles/eig_ortho_lobpcg.txt]

Cases: poisson3d(216) with k = 4 and k = 8 under set_kernel_config(kind=0), fem_unstructured() with k = 4.  Every case runs in a
process of its own under `timeout`; the first case that fails stops the rest.  Per case one JSON line:
  iterations, ms_per_iteration                   one timed eigs_dev call (HIP-event time) after a warm-up call
  final_rn_over_bound                            per column, the last residual norm over tol |lambda| ||B x|| (B = I in the standard
                                                 problem): at most 1 when the column has converged
  gram_us, update_us                             sparsh_bench_op_multi ops 2 and 3 on the solver's resident blocks
  spmv_dot_us, jacobi_us                         ops 0 and 1 on level 0 of the block path, for scale
  gram_TBps, update_TBps, *_of_copy_rate         24 and 10 block passes of 8 n W bytes over the measured time, against 6.29 TB/s
  eig_kernels_share                              (gram + update + residual estimate) / ms_per_iteration, the residual taken as 3 / 10
                                                 of the update (3 block passes against 10)
--generalised: the pencil fem_pencil() = (M + dt K, M) at full size with k = 4 and 8 through eigs_gen_dev (cases femgen:k), next to the
standard solve of the same operator (cases fem:k, which end at the cap: DESIGN.md section 5i).  The femgen lines add
  update_gen_us, b_spmv_us                       sparsh_bench_op_multi ops 4 and 5 on the solver's resident blocks
  update_gen_TBps, update_gen_of_copy_rate       15 block passes (9 in, 6 out) over the measured time
and their eig_kernels_share counts the Gram launch, the generalised update and the residual as 4 / 15 of that update.
--constrained: eigs_con_dev (constraints).  Case femcon:8: the full-size FEM pencil, eigs_gen_dev(8) and then
eigs_con_dev(8) with its eight vectors as constraints (pairs 9..16).  Case neu216:8: poisson3d_neumann(216) set up with the constant
null space, eigs_con_dev(8) with the implicit constant vector alone.  Per case:
  first_iterations, first_rc                     femcon only: the unconstrained first solve
  iterations, ms_per_iteration, rc               the constrained solve (the second of two calls)
  mt, mpad, con_bytes                            constraints in all, rounded up to the width, the bytes sparsh_eig_con_info counts
  project_us                                     sparsh_bench_op_multi op 7: one projection (Gram launch, its finalise, apply kernel) on the resident blocks
  project_model_us, project_over_model           the byte model: the Gram launch reads n (mpad + W) 8 B, the apply reads the same and
                                                 writes n W 8 B, at 6.29 TB/s; gen reads Y and BY, the model counts mpad once per launch
  project_share                                  project_us over one iteration of the constrained solve
--ortho [--guard G]: the orthonormalised basis and the guard vectors (set_eig).  Cases femgen:4, femgen:8 (the
full-size pencil), fem:4, fem:8 (the standard problem on the same operator), femgen:4+G (k = 4 with G guard vectors, wanted = 4) and
neu216:8 (the constrained solve on the Neumann box).  Every case solves twice on one handle, under the plain and under the ortho
basis, and prints for each
  rc, iterations, restarts, ms_per_iteration     one timed _dev call after a warm-up call
  worst_rn_over_bound                            over the wanted columns, the last residual norm over tol |lambda| ||B x||
  dropped_w, dropped_p, ortho_bytes              sparsh_eig_ortho_info after the ortho solve
and, where a B is set, the two new launches against their byte model at 6.29 TB/s:
  transform_us, transform_model_us               sparsh_bench_op_multi op 8: three blocks read and written in place, 6 block passes
  ortho_apply_us, ortho_apply_model_us           op 9: X and W read, W written, 3 block passes
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
CASES_GENERALISED = ["fem:4", "femgen:4", "fem:8", "femgen:8"]
CASES_CONSTRAINED = ["femcon:8", "neu216:8"]
CASES_ORTHO = ["femgen:4", "femgen:8", "fem:4", "fem:8", "femgen:4+{guard}", "neu216:8"]


def run_case_ortho(case, reps, max_iters):
    import scipy.sparse as sp

    import sparsh_amg_amd as sa
    from sparsh_amg_amd import problems

    name, ks = case.split(":")
    k, guard = (int(x) for x in ks.split("+")) if "+" in ks else (int(ks), 0)
    kk = k + guard
    gen, con = name == "femgen", name == "neu216"
    M = None
    if con:
        rp, ci, v = problems.poisson3d_neumann(216)
    else:
        (rp, ci, v), M = problems.fem_pencil()
    n = len(rp) - 1
    A = sa.sp_matrix_mg(rp, ci, v)
    if con:
        A.set_nullspace("constant")
    A.setup(sa.default_params(print_setup=0, print_solve=0))
    if gen:
        A.set_eig_b(*M)
    W = 2 if kk <= 2 else (4 if kk <= 4 else 8)
    X0 = np.ascontiguousarray(np.random.default_rng(0).standard_normal((n, kk)).T)
    xd = A.dev_alloc(8 * n * kk)
    rec = {"case": case, "rows": n, "k": k, "guard": guard, "width": W, "levels": A.nlevels}
    Bs = sp.csr_matrix((M[2], M[1], M[0]), shape=(n, n)) if gen else None
    for basis in ("plain", "ortho"):
        A.set_eig(basis, wanted=k if guard else 0)
        for _ in range(2):  # the first call reserves the blocks
            A.h2d(xd, X0)
            if con:
                lam, iters, hist, status, sec, rc = A.eigs_con_dev(kk, xd, n, max_iters=max_iters, hist_cap=max_iters + 1)
            else:
                lam, iters, hist, status, sec, rc = (A.eigs_gen_dev if gen else A.eigs_dev)(kk, xd, n, max_iters=max_iters, hist_cap=max_iters + 1)
        its = hist.shape[1] - 1
        X = np.zeros((kk, n))
        A.d2h(X, xd)
        bn = np.linalg.norm(Bs @ X.T, axis=0) if gen else np.linalg.norm(X, axis=1)
        over = hist[:, -1] / (1e-8 * np.abs(lam) * bn)
        r = dict(rc=int(rc), iterations=its, restarts=A.eig_info()["restarts"], ms_per_iteration=round(sec * 1e3 / max(its, 1), 4),
                 worst_rn_over_bound=float(np.max(over[:k])), lam=[float(x) for x in lam[:k]], active=[int(x != 0) for x in status])
        if basis == "ortho":
            r.update(A.eig_ortho_info())
            r["ortho_bytes"] = r.pop("bytes")
            if gen:
                block = 8.0 * n * W
                t8, t9 = (A.bench_op_multi(op, 0, nrhs=kk, reps=reps) for op in ("eig_transform", "eig_ortho_apply"))
                r.update(transform_us=round(t8 * 1e6, 2), transform_model_us=round(6 * block / COPY_BYTES_PER_S * 1e6, 2),
                         ortho_apply_us=round(t9 * 1e6, 2), ortho_apply_model_us=round(3 * block / COPY_BYTES_PER_S * 1e6, 2))
        rec[basis] = r
    A.set_eig("plain", wanted=0)
    A.dev_free(xd)
    A.close()
    print(json.dumps(rec), flush=True)


def run_case_constrained(case, reps, max_iters):
    import sparsh_amg_amd as sa
    from sparsh_amg_amd import problems

    name, k = case.split(":")
    k = int(k)
    gen = name == "femcon"
    if gen:
        (rp, ci, v), M = problems.fem_pencil()
    else:
        rp, ci, v = problems.poisson3d_neumann(216)
    n = len(rp) - 1
    A = sa.sp_matrix_mg(rp, ci, v)
    if not gen:
        A.set_nullspace("constant")
    A.setup(sa.default_params(print_setup=0, print_solve=0))
    if gen:
        A.set_eig_b(*M)
    W = 2 if k <= 2 else (4 if k <= 4 else 8)
    X0 = np.ascontiguousarray(np.random.default_rng(0).standard_normal((n, k)).T)  # (k, n) row-major = column-major (n, k)
    xd, yd = A.dev_alloc(8 * n * k), A.dev_alloc(8 * n * k)
    rec = {"case": case, "rows": n, "nnz": int(rp[-1]), "k": k, "width": W, "levels": A.nlevels}
    ncon = 0
    if gen:  # the first block of pairs, left on the device as the constraints of the second
        A.h2d(yd, X0)
        lam1, _, hist1, _, sec1, rc1 = A.eigs_gen_dev(k, yd, n, max_iters=max_iters, hist_cap=max_iters + 1)
        rec.update(first_rc=int(rc1), first_iterations=hist1.shape[1] - 1, first_seconds=round(sec1, 4), first_lam=[float(x) for x in lam1])
        ncon = k
    for _ in range(2):  # the first call reserves the blocks
        A.h2d(xd, X0)
        lam, iters, hist, status, sec, rc = A.eigs_con_dev(k, xd, n, ncon=ncon, Y_dev=yd if ncon else None, ldy=n, gen=gen,
                                                          max_iters=max_iters, hist_cap=max_iters + 1)
    its = hist.shape[1] - 1
    info = A.eig_con_info()
    mt = info["ncon_total"]
    mpad = -(-mt // W) * W
    rec.update(rc=int(rc), iterations=its, seconds=round(sec, 4), ms_per_iteration=round(sec * 1e3 / max(its, 1), 4),
               lam=[float(x) for x in lam], restarts=A.eig_info()["restarts"], mt=mt, mpad=mpad, implicit_constant=info["implicit_constant"],
               con_bytes=info["bytes"], eig_bytes=A.eig_info()["bytes"])
    t = A.bench_op_multi("eig_con_project", 0, nrhs=k, reps=reps)
    model = (2 * 8.0 * n * (mpad + W) + 8.0 * n * W) / COPY_BYTES_PER_S
    rec.update(project_us=round(t * 1e6, 2), project_model_us=round(model * 1e6, 2), project_over_model=round(t / model, 3),
               project_share=round(t / (sec / max(its, 1)), 4))
    A.dev_free(xd)
    A.dev_free(yd)
    A.close()
    print(json.dumps(rec), flush=True)


def run_case(case, reps, max_iters):
    import scipy.sparse as sp

    import sparsh_amg_amd as sa
    from sparsh_amg_amd import problems

    name, k = case.split(":")
    k = int(k)
    gen = name == "femgen"
    if gen:
        (rp, ci, v), M = problems.fem_pencil()
    else:
        rp, ci, v = problems.poisson3d(216) if name == "p216" else problems.fem_unstructured()
    n = len(rp) - 1
    A = sa.sp_matrix_mg(rp, ci, v)
    if name == "p216":
        A.set_kernel_config(kind=0)
    A.setup(sa.default_params(print_setup=0, print_solve=0))
    if gen:
        A.set_eig_b(*M)
    W = 2 if k <= 2 else (4 if k <= 4 else 8)
    X0 = np.ascontiguousarray(np.random.default_rng(0).standard_normal((n, k)).T)  # (k, n) row-major = column-major (n, k)
    xd = A.dev_alloc(8 * n * k)
    rec = {"case": case, "rows": n, "nnz": int(rp[-1]), "k": k, "width": W, "levels": A.nlevels}
    for _ in range(2):  # the first call reserves the blocks
        A.h2d(xd, X0)
        lam, iters, hist, status, sec, rc = (A.eigs_gen_dev if gen else A.eigs_dev)(k, xd, n, max_iters=max_iters, hist_cap=max_iters + 1)
    its = hist.shape[1] - 1
    rec.update(rc=int(rc), iterations=its, seconds=round(sec, 4), ms_per_iteration=round(sec * 1e3 / max(its, 1), 4),
               lam=[float(x) for x in lam], restarts=A.eig_info()["restarts"], eig_bytes=A.eig_info()["bytes"])
    # how far the last evaluation is from the stopping rule: rn_c / (tol |lam_c| ||B x_c||), B = I in the standard problem
    X = np.zeros((k, n))
    A.d2h(X, xd)
    bn = np.linalg.norm(sp.csr_matrix((M[2], M[1], M[0]), shape=(n, n)) @ X.T, axis=0) if gen else np.linalg.norm(X, axis=1)
    rec["final_rn_over_bound"] = [float(x) for x in hist[:, -1] / (1e-8 * np.abs(lam) * bn)]
    t = {op: A.bench_op_multi(op, 0, nrhs=k, reps=reps) for op in ("eig_gram", "eig_update", "spmv_dot", "jacobi_pingpong_resident")}
    block = 8.0 * n * W
    rec.update(gram_us=round(t["eig_gram"] * 1e6, 2), update_us=round(t["eig_update"] * 1e6, 2),
               spmv_dot_us=round(t["spmv_dot"] * 1e6, 2), jacobi_us=round(t["jacobi_pingpong_resident"] * 1e6, 2))
    rec["gram_TBps"] = round(24 * block / t["eig_gram"] / 1e12, 3)
    rec["update_TBps"] = round(10 * block / t["eig_update"] / 1e12, 3)
    rec["gram_of_copy_rate"] = round(24 * block / t["eig_gram"] / COPY_BYTES_PER_S, 3)
    rec["update_of_copy_rate"] = round(10 * block / t["eig_update"] / COPY_BYTES_PER_S, 3)
    rec["eig_kernels_share"] = round((t["eig_gram"] + 1.3 * t["eig_update"]) / (sec / max(its, 1)), 3)
    if gen:
        tg = {op: A.bench_op_multi(op, 0, nrhs=k, reps=reps) for op in ("eig_update_gen", "eig_b_spmv")}
        rec.update(update_gen_us=round(tg["eig_update_gen"] * 1e6, 2), b_spmv_us=round(tg["eig_b_spmv"] * 1e6, 2),
                   b_nnz=A.eig_b_info()["nnz"], b_bytes=A.eig_b_info()["bytes"])
        rec["update_gen_TBps"] = round(15 * block / tg["eig_update_gen"] / 1e12, 3)
        rec["update_gen_of_copy_rate"] = round(15 * block / tg["eig_update_gen"] / COPY_BYTES_PER_S, 3)
        rec["eig_kernels_share"] = round((t["eig_gram"] + (1.0 + 4.0 / 15.0) * tg["eig_update_gen"]) / (sec / max(its, 1)), 3)
    A.dev_free(xd)
    A.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="run one case in this process (used by the driver)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-seconds", type=int, default=420)
    ap.add_argument("--max-iters", type=int, default=300, help="the iteration cap of every solve")
    ap.add_argument("--generalised", action="store_true", help="the FEM pencil against its mass matrix, next to the standard solve")
    ap.add_argument("--constrained", action="store_true", help="eigs_con_dev: deflation on the FEM pencil, the singular Neumann box")
    ap.add_argument("--ortho", action="store_true", help="plain against ortho basis (set_eig) on the FEM pencil, the standard problem and the Neumann box")
    ap.add_argument("--guard", type=int, default=4, help="--ortho: the guard vectors of the k = 4 case with guards")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "eig_ortho_lobpcg.txt" if args.ortho else ("eig_con_lobpcg.txt" if args.constrained else
                                ("eig_gen_lobpcg.txt" if args.generalised else "eig_lobpcg.txt")))
    if args.case:
        (run_case_ortho if args.ortho else (run_case_constrained if args.constrained else run_case))(args.case, args.reps, args.max_iters)
        return 0
    lines = []
    cases = [c.format(guard=args.guard) for c in CASES_ORTHO] if args.ortho else (
        CASES_CONSTRAINED if args.constrained else (CASES_GENERALISED if args.generalised else CASES))
    for case in cases:  # the driver itself never opens the GPU
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps),
               "--max-iters", str(args.max_iters)] + (["--constrained"] if args.constrained else []) + (["--ortho"] if args.ortho else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:  # (a solve that ends at the cap is a result, SPARSH_ENOCONV in "rc", not a failure)
            print(f"{case}: exit status {p.returncode}; the remaining cases are not run", flush=True)
            return p.returncode
        lines += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    with open(args.out, "w") as f:
        f.write("# tools/eig_ab.py: LOBPCG on the block path, one JSON line per case (see the tool's docstring for the fields)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
