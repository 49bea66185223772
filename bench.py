#!/usr/bin/env python3
"""bench.py -- AMG-PCG solve-phase throughput on MI355X (BASELINE.json metric).

A "step" is ONE AMG-preconditioned CG iteration (loop body of Solver_PCG_1/Solver_PCG_4 of the
reference: 1 V(7,7)-cycle + 1 SpMV + 3 reductions + 3 vector updates) on the 7-pt 3D Poisson
matrix of BASELINE.json configs[2] (216^3 = 10 077 696 rows, 70 263 936 nnz, fp64/int32, b = 1,
x0 = 0), inputs resident in HBM.  W warm-up steps, then exactly K timed steps bracketed by
barrier + device sync; rank 0 prints ONE JSON line.  (The convergence test is off during the timed
region and the solve restarts from x = 0 on the device every 48 steps, so any K is valid.)

  python bench.py [--gpus N] [--steps K] [--warmup W] [--grid GRID] [--dump-outputs DIR] [--full [--no-cpu] [--no-pmc] [--no-families]]

A plain run sets up, warms up, times the K steps and prints the line; every other measurement and check
(config.single_sweeps_same_process, roofline.back_to_back_*, config.spmv_finest_level, config.full_solve_to_1e-8,
config.kernel_families, config.reference_level_policy, roofline.traffic, config.comm_us, config.multi_gpu_parity,
cpu_baseline) runs with --full only and is null otherwise.

--dump-outputs DIR writes what the timed path hands its caller after the last timed step, as float64 .npy files:
x_sample.npy (the iterate x at rows x_sample_rows.npy: every row up to 2^21 rows, above that a fixed sample of 2^21
rows drawn with seed 0; rank 0's block at N > 1) and residual_history.npy (the running solve's residual history).
The inputs are generated, not random, so two runs with the same arguments compute the same thing.

Extra objects in the line:
  "roofline"     dominant kernel = fused Jacobi sweep on the finest level.  achieved = the bytes the
                 launched layout has to move per launch (values / indices it really streams + b, x,
                 x_new; stated in DESIGN.md section 4) over the HIP-event time of those launches inside
                 the timed region; frac = achieved / 8 TB/s (<= 1 by construction).  traffic = HBM bytes
                 per launch from rocprofv3 PMC counters collected IN THIS RUN (--full: two child passes,
                 FETCH_SIZE / WRITE_SIZE, tools/pmc_traffic.py) or null.  The SURVEY section 8d CSR
                 model (12 nnz + 36 n) is kept as csr_model_GBps / csr_model_frac: an effective rate,
                 not a roofline fraction, for layouts that do not stream CSR.
  config.kernel_families   (--full) the same iterations with (i) constant-slot folding off, (ii) the CSR-stream
                 family forced (kind 0: reads rowptr/colindex/val exactly as the CSR model assumes),
                 (iii) sliced ELL (kind 2): it/s and dominant-kernel fraction of each.
  "cpu_baseline" (--full) the CPU oracle timed on this host (rank 0, N=1 only): AMG-PCG it/s, bare CSR SpMV
                 GB/s and its fraction of this host's STREAM-triad rate.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import threading
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec


def vcycle_bytes(levels, sweeps):
    """Algorithmic bytes of one V(nu,nu) cycle: per level l < L
    2nu fused sweeps (12 nnz + 36 n) + residual (12 nnz + 28 n) + restrict + prolong."""
    total = 0
    for l, (n, nnz, pn, pnnz) in enumerate(levels[:-1]):
        nc = levels[l + 1][0]
        total += 2 * sweeps * (12 * nnz + 36 * n) + (12 * nnz + 28 * n)
        total += (12 * pnnz + 8 * n + 12 * nc) + (12 * pnnz + 20 * n + 8 * nc)
    nL = levels[-1][0]
    total += 8 * nL * nL + 16 * nL  # dense inverse GEMV on the coarsest level
    return total


DUMP_ROWS = 1 << 21  # rows of x that --dump-outputs writes: 2 x 16 MB in float64 (values + row numbers)


def dump_outputs(out_dir, A, x_dev, nloc, hist):
    """--dump-outputs: the iterate x after the last timed step (a seeded sample of DUMP_ROWS rows when it has more) and the
    running solve's residual history -- what krylov_step_dev / krylov_history hand their caller -- as float64 .npy files."""
    os.makedirs(out_dir, exist_ok=True)
    x = np.empty(nloc)
    A.d2h(x, x_dev)
    rows = np.arange(nloc) if nloc <= DUMP_ROWS else np.sort(np.random.default_rng(0).choice(nloc, DUMP_ROWS, replace=False))
    np.save(os.path.join(out_dir, "x_sample.npy"), x[rows])
    np.save(os.path.join(out_dir, "x_sample_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(out_dir, "residual_history.npy"), np.asarray(hist, dtype=np.float64))


T0 = time.time()


def log(msg):
    print(f"[bench +{time.time() - T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=int(os.environ.get("SPARSH_BENCH_GRID", "216")),
                    help="grid points per side (216 -> 10.08M rows); env SPARSH_BENCH_GRID")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement and check beyond the timed steps (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu", action="store_true", default=os.environ.get("SPARSH_BENCH_NO_CPU", "0") == "1",
                    help="with --full: skip the cpu_baseline leg; env SPARSH_BENCH_NO_CPU=1")
    ap.add_argument("--cpu-iters", type=int, default=30)  # ~10 s of 16-thread CPU work at 216^3
    ap.add_argument("--rccl", action="store_true", help="install the RCCL transport even with one rank (path check)")
    ap.add_argument("--no-pmc", action="store_true", default=os.environ.get("SPARSH_BENCH_NO_PMC", "0") == "1",
                    help="with --full: skip the two rocprofv3 --pmc child passes that measure roofline.traffic; env SPARSH_BENCH_NO_PMC=1")
    ap.add_argument("--no-families", action="store_true", default=os.environ.get("SPARSH_BENCH_NO_FAMILIES", "0") == "1",
                    help="with --full: skip the general-layout / CSR-stream / sliced-ELL comparison runs")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # Exactly one line may reach stdout (the JSON record): libraries such as RCCL print banners
    # there, so everything else is routed to stderr and the record is written to the saved fd.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    dist = None
    if world > 1 or "RANK" in os.environ:
        import torch
        import torch.distributed as dist_mod

        # (local_rank % device count: several ranks may share a GPU -- a development aid to exercise the RCCL path on a one-GPU box,
        # where RCCL allows it; never used by the driver, which gives every rank a GPU of its own)
        dev_index = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(dev_index)
        dist_mod.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        dist = dist_mod

    # Multi-GPU insurance: the partitioned path (RCCL halo exchange) cannot be exercised with N >= 2 on the one-GPU boxes this
    # repo is developed on, so the whole multi-rank run sits under a watchdog.  A hang (a defect to diagnose from the log, not a
    # measurement) ends with ONE record that says so and a non-zero exit code instead of blocking the launcher forever.
    dist_dog = None
    emitted = [False]
    if world > 1:
        def dist_bail():
            msg = f"multi-GPU run did not finish within {dist_timeout:.0f} s on rank {rank} (hang in the partitioned solver or its transport)"
            log(msg)
            if rank == 0 and not emitted[0]:
                rec = {"metric": "AMG-PCG solve iterations/sec (7-pt 3D Poisson, fp64) + HBM GB/s", "value": 0.0, "unit": "iterations/s", "n_gpus": world,
                       "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
                       "dtype": "f64", "data": "synthetic", "failed": True, "config": {"workload": f"7-pt 3D Poisson CSR {args.grid}^3", "failure": msg}}
                os.write(json_fd, (json.dumps(rec) + "\n").encode())
            os._exit(5)

        dist_timeout = float(os.environ.get("SPARSH_BENCH_DIST_TIMEOUT", "900"))
        dist_dog = threading.Timer(dist_timeout, dist_bail)
        dist_dog.daemon = True
        dist_dog.start()

    import sparsh_amg_amd as sa
    from sparsh_amg_amd import problems

    kcfg = os.environ.get("SPARSH_BENCH_KCFG")  # A/B runs: "kind,vec,nt,remap" instead of the per-operator policy
    no_fold = os.environ.get("SPARSH_BENCH_NO_FOLD", "0") == "1"  # profile the general layout (what a variable-coefficient operator gets)

    def new_handle(fold=True, cfg=None, idx16=None):
        H = sa.sp_matrix_mg(rp, ci, v)
        if not fold:
            H.set_const_slots(False)
        if idx16 is not None:
            H.set_index_compression(idx16)
        if cfg:
            H.set_kernel_config(*cfg)
        return H

    if sa.device_count() < 1:
        raise SystemExit("bench.py needs a GPU: the HIP path is the only compute path")

    log(f"generating 7-pt Poisson {args.grid}^3")
    t_gen = time.time()
    rp, ci, v = problems.poisson3d(args.grid)
    n = len(rp) - 1
    nnz = int(rp[-1])
    t_gen = time.time() - t_gen

    # tol = 0: the loop never stops early, so exactly W + K iterations run (the real solve
    # converges to 1e-8 in ~41 iterations; reported separately as config.full_solve_to_1e-8)
    host_threads = max(1, sa.host_cpus() // max(1, local_world))
    prm = sa.default_params(print_setup=0, print_solve=0, tol=0.0, device=local_rank, check_every=1 << 30, host_threads=host_threads)
    main_cfg = [int(t) for t in kcfg.split(",")] if kcfg else None
    main_idx16 = int(os.environ["SPARSH_BENCH_IDX16"]) if "SPARSH_BENCH_IDX16" in os.environ else None  # profiling runs of the 16-bit index family
    A = new_handle(fold=not no_fold, cfg=main_cfg, idx16=main_idx16)
    mode, mode_note = "single", None
    if world > 1 or args.rccl:
        # one process per GPU: row-block partition, halo exchange over RCCL.  The 128-byte RCCL id
        # travels from rank 0 through torch.distributed.  If any rank fails to bring the transport
        # or the partitioned hierarchy up, ALL ranks agree (torch all-reduce) to fall back to N
        # independent replicas, and the record says so.
        ok, err = 1, ""
        try:
            sa.set_device(local_rank % max(1, sa.device_count()))
            uid = [sa.comm_unique_id() if rank == 0 else None]
            if dist is not None:
                dist.broadcast_object_list(uid, src=0)
            A.comm_init_rccl(uid[0], rank, world)
            if os.environ.get("SPARSH_BENCH_DEEP_HALO", "1") != "1":
                A.set_deep_halo(False)
            log(f"setup ({host_threads} host threads, partitioned)")
            A.setup(prm)
            mode = "partitioned"
        except Exception as e:  # noqa: BLE001
            ok, err = 0, repr(e)
            log(f"partitioned setup failed on rank {rank}: {err}")
        if dist is not None:
            import torch

            flag = torch.tensor([ok], device="cuda")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            ok = int(flag.item())
        if not ok:
            mode, mode_note = "replicas", (f"FAILED for the multi-GPU metric: partitioned start-up failed ({err or 'on another rank'}); "
                                           f"each of the {world} ranks ran an independent replica and `value` is ONE replica's rate")
            A = new_handle(fold=not no_fold, cfg=main_cfg)
            A.setup(prm)
    else:
        log(f"setup ({host_threads} host threads)")
        A.setup(prm)
    log(f"setup done: {A.nlevels} levels, host setup {A.setup_seconds:.1f}s, mode {mode}")
    coarse = A.coarse_info()
    levels = []
    for l in range(A.nlevels):
        i = A.level_info(l)
        levels.append((i["nrow"], i["nnz"], i["p_ncol"], i["p_nnz"]))
    sweeps = prm.sweeps

    lo, hi, replicated = A.local_range(0)
    nloc = hi - lo
    b = np.ones(n)
    bd = A.dev_alloc(8 * nloc)
    xd = A.dev_alloc(8 * nloc)
    A.h2d(bd, b[lo:hi])
    A.h2d(xd, np.zeros(nloc))
    partitioned_levels = sum(1 for l in range(A.nlevels) if not A.local_range(l)[2])

    def barrier():
        A.sync()
        if dist is not None:
            dist.barrier()
        A.sync()

    # CG converges: after ~40 iterations the residual is at rounding level and after a few hundred
    # the recurrences underflow (0/0).  To time ANY number of steps the solve is restarted from
    # x = 0 every RESTART iterations, entirely on the device; the restart (one SpMV, one V-cycle,
    # two reductions: about one more iteration of work) stays inside the timed region but is not
    # counted as a step, so long runs read slightly LOW, never high.
    RESTART = 48
    since_init = [0]
    first_segment = []  # residual history of the first solve segment (parity checks compare this one)

    def run_steps(k):
        left = k
        while left > 0:
            if since_init[0] >= RESTART:
                if not first_segment:
                    first_segment.append(A.krylov_history())
                A.dev_fill(xd, nloc, 0.0)
                A.krylov_init_dev("pcg", bd, xd)
                since_init[0] = 0
            m = min(left, RESTART - since_init[0])
            done_m, _ = A.krylov_step_dev(m)
            assert done_m == m, (done_m, m)
            since_init[0] += m
            left -= m
        return k

    log("krylov init + warmup")
    A.krylov_init_dev("pcg", bd, xd)
    if args.warmup > 0:
        run_steps(args.warmup)
    no_profile = os.environ.get("SPARSH_BENCH_NO_PROFILE", "0") == "1"  # per-launch events keep hipGraph replay off
    if not no_profile:
        A.profile(True)
    barrier()
    log("timed region")
    ex0 = A.exchanges_issued()
    t0 = time.perf_counter()
    done = run_steps(args.steps)
    barrier()
    t1 = time.perf_counter()
    exchanges_per_step = (A.exchanges_issued() - ex0) / max(1, args.steps)
    if not no_profile:
        A.profile(False)
    assert done == args.steps, (done, args.steps)
    elapsed = t1 - t0
    if dist is not None:
        import torch

        t = torch.tensor([elapsed], device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    last_hist = A.krylov_history()
    hist = first_segment[0] if first_segment else last_hist
    if not (np.all(np.isfinite(hist)) and np.all(np.isfinite(last_hist))):
        raise SystemExit("non-finite residual in the timed run")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, A, xd, nloc, last_hist)

    # dominant kernel: fused Jacobi sweep on the finest level, timed by HIP events on the
    # engine's stream inside the timed region (sparsh_profile)
    def layout_bytes(H, nrow, nnz_l, level=0, vectors=3):
        """Bytes the layout a handle launches on a level has to move per SpMV-type launch: the value (and index) streams it
        really reads + `vectors` n-vectors (fused sweep: b, x gathered once, x_new = 3; residual 3; plain SpMV 2); the mirrors
        take d_i out of the value stream."""
        fmt, stored = H.level_format(level)
        _, _, meta = H.level_layout(level)
        vec = 8 * vectors * nrow
        if fmt == 3:
            return 8 * stored + meta + vec
        if fmt == 2:
            return 12 * stored + 4 * nrow + vec
        if H.level_kernel(level) == "csr_rowlane_kernel":
            return 12 * nnz_l + 4 * nrow + vec  # CSR-stream with the diagonal picked out of the value stream: diag[] is not read
        if H.level_kernel(level) == "csr_rowlane16_kernel":
            b16, nb = H.level_index16(level)  # 16-bit delta-coded column indices (+ 4 B of base per row block); blocks that keep col[] priced at 12 B
            return int(round((10 * b16 + 12 * (nb - b16)) / max(nb, 1) * nnz_l)) + 4 * nb + 4 * nrow + vec
        return 12 * nnz_l + 12 * nrow + vec  # CSR-stream: rowptr, col, val, d + the vectors = the SURVEY 8d model itself

    def iteration_layout_bytes(H):
        """Bytes one AMG-PCG iteration has to move with the layouts this handle launches (SURVEY 8d metric (ii), priced per
        launch as roofline.bytes_per_launch is): per level l < L 2 nu - 1 fused sweeps + the zero-guess sweep (x = w b / d: 3
        vectors; on level 0 it rides in cg_update) + residual + aggregation restrict / prolong, the coarsest solve, and on
        level 0 the Krylov step: SpMV with the p.Ap dot, cg_update (p, Ap, x, r, d read; x, r, z written), p update."""
        total = 0
        prev_paired = False
        zero_written = {}
        dvec = [0 if H.level_constant_diagonal(l)[0] else 8 for l in range(len(levels))]  # bytes per row of a level's diag[] stream where it is read
        for l, (nl, nnzl, pn, pnnz) in enumerate(levels[:-1]):
            ncl = levels[l + 1][0]
            from_b = world == 1 and H.level_double_sweep(l)["on"] and sweeps >= 3  # the down-leg's first launch: sweeps 1 - 3 from b alone (16 B per row)
            if world == 1 and H.level_double_sweep(l)["on"]:
                # both legs: (sweeps - 1) plain sweeps run as pairs (one pass over x, b, y: 24 B per row), the rest -- and the last
                # post-sweep, which carries the dot / the prolongation -- as single sweeps
                pairs = 2 * ((sweeps - 1) // 2)
                singles = 2 * ((sweeps - 1) % 2) + 1
                total += pairs * 24 * nl + singles * layout_bytes(H, nl, nnzl, l, 3) - (8 * nl if from_b else 0)
            else:
                total += (2 * sweeps - 1) * layout_bytes(H, nl, nnzl, l, 3)
            zero_written[l] = not from_b
            if l > 0 and not prev_paired and not from_b:
                total += (16 + dvec[l]) * nl
            prev_paired = H.level_paired(l)
            if prev_paired:  # residual + restriction + the coarse zero-guess sweep in one launch: x, b in; b_c, x_c out, d_c in
                nxt_from_b = world == 1 and l + 1 < len(levels) - 1 and H.level_double_sweep(l + 1)["on"] and sweeps >= 3
                total += layout_bytes(H, nl, nnzl, l, 2) + (8 if nxt_from_b else 16 + dvec[l + 1]) * ncl
            else:
                total += layout_bytes(H, nl, nnzl, l, 3) + (4 * (ncl + 1) + 4 * pnnz + 8 * nl + 8 * ncl)
            form = H.level_prolong_fused(l + 1)
            if form:  # level l+1's last post-sweep adds its result to x_l itself: x_l read + written, (first, second) records unless the
                      # aggregates are the row pairs; that sweep does not store its own result
                total += 16 * nl + (8 * ncl if form == 2 else 0) - 8 * ncl
            else:
                total += 4 * nl + 8 * ncl + 16 * nl
        total += coarse["bytes"] + 16 * levels[-1][0]
        n0, nnz0 = levels[0][0], levels[0][1]
        # Krylov step: A p with the dot; residual update (Ap, r read; r [, z0] written [, d read]); x += alpha p and p = z + beta p in one kernel
        # (z, p, x read; p, x written)
        total += layout_bytes(H, n0, nnz0, 0, 2) + ((24 if zero_written.get(0) is False else 32 + dvec[0])) * n0 + 40 * n0
        return total

    def double_sweep(H):
        return world == 1 and mode == "single" and H.level_double_sweep(0)["on"]

    def kernel_label(H):
        nt, remap = H.level_placement(0)
        if double_sweep(H):
            d = H.level_double_sweep(0)
            return (f"sdia_box2_kernel<Q={d['points_per_thread']}, TAG=1> (TWO fused Jacobi sweeps per launch on the finest level: {d['lines_per_tile']} grid lines x "
                    f"{d['planes_per_chunk']} planes per workgroup, first sweep's plane in LDS)")
        return f"{H.level_kernel(0)}<OP_JACOBI=2, NT={'true' if nt else 'false'}, TAG=1> (fused Jacobi sweep, finest level; XCD remap mode {remap})"

    pr = A.profile_read()
    jac_bytes = 12 * pr["nnz"] + 36 * pr["nrow"]  # SURVEY §8d CSR model, this rank's block of the finest level
    fmt, stored = A.level_format(0)
    slots, vblocks, meta_bytes = A.level_layout(0)
    fmt_bytes = layout_bytes(A, pr["nrow"], pr["nnz"])
    dbl = double_sweep(A)
    if dbl:
        # one launch = two sweeps in one pass: x and b read, the second sweep's result written -- no matrix stream, no masks
        fmt_bytes = 24 * pr["nrow"]
        jac_bytes *= 2
    single_sweeps = None
    if dbl and args.full:
        # the same handle, same hierarchy, with the double sweep switched off (outside the timed region): what the launch-per-sweep
        # path gives on this box in this process; histories are bitwise the same (tests/test_gpu_parity.py)
        try:
            A.set_double_sweep(0)
            run_steps(min(args.steps, 24))
            barrier()
            ts0 = time.perf_counter()
            run_steps(args.steps)
            barrier()
            ts1 = time.perf_counter()
            single_sweeps = {"iterations_per_s": round(args.steps / (ts1 - ts0), 2), "steps": args.steps,
                             "note": "sparsh_set_double_sweep(0): every Jacobi sweep a launch of its own (the round-2 path)"}
        except Exception as e:  # noqa: BLE001
            single_sweeps = {"error": repr(e)}
        finally:
            A.set_double_sweep(1)
    roof = None
    if pr["launches"] > 0:
        avg = pr["seconds"] / pr["launches"]
        achieved = fmt_bytes / avg / 1e9
        roof = {
            "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
            "kernel": kernel_label(A), "launches": pr["launches"],
            "avg_us": round(avg * 1e6, 2), "bytes_per_launch": fmt_bytes,
            "note": "achieved/frac price the kernel with the bytes its own layout streams per launch (bytes_per_launch; DESIGN.md section 4). "
                    "csr_model_* price the same launch with SURVEY section 8d's CSR model (12*nnz + 36*n): an effective rate, above the HBM peak "
                    "when the layout does not stream column indices / folded constant diagonals. traffic = PMC bytes per launch measured in this run "
                    "(null when the counter passes were skipped or failed). A value-free table sweep is bound by L2->CU delivery, not HBM "
                    "(DESIGN.md section 4), so its HBM fraction is low by construction; the CSR-stream family in config.kernel_families is the "
                    "HBM-bound path of north_star",
            "csr_model_bytes_per_launch": jac_bytes, "csr_model_GBps": round(jac_bytes / avg / 1e9, 1),
            "csr_model_frac": round(jac_bytes / avg / 1e9 / HBM_PEAK_GBS, 4),
            "layout": {"slots": slots, "value_blocks": vblocks, "constant_slots": slots - vblocks, "descriptor_bytes": meta_bytes} if fmt == 3 else None,
        }
        if dbl:
            single = layout_bytes(A, pr["nrow"], pr["nnz"])
            roof["sweeps_per_launch"] = 2
            roof["us_per_sweep"] = round(avg * 1e6 / 2, 2)
            # what two launches of the single-sweep kernel would have to sustain to finish in the same time: an EFFECTIVE rate (above the HBM
            # peak: the point of temporal blocking), not a bandwidth
            roof["two_single_sweeps_equivalent_GBps"] = round(2 * single / avg / 1e9, 1)
            roof["double_sweep"] = A.level_double_sweep(0)
            roof["note"] = ("the dominant kernel is the double sweep (sparsh_set_double_sweep; DESIGN.md section 4): ONE launch performs TWO Jacobi sweeps of the finest level in one "
                            "pass over x, b and the result (temporal blocking: the first sweep's plane stays in LDS, its halo is recomputed). achieved/frac price a LAUNCH with the "
                            "bytes it has to move -- bytes_per_launch = 24 B per row: x and b read, the second sweep's result written; the operator itself is seven kernel arguments. "
                            f"Two launches of the single-sweep kernel this replaces move 2 x {single} B. traffic = PMC bytes per launch of this kernel (halo lines and planes "
                            "are read by two workgroups; what the L2s and the Infinity Cache do not absorb shows there). csr_model_* price the launch with SURVEY section 8d's CSR "
                            "model for TWO sweeps (2 x (12*nnz + 36*n)): an effective rate, not a bandwidth. With 16 waves per CU and two workgroup barriers per plane the kernel "
                            "is bound by fp64 VALU issue (7 mul + 7 add + an IEEE division per row and sweep, 2.3 sweep-equivalents per launch with the recomputed halo) about "
                            "as much as by HBM; avg_us is measured inside the solve over runs of consecutive double-sweep launches")
        if args.full and world == 1 and mode == "single":
            # the same kernel launched back to back in this process (outside the timed region): the in-solve figure above varies
            # from process to process with the physical placement of a working set the size of the Infinity Cache
            try:
                pinfo = A.placement_info()
                # on the buffers the solve uses (the setup's placement search timed exactly this), else on fresh ones
                if dbl:  # (the placement search times the kernel the legs run and reports us per SWEEP)
                    b2b = 2 * pinfo["chosen_us"] * 1e-6 if pinfo["triples"] > 0 else A.bench_op("jacobi_double", 0, 20)
                else:
                    b2b = pinfo["chosen_us"] * 1e-6 if pinfo["triples"] > 0 else A.bench_op("jacobi_pingpong", 0, 20)
                roof["back_to_back_us"] = round(b2b * 1e6, 2)
                roof["back_to_back_frac"] = round(fmt_bytes / b2b / 1e9 / HBM_PEAK_GBS, 4)
                roof["note"] += (". avg_us is measured inside the solve; back_to_back_us is the same kernel ping-ponging between two vectors alone. "
                                 "For the default table path at 216^3 the three sweep vectors (0.24 GB) are the size of the Infinity Cache: the same sweep takes 42-64 us "
                                 "depending on the physical pages behind them, so sparsh_setup picks the buffers by timing (config.placement_search; "
                                 "profiles/r02_finest_sweep_placement_luck.txt)")
            except Exception as e:  # noqa: BLE001
                log(f"back-to-back measurement failed: {e!r}")

    # whole-iteration algorithmic bytes: V-cycle + SpMV + 2 dot + nrm2 + 3 axpy-type
    it_bytes = vcycle_bytes(levels, sweeps) + (12 * nnz + 20 * n) + 2 * 16 * n + 8 * n + 3 * 24 * n
    its_per_s = args.steps / elapsed  # replicas fallback: ONE replica's rate (never multiplied by the rank count)

    # the metric's second half: plain SpMV y = A x on the finest level (HIP events, 20 launches, outside
    # the timed region), priced with the CSR model 12*nnz + 20*n of SURVEY §8d
    spmv = None
    if args.full and mode != "replicas":
        try:
            t_spmv = A.bench_op("spmv", 0, 20)
            sp_bytes = 12 * pr["nnz"] + 20 * pr["nrow"]
            sp_layout = layout_bytes(A, pr["nrow"], pr["nnz"], 0, 2)
            spmv = {"us": round(t_spmv * 1e6, 2), "kernel": A.level_kernel(0), "bytes_per_launch": sp_layout,
                    "GBps": round(sp_layout / t_spmv / 1e9, 1), "frac": round(sp_layout / t_spmv / 1e9 / HBM_PEAK_GBS, 4),
                    "csr_model_bytes": sp_bytes, "csr_model_effective_GBps": round(sp_bytes / t_spmv / 1e9, 1),
                    "note": "GBps / frac price the SpMV with the bytes the launched layout streams (value / index streams + x, y); csr_model_effective_GBps "
                            "prices it with SURVEY 8d's 12 nnz + 20 n: an effective rate (above the HBM peak where the layout does not stream CSR), not a bandwidth",
                    "rows": pr["nrow"], "nnz": pr["nnz"]}
        except Exception as e:  # noqa: BLE001
            spmv = {"error": repr(e)}

    # outside the timed region: a complete solve to the reference tolerance on the same hierarchy
    full = None
    if args.full:
        log("full solve to tol=1e-8")
        A.set_stopping(1e-8, 100000, 1)
        A.h2d(xd, np.zeros(nloc))
        hfull, it_full, sec_full, rc_full = A.solve_dev("pcg", bd, xd)
        full = {"iterations": it_full, "seconds": round(sec_full, 4), "final_residual": float(hfull[-1]) if len(hfull) else None, "rc": rc_full}

    # the boundary hands over host buffers (reference API): same full solve through sparsh_solve,
    # which adds H2D of b and x and D2H of x over PCIe -- reported, never used as `value`
    if args.full and world == 1 and mode == "single":
        xh = np.zeros(n)
        t_h = time.perf_counter()
        hh, rc_h = A.solve("pcg", b, xh)
        t_h = time.perf_counter() - t_h
        full["host_buffer_path_seconds"] = round(t_h, 4)
        full["host_buffer_path_iterations_per_s"] = round(len(hh) / t_h, 2)

    # transparency: the same iterations through the other layouts / kernel families, each on a handle of its
    # own (per-handle config), driver-timed in this process: (i) constant-slot folding off = what a
    # variable-coefficient operator gets (8 B per stored entry, no indices); (ii) the CSR-stream family
    # forced (rowptr/colindex/val streamed exactly as north_star describes; what every unstructured matrix
    # gets); (iii) sliced ELL.  Residual histories must equal the main run's (all families are bitwise equal).
    general = None
    families = None
    if args.full and world == 1 and mode == "single" and not args.no_families:
        families = {}
        runs = [("general_values_layout", dict(fold=False, cfg=None), "constant-slot folding off: sliced diagonals with 8 B per stored entry, no column indices"),
                ("csr_stream_kind0", dict(fold=True, cfg=(0, 3, -1, -1)), "workgroup CSR-stream kernels forced on every level: rowptr + colindex + val streamed (12 B per entry); "
                                                                        "levels that stream from HBM run csr_rowlane_kernel (gathers in row-lane order), cache-resident ones csr_block_kernel"),
                ("csr_stream_kind0_idx16", dict(fold=True, cfg=(0, 3, -1, -1), idx16=2), "CSR-stream with compressed column indices (SURVEY 8f-4): 16-bit deltas per row block, 10 B per entry; "
                                                                                       "levels that stream from HBM run csr_rowlane16_kernel"),
                ("csr_stream_kind0_block_kernel", dict(fold=True, cfg=(0, 1, -1, -1)), "the same with the round-1 csr_block_kernel (gathers in CSR order) on every level"),
                ("sliced_ell_kind2", dict(fold=True, cfg=(2, 0, -1, -1)), "sliced-ELL mirror forced where it exists (12 B per padded entry)")]
        for key, kw, note in runs:
            log(f"kernel family run: {key}")
            try:
                A2 = new_handle(**kw).setup(prm)
                b2 = A2.dev_alloc(8 * n)
                x2 = A2.dev_alloc(8 * n)
                A2.h2d(b2, b)
                A2.h2d(x2, np.zeros(n))
                A2.krylov_init_dev("pcg", b2, x2)
                kk = min(args.steps, RESTART - 4)
                A2.krylov_step_dev(3)
                A2.profile(True)
                A2.sync()
                t_g = time.perf_counter()
                A2.krylov_step_dev(kk)
                A2.sync()
                t_g = time.perf_counter() - t_g
                A2.profile(False)
                p2 = A2.profile_read()
                h2 = A2.krylov_history()
                m2 = min(len(h2), len(hist))
                lb = layout_bytes(A2, n, nnz)
                avg2 = p2["seconds"] / p2["launches"] if p2["launches"] else float("nan")
                sp2 = A2.bench_op("spmv", 0, 20)
                fam = {"iterations_per_s": round(kk / t_g, 2), "steps": kk, "kernel": kernel_label(A2),
                       "jacobi_fine_us_in_solve": round(avg2 * 1e6, 2), "jacobi_fine_us_back_to_back": round(A2.bench_op("jacobi", 0, 20) * 1e6, 2),
                       "bytes_per_launch": lb, "GBps": round(lb / avg2 / 1e9, 1), "frac": round(lb / avg2 / 1e9 / HBM_PEAK_GBS, 4),
                       "csr_model_frac": round((12 * nnz + 36 * n) / avg2 / 1e9 / HBM_PEAK_GBS, 4),
                       "spmv_us": round(sp2 * 1e6, 2), "spmv_csr_model_GBps": round((12 * nnz + 20 * n) / sp2 / 1e9, 1),
                       "residual_history_identical": bool(np.array_equal(h2[:m2], hist[:m2])), "note": note}
                families[key] = fam
                A2.close()
            except Exception as e:  # noqa: BLE001
                families[key] = {"error": repr(e)}
        general = families.get("general_values_layout")

    # transparency: the same problem with the REFERENCE's own level policy (level1 = 6 levels, whatever is left -- 314 928 rows at 216^3 --
    # goes to the direct solver, src/AMG_phases.cpp:51,77,89): iterations to 1e-8, time, and the steady iteration rate
    ref_policy = None
    if args.full and world == 1 and mode == "single" and not args.no_families and coarse["extended"]:
        log("reference level policy run (6 levels, direct solve of the rest)")
        try:
            prm_ref = sa.default_params(print_setup=0, print_solve=0, device=local_rank, host_threads=host_threads, coarse_limit=1 << 30)
            A3 = new_handle(fold=not no_fold, cfg=main_cfg).setup(prm_ref)
            b3 = A3.dev_alloc(8 * n)
            x3 = A3.dev_alloc(8 * n)
            A3.h2d(b3, b)
            A3.h2d(x3, np.zeros(n))
            h3, it3, sec3, rc3 = A3.solve_dev("pcg", b3, x3)
            c3 = A3.coarse_info()
            ref_policy = {"levels": [A3.level_info(l)["nrow"] for l in range(A3.nlevels)], "coarsest_level": c3,
                          "coarse_solve_us": round(A3.bench_op("coarse", A3.nlevels - 1, 10) * 1e6, 1),
                          "iterations_to_1e-8": it3, "seconds": round(sec3, 4), "iterations_per_s": round(it3 / sec3, 2), "rc": rc3,
                          "setup_seconds": round(A3.setup_seconds, 2),
                          "note": "the iteration the reference itself runs at this size (its PARDISO solve of the 6th level done by the device's nested-dissection "
                                  "factors); `value` is measured on the extended hierarchy, whose iterations are cheaper and more numerous"}
            A3.close()
        except Exception as e:  # noqa: BLE001
            ref_policy = {"error": repr(e)}

    # roofline.traffic: HBM bytes per launch of the dominant kernel from PMC counters, collected in THIS run by
    # two child processes (separate FETCH_SIZE / WRITE_SIZE passes, MI355X_MICROARCH.md), same grid, same
    # kernel configuration; corrected with calibration kernels of known size run in the same child.
    pmc_iteration = None
    if args.full and roof is not None and rank == 0 and world == 1 and mode == "single" and not args.no_pmc:
        import shutil
        import subprocess
        import tempfile

        rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        tmpd = tempfile.mkdtemp(prefix="sparsh_pmc_", dir="/tmp")
        lay = os.path.join(tmpd, "layout.json")
        try:
            if not os.path.exists(rocprof):
                raise RuntimeError("rocprofv3 not found")
            env = dict(os.environ, TMPDIR="/tmp")
            for ctr, sub in (("FETCH_SIZE", "fetch"), ("WRITE_SIZE", "write")):
                log(f"PMC pass {ctr}")
                cmd = [rocprof, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmpd, sub), "--",
                       sys.executable, os.path.join(ROOT, "tools", "pmc_traffic.py"), "--run", "--grid", str(args.grid), "--layout", lay, "--iters", "10"]
                if kcfg:
                    cmd += ["--kcfg", kcfg]
                if no_fold:
                    cmd += ["--no-fold"]
                subprocess.run(cmd, cwd="/tmp", env=env, timeout=240, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import pmc_traffic

            res = pmc_traffic.summarize(os.path.join(tmpd, "fetch"), os.path.join(tmpd, "write"), None, args.grid, lay, quiet=True)
            measured_kernel = json.load(open(lay)).get("kernel")
            want_kernel = "sdia_box2_kernel" if dbl else A.level_kernel(0)
            if measured_kernel != want_kernel:
                raise RuntimeError(f"PMC child ran {measured_kernel}, the timed run {want_kernel}")
            traffic = float(res["jacobi_fine_bytes_per_launch"])
            avg = roof["avg_us"] * 1e-6
            roof["traffic"] = round(traffic)
            roof["traffic_GBps"] = round(traffic / avg / 1e9, 1)
            roof["traffic_frac"] = round(traffic / avg / 1e9 / HBM_PEAK_GBS, 4)
            roof["traffic_over_layout_bytes"] = round(traffic / fmt_bytes, 3)
            pmc_iteration = res.get("iteration")
            roof["traffic_how"] = ("rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE child passes of this run (tools/pmc_traffic.py): counter KiB -> bytes, "
                                   f"FETCH_SIZE x{res['fetch_correction']['8B_per_lane(axpby)']:.4f} from an axpby of known size in the same process")
            try:
                os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
                json.dump(res, open(os.path.join(ROOT, "gpurun_out", "pmc_bench_run.json"), "w"), indent=1)
            except OSError:
                pass
        except Exception as e:  # noqa: BLE001
            log(f"PMC passes failed: {e!r}")
            roof["traffic"] = None
            roof["traffic_how"] = f"not measured in this run ({e!r})"
        finally:
            shutil.rmtree(tmpd, ignore_errors=True)
    elif roof is not None:
        roof["traffic_how"] = "not measured in this run (counter passes run with --full at N=1 on rank 0 only, unless disabled)"

    # SURVEY 8d metric (ii): HBM GB/s of the whole iteration -- on the bytes the launched layouts have to move, and on the bytes
    # the PMC counters saw (the same child passes as roofline.traffic, 10 iterations between marker launches)
    whole = None
    if mode == "single" and world == 1:
        lay_it = iteration_layout_bytes(A)
        whole = {"layout_GB_per_iteration": round(lay_it / 1e9, 4), "layout_GBps": round(lay_it * its_per_s / 1e9, 1),
                 "layout_frac": round(lay_it * its_per_s / 1e9 / HBM_PEAK_GBS, 4),
                 "hbm_GB_per_iteration": None, "hbm_GBps": None, "hbm_frac": None,
                 "note": "layout_* = bytes the launched layouts have to move per iteration (every SpMV-type launch priced like roofline.bytes_per_launch, "
                         "+ transfer, Krylov and coarsest-solve bytes) x iterations/s; hbm_* = FETCH_SIZE + WRITE_SIZE summed over every dispatch of 10 "
                         "iterations in the PMC child passes of this run x iterations/s (Infinity-Cache hits are counted by these counters); both <= 1 of 8 TB/s"}
        if pmc_iteration:
            hb = pmc_iteration["hbm_bytes_per_iteration"]
            whole.update({"hbm_GB_per_iteration": round(hb / 1e9, 4), "hbm_GBps": round(hb * its_per_s / 1e9, 1),
                          "hbm_frac": round(hb * its_per_s / 1e9 / HBM_PEAK_GBS, 4),
                          "hbm_read_GB_per_iteration": round(pmc_iteration["hbm_read_bytes_per_iteration"] / 1e9, 4),
                          "hbm_write_GB_per_iteration": round(pmc_iteration["hbm_write_bytes_per_iteration"] / 1e9, 4),
                          "dispatches_per_iteration": pmc_iteration["dispatches_per_iteration"]})

    # multi-GPU diagnostics for tuning (collective calls, every rank): what one halo exchange, one
    # scalar all-reduce and the all-gather at the replication boundary cost on this node
    comm_us = None
    if args.full and mode == "partitioned":
        try:
            comm_us = {"halo_exchange_level": {}, "note": "average of 50 back-to-back steps alone on the engine's stream (HIP events, rank 0)"}
            for l in range(A.nlevels):
                if A.local_range(l)[2]:
                    break
                t_h = A.bench_comm("halo", l, 50)
                comm_us["halo_exchange_level"][str(l)] = round(t_h * 1e6, 2) if t_h >= 0 else None
            t_r = A.bench_comm("allreduce", 0, 50)
            t_g = A.bench_comm("allgather", 0, 20)
            comm_us["allreduce_16B"] = round(t_r * 1e6, 2) if t_r >= 0 else None
            comm_us["allgather_at_replication_boundary"] = round(t_g * 1e6, 2) if t_g >= 0 else None
        except Exception as e:  # noqa: BLE001
            comm_us = {"error": repr(e)}

    # multi-GPU parity: rank 0 repeats the same iterations on ONE GPU (fresh handle, no transport)
    # and compares residual histories; the other ranks wait at the barrier below.
    parity = None
    if args.full and mode == "partitioned" and world > 1:
        if rank == 0:
            log("1-GPU reference run for the parity check")
            A1 = sa.sp_matrix_mg(rp, ci, v).setup(prm)
            b1 = A1.dev_alloc(8 * n)
            x1 = A1.dev_alloc(8 * n)
            A1.h2d(b1, b)
            A1.h2d(x1, np.zeros(n))
            A1.krylov_init_dev("pcg", b1, x1)
            A1.krylov_step_dev(min(args.warmup + args.steps, RESTART))
            h1 = A1.krylov_history()
            m = min(len(h1), len(hist))
            dev = float(np.max(np.abs(hist[:m] - h1[:m]) / h1[:m])) if m else None
            parity = {"iterations_compared": m, "max_rel_deviation_vs_1gpu": dev, "ok": bool(m > 0 and dev < 1e-6)}
            A1.close()
        if dist is not None:
            dist.barrier()

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu:
        import oracle

        ncores = sa.host_cpus()
        log(f"cpu_baseline: oracle setup with {ncores} threads")
        t_o = time.time()
        OA = oracle.Csr(rp, ci, v)
        # The oracle's direct solver is a banded LU (its stand-in for PARDISO): on the 39 366-row coarsest level the device run stops
        # at, that would be ~100 GFlop of factorisation and a sequential band sweep per cycle -- nothing like the reference's PARDISO.
        # The CPU gets the hierarchy that suits it best instead: extended by the same coarsening rule until <= limit_upper rows
        # (cheap dense-ish coarsest solve), i.e. round 2's hierarchy; the level counts of both runs are in the record.
        cpu_levels = len(levels)
        if coarse["extended"] and not coarse["dense"]:
            nl = levels[-1][0]
            while nl > prm.limit_upper:
                nl = (nl + 1) // 2
                cpu_levels += 1
        oprm = oracle.params(threads=ncores, max_levels=cpu_levels, tol=0.0)
        H = oracle.Hierarchy(OA, oprm)
        t_setup = time.time() - t_o
        log(f"cpu_baseline: oracle setup {t_setup:.1f}s; {args.cpu_iters} PCG iterations")
        _, ho, sec = H.pcg(b, max_it=args.cpu_iters)
        log(f"cpu_baseline: done in {sec:.1f}s")
        cpu_its = len(ho) / sec
        # the reference's own thread setting (`th` = 2, include/AMG.hpp:15) on a short sample
        two = None
        try:
            H2 = oracle.Hierarchy(OA, oracle.params(threads=2, max_levels=cpu_levels, tol=0.0))
            _, h2, sec2 = H2.pcg(b, max_it=3)
            two = {"value": round(len(h2) / sec2, 4), "unit": "iterations/s", "cores": 2,
                   "sample": f"{len(h2)} iterations, {sec2:.1f} s (the reference's compile-time default th = 2)"}
            del H2
        except Exception as e:  # noqa: BLE001
            two = {"error": repr(e)}
        # bare CSR SpMV on the host and the host's STREAM-triad rate
        spmv_cpu = None
        try:
            t_sp = oracle.time_spmv(OA, reps=5, threads=ncores)
            triad = oracle.stream_triad(1 << 27, 4, ncores)
            sp_bytes = 12 * nnz + 20 * n
            spmv_cpu = {"seconds": round(t_sp, 5), "GBps": round(sp_bytes / t_sp / 1e9, 2), "bytes_csr_model": sp_bytes, "threads": ncores,
                        "stream_triad_GBps": round(triad, 1), "frac_of_stream_triad": round(sp_bytes / t_sp / 1e9 / triad, 3) if triad > 0 else None,
                        "sample": "5 repetitions of y = A x (oracle_spmv, OpenMP static rows) on the same CSR; triad over 2^27 doubles, best of 4"}
        except Exception as e:  # noqa: BLE001
            spmv_cpu = {"error": repr(e)}
        cpu_model = "unknown"
        try:
            for ln in open("/proc/cpuinfo"):
                if ln.startswith("model name"):
                    cpu_model = ln.split(":", 1)[1].strip()
                    break
        except OSError:
            pass
        log(f"cpu_baseline: {cpu_its:.2f} it/s with {ncores} threads on {cpu_model}")
        cpu = {
            "value": round(cpu_its, 4), "unit": "iterations/s", "cores": ncores, "kind": "port",
            "sample": f"{len(ho)} AMG-PCG iterations of oracle/amg_oracle.c (OpenMP, {ncores} threads) on the same "
                      f"{n}-row matrix; solve loop only ({sec:.1f} s; oracle setup {t_setup:.1f} s excluded)",
            "gbs": round(it_bytes * cpu_its / 1e9, 1),
            "cpu_model": cpu_model, "host_cpus_visible": os.cpu_count(),
            "reference_default_2_threads": two,
            "spmv": spmv_cpu,
            "hierarchy": (f"{H.nlevels} levels: the reference's coarsening rule continued until <= {prm.limit_upper} rows (the oracle's direct solver is a banded LU, "
                          f"not PARDISO; the device run stops at {levels[-1][0]} rows with {len(levels)} levels and factors that level by nested dissection)"
                          if cpu_levels != len(levels) else f"the device run's {len(levels)} levels"),
            "first_residuals_match_gpu": (bool(np.allclose(ho[: min(len(ho), len(hist))], hist[: min(len(ho), len(hist))], rtol=1e-6))
                                          if cpu_levels == len(levels) else None),
        }

    if True:
        line = {
            "metric": "AMG-PCG solve iterations/sec (7-pt 3D Poisson, fp64) + HBM GB/s (roofline: dominant kernel; config.whole_iteration: the iteration)",
            "value": round(its_per_s, 3),
            "unit": "iterations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "strong" if mode != "replicas" else "weak",
            "failed": True if mode == "replicas" else None,
            "vs_baseline": None,
            "dtype": "f64" if not prm.precond_fp32 else "f64 Krylov loop + f32 preconditioner hierarchy (opt-in mode, not the parity path)",
            "data": "synthetic",
            "config": {
                "workload": f"7-pt 3D Poisson CSR {args.grid}^3 = {n} rows, {nnz} nnz, fp64/int32, AMG-preconditioned CG "
                            f"(HEM aggregation, V({sweeps},{sweeps}) weighted-Jacobi omega=0.66667), b=1, x0=0",
                "levels": [lv[0] for lv in levels],
                "levels_policy": ((f"reference level1=6 EXTENDED by the same coarsening rule until the device direct solver can take over (<= coarse_limit = {prm.coarse_limit} rows"
                                   f"{'' if not prm.extend_until else ', extend_until = ' + str(prm.extend_until)}): {len(levels)} levels, coarsest level {levels[-1][0]} rows, "
                                   f"{coarse['form']} direct solve; the reference itself would hand {levels[5][0] if len(levels) > 5 else levels[-1][0]} rows to PARDISO")
                                  if coarse["extended"] else "the reference's own policy: level1 = 6 levels, the rest to the direct solver"),
                "coarsest_level": coarse,
                # levels whose residual, restriction and the next level's zero-guess sweep are one launch (aggregates = row pairs 2J, 2J+1)
                "paired_restriction_levels": [l for l in range(len(levels) - 1) if A.level_paired(l)],
                # levels whose last post-sweep prolongates into the level above itself (no prolongation launch)
                "fused_prolongation_levels": [l for l in range(len(levels)) if A.level_prolong_fused(l)],
                # box-grid levels whose smoothing legs run two sweeps per launch, with the setup's timings (us per pair of sweeps)
                "double_sweep_levels": ({l: A.level_double_sweep(l) for l in range(len(levels)) if A.level_double_sweep(l)["on"]} if world == 1 else None),
                "single_sweeps_same_process": single_sweeps,
                # box-grid levels whose epilogue-carrying launches (SpMV + dot, last post-sweep, residual + pair restriction) run the plane-marching kernel
                "marching_ops_levels": ({l: A.level_marching_ops(l) for l in range(len(levels)) if A.level_marching_ops(l)["on"]} if world == 1 else None),
                "parallelism": "1 GPU" if world == 1 else (mode_note or (
                    f"{world} GPUs, one process each: contiguous row blocks on the {partitioned_levels} finest levels; deep-halo smoothing "
                    f"(sweeps+1 ghost layers per block, ONE ghost-layer exchange per smoothing leg, grouped ncclSend/ncclRecv of packed "
                    f"buffers: {exchanges_per_step:.1f} transport calls per iteration), 16-byte ncclAllReduce per fused scalar, coarser levels replicated")),
                "transport_calls_per_iteration": round(exchanges_per_step, 2) if mode == "partitioned" else None,
                "hierarchy_setup": (None if mode != "partitioned" else
                                    (lambda bi: f"rank 0 ran the host setup, {bi[1] / 1e6:.0f} MB hierarchy image broadcast to the other ranks (ncclBroadcast)"
                                     if bi[1] > 0 else "every rank ran the host setup itself")(A.setup_share_info())),
                "placement_search": A.placement_info() if world == 1 else None,  # setup-time choice of the finest level's sweep buffers
                "multi_gpu_parity": parity,
                "whole_iteration": whole,
                "csr_model_GB_per_iteration": round(it_bytes / 1e9, 3),
                "csr_model_effective_GBps": round(it_bytes * its_per_s / 1e9, 1),
                "spmv_finest_level": spmv,
                "residual_after_timed_steps": float(last_hist[-1]),
                "solve_restarted_every": RESTART,
                "full_run": args.full,  # --full: the measurements and checks beyond the timed steps ran (null fields otherwise)
                "full_solve_to_1e-8": full,
                "general_values_layout": general,
                "kernel_families": families,
                "reference_level_policy": ref_policy,
                "comm_us": comm_us,
                "comm_schedule": ({"measured": A.comm_measured(), "levels": A.comm_schedule()} if mode == "partitioned" or world > 1 else None),
                "setup_seconds_host": round(A.setup_seconds, 2),
                "generate_seconds": round(t_gen, 2),
            },
            "roofline": roof,
            "cpu_baseline": cpu,
        }

    printed = threading.Event()

    def emit():
        if rank == 0 and not printed.is_set():
            printed.set()
            emitted[0] = True
            sys.stdout.flush()
            os.write(json_fd, (json.dumps(line) + "\n").encode())

    # ---- multi-GPU phase B: the same K timed steps with the halo exchange overlapped with the
    # interior slices (second stream).  This schedule has only been exercised with the in-process
    # test transport, never on xGMI, so it runs under a watchdog: if it hangs, fails the parity
    # check against phase A, or is not faster, the phase-A record above is the one that is printed.
    force_b = os.environ.get("SPARSH_BENCH_FORCE_PHASE_B", "0") == "1"  # exercise this code path on one GPU
    # Off by default since round 2: the partitioned levels run the deep-halo schedule (one exchange per smoothing leg), on
    # which the overlap of a per-sweep exchange has nothing to act; SPARSH_BENCH_DEEP_HALO=0 SPARSH_BENCH_TRY_OVERLAP=1
    # measures the per-sweep-exchange schedule with and without overlap instead.
    if mode == "partitioned" and (world > 1 or force_b) and os.environ.get("SPARSH_BENCH_TRY_OVERLAP", "0") == "1":
        def bail():
            # a hang is a defect to diagnose, not a success: record it, print the phase-A measurement, exit non-zero
            log("overlap phase timed out (hang in the overlapped exchange schedule): reporting the non-overlapped measurement, exit code 4")
            line["config"]["overlap_phase"] = {"timed_out": True, "adopted": False}
            emit()
            os._exit(4)

        dog = threading.Timer(float(os.environ.get("SPARSH_BENCH_OVERLAP_TIMEOUT", "90")), bail)
        dog.daemon = True
        dog.start()
        try:
            import torch

            log("phase B: overlapped halo exchange")
            A.set_overlap(True)
            A.set_stopping(0.0, 100000, 1 << 30)
            A.h2d(xd, np.zeros(nloc))
            A.krylov_init_dev("pcg", bd, xd)
            since_init[0] = 0
            first_segment.clear()
            if args.warmup > 0:
                run_steps(args.warmup)
            if not no_profile:
                A.profile(True)  # same per-launch event overhead as phase A
            barrier()
            tb0 = time.perf_counter()
            done_b = run_steps(args.steps)
            barrier()
            el_b = time.perf_counter() - tb0
            if not no_profile:
                A.profile(False)
            hist_b = first_segment[0] if first_segment else A.krylov_history()
            m = min(len(hist_b), len(hist))
            good = int(done_b == args.steps and m > 0 and np.all(np.isfinite(hist_b)) and
                       float(np.max(np.abs(hist_b[:m] - hist[:m]) / hist[:m])) < 1e-6)
            if dist is not None:
                t = torch.tensor([el_b, -float(good)], device="cuda")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)  # slowest rank's time; any rank's failure
                el_b, good = float(t[0].item()), int(-t[1].item()) == 1
            good = bool(good)
            line["config"]["overlap_phase"] = {"ms_per_step": round(el_b / args.steps * 1e3, 4), "history_matches_phase_a": good,
                                               "adopted": bool(good and el_b < elapsed)}
            line["config"]["non_overlapped_ms_per_step"] = line["ms_per_step"]
            if good and el_b < elapsed:
                line["value"] = round(args.steps / el_b, 3)
                line["ms_per_step"] = round(el_b / args.steps * 1e3, 4)
                line["config"]["csr_model_effective_GBps"] = round(it_bytes * args.steps / el_b / 1e9, 1)
                line["config"]["parallelism"] += "; halo exchange overlapped with the interior slices on a second stream"
        except Exception as e:  # noqa: BLE001
            log(f"overlap phase failed: {e!r}")
            line["config"]["overlap_phase"] = {"error": repr(e), "adopted": False}
        dog.cancel()
    emit()
    if dist_dog is not None:
        dist_dog.cancel()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if mode == "replicas":
        sys.exit(3)  # the multi-GPU metric was not measured: the record says so and the exit code does too


if __name__ == "__main__":
    main()
