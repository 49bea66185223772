#!/usr/bin/env python3
"""Every candidate launch plan of the box-grid kernels on each box level of an n^3 hierarchy, timed alone (run ON the GPU box).

usage: box_plan_sweep.py [n = 216] [reps = 200]
First the plans the default setup chose (Engine::tune_box_kernels) with its own timings, then, on a handle with both kernels switched
on everywhere, the candidates of box_plan_candidates for each level and kernel through bench_op: the double sweep ping-ponging on the
level's resident buffers (us per launch = per pair of sweeps) and the last post-sweep + dot of the marching kernel (us per launch), the
smaller of two runs of `reps` launches.  '*' marks the fastest plan of a level, 'p' the planner's.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

n = int(sys.argv[1]) if len(sys.argv) > 1 else 216
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rp, ci, v = problems.poisson3d(n)
quiet = sa.default_params(print_setup=0, print_solve=0)

A = sa.sp_matrix_mg(rp, ci, v).setup(quiet)
print(f"# Box-grid levels of the default {n}^3 hierarchy: the plans the setup chose (threads Q TY CZ) and what it measured, us")
print("level  grid              double sweep: threads Q TY CZ   two singles  one double | marching: threads Q TY CZ   table  marching")
for l in range(A.nlevels - 1):
    d2, d1 = A.level_double_sweep(l), A.level_marching_ops(l)
    if d2["grid"][0] <= 0:
        continue
    t2, t1 = A.level_box_threads(l)
    p2 = f"{t2:4d} {d2['points_per_thread']} {d2['lines_per_tile']:2d} {d2['planes_per_chunk']:2d}" if d2["on"] else "   -  -  -  -"
    p1 = f"{t1:4d} {d1['points_per_thread']} {d1['lines_per_tile']:2d} {d1['planes_per_chunk']:2d}" if d1["on"] else "   -  -  -  -"
    print(f"{l:5d}  {str(d2['grid']):17s}               {p2}   {d2['two_single_sweeps_us']:11.2f} {d2['double_sweep_us']:11.2f} |"
          f"           {p1}   {d1['table_kernel_us']:6.2f} {d1['marching_kernel_us']:9.2f}")
A.close()

A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(quiet)
print(f"# Candidates timed alone ({reps} launches, smaller of two runs); two single sweeps of the table kernel for comparison")
print("level  grid              kernel    threads Q TY CZ  workgroups      us")
for l in range(A.nlevels - 1):
    d2 = A.level_double_sweep(l)
    grid = d2["grid"]
    if grid[0] <= 0 or not d2["on"]:
        continue
    singles = 2e6 * min(A.bench_op("jacobi_pingpong_resident", l, reps) for _ in range(2))
    print(f"{l:5d}  {str(grid):17s} table     two single sweeps {singles:24.2f}")
    for kernel, op in ((2, "jacobi_double"), (1, "jacobi_dot_marching")):
        if kernel == 1 and not A.level_marching_ops(l)["on"]:
            continue
        rows = []
        for i, (threads, q, ty, cz) in enumerate(sa.box_plan_candidates(kernel, *grid)):
            try:
                A.set_box_plan(l, kernel, q, ty, cz, threads=threads)
            except sa.SparshError:  # (more marching workgroups than the partial buffers of this handle hold)
                continue
            us = 1e6 * min(A.bench_op(op, l, reps) for _ in range(2))
            rows.append((us, i == 0, threads, q, ty, cz))
        A.set_box_plan(l, kernel)
        best = min(r[0] for r in rows)
        for us, planner, threads, q, ty, cz in rows:
            wgs = -(-grid[1] // ty) * -(-grid[2] // cz)
            mark = ("*" if us == best else " ") + ("p" if planner else " ")
            print(f"{l:5d}  {str(grid):17s} {'double' if kernel == 2 else 'marching':9s} {threads:5d} {q} {ty:2d} {cz:3d}  {wgs:10d} {us:9.2f} {mark}", flush=True)
A.close()
