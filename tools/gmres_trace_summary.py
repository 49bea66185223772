#!/usr/bin/env python3
"""Per-step times of the GMRES orthogonalisation kernels from a rocprofv3 kernel trace of ONE pgmres solve:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/config_bench.py GMRES_poisson3d_216 \\
      --methods=pgmres --reps=1 --no-orth-ab
  python tools/gmres_trace_summary.py <dir> <rows>
Walks the dispatches in start order.  j = gmres_step_kernel launches since the last gmres_solve_kernel (a restart cycle's end);
the launches between two step kernels belong to step j: gs_dot (sums of all its chunks), the update with dots, the update
without.  Bytes: gs_dot 8 n (j + 2) per pass over the basis, an update 8 n (j + 3); a chunked step (more than 16 vectors) reads and
writes w once more per extra launch, which the model leaves out.  The yardstick is dot_kernel (16 n bytes) in the same trace."""
import csv
import glob
import os
import sys
from collections import defaultdict


def main():
    d, n = sys.argv[1], int(sys.argv[2])
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under " + d)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    j = 0
    step = defaultdict(lambda: defaultdict(list))  # j -> kind -> [us per step]
    cur = defaultdict(float)
    dots = []
    for r in rows:
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        if "gs_dot_kernel" in name:
            cur["gs_dot"] += us
        elif "gs_update_kernel" in name:
            cur["gs_update_dot" if "true" in name or "Lb1" in name else "gs_update"] += us
        elif "gs_scale_kernel" in name:
            cur["gs_scale"] += us
        elif "gmres_step_kernel" in name:
            cur["gmres_step"] += us
        elif "gs_finalize_kernel" in name:
            cur["gs_finalize"] += us
        elif "gmres_solve_kernel" in name:
            j = 0
            cur.clear()
            continue
        elif "dot_kernel" in name and "spmv" not in name.lower() and n > 0 and "dot2" not in name and "cvt" not in name:
            dots.append(us)
            continue
        else:
            continue
        if "gs_scale_kernel" in name and "gmres_step" in cur:  # the step's last launch
            for k, v in cur.items():
                step[j][k].append(v)
            cur.clear()
            j += 1
    gb = 8.0 * n * 1e-9
    if dots:
        dots.sort()
        med = dots[len(dots) // 2]
        print(f"dot_kernel: {len(dots)} launches, median {med:.1f} us, min {dots[0]:.1f}, max {dots[-1]:.1f}; {2 * gb / (med * 1e-6) / 1e3:.2f} TB/s on 16 n bytes")
    print("j  steps  gs_dot us (TB/s)  gs_update_dot us (TB/s)  gs_update us (TB/s)  finalize+step+scale us")
    for jj in sorted(step):
        s = step[jj]
        avg = lambda k: sum(s[k]) / len(s[k]) if s[k] else 0.0
        # a step of nv = j + 1 <= 16 vectors: one gs_dot, one update with dots, one without; above: two gs_dot passes and two plain updates
        fused = jj + 1 <= 16
        dot_bytes = (1 if fused else 2) * gb * (jj + 2)
        upd_bytes = gb * (jj + 3)
        rate = lambda b, us: b / (us * 1e-6) / 1e3 if us > 0 else 0.0
        small = avg("gs_finalize") + avg("gmres_step") + avg("gs_scale")
        print(f"{jj:2d} {len(s['gmres_step']):3d}   {avg('gs_dot'):8.1f} ({rate(dot_bytes, avg('gs_dot')):.2f})   "
              f"{avg('gs_update_dot'):8.1f} ({rate(upd_bytes, avg('gs_update_dot')):.2f})   "
              f"{avg('gs_update'):8.1f} ({rate((1 if fused else 2) * upd_bytes, avg('gs_update')):.2f})   {small:8.1f}")


if __name__ == "__main__":
    main()
