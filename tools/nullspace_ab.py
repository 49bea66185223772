"""Cost of the constant-null-space projection on the device.

    python tools/nullspace_ab.py [--grid 216] [--rounds 5] [--reps 200] [--out FILE]

Two handles in one process: the pure Neumann 7-point Poisson problem on grid^3 set up under SPARSH_NULLSPACE_CONSTANT, and the
Dirichlet problem of the same size under the default (the benchmark's operator) as the yardstick.  After one warm-up round the
measurements alternate, --rounds times:
  - sparsh_bench_op 18 on the Neumann handle: one launch_sum + launch_project pair with the dot on level 0's resident x and r
    (HIP events around --reps back-to-back pairs), against its byte model of 5 vector passes (40 bytes per row) at the 6.29 TB/s
    copy rate measured for this device; 4 of them are memory streams of the two launches (the sum reads x; the projection reads
    x and r and writes x);
  - one AMG-PCG solve of a consistent system on the Neumann handle (HIP-event time of sparsh_solve_dev over its iterations);
  - one AMG-PCG solve on the Dirichlet handle.
Reported: every round's figures, their medians, and which kernel family and box-grid path the finest level of each handle took.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sparsh_amg_amd as sa  # noqa: E402
from sparsh_amg_amd import problems  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, the project's measured device copy rate


class Handle:
    def __init__(self, name, csr, nullspace):
        rp, ci, v = csr
        self.name, self.n = name, len(rp) - 1
        self.keep = (rp, ci, v)  # the handle aliases the arrays
        self.A = sa.sp_matrix_mg(rp, ci, v).set_nullspace(nullspace).setup(sa.default_params(print_setup=0, print_solve=0))
        S = sp.csr_matrix((v, ci, rp), shape=(self.n, self.n))
        xt = np.random.default_rng(7).standard_normal(self.n)
        xt -= xt.mean()
        self.b = S @ xt
        self.bd, self.xd = self.A.dev_alloc(self.n * 8), self.A.dev_alloc(self.n * 8)
        self.A.h2d(self.bd, self.b)

    def layout(self):
        A = self.A
        ds = A.level_double_sweep(0)
        return (f"{self.name}: {A.nlevels} levels, level 0 kernel {A.level_kernel(0)}, format {A.level_format(0)}, "
                f"double sweep {ds}, marching ops {A.level_marching_ops(0)}, null space {A.nullspace_info()}")

    def pcg(self):
        self.A.dev_fill(self.xd, self.n, 0.0)
        hist, iters, sec, rc = self.A.solve_dev("pcg", self.bd, self.xd)
        if rc != sa.SPARSH_OK:
            raise RuntimeError(f"{self.name}: pcg returned {rc}")
        return iters, sec, hist[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if sa.device_count() < 1:
        raise SystemExit("nullspace_ab.py measures on the device: no GPU visible")
    g = args.grid
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    neu = Handle(f"neumann {g}^3, CONSTANT", problems.poisson3d_neumann(g), "constant")
    dirichlet = Handle(f"dirichlet {g}^3, NONE", problems.poisson3d(g), "none")
    say(neu.layout())
    say(dirichlet.layout())
    n = neu.n
    model_us = 5 * 8 * n / COPY_RATE * 1e6
    say(f"projection byte model: 5 vector passes of {n} rows = {5 * 8 * n / 1e6:.0f} MB = {model_us:.1f} us at {COPY_RATE / 1e12:.2f} TB/s")
    say(f"(of the 5 passes the two launches issue 4 as memory streams -- the sum reads x; the projection reads x and r and writes x: "
        f"{4 * 8 * n / 1e6:.0f} MB = {4 * 8 * n / COPY_RATE * 1e6:.1f} us -- and the second read of x can hit the Infinity Cache)")
    rows = []
    for rnd in range(args.rounds + 1):
        proj_us = neu.A.bench_op("project_dot", 0, args.reps) * 1e6
        it_n, sec_n, res_n = neu.pcg()
        it_d, sec_d, res_d = dirichlet.pcg()
        tag = "warm-up" if rnd == 0 else f"round {rnd}"
        say(f"{tag}: projection + dot {proj_us:.1f} us ({model_us / proj_us:.2f} of the byte model's rate) | neumann pcg {it_n} iterations, "
            f"{sec_n * 1e3 / it_n:.3f} ms/iteration, ||r|| {res_n:.2e} | dirichlet pcg {it_d} iterations, {sec_d * 1e3 / it_d:.3f} ms/iteration, "
            f"||r|| {res_d:.2e}")
        if rnd > 0:
            rows.append((proj_us, sec_n * 1e3 / it_n, sec_d * 1e3 / it_d))
    med = [statistics.median(c) for c in zip(*rows)]
    say(f"medians of {args.rounds} rounds: projection + dot {med[0]:.1f} us (byte model {model_us:.1f} us), neumann CONSTANT pcg {med[1]:.3f} ms/iteration, "
        f"dirichlet NONE pcg {med[2]:.3f} ms/iteration")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
