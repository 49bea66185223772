"""A program written against the reference's API, as its main.cpp is, must compile and link against
this repo's headers and library (drop-in boundary): tests/cpp/dropin_driver.cpp makes
main.cpp's calls in main.cpp's order.  Running it needs a GPU (tests/test_gpu_c0.py), so this CPU
test stops at the link step and checks that every C++ entry point of include/AMG.hpp is exported."""
import os

import numpy as np
import re
import subprocess

from conftest import ROOT

LIB_DIR = os.path.join(ROOT, "sparsh_amg_amd")
ENTRY_POINTS = [
    "readcoo", "read_coo_new_format", "AMG_Solver_CPU_baseline", "AMG_Solver_1", "AMG_Solver_2", "Solver_CG_1",
    "Solver_CG_2", "Solver_PCG_1", "Solver_PCG_2", "Solver_PCG_3", "Solver_PCG_4", "AMG_Solver_CPU_GPU_CI",
    "AMG_Solver_CPU_GPU_MI", "Solver_BiCG_1", "Solver_PBiCG_1", "Solver_PBiCG_2", "Solver_PBiCG_3", "Solver_PBiCG_4",
    "coarsening_2",
]


def test_cpp_entry_points_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", "-C", os.path.join(LIB_DIR, "libsparsh_amg.so")], text=True)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bT {name}\(", out), name
    for cls in ("AMG_solver::AMG_solver_setup_jacobi(sp_matrix_mg&)", "AMG_solver::AMG_solve_jacobi(double*&, double*&, int)",
                "AMG_GPU1_solver::AMG_Solve(double*, double*, int)", "AMG_GPU1_solver::helper(double*, double*, int)",
                "AMG_GPU_solver::AMG_GPU_solve(double*, double*, int)", "sp_matrix_gpu::sp_matrix_gpu(sp_matrix_mg&)",
                "sp_matrix_gpu::smooth_jacobi(double*, double*, double*, ihipStream_t*, int)", "gpu_swap_pointers(sp_matrix_gpu*&, sp_matrix_gpu*&)"):
        assert cls in out, cls
    for cls in ("sp_matrix::sp_matrix(int, int, int)", "sp_matrix_mg::sp_matrix_fill()", "sp_matrix_mg::sp_matrix_fill_diagonal()",
                "sp_matrix_mg::~sp_matrix_mg()", "sp_matrix_mg::scale_system(double*&)", "sp_matrix_mg::normalize_matrix()"):
        assert cls in out, cls
    # operator-level building blocks (AMG_smoothers / AMG_cycle_utilities / AMG_coarsening / AMG_coarse_level_solver)
    for fn in ("parallel::jacobi_smoother(sp_matrix_mg&, double*&, double*&, int)", "sequential::jacobi_smoother(sp_matrix_mg&, double*&, double*&, int)",
               "parallel::residual(sp_matrix_mg&, double*&, double*&)", "parallel::transfer_residual(sp_matrix_mg&, double*&, double*&)",
               "parallel::transfer_solution(sp_matrix_mg&, double*&, double*&)", "parallel::store_residual(sp_matrix_mg&, double*&, double*&, double*&)",
               "parallel::coarsen_matrix(sp_matrix_mg&, sp_matrix_mg*&, sp_matrix_mg&)", "sequential::HEM_Prolongator(sp_matrix_mg&, sp_matrix_mg*&, int)",
               "sequential::beck_prolongator(sp_matrix_mg&, sp_matrix_mg*&)", "Direct_Solver_Pardiso::Direct_Solver_Pardiso(sp_matrix_mg&)",
               "Direct_Solver_Pardiso::Direct_Solver_Pardiso_solve(double*&, double*&)"):
        assert fn in out, fn


def test_host_building_blocks_without_gpu(tmp_path):
    """The host-side building blocks (HEM / Beck / Galerkin coarsen_matrix) need no GPU; the device ones
    must refuse loudly when no HIP device is visible (no CPU fallback)."""
    src = tmp_path / "hb.cpp"
    src.write_text(r'''
#include "AMG.hpp"
#include "AMG_coarsening.hpp"
#include "AMG_cycle_utilities.hpp"
#include "AMG_smoothers.hpp"
#include <cstdio>
#include <cstring>
int main(int argc, char **argv)
{
    const int n = 6;  // 1D Laplacian
    sp_matrix_mg *A = new sp_matrix_mg(n, n, 3 * n - 2);
    int k = 0;
    for (int i = 0; i < n; i++) {
        A->rowptr[i] = k;
        if (i > 0) { A->colindex[k] = i - 1; A->val[k++] = -1.0; }
        A->colindex[k] = i; A->val[k++] = 2.0;
        if (i < n - 1) { A->colindex[k] = i + 1; A->val[k++] = -1.0; }
    }
    A->rowptr[n] = k;
    A->sp_matrix_fill();
    A->sp_matrix_fill_diagonal();
    sp_matrix_mg *P = nullptr, *Ac = nullptr;
    sequential::HEM_Prolongator(*A, P, 0);
    sequential::coarsen_matrix(*A, Ac, *P);
    std::printf("HB %d %d %d %d", P->nrow, P->ncol, Ac->nrow, Ac->rowptr[Ac->nrow]);
    for (int i = 0; i < Ac->nrow; i++) std::printf(" %g", Ac->diagonal[i]);
    std::printf("\n");
    std::fflush(stdout);
    if (argc > 1 && !std::strcmp(argv[1], "dev")) {
        double b[n] = {1, 1, 1, 1, 1, 1}, x[n] = {0};
        double *bp = b, *xp = x;
        parallel::jacobi_smoother(*A, bp, xp, 2);
        std::printf("SMOOTHED %g\n", x[0]);
    }
    return 0;
}
''')
    exe = tmp_path / "hb"
    cmd = ["g++", "-std=c++17", "-O1", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe),
           f"-L{LIB_DIR}", "-lsparsh_amg", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib/llvm/lib",
           "-L/opt/rocm/lib", "-L/opt/rocm/lib/llvm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-1000:])
    # pairs (0,1) (2,3) (4,5): Ac = tridiag(-1, 2, -1) of order 3 with explicit structure
    assert r.stdout.strip() == "HB 6 3 3 7 2 2 2", r.stdout
    # ask the product's own HIP runtime: torch ships a second copy, and once that one has opened the GPU, the product's
    # runtime sees no device for the rest of this process (every later GPU test in the same pytest run would fail)
    import sparsh_amg_amd as sa
    if sa.device_count() < 1:
        r = subprocess.run([str(exe), "dev"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "SMOOTHED" not in r.stdout and "no HIP device" in r.stdout


def test_dropin_driver_compiles_and_links(tmp_path):
    main_cpp = os.path.join(ROOT, "tests", "cpp", "dropin_driver.cpp")
    exe = tmp_path / "main"
    cmd = ["g++", "-std=c++17", "-O1", f"-I{os.path.join(ROOT, 'include')}", main_cpp, "-o", str(exe),
           f"-L{LIB_DIR}", "-lsparsh_amg", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib/llvm/lib",
           "-L/opt/rocm/lib", "-L/opt/rocm/lib/llvm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert exe.exists()


def test_readcoo_roundtrip(tmp_path):
    """C++ readcoo (through a tiny driver) and the Python reader agree on a generated file."""
    import numpy as np

    import sparsh_amg_amd as sa
    from sparsh_amg_amd import problems

    rp, ci, v = problems.poisson2d(12)
    b = np.arange(len(rp) - 1, dtype=float) * 0.5 + 1
    mf, rf = str(tmp_path / "m.txt"), str(tmp_path / "r.txt")
    problems.write_coo(mf, rf, rp, ci, v, b)
    A, b2 = sa.readcoo(mf, rf)
    assert np.array_equal(A.rowptr, rp) and np.array_equal(A.colindex, ci) and np.array_equal(A.val, v) and np.array_equal(b2, b)
    drv = tmp_path / "drv.cpp"
    drv.write_text(
        '#include "AMG.hpp"\n#include <cstdio>\n'
        "int main(int, char** argv){ sp_matrix_mg* A; double* b; readcoo(argv[1], argv[2], A, b);\n"
        " A->sp_matrix_fill(); A->sp_matrix_fill_diagonal();\n"
        ' std::printf("%d %d %d %.17g %.17g %d\\n", A->nrow, A->ncol, A->rowptr[A->nrow], A->diagonal[3], b[5], A->colindex[7]);\n'
        " A->~sp_matrix_mg(); delete[] b; return 0; }\n"
    )
    exe = tmp_path / "drv"
    cmd = ["g++", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}", str(drv), "-o", str(exe), f"-L{LIB_DIR}", "-lsparsh_amg",
           f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib/llvm/lib", "-L/opt/rocm/lib", "-L/opt/rocm/lib/llvm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.check_output([str(exe), mf, rf], text=True).split()
    assert int(out[0]) == len(rp) - 1 and int(out[2]) == rp[-1]
    assert float(out[3]) == 4.0 and float(out[4]) == b[5] and int(out[5]) == ci[7]


def test_matrix_market_reader_and_binary_cache(tmp_path):
    """read_matrix_market (1-based, comments, symmetric expansion, unordered entries, duplicates summed,
    pattern) and the binary CSR cache round trip -- host code, no GPU."""
    import scipy.io
    import scipy.sparse as sp

    rng = np.random.default_rng(4)
    n = 37
    B = sp.random(n, n, density=0.15, random_state=5, format="coo")
    S = (B + B.T + sp.identity(n) * 3.0).tocoo()
    gen = tmp_path / "general.mtx"
    sym = tmp_path / "symmetric.mtx"
    scipy.io.mmwrite(str(gen), B.tocoo(), comment="general, unordered")
    scipy.io.mmwrite(str(sym), sp.tril(S).tocoo(), symmetry="symmetric")
    dup = tmp_path / "dups.mtx"
    dup.write_text("%%MatrixMarket matrix coordinate real general\n% duplicates are summed\n3 3 5\n3 1 2.0\n1 1 1.0\n3 1 0.5\n2 2 4.0\n1 3 -1.0\n")
    pat = tmp_path / "pattern.mtx"
    pat.write_text("%%MatrixMarket matrix coordinate pattern symmetric\n3 3 3\n1 1\n3 1\n2 2\n")
    src = tmp_path / "mm.cpp"
    src.write_text(r'''
#include "AMG.hpp"
#include <cstdio>
static void dump(const char *tag, sp_matrix_mg *A)
{
    std::printf("%s %d %d %d", tag, A->nrow, A->ncol, A->rowptr[A->nrow]);
    double s = 0; long cs = 0;
    for (int i = 0; i < A->nrow; i++)
        for (int j = A->rowptr[i]; j < A->rowptr[i + 1]; j++) { s += A->val[j] * (i + 1) * (A->colindex[j] + 2); cs += A->colindex[j]; if (j > A->rowptr[i] && A->colindex[j] <= A->colindex[j - 1]) cs = -1000000; }
    std::printf(" %.15g %ld\n", s, cs);
}
int main(int argc, char **argv)
{
    sp_matrix_mg *A = nullptr, *B = nullptr;
    for (int k = 1; k <= 4; k++) {
        if (!read_matrix_market(argv[k], A)) return 10 + k;
        dump(argv[k], A);
        if (k == 2) {
            if (!write_csr_binary(argv[5], *A) || !read_csr_binary(argv[5], B)) return 20;
            dump("binary", B);
            delete B;
        }
        delete A;
    }
    if (read_matrix_market(argv[5], A) || A != nullptr) return 30;  // not a MatrixMarket file
    if (read_csr_binary(argv[1], A) || A != nullptr) return 31;     // not a binary file
    return 0;
}
''')
    exe = tmp_path / "mm"
    cmd = ["g++", "-std=c++17", "-O1", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe),
           f"-L{LIB_DIR}", "-lsparsh_amg", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib/llvm/lib",
           "-L/opt/rocm/lib", "-L/opt/rocm/lib/llvm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), str(gen), str(sym), str(dup), str(pat), str(tmp_path / "cache.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)

    def expect(M):
        M = sp.csr_matrix(M)
        M.sum_duplicates()
        M.sort_indices()
        rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
        return M.shape[0], M.shape[1], M.nnz, float(np.sum(M.data * (rows + 1) * (M.indices + 2))), int(M.indices.sum())

    lines = [ln.split() for ln in r.stdout.strip().splitlines() if len(ln.split()) == 6]
    got = {os.path.basename(t[0]): (int(t[1]), int(t[2]), int(t[3]), float(t[4]), int(t[5])) for t in lines}
    D = sp.coo_matrix(([2.0, 1.0, 0.5, 4.0, -1.0], ([2, 0, 2, 1, 0], [0, 0, 0, 1, 2])), shape=(3, 3))
    P = sp.coo_matrix(([1.0, 1.0, 1.0, 1.0], ([0, 2, 0, 1], [0, 0, 2, 1])), shape=(3, 3))
    for name, M in (("general.mtx", B), ("symmetric.mtx", S), ("binary", S), ("dups.mtx", D), ("pattern.mtx", P)):
        e = expect(M)
        g = got[name]
        assert g[:3] == e[:3] and g[4] == e[4] and abs(g[3] - e[3]) <= 1e-12 * max(1.0, abs(e[3])), (name, g, e)
