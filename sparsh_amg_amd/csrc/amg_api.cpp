// amg_api.cpp -- the drop-in C++ API (include/AMG.hpp of this repo) on top of the C ABI.
// Behaviour mirrored from the reference (file:line relative to the reference tree):
//   sp_matrix / sp_matrix_mg          src/AMG_matrix.cpp:15-68, src/AMG_cpu_matrix.cpp:17-77,203-237
//   readcoo / read_coo_new_format     src/AMG_file_read.cpp:39-185
//   solver entry points + prints      src/AMG_main_solvers.cpp:14-26, 47-167, 240-458
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cctype>
#include <cstring>
#include <fstream>
#include <numeric>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/sparsh_amg.h"
// AMG.hpp defines short macros (omega, th, ...): include it last and only for the declarations
#include "../../include/AMG.hpp"
#include "../../include/AMG_gpu_phases.hpp"
#include "../../include/AMG_gpu_phases_2.hpp"

// ------------------------------------------------------------------------------ containers

sp_matrix::sp_matrix(int r, int c, int n)
{
    nrow = r;
    ncol = c;
    nnz = n;
    rowptr = new int[(size_t)r + 1]();
    colindex = new int[(size_t)(n > 0 ? n : 1)]();
    val = new double[(size_t)(n > 0 ? n : 1)]();
}

sp_matrix::sp_matrix()
{
    nrow = 0;
    ncol = 0;
    nnz = 0;
}

void sp_matrix::check_sp_matrix()
{
    std::cout << "\n Number of Rows: " << nrow;
    std::cout << "\n Number of columns " << ncol;
    std::cout << "\n Number of non-zeros " << nnz;
    std::cout << std::endl;
    for (int i = 0; i < nrow; i++) {
        std::cout << i << std::endl;
        for (int j = rowptr[i]; j < rowptr[i + 1]; j++) std::cout << colindex[j] << "\t" << val[j] << "\t" << std::endl;
        std::cout << std::endl << std::endl;
    }
}

// What mkl_sparse_d_create_csr + mkl_sparse_order did: order the columns of each row in place.
void sp_matrix_mg::sp_matrix_fill()
{
    std::vector<std::pair<int, double>> tmp;
    for (int i = 0; i < nrow; i++) {
        const int s = rowptr[i], e = rowptr[i + 1];
        if (std::is_sorted(colindex + s, colindex + e)) continue;
        tmp.clear();
        for (int j = s; j < e; j++) tmp.emplace_back(colindex[j], val[j]);
        std::stable_sort(tmp.begin(), tmp.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (int j = s; j < e; j++) {
            colindex[j] = tmp[j - s].first;
            val[j] = tmp[j - s].second;
        }
    }
    sA = 0;
    des.type = 20;  // "general"
    // A1 (the MKL handle of the reference) later holds the device mirror the building-block
    // functions create on first use (csrc/blocks_api.cpp)
}

void sp_matrix_mg::sp_matrix_fill_diagonal()
{
    des.type = 20;
    delete[] diagonal;
    delete[] helper;
    diagonal = new double[(size_t)nrow]();
    helper = new double[(size_t)nrow]();
    for (int i = 0; i < nrow; i++) {
        for (int j = rowptr[i]; j < rowptr[i + 1]; j++) {
            if (colindex[j] == i) {
                diagonal[i] = val[j];
                break;
            }
        }
    }
}

// Tolerates the explicit `A->~sp_matrix_mg()` of the reference's main.cpp:40 (pointers are reset).
void sparsh_release_mirror(void *a1);  // blocks_api.cpp

sp_matrix_mg::~sp_matrix_mg()
{
    if (A1) sparsh_release_mirror(A1);
    A1 = nullptr;
    delete[] diagonal;
    delete[] helper;
    delete[] entries;
    delete[] color;
    delete[] color_count;
    diagonal = helper = entries = nullptr;
    color = color_count = nullptr;
}

void sp_matrix_mg::color_matrix_and_reorder()
{
    std::cerr << "sparsh: color_matrix_and_reorder (multi-colour SOR) is not part of the MI355X build" << std::endl;
}

void sp_matrix_mg::normalize_matrix()
{
    std::vector<double> norm1((size_t)ncol, 0.0);
    for (int i = 0; i < nrow; i++)
        for (int j = rowptr[i]; j < rowptr[i + 1]; j++) norm1[colindex[j]] += val[j] * val[j];
    for (int i = 0; i < nrow; i++)
        for (int j = rowptr[i]; j < rowptr[i + 1]; j++) val[j] = val[j] / norm1[colindex[j]];
}

void sp_matrix_mg::scale_system(double *&b)
{
    for (int i = 0; i < nrow; i++) {
        for (int j = rowptr[i]; j < rowptr[i + 1]; j++) val[j] = val[j] / diagonal[i];
        b[i] = b[i] / std::sqrt(diagonal[i]);
    }
}

// ------------------------------------------------------------------------------ readers

// The reference's native text format (src/AMG_file_read.cpp:39-72): "nrow ncol nnz", then nnz triplets "row col val"
// (0-based, sorted by row), and a second file "nrow" + one right-hand-side value per line.  Read here into
// triplet vectors first, then turned into CSR by a count pass and a prefix sum; triplets that are not sorted by
// row are placed correctly too (a stable counting sort), where the reference silently builds a wrong matrix.
void readcoo(char *matrixfile, char *rhsfile, sp_matrix_mg *&A, double *&b)
{
    A = nullptr;
    b = nullptr;
    std::ifstream min(matrixfile);
    if (!min) {
        std::cout << "Cannot open " << matrixfile << std::endl;
        return;
    }
    int nrow = 0, ncol = 0, nnz = 0;
    min >> nrow >> ncol >> nnz;
    if (!min || nrow < 0 || ncol < 0 || nnz < 0) {
        std::cout << matrixfile << ": bad header" << std::endl;
        return;
    }
    std::vector<int> trow((size_t)nnz), tcol((size_t)nnz);
    std::vector<double> tval((size_t)nnz);
    int got = 0;
    while (got < nnz && (min >> trow[got] >> tcol[got] >> tval[got])) ++got;
    if (got != nnz) std::cout << matrixfile << ": " << got << " of " << nnz << " entries read" << std::endl;
    A = new sp_matrix_mg(nrow, ncol, nnz);  // zero-filled (rowptr included)
    for (int e = 0; e < got; ++e)
        if (trow[e] >= 0 && trow[e] < nrow) ++A->rowptr[trow[e] + 1];
    std::partial_sum(A->rowptr, A->rowptr + nrow + 1, A->rowptr);
    std::vector<int> next(A->rowptr, A->rowptr + nrow);
    for (int e = 0; e < got; ++e) {
        if (trow[e] < 0 || trow[e] >= nrow) continue;
        const int at = next[trow[e]]++;
        A->colindex[at] = tcol[e];
        A->val[at] = tval[e];
    }
    b = new double[(size_t)nrow]();
    std::ifstream rin(rhsfile);
    int declared = 0;
    rin >> declared;
    for (int i = 0; i < nrow && (rin >> b[i]); ++i) {
    }
}

bool read_matrix_market(const char *file, sp_matrix_mg *&A)
{
    A = nullptr;
    std::ifstream in(file);
    if (!in) {
        std::cout << "Cannot open " << file << std::endl;
        return false;
    }
    std::string line;
    if (!std::getline(in, line) || line.compare(0, 14, "%%MatrixMarket") != 0) {
        std::cout << file << ": not a MatrixMarket file" << std::endl;
        return false;
    }
    std::string low(line);
    for (char &c : low) c = (char)std::tolower((unsigned char)c);
    if (low.find("coordinate") == std::string::npos || low.find("complex") != std::string::npos) {
        std::cout << file << ": only real / integer / pattern coordinate matrices are supported" << std::endl;
        return false;
    }
    const bool pattern = low.find("pattern") != std::string::npos;
    const bool symmetric = low.find("symmetric") != std::string::npos && low.find("skew") == std::string::npos;
    const bool skew = low.find("skew-symmetric") != std::string::npos;
    while (std::getline(in, line))
        if (!line.empty() && line[0] != '%') break;
    long nrow = 0, ncol = 0, nent = 0;
    {
        std::istringstream hs(line);
        if (!(hs >> nrow >> ncol >> nent) || nrow <= 0 || ncol <= 0 || nent < 0) {
            std::cout << file << ": bad size line" << std::endl;
            return false;
        }
    }
    struct Ent {
        int r, c;
        double v;
    };
    std::vector<Ent> e;
    e.reserve((size_t)nent * ((symmetric || skew) ? 2 : 1));
    for (long k = 0; k < nent; ++k) {
        long r = 0, c = 0;
        double v = 1.0;
        if (!(in >> r >> c) || (!pattern && !(in >> v)) || r < 1 || c < 1 || r > nrow || c > ncol) {
            std::cout << file << ": bad entry " << k + 1 << std::endl;
            return false;
        }
        e.push_back({(int)(r - 1), (int)(c - 1), v});
        if ((symmetric || skew) && r != c) e.push_back({(int)(c - 1), (int)(r - 1), skew ? -v : v});
    }
    std::stable_sort(e.begin(), e.end(), [](const Ent &a, const Ent &b) { return a.r != b.r ? a.r < b.r : a.c < b.c; });
    size_t m = 0;  // sum duplicates in file order
    for (size_t k = 0; k < e.size(); ++k) {
        if (m > 0 && e[m - 1].r == e[k].r && e[m - 1].c == e[k].c)
            e[m - 1].v += e[k].v;
        else
            e[m++] = e[k];
    }
    if (m >= (size_t)1 << 31) {
        std::cout << file << ": more than 2^31 - 1 entries" << std::endl;
        return false;
    }
    A = new sp_matrix_mg((int)nrow, (int)ncol, (int)m);
    for (size_t k = 0; k < m; ++k) {
        A->rowptr[e[k].r + 1]++;
        A->colindex[k] = e[k].c;
        A->val[k] = e[k].v;
    }
    for (long i = 0; i < nrow; ++i) A->rowptr[i + 1] += A->rowptr[i];
    return true;
}

namespace {
const char kBinMagic[8] = {'S', 'P', 'A', 'R', 'S', 'H', 'B', '1'};
}

bool write_csr_binary(const char *file, const sp_matrix_mg &A)
{
    std::ofstream out(file, std::ios::binary);
    if (!out) return false;
    const int nnz = A.rowptr[A.nrow];
    const int hdr[3] = {A.nrow, A.ncol, nnz};
    out.write(kBinMagic, 8);
    out.write(reinterpret_cast<const char *>(hdr), sizeof(hdr));
    out.write(reinterpret_cast<const char *>(A.rowptr), sizeof(int) * ((size_t)A.nrow + 1));
    out.write(reinterpret_cast<const char *>(A.colindex), sizeof(int) * (size_t)nnz);
    out.write(reinterpret_cast<const char *>(A.val), sizeof(double) * (size_t)nnz);
    return (bool)out;
}

bool read_csr_binary(const char *file, sp_matrix_mg *&A)
{
    A = nullptr;
    std::ifstream in(file, std::ios::binary);
    if (!in) {
        std::cout << "Cannot open " << file << std::endl;
        return false;
    }
    char magic[8];
    int hdr[3] = {0, 0, 0};
    in.read(magic, 8);
    in.read(reinterpret_cast<char *>(hdr), sizeof(hdr));
    if (!in || std::memcmp(magic, kBinMagic, 8) != 0 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] < 0) {
        std::cout << file << ": not a sparsh binary CSR file" << std::endl;
        return false;
    }
    sp_matrix_mg *M = new sp_matrix_mg(hdr[0], hdr[1], hdr[2]);
    in.read(reinterpret_cast<char *>(M->rowptr), sizeof(int) * ((size_t)hdr[0] + 1));
    in.read(reinterpret_cast<char *>(M->colindex), sizeof(int) * (size_t)hdr[2]);
    in.read(reinterpret_cast<char *>(M->val), sizeof(double) * (size_t)hdr[2]);
    bool ok = (bool)in && M->rowptr[0] == 0 && M->rowptr[hdr[0]] == hdr[2];
    for (int i = 0; ok && i < hdr[0]; ++i) ok = M->rowptr[i] <= M->rowptr[i + 1];
    for (int k = 0; ok && k < hdr[2]; ++k) ok = M->colindex[k] >= 0 && M->colindex[k] < hdr[1];
    if (!ok) {
        std::cout << file << ": truncated or inconsistent binary CSR file" << std::endl;
        delete M;
        return false;
    }
    A = M;
    return true;
}

void read_coo_new_format(char *matrixfile, sp_matrix_mg *&A, double *&b)
{
    std::ifstream in(matrixfile);
    if (!in) {
        std::cout << "Cannot open " << matrixfile << std::endl;
        A = nullptr;
        b = nullptr;
        return;
    }
    std::string line;
    std::getline(in, line);  // banner: words such as matrix/coordinate/real/general are accepted, not acted on
    std::streampos pos = in.tellg();
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '%') {
            pos = in.tellg();
            continue;
        }
        break;
    }
    in.clear();
    in.seekg(pos);
    int nrow = 0, ncol = 0, nnnz = 0;
    in >> nrow >> ncol >> nnnz;
    A = new sp_matrix_mg(nrow, ncol, nnnz);
    b = new double[(size_t)nrow]();
    for (int i = 0; i < nnnz; i++) {
        int k = 0;
        in >> k >> A->colindex[i] >> A->val[i];  // 0-based, like the reference's reader
        A->rowptr[k + 1]++;
    }
    for (int i = 0; i < nrow; i++) {
        in >> b[i];
        A->rowptr[i + 1] += A->rowptr[i];
    }
}

// ------------------------------------------------------------------------------ solvers

namespace {

double now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Times {
    double setup = 0, solve = 0;
};

// Build the hierarchy, run one method on the device, leave the solution in x.
bool run_device(sp_matrix_mg &A, double *b, double *x, int method, Times &t)
{
    sparsh_handle h = nullptr;
    if (sparsh_create_csr(A.nrow, A.ncol, A.rowptr, A.colindex, A.val, &h) != SPARSH_OK) {
        std::cout << "sparsh: " << sparsh_last_error() << std::endl;
        return false;
    }
    sparsh_params p;
    sparsh_default_params(&p);
    const double t1 = now();
    int rc = sparsh_setup(h, &p);
    const double t2 = now();
    if (rc != SPARSH_OK) {
        std::cout << "sparsh: setup failed: " << sparsh_last_error() << std::endl;
        sparsh_destroy(h);
        if (rc == SPARSH_ENODEV) std::exit(1);  // the reference exits when its backend fails (PARDISO error path)
        return false;
    }
    int iters = 0;
    rc = sparsh_solve(h, method, b, x, nullptr, 0, &iters);
    const double t3 = now();
    if (rc != SPARSH_OK) std::cout << "sparsh: " << sparsh_last_error() << std::endl;
    t.setup = t2 - t1;
    t.solve = t3 - t2;
    sparsh_destroy(h);
    return rc == SPARSH_OK;
}

}  // namespace

void AMG_Solver_CPU_baseline(sp_matrix_mg &A, double *&b, double *&x)
{
    Times t;
    run_device(A, b, x, SPARSH_AMG, t);
    std::cout << "CPU Based Solver Setup Phase Time\t" << t.setup << "\n";
    std::cout << "CPU Based Solver Solve Phase Time\t" << t.solve << "\n";
    std::cout << "CPU Based Solver Total Time\t      " << t.setup + t.solve << "\n";
}

void AMG_Solver_1(sp_matrix_mg &A, double *&b, double *&x) { AMG_Solver_CPU_baseline(A, b, x); }

void AMG_Solver_2(sp_matrix_mg &A, double *&, double *&)
{
    (void)A;
    std::cerr << "sparsh: AMG_Solver_2 (SOR smoother) is not part of the MI355X build; x left unchanged" << std::endl;
}

void coarsening_2(sp_matrix_mg &A, double *&, double *&)
{
    (void)A;
    std::cerr << "sparsh: coarsening_2 (SOR test stub) is not part of the MI355X build" << std::endl;
}

void AMG_Solver_CPU_GPU_CI(sp_matrix_mg &A, double *&b, double *&x)
{
    // The reference's CI variant streams levels over PCIe each cycle to fit small GPUs; with 288 GB
    // of HBM the hierarchy is resident, so CI is the MI engine under its old name.
    Times t;
    run_device(A, b, x, SPARSH_AMG, t);
    std::cout << "Time AMG Hybrid AMG 1\t" << t.setup + t.solve << std::endl;
}

void AMG_Solver_CPU_GPU_MI(sp_matrix_mg &A, double *&b, double *&x)
{
    Times t;
    run_device(A, b, x, SPARSH_AMG, t);
    std::cout << "Time AMG Hybrid AMG 2\t" << t.setup + t.solve << std::endl;
}

#define SPARSH_KRYLOV_ENTRY(NAME, METHOD)                      \
    void NAME(sp_matrix_mg &A, double *&b, double *&x)         \
    {                                                          \
        Times t;                                               \
        run_device(A, b, x, METHOD, t);                        \
    }

SPARSH_KRYLOV_ENTRY(Solver_CG_1, SPARSH_CG)
SPARSH_KRYLOV_ENTRY(Solver_CG_2, SPARSH_CG)
SPARSH_KRYLOV_ENTRY(Solver_PCG_1, SPARSH_PCG)
SPARSH_KRYLOV_ENTRY(Solver_PCG_2, SPARSH_PCG)
SPARSH_KRYLOV_ENTRY(Solver_PCG_3, SPARSH_PCG)
SPARSH_KRYLOV_ENTRY(Solver_PCG_4, SPARSH_PCG)
SPARSH_KRYLOV_ENTRY(Solver_BiCG_1, SPARSH_BICG)
SPARSH_KRYLOV_ENTRY(Solver_PBiCG_1, SPARSH_PBICG)
SPARSH_KRYLOV_ENTRY(Solver_PBiCG_2, SPARSH_PBICG)
SPARSH_KRYLOV_ENTRY(Solver_PBiCG_3, SPARSH_PBICG)
SPARSH_KRYLOV_ENTRY(Solver_PBiCG_4, SPARSH_PBICG)
SPARSH_KRYLOV_ENTRY(Solver_GMRES_1, SPARSH_GMRES)
SPARSH_KRYLOV_ENTRY(Solver_PGMRES_1, SPARSH_PGMRES)
SPARSH_KRYLOV_ENTRY(Solver_FCG_1, SPARSH_FCG)

// ------------------------------------------------------------------------------ solver objects
// AMG_solver / AMG_GPU1_solver / AMG_GPU_solver (include/AMG_phases.hpp, AMG_gpu_phases*.hpp of the
// reference): user code that drives V-cycles itself, as the reference's own Krylov solvers do
// (src/AMG_main_solvers.cpp:129-147: setup once, then AMG_solve_jacobi(r, z, 1) per iteration).

AMG_solver::AMG_solver() {}

void AMG_solver::release()
{
    if (engine_) sparsh_destroy(static_cast<sparsh_handle>(engine_));
    engine_ = nullptr;
    if (Av) {
        for (int q = 1; q <= l; q++) {  // Av[0] is the caller's object
            if (Av[q]) {
                delete[] Av[q]->rowptr;
                delete[] Av[q]->colindex;
                delete[] Av[q]->val;
                delete Av[q];
            }
        }
        delete[] Av;
        Av = nullptr;
    }
    if (Pv) {
        for (int q = 0; q < l; q++) {
            if (Pv[q]) {
                delete[] Pv[q]->rowptr;
                delete[] Pv[q]->colindex;
                delete[] Pv[q]->val;
                delete Pv[q];
            }
        }
        delete[] Pv;
        Pv = nullptr;
    }
    l = 0;
}

AMG_solver::~AMG_solver() { release(); }  // also tolerates the explicit `S->~AMG_solver()` of the reference

void AMG_solver::AMG_solver_setup_jacobi(sp_matrix_mg &A)
{
    release();
    sparsh_handle h = nullptr;
    if (sparsh_create_csr(A.nrow, A.ncol, A.rowptr, A.colindex, A.val, &h) != SPARSH_OK) {
        std::cout << "sparsh: " << sparsh_last_error() << std::endl;
        return;
    }
    sparsh_params p;
    sparsh_default_params(&p);
    const int rc = sparsh_setup(h, &p);
    if (rc != SPARSH_OK) {
        std::cout << "sparsh: setup failed: " << sparsh_last_error() << std::endl;
        sparsh_destroy(h);
        if (rc == SPARSH_ENODEV) std::exit(1);
        return;
    }
    engine_ = h;
    const int nl = sparsh_num_levels(h);
    l = nl - 1;
    Av = new sp_matrix_mg *[nl]();
    Pv = new sp_matrix_mg *[nl > 1 ? nl - 1 : 1]();
    Av[0] = &A;
    for (int q = 0; q < nl; q++) {
        int nrow = 0, nnz = 0, pn = 0, pnnz = 0;
        sparsh_level_info(h, q, &nrow, &nnz, &pn, &pnnz);
        if (q > 0) {
            Av[q] = new sp_matrix_mg(nrow, nrow, nnz);
            sparsh_level_csr(h, q, 0, Av[q]->rowptr, Av[q]->colindex, Av[q]->val);
            Av[q]->sp_matrix_fill_diagonal();
        }
        if (q < l) {
            Pv[q] = new sp_matrix_mg(nrow, pn, pnnz);
            sparsh_level_csr(h, q, 1, Pv[q]->rowptr, Pv[q]->colindex, Pv[q]->val);
        }
    }
}

void AMG_solver::AMG_solver_setup_SOR(sp_matrix_mg &)
{
    std::cerr << "sparsh: AMG_solver_setup_SOR (SOR smoother) is not part of the MI355X build" << std::endl;
}

void AMG_solver::AMG_solve_jacobi(double *&b, double *&x, int iterations)
{
    if (!engine_) {
        std::cout << "sparsh: AMG_solve_jacobi called before AMG_solver_setup_jacobi" << std::endl;
        return;
    }
    int cycles = 0;
    if (sparsh_vcycle(static_cast<sparsh_handle>(engine_), b, x, iterations, nullptr, 0, &cycles) != SPARSH_OK)
        std::cout << "sparsh: " << sparsh_last_error() << std::endl;
}

void AMG_solver::AMG_solve_SOR(double *&, double *&, int)
{
    std::cerr << "sparsh: AMG_solve_SOR (SOR smoother) is not part of the MI355X build; x left unchanged" << std::endl;
}

void AMG_GPU1_solver::GPU_Allocations() {}

void AMG_GPU1_solver::helper(double *b, double *x, int iterations) { AMG_solve_jacobi(b, x, iterations); }

void AMG_GPU1_solver::AMG_Solve(double *b, double *x, int iterations)
{
    if (!engine_) {
        std::cout << "sparsh: AMG_Solve called before AMG_solver_setup_jacobi" << std::endl;
        return;
    }
    int cycles = 0;
    if (sparsh_vcycle_dev(static_cast<sparsh_handle>(engine_), b, x, iterations, nullptr, 0, &cycles) != SPARSH_OK)
        std::cout << "sparsh: " << sparsh_last_error() << std::endl;
}

void AMG_GPU_solver::GPU_Allocations() {}

void AMG_GPU_solver::AMG_GPU_solve(double *b, double *x, int iterations) { AMG_solve_jacobi(b, x, iterations); }

void AMG_GPU_solver::AMG_GPU_solve_1(double *b, double *x, int iterations)
{
    if (!engine_) {
        std::cout << "sparsh: AMG_GPU_solve_1 called before AMG_solver_setup_jacobi" << std::endl;
        return;
    }
    int cycles = 0;
    if (sparsh_vcycle_dev(static_cast<sparsh_handle>(engine_), b, x, iterations, nullptr, 0, &cycles) != SPARSH_OK)
        std::cout << "sparsh: " << sparsh_last_error() << std::endl;
}
