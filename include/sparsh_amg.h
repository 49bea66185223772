/*
 * sparsh_amg.h -- C ABI of libsparsh_amg.so: the MI355X-native AMG solve phase.
 *
 * The reference (cmgcds/SParSH-AMG) has no C ABI or plugin interface; its boundary is the
 * C++ source-level API of include/AMG.hpp (17 free functions on sp_matrix_mg, statically
 * linked).  That C++ surface is re-exported by this library through include/AMG.hpp,
 * include/AMG_matrix.hpp and include/AMG_cpu_matrix.hpp of THIS repo (same names, same
 * signatures), so the reference's main.cpp links against libsparsh_amg.so unchanged.
 *
 * This header is the plain-C mirror a non-C++ host (ctypes, cgo, JNI ...) binds: plain
 * pointers and sizes, int return codes, no globals.  Each entry cites the reference
 * interface it stands for (file:line relative to the reference tree).
 *
 * Conventions: 0-based CSR, int32 indices, fp64 values, caller-owned host buffers unless a
 * name ends in _dev (device pointers in HBM of the handle's GPU).  Return 0 on success,
 * negative SPARSH_E* otherwise; sparsh_last_error() gives the text.
 */
#ifndef SPARSH_AMG_H_
#define SPARSH_AMG_H_

#ifdef __cplusplus
extern "C" {
#endif

#define SPARSH_OK 0
#define SPARSH_EINVAL -1    /* bad argument */
#define SPARSH_ENODEV -2    /* no HIP device / HIP runtime error (on the solve path: sticky until the next sparsh_setup) */
#define SPARSH_ESTATE -3    /* call order violated (e.g. solve before setup) */
#define SPARSH_ENUMERIC -4  /* singular coarse matrix, NaN residual */
#define SPARSH_ENOCONV -5   /* iteration cap reached before ||r|| <= tol (x still returned) */
#define SPARSH_ECOMM -6     /* transport (RCCL) failure on the solve path; sticky until the next sparsh_setup */

/* Solver selection: which reference entry point's arithmetic is followed. */
#define SPARSH_AMG 0    /* AMG_Solver_CPU_baseline / _CPU_GPU_MI / _CPU_GPU_CI  (src/AMG_main_solvers.cpp:14-26,240-268) */
#define SPARSH_CG 1     /* Solver_CG_1 / Solver_CG_2        (src/AMG_main_solvers.cpp:47-103, .cu:35-139)  */
#define SPARSH_PCG 2    /* Solver_PCG_1..4                  (src/AMG_main_solvers.cpp:107-167, .cu:269-413) */
#define SPARSH_BICG 3   /* Solver_BiCG_1                    (src/AMG_main_solvers.cpp:271-355) */
#define SPARSH_PBICG 4  /* Solver_PBiCG_1..4                (src/AMG_main_solvers.cpp:358-458) */
#define SPARSH_GMRES 5  /* restarted GMRES without a preconditioner (sparsh_set_gmres) */
#define SPARSH_PGMRES 6 /* restarted GMRES, right-preconditioned with one V-cycle from a zero guess: the z = M v of SPARSH_PBICG */
#define SPARSH_FCG 7    /* flexible preconditioned CG (Notay's FCG(1)): the Krylov method that takes the K-cycle; see "W- and K-cycles" below */
#define SPARSH_BCG 8    /* block conjugate gradients: sparsh_solve_multi / sparsh_solve_multi_dev only; see "block CG" below */
#define SPARSH_MBICG 10 /* block BiCGStab (unsymmetric systems): sparsh_solve_multi / sparsh_solve_multi_dev only; see "block BiCGStab" below.
                         * 9 is no method and stays SPARSH_EINVAL everywhere */

/* Smoother of the V-cycle (sparsh_set_smoother). */
#define SPARSH_SMOOTH_JACOBI 0  /* weighted Jacobi, parallel::jacobi_smoother (default) */
#define SPARSH_SMOOTH_SOR 1     /* multicolour SOR, parallel::sor_smoother (src/AMG_smoothers.cpp:78-102) */
#define SPARSH_SMOOTH_CHEBYSHEV 3 /* Chebyshev polynomial in D^-1 A (see "Chebyshev polynomial smoother" below); 2 is no smoother and
                                   * stays SPARSH_EINVAL, as sparsh_set_smoother has always reported it */
#define SPARSH_SOR_FORWARD 0    /* post-smoothing takes the colours 1..C, as AMG_solve_SOR (src/AMG_phases.cpp:234-306) */
#define SPARSH_SOR_SYMMETRIC 1  /* post-smoothing takes the colours C..1: a symmetric preconditioner (required by SPARSH_PCG) */

/* Runtime form of the compile-time macros of the reference's include/AMG.hpp:15-27.
 * sparsh_default_params() fills the reference values; the env variables in brackets
 * override them inside sparsh_default_params(). */
typedef struct sparsh_params {
    double omega;       /* omega = 0.66667 (not 2/3)                          [SPARSH_OMEGA]   */
    double tol;         /* tol1 = 1e-8, absolute ||b-Ax||_2                   [SPARSH_TOL]     */
    int sweeps;         /* Jacobi sweeps per smoothing step. CPU path of the reference does
                           smooth_iter+1 = 7 (src/AMG_smoothers.cpp:59-60); its GPU path 6. [SPARSH_NU] */
    int max_levels;     /* level1 = 6                                          [SPARSH_LEVELS]  */
    int limit_upper;    /* limit_upper = 4000                                                  */
    int limit_lower;    /* limit_lower = 2000                                                  */
    int coarsening;     /* 0 = HEM pairwise aggregation (default, src/AMG_phases.cpp:60),
                           1 = Beck (src/AMG_phases.cpp:63)                    [SPARSH_COARSENING=hem|beck] */
    int max_iter;       /* guard the reference lacks: cap on cycles/iterations [SPARSH_MAXIT]   */
    int coarse_limit;   /* largest coarsest level max_levels may leave for the device direct solver
                           (default 40000: up to ~1.3 M rows the hierarchy is exactly the reference's,
                           src/AMG_phases.cpp:51,77,89).  If max_levels would leave more, coarsening
                           continues by the same rule until <= extend_until rows (documented deviation
                           from the reference, which hands any size to PARDISO; 1<<30 disables it).
                                                                               [SPARSH_COARSE_LIMIT] */
    int host_threads;   /* OpenMP threads for the host setup (0 = all)        [SPARSH_THREADS] */
    int device;         /* HIP device ordinal (-1 = current / LOCAL_RANK)                     */
    int print_setup;    /* print_setup_phase_details = 1                       [SPARSH_PRINT]   */
    int print_solve;    /* print_solve_phase_details = 1                       [SPARSH_PRINT]   */
    int check_every;    /* Krylov/AMG loops read the residual norm back every k iterations
                           (1 = reference behaviour: every iteration)                          */
    int use_graph;      /* capture one V-cycle into a hipGraph and replay it   [SPARSH_GRAPH]   */
    int replicate_rows; /* multi-GPU: levels with at most this many rows are held and computed by every
                           rank (no halo exchange below that size).  0 (default): chosen at setup from the measured
                           transport, see sparsh_set_comm_tuning (1 500 000 when that is off) [SPARSH_REPLICATE_ROWS] */
    int precond_fp32;   /* 0 (default): everything fp64, bitwise parity with the reference's arithmetic.
                           1: SPARSH_PCG / SPARSH_PBICG run their V-cycle on a float copy of the hierarchy (float values
                           and vectors: the sliced-diagonal value blocks where a level has that layout, the
                           CSR values otherwise; one GPU) while
                           the CG recurrences, residuals and the stopping test stay fp64.  Not a parity
                           mode: a different (cheaper) preconditioner, same solution to tol.
                                                                               [SPARSH_PRECOND_FP32] */
    int dense_limit;    /* coarsest levels up to this many rows are solved with an explicit dense inverse
                           (one GEMV per V-cycle); larger ones with the block-tridiagonal factorisation of
                           the RCM-ordered operator, factored and applied on the device (csrc/coarse.cpp).
                           Default 8192.                                       [SPARSH_DENSE_LIMIT] */
    int extend_until;   /* where a hierarchy that had to be extended past max_levels (see coarse_limit) stops:
                           0 (default) = at the first level of at most coarse_limit rows, i.e. as soon as the
                           device direct solver can take over -- the closest to the reference's "6 levels, then
                           a direct solve" that fits; > 0 = at the first level of at most that many rows
                           (4000 = limit_upper: round 2's behaviour, 13 levels at 10 M rows).
                                                                               [SPARSH_EXTEND_UNTIL] */
    int coarse_factor_mb; /* the reference's own coarsest level (what max_levels leaves) is kept, whatever its row count, while the
                           ESTIMATED size of its nested-dissection factors stays below this many MB (one breadth-first search gives
                           the graph's effective dimension: ~ n log n bytes for 2D-like operators, ~ n^(4/3) for 3D-like ones).
                           Default 1024: a 9 M-row 2D problem keeps the reference's 6 levels (281 250-row direct solve, 0.5 GB),
                           136^3 does (78 608 rows, 0.4 GB), 216^3 does not (314 928 rows, 2.4 GB: extended).  0: coarse_limit
                           alone decides.                                      [SPARSH_COARSE_FACTOR_MB] */
} sparsh_params;

typedef struct sparsh_handle_s *sparsh_handle;

const char *sparsh_last_error(void);
int sparsh_version(void);
int sparsh_device_count(void);
int sparsh_host_cpus(void); /* CPUs this process may use (affinity mask and cgroup quota) */

void sparsh_default_params(sparsh_params *p);

/* sp_matrix_mg + sp_matrix_fill + sp_matrix_fill_diagonal (include/AMG_cpu_matrix.hpp:12-51,
 * src/AMG_cpu_matrix.cpp:17-51): register a host CSR.  The arrays are aliased, not copied
 * (as AMG_solver::Av[0] aliases the caller's matrix, src/AMG_phases.cpp:40) and must
 * outlive the handle.  Columns must be sorted within each row. */
int sparsh_create_csr(int nrow, int ncol, const int *rowptr, const int *colindex, const double *val, sparsh_handle *out);
void sparsh_destroy(sparsh_handle h);

/* AMG_solver::AMG_solver_setup_jacobi (src/AMG_phases.cpp:35-90) followed by what
 * AMG_GPU1_solver::GPU_Allocations does (src/AMG_gpu_phases_2.cu:13-94): build the hierarchy
 * on the host, factor the coarsest level, upload everything to HBM (resident). */
int sparsh_setup(sparsh_handle h, const sparsh_params *p);

/* Change the stopping rule of an already set-up handle (tol1 of include/AMG.hpp:18; iteration
 * cap; how often the residual norm is read back).  max_iter/check_every <= 0 keep their value. */
int sparsh_set_stopping(sparsh_handle h, double tol, int max_iter, int check_every);

/* Per-handle choice of the SpMV-type kernel family (A/B measurements; all families produce
 * bitwise identical results; nothing here is process-wide state).  kind: 0 workgroup CSR-stream, 1 wave CSR-stream, 2 sliced-ELL mirror,
 * 3 sliced-diagonal mirror (default); 2 and 3 fall back (3 -> 2 -> 0) where the operator does not
 * qualify for the mirror; vec (CSR-stream kernels): 0 one entry per load, 1 paired 16-B/8-B loads in the stream phase,
 * 2 col/val staged in LDS with the x gathers issued in row-lane order (csr_rowlane_kernel), 3 (default) = 2 for operators
 * that stream from HBM, 1 for cache-resident ones, 4 = 2 with 16-bit delta-coded column indices (csr_rowlane16_kernel) where the
 * operator carries them (sparsh_set_index_compression); nt: non-temporal loads for the matrix stream; remap: 0 none, 1 each XCD owns a
 * contiguous eighth of the row blocks, G > 1 groups of G row blocks dealt round-robin to the XCDs.
 * nt < 0 or remap < 0 selects the built-in per-operator policy (default). */
int sparsh_set_kernel_config(sparsh_handle h, int kind, int vec, int nt, int remap);

/* Which layout the SpMV-type kernels of a level use under the current config (3 sliced diagonals,
 * 2 sliced ELL, 1 wave CSR-stream, 0 workgroup CSR-stream) and how many entries it stores
 * (padding included). */
int sparsh_level_format(sparsh_handle h, int level, int *kind, long *stored_entries);

/* Sliced-diagonal layout of a level: number of (slice, diagonal) slots and how many of them own a
 * 64-value block.  A slot whose present entries all carry the same value ("constant slot":
 * constant-coefficient stencils and their aggregated coarse operators) keeps that value once in
 * its header and owns no block; the arithmetic is unchanged (same products, same order).  Slices
 * made of at most 8 constant slots are described by one fixed-stride 192-byte record (offsets,
 * lane masks, constants, count) the kernel fetches with a single batch of scalar loads; when
 * (nearly) all of them draw their (offset, constant) pairs from one set of at most 8, that set
 * travels as a kernel argument and a slice only needs its 8 lane masks (64 B).
 * meta_bytes = bytes of slice/slot descriptors one sweep reads.  All 0 when the level does not use
 * the layout.  sparsh_set_const_slots(h, 0) before sparsh_setup(h, ...) turns the folding off for that
 * handle (A/B measurements; default on). */
int sparsh_level_layout(sparsh_handle h, int level, long *slots, long *value_blocks, long *meta_bytes);
int sparsh_set_const_slots(sparsh_handle h, int enable);
/* Compressed column indices for the CSR-stream family: per row block of the workgroup kernel the indices
 * are also kept as 16-bit deltas (first entry of a row relative to the block's smallest first column, every further entry
 * relative to the previous column of its row), 10 instead of 12 bytes per stored entry; blocks a delta does not fit (a gap
 * of 65536 or more, an unsorted row, a single row longer than the LDS buffer) keep the 32-bit indices.  Same products, same
 * order of additions: results are bitwise those of the other families.  mode, read by sparsh_setup: 0 never build the form,
 * 1 (default) for operators the default policy streams from HBM through the CSR-stream kernel (> 240 MB, no sliced mirror),
 * 2 for every operator (A/B measurements with sparsh_set_kernel_config(h, 0, 4, ...)).
 * sparsh_level_index16: how many row blocks of a level's operator use the 16-bit form, out of how many. */
int sparsh_set_index_compression(sparsh_handle h, int mode);
/* Consecutive Jacobi sweeps of a smoothing leg may walk the level's row blocks in alternating directions: a sweep then starts
 * on the part of the vectors the previous one touched last, which is still in the memory-side cache.  Placement only -- every
 * row is computed exactly as before.  mode 0: always ascending; 1 (default): alternate where one sweep streams more than
 * 640 MB = 2.5x the Infinity Cache (matrix-streaming layouts of large levels: -3...6 % per sweep; smaller levels and the
 * value-free table path measured neutral within +-1 %); 2: always alternate (A/B). */
int sparsh_set_alternate_sweeps(sparsh_handle h, int mode);
/* On a lexicographically ordered grid the aggregation (HEM, src/AMG_coarsening.cpp) joins rows 2J and 2J+1 on most
 * levels.  There the residual kernel of the table path hands each row's residual to the lane next door, adds the pair in the
 * order transfer_residual does and writes the coarse right-hand side and the coarse level's zero-guess sweep directly: the
 * level's residual vector is neither written nor read back and one launch replaces two (parallel::store_residual +
 * parallel::transfer_residual, src/AMG_cycle_utilities.cpp:115-123 and :97-104).  Same expressions in the same order --
 * results are bitwise unchanged.  enable: 1 (default) / 0 (A/B).
 * Box-grid levels (sparsh_level_double_sweep) whose aggregates pair a grid point with its neighbour one line or one plane up get the
 * same fusion from a kernel of their own: one thread per aggregate computes both residuals from the seven-point stencil; neither r nor
 * R is touched.
 * sparsh_level_paired: whether a level of the built hierarchy takes this path under the current configuration: 0 no, 1 row pairs
 * (2J, 2J+1), 2 / 3 box-grid level paired along y / z. */
int sparsh_set_paired_restriction(sparsh_handle h, int enable);
/* Up-leg: with an aggregation prolongator every fine row has exactly one coarse owner, so the last post-smoothing sweep of
 * level l can add its result to the rows of level l - 1 it owns (x_f = 1.0 * x_c + x_f, parallel::transfer_solution,
 * src/AMG_cycle_utilities.cpp:107-112) instead of storing it for a prolongation launch: one launch and one pass over the
 * coarse iterate less per level.  Used where the aggregates hold one or two rows (pairwise matching), on one GPU.  Same
 * expressions -- results are bitwise unchanged.  enable: 1 (default) / 0 (A/B).
 * sparsh_level_prolong_fused: whether level `level`'s last post-sweep prolongates into level - 1 itself: 0 no, 1 yes with
 * the aggregates being the row pairs (2J, 2J+1) (no index read), 2 yes through an 8-byte (first, second) record per aggregate. */
int sparsh_set_fused_prolongation(sparsh_handle h, int enable);
/* Levels whose diagonal is one constant (constant-coefficient stencils and their Galerkin products): the kernels that only
 * divide by d_i -- the zero-guess sweeps x = omega b / d (parallel::jacobi_smoother's first pass, src/AMG_smoothers.cpp:53-76)
 * fused into the PCG update and into the restriction -- take the constant as an argument instead of streaming diag[]
 * (8 of 64 bytes per row of the PCG update).  Same division, same bits.  enable: 1 (default) / 0 (A/B).
 * sparsh_level_constant_diagonal: whether a level of the built hierarchy qualifies under the current configuration, and the value. */
int sparsh_set_constant_diagonal(sparsh_handle h, int enable);
/* Double sweep.  A level whose operator is the 7-point stencil of an nx x ny x nz box grid in lexicographic order (constant
 * coefficients; the finest levels of BASELINE configs[1]'s 3D cases and their Galerkin products) can run two sweeps of
 * parallel::jacobi_smoother (src/AMG_smoothers.cpp:53-76) in one pass over x, b and the result: a workgroup marches through
 * the planes of its tile with the first sweep's plane in LDS, so that sweep's result is never written (temporal blocking;
 * ~30 instead of 48 bytes per row and pair of sweeps).  Every row is computed with the same products in the same order:
 * results are bitwise those of two single sweeps.  mode, read by sparsh_setup: 0 never; 1 (default) on levels of >= 400 000 rows
 * where the setup times it faster than two single sweeps; 2 on every box-grid level that has a launch plan (tests, A/B).
 * After setup the mode may be switched between 0 and its setup value.
 * sparsh_level_double_sweep: on = the level's smoothing legs use it; dims = {nx, ny, nz} (0: not a box grid); plan = {points per
 * thread, lines per tile, planes per chunk}; the setup's timings of two single sweeps / one double sweep in us (0: not timed).
 * Any output pointer may be NULL. */
int sparsh_set_double_sweep(sparsh_handle h, int mode);
/* The launches of a box-grid level that carry an epilogue of their own -- A p with the p.Ap dot (Solver_PCG's mv + cublasDdot,
 * src/AMG_main_solvers.cu), the last post-sweep with the z.r dot or with the prolongation, the residual with the pair restriction --
 * through the same plane-marching scheme with one stencil application per launch (sdia_box1_kernel): x of the current plane in LDS,
 * its neighbours in z in registers, so every x is read once instead of being gathered by seven rows.  The vectors it stores are
 * bitwise the table kernel's; its fused dot products are summed per workgroup of this kernel rather than per 256 rows -- same
 * terms, another order of additions, i.e. a difference in the last bits of a reduction (within the 1e-12 the parity tests hold
 * reductions to).  mode as for the double sweep (0 / 1 timed at setup, default / 2 forced).  sparsh_level_marching_ops: on, plan =
 * {points per thread, lines per tile, planes per chunk}, the setup's timing of the last post-sweep + dot through the table kernel
 * and through this one (us, 0: not timed). */
int sparsh_set_marching_ops(sparsh_handle h, int mode);
/* Double-sweep levels: a smoothing leg that starts from a zero guess (every down-leg below the finest level, and the finest level's
 * inside PCG) runs its first THREE sweeps as one launch: the matrix-free first sweep x = omega b / d (parallel::jacobi_smoother from
 * x = 0) is evaluated where the double sweep would load its input, from the right-hand side the two stencil stages read anyway, so
 * the iterate is not read at all (16 instead of 31 bytes per row for that launch).  Bitwise the three separate sweeps.
 * enable: 1 (default) / 0 (A/B). */
int sparsh_set_zero_start(sparsh_handle h, int enable);
/* PCG (Solver_PCG_*, src/AMG_main_solvers.cu): x += alpha p is applied by the kernel that updates the search direction at the end of
 * the same iteration instead of by the one that updates the residual -- nothing reads x in between and p is then read once for both
 * updates (one n-vector stream less per iteration).  Same expressions, same bits.  enable: 1 (default) / 0 (A/B). */
int sparsh_set_deferred_x(sparsh_handle h, int enable);
int sparsh_level_marching_ops(sparsh_handle h, int level, int *on, int *plan, double *table_us, double *marching_us);
/* Test hook: the launch plan {points per thread q, lines per tile ty, planes per chunk cz} of a box-grid level's double sweep
 * (kernel 2) or plane-marching kernel (kernel 1) instead of the planner's; (0, 0, 0) restores the planner's plan (box_planner,
 * csrc/box_plan.cpp), kernel 3 with (0, 0, 0) takes the marching kernel's shared-CU plan without timing it.  SPARSH_EINVAL for a level that
 * is not a box grid and for a plan the kernel cannot run: q outside {2, 3, 4}, ty outside 1 .. ny, cz outside 1 .. nz, a tile region
 * ((ty + 4) nx points for kernel 2, (ty + 2) nx for kernel 1) larger than q 1024 threads cover or than 64 KiB of LDS, a marching
 * launch with more workgroups than the reduction buffers hold.  Does not switch a kernel on (sparsh_set_double_sweep /
 * sparsh_set_marching_ops); drops a captured graph.  sparsh_level_double_sweep / sparsh_level_marching_ops report the plan in force. */
int sparsh_set_box_plan(sparsh_handle h, int level, int kernel, int q, int ty, int cz);
/* The same with the workgroup size as a fourth dimension of the plan: threads = 256, 512 or 1024 (anything else: SPARSH_EINVAL), and the
 * tile region must fit q * threads points.  sparsh_set_box_plan is this call with threads = 1024; (q, ty, cz) = (0, 0, 0) restores the
 * planner's plan on 1024 threads whatever `threads` says. */
int sparsh_set_box_plan_ex(sparsh_handle h, int level, int kernel, int threads, int q, int ty, int cz);
/* Threads per workgroup of the plans in force on a box-grid level (0 where the kernel has no plan): the setup's timing may have chosen
 * 256 or 512 (levels of >= 60 000 rows under the default modes of sparsh_set_double_sweep / sparsh_set_marching_ops). */
int sparsh_level_box_threads(sparsh_handle h, int level, int *double_threads, int *marching_threads);
/* Debug entry (no handle, no device): the launch plans the setup would time for kernel 2 / 1 on an nx x ny x nz box, {threads, q, ty, cz}
 * each, the planner's first; part_cap > 0 bounds the marching kernel's workgroups.  Writes at most cap plans, returns their number
 * (-1: bad kernel). */
int sparsh_debug_box_plan_candidates(int kernel, int nx, int ny, int nz, int part_cap, int cap, int *plans);
/* Box-grid levels whose six off-diagonal stencil constants are each 0 or +-2^k, k >= 0 (every level of a constant-coefficient
 * Laplacian on a uniform grid under pairwise aggregation: -1, -2, -4, ...): the box kernels (double sweep and plane-marching kernel)
 * evaluate the off-diagonal terms of their stencil sums as one FMA each.  c x is exact for such c unless it overflows, so the FMA
 * rounds what sum + c x rounds: the same bits wherever the unfused result is finite, six fp64 instructions fewer per point and stage.
 * The rule is decided once at setup from the coefficients alone.  mode: 1 (default) where the rule holds / 0 never (A/B); may be
 * called before or after setup, drops a captured graph. */
int sparsh_set_box_exact_fma(sparsh_handle h, int mode);
/* on: the level is a box grid and its box kernels run the FMA instances under the current mode; rule: its constants satisfy the rule. */
int sparsh_level_box_exact_fma(sparsh_handle h, int level, int *on, int *rule);
/* Debug entry (no handle, no device): the rule on seven stencil constants (-plane, -line, -1, diagonal, +1, +line, +plane; the
 * diagonal is not looked at).  1 / 0. */
int sparsh_debug_box_exact_offdiag(const double *c);
int sparsh_level_double_sweep(sparsh_handle h, int level, int *on, int *dims, int *plan, double *single_us, double *double_us);
int sparsh_level_constant_diagonal(sparsh_handle h, int level, int *is_const, double *value);
int sparsh_level_prolong_fused(sparsh_handle h, int level, int *fused);
int sparsh_level_paired(sparsh_handle h, int level, int *paired);
/* PCG: the x / r update kernel also writes the zero-guess sweep z0 = omega r / d of the V-cycle that follows (same bits, one
 * read of r and one launch less), and streams x, p, Ap and d past the caches (non-temporal loads / stores) so that r and z0,
 * which the cycle's first sweep reads next, are what stays resident.  mode 2 (default): both; 1: fused, ordinary loads;
 * 0: separate launch (A/B). */
int sparsh_set_fused_zero_sweep(sparsh_handle h, int mode);
/* Placement search (single GPU, stencil-table levels whose three sweep vectors together are about the size of the 256 MB
 * Infinity Cache): sparsh_setup times the finest-level sweep on candidate triples among the equally sized buffers the
 * engine owns anyway (plus five spares, freed again) until one runs cache-resident, at most 260 triples (~0.1 s), and lets
 * the fastest triple hold iterate / ping-pong twin / Krylov residual -- the same sweep takes 44 to
 * 63 us depending on the physical pages behind the three vectors.  Pointers only: no extra memory, identical results.
 * sparsh_set_placement_search(h, 0) before sparsh_setup keeps the allocation order (A/B).  sparsh_placement_info: sweep time
 * of the chosen, the worst and the initial triple in microseconds, the number of triples timed (0: search not run) and the
 * seconds the search took. */
int sparsh_set_placement_search(sparsh_handle h, int enable);
int sparsh_placement_info(sparsh_handle h, double *chosen_us, double *worst_us, double *initial_us, int *triples, double *seconds);
/* Multi-GPU setup: by default rank 0 alone runs the host setup (coarsening, Galerkin products, coarse factor) and the other
 * ranks receive the finished hierarchy through the transport (one RCCL broadcast of its byte image, staged through HBM in
 * 256 MB pieces) instead of repeating the identical setup N times; every rank then cuts out and uploads its own row
 * blocks as before.  sparsh_set_setup_broadcast(h, 0) before sparsh_setup: every rank builds its own copy (round-1
 * behaviour; the hierarchies are identical either way -- the setup is deterministic).  Collective: all ranks must use
 * the same setting.  sparsh_setup_share_info: whether this rank built the hierarchy itself, and the image size in bytes
 * (0 when nothing was broadcast). */
int sparsh_set_setup_broadcast(sparsh_handle h, int enable);
int sparsh_setup_share_info(sparsh_handle h, int *built_locally, long *image_bytes);
/* Test hook (host only, after sparsh_setup_host): writes the byte image, reads it back (only the first truncate_to bytes when
 * truncate_to >= 0) and compares every array of the two hierarchies; returns the image size or a negative SPARSH_E*. */
long sparsh_debug_hierarchy_roundtrip(sparsh_handle h, long truncate_to);
int sparsh_level_index16(sparsh_handle h, int level, long *blocks16, long *blocks);
/* Test hook (host only, no handle): builds the row-block schedule and the 16-bit delta form of a CSR pattern, decodes it again
 * and compares with colindex; reports how many row blocks took the 16-bit form. */
int sparsh_debug_index16_roundtrip(int nrow, const int *rowptr, const int *colindex, long *blocks16, long *blocks);
/* Table levels of grid stencils (offsets -1, 0, +1, +-line[, +-plane]) run, on whole-level launches, a
 * variant that stages x[r0 - line, r0 + T + line) of every workgroup's T rows in LDS, so the centre, +-1 and
 * +-line neighbours come out of LDS and only the +-plane neighbours are gathered from L2 (bitwise the same
 * results).  sparsh_set_tile(h, 0) switches it off for the handle (A/B measurements; default on);
 * sparsh_level_tile_rows reports T for a level (0: the variant is not used there). */
int sparsh_set_tile(sparsh_handle h, int enable);
int sparsh_level_tile_rows(sparsh_handle h, int level, int *rows);
/* Multi-GPU diagnostics (collective: every rank calls it with the same arguments): average seconds
 * of one communication step alone, timed with HIP events on the engine's stream.  what = 0: halo
 * exchange of level `level`'s operator; 1: the 16-byte all-reduce of the fused scalars; 2: the
 * all-gather at the partitioned -> replicated boundary.  *avg_seconds = -1 when there is no such
 * step (single GPU, replicated level). */
int sparsh_bench_comm(sparsh_handle h, int what, int level, int reps, double *avg_seconds);
/* name of the kernel the SpMV-type operations of a level launch under the current config
 * ("sdia_tab_kernel", "sdia_kernel", "sell_kernel", "csr_wave_kernel", "csr_block_kernel") */
const char *sparsh_level_kernel(sparsh_handle h, int level);
/* placement the launcher uses for that level's operator under the handle's config: nt = 1 when the
 * matrix stream is read with non-temporal loads, remap = XCD mapping mode (see sparsh_set_kernel_config) */
int sparsh_level_placement(sparsh_handle h, int level, int *nt, int *remap);

/* Host half of sparsh_setup only (coarsening, Galerkin products, coarse factorisation); needs
 * no GPU.  Enables the inspection calls below; solvers still require sparsh_setup. */
int sparsh_setup_host(sparsh_handle h, const sparsh_params *p);

/* hierarchy inspection (tests; "Level k:\t nrow" lines of src/AMG_phases.cpp:55-58) */
int sparsh_num_levels(sparsh_handle h);
int sparsh_level_info(sparsh_handle h, int level, int *nrow, int *nnz, int *p_ncol, int *p_nnz);
/* which: 0 = A_level, 1 = P_level, 2 = R_level = P_level^T as the restriction kernels read it (rows = coarse rows, entries in ascending
 * fine-row order); 1 and 2 on level < last.  Buffers sized from sparsh_level_info (R: p_ncol rows, p_nnz entries). */
int sparsh_level_csr(sparsh_handle h, int level, int which, int *rowptr, int *colindex, double *val);
/* explicit inverse of the coarsest operator, row-major nL x nL (what the device GEMV applies in
 * place of Direct_Solver_Pardiso_solve); available after sparsh_setup_host when the coarsest level
 * has at most dense_limit rows */
int sparsh_coarse_inverse(sparsh_handle h, double *inv);
/* form of the coarsest-level direct solver: info6 = {rows, dense (1) or factored on the device (0), block size,
 * number of blocks, RCM bandwidth, hierarchy extended past max_levels (1/0)}; *bytes = HBM held by the
 * factors.  After sparsh_setup (block fields are 0 unless the block-tridiagonal form is in use). */
int sparsh_coarse_info(sparsh_handle h, int *info6, long *bytes);
/* Which direct solver a coarsest level above dense_limit rows gets (both replace Direct_Solver_Pardiso,
 * src/AMG_coarse_level_solver.cpp:9-76); call before sparsh_setup.
 *   form 0 (default): nested-dissection multifrontal factorisation -- the operator's graph is dissected recursively, every
 *     tree node's pivot block is inverted explicitly and its couplings to the ancestors are kept as dense blocks; a solve is
 *     one launch per tree level upwards and one downwards (csrc/nd_plan.cpp, nd_solver.cpp, nd_kernels.hip).
 *   form 1: block-tridiagonal factorisation of the RCM-ordered operator (csrc/coarse.cpp), ~ n / bandwidth dependent steps.
 * leaf > 0: largest subgraph kept as one dense block (default 64); merge_rows >= 0: separators of successive bisections are
 * eliminated as one pivot block while their total stays below this (default 384; 0 = plain bisection).
 * sparsh_coarse_nd_info: info6 = {nested dissection in use (1/0), tree nodes, tree levels, largest pivot block,
 * launches per solve, leaf size}. */
int sparsh_set_coarse_form(sparsh_handle h, int form, int leaf, int merge_rows);
/* the same cap for the nodes near the root of the dissection tree: top_merge_rows for the root, halved per tree depth until it
 * meets merge_rows (default 2048; 0 = merge_rows everywhere).  Near the root a tree level holds 1, 2, 4 ... nodes and costs two
 * dependent launches per solve whatever it holds. */
int sparsh_set_coarse_top_merge(sparsh_handle h, int top_merge_rows);
int sparsh_coarse_nd_info(sparsh_handle h, int *info6);
/* Pivoting of the device factorisation, counted by the inversion kernels during sparsh_setup: out4 = {pivot steps, steps whose
 * pivot row was not the diagonal row} of the one-workgroup LDS inversions (nested dissection, pivot blocks of at most 80 rows), then
 * the same pair for the one-launch-per-step inversions (nested dissection: larger pivot blocks; block tridiagonal: every diagonal
 * block).  All zero for the dense form and before sparsh_setup. */
int sparsh_coarse_pivot_info(sparsh_handle h, int *out4);
/* Interface form of the block-tridiagonal solve: where the RCM band is narrow against the block (2 * window <= block,
 * window = bandwidth rounded up to 64) only the first / last `window` rows of a block couple to its neighbours, so the
 * chain of dependent steps runs on those rows alone (products S_i^-1 A[i,neighbour] kept in HBM) and everything else is
 * two whole-level launches; the chain itself -- an affine recurrence with constant W x W matrices -- is unrolled at setup
 * into block-triangular matrices, so each of its two passes is ONE triangular matrix-vector product (while those matrices
 * stay under 1 GiB; otherwise one launch per chain step).  *window = 0 when the solver does not use the form.
 * sparsh_set_coarse_interface(h, mode) before sparsh_setup: 0 keeps the plain chain of B x B steps, 1 (default) as
 * described, 2 the interface form with one launch per chain step (A/B measurements). */
int sparsh_coarse_window(sparsh_handle h, int *window);
int sparsh_set_coarse_interface(sparsh_handle h, int enable);
/* Block size of the block-tridiagonal coarse factorisation: rows > 0 before sparsh_setup replaces the built-in rule
 * (rounded up to 64 and never below the RCM bandwidth); 0 restores the rule.  A/B measurements. */
int sparsh_set_coarse_block(sparsh_handle h, int rows);
double sparsh_setup_seconds(sparsh_handle h);

/* AMG_solver::AMG_solve_jacobi(b, x, iterations) (src/AMG_phases.cpp:151-230) ==
 * AMG_GPU1_solver::helper (src/AMG_gpu_phases_2.cu:242-263): host b/x, V-cycles on the device.
 * iterations > 0: exactly that many cycles; -1: until ||Ax-b|| <= tol.
 * hist[k] = residual after cycle k+1 (the value the reference prints). */
int sparsh_vcycle(sparsh_handle h, const double *b, double *x, int iterations, double *hist, int hist_cap, int *ncycles);

/* Same with b/x already in HBM: AMG_GPU1_solver::AMG_Solve (src/AMG_gpu_phases_2.cu:96-240). */
int sparsh_vcycle_dev(sparsh_handle h, const double *b_dev, double *x_dev, int iterations, double *hist, int hist_cap, int *ncycles);

/* The 17 solver entry points of include/AMG.hpp:40-85 reduce to five methods (SPARSH_*).
 * x: initial guess in, solution out.  hist[k] = residual the reference prints at step k. */
int sparsh_solve(sparsh_handle h, int method, const double *b, double *x, double *hist, int hist_cap, int *iters);

/* Same with b/x already in HBM (AMG_GPU1_solver::AMG_Solve / Solver_PCG_4 inner loop,
 * src/AMG_gpu_phases_2.cu:96-240, src/AMG_main_solvers.cu:269-413).  max_iters bounds the
 * loop (<=0: params.max_iter); *seconds returns the loop time measured with HIP events on the
 * engine's stream (NULL to skip). */
int sparsh_solve_dev(sparsh_handle h, int method, const double *b_dev, double *x_dev, int max_iters, double *hist, int hist_cap, int *iters, double *seconds);

/* Stepwise form of the CG / AMG-PCG loop: init = everything before the reference's while loop
 * (src/AMG_main_solvers.cpp:124-133), step = nsteps passes of the loop body (:136-159), stopping
 * early only when ||r|| <= tol.  Lets a caller time exactly k iterations.  *residual = last
 * ||r|| read back; history = residual after each iteration so far. */
int sparsh_krylov_init_dev(sparsh_handle h, int method, const double *b_dev, double *x_dev);
int sparsh_krylov_step_dev(sparsh_handle h, int nsteps, int *done, double *residual);
int sparsh_krylov_history(sparsh_handle h, double *hist, int hist_cap, int *iters);

/* ---- operator-level entry points (kernel parity tests, roofline measurement) ----
 * Host vectors in/out; each runs exactly one device operator of the given level.
 *   spmv      : y = A_l x                      mkl_sparse_d_mv / cusparseDcsrmv (src/AMG_gpu_phase_utilities.cu:143)
 *   jacobi    : sweeps x { x += omega (b - A_l x)/d }   parallel::jacobi_smoother (src/AMG_smoothers.cpp:53-76)
 *   residual  : r = b - A_l x                  parallel::store_residual (src/AMG_cycle_utilities.cpp:115-123)
 *   resnorm   : ||A_l x - b||_2                parallel::residual (src/AMG_cycle_utilities.cpp:83-94)
 *   restrict  : b_{l+1} = P_l^T r              parallel::transfer_residual (src/AMG_cycle_utilities.cpp:97-104)
 *   prolong   : x_l += P_l x_{l+1}             parallel::transfer_solution (src/AMG_cycle_utilities.cpp:107-112)
 *   coarse    : x_L = A_L^{-1} b_L             Direct_Solver_Pardiso_solve (src/AMG_coarse_level_solver.cpp:64-76)
 *   dot/nrm2/axpby : cublasDdot / cublasDnrm2 / daxpby kernel (src/AMG_main_solvers.cu:17-24)
 */
int sparsh_op_spmv(sparsh_handle h, int level, const double *x, double *y);
int sparsh_op_jacobi(sparsh_handle h, int level, const double *b, double *x, int sweeps, int x_is_zero);
int sparsh_op_residual(sparsh_handle h, int level, const double *b, const double *x, double *r);
int sparsh_op_resnorm(sparsh_handle h, int level, const double *b, const double *x, double *nrm);
int sparsh_op_restrict(sparsh_handle h, int level, const double *r, double *bc);
/* levels sparsh_level_paired reports: bc = P_l^T (b - A_l x) and xc = omega bc / d_{l+1} from the one fused launch the
 * V-cycle uses there (store_residual + transfer_residual + the coarse level's first sweep from a zero guess) */
int sparsh_op_residual_restrict(sparsh_handle h, int level, const double *b, const double *x, double *bc, double *xc);
int sparsh_op_prolong(sparsh_handle h, int level, const double *xc, double *xf);
/* levels sparsh_level_prolong_fused reports: xf (level - 1, in/out) += P_{level-1} J(x), J = one Jacobi sweep of `level`
 * from x with right-hand side b -- the one launch the V-cycle's up-leg uses there */
int sparsh_op_jacobi_prolong(sparsh_handle h, int level, const double *b, const double *x, double *xf);
/* the launches with a fused dot product, as PCG and the V-cycle's last post-sweep run them on the level (table or plane-marching
 * kernel, then the same final reduction): y = A_l x and *dot = x.y; y = one Jacobi sweep of x and *dot = y.b */
int sparsh_op_spmv_dot(sparsh_handle h, int level, const double *x, double *y, double *dot);
int sparsh_op_jacobi_dot(sparsh_handle h, int level, const double *b, const double *x, double *y, double *dot);
int sparsh_op_coarse(sparsh_handle h, const double *b, double *x);
/* z = V32(r): one application of the opt-in fp32 preconditioner (params.precond_fp32 = 1): a V(nu,nu) cycle from a
 * zero guess on the float copy of the hierarchy, fp64 in/out.  Checked against oracle_vcycle_f32. */
int sparsh_op_precond_f32(sparsh_handle h, const double *r, double *z);
/* The steps sparsh_op_precond_f32's cycle is made of, one at a time (the cycle itself calls the same engine functions): float vectors in
 * and out, nothing converted on the way.  Every call needs params.precond_fp32 = 1 and at least two levels (else SPARSH_ESTATE with the
 * message of sparsh_op_precond_f32, also on a host-only handle); `level` is a level below the coarsest (SPARSH_EINVAL for a level out
 * of range and for the coarsest one, which has no float operator).
 *   sparsh_level_f32_layout: *layout = 1 the level's float operator is the sliced-diagonal mirror, 2 float CSR values, 0 none (coarsest)
 *   sparsh_op_jacobi_f32:    `sweeps` sweeps x <- x + (w (b - A x)) / d, w = (float)omega; x_is_zero: the first is x = (w b) / d
 *   sparsh_op_residual_f32:  r = b - A_level x
 *   sparsh_op_restrict_f32:  bc = R_level r, the products (float)R_ij * r_j added in R's stored order (sparsh_level_csr, which = 2)
 *   sparsh_op_prolong_f32:   xf <- P_level xc + xf (one gathered entry per row under aggregation)
 *   sparsh_op_coarse_f32:    x = the coarsest-level solve of b: the float copy of the dense inverse applied by one wavefront per row,
 *                            or b widened, the fp64 factors, the solution rounded to float
 *   sparsh_op_cvt_f32:       out[i] = (float)in[i] (round to nearest even), any n > 0
 *   sparsh_op_cvt_f2d_dot:   z[i] = (double)z32[i] and *dot = sum z[i] r[i], any n > 0 */
int sparsh_level_f32_layout(sparsh_handle h, int level, int *layout);
int sparsh_op_jacobi_f32(sparsh_handle h, int level, const float *b, float *x, int sweeps, int x_is_zero);
int sparsh_op_residual_f32(sparsh_handle h, int level, const float *b, const float *x, float *r);
int sparsh_op_restrict_f32(sparsh_handle h, int level, const float *r, float *bc);
int sparsh_op_prolong_f32(sparsh_handle h, int level, const float *xc, float *xf);
int sparsh_op_coarse_f32(sparsh_handle h, const float *b, float *x);
int sparsh_op_cvt_f32(sparsh_handle h, long n, const double *in, float *out);
int sparsh_op_cvt_f2d_dot(sparsh_handle h, int n, const float *z32, const double *r, double *z, double *dot);
/* z = M r exactly as the Krylov loops (SPARSH_PBICG, SPARSH_PGMRES) apply it: the V-cycle of the current smoother from a zero
 * guess with the launches a zero start takes, or the fp32 cycle under params.precond_fp32 */
int sparsh_op_precond(sparsh_handle h, const double *r, double *z);
int sparsh_op_dot(sparsh_handle h, int n, const double *x, const double *y, double *out);
int sparsh_op_nrm2(sparsh_handle h, int n, const double *x, double *out);
int sparsh_op_axpby(sparsh_handle h, int n, double a, const double *x, double bcoef, double *y);
/* Test hooks of the GMRES kernels.  They need a ready single-GPU handle for its stream and allocator only:
 * n is free and independent of the handle's matrix.  V is the host basis V[nv][n] (row k = v_k); the device basis is laid out by the
 * engine's own code (stride = n rounded up to 2 doubles / 4 floats; under SPARSH_BASIS_FP32 V is rounded to float on the host and
 * zero-padded).  Bad arguments (NULL handle or array, n <= 0, nv outside 1..65, another precision) are SPARSH_EINVAL, device or not.
 * sparsh_op_gs_dot: launch_gs_dot + launch_gs_finalize; sums[k] = v_k . w for k < nv, and sums[nv] = w . w when want_ww.
 * sparsh_op_gs_update: launch_gs_update + launch_gs_finalize.  w_out = w_in - sum of coef[k] v_k, k ascending; w_in NULL: from 0;
 * in_place: w_in and w_out are one device vector.  want_dots: sums[k] = v_k . w_out; want_ww: sums[nv] = w_out . w_out; sums has
 * nv + 1 entries and those not asked for come back 0.  The device w_out holds `stride` elements, filled with `sentinel` before the
 * launch; the *ntail (<= 3) elements behind row n come back in tail.
 * sparsh_op_gs_scale: launch_gs_scale with the scalar d on the device.  SPARSH_BASIS_FP64: v = w / d in place (vd, tail unused,
 * *ntail = 0).  SPARSH_BASIS_FP32: v = the float vector widened to double, vd = its fp64 copy, tail = the *ntail (<= 3) stored
 * elements behind row n of the float vector.
 * sparsh_op_gmres_small: launch_gmres_step for j = 0..m-1 on a freshly zeroed GmresState, then launch_gmres_solve(k), 0 <= k <= m <= 64.
 * hcol / ccol: the two Gram-Schmidt coefficient columns, packed (column j has j + 1 entries, m (m + 1) / 2 in all); ww_partial[m][nblk]:
 * the partial sums of w . w of step j.  Out: hist[m], R[64 * 64] (column j at R + 64 j), cs[64], sn[64], g[65], ny[64]. */
int sparsh_op_gs_dot(sparsh_handle h, int n, int nv, int precision, const double *V, const double *w, int want_ww, double *sums);
int sparsh_op_gs_update(sparsh_handle h, int n, int nv, int precision, const double *V, const double *coef, const double *w_in,
                        int in_place, int want_dots, int want_ww, double sentinel, double *w_out, double *sums, double *tail, int *ntail);
int sparsh_op_gs_scale(sparsh_handle h, int n, int precision, const double *w, double d, double *v, double *vd, double *tail, int *ntail);
int sparsh_op_gmres_small(sparsh_handle h, int m, int nblk, const double *hcol, const double *ccol, const double *ww_partial, double beta,
                          int k, double *hist, double *R, double *cs, double *sn, double *g, double *ny);
/* Test hooks of the single-vector Krylov kernels (dot2, cg_update, cg_update_zero, p_update, xp_update, bicg_s, bicg_xr, bicg_p) and
 * of finalize_kernel.  One launch through the launcher the loops use; the handle lends its stream and
 * allocator only, n is free.  Vectors that are only read hold n doubles.  Every array a kernel writes -- updated vectors, partial
 * sums, the history -- is padded: the host array holds SPARSH_OP_PAD doubles more than its logical length, goes to the device whole
 * and comes back whole, so the caller sees whatever was written behind the end.  A partial-sum array has the logical length
 * SPARSH_OP_PARTIALS (the cap of the elementwise grid); *nblk returns how many of them the launch wrote.  A host array given for two
 * arguments is one device vector (BiCGStab's As, s, As, As); give the written arguments the padded array.  Coefficients are passed
 * by value and put into the slots of a zeroed scalar block, alpha and nalpha each as given.
 * sparsh_op_cg_update: zero = 0 cg_update_kernel; zero = 1 cg_update_zero_kernel<nt> with d (NULL: dconst), omega and z0.  x NULL:
 * the deferred-x form.
 * sparsh_op_finalize: `repeat` (1..64) back-to-back launch_finalize calls on the same arrays.  code 0..10 (the Fin codes), mode 0,
 * 1 or 2; p0[nblk] (not read in mode 2, may be NULL there), p1[nblk1] or NULL; scal: the SPARSH_OP_SCALARS slots, in and out;
 * hist: hist_cap (+ pad) doubles in and out, or NULL; it: the history slot, < 0: taken from the device counter, whose value goes in
 * and comes out through *iter_ctr (>= 0).  Nothing is all-reduced between modes 1 and 2.
 * SPARSH_EINVAL, device or not: NULL handle or required array, n <= 0, a code, mode, slot or count out of range. */
#define SPARSH_OP_PAD 4
#define SPARSH_OP_PARTIALS 2048
#define SPARSH_OP_SCALARS 18
int sparsh_op_dot2(sparsh_handle h, int n, const double *a, const double *b, const double *c, const double *d, double *p0, double *p1,
                   int *nblk);
int sparsh_op_cg_update(sparsh_handle h, int n, double alpha, double nalpha, const double *p, const double *Ap, double *x, double *r,
                        double *partial, int *nblk, int zero, const double *d, double dconst, double omega, int nt, double *z0);
int sparsh_op_p_update(sparsh_handle h, int n, double beta, const double *z, double *p);
int sparsh_op_xp_update(sparsh_handle h, int n, double alpha, double beta, const double *z, double *p, double *x);
int sparsh_op_bicg_s(sparsh_handle h, int n, double alpha, const double *r, const double *Ap, double *s);
int sparsh_op_bicg_xr(sparsh_handle h, int n, double alpha, double omega1, const double *p1, const double *s1, const double *s,
                      const double *As, const double *r0, double *x, double *r, double *q0, double *q1, int *nblk);
int sparsh_op_bicg_p(sparsh_handle h, int n, double beta, double omega1, const double *r, const double *Ap, double *p);
int sparsh_op_finalize(sparsh_handle h, int code, int mode, const double *p0, int nblk, const double *p1, int nblk1, double *scal,
                       int slot_a, double *hist, int hist_cap, int it, int *iter_ctr, int repeat);

/* Time `reps` back-to-back launches of one operator on resident device data with HIP events
 * on the engine's stream; returns average seconds per launch.  op: 0 spmv, 1 fused jacobi
 * sweep, 2 residual, 3 restrict, 4 prolong, 5 coarse GEMV, 6 dot, 7 axpby, 8 int32 copy (4-byte
 * stream, calibrates the profiler's byte counters), 9 fused Jacobi sweeps ping-ponging between two vectors (the
 * access pattern of a smoothing leg), 10 the same on the level's own resident x / x2 / r buffers, 11 double sweeps
 * (sparsh_set_double_sweep) ping-ponging on those buffers: seconds per launch = per PAIR of sweeps, 12 one SOR sweep (all
 * colours) on the level's own x with r as the right-hand side, issued as a smoothing leg issues it (sparsh_set_sor_path),
 * 13 one GMRES orthogonalisation step on level 0 (`level` must be 0): the last step of a restart cycle, w against
 * restart basis vectors filled with a fixed pattern, through the fused kernels (two dot / update passes, reductions, rotation,
 * normalisation; plus one copy that stands for the store of w), 14 the same step through one launch_dot + reduction and one
 * launch_axpby per basis vector and pass, which is what the fused kernels replace (13 and 14 want SPARSH_BASIS_FP64 on the handle,
 * SPARSH_ESTATE otherwise), 15 the fused step of 13 on a float basis: the same fill pattern rounded to float (`level` must be 0; wants
 * SPARSH_BASIS_FP32 on the handle, SPARSH_ESTATE otherwise), 16 the last post-sweep with its dot through the plane-marching kernel on
 * the level's resident buffers (SPARSH_ESTATE where the level does not run it), 17 one Chebyshev step (the k >= 1 form: both
 * coefficients and the previous correction in use) ping-ponging on the level's resident x / x2 buffers with its d vector and r as
 * the right-hand side: the counterpart of 10 (single-GPU handles), 18 one projection onto mean zero with its dot (launch_sum +
 * launch_project, see "singular systems" below) on level 0's resident x and r (`level` must be 0; single-GPU handles; needs no
 * SPARSH_NULLSPACE_CONSTANT handle). */
int sparsh_bench_op(sparsh_handle h, int op, int level, int reps, double *avg_seconds);

/* ---- restarted GMRES (SPARSH_GMRES, SPARSH_PGMRES) ----
 * GMRES(m) with right preconditioning: x_k = x_0 + M V_k y_k, so the recurrence residual |g_{k+1}| that is stored in the history and
 * compared with tol is the norm of the true residual b - A x up to rounding.  M is one V-cycle from a zero guess under the handle's
 * smoother (Jacobi, SOR in either order -- GMRES needs no symmetric preconditioner) or the fp32 cycle; the identity for SPARSH_GMRES.
 * Orthogonalisation is classical Gram-Schmidt applied twice, fused into one pass over the basis per sweep; the Hessenberg column,
 * the Givens rotations, g and y stay in device memory and the host reads one history entry every check_every iterations (so up to
 * check_every - 1 steps may run past convergence).  Every restart cycle starts from the true residual, whose norm is the stopping
 * test of the solve and is not appended to the history.  SPARSH_ENOCONV at the iteration cap with x updated from the steps taken,
 * SPARSH_ENUMERIC on a NaN.  A lucky breakdown (h_{j+1} not > 0) writes v_{j+1} = 0 without dividing; the cycle ends at its next check.
 * params.use_graph = 1 is accepted and ignored: GMRES launches eagerly, because kernel arguments change with the step index.
 * Refused with SPARSH_EINVAL on a partitioned (multi-GPU) handle: the j + 2 sums of a step need an all-reduce wider than the
 * 16-byte one the engine has; that is a later change.
 * sparsh_set_gmres: restart length 1..64, 0 restores the default of 30, anything else SPARSH_EINVAL.  Callable before or after
 * sparsh_setup, needs no device.  A changed length frees the basis; the next GMRES solve reallocates it.
 * sparsh_gmres_info: the restart length and the device bytes now held for the basis (restart + 1 vectors of level 0 and their
 * per-workgroup partial sums): 0 until the first GMRES solve of the handle, after sparsh_setup and after a changed restart length.
 * Any pointer may be NULL.
 * sparsh_set_gmres_basis: how the basis vectors are stored.  SPARSH_BASIS_FP64 (the default) is the path described above.
 * SPARSH_BASIS_FP32 stores every v_k as the fp64 value rounded once to float (compressed-basis GMRES) and keeps all arithmetic in
 * fp64: w lives in one fp64 vector of its own, the orthogonalisation, the Hessenberg column and V y use the vectors as stored, and
 * the vector handed to M / A is the stored one widened back.  The basis then takes 0.53 of the memory (restart 30) and by byte count 0.55 - 0.6 of a step's traffic.  The
 * history entry |g_{j+1}| becomes an estimate of the true residual (the rounded basis is orthonormal to about 6e-8 only); the solve
 * still ends with SPARSH_OK only when the true residual b - A x of a cycle start is <= tol, and a cycle that ends on |g_{j+1}| <=
 * tol while the true residual is larger is followed by another cycle.  Works with every preconditioner GMRES accepts.  Callable
 * before or after sparsh_setup, needs no device; a changed precision frees the basis like a changed restart length; anything
 * other than the two constants is SPARSH_EINVAL and changes nothing.  Under SPARSH_BASIS_FP32 sparsh_gmres_info counts
 * (restart + 1) vectors of n rounded up to 4 floats, the partial sums and the fp64 vector of w (n rounded up to 4 doubles).
 * sparsh_gmres_basis reads the precision back. */
#define SPARSH_BASIS_FP64 0 /* default: basis vectors stored as double */
#define SPARSH_BASIS_FP32 1 /* basis vectors stored as float, all arithmetic fp64 */
int sparsh_set_gmres(sparsh_handle h, int restart);
int sparsh_gmres_info(sparsh_handle h, int *restart, long *basis_bytes);
int sparsh_set_gmres_basis(sparsh_handle h, int precision);
int sparsh_gmres_basis(sparsh_handle h, int *precision);

/* ---- multicolour SOR smoother ----
 * sparsh_set_smoother: kind SPARSH_SMOOTH_JACOBI (default), SPARSH_SMOOTH_SOR or SPARSH_SMOOTH_CHEBYSHEV (below); sweeps per leg (0: the default -- 6 for SOR,
 * the count AMG_solve_SOR hard-codes, params.sweeps for Jacobi); order SPARSH_SOR_FORWARD / SPARSH_SOR_SYMMETRIC (SOR only).
 * May be called before or after sparsh_setup, also between sparsh_krylov_init_dev and sparsh_krylov_step_dev (the steps then
 * use the new smoother); selecting Jacobi again restores the Jacobi cycle exactly.  SOR is refused (SPARSH_EINVAL) on
 * partitioned (multi-GPU) handles and with params.precond_fp32, as is a Jacobi sweep count on a partitioned handle after its
 * setup; SPARSH_PCG requires SPARSH_SOR_SYMMETRIC (sparsh_solve*, sparsh_krylov_init_dev and sparsh_krylov_step_dev return
 * SPARSH_EINVAL otherwise).
 * Colouring: greedy first-fit over the rows in ascending order on the pattern of A + A^T without the diagonal, colours from 1.
 * One sweep: for c = 1..C (C..1 reversed), all rows i of colour c at once, in place: s = sum_j a_ij x_j in stored order,
 * h = s - b_i, x_i = x_i - (omega*h)/d_i.  The V-cycle keeps the Jacobi hierarchy and order of operations: pre-smoothing
 * forward, coarse levels from x = 0, post-smoothing in the chosen order. */
int sparsh_set_smoother(sparsh_handle h, int kind, int sweeps, int order);
/* colour classes of a level (after sparsh_setup_host; no device needed): number of colours, rows of colour c at
 * rows_per_color[c - 1] (may be NULL) */
int sparsh_level_colors(sparsh_handle h, int level, int *ncolors, int *rows_per_color);
/* colour (1..C) of every row of the level (nrow ints) */
int sparsh_level_color_of_rows(sparsh_handle h, int level, int *color);
/* `sweeps` SOR sweeps of a level on host vectors, colours C..1 when reverse; x_is_zero: x is taken as 0 (not read) */
int sparsh_op_sor(sparsh_handle h, int level, const double *b, double *x, int sweeps, int reverse, int x_is_zero);
/* Debug / measurement knob of the SOR legs: 0 (default) the level policy -- one launch per colour and sweep on every level,
 * since the single-workgroup launch of a whole leg measured slower on every level tried; 1 per-colour launches
 * on every level; 2 the single launch on every level.  Both paths give the same bits. */
int sparsh_set_sor_path(sparsh_handle h, int mode);
/* SOR layout of a level: colours, whether a leg is one launch under the current path, device bytes of the colour-compacted
 * copy.  The smoothed levels (all but the coarsest, which is solved directly) get theirs at sparsh_setup when SOR was selected
 * before it, else at the first SOR solve; any level at its first sparsh_op_sor.  SPARSH_ESTATE when it is not built. */
int sparsh_level_sor_layout(sparsh_handle h, int level, int *ncolors, int *single_launch, long *bytes);

/* ---- Chebyshev polynomial smoother ----
 * sparsh_set_smoother(h, SPARSH_SMOOTH_CHEBYSHEV, degree, 0): a smoothing leg is a Chebyshev polynomial of that degree in D^-1 A
 * (1..16; 0: the default of 4; order must be 0; anything else SPARSH_EINVAL).  One step costs one pass over A, like a Jacobi
 * sweep, plus one vector d per smoothed level (read and written: 16 B per row).  The leg is symmetric, so SPARSH_PCG takes it as
 * it is; SPARSH_AMG, SPARSH_PBICG, SPARSH_PGMRES, sparsh_op_precond and the stepwise Krylov calls accept it too.  Refused
 * (SPARSH_EINVAL) on partitioned (multi-GPU) handles and with params.precond_fp32, like SOR.  The V-cycle keeps the Jacobi hierarchy
 * and order of operations; selecting Jacobi again restores the Jacobi cycle exactly.
 * Bounds, per smoothed level (every level but the coarsest), on the host: gershgorin = max_i sum_j |a_ij| / |a_ii|; lanczos = the
 * largest Ritz value of D^-1/2 A D^-1/2 after min(steps, n) steps of plain Lanczos from a fixed start vector (independent of the
 * thread count); lmax = min(1.1 * lanczos, gershgorin); lmin = lmax / ratio.  Where some a_ii is not positive and finite, lanczos = 0
 * and lmax = gershgorin.  Computed at sparsh_setup / sparsh_setup_host when Chebyshev was selected before it, otherwise at first use.
 * The polynomial assumes a real positive spectrum in [lmin, lmax]: an unsymmetric A is accepted (SPARSH_PGMRES, SPARSH_PBICG), and
 * whether its spectrum is close enough to such an interval is the caller's risk.
 * Step k of a leg (coefficients in double on the host: theta = (lmax + lmin)/2, delta = (lmax - lmin)/2, sigma = theta/delta,
 * rho_0 = 1/sigma, c1_0 = 0, c2_0 = 1/theta; rho_k = 1/(2 sigma - rho_{k-1}), c1_k = rho_k rho_{k-1}, c2_k = 2 rho_k/delta):
 *   h = b_i - s_i ; d_i = c1_k d_i + (c2_k h)/a_ii ; x_i = x_i + d_i      (s_i = sum_j a_ij x_j in stored order, d = 0 before step 0)
 * sparsh_set_chebyshev: ratio > 1 (0: the default of 30) and Lanczos steps 1..64 (0: the default of 10); callable before or after
 * the setup; a changed step count drops the computed bounds.
 * sparsh_set_chebyshev_lmax: the caller's own upper bound for a level (> 0 and finite; 0 restores the estimate); after
 * sparsh_setup_host, and dropped by the next setup.
 * sparsh_level_chebyshev: the bounds of a level (after sparsh_setup_host; no device needed; any pointer may be NULL); lmax and
 * lmin are the ones in use (a forced lmax included).  The coarsest level, which the cycle solves directly, gets bounds on request
 * like any other: they serve sparsh_op_cheby and sparsh_bench_op there.
 * sparsh_op_cheby: one leg of `degree` steps (0..16) of a level on host vectors; x_is_zero: x is taken as 0 (not read). */
int sparsh_set_chebyshev(sparsh_handle h, double ratio, int lanczos_steps);
int sparsh_set_chebyshev_lmax(sparsh_handle h, int level, double lmax);
int sparsh_level_chebyshev(sparsh_handle h, int level, double *lmax, double *lmin, double *gershgorin, double *lanczos);
int sparsh_op_cheby(sparsh_handle h, int level, const double *b, double *x, int degree, int x_is_zero);

/* ---- W- and K-cycles at chosen levels, and flexible CG ----
 * Opt-in: under SPARSH_CYCLE_V (the default) every path, launch and bit is what it was.  Level l is a "WK level" when 1 <= l < last and
 * l % stride == 0; the coarsest level is solved exactly and never recurses.  A level is visited 2^(number of WK levels <= l) times per cycle.
 * The cycle, with the legs of the handle's current smoother and nothing fused across launches (Jacobi: params.sweeps plain sweeps,
 * SOR in its chosen order, Chebyshev of its degree -- exactly what sparsh_op_jacobi, sparsh_op_sor and sparsh_op_cheby compute):
 *   cycle(l, b), from a zero guess (level 0 of the stand-alone iteration: from the caller's x):
 *     l last: x = coarse solve of b.
 *     else:   x = pre-leg(b) ; r = b - A_l x ; b_c = R r ; x_c = solve_coarse(l + 1, b_c) ; x += P x_c ; x = post-leg(b, x).
 *   solve_coarse(l, b):
 *     not a WK level, or kind V:  cycle(l, b).
 *     W:  c = cycle(l, b) ; r = b - A_l c ; d = cycle(l, r) ; x = c + d.
 *     K:  c = cycle(l, b) ; v = A_l c ; rho1 = c.v ; alpha1 = c.b ; q = alpha1 / rho1 ;
 *         r_i = b_i - q v_i ; d = cycle(l, r) ; w = A_l d ;
 *         gamma = d.v ; beta = d.w ; alpha2 = d.r ; rho2 = beta - gamma^2 / rho1 ;
 *         k1 = q - gamma alpha2 / (rho1 rho2) ; k2 = alpha2 / rho2 ; x_i = k1 c_i + k2 d_i.
 *         Guards, decided on the device without a host read: rho1 not finite and > 0: q = 1, k1 = 1, k2 = 1 (the W step; rho2 is then not
 *         formed and reported as 0); else rho2 not finite and > 0: k1 = q, k2 = 0.  No early exit after the first step: the launch
 *         sequence does not depend on data.  Every product and sum of the two vector updates is rounded on its own (no contraction);
 *         the five sums are per-workgroup partial sums added in a fixed order (no atomics, bitwise reproducible run to run).
 * sparsh_set_cycle: kind SPARSH_CYCLE_V / _W / _K; stride 1..8, 0 = the default of 3; anything else is SPARSH_EINVAL and changes nothing.
 * Callable before or after sparsh_setup, needs no device, drops a captured graph.  Selecting V again restores the V-cycle exactly.
 * What accepts what.  W: every method that takes a preconditioner, the stand-alone SPARSH_AMG iteration and sparsh_op_precond (under W
 * params.use_graph is accepted and ignored).  K is not a fixed linear operator: SPARSH_FCG, SPARSH_AMG and sparsh_op_precond only;
 * SPARSH_PCG, SPARSH_PBICG, SPARSH_PGMRES and the stepwise calls return SPARSH_EINVAL and name SPARSH_FCG.  W and K are refused
 * (SPARSH_EINVAL) on partitioned (multi-GPU) handles, with params.precond_fp32 and by sparsh_solve_multi.  A configuration with more
 * than 1024 level visits per cycle, all levels together, is SPARSH_EINVAL at the solve; the message names the strides that fit.
 * sparsh_cycle_info / sparsh_level_cycle: the counts above, available after sparsh_setup_host (no device; any pointer may be NULL;
 * before it nlevels_wk and level_visits are 0).  bytes = device memory held for the cycle's extra vectors (per WK level c and r, under
 * K also v, plus the K step's partial sums and scalars): allocated at first use, 0 until then and after every sparsh_setup; freed by
 * sparsh_setup and sparsh_destroy.
 * SPARSH_FCG: r = b - A x ; z = M r ; p = z ; rho = z.r ; then per iteration q = A p ; sigma = p.q ; alpha = rho / sigma ; x += alpha p ;
 * r -= alpha q ; hist = ||r|| ; z = M r ; rho = z.r and tau = z.q in one pass ; beta = -tau / sigma ; p = z + beta p.  Equal to
 * SPARSH_PCG in exact arithmetic when M is fixed, linear and symmetric.  Scalars stay on the device; check_every, max_iter, the history,
 * SPARSH_ENOCONV and SPARSH_ENUMERIC behave as in SPARSH_PBICG; params.use_graph is accepted and ignored.  One GPU, fp64 recurrences; takes
 * every cycle, every smoother (SOR under the symmetric-order rule of SPARSH_PCG) and the fp32 preconditioner.  The stepwise
 * sparsh_krylov_* calls refuse it with SPARSH_EINVAL.
 * sparsh_op_kstep (test hook): the K step's own launches on host vectors of the level's rows with c and d given -- v = A c, the two
 * sums, q, r ; w = A d, the three sums, the scalars, x; returns r, x and scal8 = {rho1, alpha1, gamma, beta, alpha2, rho2, k1, k2}.  Any
 * level is valid, the coarsest included. */
#define SPARSH_CYCLE_V 0 /* default */
#define SPARSH_CYCLE_W 1
#define SPARSH_CYCLE_K 2
int sparsh_set_cycle(sparsh_handle h, int kind, int stride);
int sparsh_cycle_info(sparsh_handle h, int *kind, int *stride, int *nlevels_wk, long *level_visits, long *bytes);
int sparsh_level_cycle(sparsh_handle h, int level, int *is_wk, long *visits);
int sparsh_op_kstep(sparsh_handle h, int level, const double *b, const double *c, const double *d, double *r, double *x, double *scal8);

/* ---- singular systems: the constant vector as the null space (pure Neumann, fully periodic) ----
 * Opt-in: under SPARSH_NULLSPACE_NONE (the default) every path, launch and bit is what it was.  SPARSH_NULLSPACE_CONSTANT states that
 * A 1 = 0 and 1^T A = 0; the solvers then solve the consistent problem A x = b - mean(b) for the x of mean zero.
 * sparsh_set_nullspace stores the kind on the handle (no device needed); the next sparsh_setup_host / sparsh_setup reads it.  Any other
 * value is SPARSH_EINVAL and changes nothing.
 * sparsh_nullspace_info: the kind the present hierarchy was built with (NONE before any setup), the pinned row of the coarsest level
 * (-1: none) and the two defects of level 0 (0 under NONE); any pointer may be NULL.
 * Setup under CONSTANT.  row_defect = max_i |sum_j a_ij| / sum_j |a_ij| and col_defect, the same over the columns, are taken on
 * level 0; either above 1e-12 is SPARSH_EINVAL (the message says the constant vector is not in the null space and gives the value).
 * Also SPARSH_EINVAL, each message naming the null space: Beck coarsening (params.coarsening = 1: its interpolation does not reproduce
 * constants exactly), params.precond_fp32, a handle with a multi-rank transport.  The coarsest-level solver -- the dense inverse
 * (sparsh_coarse_inverse returns it), the nested-dissection and the block-tridiagonal factorisation alike -- gets A_L with row and
 * column nL - 1 replaced by the unit row and column (pinned_row = nL - 1), a nonsingular matrix; A_L itself stays on the level
 * (sparsh_level_csr, the level's SpMV).  A single-level hierarchy is pinned the same way.  A larger null space (a disconnected
 * domain) is out of scope and behaves as any singular matrix does under NONE.
 * Solves on a hierarchy built under CONSTANT (one GPU, fp64):
 *   - at the start of every solve (SPARSH_AMG .. SPARSH_FCG, sparsh_vcycle*, sparsh_krylov_init_dev) the right-hand side is copied to
 *     a vector of the engine and projected there, b - mean(b): the caller's b is never written; the initial guess x is projected in place;
 *   - every application of the preconditioner returns z - mean(z) (all smoothers, all cycle kinds, sparsh_op_precond included); where
 *     the Krylov loop wants the partial sums of z.r fused, the projection launch delivers them in place of the cycle's last sweep;
 *   - x is projected once more when a solve returns and when a sparsh_krylov_step_dev call returns (rounding drift; the Jacobi legs of
 *     the stand-alone SPARSH_AMG iteration move the mean).
 * Histories and the stopping test are those of the projected system.  params.use_graph is accepted and ignored under CONSTANT.
 * sparsh_solve_multi* and sparsh_op_precond_multi return SPARSH_EINVAL on such a handle.
 * A projection is two launches without a host read or atomics: per-workgroup partial sums of x; then every workgroup adds those in one
 * fixed order, so all hold the same mean bit for bit, and stores x_i - mean (and the partial sums of (x_i - mean) r_i) -- bitwise
 * reproducible run to run.
 * Test hooks (any n > 0; they need a ready single-GPU handle for its stream only, as sparsh_op_gs_*): sparsh_op_project: x -= mean(x),
 * *mean = the mean removed; sparsh_op_project_dot: z -= mean(z) and *dot = z.r of the projected z (partial sums + the engine's final
 * reduction).  Host vectors; the device copies are 16-byte aligned.  sparsh_op_project_dev is the same pair of launches on device
 * vectors, which may sit on any 8-byte boundary (r_dev NULL: no dot; mean / dot may be NULL).
 * sparsh_bench_op op 18: one such pair with the dot on level 0's resident x and r (`level` must be 0; no CONSTANT handle needed). */
#define SPARSH_NULLSPACE_NONE 0      /* default: every path, launch and bit as today */
#define SPARSH_NULLSPACE_CONSTANT 1  /* A 1 = 0 and 1^T A = 0: solve the consistent, mean-free problem */
int sparsh_set_nullspace(sparsh_handle h, int kind);
int sparsh_nullspace_info(sparsh_handle h, int *kind, int *pinned_row, double *row_defect, double *col_defect);
int sparsh_op_project(sparsh_handle h, int n, double *x, double *mean);                       /* x -= mean(x) */
int sparsh_op_project_dot(sparsh_handle h, int n, double *z, const double *r, double *mean, double *dot); /* z -= mean(z); dot = z.r */
int sparsh_op_project_dev(sparsh_handle h, int n, double *x_dev, const double *r_dev, double *mean, double *dot);

/* ---- a block of up to SPARSH_MAX_RHS right-hand sides in one AMG-PCG run ----
 * k systems with one matrix -- load cases, solution components, columns of a block method -- solved together: every kernel of the
 * V-cycle and of the Krylov loop reads the operator once for all columns.  Arrays are column-major: column c at B + c * ldb, ldb >= n
 * (ldx likewise); inside the engine the block is row-interleaved with width 2, 4 or 8 (nrhs rounded up; padding columns hold zeros
 * and are frozen from the start) and callers never see that layout.  Per column the arithmetic is that of the single-vector kernels
 * (row sums in stored order, the epilogues of the Jacobi cycle, the recurrences of SPARSH_PCG); the cycle is the plain Jacobi
 * V(nu,nu) cycle from a zero guess with nothing fused, so column c follows sparsh_solve(SPARSH_PCG) of the same right-hand side up to
 * the last bits of the reductions and of the box-grid kernels' fused launches.
 * method: SPARSH_PCG here (SPARSH_BCG: the coupled loop described further below; SPARSH_MBICG: block BiCGStab, further below).  X: initial guesses in, solutions out.  hist[c * hist_cap + k] = column c's residual after iteration
 * k + 1; entries from iters[c] on are left untouched.  iters / status: nrhs ints each.  All scalars stay on the device, one set per
 * column; a column whose residual is <= tol (at the start or after an iteration) is frozen there and then: its x and r are never
 * written again (predicated writes) and its iteration count stands, so it ends with the iterate a single solve with check_every = 1
 * returns whatever check_every the block uses; a column with a NaN residual is frozen with status SPARSH_ENUMERIC and the others go
 * on.  The host reads the flags every params.check_every iterations and stops when every column is frozen or at params.max_iter
 * (max_iters of the _dev form when > 0; never more than n iterations); the columns still running then get SPARSH_ENOCONV with x
 * updated.  Returns SPARSH_OK if every column converged, else SPARSH_ENUMERIC if any column has it, else SPARSH_ENOCONV.
 * SPARSH_EINVAL (with or without a device): nrhs outside 1..8, a NULL array, ldb or ldx below n, another method, a partitioned
 * (multi-GPU) handle, params.precond_fp32, a smoother other than Jacobi.  SPARSH_ESTATE before sparsh_setup.  params.use_graph is
 * accepted and ignored.  The block vectors (x, x2, b, r of every level; x, r, p, Ap of the loop; scalars, partial sums, histories)
 * are allocated at the first block call for a width and replaced by a call with another width; sparsh_setup and sparsh_destroy
 * free them.  sparsh_multi_info: the width in force and the device bytes held, both 0 until the first block call. */
#define SPARSH_MAX_RHS 8
int sparsh_solve_multi(sparsh_handle h, int method, int nrhs, const double *B, long ldb, double *X, long ldx, double *hist, int hist_cap,
                       int *iters, int *status);
/* the same on device arrays; *seconds (may be NULL): HIP-event time of the whole call on the engine's stream */
int sparsh_solve_multi_dev(sparsh_handle h, int method, int nrhs, const double *B_dev, long ldb, double *X_dev, long ldx, int max_iters,
                           double *hist, int hist_cap, int *iters, int *status, double *seconds);
int sparsh_multi_info(sparsh_handle h, int *width, long *bytes);
/* Operator-level hooks of the block kernels: column-major host arrays with ld = the level's rows (restrict: BC has the coarser
 * level's rows; prolong: XC the coarser level's, XF in/out).  Each interleaves, runs the block launch of the V-cycle and
 * de-interleaves.  spmv_dot: Y = A_l X and dots[c] = x_c . y_c; jacobi: `sweeps` sweeps in X (x_is_zero: X is taken as 0, not read);
 * coarse: the coarsest level's solve (the dense inverse read once for all columns; a factored coarsest level is solved column by
 * column); precond: one block V-cycle from a zero guess, Z = M R (refused like sparsh_solve_multi). */
int sparsh_op_spmv_dot_multi(sparsh_handle h, int level, int nrhs, const double *X, double *Y, double *dots);
int sparsh_op_residual_multi(sparsh_handle h, int level, int nrhs, const double *B, const double *X, double *R);
int sparsh_op_jacobi_multi(sparsh_handle h, int level, int nrhs, const double *B, double *X, int sweeps, int x_is_zero);
int sparsh_op_restrict_multi(sparsh_handle h, int level, int nrhs, const double *R, double *BC);
int sparsh_op_prolong_multi(sparsh_handle h, int level, int nrhs, const double *XC, double *XF);
int sparsh_op_coarse_multi(sparsh_handle h, int nrhs, const double *B, double *X);
int sparsh_op_precond_multi(sparsh_handle h, int nrhs, const double *R, double *Z);
/* average seconds of `reps` back-to-back block launches on the level's resident block buffers: op 0 = SpMV + dot, 1 = Jacobi
 * sweeps ping-ponging (the counterpart of sparsh_bench_op 10); on the eigensolver's resident blocks of width multi_width(nrhs)
 * (level 0 whatever `level` says; reserved by the call): op 2 = the twelve-pair Gram launch with its finalise, 3 = one update;
 * with the generalised solver's blocks beside them (reserved by the call; SPARSH_ESTATE without a B): 4 = the generalised update,
 * 5 = the block SpMV with B; 7 = one projection of the constrained eigensolver (the Gram launch with its finalise, then the apply kernel) of the resident W block with the
 * constraints the last constrained solve left resident (SPARSH_ESTATE unless one of this width has run).  6 is not assigned.
 * Under SPARSH_EIG_BASIS_ORTHO (SPARSH_ESTATE otherwise, and without a B), on the generalised solver's blocks and the mode's small
 * arrays: 8 = the transform of three blocks in place, 9 = the masked subtraction W <- W - X C. */
int sparsh_bench_op_multi(sparsh_handle h, int op, int level, int nrhs, int reps, double *avg_seconds);

/* ---- block CG: the columns of a block share one search space ----
 * sparsh_solve_multi / sparsh_solve_multi_dev with method SPARSH_BCG: O'Leary's block conjugate gradients with the block V-cycle as
 * preconditioner.  Every column minimises over the union of all columns' search directions, which buys iterations where the
 * preconditioner is weak (the unstructured FEM problem) and little where it is good (box grids).  Arguments, refusals, memory rules
 * and the column-major interface are those of the block PCG call; SPARSH_PCG through those calls keeps its bits, launches and bytes.
 * Notation: W = the block width, k = nrhs, padding columns are zero.  Every product and sum is rounded on its own; sums over columns
 * run with c ascending.
 *   R = B - A X ; Z = M R ; P = Z ; then per iteration
 *   Q = A P (block SpMV) ; G = P^T Q and C1 = P^T R (one Gram launch, two pairs) ; alpha = pinv(G) C1 (one wavefront) ;
 *   X += P alpha ; R -= Q alpha ; rn_c = ||R_c|| (one pass; partial sums added in a fixed order by the finalise, no atomics) ;
 *   hist, done = all rn_c <= tol ; Z = M R ; C2 = Q^T Z (Gram launch, one pair) ; beta = -pinv(G) C2 (the factor kept) ;
 *   P = Z + P beta (one pass).
 * pinv: LDL^T of G (upper triangle read) without square roots and with dropped directions: d_j = g_jj - sum_{m<j, kept} l_jm^2 d_m;
 * column j is kept iff g_jj > 0 and d_j > 1e-14 g_jj, else its row of the coefficient matrix is zero and it takes no part in later
 * steps; l_ij = (g_ij - sum_{m<j, kept} l_im l_jm d_m) / d_j; forward, diagonal and backward substitution on the kept set.  A block
 * with equal, dependent, zero or converged columns therefore loses rank, not the solve.
 * Nothing is frozen: the loop ends at the first iteration whose recurrence residuals are all <= tol (read back every
 * params.check_every iterations; the kernels of iterations queued past that point leave at once).  iters[c]: the iterations run, the
 * same for every column, 0 if every column starts <= tol.  hist[c * hist_cap + it]: column c's residual after iteration it + 1.
 * status[c] and the return code: SPARSH_OK, SPARSH_ENOCONV at the cap (X updated), SPARSH_ENUMERIC on a NaN residual or a Gram matrix
 * of rank 0 while a residual is above tol.
 * Memory: P and Q are the block PCG's p and Ap.  Three Gram results, two coefficient matrices, the factor, the flags and the Gram
 * launch's partial sums (2 W^2 * 512 doubles) are the solver's own, reserved at the first SPARSH_BCG call for a width and released
 * with the block vectors; they are counted by sparsh_bcg_info, never by sparsh_multi_info.
 * sparsh_bcg_info: the iterations, the smallest rank and the dropped directions (all iterations together) of the last SPARSH_BCG solve
 * and those bytes; zeros before the first.  Any pointer may be NULL. */
int sparsh_bcg_info(sparsh_handle h, int *iterations, int *min_rank, int *dropped, long *bytes);
/* pinv alone, on the host: coef = sign * pinv(G) C for k x k row-major G (upper triangle read) and C, keep[j] = 1 for a kept column.
 * Returns the rank, or SPARSH_EINVAL (k outside 1..8, a NULL array).  Needs no handle and no device. */
int sparsh_debug_bcg_small(int k, const double *G, const double *C, double sign, double *coef, int *keep);
/* Operator-level hooks of block CG's kernels: host arrays, any n > 0, a ready handle lends its stream only.  Blocks are column-major
 * n x k (ld = n), coefficient matrices k x k row-major; the device runs them at width W (bcg_small: the W given, 2, 4 or 8, k <= W;
 * the others: k rounded up).  bcg_small: the device kernel, run twice (factorising, then with the kept factor; SPARSH_ENUMERIC if the
 * two differ); returns the rank like sparsh_debug_bcg_small.  bcg_update: Xo = X + P alpha, Ro = R - Q alpha, norms[c] = ||Ro_c||;
 * bcg_dir: Po = Z + P beta.  An output that is the array it replaces (Xo == X, Ro == R, Po == P) is updated in place on the device
 * too.  SPARSH_ENUMERIC if a padding entry comes back nonzero. */
int sparsh_op_bcg_small(sparsh_handle h, int W, int k, const double *G, const double *C, double sign, double *coef, int *keep);
int sparsh_op_bcg_update(sparsh_handle h, int n, int k, const double *X, const double *R, const double *P, const double *Q,
                         const double *alpha, double *Xo, double *Ro, double *norms);
int sparsh_op_bcg_dir(sparsh_handle h, int n, int k, const double *Z, const double *P, const double *beta, double *Po);

/* ---- block BiCGStab: up to SPARSH_MAX_RHS right-hand sides of an unsymmetric system ----
 * sparsh_solve_multi / sparsh_solve_multi_dev with method SPARSH_MBICG.  Block PCG, block CG and the eigensolvers need a symmetric
 * operator; this is the block method for a general one.  Arguments, the column-major layout, the hist / iters / status conventions,
 * the return codes, the refusals and the memory rules are those of SPARSH_PCG through those calls; SPARSH_PCG and SPARSH_BCG keep
 * their bits, launches and bytes.  sparsh_solve, sparsh_solve_dev and sparsh_krylov_init_dev refuse the method (SPARSH_EINVAL, with
 * or without a device), and SPARSH_PBICG stays refused by the block calls.
 * Per column the arithmetic is that of sparsh_solve(SPARSH_PBICG), parentheses included; all columns go through two block V-cycles
 * and two block SpMVs per iteration, so the hierarchy is read twice per iteration whatever nrhs:
 *   R0 = B - A X ; R = R0 ; P = R0 ; res_c = ||R0_c|| ; then per iteration
 *   P1 = M P ; AP = A P1 ; alpha1_c = (R.R0)_c, alpha_c = alpha1_c / (AP.R0)_c ; S = R - alpha_c AP ; S1 = M S ; AS = A S1 ;
 *   omega_c = (AS.S)_c / (AS.AS)_c (0 if (AS.AS)_c = 0) ; X = (X + alpha_c P1) + omega_c S1 ; R = S - omega_c AS ;
 *   beta_c = (R.R0)_c / alpha1_c * (alpha_c / omega_c) ; res_c = ||R_c|| ; P = R + beta_c (P - omega_c AP).
 * Every scalar stays on the device, one set per column.  A column whose residual is <= tol (at the start or after an iteration), and
 * a column with a NaN residual (status SPARSH_ENUMERIC), is frozen there and then, as in block PCG: its X, R, P, S and scalars are
 * never written again (predicated stores), it keeps the x it had bit for bit, and it rides through the cycles and SpMVs of the
 * others.  Columns never interact.  A zero denominator is not trapped: the NaN or inf it gives turns the next residual into
 * SPARSH_ENUMERIC, as in the single loop.  Reductions: one partial sum per column and workgroup, added in a fixed order; no atomics.
 * Memory: X, R, P, AP are the block PCG's; R0, S, AS, P1 (n * width doubles each) and the per-column state are the solver's own,
 * reserved at the first SPARSH_MBICG call for a width and released with the block vectors.  sparsh_mbicg_info: the iterations of the
 * last such solve (the largest count of a column) and those bytes, never counted by sparsh_multi_info; zeros before the first.  Any
 * pointer may be NULL. */
int sparsh_mbicg_info(sparsh_handle h, int *iterations, long *bytes);
/* Operator-level hooks of block BiCGStab's kernels: one launch each through the loop's own launcher, on host blocks that are
 * column-major n x nrhs (ld = n) with any n > 0; a ready handle lends its stream only.  The device runs them at the width
 * W = nrhs rounded up to 2, 4 or 8.  frozen: nrhs ints, nonzero = the column must come back untouched; alpha, omega, beta: nrhs
 * coefficients.  Written blocks (S; X and R; P) are in/out: a frozen column keeps its input.  The padding columns of a written block
 * hold a sentinel before the launch and SPARSH_ENUMERIC is returned unless they still do after it.
 * dot2: part0[c * g + w] / part1[c * g + w] = workgroup w's share of a_c . b_c / c_c . d_c, c < W, *nblk = g (the blocks may be one
 * another); the part arrays hold SPARSH_MAX_RHS * SPARSH_MBICG_PARTIALS doubles.  bicg_xr likewise: shares of R_c . R0_c and R_c . R_c.
 * mbicg_finalize: code 0 INIT, 1 ALPHA, 2 OMEGA, 3 BETA_RES on part0 (W * n0 doubles, column c's n0 partials at c * n0) and part1 (may
 * be NULL); scal: SPARSH_MBICG_SCALARS x SPARSH_MAX_RHS, slot-major, in/out, slots in the order alpha1, apr0, alpha, ass, asas, omega1,
 * beta, rr0, res; frozen / iters / status: nrhs ints each, in/out (status 1: frozen on a NaN); hist: nrhs x hist_cap, in/out. */
#define SPARSH_MBICG_SCALARS 9
#define SPARSH_MBICG_PARTIALS 2048
int sparsh_op_dot2_multi(sparsh_handle h, int n, int nrhs, const double *a, const double *b, const double *c, const double *d, double *part0,
                         double *part1, int *nblk);
int sparsh_op_bicg_s_multi(sparsh_handle h, int n, int nrhs, const int *frozen, const double *alpha, const double *R, const double *AP,
                           double *S);
int sparsh_op_bicg_xr_multi(sparsh_handle h, int n, int nrhs, const int *frozen, const double *alpha, const double *omega, const double *P1,
                            const double *S1, const double *S, const double *AS, const double *R0, double *X, double *R, double *part0,
                            double *part1, int *nblk);
int sparsh_op_bicg_p_multi(sparsh_handle h, int n, int nrhs, const int *frozen, const double *beta, const double *omega, const double *R,
                           const double *AP, double *P);
int sparsh_op_mbicg_finalize(sparsh_handle h, int code, int nrhs, const double *part0, int n0, const double *part1, int n1, double *scal,
                             int *frozen, int *iters, int *status, double tol, double *hist, int hist_cap, int it);

/* ---- the lowest eigenpairs of the SPD level-0 operator by LOBPCG on the block path ----
 * nev <= SPARSH_MAX_RHS eigenpairs A x = lambda x with the smallest lambda, the block V-cycle as preconditioner.  The standard
 * problem here, the generalised one A x = lambda B x in sparsh_eigs_gen below; SPD operators only, no null-space handles (those, and
 * constraints, in sparsh_eigs_con further below).  X is column-major, column c at X + c * ldx, ldx >= n: the
 * start block on entry (it must have full rank), the Ritz vectors on return, orthonormal and ordered by ascending lambda[c].
 * Notation: k = nev, W = the block width 2, 4 or 8 (k rounded up; padding columns hold zeros and are never active).
 *  1. start: AX = A X; Rayleigh-Ritz on the pencil (X^T AX, X^T X) gives theta and C; X <- X C, AX <- AX C; there is no P yet.
 *  2. R = AX - X diag(theta) (product and subtraction rounded separately), rn_c = ||R_c||_2.  Column c is active when
 *     rn_c > tol |theta_c|; this is evaluated afresh every iteration (soft locking).  The solve stops when no column is active.
 *  3. W = M R: one block V-cycle from a zero guess on all columns; AW = A W: one block SpMV.
 *  4. the Gram matrices S^T S and S^T A S of S = [X, W, P], A S = [AX, AW, AP]: the upper block triangles, twelve W x W blocks, from one
 *     launch over the pair list and one that adds the per-workgroup partial sums in a fixed order (no atomics).  Both matrices and
 *     the residual norms reach the host in one pinned read.
 *  5. host Rayleigh-Ritz on the rows and columns [all k of X, the active of W, the active of P] (no P in the first iteration):
 *     scale by D = diag(GB)^-1/2, Cholesky D GB D = L L^T (a diagonal entry of L below 1e-7 is a breakdown: a condition number
 *     near 1e14, past which the Ritz values carry no digits), T = L^-1 D GA D L^-T symmetrised, cyclic Jacobi to an off-diagonal
 *     norm of at most eps ||T||_F, eigenvalues ascending, C = D L^-T Y[:, :k].  After a breakdown the step is repeated once without
 *     P and a restart is counted; a second breakdown ends the solve.  C returns to the device as three W x W matrices Cx, Cw, Cp
 *     whose rows of inactive and padding columns are zero.
 *  6. update, one pass, every product and sum rounded on its own and c ascending over 0 .. k - 1:
 *     P'_ij = sum_c W_ic Cw_cj, the running sum continued by + P_ic Cp_cj;  X'_ij = (sum_c X_ic Cx_cj) + P'_ij;  AP' and AX' likewise
 *     from AW, AP, AX with the same coefficients.  Then theta <- the new Ritz values.
 * One iteration is one host synchronisation: (3W)^2 * 16 + W * 8 bytes down, (3 W^2 + W) * 8 bytes up.  params.check_every is
 * ignored.  The Gram launch of an iteration is queued before the host knows the residual norms, so the iteration that finds every
 * column converged has run one cycle it did not need.
 * hist[c * hist_cap + it] = rn_c at the start of iteration it (the evaluation that ends the solve included, while it < hist_cap; other
 * entries are left untouched); iters[c] = the iterations in which column c was active; status[c] = SPARSH_OK or SPARSH_ENOCONV.
 * max_iters <= 0 means params.max_iter.  Returns SPARSH_OK; SPARSH_ENOCONV at the cap (X and lambda then hold the last Ritz pairs,
 * still orthonormal); SPARSH_ENUMERIC on a NaN or when the Rayleigh-Ritz step breaks down at the start (the message then says that
 * the start block is rank deficient) or even after a restart (status[c] = SPARSH_ENUMERIC for every column, X is not written).
 * SPARSH_EINVAL (with or without a device): nev outside 1..8 or above n, a NULL array, ldx below n, tol not finite or not positive,
 * and every handle sparsh_solve_multi refuses: a partitioned (multi-GPU) handle, params.precond_fp32, a W- or K-cycle, a smoother
 * other than Jacobi, a null-space handle.  SPARSH_ESTATE before sparsh_setup.  params.use_graph is accepted and ignored.  On a
 * constant-coefficient box grid the solver runs the block path's CSR kernels, not the matrix-free ones.
 * Memory: seven blocks of n * W doubles (X, AX, W, AW, P, AP, R), (12 W^2 + W) * 512 partial sums, 18 W^2 + W doubles of Gram
 * matrices and residual norms and 3 W^2 + W of coefficients and theta, the solver's own: reserved at the first call for a width,
 * replaced by a call with another width, freed by sparsh_setup and sparsh_destroy.  The cycle runs in the block vectors of
 * sparsh_solve_multi (reserved alongside, see sparsh_multi_info), which carry nothing from call to call: a single or block solve
 * before and after an eigen solve gives the same bits.  sparsh_eig_info: the width in force, the device bytes held by the above
 * (both 0 until the first call) and the restarts of the last solve. */
int sparsh_eigs(sparsh_handle h, int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap,
                int *iters, int *status);
/* the same on a device array; *seconds (may be NULL): HIP-event time of the whole call on the engine's stream */
int sparsh_eigs_dev(sparsh_handle h, int nev, double *X_dev, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap,
                    int *iters, int *status, double *seconds);
int sparsh_eig_info(sparsh_handle h, int *width, long *bytes, int *restarts);

/* ---- the generalised problem A x = lambda B x ----
 * sparsh_eig_set_b: B is n x n (n = the handle's rows), symmetric positive definite, 0-based CSR with sorted columns.  The arrays are
 * copied to the device: the caller may free them.  rowptr == NULL drops B.  B lives until the next sparsh_setup, sparsh_destroy or
 * sparsh_eig_set_b.  Arguments are checked first, on the host, with or without a device, SPARSH_EINVAL with a message that names
 * the defect: a NULL colindex or val; rowptr[0] != 0 or rowptr not non-decreasing; a column out of range or not strictly ascending
 * within its row; a value that is not finite; a row without a stored diagonal or with a diagonal <= 0; B not symmetric, which is some
 * |b_ij - b_ji| > 1e-12 max|b| with a missing transpose entry counting as 0; a handle sparsh_solve_multi refuses.  Then
 * SPARSH_ESTATE before sparsh_setup.  Positive definiteness beyond the diagonal is the caller's statement: an indefinite B surfaces as
 * the Rayleigh-Ritz breakdown at the start.  sparsh_eig_b_info: whether a B is set, its stored entries and the device bytes it holds
 * (all 0 without one).
 * sparsh_eigs_gen / sparsh_eigs_gen_dev: the arguments, refusals, return codes and memory rules of sparsh_eigs / sparsh_eigs_dev, and
 * SPARSH_ESTATE when no B is set.  They return the nev lowest pairs of A x = lambda B x, X B-orthonormal (X^T B X = I) and ordered
 * by ascending lambda.  The steps are those above with B S = [BX, BW, BP] carried beside A S:
 *  1. AX = A X and BX = B X; Rayleigh-Ritz on (X^T AX, X^T BX); X, AX, BX <- . C.
 *  2. R = AX - BX diag(theta) (product and subtraction rounded separately); rn_c = ||R_c||_2 and bn_c = ||BX_c||_2 from one pass.
 *     Column c is active when rn_c > tol |theta_c| bn_c, which no scaling of B changes and which is the rule above for B = I.  hist
 *     stores rn_c.
 *  3. W = M R; AW = A W and BW = B W by two block SpMVs.
 *  4. S^T A S and S^T B S from the same Gram launch, the pairs (S_i, BS_j) in place of (S_i, S_j): twelve pairs, two at the start.
 *     Both matrices and both norm vectors reach the host in the one pinned read (bn in the first row of the unused block below the
 *     diagonal of S^T B S).
 *  5. as above.
 *  6. as above, and BP', BX' from BW, BP, BX with the same coefficients in the same pass (nine blocks in, six out).
 * Memory: the blocks BX, BW, BP (n * W doubles each) are reserved at the first generalised call for a width, beside the seven blocks
 * and small arrays of sparsh_eigs, and are counted in sparsh_eig_info from then on; until then sparsh_eigs, sparsh_eigs_dev and
 * sparsh_eig_info keep their bits, launches and byte counts. */
int sparsh_eig_set_b(sparsh_handle h, const int *rowptr, const int *colindex, const double *val);
int sparsh_eig_b_info(sparsh_handle h, int *is_set, long *nnz, long *bytes);
int sparsh_eigs_gen(sparsh_handle h, int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap,
                    int *iters, int *status);
int sparsh_eigs_gen_dev(sparsh_handle h, int nev, double *X_dev, long ldx, double tol, int max_iters, double *lambda, double *hist,
                        int hist_cap, int *iters, int *status, double *seconds);

/* ---- eigenpairs under constraints: singular operators, more than SPARSH_MAX_RHS pairs ----
 * sparsh_eigs_con / sparsh_eigs_con_dev: the nev <= 8 lowest pairs of A x = lambda B x subject to (B y_j)^T x = 0 for every constraint
 * y_j, X B-orthonormal and ascending in lambda: LOBPCG with constraints (the Y of scipy.sparse.linalg.lobpcg).  gen = 0: the standard
 * problem (B = I, Euclidean orthogonality); gen = 1: the pencil (A, B) of sparsh_eig_set_b (on a null-space handle: of
 * sparsh_eig_con_set_b below), SPARSH_ESTATE without a B.  Y is
 * column-major, n x ncon, ldy >= n; NULL is allowed when ncon == 0.  All other arguments, results, codes and memory rules are those
 * of sparsh_eigs.  Uses: the converged vectors of a first call as Y give the pairs 9..16, and so on (the constraints are only as
 * good as those vectors: eigenvalues shift by the order of their tolerance).
 * Null-space handles: these calls are the eigensolver of a handle set up under SPARSH_NULLSPACE_CONSTANT (a graph Laplacian, a
 * pure-Neumann problem, a floating subdomain).  The constant vector is appended to the constraints implicitly, the pairs returned are
 * the lowest nonzero ones and column 0 is the Fiedler pair.  A is positive semidefinite then, and positive definite on the
 * constrained subspace, which is all the method needs; the block V-cycle runs on the pinned coarsest operator of such a handle.
 * sparsh_eigs, sparsh_eigs_gen, sparsh_solve_multi and sparsh_op_precond_multi keep refusing null-space handles: without the
 * constraint their iterates drift along the null space, which the block cycle does not project out.
 * Notation: mt = ncon (+ 1 on a null-space handle), Pi V = V - Y G^-1 (BY)^T V with G = Y^T (BY).
 *  At entry: Y is interleaved into ceil(mt / W) blocks of the solve's width W (zero padding columns; the column of ones last),
 *  BY = B Y by the block SpMV per block when gen = 1 (BY is Y when gen = 0), G comes from the Gram launch of step 4 and is inverted
 *  on the host (the scaling and Cholesky of step 5, two triangular solves) and uploaded: one extra host read per call.
 *  Step 1: X <- Pi X before AX and BX are formed.  Step 3: W <- Pi (M R) before AW and BW are formed; the projection writes the
 *  cycle's output straight into W and so replaces the copy of the unconstrained loop.  P and R are not projected (P is a
 *  combination of projected blocks) and X is not projected again at return: X^T B X = I holds to the accuracy of sparsh_eigs, the
 *  constraint holds to rounding noise.  Everything else is the loop above.
 *  One projection is the Gram launch with its finalise (two kernels: C = (BY)^T V in a fixed summation order) and then one kernel,
 *  without a host read or atomics: a pass in which every workgroup forms coef = G^-1 C (coef_jc = sum_i Ginv_ji C_ic, i ascending, every product and sum rounded
 *  on its own) and streams dst_ic = src_ic - sum_j Y_ij coef_jc, j ascending from the product of j = 0, one subtraction at the end.
 *  It costs O(n mt) per iteration: the blocks of Y and BY are read once each.
 * With mt == 0 (no constraints, ordinary handle) the call issues the launches of sparsh_eigs / sparsh_eigs_gen, takes no constraint
 * memory and returns their bits.
 * SPARSH_EINVAL (with or without a device): everything sparsh_eigs refuses except a null-space handle; gen outside {0, 1}; ncon
 * outside 0 .. SPARSH_MAX_CON; Y == NULL with ncon > 0; ldy < n; nev + mt > n.  SPARSH_ENUMERIC with "the constraints are rank
 * deficient" when Y^T B Y fails the Cholesky test of step 5 (this includes a caller's constant vector on a null-space handle); the
 * constraint blocks of such a call are freed again and sparsh_eig_con_info reports zeros.
 * Memory: the blocks of Y, those of BY when gen = 1, G (padded order), G^-1 and C are the solver's own, reserved per call shape
 * (width, mt, gen), replaced by a call of another shape, freed by sparsh_setup, sparsh_destroy and a change of width.  They are
 * counted by sparsh_eig_con_info (the constraints in force, whether the constant vector is among them, the bytes; zeros until a
 * constrained call), never by sparsh_eig_info: sparsh_eigs and sparsh_eigs_gen keep their bits, launches and byte counts whatever
 * was called before.
 * The constraints are meant to span an invariant subspace of the pencil, to the accuracy wanted: converged eigenvectors, a null
 * vector.  The stopping rule looks at the unprojected residual A x - lambda B x (R is not projected), which at the solution of a
 * problem constrained by other vectors is a combination of B Y and not zero: such a solve finds the right Ritz values and ends at the
 * iteration cap with SPARSH_ENOCONV.
 * Limits: one GPU, fp64, the Jacobi V-cycle, the constant null space only. */
#define SPARSH_MAX_CON 16
int sparsh_eigs_con(sparsh_handle h, int gen, int nev, double *X, long ldx, int ncon, const double *Y, long ldy, double tol, int max_iters,
                    double *lambda, double *hist, int hist_cap, int *iters, int *status);
int sparsh_eigs_con_dev(sparsh_handle h, int gen, int nev, double *X_dev, long ldx, int ncon, const double *Y_dev, long ldy, double tol,
                        int max_iters, double *lambda, double *hist, int hist_cap, int *iters, int *status, double *seconds);
int sparsh_eig_con_info(sparsh_handle h, int *ncon_total, int *implicit_constant, long *bytes);
/* sparsh_eig_set_b for the constrained calls: the same B, checks and lifetime, but a null-space handle is accepted (L x = lambda D x
 * on a graph Laplacian).  sparsh_eig_set_b itself keeps refusing such a handle, as sparsh_eigs_gen does. */
int sparsh_eig_con_set_b(sparsh_handle h, const int *rowptr, const int *colindex, const double *val);
/* hook of the projection (any n > 0; k in 1..8; m in 1..17; a ready handle lends its stream): Y, BY (n x m) and V (n x k) column-major,
 * Ginv m x m row-major.  C returns (BY)^T V (m x k, row-major), Vout the projected block; V == Vout means in place on the device.
 * SPARSH_ENUMERIC if a padding column of the device block comes back nonzero. */
int sparsh_op_eig_con_project(sparsh_handle h, int n, int k, int m, const double *Y, const double *BY, const double *Ginv, const double *V,
                              double *Vout, double *C);

/* step 5 alone on a compacted pencil of order m <= 24 (row-major, upper triangles read): theta[k], C (m x k, row-major).  Returns
 * 0, or 1 for a breakdown.  Needs no handle and no device. */
int sparsh_debug_eig_small(int m, int k, const double *GA, const double *GB, double *theta, double *C);
/* Operator-level hooks of the eigensolver's kernels: column-major host arrays of any n > 0 rows (ld = n); a ready handle lends its
 * stream only.  gram: G = U^T V (nu x nv, row-major; nu, nv in 1..8).  eig_residual: R = AX - X diag(theta), norms[c] = ||R_c||_2.
 * eig_update: step 6 with k x k row-major coefficient matrices; an output that is the array it replaces (Xo == X, Po == P,
 * AXo == AX, APo == AP) is updated in place on the device too. */
int sparsh_op_gram_multi(sparsh_handle h, int n, int nu, const double *U, int nv, const double *V, double *G);
int sparsh_op_eig_residual(sparsh_handle h, int n, int k, const double *AX, const double *X, const double *theta, double *R, double *norms);
int sparsh_op_eig_update(sparsh_handle h, int n, int k, const double *X, const double *W, const double *P, const double *AX, const double *AW,
                         const double *AP, const double *Cx, const double *Cw, const double *Cp, double *Xo, double *Po, double *AXo,
                         double *APo);
/* The generalised solver's: eig_b_multi: Y = B X (n rows of the handle, nrhs columns) through the block SpMV on the stored B
 * (SPARSH_ESTATE without one).  eig_residual_gen: R = AX - BX diag(theta), rnorms[c] = ||R_c||_2, bnorms[c] = ||BX_c||_2, any n > 0.
 * eig_update_gen: step 6 on nine blocks; in = X, W, P, AX, AW, AP, BX, BW, BP and out = X', P', AX', AP', BX', BP'; an out[i] that is
 * the array it replaces (in[0], in[2], in[3], in[5], in[6], in[8] in that order) is updated in place on the device too. */
int sparsh_op_eig_b_multi(sparsh_handle h, int nrhs, const double *X, double *Y);
int sparsh_op_eig_residual_gen(sparsh_handle h, int n, int k, const double *AX, const double *BX, const double *theta, double *R,
                               double *rnorms, double *bnorms);
int sparsh_op_eig_update_gen(sparsh_handle h, int n, int k, const double *const in[9], const double *Cx, const double *Cw, const double *Cp,
                             double *const out[6]);

/* ---- LOBPCG for clustered spectra: an orthonormalised basis and guard vectors ----
 * sparsh_set_eig_options: two settings of the handle for sparsh_eigs, sparsh_eigs_gen, sparsh_eigs_con and their _dev forms.  Callable
 * before or after sparsh_setup, with or without a device; both survive sparsh_setup.  SPARSH_EINVAL for an unknown basis or a wanted
 * outside 0 .. 8.  With the defaults (PLAIN, 0) every bit, launch and byte count of those calls is what it was without this call.
 *
 * wanted (guard vectors): 0 = all nev columns are wanted.  With 1 <= wanted < nev a solve stops as soon as the columns 0 .. wanted - 1
 * (the lowest Ritz pairs) are inactive and returns SPARSH_OK; the other columns are guard vectors, returned as they stand, with
 * status[c] = SPARSH_ENOCONV where they are still active.  wanted > nev at the time of a solve is SPARSH_EINVAL in that solve.  Guard
 * vectors keep the last wanted column away from the edge of the block, where it converges at the rate of the gap to the next
 * eigenvalue; the padding columns of a block of width 4 or 8 are paid for anyway.  Works under both bases.
 *
 * basis = SPARSH_EIG_BASIS_ORTHO changes steps 2-5 of sparsh_eigs (and of the generalised and constrained loops alike):
 *  2. the active mask is decided on the device, by a small kernel after the residual's finalise, with the rule of step 2 on the norms
 *     the finalise wrote; the host reads it in the iteration's one pinned read, with the Gram matrices, and does not decide it again.
 *  P. if there is a P: G = P^T (B P) by the Gram launch on one pair; a one-wavefront kernel forms, on the rows and columns of the
 *     active columns, D = diag(G)^-1/2, the Cholesky factor D G D = L L^T (sums over p ascending, one rounding per product and sum, as
 *     step 5) and T = D L^-T, an upper-triangular W x W matrix whose rows and columns of all other columns are zero.  An active
 *     column whose diagonal is not finite and positive or whose pivot is below the 1e-7 of step 5 is dropped for this iteration: its
 *     column of T is zero and its bit in the mask "P in the basis" is cleared.  Then P, AP (and BP) <- . T in place, every row on its
 *     own, sums over c ascending, every product and sum rounded on its own.
 *  3. W0 = M R (in a constrained solve: Pi M R); C = (B X)^T W0 by the Gram launch on one pair; W <- W0 - X C on the active columns
 *     and exact zeros on the others (sum over j ascending, one subtraction; this launch stands in for the copy); if there is a P,
 *     the same pair of launches once more against the orthonormalised P: C = (B P)^T W, W <- W - P C in place (without this W and P
 *     grow parallel near convergence and the small pencil loses its accuracy just above the breakdown rule); B W by the block
 *     SpMV (W itself in the standard problem); then twice: G = W^T (B W), T as above with the mask "W in the basis", W and B W <- . T.
 *     B W follows W by the same transforms, so B is applied once.  Then AW = A W.
 *  5. Rayleigh-Ritz on [all k of X, the W columns of the W mask, the P columns of the P mask]; the breakdown rule and the restart
 *     without P stay as the last resort.
 * One host synchronisation per iteration, as before.  The mode's own device memory -- three masks of W doubles and two W x W
 * matrices -- is reserved at the first ortho solve for a width, freed with the solver's blocks and by a change of basis, and
 * counted by sparsh_eig_ortho_info (with the columns of W and of P dropped in the last solve), never by sparsh_eig_info.
 * Refusals are those of sparsh_eigs; sparsh_solve_multi and block CG do not look at either setting. */
#define SPARSH_EIG_BASIS_PLAIN 0   /* default: the loop as documented above */
#define SPARSH_EIG_BASIS_ORTHO 1   /* W and P B-orthonormalised every iteration */
int sparsh_set_eig_options(sparsh_handle h, int basis, int wanted);
int sparsh_eig_options(sparsh_handle h, int *basis, int *wanted);
int sparsh_eig_ortho_info(sparsh_handle h, int *dropped_w, int *dropped_p, long *bytes);
/* The small Cholesky step on the host (no handle, no device): G of order m <= 8 row-major (only the upper triangle, and only the rows
 * and columns of mask_in, are read), T m x m row-major, mask_out[i] = 1 for the kept columns.  sparsh_op_eig_chol_small: the same
 * through the one-wavefront kernel at width W = 2, 4 or 8, bit for bit. */
int sparsh_debug_eig_chol(int m, const double *G, const int *mask_in, double *T, int *mask_out);
int sparsh_op_eig_chol_small(sparsh_handle h, int W, const double *G, const int *mask_in, double *T, int *mask_out);
/* Operator-level hooks of the other three kernels, in the style of sparsh_op_eig_update (column-major host arrays of any n > 0 rows,
 * k x k row-major small matrices, masks of k ints).  eig_transform: V[b] <- V[b] T in place for b < nb <= 3.  eig_ortho_apply:
 * Wout = W0 - X C on the columns of the mask, zeros elsewhere; Wout == W0 runs in place on the device too.  eig_active_mask: the rule
 * of step 2 (gen: with bn) on given norms.  All return SPARSH_ENUMERIC if a padding column of a device block came back nonzero. */
int sparsh_op_eig_transform(sparsh_handle h, int n, int k, int nb, double *const V[3], const double *T);
int sparsh_op_eig_ortho_apply(sparsh_handle h, int n, int k, const double *X, const double *C, const int *mask, const double *W0,
                              double *Wout);
int sparsh_op_eig_active_mask(sparsh_handle h, int k, int gen, double tol, const double *theta, const double *rn, const double *bn,
                              int *mask);

/* device memory helpers so a host language needs no HIP binding of its own */
int sparsh_dev_alloc(sparsh_handle h, long nbytes, void **out);
int sparsh_dev_free(sparsh_handle h, void *p);
int sparsh_dev_fill(sparsh_handle h, double *dst_dev, long n, double value); /* on the engine's stream (thrust::fill of the reference) */
int sparsh_h2d(sparsh_handle h, void *dst_dev, const void *src, long nbytes);
int sparsh_d2h(sparsh_handle h, void *dst, const void *src_dev, long nbytes);
int sparsh_sync(sparsh_handle h);

/* Per-kernel-class device time of the last sparsh_solve_dev call when profiling is enabled
 * (sparsh_profile(h,1)): HIP-event time of every fine-level fused Jacobi sweep launch.
 * out[0] = launches, out[1] = total seconds, out[2] = rows, out[3] = nnz of that level. */
int sparsh_profile(sparsh_handle h, int enable);
int sparsh_profile_read(sparsh_handle h, double *out4);

/* ---- multi-GPU (new design; the reference is single-GPU).  One process per GPU.  Every level
 * above params.replicate_rows is split into contiguous row blocks, one per rank; a smoothing leg
 * exchanges the ghost layers of its vectors once (deep halo, see sparsh_set_deep_halo), every other
 * SpMV-type kernel the neighbours' boundary entries of its input vector, over RCCL (grouped
 * ncclSend/ncclRecv, xGMI); fused scalars are all-reduced; smaller levels and the coarsest solve
 * are computed by every rank.  All ranks run the same host setup on the whole matrix.
 * Bootstrap: rank 0 calls sparsh_comm_unique_id, the 128 bytes travel by any side channel
 * (e.g. a torch.distributed broadcast), every rank calls sparsh_comm_init_rccl BEFORE
 * sparsh_setup.  After setup, vectors passed to the *_dev entry points are the rank's own block
 * [lo, hi) of level 0 (sparsh_local_range). */
int sparsh_set_device(int device); /* make `device` current for this thread (call before sparsh_comm_init_rccl) */
int sparsh_comm_unique_id(char id128[128]);
int sparsh_comm_init_rccl(sparsh_handle h, const char id128[128], int rank, int nranks);
int sparsh_local_range(sparsh_handle h, int level, int *lo, int *hi, int *replicated);
/* Overlap the halo exchange with computation (default off): the exchange is issued on a second
 * stream while the 64-row slices that reference no halo column are processed; the boundary slices
 * follow once the halo has landed.  Same arithmetic, same results.  May be toggled between solves. */
int sparsh_set_overlap(sparsh_handle h, int enable);

/* Deep-halo (communication-avoiding) smoothing on the partitioned levels, default ON; read by sparsh_setup.  Every rank
 * holds, next to its own rows, K = sweeps + 1 layers of ghost rows of the level operator; a smoothing leg exchanges the
 * ghost layers of its right-hand side and of its iterate ONCE and then sweeps a shrinking set of rows (sweep s updates the
 * own rows and the layers <= K - s), so the own rows and the first ghost layer end up exactly as in the global sweep and
 * the residual needs no exchange either: ~13 transport calls per AMG-PCG iteration instead of ~49 with three partitioned
 * levels.  Same arithmetic per row (bitwise the one-rank results for a fixed number of cycles).  0 restores one halo
 * exchange in front of every sweep (the overlap mode below applies to that schedule only).
 * sparsh_exchanges_issued: transport calls (halo or ghost-layer exchanges) this handle has issued so far. */
int sparsh_set_deep_halo(sparsh_handle h, int enable);
/* Inspection / test hooks of a deep-halo level of this rank: info4 = {K (0: not a deep level), local rows (own + padding +
 * ghost layers <= K-1), local columns (layers <= K), first ghost index}; layer_end(d) = local indices in layers 0..d;
 * prefix_spmv: y[0, rows) = rows [0, rows) of the rank-local operator times x_ext (local columns), no exchange -- lets
 * a test run every kernel family over every row prefix a smoothing leg launches. */
int sparsh_deep_info(sparsh_handle h, int level, int *info4);
int sparsh_deep_layer_end(sparsh_handle h, int level, int d, int *end);
int sparsh_deep_prefix_spmv(sparsh_handle h, int level, int rows, const double *x_ext, double *y);
long sparsh_exchanges_issued(sparsh_handle h);

/* In-process transport for tests: nranks handles driven by nranks host threads on one GPU. */
int sparsh_comm_group_create(int nranks, void **group);
void sparsh_comm_group_destroy(void *group);
int sparsh_comm_init_group(sparsh_handle h, void *group, int rank);
/* fault injection for tests: from its ncalls-th halo exchange on (counted per rank, 0-based) the in-process
 * transport fails on every rank.  Solvers must then return SPARSH_ECOMM, and the handle keeps
 * returning it (sticky) until sparsh_setup is called again.  ncalls < 0 switches the hook off. */
/* Multi-rank schedule chosen from measurements (round 3).  With more than one rank and replicate_rows <= 0 (the default)
 * sparsh_setup first measures the transport it was given -- one neighbour exchange (latency and rate), the 16-byte all-reduce,
 * one all-gather -- and the device's sweep floor and streaming rate, takes the slowest rank's numbers, models every level's
 * share of a V(nu,nu) cycle as partitioned with deep halos / partitioned with one exchange per sweep / replicated, and
 * partitions the prefix of levels (with one smoothing schedule) that minimises the total.  replicate_rows > 0 or
 * sparsh_set_comm_tuning(h, 0) keep the caller's threshold and sparsh_set_deep_halo.
 * sparsh_comm_schedule: info4 = {rows, boundary rows of a middle rank, partitioned, deep halo}, cost_us3 = modelled microseconds
 * per V-cycle {deep halo, exchange per sweep, replicated}.  sparsh_comm_measured: m7 = {exchange us, exchange us/MB, all-reduce us,
 * all-gather us, all-gather us/MB, sweep floor us, sweep us/MB}.
 * sparsh_comm_group_set_delay (in-process test transport only): every transport call occupies the caller's stream that many
 * microseconds first -- a slow link, to see the schedule move. */
int sparsh_set_comm_tuning(sparsh_handle h, int mode);
/* host-only what-if (after sparsh_setup_host; no device, no transport): the schedule the tuner would choose for `nranks` ranks from the
 * seven numbers m7 (layout of sparsh_comm_measured); read it back with sparsh_comm_schedule */
int sparsh_plan_comm_schedule(sparsh_handle h, int nranks, const double *m7);
int sparsh_comm_schedule(sparsh_handle h, int level, int *info4, double *cost_us3);
int sparsh_comm_measured(sparsh_handle h, double *m7);
int sparsh_comm_group_set_delay(void *group, double microseconds);
int sparsh_comm_group_fail_after(void *group, int ncalls);

/* Host-only planning query (after sparsh_setup_host): the block of operator `which` (0 A_l, 1 P_l,
 * 2 R_l) that `rank` of `nranks` holds when every level is partitioned, with its halo plan.
 * sizes8 = {rows, nnz, own input entries, halo entries, send segments, recv segments,
 * packed send entries, first global row}.  The _get call copies the arrays of the last query:
 * local CSR (columns renumbered: own entries first, then halo), global index of every halo
 * entry, indices to pack, and (peer, offset, count) triples of the send / receive segments. */
int sparsh_dist_local_op(sparsh_handle h, int level, int which, int rank, int nranks, int *sizes8);
int sparsh_dist_local_op_get(sparsh_handle h, int *rowptr, int *col, double *val, int *halo_global, int *send_idx, int *send_segs3,
                             int *recv_segs3);

/* Host-only planning query of the deep-halo layout (after sparsh_setup_host): the block of A_level that `rank` of `nranks`
 * holds with K ghost layers, and its exchange plan of the given depth.  sizes8 = {local rows (own + padding + layers <= K-1),
 * nnz, own rows, first ghost index (own rows rounded up to 64), local indices (all layers), send segments, receive segments,
 * packed send entries}.  _get copies: local CSR (local column numbering), global index of every local index (-1: padding),
 * layer_end[0..K], own indices to pack, (peer, offset, count) of the send segments, local position of every received entry,
 * (peer, offset, count) of the receive segments. */
int sparsh_dist_deep_op(sparsh_handle h, int level, int rank, int nranks, int K, int depth, int *sizes8);
int sparsh_dist_deep_op_get(sparsh_handle h, int *rowptr, int *col, double *val, int *global_of, int *layer_end, int *send_idx,
                            int *send_segs3, int *recv_pos, int *recv_segs3);

#ifdef __cplusplus
}
#endif
#endif
