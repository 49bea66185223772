// kernels.hpp -- launch interface of the hand-written gfx950 kernels (kernels.hip).
// Everything here works on device pointers and enqueues on the given HIP stream; nothing
// allocates, synchronises or touches the host (graph-capture safe).
#pragma once

#include <hip/hip_runtime_api.h>

#include <vector>

#include "box_plan.hpp"

namespace sparsh {

// level-wide stencil of the sliced-diagonal layout (see DevCsr::sd_tab)
struct SdTable {
    int nd = 0;
    int near = 0;  // 73 / 52 / 31: nd = 7 / 5 / 3 with offsets -1, 0, +1 in the three middle slots; else 0
    int off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double cval[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// Device CSR + the row-block schedule of the CSR-stream kernels.
struct DevCsr {
    int nrow = 0, ncol = 0, nnz = 0;
    int *rowptr = nullptr;
    int *col = nullptr;
    double *val = nullptr;
    // row blocks of the workgroup CSR-stream kernel: one record of 4 ints per block {first row, end row, first
    // entry, end entry} (16-byte aligned); nnz of a block <= kStreamNnz unless it is a single long row
    int *rowblk = nullptr;
    int nblk = 0;
    // optional compressed column indices of the row blocks (csr_rowlane16_kernel): 16-bit deltas -- first entry of a row
    // relative to cbase[block], further entries relative to the previous column of the row; cbase[block] = -1 where a
    // delta does not fit (that block reads col[])
    unsigned short *col16 = nullptr;
    int *cbase = nullptr;
    int nblk16 = 0;  // blocks that use the 16-bit form
    // wave-granular schedule: wave-block k owns rows [waveblk[k], waveblk[k+1]) (<= 64 rows,
    // <= kWaveNnz products unless it is a single long row)
    int *waveblk = nullptr;
    int nwblk = 0;
    // optional sliced-ELL mirror (slices of 64 rows, column-major inside a slice) for operators
    // with near-uniform row length: lane = row, every access of a wave is one contiguous segment
    int nslice = 0;
    int *slice_ptr = nullptr;   // nslice+1 offsets (in entries) into sell_col / sell_val
    int *sell_col = nullptr;
    double *sell_val = nullptr;
    long sell_entries = 0;
    // optional sliced-diagonal mirror for stencil-like operators: per slice of 64 rows the distinct
    // offsets (col - row) are stored once, values sit column-major by offset slot, a 64-bit lane
    // mask per slot says which rows really hold an entry there.  No per-entry column index: 8 B
    // instead of 12 B per stored entry.
    int *sd_ptr = nullptr;              // nslice+1: first slot of every slice (| kSdConstBit, see below)
    int *sd_off = nullptr;              // per slot: col - row
    unsigned long long *sd_mask = nullptr;  // per slot: lanes (rows of the slice) that hold an entry
    double *sd_val = nullptr;           // value blocks (64 values, lane-major) of the slots that need one
    long sd_slots = 0;
    // constant slots: where every present entry of a slot carries the same value (constant-
    // coefficient stencils and their aggregated coarse operators) the value lives once in sd_cval
    // and the slot owns no block: sd_vidx = -1.  Otherwise sd_vidx = index of its block in sd_val.
    int *sd_vidx = nullptr;
    double *sd_cval = nullptr;
    long sd_vblocks = 0;                // blocks stored in sd_val
    // fixed-stride records (kSdRecInts ints per slice) for slices made of <= 8 constant slots: one
    // address computation and one scalar round trip give the kernel everything it needs about the
    // slice (offsets, lane masks, constants, slot count); other slices carry count -1 and go through
    // sd_ptr.  Layout: int off[8]; u64 mask[8]; double cval[8]; int count; pad.
    int *sd_rec = nullptr;
    // level-wide stencil table: when (nearly) all value-free slices draw their (offset, constant)
    // pairs from one set of <= 8, that set travels as a kernel argument and a slice only needs its
    // 8 lane masks (sd_tmask, 64 B per slice; sd_tconf = 1 where the slice conforms).  The wave then
    // issues its x gathers straight from the kernel arguments, in parallel with the mask load,
    // instead of after a record round trip.
    SdTable sd_tab;
    unsigned long long *sd_tmask = nullptr;
    int *sd_tconf = nullptr;
    bool has_sdia() const { return sd_ptr != nullptr; }
    // box grid: the table is the 7-point stencil (-plane, -line, -1, 0, +1, +line, +plane) of an nx x ny x nz grid in lexicographic
    // order, every slice conforms and a row lacks exactly the neighbours that would lie outside the box.  Such a level can run
    // two Jacobi sweeps in one pass over its vectors (sdia_box2_kernel); box2 = the launch plan (box_planner, or a timed or forced
    // one; q == 0: none), box_on = the setup's verdict that the double sweep beats two single ones on this level (timed there, or forced)
    int box_nx = 0, box_ny = 0, box_nz = 0;
    BoxPlan box2;
    bool box_on = false;
    // the same for the single-stage kernel of the launches that carry an epilogue (sdia_box1_kernel): plan and the setup's verdict
    BoxPlan box1;
    bool box1_on = false;
    // box_exact = the stencil's off-diagonal constants are all 0 or +-2^k, k >= 0 (box_exact_offdiag: decided at setup from sd_tab.cval,
    // the operator alone); box_fma = box_exact under KernelConfig::box_exact_fma: both box kernels then take the instances whose
    // off-diagonal terms are one FMA each -- the same bits, six fp64 instructions fewer per point and stage
    bool box_exact = false, box_fma = false;
    // rank-local blocks: slices whose rows touch no halo column (interior) / some (boundary)
    int *int_list = nullptr, *bnd_list = nullptr;
    int nint = 0, nbnd = 0;
};

// per-handle choice of the SpMV-type kernel family (A/B measurements; defaults = the fastest measured).
// Lives in the Engine (sparsh_set_kernel_config / sparsh_set_const_slots act on a handle): no
// process-wide state.
struct KernelConfig {
    int kind = 3;       // 0 workgroup CSR-stream, 1 wave CSR-stream, 2 sliced ELL, 3 sliced diagonals; 2 and 3 fall
                        // back (3 -> 2 -> 0) where the operator does not qualify for the mirror
    int vec = 3;        // CSR-stream kernels: 0 one entry per load, 1 two entries per lane (16-B val / 8-B col loads), 2 (workgroup kernel)
                        // col/val staged in LDS and the x gathers issued in row-lane order (csr_rowlane_kernel), 3 = 2 for operators
                        // that stream from HBM (> 240 MB of CSR bytes), 1 below (a cache-resident ragged operator is faster on 1);
                        // 4 = 2 with 16-bit delta-coded column indices where the operator carries them (csr_rowlane16_kernel)
    bool auto_policy = true;  // choose nt / remap per operator from its size (overrides the two below)
    bool nt = true;     // non-temporal loads for the matrix stream
    int remap = 1;      // 0 none, 1 XCD x owns the x-th contiguous eighth, G>1 groups of G row blocks dealt round-robin to XCDs
    bool table = true;  // use the level-wide stencil table where a level has one
    bool tile = false;  // table levels of grid stencils: stage x tiles in LDS (sdia_tile_kernel) on whole-level launches
    bool const_slots = true;  // layout option read at setup: fold constant diagonals of a slice into one scalar
    bool place_search = true; // setup: choose by timing which buffers hold the finest level's iterate, its twin and the Krylov residual
    bool cg_nt = true;        // ... with x, p, Ap, d streamed past the caches (non-temporal): r and z0, which the cycle's first sweep reads,
                              // stay resident (+1.3 % it/s at 216^3 in a same-process A/B)
    bool fuse_cg_zero = true; // PCG: the cg_update kernel also writes the V-cycle's zero-guess sweep of level 0
    int alt_dir = 1;          // consecutive sweeps of a smoothing leg walk the level in alternating directions (CsrArgs::reverse):
                              // 0 never, 1 where a sweep streams more than 640 MB (2.5x the Infinity Cache), 2 always
    bool defer_x = true;       // PCG: x += alpha p rides in the direction update at the end of the iteration (xp_update_kernel) instead of in the
                               // residual update: p is read once for both
    bool zero_start = true;    // double-sweep levels: a leg that starts from a zero guess runs its first three sweeps as one launch that
                               // reads only the right-hand side (launch_box2 from_zero)
    int box1 = 1;              // box-grid levels: the launches with an epilogue of their own (SpMV + dot, last post-sweep + dot / + prolongation,
                               // residual + pair restriction) through the plane-marching kernel (sdia_box1_kernel): 0 never, 1 where the setup
                               // measured it faster than the table kernel (levels of >= 400 000 rows), 2 wherever a plan exists
    int box2 = 1;              // box-grid levels (DevCsr::box_nx): two Jacobi sweeps per launch (sdia_box2_kernel): 0 never, 1 where the
                               // setup measured it faster than two single sweeps (levels of >= 400 000 rows), 2 wherever a plan exists
    int box_exact_fma = 1;     // box-grid levels: the off-diagonal terms of the box kernels' stencil sums as one FMA each (DevCsr::box_fma):
                               // 0 never, 1 where the level's constants make that exact (DevCsr::box_exact)
    bool const_diag = true;    // levels whose diagonal is one constant: the vector kernels that divide by it (zero-guess sweeps fused
                               // into cg_update / the restriction) take it as an argument instead of streaming diag[]
    bool fuse_prolong = true;  // V-cycle: the last post-sweep of a level adds its result to the finer level's iterate itself
                               // (OP_JACOBI_PROLONG) instead of storing it for a prolongation launch
    bool pair_restrict = true; // V-cycle: on levels whose aggregates are the row pairs (2J, 2J+1) the residual kernel also
                               // restricts and writes the coarse level's zero-guess sweep (OP_RESID_PAIR)
    int idx16 = 1;      // layout option read at setup: build the 16-bit delta column form (DevCsr::col16) for 0 no operator,
                        // 1 operators whose default family is the CSR-stream kernel streaming from HBM, 2 every operator
};

// which kernel a launch of launch_csr on operator A runs under cfg (one decision, used by the
// launcher and by every report of it)
enum CsrFamily : int { FAM_CSR_BLOCK = 0, FAM_CSR_WAVE = 1, FAM_SELL = 2, FAM_SDIA = 3, FAM_SDIA_TAB = 4, FAM_CSR_ROWLANE = 5, FAM_CSR_ROWLANE16 = 6 };

constexpr int kBlock = 256;       // threads per workgroup (4 waves)
constexpr int kEwGridMax = 2048;  // workgroups of an elementwise launch (grid-stride: ~8 per CU) = the most partial sums it writes
constexpr int kStreamNnz = 2048;  // products staged in LDS per workgroup (16 KiB)
constexpr int kWaveNnz = 512;     // products staged in LDS per wave (4 KiB) in the wave-granular kernel
constexpr int kSdRecInts = 48;        // 192 B per slice record
constexpr int kSdConstBit = 1 << 30;  // set in sd_ptr[s] when every slot of slice s is a constant slot
constexpr int kSdPlainBit = 1 << 29;  // set in sd_ptr[s] when no slot of slice s is (its value blocks are consecutive)
constexpr int kSdPtrMask = (1 << 29) - 1;
constexpr int kCsrPad = 4;        // zeroed entries appended to col/val so paired loads stay in bounds

// epilogue selector of the CSR-stream kernel: what happens to the row sum s_i = (A x)_i
enum CsrOp : int {
    OP_SPMV = 0,      // y_i = s_i
    OP_RESID = 1,     // y_i = b_i - s_i                          (store_residual)
    OP_JACOBI = 2,    // y_i = x_i + omega*(b_i - s_i)/d_i        (one fused Jacobi sweep, y != x)
    OP_ADD = 3,       // y_i = s_i + y_i                          (transfer_solution, beta = 1)
    OP_SPMV_DOT = 4,  // y_i = s_i ; partial += x_i*s_i           (Ap and p.Ap of CG)
    OP_RESNORM = 5,   // partial += (s_i - b_i)^2                 (residual norm, nothing stored)
    OP_JACOBI_DOT = 6, // Jacobi sweep ; partial += y_i*b_i        (last post-sweep of PCG: z.r)
    OP_JACOBI_PROLONG = 8, // Jacobi sweep whose result is not stored but added to the finer level's iterate: y2_f = 1.0*xn_i + y2_f
                           // for the (at most two) fine rows f of aggregate i -- the last post-sweep of a level and
                           // transfer_solution into the level above in one launch (aggregation P only: every fine row has one owner)
    OP_CHEBY = 9,     // one Chebyshev step: dn_i = beta*dprev_i + (omega*(b_i - s_i))/d_i (dprev == nullptr: the first step of a leg,
                      // dn_i = (omega*(b_i - s_i))/d_i) ; y_i = x_i + dn_i ; y2_i = dn_i   (y != x; dprev may be y2 or x)
    OP_CHEBY_DOT = 10, // the same ; partial += y_i*b_i                 (last post-smoothing step of PCG: z.r)
    OP_RESID_PAIR = 7  // levels whose aggregates are the row pairs (2J, 2J+1): y_J = (b - s)_2J + (b - s)_2J+1 and
                       // y2_J = omega*y_J/d_J -- residual, restriction and the coarse level's zero-guess sweep in one
                       // launch (table kernel only: launch_resid_pair)
};

struct CsrArgs {
    const double *x = nullptr;   // input vector (gathered)
    const double *b = nullptr;   // rhs (RESID/JACOBI/RESNORM)
    const double *d = nullptr;   // diagonal (JACOBI)
    double *y = nullptr;         // output
    double *y2 = nullptr;        // second output (CHEBY: the step's correction dn; RESID_PAIR: the coarse level's zero-guess sweep; d is then the coarse diagonal;
                                 // JACOBI_PROLONG: the finer level's iterate)
    double dconst = 0.0;         // RESID_PAIR with d == nullptr: the coarse level's constant diagonal
    const int *members = nullptr; // JACOBI_PROLONG: two fine rows per row (second -1 for a single); nullptr = rows (2i, 2i+1)
    int nfine = 0;                // JACOBI_PROLONG: rows of the finer level
    double omega = 0.0;          // (CHEBY: the step's coefficient c2)
    const double *dprev = nullptr; // CHEBY: the previous step's correction (entry i is read by row i alone: may alias y2, or x after a
                                   // zero-guess step, whose iterate is its correction); nullptr on the first step of a leg
    double beta = 0.0;           // CHEBY: the step's coefficient c1
    double *partial = nullptr;   // per-block partial sums (reductions), size >= nblk
    // optional subset launch of the sliced kernels (multi-GPU overlap): process only the slices
    // listed, write reduction partials from index partial_off on
    const int *slice_list = nullptr;
    int nlist = 0;
    int partial_off = 0;
    // walk the row blocks / slices from the last to the first: consecutive sweeps of a smoothing leg alternate, so a sweep starts on
    // the part of the iterate the previous one wrote last (still in the memory-side cache); placement only, results unchanged
    int reverse = 0;
};

// host-side builder of the row-block schedule (returns number of blocks; out sized nrow+1 max)
int build_rowblocks(int nrow, const int *rowptr, int *out);
int build_waveblocks(int nrow, const int *rowptr, int *out);
// the row-block schedule as the 4-int records DevCsr::rowblk holds (4 * *nblk ints)
std::vector<int> rowblock_records(int nrow, const int *rowptr, int *nblk);
// 16-bit delta form of the column indices for the row blocks `rec` (DevCsr::col16 / cbase); col16 holds nnz entries,
// cbase nblk; returns the number of blocks that took the 16-bit form
int build_col16(const int *rowptr, const int *col, const int *rec, int nblk, unsigned short *col16, int *cbase);

// returns the number of per-workgroup partial sums the launch writes (reducing ops)
// `finest`: launch on the finest level (selects a separately named kernel instance for profilers)
int launch_csr(const DevCsr &A, CsrOp op, const CsrArgs &a, bool finest, hipStream_t st, const KernelConfig &cfg);
CsrFamily csr_family(const DevCsr &A, const KernelConfig &cfg);
// Double Jacobi sweep y = J(J(x)) on a box-grid level (DevCsr::box_nx > 0), bitwise what two OP_JACOBI launches give.
// box2_applies = the level has a plan (DevCsr::box2) and runs it under cfg
bool box2_applies(const DevCsr &A, const KernelConfig &cfg);
// from_zero: the leg starts from x = 0: x is not read, y = J(J(omega b / d)) = the first three sweeps of the leg
void launch_box2(const DevCsr &A, const double *x, const double *b, double *y, double omega, bool finest, hipStream_t st, bool from_zero = false);
// box-grid level whose aggregates pair a point with its neighbour one line (axis +-1) or one plane (axis +-2) up: residual, restriction and
// the coarse zero-guess sweep in one launch (dc == nullptr: constant coarse diagonal dconst); axis < 0: aggregates numbered from the far
// end of the coarse box (J = nc - 1 - lexicographic index)
void launch_box_resid_pair(const DevCsr &A, int axis, const double *x, const double *b, const double *dc, double dconst, double omega,
                           double *bc, double *xc, hipStream_t st);
// Single-stage plane-marching kernel on a box-grid level (sdia_box1_kernel); epi: 0 y = A x + partial x.Ax, 1 Jacobi sweep into y + partial
// y.b, 2 residual + pair restriction (aggregates = row pairs; y = coarse rhs, y2 = coarse zero-guess sweep, d / dconst = coarse diagonal),
// 3 Jacobi sweep added to the finer iterate y2 (members / nfine as OP_JACOBI_PROLONG), 4 plain Jacobi sweep into y (the odd sweep of a leg
// that runs double sweeps).  Returns the number of partial sums written.
bool box1_applies(const DevCsr &A, const KernelConfig &cfg);
int launch_box1(const DevCsr &A, int epi, const CsrArgs &a, bool finest, hipStream_t st);
// OP_RESID_PAIR over the whole of A (a.y = coarse rhs, a.y2 = coarse iterate, a.d = coarse diagonal); applies to operators
// that run the table kernel under cfg -- resid_pair_applies says whether launch_resid_pair may be called
bool resid_pair_applies(const DevCsr &A, const KernelConfig &cfg);
void launch_resid_pair(const DevCsr &A, const CsrArgs &a, bool finest, hipStream_t st, const KernelConfig &cfg);
// whether consecutive sweeps over A alternate their walking direction under cfg (KernelConfig::alt_dir)
bool csr_alternates(const DevCsr &A, const KernelConfig &cfg);
const char *csr_family_name(CsrFamily f);
int sdia_tile_rows(const DevCsr &A, const KernelConfig &cfg);  // rows per workgroup of the LDS-tiled table kernel, 0 = not used
// placement the launcher picks for A under cfg: non-temporal matrix stream, XCD remap mode
void csr_placement(const DevCsr &A, const KernelConfig &cfg, bool *nt, int *remap);

// x_i = omega*b_i/d_i : first Jacobi sweep from a zero guess (bitwise equal to the full sweep)
// (here and below: d == nullptr means every row's diagonal entry is dconst -- constant-coefficient stencils: the stream is not read)
void launch_jacobi_zero(int n, const double *b, const double *d, double dconst, double omega, double *x, hipStream_t st);
// xf_i = xc[agg_i] + xf_i : prolongation for an aggregation P (one unit entry per row)
void launch_prolong_agg(int n, const int *agg, const double *xc, double *xf, hipStream_t st);
// bc[J] = sum of r over aggregate J (R = P^T of an aggregation P: all values 1.0, not read)
void launch_restrict_agg(int nc, const int *rowptr, const int *col, const double *r, double *bc, hipStream_t st);
// the same, and xc[J] = omega*bc[J]/dc[J]: the coarse level's zero-guess sweep in the same launch
void launch_restrict_agg_zero(int nc, const int *rowptr, const int *col, const double *r, double *bc, const double *dc, double dconst,
                              double omega, double *xc, hipStream_t st);
// x = A^{-1} b with the explicit row-major inverse (coarsest level)
void launch_gemv(int n, const double *M, const double *b, double *x, hipStream_t st);

// ---- multicolour SOR smoother (parallel::sor_smoother, src/AMG_smoothers.cpp:78-102) on a level's colour-compacted copy
struct SorArgs {
    const int *rows = nullptr;     // level row of every compacted row (colour by colour, ascending inside a colour)
    const int *rowptr = nullptr;   // compacted CSR: rowptr / col / val (col and val carry kCsrPad zeroed tail entries)
    const int *col = nullptr;
    const double *val = nullptr;
    const double *diag = nullptr;  // diagonal entry of every compacted row
    const double *b = nullptr;     // right-hand side, by level row
    double *x = nullptr;           // iterate, by level row, updated in place
    double omega = 0.0;
};
// one colour: rec = that colour's row-block records (4 ints each, rowblock_records over the compacted rowptr); nt: non-temporal
// loads of the matrix stream
void launch_sor_colour(const int *rec, int nblk, bool nt, const SorArgs &a, hipStream_t st);
// every colour (C..1 when reverse) of `sweeps` sweeps in one single-workgroup launch; cstart = ncolors + 1 compacted row offsets
void launch_sor_level(const int *cstart, int ncolors, int sweeps, bool reverse, const SorArgs &a, hipStream_t st);

// ---- BLAS-1 (daxpby/daxpbyc kernels, cublasDaxpy/Ddot/Dnrm2, thrust::fill of the reference)
void launch_fill(int n, double v, double *x, hipStream_t st);
void launch_copy(int n, const double *x, double *y, hipStream_t st);
void launch_copy_int(int n, const int *x, int *y, hipStream_t st);  // PMC calibration of 4-byte streams
void launch_spin(double microseconds, hipStream_t st);              // occupies the stream for that long (injected transport latency, tests)
// y = a*x + b*y with host scalars
void launch_axpby(int n, double a, const double *x, double b, double *y, hipStream_t st);
// partial sums of x.y (nblocks returned through *nblk)
void launch_dot(int n, const double *x, const double *y, double *partial, int *nblk, hipStream_t st);

// ---- projection onto mean zero (nullspace_kernels.hip; constant null space): two launches, no host read, no atomics.  x may be any
// 8-byte aligned device pointer.  launch_sum: one partial sum of x per workgroup, *nblk = ns_grid(n) of them (at most 2048).
// launch_project: every workgroup adds the nblk partials in one fixed order, m = S / n, x_i = x_i - m; r non-null: dot_partial gets
// ns_grid(n) partial sums of (x_i - m) * r_i (r any 8-byte aligned pointer); workgroup 0 writes m to *mean_slot.
int ns_grid(int n);
void launch_sum(int n, const double *x, double *partial, int *nblk, hipStream_t st);
void launch_project(int n, const double *partial, int nblk, double *x, const double *r, double *dot_partial, double *mean_slot,
                    hipStream_t st);

// ---- fp32 preconditioner hierarchy (opt-in; SURVEY §8f-4 "mixed precision"): the V-cycle runs on a
// float copy of the sliced-diagonal layout with float vectors, the Krylov loop stays fp64.
struct SdiaF32 {
    int nrow = 0, nslice = 0;
    const int *sd_ptr = nullptr;                  // shared with the fp64 mirror
    const int *sd_off = nullptr;
    const unsigned long long *sd_mask = nullptr;
    float *val = nullptr;                         // per slot 64 floats
    long slots = 0;
};
// op: OP_JACOBI (y = x + omega (b - A x)/d) or OP_RESID (y = b - A x); all vectors float
void launch_sdia_f32(const SdiaF32 &A, CsrOp op, const float *x, const float *b, float *y, float omega, hipStream_t st);
// same two ops for a level that has no sliced-diagonal mirror (thread per CSR row over a float copy of the values)
void launch_csr_f32(const DevCsr &A, const float *val32, CsrOp op, const float *diag, const float *x, const float *b, float *y, float omega,
                    hipStream_t st);
void launch_jacobi_zero_f32(int n, const float *b, const float *d, float omega, float *x, hipStream_t st);
void launch_restrict_f32(int nc, const int *rowptr, const int *col, const double *val, const float *r, float *bc, hipStream_t st);
void launch_prolong_agg_f32(int n, const int *agg, const float *xc, float *xf, hipStream_t st);
void launch_prolong_csr_f32(int n, const int *rowptr, const int *col, const double *val, const float *xc, float *xf, hipStream_t st);
void launch_gemv_f32(int n, const float *M, const float *b, float *x, hipStream_t st);
void launch_cvt_d2f(long n, const double *in, float *out, hipStream_t st);
// z64 = (double) z32 ; partial += z64 * r64   (preconditioned residual back to fp64 + fused z.r)
void launch_cvt_f2d_dot(int n, const float *z32, const double *r64, double *z64, double *partial, int *nblk, hipStream_t st);

// device-resident scalar slots used by the Krylov loops
enum Slot : int {
    S_RZ = 0, S_PAP, S_ALPHA, S_NALPHA, S_BETA, S_RR, S_RES, S_ZR,
    S_ALPHA1, S_APR0, S_ASS, S_ASAS, S_OMEGA1, S_RR0, S_TMP, S_SUM0, S_SUM1,
    S_MEAN,  // the mean the last projection removed (nullspace_kernels.hip)
    S_COUNT
};

// finalize codes: reduce partial arrays, then one thread updates the scalar slots
enum Fin : int {
    FIN_STORE = 0,     // scal[slot_a] = sum0
    FIN_SQRT = 1,      // scal[slot_a] = sqrt(sum0) ; hist[it] = that
    FIN_PCG_ALPHA = 2, // pAp=sum0 ; alpha = rz/pAp ; nalpha = -alpha
    FIN_PCG_BETA = 3,  // zr=sum0 ; beta = zr/rz ; rz = zr
    FIN_CG_BETA = 4,   // rr_new=sum0 ; beta = rr_new/rr ; res = sqrt(rr*beta) ; rr = rr_new ; hist
    FIN_CG_ALPHA = 5,  // pAp=sum0 ; alpha = rr/pAp ; nalpha = -alpha
    FIN_BICG_ALPHA = 6,// alpha1 = sum0 (r.r0) ; apr0 = sum1 (Ap.r0) ; alpha = alpha1/apr0
    FIN_BICG_OMEGA = 7,// ass = sum0 (As.s) ; asas = sum1 (As.As) ; omega1 = ass/asas
    FIN_BICG_BETA = 8, // rr0 = sum0 (r.r0) ; rr = sum1 (r.r) ; beta = rr0/alpha1*(alpha/omega1) ; res = sqrt(rr) ; hist
    FIN_PCG_BETA_RES = 9, // FIN_PCG_BETA on sum0 (z.r) and res = sqrt(sum1) (r.r) ; hist
    FIN_FCG_BETA = 10     // flexible CG: rz = sum0 (z.r) ; beta = -sum1 (z.Ap) / pAp
};
// it >= 0: residual-history slot; it < 0: take the slot from the device counter *iter_ctr (graph replays), which only the codes
// that store a residual advance.  The slot is clamped to hist_cap - 1.
// mode 0: reduce the partials and apply `code` (single GPU); mode 1: reduce only, local sums to
// scal[S_SUM0], scal[S_SUM1] (then all-reduced across ranks); mode 2: apply `code` to those sums
void launch_finalize(Fin code, const double *partial0, const double *partial1, int nblk, double *scal, int slot_a,
                     double *hist, int it, hipStream_t st, int mode = 0, int *iter_ctr = nullptr, int hist_cap = 1 << 30,
                     int nblk1 = -1);  // nblk1: length of partial1 when it differs from nblk
// sendbuf[k] = vec[idx[k]] : pack the entries the peers need (halo exchange)
void launch_pack(int n, const int *idx, const double *vec, double *sendbuf, hipStream_t st);
// vec[pos[k]] = buf[k] : scatter received ghost-layer entries to their local positions (deep-halo exchange)
void launch_unpack(int n, const int *pos, const double *buf, double *vec, hipStream_t st);

// Krylov vector updates with device-resident coefficients (no host round trip)
// PCG/CG: x += alpha p ; r += (-alpha) Ap ; partial += r_i^2
void launch_cg_update(int n, const double *scal, const double *p, const double *Ap, double *x, double *r, double *partial,
                      int *nblk, hipStream_t st);
// the same, and z0 = omega * r / d on the new residual: the zero-guess sweep of the V-cycle that follows (PCG)
void launch_cg_update_zero(int n, const double *scal, const double *p, const double *Ap, double *x, double *r, double *partial,
                           int *nblk, const double *d, double dconst, double omega, double *z0, hipStream_t st, bool nt = false);
// p = 1.0*z + beta*p
void launch_p_update(int n, const double *scal, const double *z, double *p, hipStream_t st);
// x += alpha p ; p = 1.0*z + beta*p  (PCG with the x update moved here: launch_cg_update / _zero are then called with x = nullptr)
void launch_xp_update(int n, const double *scal, const double *z, double *p, double *x, hipStream_t st);
// two dots at once: partial0 += a.b, partial1 += c.d
void launch_dot2(int n, const double *a, const double *b, const double *c, const double *d, double *partial0, double *partial1,
                 int *nblk, hipStream_t st);
// BiCGStab: s = r - alpha*Ap
void launch_bicg_s(int n, const double *scal, const double *r, const double *Ap, double *s, hipStream_t st);
// BiCGStab: x = x + alpha*p1 + omega1*s1 ; r = s - omega1*As ; partial0 += r.r0 ; partial1 += r.r
void launch_bicg_xr(int n, const double *scal, const double *p1, const double *s1, const double *s, const double *As,
                    const double *r0, double *x, double *r, double *partial0, double *partial1, int *nblk, hipStream_t st);
// BiCGStab: p = r + beta*(p - omega1*Ap)
void launch_bicg_p(int n, const double *scal, const double *r, const double *Ap, double *p, hipStream_t st);

// ---- K step of the K-cycle (kcycle_kernels.hip): two flexible-CG steps on a coarse level with everything but the
// two inner cycles and the two SpMVs done here, scalars in device memory.  Slots of the scalar block s (kKcScalDoubles doubles):
enum KcSlot : int { KC_RHO1 = 0, KC_ALPHA1, KC_GAMMA, KC_BETA, KC_ALPHA2, KC_RHO2, KC_K1, KC_K2, KC_Q };
constexpr int kKcScalDoubles = 16;
constexpr int kKcMaxGrid = 512;                      // workgroups of a reducing launch: one per 2048 rows, capped
constexpr int kKcPartialDoubles = 3 * kKcMaxGrid;   // sum k of a launch at partial[k * kKcMaxGrid + workgroup]
int kc_grid(int n);
// partial sums of c.v and c.b (dot2) / of d.v, d.w and d.r (dot3), the first vector read once; return the number of partials per sum
int launch_kc_dot2(int n, const double *c, const double *v, const double *b, double *partial, hipStream_t st);
int launch_kc_dot3(int n, const double *d, const double *v, const double *w, const double *r, double *partial, hipStream_t st);
// one workgroup adds the partials in a fixed order; scal1: rho1, alpha1, q (1 when rho1 is not finite and > 0); scal2: gamma, beta,
// alpha2, rho2 = beta - gamma^2 / rho1, k1 = q - gamma alpha2 / (rho1 rho2), k2 = alpha2 / rho2 -- with rho1 unusable rho2 = 0 and
// k1 = k2 = 1, else with rho2 not finite and > 0 k1 = q and k2 = 0
void launch_kc_scal1(const double *partial, int nblk, double *s, hipStream_t st);
void launch_kc_scal2(const double *partial, int nblk, double *s, hipStream_t st);
// r = b - q v and x = k1 c + k2 d (x may be d), coefficients read from s; every product and sum rounded on its own
void launch_kc_resid(int n, const double *s, const double *b, const double *v, double *r, hipStream_t st);
void launch_kc_combine(int n, const double *s, const double *c, const double *d, double *x, hipStream_t st);

// ---- restarted GMRES (krylov_kernels.hip): block Gram-Schmidt against the basis v_k = V + k * stride and the device-resident
// small problem.  Partial sums are per workgroup, gs_grid(n) of them per sum: sum k at partial[k * gs_grid(n) + workgroup].
// The basis is of double or of float (SPARSH_BASIS_FP32: stored values widened to double before use, every product and sum fp64).
// A float basis wants stride % 4 == 0, 16-byte aligned vectors and zeros in [n, stride) of every vector: its loads are float2 / float4
// and run to the end of the last group of rows.  w, w_in, w_out of the float overloads are 16-byte aligned and hold n doubles.
constexpr int kGmresMaxRestart = 64;  // restart lengths 1..64
constexpr int kGsMaxK = 16;           // basis vectors one launch orthogonalises against (partial sums a thread keeps in registers)
int gs_grid(int n);
// partial[k] <- v_k . w for k < nv; ww_partial (nullptr: not wanted) <- w . w.  nv > kGsMaxK: one launch per chunk.
void launch_gs_dot(int n, long stride, const double *V, int nv, const double *w, double *partial, double *ww_partial, hipStream_t st);
void launch_gs_dot(int n, long stride, const float *V, int nv, const double *w, double *partial, double *ww_partial, hipStream_t st);
// w_out = w_in - sum_k h[k] v_k, k ascending, h in device memory (w_in == nullptr: from zero; w_in may be w_out);
// partial (nullptr: not wanted)[k] <- v_k . w_out, ww_partial (nullptr: not wanted) <- w_out . w_out.
// nv > kGsMaxK: update-only launches per chunk, then launch_gs_dot -- the same values.
void launch_gs_update(int n, long stride, const double *V, int nv, const double *h, const double *w_in, double *w_out, double *partial,
                      double *ww_partial, hipStream_t st);
void launch_gs_update(int n, long stride, const float *V, int nv, const double *h, const double *w_in, double *w_out, double *partial,
                      double *ww_partial, hipStream_t st);
// out[k] = partial[k * nblk .. + nblk) added in a fixed order, one workgroup per k < rows
void launch_gs_finalize(const double *partial, int nblk, int rows, double *out, hipStream_t st);
// v = v / *d ; v = 0 when *d is not > 0
void launch_gs_scale(int n, double *v, const double *d, hipStream_t st);
// float basis: v = (float)(w / *d), vd = that float widened back to double (n doubles); zeros when *d is not > 0
void launch_gs_scale(int n, const double *w, float *v, double *vd, const double *d, hipStream_t st);
// device-resident state of one restart cycle
struct GmresState {
    double *hcol = nullptr, *ccol = nullptr;  // V^T w of the first / second Gram-Schmidt pass (kGmresMaxRestart + 2 each)
    double *R = nullptr;                      // rotated Hessenberg columns, column j at R + j * kGmresMaxRestart
    double *cs = nullptr, *sn = nullptr;      // Givens rotations
    double *g = nullptr;                      // rotated right-hand side (kGmresMaxRestart + 1)
    double *ny = nullptr;                     // -y of the last launch_gmres_solve
    double *hnext = nullptr;                  // h_{j+1} of the last step
};
constexpr int kGmresStateDoubles = 2 * (kGmresMaxRestart + 2) + kGmresMaxRestart * kGmresMaxRestart + 4 * kGmresMaxRestart + 2;
// end of inner iteration j: column h = hcol + ccol, h_{j+1} = sqrt(sum of ww_partial[0, nblk)), rotations, hist[slot] = |g_{j+1}|;
// j == 0 takes g_0 from *beta
void launch_gmres_step(int j, const double *ww_partial, int nblk, const GmresState &s, const double *beta, double *hist, int slot,
                       hipStream_t st);
// ny = -R^{-1} g over the first k columns (zero pivot: that y is 0)
void launch_gmres_solve(int k, const GmresState &s, hipStream_t st);

// ---- block of up to 8 right-hand sides (multi_kernels.hip).  A block of W = 2, 4 or 8 vectors is row-interleaved:
// element (row i, column c) at v[i * W + c].  Per column the arithmetic is that of the single-vector kernels above; reducing launches
// write one partial per column and workgroup to partial[c * nblk + workgroup] and return nblk.
constexpr int kMultiMax = 8;  // SPARSH_MAX_RHS
constexpr int kMultiGridMax = 2048;  // workgroups of a grid-stride elementwise block kernel: ~8 per CU
inline int multi_width(int nrhs) { return nrhs <= 2 ? 2 : (nrhs <= 4 ? 4 : 8); }
struct MultiArgs {
    const double *x = nullptr;  // input block (gathered)
    const double *b = nullptr;  // RESID / JACOBI (may be y: element i is read before it is written, by the same thread)
    const double *d = nullptr;  // JACOBI: the level's diagonal, one entry per row
    double *y = nullptr;        // output block (ADD: read and written)
    double omega = 0.0;
    double *partial = nullptr;  // SPMV_DOT: W * nblk partial sums of x_c . (A x)_c
};
// OP_SPMV, OP_SPMV_DOT, OP_RESID, OP_JACOBI or OP_ADD on A's CSR arrays and row-block records; a row longer than kStreamNnz is summed
// in stored order, chunk by chunk.  Blocks must be 16-byte aligned (a lane owns two neighbouring columns).  multi_placement: the
// non-temporal / XCD-remap choice of the launch under cfg, the rule of csr_placement applied to the bytes one block sweep streams.
int launch_csr_multi(const DevCsr &A, int W, CsrOp op, const MultiArgs &a, hipStream_t st, const KernelConfig &cfg);
void multi_placement(const DevCsr &A, int W, const KernelConfig &cfg, bool *nt, int *remap);
// column-major (column c at B + c * ld) <-> interleaved; the padding columns nrhs .. W - 1 are written as zeros / not read
void launch_interleave(int n, int nrhs, int W, const double *B, long ld, double *v, hipStream_t st);
void launch_deinterleave(int n, int nrhs, int W, const double *v, double *X, long ld, hipStream_t st);
// launch_jacobi_zero / launch_prolong_agg / launch_restrict_agg / launch_gemv per column (gemv: the inverse is read once for all columns)
void launch_jacobi_zero_multi(int n, int W, const double *b, const double *d, double dconst, double omega, double *x, hipStream_t st);
void launch_prolong_agg_multi(int n, int W, const int *agg, const double *xc, double *xf, hipStream_t st);
void launch_restrict_agg_multi(int nc, int W, const int *rowptr, const int *col, const double *r, double *bc, hipStream_t st);
void launch_gemv_multi(int n, int W, const double *M, const double *b, double *x, hipStream_t st);
// device-resident state of block PCG: scal[slot * kMultiMax + c], and per column whether it is frozen, its iteration count and status
enum MultiSlot : int { MS_RZ = 0, MS_PAP, MS_ALPHA, MS_NALPHA, MS_BETA, MS_RES, MS_TMP, MS_COUNT };
constexpr int kMultiStatusNumeric = 1;  // status of a column frozen on a NaN residual (0: converged or still running)
struct MultiState {
    double *scal = nullptr;  // MS_COUNT * kMultiMax
    int *frozen = nullptr, *iters = nullptr, *status = nullptr;  // kMultiMax each
};
enum MultiFin : int {
    MFIN_STORE = 0,    // scal[slot][c] = sum0
    MFIN_INIT = 1,     // res = sqrt(sum0); freezes the padding columns and the columns with res <= tol (iters 0) or a NaN
    MFIN_ALPHA = 2,    // FIN_PCG_ALPHA per column
    MFIN_BETA_RES = 3  // FIN_PCG_BETA_RES per column; on a column that is not frozen: hist[c * hist_cap + it] = res, iters = it + 1, and the freeze
};
int launch_dot_multi(int n, int W, const double *x, const double *y, double *partial, hipStream_t st);
// x += alpha_c p ; r += (-alpha_c) Ap on the columns that are not frozen (predicated writes) ; partials of r.r
int launch_cg_update_multi(int n, int W, const MultiState &s, const double *p, const double *Ap, double *x, double *r, double *partial, hipStream_t st);
// p = 1.0 z + beta_c p on the columns that are not frozen
void launch_p_update_multi(int n, int W, const MultiState &s, const double *z, double *p, hipStream_t st);
// one workgroup: p0 (W x n0 partials) and p1 (W x n1, may be nullptr) added per column in a fixed order, then `code`
void launch_finalize_multi(MultiFin code, int W, int nrhs, const double *p0, int n0, const double *p1, int n1, const MultiState &s, int slot,
                           double tol, double *hist, int hist_cap, int it, hipStream_t st);

// ---- LOBPCG eigensolver on interleaved blocks (eig_kernels.hip).  Every product and sum is rounded on its own;
// reducing launches write one partial per sum and workgroup, eig_grid(n, W) of them, and combine them in a fixed order.
constexpr int kEigPairs = 12;     // block pairs of one Gram launch: the upper block triangles of S^T S and S^T A S, S = [X, W, P]
constexpr int kEigMaxGrid = 512;  // workgroups (per pair) of a launch: one per 512 / W rows, capped
int eig_grid(int n, int W);
struct GramPairs {
    const double *u[kEigPairs], *v[kEigPairs];  // pair p: U^T V of the blocks u[p], v[p] (n x W, interleaved; may be one block)
    int dst[kEigPairs];                         // offset of its W x W result in G
};
// G[dst[p] + a * ldg + b] = sum_i u[p]_ia v[p]_ib for p < npairs, one launch for all pairs (blockIdx.y) and one that adds the partials;
// partial holds npairs * W * W * eig_grid(n, W) doubles.  Returns the number of partials per sum.
int launch_gram_multi(int n, int W, int npairs, const GramPairs &prs, double *partial, double *G, int ldg, hipStream_t st);
// R = AX - X * theta_c with theta in device memory, norms[c] = ||R_c||_2 (partial: W * eig_grid(n, W) doubles)
void launch_eig_residual(int n, int W, const double *AX, const double *X, const double *theta, double *R, double *partial, double *norms,
                         hipStream_t st);
// the subspace update on the columns j < k, coef = Cx, Cw, Cp (W x W each, row-major, device memory), every sum over c < k ascending:
//   P'_ij = sum_c W_ic Cw_cj, continued by + sum_c P_ic Cp_cj ;  X'_ij = (sum_c X_ic Cx_cj) + P'_ij ;  AP', AX' likewise from AW, AP, AX.
// Columns j >= k are written as zeros.  An output may be the block it replaces.
void launch_eig_update(int n, int W, int k, const double *X, const double *Wb, const double *P, const double *AX, const double *AW,
                       const double *AP, const double *coef, double *Xo, double *Po, double *AXo, double *APo, hipStream_t st);

// the pencil (A, B): R = AX - BX * theta_c, rnorms[c] = ||R_c||_2 and bnorms[c] = ||BX_c||_2 from one pass (partial: 2 W * eig_grid(n, W)
// doubles).  rnorms has the bits launch_eig_residual gives for the same R.
void launch_eig_residual_gen(int n, int W, const double *AX, const double *BX, const double *theta, double *R, double *partial, double *rnorms,
                             double *bnorms, hipStream_t st);
// launch_eig_update with B S carried along.  in = X, W, P, AX, AW, AP, BX, BW, BP; out = X', P', AX', AP', BX', BP' with BP' = BW Cw + BP Cp
// and BX' = BX Cx + BP'.  An output may be the block it replaces.
void launch_eig_update_gen(int n, int W, int k, const double *const in[9], const double *coef, double *const out[6], hipStream_t st);

// ---- constraints of the LOBPCG eigensolver (eig_con_kernels.hip).  The mt <= kEigConMax constraints are ceil(mt / W) interleaved
// blocks of width W, block b at Y + b * n * W, constraint j in column j % W of block j / W, zeros past mt.
constexpr int kEigConMax = 17;  // SPARSH_MAX_CON and the implicit constant of a null-space handle
// dst = src - Y Ginv (BY)^T src by the Gram launch with its finalise and one more kernel: C = (BY)^T src (mt x W row-major; room for ceil(mt / W) * W * W doubles) by the Gram
// launch (partial: ceil(mt / W) * W * W * eig_grid(n, W) doubles), then the apply with coef = Ginv C (Ginv mt x mt row-major, device)
// formed by every workgroup, sums over j ascending.  dst may be src; BY may be Y.
void launch_eig_con_project(int n, int W, int mt, const double *Y, const double *BY, const double *Ginv, const double *src, double *dst,
                            double *C, double *partial, hipStream_t st);
// column col of the interleaved block v <- value
void launch_eig_con_fill_column(int n, int W, int col, double value, double *v, hipStream_t st);

// ---- the orthonormalised basis of the LOBPCG eigensolver (eig_ortho_kernels.hip; SPARSH_EIG_BASIS_ORTHO).  Masks are W doubles in
// device memory, 1.0 in and 0.0 out; small matrices are W x W row-major.  No launch here reduces over rows or uses atomics.
// masks[c] = rn_c > tol |theta_c| (gen: > (tol |theta_c|) bn_c) for c < k, 0 past k; masks[W .. 3 W) (the masks of W and P) are cleared
void launch_eig_active_mask(int W, int k, bool gen, double tol, const double *theta, const double *rn, const double *bn, double *masks,
                            hipStream_t st);
// eig_chol of eig_chol.hpp on one wavefront: T and mask_out from the upper triangle of G and mask_in (mask_out may be mask_in)
void launch_eig_chol_small(int W, const double *G, const double *mask_in, double *T, double *mask_out, hipStream_t st);
// V <- V T in place on the nb <= 3 blocks V[0 .. nb), sums over c < k ascending, columns j >= k written as zeros
void launch_eig_transform(int n, int W, int k, int nb, double *const V[3], const double *T, hipStream_t st);
// dst = src - X C on the columns c < k of the mask (sum over j < k ascending, one subtraction), exact zeros elsewhere; dst may be src
void launch_eig_ortho_apply(int n, int W, int k, const double *X, const double *C, const double *mask, const double *src, double *dst,
                            hipStream_t st);

// ---- block CG on interleaved blocks (bcg_kernels.hip).  The columns of a block share one search space: the
// scalars of block PCG become W x W matrices (row-major, device memory), solved for by bcg_small.hpp's LDL^T with dropped directions.
constexpr int kBcgMaxGrid = 2048;  // workgroups of the two streaming kernels: one per 512 / W rows, capped at ~8 per CU
int bcg_grid(int n, int W);
enum BcgFlag : int {
    BF_KEEP = 0,       // 8 ints: the keep mask of the last factorisation
    BF_RANK = 8,       // its rank
    BF_MIN_RANK = 9,   // the smallest rank of the solve so far
    BF_DROPPED = 10,   // directions dropped, all iterations together
    BF_DONE = 11,      // the solve is over: every kernel of the loop leaves at once
    BF_NUMERIC = 12,   // ... because of a NaN residual or a Gram matrix of rank 0
    BF_ITERS = 13,     // iterations completed
    BF_COUNT = 16
};
struct BcgState {
    double *L = nullptr;    // 64: the unit lower factor (8 x 8 row-major whatever W)
    double *d = nullptr;    // 8: its pivots
    double *res = nullptr;  // 8: the last residual norms
    int *flags = nullptr;   // BF_COUNT
};
// coef (W x W) = sign * pinv(G) C for the k columns in use.  factor: factorise G and keep the factor in s; else reuse the kept one.
void launch_bcg_small(int W, int k, bool factor, const double *G, const double *C, double sign, const BcgState &s, double *coef, int it,
                      hipStream_t st);
// X' = X + P alpha ; R' = R - Q alpha ; partial[c * grid + workgroup] = shares of ||R'_c||^2 (W * bcg_grid(n, W) doubles).  Xo may be X,
// Ro may be R.  done (may be nullptr): device flag that turns the launch into a no-op.  Returns the partials per column.
int launch_bcg_update(int n, int W, int k, const int *done, const double *X, const double *R, const double *P, const double *Q,
                      const double *alpha, double *Xo, double *Ro, double *partial, hipStream_t st);
// P' = Z + P beta; Po may be P
void launch_bcg_dir(int n, int W, int k, const int *done, const double *Z, const double *P, const double *beta, double *Po, hipStream_t st);
// res_c = sqrt of the sum of column c's partials; it < 0: start of a solve (flags reset), else the end of iteration it + 1 with
// hist[c * hist_cap + it] = res_c; done when every res_c <= tol, numeric on a NaN
void launch_bcg_finalize(int W, int nrhs, const double *partial, int nblk, const BcgState &s, double tol, double *hist, int hist_cap, int it,
                         hipStream_t st);

// ---- block BiCGStab on interleaved blocks (mbicg_kernels.hip).  Per column the arithmetic of the single
// BiCGStab kernels; the columns are frozen one by one as in block PCG.  scal[slot * kMultiMax + c]; frozen / iters / status as in
// MultiState (status kMultiStatusNumeric for a column frozen on a NaN residual).
enum MbicgSlot : int { MB_ALPHA1 = 0, MB_APR0, MB_ALPHA, MB_ASS, MB_ASAS, MB_OMEGA1, MB_BETA, MB_RR0, MB_RES, MB_COUNT };
struct MbicgState {
    double *scal = nullptr;  // MB_COUNT * kMultiMax
    int *frozen = nullptr, *iters = nullptr, *status = nullptr;  // kMultiMax each
};
enum MbicgFin : int {
    MBFIN_INIT = 0,     // res = sqrt(sum0); scalars zeroed; freezes the padding columns and the columns with res <= tol (iters 0) or a NaN
    MBFIN_ALPHA = 1,    // FIN_BICG_ALPHA per column that is not frozen: alpha1 = sum0 ; apr0 = sum1 ; alpha = alpha1 / apr0
    MBFIN_OMEGA = 2,    // FIN_BICG_OMEGA: ass = sum0 ; asas = sum1 ; omega1 = asas == 0 ? 0 : ass / asas
    MBFIN_BETA_RES = 3  // FIN_BICG_BETA: beta = sum0 / alpha1 * (alpha / omega1) ; rr0 = sum0 ; res = sqrt(sum1) ; hist[c * hist_cap + it]
                        // (it < hist_cap), iters = it + 1, and the freeze
};
// workgroups of the S and P launches: one per 512 / W rows, at most kMultiGridMax (grid-stride beyond)
int mbicg_grid(int n, int W);
// workgroups of the two reducing launches, where a lane owns a row: the grid of the single-vector elementwise kernels, one per 512
// rows, at most kMultiGridMax
int mbicg_reduce_grid(int n);
// part0[c * g + w] / part1[c * g + w]: workgroup w's shares of a_c . b_c / c_c . d_c (W * g doubles each; the blocks may be one
// another).  Returns g = mbicg_reduce_grid(n), as launch_bicg_xr_multi does.
int launch_dot2_multi(int n, int W, const double *a, const double *b, const double *c, const double *d, double *part0, double *part1,
                      hipStream_t st);
// S = R - alpha_c AP
void launch_bicg_s_multi(int n, int W, const MbicgState &s, const double *R, const double *AP, double *S, hipStream_t st);
// X = (X + alpha_c P1) + omega_c S1 ; R = S - omega_c AS ; part0: shares of R_c . R0_c ; part1: shares of R_c . R_c
int launch_bicg_xr_multi(int n, int W, const MbicgState &s, const double *P1, const double *S1, const double *S, const double *AS,
                         const double *R0, double *X, double *R, double *part0, double *part1, hipStream_t st);
// P = R + beta_c (P - omega_c AP)
void launch_bicg_p_multi(int n, int W, const MbicgState &s, const double *R, const double *AP, double *P, hipStream_t st);
// one workgroup: column c's partials of p0 (n0 of them) and p1 (n1; p1 may be nullptr: sum1 = 0) added in a fixed order, then `code`
void launch_finalize_mbicg(MbicgFin code, int W, int nrhs, const double *p0, int n0, const double *p1, int n1, const MbicgState &s, double tol,
                           double *hist, int hist_cap, int it, hipStream_t st);

}  // namespace sparsh
