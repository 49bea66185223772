// engine.hpp -- device-resident AMG hierarchy + V-cycle + Krylov loops (single GPU).
// Mirrors the behaviour of AMG_GPU1_solver ("MI": whole hierarchy resident,
// src/AMG_gpu_phases_2.cu:13-240) with the arithmetic of the CPU path
// (src/AMG_phases.cpp:151-230, src/AMG_main_solvers.cpp:47-458).
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "../../include/sparsh_amg.h"
#include "cheby_bounds.hpp"
#include "coarse.hpp"
#include "comm.hpp"
#include "dist.hpp"
#include "host_setup.hpp"
#include "kernels.hpp"

namespace sparsh {

struct DevLevel {
    // ---- deep-halo layout of a partitioned level (communication-avoiding smoothing, dist.hpp): the operator A
    // and the vectors x, x2, b carry the own rows, padding to a slice boundary and K ghost layers
    bool deep = false;
    int K = 0;                       // ghost layers (sweeps + 1)
    int npad = 0;                    // own rows rounded up to 64 = first ghost index
    std::vector<int> layer_end;      // layer_end[d] = local indices in layers 0..d
    DevDeepPlan dplan[3];            // exchange of ghost layers <= 1, <= K-1, <= K
    std::vector<int> blk_first, wblk_first;  // first row of every CSR row block / wave block (prefix launches)
    double *xc_stage = nullptr;      // prolongation input [own x_{l+1} | planP halo] (x_{l+1}'s own tail holds A's ghosts)
    double *b_ext = nullptr;         // level 0: the right-hand side with room for its ghost layers
    int n = 0;       // rows this rank holds (all of them on a replicated level)
    int nglob = 0;   // rows of the level
    bool replicated = true;  // every rank holds and computes the whole level
    DevPlan planA, planP, planR;  // halo plans of A_l x, P_l x_{l+1}, R_l r_l (empty on one GPU)
    DevCsr A, P, R;
    bool P_is_aggregation = false;
    int *members = nullptr;        // aggregates of at most two rows that are not such pairs: (first, second or -1) per coarse row, for the
                                   // coarser level's last post-sweep to prolongate into this level itself (OP_JACOBI_PROLONG)
    int pair_axis = 0;             // box-grid level whose aggregate J (lexicographic in the coarse box; < 0: from its far end) = grid point + its neighbour one line (1) /
                                   // one plane (2) up: residual + restriction without r and R (box_resid_pair_kernel)
    bool pair_aggregates = false;  // aggregate J = fine rows (2J, 2J+1) in R's stored order: residual + restriction fuse (OP_RESID_PAIR)
    double *diag = nullptr;
    double box1_table_us = 0.0, box1_us = 0.0;        // setup timing of the last post-sweep + dot: table kernel / plane-marching kernel
    double box_single_us = 0.0, box_double_us = 0.0;  // setup timing of two single sweeps / one double sweep (tune_box_kernels), 0 = not timed
    bool diag_is_const = false;  // every (own) row has the same diagonal entry, diag_const
    double diag_const = 0.0;
    double *x = nullptr, *x2 = nullptr;  // ping-pong solution buffers (Jacobi reads old, writes new)
    double *b = nullptr;                 // rhs of this level (level 0: points at the caller's vector)
    double *r = nullptr;                 // residual
    bool fine = false;                   // finest level of the hierarchy
};

// Device layout of one level for the multicolour SOR smoother: a colour-compacted copy of the operator (rows colour by colour,
// ascending inside a colour; col / val in stored order), so that each colour's launch streams one contiguous block.
struct SorLevel {
    int n = 0, ncolors = 0;
    std::vector<int> cstart;     // host copy: ncolors + 1 compacted row offsets
    std::vector<int> blk_first;  // ncolors + 1: first row-block record of every colour
    int *dcstart = nullptr, *rows = nullptr, *rowptr = nullptr, *col = nullptr, *rec = nullptr;
    double *val = nullptr, *diag = nullptr;
    bool nt = false;      // the per-colour launches stream the matrix past the caches (level larger than the Infinity Cache)
    bool single = false;  // small level: a whole leg is one launch (launch_sor_level)
    size_t bytes = 0;     // device bytes of the layout
};

// Chebyshev smoother state of one level: the spectral bounds (host, computed on first use after setup_host) and the
// correction vector d of the three-term recurrence (device, allocated on first use after setup)
struct ChebyLevel {
    bool have = false;    // est holds the bounds of the current hierarchy and Lanczos step count
    ChebyBounds est;
    double forced = 0.0;  // > 0: the caller's upper bound (sparsh_set_chebyshev_lmax) replaces est.lmax
    double *d = nullptr;
    double lmax() const { return forced > 0.0 ? forced : est.lmax; }
};

// Extra vectors of one WK level (a level where the W- or the K-cycle recurses twice): the first inner cycle's result c, v = A_l c (K
// only) and the right-hand side r of the second inner cycle.  Allocated at the first cycle that needs them.
struct WkLevel {
    double *c = nullptr, *v = nullptr, *r = nullptr;
};

struct KrylovState {
    bool active = false, precond = false;
    const double *b = nullptr;
    double *x = nullptr;
    int count = 0;
    double r1 = 0.0;
};

// what every entry point of the fp32 cycle answers (SPARSH_ESTATE) on a handle that has no float hierarchy
inline constexpr const char *kF32NotBuilt = "the fp32 preconditioner hierarchy was not built (sparsh_params.precond_fp32 = 0, or a single level)";

// float mirror of one level for the opt-in fp32 preconditioner
struct F32Level {
    SdiaF32 A;
    float *csr_val = nullptr;  // float copy of the CSR values on levels without the sliced-diagonal mirror
    float *diag = nullptr, *x = nullptr, *x2 = nullptr, *b = nullptr, *r = nullptr;
};

struct GraphState {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    double *x = nullptr;  // solution vector the captured iteration updates
    bool precond = false;
};

// HIP-event timing of the dominant kernel inside a solve: one event pair brackets each RUN of consecutive
// fused Jacobi launches on the finest level (the 6-7 sweeps of a smoothing leg), so the cost of the event
// packets themselves is spread over the run instead of being charged to every launch (an event pair
// around each single launch reads ~10 us high).
struct ProfileData {
    bool enabled = false;
    std::vector<hipEvent_t> ev;      // pairs
    std::vector<int> run_launches;   // launches bracketed by pair k
    size_t used = 0;
    double launches = 0, seconds = 0;
};

class Engine {
public:
    Engine(int nrow, int ncol, const int *rowptr, const int *col, const double *val);
    ~Engine();

    int setup_host(const sparsh_params &p);  // hierarchy on the host only (no device needed)
    // multi-GPU: rank 0 runs setup_host and the other ranks receive its hierarchy through the transport instead of
    // repeating the same setup (set_share_setup(false): every rank builds its own, as in round 1)
    int setup_host_shared(const sparsh_params &p);
    void set_share_setup(bool on) { share_setup_ = on; }
    bool built_locally() const { return built_locally_; }
    size_t shared_image_bytes() const { return image_bytes_; }
    int setup(const sparsh_params &p);       // setup_host + upload to HBM
    bool ready() const { return ready_; }
    bool host_ready() const { return host_ready_; }
    int nlevels() const { return (int)lev_.size(); }
    const HostHierarchy &host() const { return H_; }
    const CoarseSolver &coarse() const { return coarse_; }
    CoarseSolver &coarse_mut() { return coarse_; }
    const sparsh_params &params() const { return prm_; }
    // ---- smoother (SPARSH_SMOOTH_JACOBI default / SPARSH_SMOOTH_SOR / SPARSH_SMOOTH_CHEBYSHEV): sweeps 0 = default (params.sweeps / 6 /
    // degree 4)
    void set_smoother(int kind, int sweeps, int order);
    int smoother() const { return smoother_; }
    bool jacobi_on() const { return smoother_ == SPARSH_SMOOTH_JACOBI; }
    bool sor_on() const { return smoother_ == SPARSH_SMOOTH_SOR; }
    int sor_sweeps() const { return sm_sweeps_ > 0 ? sm_sweeps_ : kSorDefaultSweeps; }
    int sor_order() const { return sor_order_; }
    // debug knob: 0 the level policy (single launch up to kSorSingleNnz entries), 1 per-colour launches on every level, 2 one launch on every level
    void set_sor_path(int mode) { sor_path_ = mode; }
    // colour classes of level l (host; computed on first use after setup_host)
    const ColorClasses &level_colors(int l);
    const SorLevel *sor_level(int l) const { return l >= 0 && l < (int)sor_.size() && sor_[l].rows ? &sor_[l] : nullptr; }
    bool sor_single(int l) const { return sor_path_ == 2 || (sor_path_ == 0 && sor_[l].single); }  // a leg of level l is one launch
    // `sweeps` SOR sweeps of level l on x in place (colours C..1 when reverse), issued as a smoothing leg issues them
    void sor_leg(int l, const double *b, double *x, int sweeps, bool reverse);
    // the same as a test hook on any level whatever the smoother (x_is_zero: x is taken as 0); false if the layouts cannot be built
    bool op_sor(int l, const double *b, double *x, int sweeps, bool reverse, bool x_is_zero);
    bool build_sor_level(int l);  // layout of level l alone, the coarsest included (op_sor / bench); no-op once built for the current setup
    // ---- Chebyshev polynomial smoother (cheby_bounds.hpp)
    bool cheby_on() const { return smoother_ == SPARSH_SMOOTH_CHEBYSHEV; }
    int cheby_degree() const { return sm_sweeps_ > 0 ? sm_sweeps_ : kChebyDefaultDegree; }
    double cheby_ratio() const { return cheby_ratio_; }
    int cheby_steps() const { return cheby_steps_; }
    void set_chebyshev(double ratio, int steps);  // a changed step count drops the computed bounds
    // bounds of level l (host; computed on first use after setup_host -- at the setup for the smoothed levels, every level but the
    // coarsest, when Chebyshev was selected before it; the coarsest level's serve op_cheby and the bench alone)
    const ChebyLevel &level_cheby(int l);
    void set_cheby_lmax(int l, double lmax);  // 0: back to the estimate
    bool build_cheby_level(int l);  // bounds + d vector of level l alone (op_cheby / bench)
    // one leg of `degree` steps on level l: iterate in lev_[l].x on entry and exit (x_zero: taken as 0, not read), lev_[l].x2 is scratch;
    // dot_partial: the last step also leaves the partial sums of x.b there
    void cheby_leg(int l, const double *b, bool x_zero, int degree, double *dot_partial, int *dot_nblk);
    // the same as a test hook on caller vectors, whatever the smoother; false if the level's state cannot be built
    bool op_cheby(int l, const double *b, double *x, double *tmp, int degree, bool x_is_zero);
    // bench: one step of the k >= 1 form on the level's resident buffers (x, x2, d; r as the right-hand side)
    void cheby_bench_step(int l);
    // ---- W- and K-cycles at chosen levels.  Level l is a WK level when 1 <= l < last and l % stride == 0; there
    // the coarse problem is solved by two inner cycles (W: the second on the residual of the first; K: two flexible-CG steps).
    static constexpr int kCycleDefaultStride = 3;
    static constexpr long kCycleMaxVisits = 1024;  // level visits of one cycle, all levels together
    void set_cycle(int kind, int stride)
    {
        cycle_kind_ = kind;
        cycle_stride_ = stride;
        config_changed();
    }
    int cycle_kind() const { return cycle_kind_; }
    int cycle_stride() const { return cycle_stride_; }
    // host-side counts of the hierarchy built by setup_host, under the current kind and stride (kind V: no WK level, one visit each)
    bool wk_level(int l) const { return wk_level_for(l, cycle_stride_); }
    long level_visits(int l) const { return level_visits_for(l, cycle_stride_); }
    long cycle_visits() const { return cycle_visits_for(cycle_stride_); }
    int wk_level_count() const;
    size_t wk_bytes() const { return wk_bytes_; }
    // ---- constant null space (SPARSH_NULLSPACE_CONSTANT).  The kind asked for is read by the next setup; the
    // hierarchy remembers the kind it was built with (H_.nullspace), and only that one steers the solve path
    void set_nullspace(int kind) { ns_kind_ = kind; }
    int nullspace_built() const { return host_ready_ ? H_.nullspace : SPARSH_NULLSPACE_NONE; }
    bool ns_on() const { return nullspace_built() == SPARSH_NULLSPACE_CONSTANT; }
    int pinned_row() const { return host_ready_ ? H_.pinned_row : -1; }
    double row_defect() const { return host_ready_ ? ns_row_defect_ : 0.0; }
    double col_defect() const { return host_ready_ ? ns_col_defect_ : 0.0; }
    // v -= mean(v) on a level-0 vector through launch_sum + launch_project; r non-null: the partial sums of (v - mean) . r go to
    // dot_partial and their number to *dot_nblk, for finalize.  The mean removed stays in scal_[S_MEAN].
    void project(double *v, const double *r = nullptr, double *dot_partial = nullptr, int *dot_nblk = nullptr);
    // the same two launches on any device vector of n elements (bench); part: ns_grid(n) doubles of scratch
    void project_any(int n, double *v, const double *r, double *part, double *dot_partial, int *dot_nblk);
    // test hook: the two launches on any 8-byte aligned device vector with scratch of its own; *mean = the mean removed and, with r,
    // *dot = (v - mean) . r through the engine's final reduction (either pointer may be null); SPARSH_* code
    int op_project(int n, double *v, const double *r, double *mean, double *dot);
    // whether `method` can run under the current cycle on this handle: SPARSH_OK, or SPARSH_EINVAL with the reason in error.  Needs no
    // device; the visit cap is checked once the hierarchy exists.  SPARSH_AMG stands for every caller that takes a preconditioner
    // which changes from one application to the next (the stand-alone iteration, op_precond)
    int cycle_check(int method);
    // cycle_check and the extra vectors of the WK levels (every solver entry calls it next to smoother_prepare)
    int cycle_prepare(int method);
    // test hook: the K step's own launches on caller vectors of level l (device): v = A c, the two sums, q, r = b - q v; w = A d, the
    // three sums, the scalars, x = k1 c + k2 d; scal8 = {rho1, alpha1, gamma, beta, alpha2, rho2, k1, k2}
    int op_kstep(int l, const double *b, const double *c, const double *d, double *r, double *x, double *scal8);
    // SOR layouts / Chebyshev bounds and d vectors of the smoothed levels (all but the coarsest) ready for a solve on this handle, built
    // now if the smoother was chosen after setup; SPARSH_* code (every solver entry calls it)
    int smoother_prepare();
    static constexpr int kSorDefaultSweeps = 6;  // AMG_solve_SOR's count (src/AMG_phases.cpp:252)
    // levels with at most this many entries run a leg as one launch: 0, the single launch was slower than the per-colour launches on
    // every level measured on the MI355X, down to 3 774 rows / 25 940 entries
    static constexpr long kSorSingleNnz = 0;
    // kernel-family / layout choices of THIS handle (const_slots is read when the layouts are built)
    // (mutable access is for the C ABI's setters, which call config_changed() afterwards)
    KernelConfig &kernel_cfg() { return cfg_; }
    const KernelConfig &kernel_cfg() const { return cfg_; }
    // a captured hipGraph of the iteration replays the kernels of the configuration it was captured under: drop it
    void config_changed() { drop_graph(); }
    // diag[] of a level for the kernels that only divide by it: nullptr (+ diag_const) where it is one constant
    const double *diag_stream(const DevLevel &L) const { return cfg_.const_diag && L.diag_is_const ? nullptr : L.diag; }
    // a smoothing leg of this level that starts from a zero guess runs sweeps 1 - 3 as one launch reading b alone
    bool zero_start(const DevLevel &L) const { return cfg_.zero_start && (!dist_ || L.replicated) && !L.deep && box2_applies(L.A, cfg_); }
    // whether level l's last post-sweep also prolongates into level l - 1 (OP_JACOBI_PROLONG)
    bool level_prolong_fused(int l) const
    {
        if (l < 1 || l + 1 >= (int)lev_.size() || !cfg_.fuse_prolong || prm_.sweeps < 1 || prm_.precond_fp32) return false;
        const DevLevel &F = lev_[l - 1];
        if (dist_ && !F.replicated) return false;  // several GPUs: between replicated levels only
        return F.P_is_aggregation && !F.deep && (F.pair_aggregates || F.members) && F.R.nrow == lev_[l].n;
    }
    // whether level l's residual, restriction and the next level's zero-guess sweep run as one launch (OP_RESID_PAIR)
    // 0 no; 1 aggregates = row pairs (2J, 2J+1): OP_RESID_PAIR of the table kernel; 2 / 3 box-grid level paired along y / z
    int level_paired(int l) const
    {
        if (!(l + 2 < (int)lev_.size() && prm_.sweeps > 0 && (!dist_ || lev_[l].replicated) && cfg_.pair_restrict)) return 0;
        if (lev_[l].pair_aggregates && resid_pair_applies(lev_[l].A, cfg_)) return 1;
        if (lev_[l].pair_axis != 0 && lev_[l].A.box_nx > 0 && csr_family(lev_[l].A, cfg_) == FAM_SDIA_TAB) return 1 + std::abs(lev_[l].pair_axis);
        return 0;
    }
    // average seconds of one communication step alone (collective: every rank calls it): what = 0 halo
    // exchange of level `level`'s operator, 1 the 16-byte all-reduce of the fused scalars, 2 the
    // all-gather at the partitioned -> replicated boundary.  -1 when the step does not exist.
    double bench_comm(int what, int level, int reps);
    hipStream_t stream() const { return st_; }
    double *partials() const { return part0_; }  // one slot per workgroup of a reducing launch (part_cap_ of them)
    const DevLevel &level(int l) const { return lev_[l]; }
    int n0() const { return A0_.nrow; }
    int local_n0() const { return lev_.empty() ? A0_.nrow : lev_[0].n; }
    // multi-GPU: install the transport before setup(); the engine owns it
    void set_comm(std::unique_ptr<Comm> c) { comm_ = std::move(c); }
    void set_overlap(bool on) { overlap_ = on; }
    // deep halo (default on for partitioned runs): one exchange per smoothing leg instead of one per sweep; read at setup
    void set_deep_halo(bool on) { deep_halo_ = on; }
    bool deep_halo() const { return deep_halo_; }
    // Multi-rank setup: measure the transport (neighbour exchange latency and rate, 16-byte all-reduce, all-gather) and the
    // device's sweep rate, then choose from those numbers which levels are partitioned and whether the partitioned levels smooth
    // with deep halos or exchange per sweep (mode 1, default).  Mode 0: replicate_rows / set_deep_halo decide, as in round 2.
    void set_comm_tuning(int mode) { comm_tune_ = mode; }
    struct CommLevelChoice {
        int rows = 0, halo_rows = 0;
        bool partitioned = false, deep = false;
        double cost_deep_us = 0.0, cost_per_sweep_us = 0.0, cost_replicated_us = 0.0;  // modelled time of the level's part of one V-cycle
    };
    struct CommMeasured {
        double exchange_us = 0.0, exchange_us_per_mb = 0.0, allreduce_us = 0.0, allgather_us = 0.0, allgather_us_per_mb = 0.0;
        double sweep_floor_us = 0.0, sweep_us_per_mb = 0.0;
        bool valid = false;
    };
    // host-only: the schedule the tuner would choose for `nranks` ranks from the given measurements (tests, what-if tables)
    void plan_comm_schedule(const sparsh_params &p, int nranks, const CommMeasured &m)
    {
        meas_ = m;
        meas_.valid = true;
        sched_.clear();
        tuned_repl_level_ = -1;
        decide_comm_schedule(p, nranks);
    }
    int tuned_partitioned_levels() const { return tuned_repl_level_; }
    const std::vector<CommLevelChoice> &comm_schedule() const { return sched_; }
    const CommMeasured &comm_measured() const { return meas_; }
    long exchanges_issued() const { return n_exchanges_; }
    // test hook: y[0, rows) = (A_l x_ext)[0, rows) on the local operator of a deep-halo level, no exchange
    bool debug_prefix_spmv(int l, int rows, const double *x_ext, double *y);
    bool overlap() const { return overlap_; }
    Comm *comm() const { return comm_.get(); }
    bool distributed() const { return dist_; }
    bool precond_fp32_active() const { return f32_ready_; }
    const Partition &partition(int l) const { return parts_[l]; }
    void set_stopping(double tol, int max_iter, int check_every)
    {
        prm_.tol = tol;
        if (max_iter > 0) prm_.max_iter = max_iter;
        if (check_every > 0) prm_.check_every = check_every;
    }

    // solvers on device vectors; return SPARSH_* code; iterations through *iters
    int solve_dev(int method, const double *b_dev, double *x_dev, int max_iters, double *hist, int hist_cap, int *iters,
                  double *seconds);
    int amg_solve_dev(const double *b_dev, double *x_dev, int iterations, double *hist, int hist_cap, int *ncycles);

    // stepwise CG / AMG-PCG (bench: time exactly k iterations; engine_krylov.cpp, as everything of the single-vector Krylov methods)
    int pcg_init(const double *b_dev, double *x_dev, bool precond);
    int pcg_steps(int nsteps, int *done);
    int krylov_hist(double *hist, int hist_cap);  // copies the residual history, returns iterations so far
    double krylov_residual() const { return ks_.r1; }
    // why `method` cannot run under the SOR order selected now (nullptr: it can); needs no device
    const char *sor_refusal(int method) const;

    // operator-level (device pointers)
    void op_spmv(int l, const double *x, double *y);
    void op_jacobi(int l, const double *b, double *x, double *tmp, int sweeps, bool x_is_zero);  // result in x
    void op_residual(int l, const double *b, const double *x, double *r);
    double op_resnorm(int l, const double *b, const double *x);
    // y = A_l x and x.y / y = J(x) and y.b, through the launches PCG and the V-cycle's last post-sweep use (fused dot, part0_)
    double op_spmv_dot(int l, const double *x, double *y);
    double op_jacobi_dot(int l, const double *b, const double *x, double *y);
    // test hook: the launch plan (threads per workgroup, q, ty, cz) of box-grid level l's double sweep (kernel 2) or plane-marching
    // kernel (1); q = ty = cz = 0: the planner's plan on 1024 threads, kernel 3 = the marching kernel's shared-CU plan.  Refuses (SPARSH_EINVAL, reason in error) what the kernel cannot run or
    // what writes more partials than part0_ / part1_ hold; does not switch the kernel on
    int set_box_plan(int l, int kernel, int threads, int q, int ty, int cz);
    // KernelConfig::box_exact_fma = mode (0 never, 1 where DevCsr::box_exact holds), applied to every level that exists; before or after setup
    void set_box_exact_fma(int mode);
    // fuse_zero: also write the coarse level's zero-guess sweep (aggregation P, no gather step); returns whether it did
    bool op_restrict(int l, const double *r, double *bc, bool fuse_zero = false);
    // level_paired(l) levels: b_{l+1} = R (b - A x) and x_{l+1} = omega b_{l+1} / d_{l+1} in one launch
    void op_residual_restrict(int l, const double *b, const double *x, double *bc, double *xc);
    // level_prolong_fused(l) levels: one sweep of level l from x whose result is added to xf (level l - 1) instead of stored
    void op_jacobi_prolong(int l, const double *b, const double *x, double *xf);
    void op_prolong(int l, const double *xc, double *xf);
    void op_coarse(const double *b, double *x);
    // z = V32(r): one application of the opt-in fp32 preconditioner (fp64 in/out); needs precond_fp32
    bool op_precond_f32(const double *r, double *z);
    // ---- the steps of the fp32 cycle on device float vectors (precond_fp32_active() only).  vcycle_f32 is made of these calls alone;
    // sparsh_op_*_f32 run them one at a time on the caller's vectors
    bool level_f32_sdia(int l) const { return f32_[l].A.val != nullptr; }  // float sliced-diagonal mirror (else float CSR values); l < last
    void f32_zero_sweep(int l, const float *b, float *x);                 // x = (omega b) / d: the sweep from a zero guess
    void f32_jacobi(int l, const float *b, const float *x, float *y);    // y = one Jacobi sweep of x
    void f32_residual(int l, const float *b, const float *x, float *r);  // r = b - A_l x
    void f32_restrict(int l, const float *r, float *bc);                 // b_{l+1} = R_l r
    void f32_prolong(int l, const float *xc, float *xf);                 // x_l += P_l x_{l+1} (aggregation gather or CSR rows, as the level decides)
    void f32_coarse(const float *b, float *x);                           // float inverse GEMV, or convert / fp64 factors / convert
    void f32_cvt(long n, const double *in, float *out);                  // out = (float)in
    void f32_cvt_dot(int n, const float *z32, const double *r64, double *z64, double *partial, int *nblk);  // z64 = z32 and the partial sums of z.r
    float *op_jacobi_f32(int l, const float *b, float *x, float *tmp, int sweeps, bool x_is_zero);  // returns x or tmp: the one with the result
    double op_cvt_f2d_dot(int n, const float *z32, const double *r64, double *z64);                  // f32_cvt_dot with the sum read back
    // z = M r as the Krylov loops apply it: the V-cycle of the current smoother from a zero guess, or the fp32 cycle; SPARSH_* code
    int op_precond(const double *r, double *z);
    // ---- restarted GMRES: restart length (0 = kGmresDefaultRestart); a changed length frees the basis
    static constexpr int kGmresDefaultRestart = 30;
    int set_gmres(int restart);
    int gmres_restart() const { return gm_restart_; }
    // storage of the basis vectors (SPARSH_BASIS_FP64 / SPARSH_BASIS_FP32; arithmetic is fp64 either way); a changed one frees the basis
    int set_gmres_basis(int precision);
    int gmres_basis() const { return gm_prec_; }
    // basis + its partial sums (+ the fp64 vector that holds w under a float basis); 0 until the first GMRES solve
    size_t gmres_basis_bytes() const { return gm_bytes_; }
    // bench: one orthogonalisation step of w = level-0 work vector against restart - 1 basis vectors (fixed pattern), through the
    // fused kernels (true) or through launch_dot / launch_axpby pairs with a read-back of each coefficient replaced by a fixed one (false,
    // double basis only).  The basis is of the handle's precision; under a float basis the pattern is rounded to float.
    int gmres_bench_prepare();
    void gmres_bench_step(bool fused);
    double op_dot(int n, const double *x, const double *y);
    // nvec vectors of n rows as the Gram-Schmidt kernels read them, used by gmres_reserve and by the sparsh_op_gs_* hooks: stride = n
    // rounded up to 2 doubles / 4 floats, a float basis zeroed on the stream.  Returns the bytes held (0: error set); free with dfree.
    size_t gmres_basis_alloc(int n, int nvec, int precision, double *&basis, float *&basisf, long &stride);
    // the device block behind a GmresState, zeroed on the stream, and s pointing into it (nullptr: error set); free with dfree
    double *gmres_state_alloc(GmresState &s);

    // ---- block of up to 8 right-hand sides (engine_multi.cpp).  Blocks are row-interleaved with width
    // multi_width(nrhs); callers hand over column-major device arrays.  Single-GPU handles, Jacobi smoother, fp64 cycle.
    // why a block call cannot run on this handle (nullptr: it can); needs no device
    const char *multi_refusal() const;
    // the block vectors of every level and of the Krylov loop for nrhs columns, allocated on first use and replaced when the width
    // changes; SPARSH_* code
    int multi_reserve(int nrhs);
    void multi_release();
    int multi_width_now() const { return mw_; }
    size_t multi_bytes() const { return multi_bytes_; }
    // block PCG on column-major device arrays: X = initial guesses in, solutions out; hist[c * hist_cap + k], iters[c], status[c]
    int solve_multi_dev(int nrhs, const double *B, long ldb, double *X, long ldx, int max_iters, double *hist, int hist_cap, int *iters,
                        int *status, double *seconds);
    // block CG with the arguments of solve_multi_dev: the columns share one search space, so iters is the
    // same for every column and status is per solve.  P and Q are the block PCG's p and Ap; the Gram results, coefficient matrices,
    // factor, flags and the Gram launch's partial sums are the solver's own, reserved at the first block CG call for a width and
    // counted in bcg_bytes(), never in multi_bytes().
    int solve_bcg_dev(int nrhs, const double *B, long ldb, double *X, long ldx, int max_iters, double *hist, int hist_cap, int *iters,
                      int *status, double *seconds);
    size_t bcg_bytes() const { return bcg_bytes_; }
    int bcg_iterations() const { return bcg_last_[0]; }
    int bcg_min_rank() const { return bcg_last_[1]; }
    int bcg_dropped() const { return bcg_last_[2]; }
    // block BiCGStab (engine_mbicg.cpp) with the arguments, conventions and return codes of solve_multi_dev:
    // per column the arithmetic of bicg(precond = true), the columns frozen one by one on the device.  X, R, P and AP are the block
    // PCG's x, r, p and Ap; R0, S, AS, P1 and the per-column state are the solver's own, reserved at the first such call for a
    // width and counted in mbicg_bytes(), never in multi_bytes().
    int solve_mbicg_dev(int nrhs, const double *B, long ldb, double *X, long ldx, int max_iters, double *hist, int hist_cap, int *iters,
                        int *status, double *seconds);
    size_t mbicg_bytes() const { return mbicg_bytes_; }
    int mbicg_iterations() const { return mbicg_last_; }
    // operator-level hooks on column-major device arrays (ld = rows of the level): each interleaves, runs the block launch and
    // de-interleaves.  which: 0 Y = A X with dots, 1 residual, 2 Jacobi leg (sweeps, x_is_zero), 3 restriction, 4 prolongation
    // (X = coarse block, Y = fine block in/out), 5 coarse solve, 6 one vcycle_multi from a zero guess (level 0)
    int op_multi(int which, int l, int nrhs, const double *B, const double *X, double *Y, double *dots, int sweeps, bool x_is_zero);
    // bench: op 0 = SpMV + dot, 1 = Jacobi sweeps ping-ponging, on level l's block buffers of the width in force
    int bench_multi_launch(int op, int l);

    // ---- lowest eigenpairs by LOBPCG on the block path (engine_eig.cpp).  The handles multi_refusal() turns
    // away are turned away here too.  The solver's blocks (X, AX, W, AW, P, AP, R), partial sums and small matrices are its own,
    // reserved at the first call for a width and freed by setup and the destructor; the cycle runs in the block path's level buffers.
    int eig_reserve(int nev);
    void eig_release();
    int eig_width_now() const { return ew_; }
    size_t eig_bytes() const { return eig_bytes_; }
    int eig_restarts() const { return eig_restarts_; }
    // column-major device array X (start block in, Ritz vectors out), host arrays lambda[nev], hist[c * hist_cap + it], iters, status
    int eigs_dev(int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap, int *iters, int *status,
                 double *seconds);
    // bench: op 2 = the twelve-pair Gram launch with its finalise, 3 = one update, on the resident eig blocks; with the blocks of the
    // generalised solver reserved (eig_reserve_gen) 4 = its update, 5 = the block SpMV with B
    int bench_eig_launch(int op);
    // ---- the generalised problem A x = lambda B x.  B is the caller's SPD matrix of n0() rows, checked on the host by the C layer and
    // kept on the device as a CSR operator of the block path until the next setup, the destructor or the next eig_set_b (nullptr
    // drops it).  BX, BW and BP are reserved at the first generalised call for a width, on top of eig_reserve's blocks.
    int eig_set_b(const int *rowptr, const int *col, const double *val);
    bool eig_b_set() const { return eb_set_; }
    long eig_b_nnz() const { return eb_set_ ? eB_.nnz : 0; }
    size_t eig_b_bytes() const { return eb_bytes_; }
    int eig_reserve_gen(int nev);
    // as eigs_dev; X comes back B-orthonormal
    int eigs_gen_dev(int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap, int *iters,
                     int *status, double *seconds);
    // hook: Y = B X on column-major device arrays through the block SpMV on the stored B
    int op_eig_b_multi(int nrhs, const double *X, double *Y);
    // ---- eigenpairs under constraints: the nev lowest pairs in the B-orthogonal complement of the ncon columns of Y (column-major
    // device array, ldy >= n0(); nullptr with ncon = 0), gen as in eigs_dev / eigs_gen_dev.  A null-space handle is accepted and gets
    // the constant vector as one more constraint.  Without any constraint the call is eigs_dev / eigs_gen_dev.  The constraint blocks
    // (Y, B Y when gen, the small matrices) are the solver's own, reserved per (width, count, gen) on top of eig_reserve's, dropped with
    // them and never counted in eig_bytes().
    int eigs_con_dev(bool gen, int nev, double *X, long ldx, int ncon, const double *Y, long ldy, double tol, int max_iters, double *lambda,
                     double *hist, int hist_cap, int *iters, int *status, double *seconds);
    const char *eig_con_refusal() const;  // multi_refusal() without its refusal of null-space handles
    int eig_con_total() const { return con_mt_; }
    size_t eig_con_bytes() const { return con_bytes_; }
    // bench: one projection (the Gram launch with its finalise, then the apply kernel) of the resident W block with the constraints the last constrained solve left
    int bench_eig_con_launch();
    // ---- the orthonormalised basis and the guard vectors (SPARSH_EIG_BASIS_ORTHO, `wanted`; sparsh_set_eig_options).  Both settings
    // are the handle's and survive setup; they need no device.  Under the ortho basis the active mask is decided on the device, W is
    // made B-orthogonal to X and B-orthonormalised by Cholesky-QR twice and the active columns of P are B-orthonormalised, every
    // iteration; the plain basis issues exactly the launches it always had.  The mode's own device memory (three masks and two W x W
    // matrices at the width in force) is reserved at the first ortho solve for a width, freed with the solver's blocks or by a change
    // of basis and counted by eig_ortho_bytes(), never by eig_bytes().
    int set_eig_options(int basis, int wanted);
    int eig_basis() const { return eig_basis_; }
    int eig_wanted() const { return eig_wanted_; }
    int eig_dropped_w() const { return eig_dropped_[0]; }
    int eig_dropped_p() const { return eig_dropped_[1]; }
    size_t eig_ortho_bytes() const { return ortho_bytes_; }
    // bench: 8 = the transform of three blocks (P, AP, BP) with the resident T, 9 = the masked subtraction W <- W - X C, on the
    // resident blocks of the generalised solver and the mode's small arrays
    int bench_eig_ortho_launch(int op);
    int eig_ortho_reserve();  // after eig_reserve: the masks and small matrices at width ew_

    // device memory helpers
    void *dalloc(size_t bytes);
    void dfree(void *p);
    bool check(hipError_t e, const char *what);
    std::string error;
    // Sticky fault of the solve path: the first failed HIP call (SPARSH_ENODEV) or transport step
    // (SPARSH_ECOMM) since setup.  Solvers stop at their next check and return it; every later
    // call on the handle returns it too until sparsh_setup is called again.
    int fault() const { return fault_; }
    bool note_hip(hipError_t e, const char *what);
    bool note_comm(bool ok, const char *what);

    ProfileData prof;
    void profile_begin();    // (re)arm the event pool
    void profile_collect();  // sync and sum the recorded launch times
    double setup_seconds = 0.0;
    // placement search of the last setup: sweep time of the chosen / the worst / the initial triple (us), triples tried (0: not run)
    double place_best_us = 0.0, place_worst_us = 0.0, place_first_us = 0.0;
    int place_tried = 0;
    double place_seconds = 0.0;

private:
    // one V(nu,nu) cycle: rhs b0 (device, read-only), solution accumulates in lev_[0].x.
    // x0_zero: the initial guess of level 0 is zero (preconditioner use).
    // dot_partial: when non-null the last post-sweep also leaves partial sums of x.b there.
    void vcycle(const double *b0, bool x0_zero, double *dot_partial, int *dot_nblk, bool zero_done0 = false);
    // zero_done: the zero-guess sweep x = omega*b/d has already been written to L.x (fused into the restriction)
    // prolong_to: the finer level whose iterate the last sweep adds its result to (level_prolong_fused), nullptr = store it
    void smooth(DevLevel &L, const double *b, int sweeps, bool x_zero, double *dot_partial, int *dot_nblk, bool zero_done = false,
                DevLevel *prolong_to = nullptr);
    bool halo(const DevPlan &p, double *vec);  // pack + exchange (no-op on one GPU)
    // deep-halo level: fill the ghost layers <= depth (which: 0 depth 1, 1 depth K-1, 2 depth K) of vec from their owners
    bool deep_exchange(DevLevel &L, int which, double *vec);
    // launch an A_l-type operator on the first `rows` local rows of a deep level (no exchange)
    int launch_prefix(DevLevel &L, int rows, CsrOp op, const CsrArgs &a);
    bool upload_deep_plan(const DeepPlan &h, DevDeepPlan &d);
    // A_l-type operator on level L: exchanges the halo of a.x, then launches; with overlap enabled the
    // exchange runs on a second stream while the slices that touch no halo column are processed.
    // Returns the number of reduction partials written.
    int apply_A(DevLevel &L, CsrOp op, CsrArgs a);
    void finalize(Fin code, const double *p0, const double *p1, int nblk, int slot, double *hist, int it, int nblk1 = -1);
    bool upload_plan(const HaloPlan &h, DevPlan &d);
    double read_scalar(int slot);
    double read_hist(int it);

    // z = M r from a zero guess, the one place that applies the preconditioner: the float hierarchy when it is built (z in scratch),
    // otherwise vcycle of the handle's smoother (z in lev_[0].x, which belongs to the cycle: valid until the next one).  Returns where
    // z lies.  The fp32 cycle always writes the partial sums of z.r: a null dot_partial means part0_ and a local block count.
    const double *precondition(const double *r, double *scratch, double *dot_partial = nullptr, int *dot_nblk = nullptr, bool zero_done0 = false);
    // one V(nu,nu) cycle with the SOR or the Chebyshev smoother: the Jacobi cycle's order of operations without any fused Jacobi step
    void vcycle_plain(const double *b0, bool x0_zero, double *dot_partial, int *dot_nblk);
    // one smoothing leg of that cycle on level l, iterate in lev_[l].x (x_zero: taken as 0); post: after the coarse correction;
    // dot_partial: the leg also leaves the partial sums of x.b there (Chebyshev: fused into its last step, OP_CHEBY_DOT)
    // b: the leg's right-hand side (lev_[l].b in the V-cycle; the W- and K-cycles also run a level on a residual of their own)
    void plain_leg(int l, const double *b, bool x_zero, bool post, double *dot_partial, int *dot_nblk);
    // ---- the recursive cycle (kind W or K), reached from vcycle() when the kind is not V
    // cycle(l, b): the plain V-cycle body of level l from a zero guess (level 0: from lev_[0].x unless x_zero), result in lev_[l].x;
    // below level l the coarse problems go through solve_coarse_wk.  Legs are the handle's smoother with nothing fused across launches
    void cycle_wk(int l, const double *b, bool x_zero, double *dot_partial, int *dot_nblk);
    // x_l = solve_coarse(l, lev_[l].b) in lev_[l].x: cycle(l, b) on a plain level, the W or the K step around two of them on a WK level
    void solve_coarse_wk(int l);
    void wk_leg(int l, const double *b, bool x_zero, bool post, double *dot_partial, int *dot_nblk);
    // the two halves of a K step around the second inner cycle; s: the level's scalar block
    void kstep_first(int l, const double *b, const double *c, double *v, double *r, double *s);
    void kstep_second(int l, const double *c, const double *d, const double *v, double *w, const double *r, double *x, double *s);
    bool wk_level_for(int l, int stride) const
    {
        const int last = (int)H_.levels.size() - 1;
        return cycle_kind_ != SPARSH_CYCLE_V && l >= 1 && l < last && l % stride == 0;
    }
    long level_visits_for(int l, int stride) const;
    long cycle_visits_for(int stride) const;
    bool kc_scratch();  // partial sums and scalar blocks of the K step (no-op once held)
    // refusals of a setup under SPARSH_NULLSPACE_CONSTANT and the two defects of level 0: SPARSH_OK or SPARSH_EINVAL with the reason
    int nullspace_check(const sparsh_params &p, bool with_defects);
    // the operator the coarsest-level solver factors: A_L, or A_L with the pinned row and column under a constant null space
    const HostCsr &coarse_operator();
    // the right-hand side of a solve under a constant null space: a projected copy in ns_b_ (the caller's b is never written)
    const double *ns_rhs(const double *b);
    int ns_kind_ = SPARSH_NULLSPACE_NONE;
    double ns_row_defect_ = 0.0, ns_col_defect_ = 0.0;
    HostCsr pinned_AL_;
    bool pinned_valid_ = false;
    double *ns_part_ = nullptr, *ns_b_ = nullptr;  // partial sums of launch_sum ; the projected right-hand side (both: CONSTANT only)
    int cycle_kind_ = SPARSH_CYCLE_V, cycle_stride_ = kCycleDefaultStride;
    std::vector<WkLevel> wk_;  // per level (empty until first use)
    double *kc_part_ = nullptr, *kc_scal_ = nullptr;  // kKcPartialDoubles ; kKcScalDoubles per level and one block more for op_kstep
    size_t wk_bytes_ = 0;
    // run fn with lev_[l]'s ping-pong slots pointing at the caller's x / tmp; the result ends in x
    template <class Fn> void with_borrowed_slots(int l, double *x, double *tmp, Fn fn);
    std::vector<ChebyLevel> cheb_;  // per level (empty until first use)
    double cheby_ratio_ = kChebyDefaultRatio;
    int cheby_steps_ = kChebyDefaultSteps;
    int cheby_flip_ = 0;  // cheby_bench_step
    void adopt_sweeps();  // prm_.sweeps = the Jacobi sweep count this handle's smoother selection asks for
    int smoother_ = SPARSH_SMOOTH_JACOBI;
    int sm_sweeps_ = 0;       // sweeps of sparsh_set_smoother (0: the default)
    int sor_order_ = SPARSH_SOR_FORWARD;
    int sor_path_ = 0;
    int base_sweeps_ = 0;     // params.sweeps of the last setup
    std::vector<ColorClasses> colors_;  // per level, filled on first use
    std::vector<SorLevel> sor_;         // per level device layouts (empty until built)
    bool setup_f32();
    // V(nu,nu) cycle on the float hierarchy from a zero guess: z64 = V32(r64), partial sums of z.r
    void vcycle_f32(const double *r64, double *z64, double *partial, int *nblk);
    void f32_apply(int l, CsrOp op, const float *b, const float *x, float *y);  // the level's sweep / residual launch (sdia or CSR mirror)
    // ---- the single-vector Krylov methods (engine_krylov.cpp), solve_dev's cases.  What they share:
    int krylov_prepare(int method);  // the method's refusals, then smoother_prepare and cycle_prepare when it applies M; SPARSH_* code
    // b and x under a constant null space (b then points at the projected copy), x staged in `stage` on a partitioned handle
    // (nullptr: a method that does not run there); returns the x to take the first residual from
    const double *krylov_start(const double *&b, double *x, double *stage);
    double residual_norm(const double *r, int rr_slot = -1);  // ||r|| read back (S_RES); r.r also stored in rr_slot when >= 0
    bool read_due(int count, bool last) const;                // the host reads the residual after iteration `count`
    bool read_residual(int slot, int shown, double &res);     // res = hist_dev_[slot], the print_solve line; false: NaN
    void copy_hist(int count, double *hist, int hist_cap);    // the first min(count, hist_cap) residuals to the host (stream idle)
    // projection under a null space, synchronise, history and *iters out; returns the fault if there is one, else rc
    int krylov_finish(double *x, int count, int rc, double *hist, int hist_cap, int *iters);
    // while (res > tol): iteration cap, fault, body(slot) = the launches of one iteration, which leave its residual norm in
    // hist_dev_[slot], the read schedule; `shown`: what print_solve calls the first iteration.  SPARSH_OK / ENOCONV / ENUMERIC
    template <class Body> int krylov_loop(double res, int max_iters, int shown, int &count, Body body);
    void pcg_body(bool precond, int slot);
    bool capture_graph(bool precond);
    void drop_graph();
    int pcg(const double *b, double *x, int max_iters, double *hist, int hist_cap, int *iters, bool precond);
    int bicg(const double *b, double *x, int max_iters, double *hist, int hist_cap, int *iters, bool precond);
    int fcg(const double *b, double *x, int max_iters, double *hist, int hist_cap, int *iters);
    int gmres(const double *b, double *x, int max_iters, double *hist, int hist_cap, int *iters, bool precond);
    int gmres_reserve();   // basis, partial sums and device state of the current restart length (no-op once held)
    void gmres_release();
    // w = v_{j+1} (holding A M v_j) orthogonalised against v_0..v_j twice, column j rotated, hist_dev_[slot] = |g_{j+1}|, v_{j+1} normalised
    void gmres_orthogonalise(int j, int slot, double *feed);  // feed: written under a float basis only
    double *gm_vec(int k) const { return gm_basis_ + (size_t)k * gm_stride_; }
    float *gm_vecf(int k) const { return gm_basisf_ + (size_t)k * gm_stride_; }
    int gm_restart_ = kGmresDefaultRestart;
    int gm_prec_ = SPARSH_BASIS_FP64;
    double *gm_basis_ = nullptr, *gm_part_ = nullptr, *gm_state_ = nullptr;
    float *gm_basisf_ = nullptr;  // the basis under SPARSH_BASIS_FP32 (gm_basis_ stays nullptr); stride a multiple of 4, zeros behind row n
    double *gm_w_ = nullptr;      // ... and w of the current step, which a double basis keeps in the slot of v_{j+1}
    GmresState gm_;
    long gm_stride_ = 0;
    size_t gm_bytes_ = 0;

    // block vectors of one level (interleaved, n * width doubles each); level 0 has no b: the cycle's right-hand side is the
    // Krylov residual
    struct MultiLevel {
        double *x = nullptr, *x2 = nullptr, *b = nullptr, *r = nullptr;
    };
    // one V(nu,nu) Jacobi cycle from a zero guess on a block: the order of vcycle_plain, nothing fused; result in mlev_[0].x
    void vcycle_multi(const double *b0);
    // one Jacobi leg of `sweeps` sweeps on level l: iterate in x on entry and exit (x_zero: taken as 0), x2 is scratch; the two
    // pointers are swapped as the sweeps ping-pong
    void multi_leg(int l, const double *b, double *&x, double *&x2, int sweeps, bool x_zero);
    void multi_residual(int l, const double *b, const double *x, double *r);
    void multi_restrict(int l, const double *r, double *bc);
    void multi_prolong(int l, const double *xc, double *xf);
    void multi_coarse(const double *b, double *x);
    int multi_spmv_dot(int l, const double *x, double *y, double *partial);
    void multi_forget();  // the buffers went with allocs_ (setup): drop the pointers
    int mw_ = 0;          // width in force (0: nothing allocated)
    size_t multi_bytes_ = 0;
    std::vector<MultiLevel> mlev_;
    double *mx_ = nullptr, *mr_ = nullptr, *mp_ = nullptr, *mAp_ = nullptr;  // block PCG: iterate, residual, direction, A p
    double *mpart0_ = nullptr, *mpart1_ = nullptr;                          // kMultiMax * mpart_cap_ partial sums each
    int mpart_cap_ = 0;
    double *mcs_in_ = nullptr, *mcs_out_ = nullptr;  // factored coarsest level: the block as contiguous vectors for CoarseSolver::solve
    double *mhist_ = nullptr;                        // kMultiMax * hist_cap_dev_ residual histories
    int *mflags_ = nullptr;                          // frozen, iters, status: kMultiMax ints each
    MultiState ms_;
    int mflip_ = 0;  // bench_multi_launch
    std::vector<void *> multi_allocs_;
    size_t mlen0_ = 0;  // doubles of mlev_[0].x as multi_reserve allocated it (block BiCGStab swaps a block of its own with it)
    // ---- what the block solvers share (engine_multi.cpp): block PCG, block CG and block BiCGStab all of it, LOBPCG the allocator and
    // the clock.
    // `doubles` doubles zeroed on the stream, registered in `owner` and counted in `bytes`.  ok false on entry: nothing happens; on any
    // failure what was allocated is freed, ok becomes false and nullptr comes back
    double *take_zeroed(std::vector<void *> &owner, size_t &bytes, bool &ok, size_t doubles);
    // the entry of a block solve: ready, no fault, multi_refusal(), multi_reserve(nrhs), then max_iters <= 0 -> params.max_iter and
    // the clamp to the rows of level 0 (the single loop stops at n iterations too); SPARSH_* code, the reason in error
    int block_begin(int nrhs, int &max_iters);
    // HIP-event time of the stream work from its construction to stop(), which synchronises and writes *seconds; seconds == nullptr:
    // no event is made and stop() does nothing.  The destructor drops events that no stop() took care of
    struct StreamClock {
        StreamClock(Engine &e, double *seconds);
        ~StreamClock();
        StreamClock(const StreamClock &) = delete;
        StreamClock &operator=(const StreamClock &) = delete;
        void stop();

    private:
        Engine &eng_;
        double *seconds_;
        hipEvent_t e0_ = nullptr, e1_ = nullptr;
    };
    // host[0, count) = dev[0, count) through pinned_, stream synchronised
    void read_block_flags(const int *dev, int *host, int count);
    // the loop of the three block solvers on `count` device flags and their host copy: a first read, then while running() (evaluated
    // on the host copy), below the cap and without fault: body(it) = the launches of iteration it, and after the iterations read_due
    // names another read and, under print_solve, shown(it) = the solver's own line
    template <class Running, class Body, class Shown>
    void block_loop(const int *dev, int *host, int count, int max_iters, Running running, Body body, Shown shown);
    // after the loop: the block x back into the caller's X, the last flag read, the clock stopped, launch errors noted under `what`;
    // returns the fault (SPARSH_OK: none)
    int block_finish(int nrhs, const double *x, double *X, long ldx, const int *dev, int *host, int count, StreamClock &clock, const char *what);
    // the first min(count, hist_cap) residuals of column c to hist[c * hist_cap ...] (stream idle)
    void copy_hist_multi(int c, int count, double *hist, int hist_cap);
    // block PCG's and block BiCGStab's end, from flags = [frozen, iters, status] (kMultiMax each): status[c], iters[c] and the history
    // per column, the text in error; returns the fault or SPARSH_OK / ENOCONV / ENUMERIC, and through *most the largest count
    int block_verdict(int nrhs, const int *flags, double *hist, int hist_cap, int *iters, int *status, int *most = nullptr);
    // block CG: gm = [G, C1, C2] and coef = [alpha, beta] (W x W each), the factor and flags, the Gram launch's partial sums; in
    // multi_allocs_ (they go with the block vectors) but counted on their own
    int bcg_reserve();
    BcgState bcg_;
    double *bcg_gm_ = nullptr, *bcg_coef_ = nullptr, *bcg_part_ = nullptr;
    size_t bcg_bytes_ = 0;
    int bcg_last_[3] = {0, 0, 0};  // iterations, minimum rank and dropped directions of the last solve
    // block BiCGStab: four blocks of n * width doubles and the per-column state; in multi_allocs_ too, counted on their own
    int mbicg_reserve();
    MbicgState mb_;
    double *mb_r0_ = nullptr, *mb_s_ = nullptr, *mb_as_ = nullptr, *mb_p1_ = nullptr;
    size_t mbicg_bytes_ = 0;
    int mbicg_last_ = 0;  // iterations of the last solve (the largest count of a column)

    // LOBPCG (engine_eig.cpp): seven interleaved blocks of n * width doubles, the partial sums of the Gram and residual launches,
    // G = [S^T S, S^T A S, residual norms] and coef = [Cx, Cw, Cp, theta]
    void eig_forget();  // the buffers went with allocs_ (setup): drop the pointers
    void eig_gram_pairs(GramPairs &prs, bool gen = false) const;
    struct EigCon {  // the caller's constraints of one solve (device, column-major)
        int ncon = 0;
        const double *Y = nullptr;
        long ldy = 0;
    };
    int eigs_run(bool gen, int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap, int *iters,
                 int *status, double *seconds, const EigCon *con = nullptr);
    int eig_con_reserve(int mt, bool gen);  // after eig_reserve: the constraint blocks for mt constraints at width ew_
    void eig_con_release();
    void eig_con_forget();  // the constraint blocks went with allocs_ (setup) or were freed: drop the pointers
    void eig_con_project(const double *src, double *dst);  // dst = Pi src on blocks of width ew_ (dst may be src)
    int con_mt_ = 0;        // constraints the blocks below were reserved for (0: none)
    bool con_gen_ = false;  // with B Y blocks of their own
    size_t con_bytes_ = 0;
    double *cY_ = nullptr, *cBY_ = nullptr;  // ceil(mt / W) interleaved blocks each; cBY_ == cY_ for the standard problem
    double *cG_ = nullptr, *cGinv_ = nullptr, *cC_ = nullptr;  // Y^T B Y (padded order), its inverse (order mt), (BY)^T V
    std::vector<void *> con_allocs_;
    void eig_b_spmv(const double *x, double *y);  // y = B x on interleaved blocks of width ew_
    void eig_b_forget();                          // B went with allocs_ (setup): drop the pointers
    void eig_update(bool gen, int k);             // step 6 in place on the resident blocks
    // SPARSH_EIG_BASIS_ORTHO: masks = [active, W in basis, P in basis] (W doubles each), oG_ the Gram matrix or C of one pair, oT_ the
    // transform; in ortho_allocs_
    void eig_ortho_release();
    void eig_ortho_forget();
    // one orthonormalisation of the block V (B V = BV; nullptr: BV is V) on the columns of mask_in: the one-pair Gram launch, the small
    // Cholesky step and the transform of V, BV and, when given, AV
    void eig_ortho_pass(int k, double *V, double *BV, double *AV, const double *mask_in, double *mask_out);
    int eig_basis_ = 0, eig_wanted_ = 0;
    int eig_dropped_[2] = {0, 0};  // dropped columns of W and of P in the last solve
    size_t ortho_bytes_ = 0;
    double *oM_ = nullptr, *oG_ = nullptr, *oT_ = nullptr;
    std::vector<void *> ortho_allocs_;
    int ew_ = 0;        // width in force (0: nothing allocated)
    size_t eig_bytes_ = 0;
    int eig_restarts_ = 0;
    double *eX_ = nullptr, *eAX_ = nullptr, *eW_ = nullptr, *eAW_ = nullptr, *eP_ = nullptr, *eAP_ = nullptr, *eR_ = nullptr;
    double *epart_ = nullptr, *eG_ = nullptr, *ecoef_ = nullptr;
    double *epinned_ = nullptr;  // host-pinned: G coming down, coef going up
    double *eBX_ = nullptr, *eBW_ = nullptr, *eBP_ = nullptr;  // the generalised solver's three extra blocks (in eig_allocs_)
    DevCsr eB_;                                                  // B of the pencil
    bool eb_set_ = false;
    size_t eb_bytes_ = 0;
    std::vector<void *> eb_allocs_;
    size_t dalloc_total_ = 0;  // bytes dalloc ever handed out: the difference around an upload is that upload's size
    std::vector<void *> eig_allocs_;

    std::unique_ptr<Comm> comm_;
    std::vector<Partition> parts_;  // row partition of every level
    Partition gather_part_;         // share of the first replicated level each rank restricts, then all-gathers
    int repl_level_ = 0;            // first replicated level (0: nothing is partitioned)
    bool dist_ = false;
    bool overlap_ = false;          // multi-GPU: overlap halo exchange with interior slices
    bool deep_halo_ = true;         // multi-GPU: deep-halo smoothing on the partitioned levels
    int comm_tune_ = 1;
    int tuned_repl_level_ = -1;     // >= 0: number of partitioned levels chosen by tune_comm_schedule
    bool tuned_deep_ = true;
    std::vector<CommLevelChoice> sched_;
    CommMeasured meas_;
    bool measure_transport();
    void tune_comm_schedule(const sparsh_params &p);
    void decide_comm_schedule(const sparsh_params &p, int G);
    long n_exchanges_ = 0;          // transport calls issued (halo / staged exchanges; diagnostics)
    hipStream_t st2_ = nullptr;     // exchange stream of the overlap path
    hipEvent_t ev_ready_ = nullptr, ev_halo_ = nullptr;
    std::vector<F32Level> f32_;
    float *coarse_inv_f32_ = nullptr;
    bool f32_ready_ = false;
    KrylovState ks_;
    HostCsr A0_;
    HostHierarchy H_;
    sparsh_params prm_{};
    KernelConfig cfg_;
    std::vector<DevLevel> lev_;
    CoarseSolver coarse_;  // coarsest-level direct solver (dense inverse or block-tridiagonal factors)
    double *coarse_tmp_ = nullptr;  // fp32 mode with the block-tridiagonal form: fp64 staging of b_L, x_L
    int nL_ = 0;
    hipStream_t st_ = nullptr;
    bool ready_ = false;
    bool host_ready_ = false;
    bool share_setup_ = true, built_locally_ = true;
    size_t image_bytes_ = 0;
    int fault_ = 0;
    int device_ = 0;

    // workspace
    double *scal_ = nullptr;      // S_COUNT device scalars
    double *part0_ = nullptr, *part1_ = nullptr;
    int part_cap_ = 0;
    double *hist_dev_ = nullptr;
    int *iter_ctr_ = nullptr;     // device-side residual-history index (graph replays)
    GraphState graph_;
    int hist_cap_dev_ = 0;
    double *pinned_ = nullptr;    // host-pinned staging for scalar read-back
    std::vector<double *> work_;  // level-0 work vectors of the Krylov loops
    std::vector<void *> allocs_;
    // which of the finest level's equally sized buffers play iterate / ping-pong twin / Krylov residual: chosen at setup by
    // timing the sweep on the candidates (see tune_placement)
    void tune_box_kernels();
    void tune_placement();
};

// (here because three files instantiate it: engine_multi.cpp, engine_bcg.cpp, engine_mbicg.cpp)
template <class Running, class Body, class Shown>
void Engine::block_loop(const int *dev, int *host, int count, int max_iters, Running running, Body body, Shown shown)
{
    read_block_flags(dev, host, count);
    for (int it = 0; running() && it < max_iters && fault_ == SPARSH_OK;) {
        body(it);
        ++it;
        if (read_due(it, it >= max_iters)) {
            read_block_flags(dev, host, count);
            if (prm_.print_solve) shown(it);
        }
    }
}

}  // namespace sparsh
