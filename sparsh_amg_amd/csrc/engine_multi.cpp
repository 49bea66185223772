// engine_multi.cpp -- a block of up to 8 right-hand sides through one AMG-PCG run.
//
// The block path is a family of its own on the arrays every level keeps whatever mirror it also has (DevCsr::rowptr / col / val and
// the row-block records): Engine::vcycle_multi follows vcycle_plain with Jacobi legs, Engine::solve_multi_dev follows pcg_init /
// pcg_body per column.  It shares no buffer with the single-vector path except the read-only hierarchy: a single solve before and
// after a block solve gives the same bits.
#include "engine.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace sparsh {

#define HIPCHK(call) note_hip((call), #call)

const char *Engine::eig_con_refusal() const
{
    if (dist_ || (comm_ && comm_->size > 1)) return "block solves are not available on a partitioned (multi-GPU) handle";
    if (prm_.precond_fp32) return "block solves run the fp64 cycle only: params.precond_fp32 is not supported";
    if (cycle_kind_ != SPARSH_CYCLE_V) return "block solves run the V-cycle only: select SPARSH_CYCLE_V (sparsh_set_cycle)";
    if (!jacobi_on()) return "block solves run the Jacobi cycle only: select SPARSH_SMOOTH_JACOBI";
    return nullptr;
}

const char *Engine::multi_refusal() const
{
    if (const char *why = eig_con_refusal()) return why;
    if (ns_on())
        return "block solves are not available on a handle set up with a null space (SPARSH_NULLSPACE_CONSTANT); its eigenpairs: "
               "sparsh_eigs_con";
    return nullptr;
}

void Engine::multi_forget()
{
    mw_ = 0;
    multi_bytes_ = 0;
    mlen0_ = 0;
    mlev_.clear();
    multi_allocs_.clear();
    mx_ = mr_ = mp_ = mAp_ = mpart0_ = mpart1_ = mcs_in_ = mcs_out_ = mhist_ = nullptr;
    mflags_ = nullptr;
    ms_ = MultiState();
    bcg_ = BcgState();  // block CG's small arrays are in multi_allocs_ too (engine_bcg.cpp)
    bcg_gm_ = bcg_coef_ = bcg_part_ = nullptr;
    bcg_bytes_ = 0;
    mb_ = MbicgState();  // ... and block BiCGStab's blocks (engine_mbicg.cpp)
    mb_r0_ = mb_s_ = mb_as_ = mb_p1_ = nullptr;
    mbicg_bytes_ = 0;
}

void Engine::multi_release()
{
    if (st_ && !multi_allocs_.empty()) (void)hipStreamSynchronize(st_);
    for (void *p : multi_allocs_) dfree(p);
    multi_forget();
}

int Engine::multi_reserve(int nrhs)
{
    const int W = multi_width(nrhs);
    if (W == mw_) return SPARSH_OK;
    multi_release();
    bool ok = true;
    auto take = [&](size_t doubles) { return take_zeroed(multi_allocs_, multi_bytes_, ok, std::max<size_t>(doubles, 1)); };
    const int nl = (int)lev_.size();
    mlev_.assign((size_t)nl, MultiLevel());
    int cap = kMultiMax;
    for (int l = 0; l < nl; ++l) {
        const DevLevel &L = lev_[l];
        const size_t len = (size_t)L.n * W;
        if (l == 0) mlen0_ = std::max<size_t>(len, 1);
        mlev_[l].x = take(len);
        mlev_[l].x2 = take(len);
        mlev_[l].r = take(len);
        if (l > 0) mlev_[l].b = take(len);
        cap = std::max(cap, L.A.nblk);
        if (l + 1 < nl) cap = std::max(cap, std::max(L.P.nblk, L.R.nblk));
    }
    const size_t len0 = (size_t)lev_[0].n * W;
    mx_ = take(len0);
    mr_ = take(len0);
    mp_ = take(len0);
    mAp_ = take(len0);
    mpart_cap_ = std::max(cap, 2048) + 8;  // row blocks of the largest operator, or the grid of an elementwise reducing launch
    mpart0_ = take((size_t)kMultiMax * mpart_cap_);
    mpart1_ = take((size_t)kMultiMax * mpart_cap_);
    if (!coarse_.dense()) {  // a factored coarsest level is solved column by column on contiguous vectors
        mcs_in_ = take((size_t)nL_ * W);
        mcs_out_ = take((size_t)nL_ * W);
    }
    mhist_ = take((size_t)kMultiMax * hist_cap_dev_);
    ms_.scal = take((size_t)MS_COUNT * kMultiMax);
    mflags_ = reinterpret_cast<int *>(take((3 * kMultiMax + 1) / 2));
    if (!ok) {
        multi_release();
        return SPARSH_ENODEV;
    }
    ms_.frozen = mflags_;
    ms_.iters = mflags_ + kMultiMax;
    ms_.status = mflags_ + 2 * kMultiMax;
    mw_ = W;
    return SPARSH_OK;
}

// ---------------------------------------------------------------------------- block operators (interleaved device blocks)

int Engine::multi_spmv_dot(int l, const double *x, double *y, double *partial)
{
    MultiArgs a;
    a.x = x;
    a.y = y;
    a.partial = partial;
    return launch_csr_multi(lev_[l].A, mw_, OP_SPMV_DOT, a, st_, cfg_);
}

void Engine::multi_residual(int l, const double *b, const double *x, double *r)
{
    MultiArgs a;
    a.x = x;
    a.b = b;
    a.y = r;
    launch_csr_multi(lev_[l].A, mw_, OP_RESID, a, st_, cfg_);
}

// parallel::jacobi_smoother per column: from a zero guess the first sweep is x = omega b / d
void Engine::multi_leg(int l, const double *b, double *&x, double *&x2, int sweeps, bool x_zero)
{
    const DevLevel &L = lev_[l];
    int k = 0;
    if (x_zero && sweeps > 0) {
        launch_jacobi_zero_multi(L.n, mw_, b, diag_stream(L), L.diag_const, prm_.omega, x, st_);
        k = 1;
    } else if (x_zero) {
        HIPCHK(hipMemsetAsync(x, 0, (size_t)L.n * mw_ * 8, st_));
    }
    for (; k < sweeps; ++k) {
        MultiArgs a;
        a.x = x;
        a.b = b;
        a.d = L.diag;
        a.y = x2;
        a.omega = prm_.omega;
        launch_csr_multi(L.A, mw_, OP_JACOBI, a, st_, cfg_);
        std::swap(x, x2);
    }
}

void Engine::multi_restrict(int l, const double *r, double *bc)
{
    const DevLevel &L = lev_[l];
    if (L.P_is_aggregation) {
        launch_restrict_agg_multi(L.R.nrow, mw_, L.R.rowptr, L.R.col, r, bc, st_);
        return;
    }
    MultiArgs a;
    a.x = r;
    a.y = bc;
    launch_csr_multi(L.R, mw_, OP_SPMV, a, st_, cfg_);
}

void Engine::multi_prolong(int l, const double *xc, double *xf)
{
    const DevLevel &L = lev_[l];
    if (L.P_is_aggregation) {
        launch_prolong_agg_multi(L.n, mw_, L.P.col, xc, xf, st_);
        return;
    }
    MultiArgs a;
    a.x = xc;
    a.y = xf;
    launch_csr_multi(L.P, mw_, OP_ADD, a, st_, cfg_);
}

void Engine::multi_coarse(const double *b, double *x)
{
    if (coarse_.dense()) {
        launch_gemv_multi(nL_, mw_, coarse_.dense_inverse(), b, x, st_);
        return;
    }
    // factored form: W contiguous vectors, CoarseSolver::solve once per column
    launch_deinterleave(nL_, mw_, mw_, b, mcs_in_, nL_, st_);
    for (int c = 0; c < mw_; ++c) coarse_.solve(mcs_in_ + (size_t)c * nL_, mcs_out_ + (size_t)c * nL_, st_);
    launch_interleave(nL_, mw_, mw_, mcs_out_, nL_, x, st_);
}

void Engine::vcycle_multi(const double *b0)
{
    const int last = (int)lev_.size() - 1;
    const int nu = prm_.sweeps;
    if (last == 0) {  // single level: the direct solve is the whole cycle
        multi_coarse(b0, mlev_[0].x);
        return;
    }
    for (int l = 0; l < last; ++l) {
        MultiLevel &M = mlev_[l];
        const double *b = l == 0 ? b0 : M.b;
        multi_leg(l, b, M.x, M.x2, nu, true);     // pre-smoothing from a zero guess
        multi_residual(l, b, M.x, M.r);           // store_residual
        multi_restrict(l, M.r, mlev_[l + 1].b);   // transfer_residual
    }
    multi_coarse(mlev_[last].b, mlev_[last].x);   // Direct_Solver_Pardiso_solve
    for (int l = last; l > 0; --l) {
        MultiLevel &F = mlev_[l - 1];
        multi_prolong(l - 1, mlev_[l].x, F.x);    // transfer_solution
        multi_leg(l - 1, l - 1 == 0 ? b0 : F.b, F.x, F.x2, nu, false);
    }
}

// ---------------------------------------------------------------------------- what the block solvers share

double *Engine::take_zeroed(std::vector<void *> &owner, size_t &bytes, bool &ok, size_t doubles)
{
    if (!ok) return nullptr;
    double *p = static_cast<double *>(dalloc(doubles * 8));
    if (!p || !check(hipMemsetAsync(p, 0, doubles * 8, st_), "hipMemsetAsync")) {
        ok = false;
        dfree(p);
        return nullptr;
    }
    owner.push_back(p);
    bytes += doubles * 8;
    return p;
}

int Engine::block_begin(int nrhs, int &max_iters)
{
    if (!ready_) {
        error = "sparsh_setup has not been called";
        return SPARSH_ESTATE;
    }
    if (fault_ != SPARSH_OK) return fault_;
    if (const char *why = multi_refusal()) {
        error = why;
        return SPARSH_EINVAL;
    }
    if (int rc = multi_reserve(nrhs); rc != SPARSH_OK) return rc;
    if (max_iters <= 0) max_iters = prm_.max_iter;
    max_iters = std::min(max_iters, lev_[0].nglob);
    return SPARSH_OK;
}

Engine::StreamClock::StreamClock(Engine &e, double *seconds) : eng_(e), seconds_(seconds)
{
    if (!seconds_) return;
    eng_.note_hip(hipEventCreate(&e0_), "hipEventCreate");
    eng_.note_hip(hipEventCreate(&e1_), "hipEventCreate");
    eng_.note_hip(hipEventRecord(e0_, eng_.st_), "hipEventRecord");
}

void Engine::StreamClock::stop()
{
    if (!seconds_) return;
    eng_.note_hip(hipEventRecord(e1_, eng_.st_), "hipEventRecord");
    eng_.note_hip(hipEventSynchronize(e1_), "hipEventSynchronize");
    float ms = 0.f;
    eng_.note_hip(hipEventElapsedTime(&ms, e0_, e1_), "hipEventElapsedTime");
    *seconds_ = ms * 1e-3;
    eng_.note_hip(hipEventDestroy(e0_), "hipEventDestroy");
    eng_.note_hip(hipEventDestroy(e1_), "hipEventDestroy");
    e0_ = e1_ = nullptr;
    seconds_ = nullptr;  // stopped
}

Engine::StreamClock::~StreamClock()
{
    if (e0_) (void)hipEventDestroy(e0_);
    if (e1_) (void)hipEventDestroy(e1_);
}

void Engine::read_block_flags(const int *dev, int *host, int count)
{
    HIPCHK(hipMemcpyAsync(pinned_, dev, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, st_));
    HIPCHK(hipStreamSynchronize(st_));
    std::memcpy(host, pinned_, (size_t)count * sizeof(int));
}

int Engine::block_finish(int nrhs, const double *x, double *X, long ldx, const int *dev, int *host, int count, StreamClock &clock,
                         const char *what)
{
    launch_deinterleave(lev_[0].n, nrhs, mw_, x, X, ldx, st_);
    read_block_flags(dev, host, count);
    clock.stop();
    note_hip(hipGetLastError(), what);
    return fault_;
}

void Engine::copy_hist_multi(int c, int count, double *hist, int hist_cap)
{
    const int m = std::min(std::min(count, hist_cap), hist_cap_dev_);
    if (hist && m > 0)
        HIPCHK(hipMemcpy(hist + (size_t)c * hist_cap, mhist_ + (size_t)c * hist_cap_dev_, (size_t)m * 8, hipMemcpyDeviceToHost));
}

int Engine::block_verdict(int nrhs, const int *flags, double *hist, int hist_cap, int *iters, int *status, int *most)
{
    int rc = SPARSH_OK, largest = 0;
    bool numeric = false, noconv = false;
    for (int c = 0; c < nrhs; ++c) {
        int st = SPARSH_OK;
        if (!flags[c]) st = SPARSH_ENOCONV;  // the cap came first: x holds the iterate reached
        else if (flags[2 * kMultiMax + c] == kMultiStatusNumeric) st = SPARSH_ENUMERIC;
        numeric = numeric || st == SPARSH_ENUMERIC;
        noconv = noconv || st == SPARSH_ENOCONV;
        const int k = flags[kMultiMax + c];
        largest = std::max(largest, k);
        if (status) status[c] = st;
        if (iters) iters[c] = k;
        copy_hist_multi(c, k, hist, hist_cap);
    }
    if (most) *most = largest;
    if (numeric) {
        rc = SPARSH_ENUMERIC;
        error = "NaN residual in a column of the block";
    } else if (noconv) {
        rc = SPARSH_ENOCONV;
        error = "iteration cap reached before ||r|| <= tol in a column of the block";
    }
    return fault_ != SPARSH_OK ? fault_ : rc;
}

// ---------------------------------------------------------------------------- block PCG

int Engine::solve_multi_dev(int nrhs, const double *B, long ldb, double *X, long ldx, int max_iters, double *hist, int hist_cap, int *iters,
                            int *status, double *seconds)
{
    if (int rc = block_begin(nrhs, max_iters); rc != SPARSH_OK) return rc;
    const int W = mw_, n = lev_[0].n;
    StreamClock clock(*this, seconds);
    // init: r = b - A x, ||r||, z = M r, rz = z.r, p = z
    launch_interleave(n, nrhs, W, X, ldx, mx_, st_);
    launch_interleave(n, nrhs, W, B, ldb, mr_, st_);
    multi_residual(0, mr_, mx_, mr_);
    int nb = launch_dot_multi(n, W, mr_, mr_, mpart0_, st_);
    launch_finalize_multi(MFIN_INIT, W, nrhs, mpart0_, nb, nullptr, 0, ms_, 0, prm_.tol, nullptr, 0, 0, st_);
    vcycle_multi(mr_);
    nb = launch_dot_multi(n, W, mlev_[0].x, mr_, mpart0_, st_);
    launch_finalize_multi(MFIN_STORE, W, nrhs, mpart0_, nb, nullptr, 0, ms_, MS_RZ, prm_.tol, nullptr, 0, 0, st_);
    HIPCHK(hipMemcpyAsync(mp_, mlev_[0].x, (size_t)n * W * 8, hipMemcpyDeviceToDevice, st_));

    int flags[3 * kMultiMax];
    block_loop(
        mflags_, flags, 3 * kMultiMax, max_iters, [&] { return std::count(flags, flags + nrhs, 0) > 0; },
        [&](int it) {
            const int np = multi_spmv_dot(0, mp_, mAp_, mpart0_);  // Ap = A p ; p.Ap
            launch_finalize_multi(MFIN_ALPHA, W, nrhs, mpart0_, np, nullptr, 0, ms_, 0, prm_.tol, nullptr, 0, 0, st_);
            const int nrr = launch_cg_update_multi(n, W, ms_, mp_, mAp_, mx_, mr_, mpart1_, st_);  // x += alpha p ; r -= alpha Ap ; r.r
            vcycle_multi(mr_);                                                                 // z = M r
            const int nzr = launch_dot_multi(n, W, mlev_[0].x, mr_, mpart0_, st_);               // z.r
            launch_finalize_multi(MFIN_BETA_RES, W, nrhs, mpart0_, nzr, mpart1_, nrr, ms_, 0, prm_.tol, mhist_, hist_cap_dev_,
                                  std::min(it, hist_cap_dev_ - 1), st_);
            launch_p_update_multi(n, W, ms_, mlev_[0].x, mp_, st_);  // p = z + beta p
        },
        [&](int it) { std::printf("%d\t%d of %d columns running\n", it, (int)std::count(flags, flags + nrhs, 0), nrhs); });
    if (int rc = block_finish(nrhs, mx_, X, ldx, mflags_, flags, 3 * kMultiMax, clock, "kernel launch during the block solve"); rc != SPARSH_OK)
        return rc;
    return block_verdict(nrhs, flags, hist, hist_cap, iters, status);
}

// ---------------------------------------------------------------------------- hooks

int Engine::op_multi(int which, int l, int nrhs, const double *B, const double *X, double *Y, double *dots, int sweeps, bool x_is_zero)
{
    if (const char *why = multi_refusal(); why && which == 6) {
        error = why;
        return SPARSH_EINVAL;
    }
    if (dist_) {
        error = "block operator hooks are single-GPU test hooks";
        return SPARSH_ESTATE;
    }
    if (int rc = multi_reserve(nrhs); rc != SPARSH_OK) return rc;
    const int W = mw_;
    const int last = (int)lev_.size() - 1;
    if (which == 5) l = last;
    if (which == 6) l = 0;
    const int n = lev_[l].n;
    const int nc = l < last ? lev_[l + 1].n : 0;
    if ((which == 3 || which == 4) && l >= last) {
        error = "no coarser level";
        return SPARSH_EINVAL;
    }
    // scratch blocks of the hook's own: the level's block buffers keep whatever a solve left in them
    const size_t len = (size_t)std::max(n, nc) * W;
    double *t0 = static_cast<double *>(dalloc(len * 8)), *t1 = static_cast<double *>(dalloc(len * 8)), *t2 = static_cast<double *>(dalloc(len * 8));
    int rc = SPARSH_OK;
    if (!t0 || !t1 || !t2) {
        rc = SPARSH_ENODEV;
    } else {
        switch (which) {
        case 0: {  // Y = A X, dots
            launch_interleave(n, nrhs, W, X, n, t0, st_);
            const int np = multi_spmv_dot(l, t0, t1, mpart0_);
            launch_finalize_multi(MFIN_STORE, W, nrhs, mpart0_, np, nullptr, 0, ms_, MS_TMP, 0.0, nullptr, 0, 0, st_);
            launch_deinterleave(n, nrhs, W, t1, Y, n, st_);
            HIPCHK(hipMemcpyAsync(pinned_, ms_.scal + MS_TMP * kMultiMax, kMultiMax * 8, hipMemcpyDeviceToHost, st_));
            HIPCHK(hipStreamSynchronize(st_));
            if (dots) std::memcpy(dots, pinned_, (size_t)nrhs * 8);
        } break;
        case 1:  // Y = B - A X
            launch_interleave(n, nrhs, W, B, n, t0, st_);
            launch_interleave(n, nrhs, W, X, n, t1, st_);
            multi_residual(l, t0, t1, t2);
            launch_deinterleave(n, nrhs, W, t2, Y, n, st_);
            break;
        case 2: {  // Y = `sweeps` Jacobi sweeps from X (or from 0) with right-hand side B
            launch_interleave(n, nrhs, W, B, n, t0, st_);
            if (!x_is_zero) launch_interleave(n, nrhs, W, X, n, t1, st_);
            double *x = t1, *x2 = t2;
            multi_leg(l, t0, x, x2, sweeps, x_is_zero);
            launch_deinterleave(n, nrhs, W, x, Y, n, st_);
        } break;
        case 3:  // Y = R X
            launch_interleave(n, nrhs, W, X, n, t0, st_);
            multi_restrict(l, t0, t1);
            launch_deinterleave(nc, nrhs, W, t1, Y, nc, st_);
            break;
        case 4:  // Y += P X
            launch_interleave(nc, nrhs, W, X, nc, t0, st_);
            launch_interleave(n, nrhs, W, Y, n, t1, st_);
            multi_prolong(l, t0, t1);
            launch_deinterleave(n, nrhs, W, t1, Y, n, st_);
            break;
        case 5:  // Y = A_L^-1 B
            launch_interleave(n, nrhs, W, B, n, t0, st_);
            multi_coarse(t0, t1);
            launch_deinterleave(n, nrhs, W, t1, Y, n, st_);
            break;
        case 6:  // Y = M B
            launch_interleave(n, nrhs, W, B, n, t0, st_);
            vcycle_multi(t0);
            launch_deinterleave(n, nrhs, W, mlev_[0].x, Y, n, st_);
            break;
        default: rc = SPARSH_EINVAL; break;
        }
        HIPCHK(hipStreamSynchronize(st_));
    }
    dfree(t0);
    dfree(t1);
    dfree(t2);
    note_hip(hipGetLastError(), "kernel launch of a block operator");
    return fault_ != SPARSH_OK ? fault_ : rc;
}

int Engine::bench_multi_launch(int op, int l)
{
    MultiLevel &M = mlev_[l];
    if (op == 0) {
        multi_spmv_dot(l, M.x, M.x2, mpart0_);
        return SPARSH_OK;
    }
    MultiArgs a;
    a.x = (mflip_ & 1) ? M.x2 : M.x;
    a.y = (mflip_ & 1) ? M.x : M.x2;
    a.b = M.r;
    a.d = lev_[l].diag;
    a.omega = prm_.omega;
    ++mflip_;
    launch_csr_multi(lev_[l].A, mw_, OP_JACOBI, a, st_, cfg_);
    return SPARSH_OK;
}

}  // namespace sparsh
