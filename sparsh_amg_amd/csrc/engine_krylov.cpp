// engine_krylov.cpp -- the single-vector Krylov methods of the engine: CG / AMG-PCG (in one call or stepwise), BiCGStab, flexible CG
// and restarted GMRES, and the scaffold they share.
//
// Reference behaviour followed (file:line relative to the reference tree):
//   CG / AMG-PCG                     src/AMG_main_solvers.cpp:47-103, 107-167
//   BiCGStab / AMG-PBiCGStab         src/AMG_main_solvers.cpp:271-355, 358-458
#include "engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

namespace sparsh {

#define HIPCHK(call) note_hip((call), #call)

// ---- what the four methods share (declared with their contracts in engine.hpp)

const char *Engine::sor_refusal(int method) const
{
#define NEEDS_SYMMETRIC(name) name " needs a symmetric preconditioner: the SOR smoother must use SPARSH_SOR_SYMMETRIC"
    if (!sor_on() || sor_order_ == SPARSH_SOR_SYMMETRIC) return nullptr;
    if (method == SPARSH_PCG) return NEEDS_SYMMETRIC("SPARSH_PCG");
    if (method == SPARSH_FCG) return NEEDS_SYMMETRIC("SPARSH_FCG");
    return nullptr;
#undef NEEDS_SYMMETRIC
}

// (the smoother and the cycle may change between krylov_init and krylov_step: pcg_steps asks again)
int Engine::krylov_prepare(int method)
{
    const bool gm = method == SPARSH_GMRES || method == SPARSH_PGMRES;
    const char *why = nullptr;
    if (method == SPARSH_FCG && (dist_ || (comm_ && comm_->size > 1))) why = "SPARSH_FCG is not available on a partitioned (multi-GPU) handle";
    else if (gm && dist_) why = "GMRES is not available on a partitioned (multi-GPU) handle";
    else why = sor_refusal(method);
    if (why) {
        error = why;
        return SPARSH_EINVAL;
    }
    if (method == SPARSH_CG || method == SPARSH_BICG || method == SPARSH_GMRES) return SPARSH_OK;
    if (int rc = smoother_prepare(); rc != SPARSH_OK) return rc;
    return cycle_prepare(method);
}

// Constant null space: the loop reads the projected copy of b and starts from x - mean(x).  Partitioned handle: the caller's x
// has no room for the halo.
const double *Engine::krylov_start(const double *&b, double *x, double *stage)
{
    if (ns_on()) {
        b = ns_rhs(b);
        project(x);
    }
    if (!dist_ || !stage) return x;
    launch_copy(lev_[0].n, x, stage, st_);
    return stage;
}

double Engine::residual_norm(const double *r, int rr_slot)
{
    int nb = 0;
    launch_dot(lev_[0].n, r, r, part0_, &nb, st_);
    if (rr_slot >= 0) finalize(FIN_STORE, part0_, nullptr, nb, rr_slot, nullptr, 0);
    finalize(FIN_SQRT, part0_, nullptr, nb, S_RES, nullptr, 0);
    return read_scalar(S_RES);
}

bool Engine::read_due(int count, bool last) const { return count % std::max(1, prm_.check_every) == 0 || last; }

bool Engine::read_residual(int slot, int shown, double &res)
{
    res = read_hist(slot);
    if (prm_.print_solve) std::printf("%d\t%g\n", shown, res);
    return res == res;
}

void Engine::copy_hist(int count, double *hist, int hist_cap)
{
    const int m = std::min(std::min(count, hist_cap), hist_cap_dev_);
    if (hist && m > 0) HIPCHK(hipMemcpy(hist, hist_dev_, (size_t)m * 8, hipMemcpyDeviceToHost));
}

int Engine::krylov_finish(double *x, int count, int rc, double *hist, int hist_cap, int *iters)
{
    if (ns_on()) project(x);  // rounding drift of the mean
    HIPCHK(hipStreamSynchronize(st_));
    copy_hist(count, hist, hist_cap);
    if (iters) *iters = count;
    return fault_ != SPARSH_OK ? fault_ : rc;
}

// The loop of BiCGStab and of FCG.  pcg_steps keeps its own (the nglob bound, the pieces of the stepwise interface, the graph
// replay) and so does gmres (nested in the restart cycle); all four read the residual through read_due / read_residual.
template <class Body> int Engine::krylov_loop(double res, int max_iters, int shown, int &count, Body body)
{
    for (count = 0; res > prm_.tol && fault_ == SPARSH_OK;) {
        if (count >= max_iters) return SPARSH_ENOCONV;
        const int slot = std::min(count, hist_cap_dev_ - 1);
        body(slot);
        ++count;
        if (read_due(count, count >= max_iters) && !read_residual(slot, shown + count - 1, res)) return SPARSH_ENUMERIC;
    }
    return SPARSH_OK;
}

// Solver_CG_1 (precond = false) / Solver_PCG_1 (precond = true), split into the part before
// the while loop (pcg_init: r0, ||r0||, z0 = V(r0), p = z0; src/AMG_main_solvers.cpp:124-133)
// and the loop body (pcg_steps: :136-159) so a caller can time exactly k iterations.
int Engine::pcg_init(const double *b, double *x, bool precond)
{
    if (int rc = krylov_prepare(precond ? SPARSH_PCG : SPARSH_CG); rc != SPARSH_OK) return rc;
    const int n = lev_[0].n;
    double *r = work_[0], *p = work_[1];
    int nb = 0;
    ks_ = KrylovState();
    ks_.precond = precond;
    const double *xin = krylov_start(b, x, work_[3]);
    ks_.b = b;
    ks_.x = x;
    op_residual(0, b, xin, r);  // r0 = b - A x
    ks_.r1 = residual_norm(r, precond ? -1 : S_RR);
    const double *z = r;
    if (precond) {
        z = precondition(r, work_[4], part0_, &nb);  // z0 = M r0 ; z0.r0
        finalize(FIN_STORE, part0_, nullptr, nb, S_RZ, nullptr, 0);
    }
    launch_copy(n, z, p, st_);
    ks_.active = true;
    return fault_;
}

// One pass of the loop body of Solver_PCG_1 / Solver_CG_1 (src/AMG_main_solvers.cpp:138-152,
// :72-79) as stream work only; slot = residual-history index, or -1 to take it from the device
// counter (graph replay).
void Engine::pcg_body(bool precond, int slot)
{
    const int n = lev_[0].n;
    double *r = work_[0], *p = work_[1], *Ap = work_[2];
    double *x = ks_.x;
    int nb = 0;
    CsrArgs a;
    a.x = p;
    a.y = Ap;
    a.partial = part0_;
    const int np = apply_A(lev_[0], OP_SPMV_DOT, a);  // Ap = A p ; p.Ap
    finalize(precond ? FIN_PCG_ALPHA : FIN_CG_ALPHA, part0_, nullptr, np, 0, nullptr, 0);
    // x += alpha p ; r -= alpha Ap ; r.r -- with a preconditioner the r.r partials wait in part1_ and
    // are reduced together with z.r after the V-cycle: one finalize launch (one all-reduce) less
    // with the fp64 V-cycle behind it the update also writes the cycle's zero-guess sweep of level 0 (z0 = omega r / d)
    // (... unless the cycle's first launch on level 0 is the three-sweep one, which reads r alone)
    const bool fuse_zero = cfg_.fuse_cg_zero && precond && !f32_ready_ && jacobi_on() && cycle_kind_ == SPARSH_CYCLE_V && lev_.size() > 1 && !lev_[0].deep && prm_.sweeps > 0 &&
                           !(prm_.sweeps >= 3 && zero_start(lev_[0]));
    // with the fp64 V-cycle behind it x += alpha p waits for the direction update at the end of this iteration (one read of p for both)
    const bool defer_x = cfg_.defer_x && precond && !f32_ready_;
    double *x_now = defer_x ? nullptr : x;
    if (fuse_zero)
        launch_cg_update_zero(n, scal_, p, Ap, x_now, r, part1_, &nb, diag_stream(lev_[0]), lev_[0].diag_const, prm_.omega, lev_[0].x, st_, cfg_.cg_nt);
    else
        launch_cg_update(n, scal_, p, Ap, x_now, r, precond ? part1_ : part0_, &nb, st_);
    if (precond) {
        const int nb_rr = nb;
        const double *z = precondition(r, work_[4], part0_, &nb, fuse_zero);  // z0 = M r0 ; fused z0.r0
        finalize(FIN_PCG_BETA_RES, part0_, part1_, nb, 0, hist_dev_, slot, nb_rr);
        if (defer_x) launch_xp_update(n, scal_, z, p, x, st_);  // x += alpha p ; p = z0 + beta p
        else launch_p_update(n, scal_, z, p, st_);                // p = z0 + beta p
    } else {
        finalize(FIN_CG_BETA, part0_, nullptr, nb, 0, hist_dev_, slot);
        launch_p_update(n, scal_, r, p, st_);
    }
}

void Engine::drop_graph()
{
    if (graph_.exec) HIPCHK(hipGraphExecDestroy(graph_.exec));
    if (graph_.graph) HIPCHK(hipGraphDestroy(graph_.graph));
    graph_ = GraphState();
}

// Capture one PCG iteration (≈230 kernel launches at 13 levels) into a hipGraph.  Every buffer
// the iteration touches is engine-owned and fixed; the Jacobi ping-pong makes a V-cycle from a
// zero guess start and end in fixed buffers, so the captured launches stay valid for every
// later iteration and solve on the same x vector.
bool Engine::capture_graph(bool precond)
{
    drop_graph();
    if (hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
    pcg_body(precond, -1);
    hipGraph_t g = nullptr;
    if (hipStreamEndCapture(st_, &g) != hipSuccess || !g) return false;
    hipGraphExec_t e = nullptr;
    if (hipGraphInstantiate(&e, g, nullptr, nullptr, 0) != hipSuccess) {
        HIPCHK(hipGraphDestroy(g));
        return false;
    }
    graph_.graph = g;
    graph_.exec = e;
    graph_.x = ks_.x;
    graph_.precond = precond;
    return true;
}

int Engine::pcg_steps(int nsteps, int *done)
{
    if (!ks_.active) {
        error = "krylov_init has not been called";
        return SPARSH_ESTATE;
    }
    const bool precond = ks_.precond;
    if (int rc = krylov_prepare(precond ? SPARSH_PCG : SPARSH_CG); rc != SPARSH_OK) {
        if (done) *done = 0;
        return rc;
    }
    int rc = SPARSH_OK;
    int did = 0;
    // hipGraph replay: single GPU, no per-launch profiling events
    // (the W-cycle launches eagerly: its WK levels exchange their buffers from one inner cycle to the next)
    // (under a constant null space use_graph is accepted and ignored)
    bool use_graph = prm_.use_graph && !dist_ && !prof.enabled && (int)lev_.size() > 1 && (!precond || cycle_kind_ == SPARSH_CYCLE_V) && !ns_on();
    if (use_graph && !(graph_.exec && graph_.x == ks_.x && graph_.precond == precond)) use_graph = capture_graph(precond);
    if (use_graph) HIPCHK(hipMemcpyAsync(iter_ctr_, &ks_.count, sizeof(int), hipMemcpyHostToDevice, st_));
    while (ks_.count < lev_[0].nglob && ks_.r1 > prm_.tol && did < nsteps && fault_ == SPARSH_OK) {
        const int count = ++ks_.count;
        ++did;
        const int slot = std::min(count - 1, hist_cap_dev_ - 1);
        if (use_graph)
            HIPCHK(hipGraphLaunch(graph_.exec, st_));
        else
            pcg_body(precond, slot);
        if (read_due(count, did >= nsteps) && !read_residual(slot, count, ks_.r1)) {
            rc = SPARSH_ENUMERIC;
            break;
        }
    }
    if (ns_on()) {
        project(ks_.x);  // rounding drift of the mean
        HIPCHK(hipStreamSynchronize(st_));  // the call returns with the stream idle, as it does without a null space
    }
    if (done) *done = did;
    return fault_ != SPARSH_OK ? fault_ : rc;
}

int Engine::krylov_hist(double *hist, int hist_cap)
{
    HIPCHK(hipStreamSynchronize(st_));
    copy_hist(ks_.count, hist, hist_cap);
    return ks_.count;
}

int Engine::pcg(const double *b, double *x, int max_iters, double *hist, int hist_cap, int *iters, bool precond)
{
    int rc = pcg_init(b, x, precond);
    if (rc != SPARSH_OK) return rc;
    int did = 0;
    rc = pcg_steps(max_iters, &did);
    if (rc == SPARSH_OK && ks_.r1 > prm_.tol && ks_.count < lev_[0].nglob) rc = SPARSH_ENOCONV;
    if (fault_ != SPARSH_OK) rc = fault_;
    const int count = krylov_hist(hist, hist_cap);
    if (iters) *iters = count;
    ks_.active = false;
    return rc;
}

// Solver_BiCG_1 (precond = false) / Solver_PBiCG_1 (precond = true).
int Engine::bicg(const double *b, double *x, int max_iters, double *hist, int hist_cap, int *iters, bool precond)
{
    if (int rc = krylov_prepare(precond ? SPARSH_PBICG : SPARSH_BICG); rc != SPARSH_OK) return rc;
    const int n = lev_[0].n;
    double *r0 = work_[0], *r = work_[1], *p = work_[2], *Ap = work_[3], *s = work_[4], *As = work_[5], *p1buf = work_[6];
    const double *xin = krylov_start(b, x, work_[7]);
    op_residual(0, b, xin, r0);
    launch_copy(n, r0, r, st_);
    launch_copy(n, r0, p, st_);
    const double res0 = residual_norm(r0);
    int count = 0;
    const int rc = krylov_loop(res0, max_iters, 0, count, [&](int slot) {  // (print_solve numbers BiCGStab's iterations from 0)
        int nb = 0;
        const double *p1 = p;
        if (precond) {
            const double *z = precondition(p, p1buf);  // p1 = M p, kept in p1buf: the second application overwrites the cycle's own buffer
            if (z != p1buf) launch_copy(n, z, p1buf, st_);
            p1 = p1buf;
        }
        op_spmv(0, p1, Ap);
        launch_dot2(n, r, r0, Ap, r0, part0_, part1_, &nb, st_);  // alpha1 = r.r0 ; Ap.r0
        finalize(FIN_BICG_ALPHA, part0_, part1_, nb, 0, nullptr, 0);
        launch_bicg_s(n, scal_, r, Ap, s, st_);
        const double *s1 = s;
        if (precond) s1 = precondition(s, work_[7]);  // s1 = M s
        op_spmv(0, s1, As);
        launch_dot2(n, As, s, As, As, part0_, part1_, &nb, st_);
        finalize(FIN_BICG_OMEGA, part0_, part1_, nb, 0, nullptr, 0);
        launch_bicg_xr(n, scal_, p1, s1, s, As, r0, x, r, part0_, part1_, &nb, st_);
        finalize(FIN_BICG_BETA, part0_, part1_, nb, 0, hist_dev_, slot);
        launch_bicg_p(n, scal_, r, Ap, p, st_);
    });
    return krylov_finish(x, count, rc, hist, hist_cap, iters);
}

// Flexible CG, Notay's FCG(1): PCG whose new direction is made A-orthogonal to the previous one explicitly (beta = -z.Ap / p.Ap), so
// the preconditioner may change from one application to the next (the K-cycle).  With a fixed symmetric M it is PCG in exact arithmetic.
int Engine::fcg(const double *b, double *x, int max_iters, double *hist, int hist_cap, int *iters)
{
    if (int rc = krylov_prepare(SPARSH_FCG); rc != SPARSH_OK) return rc;
    const int n = lev_[0].n;
    double *r = work_[0], *p = work_[1], *Ap = work_[2];
    int nb = 0;
    krylov_start(b, x, nullptr);
    op_residual(0, b, x, r);  // r0 = b - A x
    const double res0 = residual_norm(r);
    if (res0 > prm_.tol) {
        const double *z = precondition(r, work_[4]);  // z0 = M r0
        launch_dot(n, z, r, part0_, &nb, st_);
        finalize(FIN_STORE, part0_, nullptr, nb, S_RZ, nullptr, 0);  // rho = z0.r0
        launch_copy(n, z, p, st_);
    }
    int count = 0;
    const int rc = krylov_loop(res0, max_iters, 1, count, [&](int slot) {
        CsrArgs a;
        a.x = p;
        a.y = Ap;
        a.partial = part0_;
        const int np = apply_A(lev_[0], OP_SPMV_DOT, a);  // q = A p ; sigma = p.q
        finalize(FIN_PCG_ALPHA, part0_, nullptr, np, 0, nullptr, 0);  // alpha = rho / sigma
        launch_cg_update(n, scal_, p, Ap, x, r, part1_, &nb, st_);   // x += alpha p ; r -= alpha q ; r.r
        finalize(FIN_SQRT, part1_, nullptr, nb, S_RES, hist_dev_, slot);
        const double *z = precondition(r, work_[4]);                // z = M r
        launch_dot2(n, z, r, z, Ap, part0_, part1_, &nb, st_);       // rho = z.r ; tau = z.q
        finalize(FIN_FCG_BETA, part0_, part1_, nb, 0, nullptr, 0);  // beta = -tau / sigma
        launch_p_update(n, scal_, z, p, st_);                        // p = z + beta p
    });
    return krylov_finish(x, count, rc, hist, hist_cap, iters);
}

// ---- restarted GMRES, right-preconditioned
int Engine::set_gmres(int restart)
{
    if (restart < 0 || restart > kGmresMaxRestart) {
        error = "restart must be in 1.." + std::to_string(kGmresMaxRestart) + " (0: the default of " + std::to_string(kGmresDefaultRestart) + ")";
        return SPARSH_EINVAL;
    }
    const int m = restart == 0 ? kGmresDefaultRestart : restart;
    if (m != gm_restart_) gmres_release();
    gm_restart_ = m;
    return SPARSH_OK;
}

int Engine::set_gmres_basis(int precision)
{
    if (precision != SPARSH_BASIS_FP64 && precision != SPARSH_BASIS_FP32) {
        error = "basis precision must be SPARSH_BASIS_FP64 (0) or SPARSH_BASIS_FP32 (1)";
        return SPARSH_EINVAL;
    }
    if (precision != gm_prec_) gmres_release();
    gm_prec_ = precision;
    return SPARSH_OK;
}

void Engine::gmres_release()
{
    if ((gm_basis_ || gm_basisf_) && st_) (void)hipStreamSynchronize(st_);
    dfree(gm_basis_);
    dfree(gm_basisf_);
    dfree(gm_w_);
    dfree(gm_part_);
    dfree(gm_state_);
    gm_basis_ = gm_part_ = gm_state_ = gm_w_ = nullptr;
    gm_basisf_ = nullptr;
    gm_bytes_ = 0;
}

// The layout the Gram-Schmidt kernels read: 16-byte aligned vectors (n rounded up to 2 doubles or to 4 floats); the float kernels
// load whole groups of 4 rows, so a float basis is zeroed: zeros behind row n, which no kernel overwrites with anything else.
size_t Engine::gmres_basis_alloc(int n, int nvec, int precision, double *&basis, float *&basisf, long &stride)
{
    const bool f32b = precision == SPARSH_BASIS_FP32;
    basis = nullptr, basisf = nullptr;
    stride = f32b ? ((long)n + 3) & ~3L : ((long)n + 1) & ~1L;
    const size_t bytes = (size_t)nvec * (size_t)stride * (f32b ? 4 : 8);
    void *p = dalloc(bytes);
    if (!p) return 0;
    if (f32b && !check(hipMemsetAsync(p, 0, bytes, st_), "hipMemsetAsync")) {
        dfree(p);
        return 0;
    }
    if (f32b) basisf = static_cast<float *>(p);
    else basis = static_cast<double *>(p);
    return bytes;
}

double *Engine::gmres_state_alloc(GmresState &s)
{
    double *mem = static_cast<double *>(dalloc((size_t)kGmresStateDoubles * 8));
    if (!mem) return nullptr;
    if (!check(hipMemsetAsync(mem, 0, (size_t)kGmresStateDoubles * 8, st_), "hipMemsetAsync")) {
        dfree(mem);
        return nullptr;
    }
    double *q = mem;
    s.hcol = q, q += kGmresMaxRestart + 2;
    s.ccol = q, q += kGmresMaxRestart + 2;
    s.R = q, q += kGmresMaxRestart * kGmresMaxRestart;
    s.cs = q, q += kGmresMaxRestart;
    s.sn = q, q += kGmresMaxRestart;
    s.g = q, q += kGmresMaxRestart + 1;
    s.ny = q, q += kGmresMaxRestart;
    s.hnext = q;
    return mem;
}

int Engine::gmres_reserve()
{
    if (gm_basis_ || gm_basisf_) return SPARSH_OK;
    const int n = lev_[0].n, m = gm_restart_;
    const bool f32b = gm_prec_ == SPARSH_BASIS_FP32;
    const size_t basis = gmres_basis_alloc(n, m + 1, gm_prec_, gm_basis_, gm_basisf_, gm_stride_);
    const size_t wvec = f32b ? (size_t)gm_stride_ * 8 : 0;
    const size_t part = (size_t)(m + 1) * (size_t)gs_grid(n) * 8;  // m sums against the basis + w.w, gs_grid(n) workgroups each
    if (basis && f32b) gm_w_ = static_cast<double *>(dalloc(wvec));
    if (basis) gm_part_ = static_cast<double *>(dalloc(part));
    if (basis) gm_state_ = gmres_state_alloc(gm_);
    if (!basis || (f32b && !gm_w_) || !gm_part_ || !gm_state_) {
        gmres_release();
        const size_t want = (size_t)(m + 1) * (size_t)gm_stride_ * (f32b ? 4 : 8);
        error = "GMRES basis of " + std::to_string(m + 1) + " vectors (" + std::to_string(want >> 20) + " MiB) does not fit the device: " + error;
        return SPARSH_ENODEV;
    }
    if (f32b && !check(hipMemsetAsync(gm_w_, 0, wvec, st_), "hipMemsetAsync")) return SPARSH_ENODEV;
    gm_bytes_ = basis + part + wvec;
    return SPARSH_OK;
}

// Classical Gram-Schmidt twice on w = v_{j+1} against v_0..v_j: V^T w, w -= V h and V^T w_new in one pass, w -= V c and ||w||^2 in
// one pass; then the one-workgroup kernel that rotates the column, and the normalisation as a launch of its own.
// Float basis: w is gm_w_, the sums run against the stored (rounded) vectors, and the normalisation writes the float v_{j+1} and its
// widened copy `feed`, the input of the next step's M / A.
void Engine::gmres_orthogonalise(int j, int slot, double *feed)
{
    const int n = lev_[0].n, nv = j + 1, g = gs_grid(n), m = gm_restart_;
    double *ww = gm_part_ + (size_t)m * g;
    auto against = [&](auto *basis, double *w) {  // the launches are overloaded on the basis' type
        launch_gs_dot(n, gm_stride_, basis, nv, w, gm_part_, nullptr, st_);
        launch_gs_finalize(gm_part_, g, nv, gm_.hcol, st_);
        launch_gs_update(n, gm_stride_, basis, nv, gm_.hcol, w, w, gm_part_, nullptr, st_);
        launch_gs_finalize(gm_part_, g, nv, gm_.ccol, st_);
        launch_gs_update(n, gm_stride_, basis, nv, gm_.ccol, w, w, nullptr, ww, st_);
        launch_gmres_step(j, ww, g, gm_, scal_ + S_RES, hist_dev_, slot, st_);
    };
    if (gm_prec_ == SPARSH_BASIS_FP32) {
        against(gm_basisf_, gm_w_);
        launch_gs_scale(n, gm_w_, gm_vecf(j + 1), feed, gm_.hnext, st_);
    } else {
        against(gm_basis_, gm_vec(j + 1));
        launch_gs_scale(n, gm_vec(j + 1), gm_.hnext, st_);
    }
}

int Engine::gmres(const double *b, double *x, int max_iters, double *hist, int hist_cap, int *iters, bool precond)
{
    if (int rc = krylov_prepare(precond ? SPARSH_PGMRES : SPARSH_GMRES); rc != SPARSH_OK) return rc;
    if (int rc = gmres_reserve(); rc != SPARSH_OK) return rc;
    const int n = lev_[0].n, m = gm_restart_;
    const bool f32b = gm_prec_ == SPARSH_BASIS_FP32;
    double *u = work_[0], *z32 = work_[4];
    double *feed = work_[2];  // float basis: v_j as stored, widened to double
    int it = 0, rc = SPARSH_OK;
    krylov_start(b, x, nullptr);
    // z = M v (nullptr: the identity); the fp64 cycle leaves z in lev_[0].x, which belongs to the cycle: consumed by the next launch
    auto apply_M = [&](const double *v) { return precond ? precondition(v, z32) : v; };
    // The only exit with SPARSH_OK is the true residual of a cycle start being <= tol.  |g_{j+1}| <= tol only ends the cycle, which
    // matters under a float basis, where |g_{j+1}| is an estimate of the residual: the next cycle start decides.
    for (;;) {  // one restart cycle
        if (fault_ != SPARSH_OK) break;
        double *r = f32b ? gm_w_ : gm_vec(0);
        op_residual(0, b, x, r);  // true residual
        const double beta = residual_norm(r);
        if (!(beta == beta)) {
            rc = SPARSH_ENUMERIC;
            break;
        }
        if (beta <= prm_.tol) break;
        if (it >= max_iters) {
            rc = SPARSH_ENOCONV;
            break;
        }
        // v_0 = r / beta
        if (f32b) launch_gs_scale(n, r, gm_vecf(0), feed, scal_ + S_RES, st_);
        else launch_gs_scale(n, r, scal_ + S_RES, st_);
        int steps = 0;
        for (int j = 0; j < m && it < max_iters; ++j) {
            op_spmv(0, apply_M(f32b ? feed : gm_vec(j)), f32b ? gm_w_ : gm_vec(j + 1));  // w = A M v_j
            const int slot = std::min(it, hist_cap_dev_ - 1);
            gmres_orthogonalise(j, slot, feed);
            ++it;
            ++steps;
            if (read_due(it, it >= max_iters)) {
                double res;
                if (!read_residual(slot, it, res)) {
                    rc = SPARSH_ENUMERIC;
                    break;
                }
                if (res <= prm_.tol) break;
            }
            if (fault_ != SPARSH_OK) break;
        }
        if (rc != SPARSH_OK || fault_ != SPARSH_OK) break;
        // x += M (V y), y = R^{-1} g over the steps taken; u = 0 - V (-y)
        launch_gmres_solve(steps, gm_, st_);
        if (f32b) launch_gs_update(n, gm_stride_, gm_basisf_, steps, gm_.ny, nullptr, u, nullptr, nullptr, st_);
        else launch_gs_update(n, gm_stride_, gm_basis_, steps, gm_.ny, nullptr, u, nullptr, nullptr, st_);
        launch_axpby(n, 1.0, apply_M(u), 1.0, x, st_);
    }
    return krylov_finish(x, it, rc, hist, hist_cap, iters);
}

int Engine::gmres_bench_prepare()
{
    if (dist_) return SPARSH_EINVAL;
    if (int rc = gmres_reserve(); rc != SPARSH_OK) return rc;
    // gmres_reserve zeroes a new float basis on st_, which the copies below (null stream) are not ordered against
    if (!check(hipStreamSynchronize(st_), "hipStreamSynchronize")) return SPARSH_ENODEV;
    const int n = lev_[0].n, m = gm_restart_;
    std::vector<double> pat((size_t)n + m + 1);
    const double scale = 1.0 / (6.0 * std::sqrt((double)n));
    for (size_t i = 0; i < pat.size(); ++i) pat[i] = (double)((long)((i * 7919) % 13) - 6) * scale;
    if (gm_prec_ == SPARSH_BASIS_FP32) {
        std::vector<float> patf(pat.size());
        for (size_t i = 0; i < pat.size(); ++i) patf[i] = (float)pat[i];
        for (int k = 0; k <= m; ++k)
            if (!check(hipMemcpy(gm_vecf(k), patf.data() + k, (size_t)n * 4, hipMemcpyHostToDevice), "hipMemcpy")) return SPARSH_ENODEV;
    } else {
        for (int k = 0; k <= m; ++k)
            if (!check(hipMemcpy(gm_vec(k), pat.data() + k, (size_t)n * 8, hipMemcpyHostToDevice), "hipMemcpy")) return SPARSH_ENODEV;
    }
    if (!check(hipMemcpy(work_[1], pat.data() + m + 1, (size_t)n * 8, hipMemcpyHostToDevice), "hipMemcpy")) return SPARSH_ENODEV;
    return SPARSH_OK;
}

void Engine::gmres_bench_step(bool fused)
{
    const int n = lev_[0].n, j = gm_restart_ - 1, nv = j + 1;  // the last step of a cycle
    double *w = gm_prec_ == SPARSH_BASIS_FP32 ? gm_w_ : gm_vec(j + 1);
    launch_copy(n, work_[1], w, st_);  // (stands for the SpMV's store of w; keeps the values bounded over repetitions)
    if (fused) {
        gmres_orthogonalise(j, hist_cap_dev_ - 1, work_[2]);
        return;
    }
    // what the fused kernels replace: a launch_dot + reduction per coefficient and an axpby per basis vector, twice, then the norm
    // and the scaling (coefficients through the host would add a read-back each; a fixed one stands in)
    int nb = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < nv; ++k) {
            launch_dot(n, gm_vec(k), w, part0_, &nb, st_);
            finalize(FIN_STORE, part0_, nullptr, nb, S_TMP, nullptr, 0);
        }
        for (int k = 0; k < nv; ++k) launch_axpby(n, -1e-3, gm_vec(k), 1.0, w, st_);
    }
    launch_dot(n, w, w, part0_, &nb, st_);
    finalize(FIN_STORE, part0_, nullptr, nb, S_TMP, nullptr, 0);
    launch_axpby(n, 0.0, gm_vec(0), 0.5, w, st_);
}

}  // namespace sparsh
