// engine_eig.cpp -- the lowest eigenpairs of the SPD level-0 operator by LOBPCG, preconditioned with the block V-cycle (DESIGN.md
// section 5i).
//
// The device keeps the search space S = [X, W, P] and A S as interleaved blocks and computes the Gram matrices S^T S and S^T A S; the
// host solves the small pencil (eig_small.cpp) on the rows and columns of the active columns and sends back the coefficients of the
// update.  One iteration is one host synchronisation.  The cycle and the block SpMV are those of engine_multi.cpp (vcycle_multi,
// multi_spmv_dot) and run in the block path's level buffers, which hold nothing between calls; everything that carries state here is
// the solver's own allocation.
#include "eig_small.hpp"
#include "engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace sparsh {

#define HIPCHK(call) note_hip((call), #call)

namespace {

// both Gram matrices and the residual norms, then the three masks of the ortho basis
constexpr int kEigPinnedDown = 2 * kEigSmallMax * kEigSmallMax + kMultiMax + 3 * kMultiMax;
constexpr int kEigPinnedUp = 3 * kMultiMax * kMultiMax + kMultiMax;          // Cx, Cw, Cp and theta

}  // namespace

void Engine::eig_forget()
{
    ew_ = 0;
    eig_bytes_ = 0;
    eig_restarts_ = 0;
    eig_allocs_.clear();
    eX_ = eAX_ = eW_ = eAW_ = eP_ = eAP_ = eR_ = epart_ = eG_ = ecoef_ = nullptr;
    eBX_ = eBW_ = eBP_ = nullptr;
    eig_con_forget();
    eig_ortho_forget();
}

void Engine::eig_ortho_forget()
{
    ortho_bytes_ = 0;
    ortho_allocs_.clear();
    oM_ = oG_ = oT_ = nullptr;
}

void Engine::eig_ortho_release()
{
    if (st_ && !ortho_allocs_.empty()) (void)hipStreamSynchronize(st_);
    for (void *p : ortho_allocs_) dfree(p);
    eig_ortho_forget();
}

// the handle's settings; a change of basis gives the mode's own memory back
int Engine::set_eig_options(int basis, int wanted)
{
    if (basis != eig_basis_) eig_ortho_release();
    eig_basis_ = basis;
    eig_wanted_ = wanted;
    return SPARSH_OK;
}

// the masks and the two small matrices at the width in force (a change of width has dropped them with the blocks)
int Engine::eig_ortho_reserve()
{
    if (oM_) return SPARSH_OK;
    const int W = ew_;
    bool ok = true;
    auto take = [&](size_t doubles) { return take_zeroed(ortho_allocs_, ortho_bytes_, ok, doubles); };
    oM_ = take((size_t)3 * W);
    oG_ = take((size_t)W * W);
    oT_ = take((size_t)W * W);
    if (!ok) {
        eig_ortho_release();
        return SPARSH_ENODEV;
    }
    return SPARSH_OK;
}

// (the Gram partials are free wherever the loop orthonormalises: the launches that filled them last have been read out on the stream)
void Engine::eig_ortho_pass(int k, double *V, double *BV, double *AV, const double *mask_in, double *mask_out)
{
    const int n = lev_[0].n, W = ew_;
    GramPairs one{};
    one.u[0] = V;
    one.v[0] = BV ? BV : V;
    one.dst[0] = 0;
    launch_gram_multi(n, W, 1, one, epart_, oG_, W, st_);
    launch_eig_chol_small(W, oG_, mask_in, oT_, mask_out, st_);
    double *blocks[3] = {V, nullptr, nullptr};
    int nb = 1;
    if (BV) blocks[nb++] = BV;
    if (AV) blocks[nb++] = AV;
    launch_eig_transform(n, W, k, nb, blocks, oT_, st_);
}

void Engine::eig_con_forget()
{
    con_mt_ = 0;
    con_gen_ = false;
    con_bytes_ = 0;
    con_allocs_.clear();
    cY_ = cBY_ = cG_ = cGinv_ = cC_ = nullptr;
}

void Engine::eig_release()
{
    if (st_ && !(eig_allocs_.empty() && con_allocs_.empty() && ortho_allocs_.empty())) (void)hipStreamSynchronize(st_);
    for (void *p : eig_allocs_) dfree(p);
    for (void *p : con_allocs_) dfree(p);
    for (void *p : ortho_allocs_) dfree(p);
    eig_forget();
}

void Engine::eig_con_release()
{
    if (st_ && !con_allocs_.empty()) (void)hipStreamSynchronize(st_);
    for (void *p : con_allocs_) dfree(p);
    eig_con_forget();
}

// the constraint blocks of one call shape (width ew_, mt constraints, B Y beside Y or not); another shape replaces them
int Engine::eig_con_reserve(int mt, bool gen)
{
    if (mt == con_mt_ && gen == con_gen_) return SPARSH_OK;
    eig_con_release();
    const int W = ew_, nblk = (mt + W - 1) / W, mpad = nblk * W;
    bool ok = true;
    auto take = [&](size_t doubles) { return take_zeroed(con_allocs_, con_bytes_, ok, doubles); };
    const size_t len = (size_t)lev_[0].n * W;
    cY_ = take(len * nblk);
    cBY_ = gen ? take(len * nblk) : cY_;
    cG_ = take((size_t)mpad * mpad);
    cGinv_ = take((size_t)mt * mt);
    cC_ = take((size_t)mpad * W);
    if (!ok) {
        eig_con_release();
        return SPARSH_ENODEV;
    }
    con_mt_ = mt;
    con_gen_ = gen;
    return SPARSH_OK;
}

// (the Gram partials are free wherever the loop projects: the launches that filled them last have been read out on the stream)
void Engine::eig_con_project(const double *src, double *dst)
{
    launch_eig_con_project(lev_[0].n, ew_, con_mt_, cY_, cBY_, cGinv_, src, dst, cC_, epart_, st_);
}

int Engine::eig_reserve(int nev)
{
    const int W = multi_width(nev);
    if (W == ew_) return SPARSH_OK;
    eig_release();
    bool ok = true;
    auto take = [&](size_t doubles) { return take_zeroed(eig_allocs_, eig_bytes_, ok, doubles); };
    const size_t len = (size_t)lev_[0].n * W;
    double **blocks[7] = {&eX_, &eAX_, &eW_, &eAW_, &eP_, &eAP_, &eR_};
    for (double **b : blocks) *b = take(len);
    epart_ = take((size_t)(kEigPairs * W * W + W) * kEigMaxGrid);  // Gram partials, then the residual's
    eG_ = take((size_t)2 * 9 * W * W + W);                         // S^T S, S^T A S (order 3 W each), residual norms
    ecoef_ = take((size_t)3 * W * W + W);                          // Cx, Cw, Cp, theta
    if (ok && !epinned_)
        ok = check(hipHostMalloc(reinterpret_cast<void **>(&epinned_), (kEigPinnedDown + kEigPinnedUp) * sizeof(double), hipHostMallocDefault),
                   "hipHostMalloc");
    if (!ok) {
        eig_release();
        return SPARSH_ENODEV;
    }
    ew_ = W;
    return SPARSH_OK;
}

// the three blocks B X, B W, B P of the generalised solver, on top of eig_reserve's: a change of width drops them with the rest
int Engine::eig_reserve_gen(int nev)
{
    if (int rc = eig_reserve(nev); rc != SPARSH_OK) return rc;
    if (eBX_) return SPARSH_OK;
    bool ok = true;
    double **blocks[3] = {&eBX_, &eBW_, &eBP_};
    for (double **b : blocks) *b = take_zeroed(eig_allocs_, eig_bytes_, ok, (size_t)lev_[0].n * ew_);
    if (!ok) {
        eig_release();
        return SPARSH_ENODEV;
    }
    return SPARSH_OK;
}

void Engine::eig_b_spmv(const double *x, double *y)
{
    MultiArgs a;
    a.x = x;
    a.y = y;
    launch_csr_multi(eB_, ew_, OP_SPMV, a, st_, cfg_);
}

// the pair list of one Gram launch: X^T X and X^T AX first (the start needs these two only), then the rest of the upper block
// triangles of S^T S (at G) and S^T A S (at G + 9 W^2), S = [X, W, P].  gen: S^T B S in place of S^T S, from the pairs (S_i, B S_j)
void Engine::eig_gram_pairs(GramPairs &prs, bool gen) const
{
    const int W = ew_, ld = 3 * W;
    const double *S[3] = {eX_, eW_, eP_}, *AS[3] = {eAX_, eAW_, eAP_}, *BS[3] = {eBX_, eBW_, eBP_};
    int p = 0;
    auto add = [&](int bi, int bj, bool a) {
        prs.u[p] = S[bi];
        prs.v[p] = a ? AS[bj] : (gen ? BS[bj] : S[bj]);
        prs.dst[p] = (a ? ld * ld : 0) + bi * W * ld + bj * W;
        ++p;
    };
    add(0, 0, false);
    add(0, 0, true);
    for (int a = 0; a < 2; ++a)
        for (int bi = 0; bi < 3; ++bi)
            for (int bj = bi; bj < 3; ++bj)
                if (bi + bj > 0) add(bi, bj, a != 0);
}

int Engine::eigs_dev(int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap, int *iters,
                     int *status, double *seconds)
{
    return eigs_run(false, nev, X, ldx, tol, max_iters, lambda, hist, hist_cap, iters, status, seconds);
}

int Engine::eigs_gen_dev(int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap, int *iters,
                         int *status, double *seconds)
{
    return eigs_run(true, nev, X, ldx, tol, max_iters, lambda, hist, hist_cap, iters, status, seconds);
}

int Engine::eigs_con_dev(bool gen, int nev, double *X, long ldx, int ncon, const double *Y, long ldy, double tol, int max_iters, double *lambda,
                         double *hist, int hist_cap, int *iters, int *status, double *seconds)
{
    EigCon con;
    con.ncon = ncon;
    con.Y = Y;
    con.ldy = ldy;
    return eigs_run(gen, nev, X, ldx, tol, max_iters, lambda, hist, hist_cap, iters, status, seconds, &con);
}

// step 6 in place on the resident blocks
void Engine::eig_update(bool gen, int k)
{
    const int n = lev_[0].n;
    if (!gen) {
        launch_eig_update(n, ew_, k, eX_, eW_, eP_, eAX_, eAW_, eAP_, ecoef_, eX_, eP_, eAX_, eAP_, st_);
        return;
    }
    const double *in[9] = {eX_, eW_, eP_, eAX_, eAW_, eAP_, eBX_, eBW_, eBP_};
    double *out[6] = {eX_, eP_, eAX_, eAP_, eBX_, eBP_};
    launch_eig_update_gen(n, ew_, k, in, ecoef_, out, st_);
}

// the loop of both solvers.  gen: the pencil (A, B) with B S carried beside A S; the standard solve's launches are those it always had.
// con: the constrained entry points, which take null-space handles (the constant vector is then one more constraint); with no
// constraint at all the launches are those of con == nullptr.  The handle's basis (set_eig_options) picks the loop body: under the
// plain basis the launches are those the solver always had; under the ortho basis the active mask is decided on the device and W
// and P are B-orthonormalised before the Gram launch.  `wanted` ends a solve in either once the lowest `wanted` columns are inactive.
int Engine::eigs_run(bool gen, int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap, int *iters,
                     int *status, double *seconds, const EigCon *con)
{
    if (!ready_) {
        error = "sparsh_setup has not been called";
        return SPARSH_ESTATE;
    }
    if (fault_ != SPARSH_OK) return fault_;
    if (const char *why = con ? eig_con_refusal() : multi_refusal()) {
        error = why;
        return SPARSH_EINVAL;
    }
    const int ncon = con ? con->ncon : 0;
    const int mt = con ? ncon + (ns_on() ? 1 : 0) : 0;  // constraints in all
    if (ncon < 0 || mt > kEigConMax || nev + mt > lev_[0].n || (ncon > 0 && (!con->Y || con->ldy < lev_[0].n))) {
        error = "bad constraints: at most SPARSH_MAX_CON columns of n rows, and nev + their number must not exceed n";
        return SPARSH_EINVAL;
    }
    if (gen && !eb_set_) {
        error = "sparsh_eig_set_b has not been called: the generalised problem needs its B";
        return SPARSH_ESTATE;
    }
    if (int rc = multi_reserve(nev); rc != SPARSH_OK) return rc;  // the cycle's own blocks
    if (int rc = gen ? eig_reserve_gen(nev) : eig_reserve(nev); rc != SPARSH_OK) return rc;
    if (mt > 0)
        if (int rc = eig_con_reserve(mt, gen); rc != SPARSH_OK) return rc;
    const bool ortho = eig_basis_ == SPARSH_EIG_BASIS_ORTHO;
    if (eig_wanted_ > nev) {
        error = "wanted exceeds nev: sparsh_set_eig_options asked for more wanted columns than this solve has";
        return SPARSH_EINVAL;
    }
    if (ortho)
        if (int rc = eig_ortho_reserve(); rc != SPARSH_OK) return rc;
    const int need = (eig_wanted_ > 0 && eig_wanted_ < nev) ? eig_wanted_ : nev;  // the columns whose convergence ends the solve
    if (max_iters <= 0) max_iters = prm_.max_iter;
    const int W = ew_, n = lev_[0].n, k = nev, ld = 3 * W;
    const size_t len = (size_t)n * W;
    const int ndown = 2 * ld * ld + W, nup = 3 * W * W + W;
    double *down = epinned_, *up = epinned_ + kEigPinnedDown;
    eig_restarts_ = 0;
    eig_dropped_[0] = eig_dropped_[1] = 0;
    const double *mdown = down + ndown;  // the masks as they came down: active, W in the basis, P in the basis
    StreamClock clock(*this, seconds);
    GramPairs prs;
    eig_gram_pairs(prs, gen);
    double *norms = eG_ + 2 * ld * ld, *theta_dev = ecoef_ + 3 * W * W, *rpart = epart_ + (size_t)kEigPairs * W * W * kEigMaxGrid;
    // the generalised residual's second norm vector, ||B x_c||, travels in the first row of the (W, X) block of S^T B S: the Gram
    // launch fills the upper block triangle only and the host reads nothing below it
    double *bnorms = eG_ + (size_t)W * ld;
    double theta[kMultiMax] = {0}, rn[kMultiMax] = {0}, bn[kMultiMax] = {0};
    bool active[kMultiMax] = {false};
    double GA[kEigSmallMax * kEigSmallMax], GB[kEigSmallMax * kEigSmallMax], C[kEigSmallMax * kMultiMax];
    int idx[kEigSmallMax];

    auto read_down = [&](int first, int count) {  // G[first, first + count) -> down[first, ...), one pinned read (ortho: with the masks)
        if (ortho) HIPCHK(hipMemcpyAsync(down + ndown, oM_, (size_t)3 * W * 8, hipMemcpyDeviceToHost, st_));
        HIPCHK(hipMemcpyAsync(down + first, eG_ + first, (size_t)count * 8, hipMemcpyDeviceToHost, st_));
        HIPCHK(hipStreamSynchronize(st_));
    };
    // the compacted pencil on the rows and columns idx[0, m) of G, its k lowest pairs, and the coefficient matrices on their way up
    auto rayleigh_ritz = [&](int m) -> int {
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) {
                const int a = std::min(idx[i], idx[j]), b = std::max(idx[i], idx[j]);  // the device fills the upper block triangle
                GB[i * m + j] = down[a * ld + b];
                GA[i * m + j] = down[ld * ld + a * ld + b];
            }
        if (eig_small(m, k, GA, GB, theta, C) != 0) return 1;
        std::fill(up, up + nup, 0.0);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < k; ++j) up[(idx[i] / W) * W * W + (idx[i] % W) * W + j] = C[i * k + j];
        std::copy(theta, theta + k, up + 3 * W * W);
        HIPCHK(hipMemcpyAsync(ecoef_, up, (size_t)nup * 8, hipMemcpyHostToDevice, st_));
        return 0;
    };
    auto finite = [&](const double *p, int cnt) {
        for (int i = 0; i < cnt; ++i)
            if (!std::isfinite(p[i])) return false;
        return true;
    };
    auto numeric = [&](const char *what) {
        clock.stop();
        for (int c = 0; c < k; ++c) status[c] = SPARSH_ENUMERIC;
        if (fault_ != SPARSH_OK) return fault_;  // (a NaN that a failed launch left behind: the fault's own message stands)
        error = what;
        return (int)SPARSH_ENUMERIC;
    };

    // 1. start: AX = A X, Rayleigh-Ritz on (X^T AX, X^T X), X <- X C, AX <- AX C; no P yet
    for (int c = 0; c < k; ++c) iters[c] = 0, status[c] = SPARSH_OK;
    if (mt > 0) {
        // the constraints: Y in blocks of width W (a null-space handle's column of ones last), BY = B Y, G = Y^T (BY) from the Gram
        // launch, its inverse from the host: the one extra host read of a constrained call
        const int nblk = (mt + W - 1) / W, mpad = nblk * W;
        for (int b = 0; b < nblk; ++b) {
            const int cols = std::min(W, ncon - b * W);
            if (cols > 0) launch_interleave(n, cols, W, con->Y + (size_t)b * W * con->ldy, con->ldy, cY_ + b * len, st_);
            else HIPCHK(hipMemsetAsync(cY_ + b * len, 0, len * 8, st_));
        }
        if (mt > ncon) launch_eig_con_fill_column(n, W, ncon % W, 1.0, cY_ + (size_t)(ncon / W) * len, st_);
        if (gen)
            for (int b = 0; b < nblk; ++b) eig_b_spmv(cY_ + b * len, cBY_ + b * len);
        GramPairs cp{};
        int np = 0;
        auto flush = [&]() {
            if (np > 0) launch_gram_multi(n, W, np, cp, epart_, cG_, mpad, st_);
            np = 0;
        };
        for (int bi = 0; bi < nblk; ++bi)
            for (int bj = bi; bj < nblk; ++bj) {  // the upper block triangle, at most kEigPairs pairs per launch
                cp.u[np] = cY_ + bi * len;
                cp.v[np] = cBY_ + bj * len;
                cp.dst[np] = bi * W * mpad + bj * W;
                if (++np == kEigPairs) flush();
            }
        flush();
        HIPCHK(hipMemcpyAsync(down, cG_, (size_t)mpad * mpad * 8, hipMemcpyDeviceToHost, st_));
        HIPCHK(hipStreamSynchronize(st_));
        if (fault_ != SPARSH_OK) {
            clock.stop();
            return fault_;
        }
        double Gc[kEigConMax * kEigConMax], Gi[kEigConMax * kEigConMax];
        for (int i = 0; i < mt; ++i)
            for (int j = 0; j < mt; ++j) Gc[i * mt + j] = down[std::min(i, j) * mpad + std::max(i, j)];
        // constraints that cannot be used are not left in force: sparsh_eig_con_info reports zeros again
        if (!finite(Gc, mt * mt)) {
            eig_con_release();
            return numeric(gen ? "NaN in the constraints or in B times the constraints" : "NaN in the constraints");
        }
        if (eig_spd_inverse(mt, Gc, Gi) != 0) {
            eig_con_release();
            return numeric("the constraints are rank deficient");
        }
        std::copy(Gi, Gi + mt * mt, down);  // (the next device write to `down` follows this upload on the stream)
        HIPCHK(hipMemcpyAsync(cGinv_, down, (size_t)mt * mt * 8, hipMemcpyHostToDevice, st_));
    }
    launch_interleave(n, k, W, X, ldx, eX_, st_);
    if (mt > 0) eig_con_project(eX_, eX_);  // X <- Pi X before AX and BX are formed
    for (double *b : {eW_, eAW_, eP_, eAP_}) HIPCHK(hipMemsetAsync(b, 0, len * 8, st_));
    if (gen)
        for (double *b : {eBW_, eBP_}) HIPCHK(hipMemsetAsync(b, 0, len * 8, st_));
    HIPCHK(hipMemsetAsync(eG_, 0, (size_t)ndown * 8, st_));
    multi_spmv_dot(0, eX_, eAX_, mpart0_);
    if (gen) eig_b_spmv(eX_, eBX_);
    launch_gram_multi(n, W, 2, prs, epart_, eG_, ld, st_);
    read_down(0, 2 * ld * ld);
    for (int c = 0; c < k; ++c) idx[c] = c;
    if (fault_ != SPARSH_OK) {  // (the fault's own message stands)
        clock.stop();
        return fault_;
    }
    if (!finite(down, 2 * ld * ld))
        return numeric(gen ? "NaN in the start block or in A or B times the start block" : "NaN in the start block or in A times the start block");
    if (rayleigh_ritz(k) != 0)
        return numeric(gen ? "Rayleigh-Ritz breakdown at the start: the start block is rank deficient or B is not positive definite"
                           : "Rayleigh-Ritz breakdown at the start: the start block is rank deficient");
    eig_update(gen, k);  // (Cw = Cp = 0: P stays 0)

    bool have_p = false, converged = false;
    for (int it = 0; fault_ == SPARSH_OK; ++it) {
        // 2. residual; at the cap only its norms are wanted
        if (gen) launch_eig_residual_gen(n, W, eAX_, eBX_, theta_dev, eR_, epart_, norms, bnorms, st_);  // (the Gram partials are free here)
        else launch_eig_residual(n, W, eAX_, eX_, theta_dev, eR_, rpart, norms, st_);
        const bool last = it >= max_iters;
        if (ortho) launch_eig_active_mask(W, k, gen, tol, theta_dev, norms, gen ? bnorms : norms, oM_, st_);
        if (!last && ortho) {
            // P on its active columns, then 3. W = M R made B-orthogonal to X and B-orthonormalised twice (B W follows W by the same
            // transforms), AW = A W ; 4. the Gram matrices as in the plain loop
            if (have_p) eig_ortho_pass(k, eP_, gen ? eBP_ : nullptr, eAP_, oM_, oM_ + 2 * W);
            vcycle_multi(eR_);
            const double *w0 = mlev_[0].x;
            if (mt > 0) {
                eig_con_project(mlev_[0].x, eW_);
                w0 = eW_;
            }
            GramPairs one{};
            one.u[0] = gen ? eBX_ : eX_;
            one.v[0] = w0;
            one.dst[0] = 0;
            launch_gram_multi(n, W, 1, one, epart_, oG_, W, st_);                 // C = (BX)^T W0
            launch_eig_ortho_apply(n, W, k, eX_, oG_, oM_, w0, eW_, st_);         // stands in for the copy
            if (have_p) {
                // W against the orthonormalised P as well, in place: without it W and P grow parallel near convergence and the
                // Rayleigh-Ritz pencil loses its accuracy just above the breakdown rule (P's dropped and inactive columns are zero)
                one.u[0] = gen ? eBP_ : eP_;
                one.v[0] = eW_;
                launch_gram_multi(n, W, 1, one, epart_, oG_, W, st_);             // C = (BP)^T W
                launch_eig_ortho_apply(n, W, k, eP_, oG_, oM_, eW_, eW_, st_);
            }
            if (gen) eig_b_spmv(eW_, eBW_);
            eig_ortho_pass(k, eW_, gen ? eBW_ : nullptr, nullptr, oM_, oM_ + W);
            eig_ortho_pass(k, eW_, gen ? eBW_ : nullptr, nullptr, oM_ + W, oM_ + W);
            multi_spmv_dot(0, eW_, eAW_, mpart0_);
            launch_gram_multi(n, W, kEigPairs, prs, epart_, eG_, ld, st_);
            read_down(0, ndown);
        } else if (!last) {
            // 3. W = M R, AW = A W ; 4. the Gram matrices of S = [X, W, P] and A S
            vcycle_multi(eR_);
            if (mt > 0) eig_con_project(mlev_[0].x, eW_);  // W <- Pi (M R): the projection stands in for the copy
            else HIPCHK(hipMemcpyAsync(eW_, mlev_[0].x, len * 8, hipMemcpyDeviceToDevice, st_));
            multi_spmv_dot(0, eW_, eAW_, mpart0_);
            if (gen) eig_b_spmv(eW_, eBW_);
            launch_gram_multi(n, W, kEigPairs, prs, epart_, eG_, ld, st_);
            read_down(0, ndown);
        } else if (gen) {
            read_down(0, ndown);  // (both norm vectors; the Gram matrices are stale and not looked at)
        } else {
            read_down(2 * ld * ld, W);
        }
        if (fault_ != SPARSH_OK) break;
        std::copy(down + 2 * ld * ld, down + 2 * ld * ld + k, rn);
        if (!finite(rn, k)) return numeric("NaN residual in the eigensolver");
        if (gen) {
            std::copy(down + W * ld, down + W * ld + k, bn);
            if (!finite(bn, k)) return numeric("NaN in B times the Ritz vectors");
        }
        int nact = 0;
        for (int c = 0; c < k; ++c) {
            // re-evaluated every iteration: soft locking
            if (ortho) active[c] = mdown[c] != 0.0;  // decided on the device, not a second time here
            else active[c] = gen ? rn[c] > tol * std::fabs(theta[c]) * bn[c] : rn[c] > tol * std::fabs(theta[c]);
            nact += active[c];
            if (hist && it < hist_cap) hist[(size_t)c * hist_cap + it] = rn[c];
        }
        if (prm_.print_solve) std::printf("%d\t%d of %d eigenpairs active\n", it, nact, k);
        int nneed = 0;
        for (int c = 0; c < need; ++c) nneed += active[c];
        if (nneed == 0) {  // (need < k: the columns past it are guard vectors and come back as they stand)
            converged = true;
            break;
        }
        if (last) break;
        if (!finite(down, 2 * ld * ld)) return numeric("NaN in the Gram matrices of the eigensolver");
        // 5. Rayleigh-Ritz on [all of X, active of W, active of P]; after a breakdown once more without P
        int m = k;
        for (int c = 0; c < k; ++c)
            if (ortho ? mdown[W + c] != 0.0 : active[c]) idx[m++] = W + c;
        const int m_xw = m;
        if (have_p)
            for (int c = 0; c < k; ++c)
                if (ortho ? mdown[2 * W + c] != 0.0 : active[c]) idx[m++] = 2 * W + c;
        if (ortho)
            for (int c = 0; c < k; ++c) {
                eig_dropped_[0] += active[c] && mdown[W + c] == 0.0;
                eig_dropped_[1] += have_p && active[c] && mdown[2 * W + c] == 0.0;
            }
        if (rayleigh_ritz(m) != 0) {
            ++eig_restarts_;
            if (m == m_xw || rayleigh_ritz(m_xw) != 0)
                return numeric("Rayleigh-Ritz breakdown even after a restart without P (the start block had full rank)");
        }
        for (int c = 0; c < k; ++c) iters[c] += active[c];
        // 6. update
        eig_update(gen, k);
        have_p = true;
    }
    launch_deinterleave(n, k, W, eX_, X, ldx, st_);
    HIPCHK(hipStreamSynchronize(st_));
    clock.stop();
    note_hip(hipGetLastError(), "kernel launch during the eigensolve");
    if (fault_ != SPARSH_OK) return fault_;
    std::copy(theta, theta + k, lambda);
    for (int c = 0; c < k; ++c) status[c] = active[c] ? SPARSH_ENOCONV : SPARSH_OK;  // (after convergence: guard vectors still active)
    if (converged) return SPARSH_OK;
    error = gen ? "iteration cap reached before ||A x - lambda B x|| <= tol |lambda| ||B x|| for every eigenpair"
                : "iteration cap reached before ||A x - lambda x|| <= tol |lambda| for every eigenpair";
    return SPARSH_ENOCONV;
}

int Engine::bench_eig_launch(int op)
{
    const int n = lev_[0].n;
    if (op == 2) {
        GramPairs prs;
        eig_gram_pairs(prs);
        launch_gram_multi(n, ew_, kEigPairs, prs, epart_, eG_, 3 * ew_, st_);
    } else if (op == 4) {
        eig_update(true, ew_);
    } else if (op == 5) {
        eig_b_spmv(eX_, eBX_);
    } else {
        launch_eig_update(n, ew_, ew_, eX_, eW_, eP_, eAX_, eAW_, eAP_, ecoef_, eX_, eP_, eAX_, eAP_, st_);
    }
    return SPARSH_OK;
}

int Engine::bench_eig_ortho_launch(int op)
{
    const int n = lev_[0].n;
    if (op == 8) {
        double *blocks[3] = {eP_, eAP_, eBP_};
        launch_eig_transform(n, ew_, ew_, 3, blocks, oT_, st_);
    } else {
        launch_eig_ortho_apply(n, ew_, ew_, eX_, oG_, oM_, eW_, eW_, st_);
    }
    return SPARSH_OK;
}

int Engine::bench_eig_con_launch()
{
    eig_con_project(eW_, eW_);
    return SPARSH_OK;
}

int Engine::op_eig_b_multi(int nrhs, const double *X, double *Y)
{
    const int n = lev_[0].n, W = multi_width(nrhs);
    const size_t bytes = (size_t)n * W * 8;
    double *bx = static_cast<double *>(dalloc(bytes)), *by = static_cast<double *>(dalloc(bytes));
    if (bx && by) {
        launch_interleave(n, nrhs, W, X, n, bx, st_);
        MultiArgs a;
        a.x = bx;
        a.y = by;
        launch_csr_multi(eB_, W, OP_SPMV, a, st_, cfg_);
        launch_deinterleave(n, nrhs, W, by, Y, n, st_);
        HIPCHK(hipStreamSynchronize(st_));
    }
    dfree(bx);
    dfree(by);
    if (!bx || !by) return SPARSH_ENODEV;
    return fault_;
}

}  // namespace sparsh
