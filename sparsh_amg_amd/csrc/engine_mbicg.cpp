// engine_mbicg.cpp -- block BiCGStab on the block path: up to 8 right-hand sides of an unsymmetric system
// through two block V-cycles and two block SpMVs per iteration.
//
// Per column the loop is Engine::bicg(precond = true): the expressions of bicg_s / bicg_xr / bicg_p and of FIN_BICG_ALPHA / OMEGA /
// BETA.  It runs on the block vectors of engine_multi.cpp (x, r, p, Ap and the cycle's level blocks) and four blocks of its own (r0,
// s, As, p1); its kernels are in mbicg_kernels.hip.  Every scalar stays on the device, one set per column, and a column is frozen
// there when its residual reaches tol (block PCG's scheme, not block CG's coupling); the host reads 24 flags every
// params.check_every iterations.
#include "engine.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace sparsh {

#define HIPCHK(call) note_hip((call), #call)

int Engine::mbicg_reserve()
{
    if (mb_.scal) return SPARSH_OK;  // reserved for the width in force (a change of width released everything)
    bool ok = true;
    size_t bytes = 0;
    auto take = [&](size_t doubles) -> double * {
        if (!ok) return nullptr;
        double *p = static_cast<double *>(dalloc(doubles * 8));
        if (!p || !check(hipMemsetAsync(p, 0, doubles * 8, st_), "hipMemsetAsync")) {
            ok = false;
            if (p) dfree(p);
            return nullptr;
        }
        multi_allocs_.push_back(p);
        bytes += doubles * 8;
        return p;
    };
    const size_t len0 = std::max<size_t>((size_t)lev_[0].n * mw_, 1);
    double *r0 = take(len0), *s = take(len0), *as = take(len0), *p1 = take(len0);
    double *scal = take((size_t)MB_COUNT * kMultiMax);
    int *flags = reinterpret_cast<int *>(take((3 * kMultiMax + 1) / 2));
    if (!ok) {
        multi_release();
        return SPARSH_ENODEV;
    }
    mb_r0_ = r0;
    mb_s_ = s;
    mb_as_ = as;
    mb_p1_ = p1;
    mb_.scal = scal;
    mb_.frozen = flags;
    mb_.iters = flags + kMultiMax;
    mb_.status = flags + 2 * kMultiMax;
    mbicg_bytes_ = bytes;
    return SPARSH_OK;
}

int Engine::solve_mbicg_dev(int nrhs, const double *B, long ldb, double *X, long ldx, int max_iters, double *hist, int hist_cap, int *iters,
                            int *status, double *seconds)
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
    if (int rc = mbicg_reserve(); rc != SPARSH_OK) return rc;
    if (max_iters <= 0) max_iters = prm_.max_iter;
    max_iters = std::min(max_iters, lev_[0].nglob);
    const int W = mw_, n = lev_[0].n;
    const size_t bytes0 = (size_t)n * W * 8;
    const int check_every = std::max(1, prm_.check_every);
    double *x = mx_, *r = mr_, *p = mp_, *Ap = mAp_, *r0 = mb_r0_, *s = mb_s_, *As = mb_as_;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (seconds) {
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, st_));
    }
    // init: r0 = b - A x, r = r0, p = r0, ||r0||
    launch_interleave(n, nrhs, W, X, ldx, x, st_);
    launch_interleave(n, nrhs, W, B, ldb, r0, st_);
    multi_residual(0, r0, x, r0);
    HIPCHK(hipMemcpyAsync(r, r0, bytes0, hipMemcpyDeviceToDevice, st_));
    HIPCHK(hipMemcpyAsync(p, r0, bytes0, hipMemcpyDeviceToDevice, st_));
    const int nb0 = launch_dot_multi(n, W, r0, r0, mpart0_, st_);
    launch_finalize_mbicg(MBFIN_INIT, W, nrhs, mpart0_, nb0, nullptr, 0, mb_, prm_.tol, nullptr, 0, 0, st_);

    int flags[3 * kMultiMax];
    auto read_flags = [&]() {
        HIPCHK(hipMemcpyAsync(pinned_, mb_.frozen, sizeof(flags), hipMemcpyDeviceToHost, st_));
        HIPCHK(hipStreamSynchronize(st_));
        std::memcpy(flags, pinned_, sizeof(flags));
    };
    auto all_frozen = [&]() {
        for (int c = 0; c < nrhs; ++c)
            if (!flags[c]) return false;
        return true;
    };
    auto spmv = [&](const double *in, double *out) {
        MultiArgs a;
        a.x = in;
        a.y = out;
        launch_csr_multi(lev_[0].A, W, OP_SPMV, a, st_, cfg_);
    };
    read_flags();
    int it = 0;
    while (!all_frozen() && it < max_iters && fault_ == SPARSH_OK) {
        vcycle_multi(p);  // p1 = M p, kept: the second cycle overwrites the cycle's own buffer, so the two blocks change places
        // (both blocks are lev_[0].n * mw_ doubles from multi_allocs_ -- multi_reserve's mlev_[0].x and mbicg_reserve's len0 -- and the
        // cycle writes all of mlev_[0].x before it reads it; a change to either allocation rule must keep the two lengths equal)
        std::swap(mlev_[0].x, mb_p1_);
        const double *p1 = mb_p1_;
        spmv(p1, Ap);
        int nb = launch_dot2_multi(n, W, r, r0, Ap, r0, mpart0_, mpart1_, st_);  // r.r0 ; Ap.r0
        launch_finalize_mbicg(MBFIN_ALPHA, W, nrhs, mpart0_, nb, mpart1_, nb, mb_, prm_.tol, nullptr, 0, 0, st_);
        launch_bicg_s_multi(n, W, mb_, r, Ap, s, st_);
        vcycle_multi(s);  // s1 = M s
        const double *s1 = mlev_[0].x;
        spmv(s1, As);
        nb = launch_dot2_multi(n, W, As, s, As, As, mpart0_, mpart1_, st_);  // As.s ; As.As
        launch_finalize_mbicg(MBFIN_OMEGA, W, nrhs, mpart0_, nb, mpart1_, nb, mb_, prm_.tol, nullptr, 0, 0, st_);
        nb = launch_bicg_xr_multi(n, W, mb_, p1, s1, s, As, r0, x, r, mpart0_, mpart1_, st_);  // r.r0 ; r.r
        launch_finalize_mbicg(MBFIN_BETA_RES, W, nrhs, mpart0_, nb, mpart1_, nb, mb_, prm_.tol, mhist_, hist_cap_dev_,
                              std::min(it, hist_cap_dev_ - 1), st_);
        launch_bicg_p_multi(n, W, mb_, r, Ap, p, st_);
        ++it;
        if (it % check_every == 0 || it >= max_iters) {
            read_flags();
            if (prm_.print_solve) std::printf("%d\t%d of %d columns running\n", it, (int)std::count(flags, flags + nrhs, 0), nrhs);
        }
    }
    launch_deinterleave(n, nrhs, W, x, X, ldx, st_);
    read_flags();
    if (seconds) {
        HIPCHK(hipEventRecord(e1, st_));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *seconds = ms * 1e-3;
        HIPCHK(hipEventDestroy(e0));
        HIPCHK(hipEventDestroy(e1));
    }
    note_hip(hipGetLastError(), "kernel launch during the block BiCGStab solve");
    if (fault_ != SPARSH_OK) return fault_;
    int rc = SPARSH_OK;
    bool numeric = false, noconv = false;
    mbicg_last_ = 0;
    for (int c = 0; c < nrhs; ++c) {
        int st = SPARSH_OK;
        if (!flags[c]) st = SPARSH_ENOCONV;  // the cap came first: x holds the iterate reached
        else if (flags[2 * kMultiMax + c] == kMultiStatusNumeric) st = SPARSH_ENUMERIC;
        numeric = numeric || st == SPARSH_ENUMERIC;
        noconv = noconv || st == SPARSH_ENOCONV;
        const int k = flags[kMultiMax + c];
        mbicg_last_ = std::max(mbicg_last_, k);
        if (status) status[c] = st;
        if (iters) iters[c] = k;
        const int m = std::min(std::min(k, hist_cap), hist_cap_dev_);
        if (hist && m > 0)
            HIPCHK(hipMemcpy(hist + (size_t)c * hist_cap, mhist_ + (size_t)c * hist_cap_dev_, (size_t)m * 8, hipMemcpyDeviceToHost));
    }
    if (numeric) {
        rc = SPARSH_ENUMERIC;
        error = "NaN residual in a column of the block";
    } else if (noconv) {
        rc = SPARSH_ENOCONV;
        error = "iteration cap reached before ||r|| <= tol in a column of the block";
    }
    return fault_ != SPARSH_OK ? fault_ : rc;
}

}  // namespace sparsh
