// engine_mbicg.cpp -- block BiCGStab on the block path: up to 8 right-hand sides of an unsymmetric system
// through two block V-cycles and two block SpMVs per iteration.
//
// Per column the loop is Engine::bicg(precond = true): the expressions of bicg_s / bicg_xr / bicg_p and of FIN_BICG_ALPHA / OMEGA /
// BETA.  It runs on the block vectors of engine_multi.cpp (x, r, p, Ap and the cycle's level blocks) and four blocks of its own (r0,
// s, As, p1); its kernels are in mbicg_kernels.hip.  Every scalar stays on the device, one set per column, and a column is frozen
// there when its residual reaches tol (block PCG's scheme, not block CG's coupling); the host reads 24 flags every
// params.check_every iterations.  The gate, the clock, the loop, the finish and the verdict are the block solvers' shared ones
// (engine_multi.cpp).
#include "engine.hpp"

#include <algorithm>
#include <cstdio>

namespace sparsh {

#define HIPCHK(call) note_hip((call), #call)

int Engine::mbicg_reserve()
{
    if (mb_.scal) return SPARSH_OK;  // reserved for the width in force (a change of width released everything)
    const size_t len0 = std::max<size_t>((size_t)lev_[0].n * mw_, 1);
    if (len0 != mlen0_) {  // the loop swaps p1 with the cycle's mlev_[0].x
        error = "block BiCGStab: its blocks and the cycle's level-0 block differ in length";
        return SPARSH_ENODEV;
    }
    bool ok = true;
    size_t bytes = 0;
    auto take = [&](size_t doubles) { return take_zeroed(multi_allocs_, bytes, ok, doubles); };
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
    if (int rc = block_begin(nrhs, max_iters); rc != SPARSH_OK) return rc;
    if (int rc = mbicg_reserve(); rc != SPARSH_OK) return rc;
    const int W = mw_, n = lev_[0].n;
    const size_t bytes0 = (size_t)n * W * 8;
    double *x = mx_, *r = mr_, *p = mp_, *Ap = mAp_, *r0 = mb_r0_, *s = mb_s_, *As = mb_as_;
    StreamClock clock(*this, seconds);
    // init: r0 = b - A x, r = r0, p = r0, ||r0||
    launch_interleave(n, nrhs, W, X, ldx, x, st_);
    launch_interleave(n, nrhs, W, B, ldb, r0, st_);
    multi_residual(0, r0, x, r0);
    HIPCHK(hipMemcpyAsync(r, r0, bytes0, hipMemcpyDeviceToDevice, st_));
    HIPCHK(hipMemcpyAsync(p, r0, bytes0, hipMemcpyDeviceToDevice, st_));
    const int nb0 = launch_dot_multi(n, W, r0, r0, mpart0_, st_);
    launch_finalize_mbicg(MBFIN_INIT, W, nrhs, mpart0_, nb0, nullptr, 0, mb_, prm_.tol, nullptr, 0, 0, st_);

    int flags[3 * kMultiMax];
    auto spmv = [&](const double *in, double *out) {
        MultiArgs a;
        a.x = in;
        a.y = out;
        launch_csr_multi(lev_[0].A, W, OP_SPMV, a, st_, cfg_);
    };
    block_loop(
        mb_.frozen, flags, 3 * kMultiMax, max_iters, [&] { return std::count(flags, flags + nrhs, 0) > 0; },
        [&](int it) {
            vcycle_multi(p);  // p1 = M p, kept: the second cycle overwrites the cycle's own buffer, so the two blocks change places
            // (equal lengths: mbicg_reserve has checked it; the cycle writes all of mlev_[0].x before it reads it)
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
        },
        [&](int it) { std::printf("%d\t%d of %d columns running\n", it, (int)std::count(flags, flags + nrhs, 0), nrhs); });
    if (int rc = block_finish(nrhs, x, X, ldx, mb_.frozen, flags, 3 * kMultiMax, clock, "kernel launch during the block BiCGStab solve");
        rc != SPARSH_OK)
        return rc;
    return block_verdict(nrhs, flags, hist, hist_cap, iters, status, &mbicg_last_);
}

}  // namespace sparsh
