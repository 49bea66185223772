// engine_bcg.cpp -- block conjugate gradients on the block path: the columns of a block of right-hand sides
// minimise over the union of their search directions (O'Leary's block CG), with a small dense solve that drops dependent directions.
//
// The loop runs on the block vectors of engine_multi.cpp (x, r, p, Ap and the cycle's level blocks) with the block V-cycle, the block
// SpMV and the eigensolver's Gram launch; its own kernels are in bcg_kernels.hip.  All coefficients stay on the device; the host reads
// 16 flags every params.check_every iterations.  The gate, the clock, the loop and the finish are the block solvers' shared ones
// (engine_multi.cpp); the verdict is its own: one status for all columns.
#include "engine.hpp"

#include <algorithm>
#include <cstdio>

namespace sparsh {

#define HIPCHK(call) note_hip((call), #call)

int Engine::bcg_reserve()
{
    if (bcg_.L) return SPARSH_OK;  // reserved for the width in force (a change of width released everything)
    const int W = mw_;
    bool ok = true;
    size_t bytes = 0;
    auto take = [&](size_t doubles) { return take_zeroed(multi_allocs_, bytes, ok, doubles); };
    double *gm = take(3 * (size_t)W * W);
    double *coef = take(2 * (size_t)W * W);
    double *part = take(2 * (size_t)W * W * kEigMaxGrid);
    double *L = take((size_t)kMultiMax * kMultiMax);
    double *d = take(kMultiMax);
    double *res = take(kMultiMax);
    int *flags = reinterpret_cast<int *>(take(BF_COUNT / 2));
    if (!ok) {
        multi_release();
        return SPARSH_ENODEV;
    }
    bcg_gm_ = gm;
    bcg_coef_ = coef;
    bcg_part_ = part;
    bcg_.L = L;
    bcg_.d = d;
    bcg_.res = res;
    bcg_.flags = flags;
    bcg_bytes_ = bytes;
    return SPARSH_OK;
}

int Engine::solve_bcg_dev(int nrhs, const double *B, long ldb, double *X, long ldx, int max_iters, double *hist, int hist_cap, int *iters,
                          int *status, double *seconds)
{
    if (int rc = block_begin(nrhs, max_iters); rc != SPARSH_OK) return rc;
    if (int rc = bcg_reserve(); rc != SPARSH_OK) return rc;
    const int W = mw_, n = lev_[0].n, k = nrhs;
    const int *done = bcg_.flags + BF_DONE;
    double *G = bcg_gm_, *C1 = bcg_gm_ + W * W, *C2 = bcg_gm_ + 2 * W * W;
    double *alpha = bcg_coef_, *beta = bcg_coef_ + W * W;
    StreamClock clock(*this, seconds);
    // init: R = B - A X, ||R_c||, Z = M R, P = Z
    launch_interleave(n, nrhs, W, X, ldx, mx_, st_);
    launch_interleave(n, nrhs, W, B, ldb, mr_, st_);
    multi_residual(0, mr_, mx_, mr_);
    const int nb = launch_dot_multi(n, W, mr_, mr_, mpart0_, st_);
    launch_bcg_finalize(W, nrhs, mpart0_, nb, bcg_, prm_.tol, nullptr, 0, -1, st_);
    vcycle_multi(mr_);
    HIPCHK(hipMemcpyAsync(mp_, mlev_[0].x, (size_t)n * W * 8, hipMemcpyDeviceToDevice, st_));

    int flags[BF_COUNT];
    GramPairs two{}, one{};
    two.u[0] = mp_, two.v[0] = mAp_, two.dst[0] = 0;      // G  = P^T Q
    two.u[1] = mp_, two.v[1] = mr_, two.dst[1] = W * W;   // C1 = P^T R
    one.u[0] = mAp_, one.dst[0] = 2 * W * W;              // C2 = Q^T Z (Z is wherever the cycle's ping-pong left it)
    block_loop(
        bcg_.flags, flags, BF_COUNT, max_iters, [&] { return !flags[BF_DONE]; },
        [&](int it) {
            MultiArgs a;
            a.x = mp_;
            a.y = mAp_;
            launch_csr_multi(lev_[0].A, W, OP_SPMV, a, st_, cfg_);  // Q = A P
            launch_gram_multi(n, W, 2, two, bcg_part_, bcg_gm_, W, st_);
            launch_bcg_small(W, k, true, G, C1, 1.0, bcg_, alpha, it, st_);  // alpha = pinv(G) C1
            const int nrr = launch_bcg_update(n, W, k, done, mx_, mr_, mp_, mAp_, alpha, mx_, mr_, mpart1_, st_);
            launch_bcg_finalize(W, nrhs, mpart1_, nrr, bcg_, prm_.tol, mhist_, hist_cap_dev_, it, st_);
            vcycle_multi(mr_);  // Z = M R
            one.v[0] = mlev_[0].x;
            launch_gram_multi(n, W, 1, one, bcg_part_, bcg_gm_, W, st_);
            launch_bcg_small(W, k, false, G, C2, -1.0, bcg_, beta, it, st_);  // beta = -pinv(G) C2, the factor kept
            launch_bcg_dir(n, W, k, done, mlev_[0].x, mp_, beta, mp_, st_);   // P = Z + P beta
        },
        [&](int it) { std::printf("%d\trank %d of %d\n", it, flags[BF_RANK], nrhs); });
    if (int rc = block_finish(nrhs, mx_, X, ldx, bcg_.flags, flags, BF_COUNT, clock, "kernel launch during the block CG solve"); rc != SPARSH_OK)
        return rc;
    const int ran = flags[BF_ITERS];
    bcg_last_[0] = ran;
    bcg_last_[1] = flags[BF_MIN_RANK];
    bcg_last_[2] = flags[BF_DROPPED];
    int rc = SPARSH_OK;
    if (flags[BF_NUMERIC]) {
        rc = SPARSH_ENUMERIC;
        error = "NaN residual or a Gram matrix of rank 0 in block CG";
    } else if (!flags[BF_DONE]) {
        rc = SPARSH_ENOCONV;  // the cap came first: X holds the iterate reached
        error = "iteration cap reached before ||r|| <= tol in every column of the block";
    }
    for (int c = 0; c < nrhs; ++c) {
        if (status) status[c] = rc;
        if (iters) iters[c] = ran;
        copy_hist_multi(c, ran, hist, hist_cap);
    }
    return fault_ != SPARSH_OK ? fault_ : rc;
}

}  // namespace sparsh
