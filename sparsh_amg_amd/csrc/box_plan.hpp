// Launch plans of the box-grid kernels: everything about a plan that is not a launch.  Pure host code, no HIP and no DevCsr: plain
// g++ compiles it (tests/cpp/box_plan_check.cpp runs it under the sanitizers).
//
// A plan is (threads per workgroup, Q points per thread, TY lines per tile, CZ planes per chunk).  The kernel is named as in the C ABI:
// 2 = double sweep (sdia_box2_kernel), 1 = plane-marching kernel (sdia_box1_kernel).
#pragma once

#include <cstddef>
#include <vector>

namespace sparsh {

struct BoxPlan {
    int threads = 1024;  // 256, 512 or 1024 (the planner plans for kBoxBlock)
    int q = 0, ty = 0, cz = 0;  // q == 0: no plan
    bool operator==(const BoxPlan &o) const { return threads == o.threads && q == o.q && ty == o.ty && cz == o.cz; }
    bool operator!=(const BoxPlan &o) const { return !(*this == o); }
    // workgroups of a launch on lines x planes = ny x nz (the marching kernel's reducing epilogues write one partial sum each); 0: no plan
    int workgroups(int ny, int nz) const { return q <= 0 || ty <= 0 || cz <= 0 ? 0 : ((ny + ty - 1) / ty) * ((nz + cz - 1) / cz); }
};

constexpr int kBoxBlock = 1024;  // the workgroup the planner plans for
constexpr int kBoxCandidates = 12;

// What tells the two kernels apart for a plan: the double sweep's region is TY + 4 lines in two LDS planes and a chunk takes CZ + 2
// steps (the second stage trails the first); the marching kernel's is TY + 2 lines in one plane, CZ + 1 steps.
constexpr int box_halo(int kernel) { return kernel == 2 ? 4 : 2; }
constexpr int box_lds_planes(int kernel) { return kernel == 2 ? 2 : 1; }
constexpr int box_extra_steps(int kernel) { return kernel == 2 ? 2 : 1; }
inline size_t box_lds_bytes(int kernel, int nx, int ty)
{
    return (size_t)box_lds_planes(kernel) * ((size_t)(ty + box_halo(kernel)) * (nx + 1) + 1) * sizeof(double);
}

// why the kernel cannot run the plan on an nx x ny x nz box grid: a message, or nullptr where it can (256, 512 or 1024 threads, one
// point per thread and q of the tile's region, 64 KiB of LDS)
const char *box_plan_refusal(int kernel, int nx, int ny, int nz, const BoxPlan &p);
// The plan with the lowest modelled cost on kBoxBlock threads, the first one on ties (q == 0: none -- lines too long for the LDS
// region).  shared_cu (marching kernel): count 512 slots for the instances of <= 3 points per thread -- the alternative plan the setup
// times against the one-workgroup-per-CU plan (Engine::tune_box_kernels); the double sweep always counts them for Q = 2.
BoxPlan box_planner(int kernel, int nx, int ny, int nz, bool shared_cu = false);
// The plans the setup times on an nx x ny x nz box (Engine::tune_box_kernels), in a fixed order: the planner's own first, then per
// thread count and Q the largest TY and half of it, each with the CZ that bring the workgroup count near 1x, 2x and 4x the 256 CUs and
// with CZ = nz; duplicates and plans box_plan_refusal rejects dropped, at most kBoxCandidates kept (the planner's own, the lowest
// modelled cost of each thread count, then the lowest costs overall).  Marching kernel: its shared-CU plan comes second, and no plan
// launches more than part_cap workgroups (part_cap <= 0: no bound).
std::vector<BoxPlan> box_plan_candidates(int kernel, int nx, int ny, int nz, int part_cap);

// Whether the six off-diagonal constants c[0..2], c[4..6] of a box-grid stencil (BoxArgs::c; the diagonal c[3] is not looked at) let the
// kernels fuse sum + c x into one FMA without changing a bit: each is 0.0 or finite with |c| = 2^k, k >= 0 (mantissa field zero, biased
// exponent from 1023 up).  Then c x is exact unless it overflows -- scaling by a power of two >= 1 rounds nothing, denormals included --
// and fma(c, x, sum) rounds the same exact value once that sum + c x does.  Magnitudes below 1 do not qualify: c x can then underflow
// inexactly.  A property of the operator alone.
bool box_exact_offdiag(const double *c);

}  // namespace sparsh
