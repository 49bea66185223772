#include "box_plan.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>

namespace sparsh {

const char *box_plan_refusal(int kernel, int nx, int ny, int nz, const BoxPlan &p)
{
    if (nx <= 0) return "the level is not a box grid";
    if (kernel != 1 && kernel != 2) return "kernel must be 2 (double sweep) or 1 (plane-marching kernel)";
    if (p.threads != 256 && p.threads != 512 && p.threads != 1024) return "threads per workgroup must be 256, 512 or 1024";
    if (p.q < 2 || p.q > 4) return "points per thread must be 2, 3 or 4";
    if (p.ty < 1 || p.ty > ny) return "lines per tile must lie in 1 .. ny";
    if (p.cz < 1 || p.cz > nz) return "planes per chunk must lie in 1 .. nz";
    // region = TY + halo lines, one point per thread and q
    if ((long)(p.ty + box_halo(kernel)) * nx > (long)p.q * p.threads) return "the tile's region has more points than the workgroup's threads hold";
    if (box_lds_bytes(kernel, nx, p.ty) > 65536) return "the tile's region does not fit the 64 KiB of LDS";
    return nullptr;
}

// Cost model (checked against tools/micro/box2_proto on MI355X: 216^3 Q4/TY14/CZ14 57 us, Q3/TY10/CZ14 94 us, 108x216x216 Q4/TY33/CZ6
// 34 us, Q2/TY14/CZ14 38 us): a workgroup's time ~ (CZ + extra steps) x Q points, the launch takes ceil(workgroups / 256 CUs) rounds of
// it.  The double sweep's Q = 2 instance needs 62 VGPRs and 31 KB of LDS, so two of its workgroups share a CU: 512 slots, each running
// at ~1/1.6 of the speed it has alone (108 x 216 x 216: Q2/TY14/CZ7 = 496 workgroups 32.9 us against 35.8 for CZ14 = 256 and 35.4 for
// Q3/TY24/CZ8 = 243).  The marching kernel's instances of <= 3 points per thread (<= 64 VGPRs, <= 32 KB of LDS) share a CU the same
// way; its planner counts that only when asked (shared_cu).
BoxPlan box_planner(int kernel, int nx, int ny, int nz, bool shared_cu)
{
    BoxPlan plan;
    if (nx < 2 || ny < 1 || nz < 1) return plan;
    const int shared_q = kernel == 2 ? 2 : (shared_cu ? 3 : 0);  // up to this Q two workgroups count as sharing a CU
    long best = -1;
    for (int Q = 2; Q <= 4; ++Q) {
        int TY = std::min(ny, Q * kBoxBlock / nx - box_halo(kernel));
        while (TY >= 1 && box_lds_bytes(kernel, nx, TY) > 65536) --TY;
        if (TY < 1) continue;
        const int ytiles = (ny + TY - 1) / TY;
        for (int zch = 1; zch <= nz; ++zch) {
            const int CZ = (nz + zch - 1) / zch;
            const int chunks = (nz + CZ - 1) / CZ;
            const long wgs = (long)ytiles * chunks;
            const long steps = CZ + box_extra_steps(kernel);
            long cost;  // in tenths of a step of one point
            if (Q <= shared_q && wgs > 256) cost = ((wgs + 511) / 512) * steps * Q * 16;
            else cost = ((wgs + 255) / 256) * steps * Q * 10;
            if (best < 0 || cost < best) {
                best = cost;
                plan = {kBoxBlock, Q, TY, CZ};
            }
        }
    }
    return plan;
}

// Pruning model of box_plan_candidates (it only decides which plans are worth timing; the timing decides): r workgroups share a CU --
// bounded by 2048 threads, by the registers (waves per SIMD at Q = 2 / 3 / 4: 8 / 5 / 4 for the double sweep, 8 / 7 / 5 for the marching
// kernel) and by 160 KiB of LDS --
// and a step of theirs costs a fixed part (load round trip and two barriers, overlapped among them: ~1500 point updates, from the
// 2.0 / 3.5 us steps of 2048 / 4096 points per CU in profiles/r03_levels_216_box_kernels.txt) plus one unit per point.
static long box_candidate_cost(int kernel, int nx, int ny, int nz, const BoxPlan &p)
{
    const long lds = (long)box_lds_bytes(kernel, nx, p.ty);
    const int waves_simd = p.q == 2 ? 8 : (kernel == 2 ? (p.q == 3 ? 5 : 4) : (p.q == 3 ? 7 : 5));
    long r = std::min<long>(2048 / p.threads, (long)waves_simd * 256 / p.threads);
    r = std::max<long>(1, std::min<long>(r, 163840 / lds));
    const long wgs = (long)((ny + p.ty - 1) / p.ty) * ((nz + p.cz - 1) / p.cz);
    const long rounds = (wgs + 256 * r - 1) / (256 * r);
    const long resident = std::min<long>(r, (wgs + 255) / 256);
    return rounds * (p.cz + box_extra_steps(kernel)) * (1536 + resident * p.q * p.threads);
}

std::vector<BoxPlan> box_plan_candidates(int kernel, int nx, int ny, int nz, int part_cap)
{
    std::vector<BoxPlan> out;
    if ((kernel != 1 && kernel != 2) || nx < 2 || ny < 1 || nz < 1) return out;
    auto add = [&](const BoxPlan &p) {
        if (box_plan_refusal(kernel, nx, ny, nz, p)) return;
        if (kernel == 1 && part_cap > 0 && (long)((ny + p.ty - 1) / p.ty) * ((nz + p.cz - 1) / p.cz) > part_cap) return;
        if (std::find(out.begin(), out.end(), p) == out.end()) out.push_back(p);
    };
    add(box_planner(kernel, nx, ny, nz));  // (no plan: refused)
    if (kernel == 1) add(box_planner(1, nx, ny, nz, true));  // the shared-CU plan, where it is another one
    const size_t first = out.size();
    for (int threads : {1024, 512, 256}) {
        for (int Q = 2; Q <= 4; ++Q) {
            int top = std::min(ny, Q * threads / nx - box_halo(kernel));
            while (top >= 1 && box_lds_bytes(kernel, nx, top) > 65536) --top;
            if (top < 1) continue;
            for (int TY : {top, std::max(1, top / 2)}) {
                const int ytiles = (ny + TY - 1) / TY;
                for (int target : {256, 512, 1024}) {
                    const int chunks = std::max(1, std::min(nz, (target + ytiles / 2) / ytiles));
                    add({threads, Q, TY, (nz + chunks - 1) / chunks});
                }
                add({threads, Q, TY, nz});
            }
        }
    }
    if ((int)out.size() > kBoxCandidates) {
        // keep the planner's plans, the lowest modelled cost of every thread count, then the lowest costs overall (first one on
        // ties); the list keeps its order
        const size_t n = out.size();
        std::vector<long> cost(n, 0);
        std::vector<char> keep(n, 0);
        for (size_t i = 0; i < n; ++i) cost[i] = i < first ? 0 : box_candidate_cost(kernel, nx, ny, nz, out[i]);
        std::vector<size_t> order;
        for (size_t i = first; i < n; ++i) order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return cost[x] < cost[y]; });
        size_t nkeep = first;
        for (size_t i = 0; i < first; ++i) keep[i] = 1;
        for (int threads : {1024, 512, 256})
            for (size_t i : order)
                if (out[i].threads == threads) {
                    keep[i] = 1;
                    ++nkeep;
                    break;
                }
        for (size_t i : order) {
            if ((int)nkeep >= kBoxCandidates) break;
            if (!keep[i]) {
                keep[i] = 1;
                ++nkeep;
            }
        }
        std::vector<BoxPlan> kept;
        for (size_t i = 0; i < n; ++i)
            if (keep[i]) kept.push_back(out[i]);
        out.swap(kept);
    }
    return out;
}

bool box_exact_offdiag(const double *c)
{
    for (int u = 0; u < 7; ++u) {
        if (u == 3) continue;
        std::uint64_t bits;
        std::memcpy(&bits, &c[u], sizeof bits);
        const std::uint64_t mag = bits & 0x7fffffffffffffffull;
        if (mag == 0) continue;  // +-0.0
        const unsigned exponent = (unsigned)(mag >> 52);
        if ((mag & 0x000fffffffffffffull) != 0 || exponent < 1023 || exponent == 2047) return false;
    }
    return true;
}

}  // namespace sparsh
