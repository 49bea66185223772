// capi.cpp -- extern "C" surface declared in include/sparsh_amg.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/sparsh_amg.h"
#include "bcg_small.hpp"
#include "eig_chol.hpp"
#include "eig_small.hpp"
#include "engine.hpp"

using namespace sparsh;

struct sparsh_handle_s {
    std::unique_ptr<Engine> eng;
    LocalOp cached_op;  // last sparsh_dist_local_op result
    DeepLocal cached_deep;  // last sparsh_dist_deep_op result
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

// end of an operator-level entry point: a fault raised inside the call wins over the copy-back status
int done(const Engine &E, bool copied_back)
{
    if (E.fault() != SPARSH_OK) return fail(E.fault(), E.error);
    return copied_back ? SPARSH_OK : fail(SPARSH_ENODEV, "D2H failed");
}

int env_int(const char *name, int dflt)
{
    const char *v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : dflt;
}

double env_dbl(const char *name, double dflt)
{
    const char *v = std::getenv(name);
    return (v && *v) ? std::atof(v) : dflt;
}

// RAII device buffer for the host-vector operator wrappers
struct DBuf {
    Engine &E;
    double *p = nullptr;
    size_t n;
    DBuf(Engine &e, size_t count, const double *src = nullptr) : E(e), n(count)
    {
        p = static_cast<double *>(E.dalloc(count * sizeof(double)));
        if (p && src) (void)hipMemcpy(p, src, count * sizeof(double), hipMemcpyHostToDevice);
    }
    DBuf(Engine &e, GmresState &s) : E(e), p(e.gmres_state_alloc(s)), n((size_t)kGmresStateDoubles) {}  // the block behind a GmresState
    ~DBuf() { E.dfree(p); }
    bool get(double *dst)
    {
        (void)hipStreamSynchronize(E.stream());
        return hipMemcpy(dst, p, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    }
};

#define REQUIRE_READY(h)                                                         \
    if (!(h) || !(h)->eng) return fail(SPARSH_EINVAL, "null handle");            \
    if (!(h)->eng->ready()) return fail(SPARSH_ESTATE, "sparsh_setup has not been called (or failed)"); \
    if ((h)->eng->fault() != SPARSH_OK) return fail((h)->eng->fault(), (h)->eng->error) /* sticky device / transport fault */

#define REQUIRE_LEVEL(h, l) \
    if ((l) < 0 || (l) >= (int)(h)->eng->host().levels.size()) return fail(SPARSH_EINVAL, "level out of range")

#define REQUIRE_SINGLE(h) \
    if ((h)->eng->distributed()) return fail(SPARSH_ESTATE, "operator-level entry points are single-GPU test hooks (host vectors carry no halo)")

// checked before REQUIRE_READY: a combination that no setup can make valid is a bad argument, with or without a device
// (SPARSH_PCG alone: SPARSH_FCG is refused by the solve itself, with its other refusals)
#define REQUIRE_SMOOTHER_FITS(h, method) \
    if (const char *why_ = (h) && (h)->eng && (method) == SPARSH_PCG ? (h)->eng->sor_refusal(method) : nullptr) return fail(SPARSH_EINVAL, why_)

// likewise: GMRES on a handle that a multi-GPU transport has been installed on
#define REQUIRE_GMRES_FITS(h, method)                                                                                              \
    if ((h) && (h)->eng && ((method) == SPARSH_GMRES || (method) == SPARSH_PGMRES) &&                                              \
        ((h)->eng->distributed() || ((h)->eng->comm() && (h)->eng->comm()->size > 1)))                                             \
    return fail(SPARSH_EINVAL, "GMRES is not available on a partitioned (multi-GPU) handle: its j + 2 sums per step need a wider all-reduce")

// likewise: a method the handle's cycle cannot serve (the K-cycle under a Krylov method that needs a fixed operator, W or K on a
// partitioned handle or with the fp32 preconditioner, more level visits than the cap)
#define REQUIRE_CYCLE_FITS(h, method) \
    if ((h) && (h)->eng && (h)->eng->cycle_check(method) != SPARSH_OK) return fail(SPARSH_EINVAL, (h)->eng->error)

// SPARSH_MBICG is a method of the block entry points alone: a bad argument with or without a device
#define REQUIRE_NOT_BLOCK_ONLY(method) \
    if ((method) == SPARSH_MBICG) return fail(SPARSH_EINVAL, "SPARSH_MBICG is a method of sparsh_solve_multi / sparsh_solve_multi_dev only")

#define REQUIRE_HOST(h)                                               \
    if (!(h) || !(h)->eng) return fail(SPARSH_EINVAL, "null handle"); \
    if (!(h)->eng->host_ready()) return fail(SPARSH_ESTATE, "sparsh_setup / sparsh_setup_host has not been called (or failed)")

}  // namespace

extern "C" {

const char *sparsh_last_error(void) { return g_err.c_str(); }

int sparsh_version(void) { return 100; }

int sparsh_host_cpus(void) { return effective_cpus(); }

int sparsh_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void sparsh_default_params(sparsh_params *p)
{
    if (!p) return;
    // reference macros, include/AMG.hpp:15-27
    p->omega = env_dbl("SPARSH_OMEGA", 0.66667);
    p->tol = env_dbl("SPARSH_TOL", 1e-8);
    p->sweeps = env_int("SPARSH_NU", 6 + 1);  // smooth_iter + 1: the CPU path's count (src/AMG_smoothers.cpp:59-60)
    p->max_levels = env_int("SPARSH_LEVELS", 6);
    p->limit_upper = 4000;
    p->limit_lower = 2000;
    p->coarsening = 0;
    if (const char *c = std::getenv("SPARSH_COARSENING")) p->coarsening = (std::strcmp(c, "beck") == 0) ? 1 : 0;
    p->max_iter = env_int("SPARSH_MAXIT", 100000);
    p->coarse_limit = env_int("SPARSH_COARSE_LIMIT", 40000);
    p->dense_limit = env_int("SPARSH_DENSE_LIMIT", 8192);
    p->extend_until = env_int("SPARSH_EXTEND_UNTIL", 0);
    p->coarse_factor_mb = env_int("SPARSH_COARSE_FACTOR_MB", 1024);
    p->host_threads = env_int("SPARSH_THREADS", 0);
    p->device = -1;
    if (const char *lr = std::getenv("LOCAL_RANK")) p->device = std::atoi(lr);
    const int pr = env_int("SPARSH_PRINT", 1);
    p->print_setup = pr;
    p->print_solve = pr;
    p->check_every = 1;
    p->use_graph = env_int("SPARSH_GRAPH", 0);
    p->replicate_rows = env_int("SPARSH_REPLICATE_ROWS", 0);
    p->precond_fp32 = env_int("SPARSH_PRECOND_FP32", 0);
}

int sparsh_create_csr(int nrow, int ncol, const int *rowptr, const int *colindex, const double *val, sparsh_handle *out)
{
    if (!out || !rowptr || nrow <= 0 || ncol <= 0) return fail(SPARSH_EINVAL, "bad CSR arguments");
    if (rowptr[0] != 0 || rowptr[nrow] < 0) return fail(SPARSH_EINVAL, "rowptr must start at 0");
    if (rowptr[nrow] > 0 && (!colindex || !val)) return fail(SPARSH_EINVAL, "null colindex/val");
    // one O(nnz) pass: a non-monotone rowptr or an out-of-range column would become an out-of-bounds
    // access on the device
    {
        long bad_rp = 0, bad_col = 0;
#pragma omp parallel for schedule(static) reduction(+ : bad_rp, bad_col)
        for (int i = 0; i < nrow; ++i) {
            const int j0 = rowptr[i], j1 = rowptr[i + 1];
            if (j1 < j0 || j0 < 0 || j1 > rowptr[nrow]) {
                ++bad_rp;
                continue;
            }
            for (int j = j0; j < j1; ++j) bad_col += (colindex[j] < 0 || colindex[j] >= ncol);
        }
        if (bad_rp) return fail(SPARSH_EINVAL, "rowptr is not monotonically non-decreasing (" + std::to_string(bad_rp) + " rows)");
        if (bad_col) return fail(SPARSH_EINVAL, "colindex out of range [0, ncol) (" + std::to_string(bad_col) + " entries)");
    }
    auto *h = new sparsh_handle_s;
    h->eng.reset(new Engine(nrow, ncol, rowptr, colindex, val));
    *out = h;
    return SPARSH_OK;
}

void sparsh_destroy(sparsh_handle h) { delete h; }

int sparsh_setup(sparsh_handle h, const sparsh_params *p)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    sparsh_params prm;
    if (p)
        prm = *p;
    else
        sparsh_default_params(&prm);
    if (prm.sweeps < 1 || prm.max_levels < 1 || prm.limit_upper < 1) return fail(SPARSH_EINVAL, "bad params");
    int rc = h->eng->setup(prm);
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

int sparsh_setup_host(sparsh_handle h, const sparsh_params *p)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    sparsh_params prm;
    if (p)
        prm = *p;
    else
        sparsh_default_params(&prm);
    if (prm.sweeps < 1 || prm.max_levels < 1 || prm.limit_upper < 1) return fail(SPARSH_EINVAL, "bad params");
    int rc = h->eng->setup_host(prm);
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

int sparsh_set_stopping(sparsh_handle h, double tol, int max_iter, int check_every)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->set_stopping(tol, max_iter, check_every);
    return SPARSH_OK;
}

int sparsh_set_kernel_config(sparsh_handle h, int kind, int vec, int nt, int remap)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (kind < 0 || kind > 3) return fail(SPARSH_EINVAL, "kind must be 0 (workgroup CSR-stream), 1 (wave CSR-stream), 2 (sliced ELL) or 3 (sliced diagonals)");
    KernelConfig &c = h->eng->kernel_cfg();
    c.kind = kind;
    c.vec = vec < 0 ? 0 : (vec > 4 ? 3 : vec);
    c.nt = nt > 0;
    c.remap = remap < 0 ? 0 : remap;
    c.auto_policy = (nt < 0 || remap < 0);
    h->eng->config_changed();
    return SPARSH_OK;
}

// which kernel family the SpMV-type operators of a level run with under the current config:
// 3 sliced diagonals, 2 sliced ELL, 1 wave CSR-stream, 0 workgroup CSR-stream; bytes_per_entry =
// what that layout streams per stored entry (values + indices), slots/entries incl. padding.
int sparsh_level_format(sparsh_handle h, int level, int *kind, long *stored_entries)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevCsr &A = h->eng->level(level).A;
    const CsrFamily fam = csr_family(A, h->eng->kernel_cfg());  // the launcher's own decision
    int k = 0;
    long e = A.nnz;
    if (fam == FAM_SDIA || fam == FAM_SDIA_TAB) {
        k = 3;
        e = A.sd_vblocks * 64;  // values actually stored: constant slots own no block
    } else if (fam == FAM_SELL) {
        k = 2;
        e = A.sell_entries;
    } else if (fam == FAM_CSR_WAVE) {
        k = 1;
    }
    if (kind) *kind = k;
    if (stored_entries) *stored_entries = e;
    return SPARSH_OK;
}

int sparsh_level_layout(sparsh_handle h, int level, long *slots, long *value_blocks, long *meta_bytes)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevCsr &A = h->eng->level(level).A;
    if (slots) *slots = A.has_sdia() ? A.sd_slots : 0;
    if (value_blocks) *value_blocks = A.has_sdia() ? A.sd_vblocks : 0;
    if (meta_bytes) {
        // what one sweep reads besides values and vectors: per-slice records (192 B) where they exist
        // (slices off the record path additionally read their 24 B/slot headers: counted for all slots
        // only when there are no records), else sd_ptr + 24 B per slot
        if (!A.has_sdia())
            *meta_bytes = 0;
        else if (A.sd_tmask)  // table path: 8 lane masks + the conformity word per slice
            *meta_bytes = (long)A.nslice * 68 + A.sd_vblocks * 24;
        else if (A.sd_rec)
            *meta_bytes = (long)A.nslice * kSdRecInts * 4 + A.sd_vblocks * 24;
        else
            *meta_bytes = (long)A.nslice * 4 + A.sd_slots * 24;
    }
    return SPARSH_OK;
}

const char *sparsh_level_kernel(sparsh_handle h, int level)
{
    if (!h || !h->eng || !h->eng->ready() || level < 0 || level >= (int)h->eng->host().levels.size()) return "";
    return csr_family_name(csr_family(h->eng->level(level).A, h->eng->kernel_cfg()));
}

int sparsh_level_placement(sparsh_handle h, int level, int *nt, int *remap)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    bool b = false;
    int r = 0;
    csr_placement(h->eng->level(level).A, h->eng->kernel_cfg(), &b, &r);
    if (nt) *nt = b ? 1 : 0;
    if (remap) *remap = r;
    return SPARSH_OK;
}

int sparsh_bench_comm(sparsh_handle h, int what, int level, int reps, double *avg_seconds)
{
    REQUIRE_READY(h);
    if (!avg_seconds) return fail(SPARSH_EINVAL, "null output");
    *avg_seconds = h->eng->bench_comm(what, level, reps);
    return SPARSH_OK;
}

int sparsh_set_tile(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->kernel_cfg().tile = enable != 0;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_level_tile_rows(sparsh_handle h, int level, int *rows)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    if (rows) *rows = csr_family(h->eng->level(level).A, h->eng->kernel_cfg()) == FAM_SDIA_TAB ? sdia_tile_rows(h->eng->level(level).A, h->eng->kernel_cfg()) : 0;
    return SPARSH_OK;
}

int sparsh_set_const_slots(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->kernel_cfg().const_slots = enable != 0;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_set_setup_broadcast(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->set_share_setup(enable != 0);
    return SPARSH_OK;
}

int sparsh_setup_share_info(sparsh_handle h, int *built_locally, long *image_bytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (built_locally) *built_locally = h->eng->built_locally() ? 1 : 0;
    if (image_bytes) *image_bytes = (long)h->eng->shared_image_bytes();
    return SPARSH_OK;
}

// test hook (host only): byte image of the hierarchy -> fresh hierarchy -> compare every array; returns the image size
long sparsh_debug_hierarchy_roundtrip(sparsh_handle h, long truncate_to)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (!h->eng->host_ready()) return fail(SPARSH_ESTATE, "sparsh_setup_host has not been called");
    const HostHierarchy &H = h->eng->host();
    std::vector<char> img;
    serialize_hierarchy(H, img);
    HostHierarchy G;
    const size_t use = truncate_to >= 0 ? std::min<size_t>((size_t)truncate_to, img.size()) : img.size();
    if (!deserialize_hierarchy(img.data(), use, H.levels[0].A, G)) return fail(SPARSH_EINVAL, G.error);
    const auto same_csr = [](const HostCsr &a, const HostCsr &b) {
        if (a.nrow != b.nrow || a.ncol != b.ncol || a.nnz() != b.nnz()) return false;
        if (!a.rowptr) return !b.rowptr;
        const size_t nnz = (size_t)a.nnz();
        return std::memcmp(a.rowptr, b.rowptr, ((size_t)a.nrow + 1) * sizeof(int)) == 0 && std::memcmp(a.col, b.col, nnz * sizeof(int)) == 0 &&
               std::memcmp(a.val, b.val, nnz * sizeof(double)) == 0;
    };
    bool same = G.levels.size() == H.levels.size() && G.nL == H.nL && G.coarse_dense == H.coarse_dense && G.extended == H.extended &&
                G.nullspace == H.nullspace && G.pinned_row == H.pinned_row && G.coarse_inverse == H.coarse_inverse;
    for (size_t l = 0; same && l < H.levels.size(); ++l)
        same = same_csr(G.levels[l].A, H.levels[l].A) && same_csr(G.levels[l].P, H.levels[l].P) && same_csr(G.levels[l].R, H.levels[l].R) &&
               G.levels[l].diag == H.levels[l].diag && G.levels[l].P_is_aggregation == H.levels[l].P_is_aggregation;
    if (!same) return fail(SPARSH_ENUMERIC, "hierarchy image round trip changed the hierarchy");
    return (long)img.size();
}

// test hook (host only): row-block schedule -> 16-bit delta form -> decoded columns, compared with the input
int sparsh_debug_index16_roundtrip(int nrow, const int *rowptr, const int *col, long *blocks16, long *blocks)
{
    if (nrow < 0 || !rowptr || (!col && rowptr[nrow] > 0)) return fail(SPARSH_EINVAL, "bad arguments");
    int nblk = 0;
    const std::vector<int> rec = rowblock_records(nrow, rowptr, &nblk);
    std::vector<unsigned short> c16((size_t)rowptr[nrow] + kCsrPad, 0);
    std::vector<int> cb((size_t)std::max(nblk, 1), -1);
    const int n16 = build_col16(rowptr, col, rec.data(), nblk, c16.data(), cb.data());
    int counted = 0;
    for (int k = 0; k < nblk; ++k) {
        if (cb[k] < 0) continue;
        ++counted;
        for (int r = rec[(size_t)4 * k]; r < rec[(size_t)4 * k + 1]; ++r) {
            int c = cb[k];
            for (int j = rowptr[r]; j < rowptr[r + 1]; ++j) {
                c += c16[j];
                if (c != col[j]) return fail(SPARSH_ENUMERIC, "16-bit delta form decodes to a different column");
            }
        }
    }
    if (counted != n16) return fail(SPARSH_ENUMERIC, "block count mismatch");
    if (blocks16) *blocks16 = n16;
    if (blocks) *blocks = nblk;
    return SPARSH_OK;
}

int sparsh_set_placement_search(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->kernel_cfg().place_search = enable != 0;
    return SPARSH_OK;
}

int sparsh_placement_info(sparsh_handle h, double *chosen_us, double *worst_us, double *initial_us, int *triples, double *seconds)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (chosen_us) *chosen_us = h->eng->place_best_us;
    if (worst_us) *worst_us = h->eng->place_worst_us;
    if (initial_us) *initial_us = h->eng->place_first_us;
    if (triples) *triples = h->eng->place_tried;
    if (seconds) *seconds = h->eng->place_seconds;
    return SPARSH_OK;
}

int sparsh_set_fused_zero_sweep(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->kernel_cfg().fuse_cg_zero = enable != 0;
    h->eng->kernel_cfg().cg_nt = enable == 2;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_set_alternate_sweeps(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (enable < 0 || enable > 2) return fail(SPARSH_EINVAL, "mode must be 0 (never), 1 (where a sweep streams more than the Infinity Cache holds) or 2 (always)");
    h->eng->kernel_cfg().alt_dir = enable;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_set_double_sweep(sparsh_handle h, int mode)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (mode < 0 || mode > 2) return fail(SPARSH_EINVAL, "mode must be 0 (never), 1 (where the setup measures it faster) or 2 (wherever the level is a box grid with a plan)");
    h->eng->kernel_cfg().box2 = mode;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_level_double_sweep(sparsh_handle h, int level, int *on, int *dims, int *plan, double *single_us, double *double_us)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevLevel &L = h->eng->level(level);
    if (on) *on = (!h->eng->distributed() || L.replicated) && box2_applies(L.A, h->eng->kernel_cfg()) ? 1 : 0;
    if (dims) {
        dims[0] = L.A.box_nx;
        dims[1] = L.A.box_ny;
        dims[2] = L.A.box_nz;
    }
    if (plan) {
        plan[0] = L.A.box2.q;
        plan[1] = L.A.box2.ty;
        plan[2] = L.A.box2.cz;
    }
    if (single_us) *single_us = L.box_single_us;
    if (double_us) *double_us = L.box_double_us;
    return SPARSH_OK;
}

int sparsh_set_deferred_x(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->kernel_cfg().defer_x = enable != 0;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_set_zero_start(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->kernel_cfg().zero_start = enable != 0;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_set_marching_ops(sparsh_handle h, int mode)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (mode < 0 || mode > 2) return fail(SPARSH_EINVAL, "mode must be 0 (never), 1 (where the setup measures it faster) or 2 (wherever the level is a box grid with a plan)");
    h->eng->kernel_cfg().box1 = mode;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_level_marching_ops(sparsh_handle h, int level, int *on, int *plan, double *table_us, double *marching_us)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevLevel &L = h->eng->level(level);
    if (on) *on = (!h->eng->distributed() || L.replicated) && box1_applies(L.A, h->eng->kernel_cfg()) ? 1 : 0;
    if (plan) {
        plan[0] = L.A.box1.q;
        plan[1] = L.A.box1.ty;
        plan[2] = L.A.box1.cz;
    }
    if (table_us) *table_us = L.box1_table_us;
    if (marching_us) *marching_us = L.box1_us;
    return SPARSH_OK;
}

int sparsh_set_box_plan_ex(sparsh_handle h, int level, int kernel, int threads, int q, int ty, int cz)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const int rc = h->eng->set_box_plan(level, kernel, threads, q, ty, cz);
    return rc == SPARSH_OK ? SPARSH_OK : fail(rc, h->eng->error);
}

int sparsh_set_box_plan(sparsh_handle h, int level, int kernel, int q, int ty, int cz)
{
    return sparsh_set_box_plan_ex(h, level, kernel, 1024, q, ty, cz);
}

int sparsh_level_box_threads(sparsh_handle h, int level, int *double_threads, int *marching_threads)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevLevel &L = h->eng->level(level);
    if (double_threads) *double_threads = L.A.box2.q > 0 ? L.A.box2.threads : 0;
    if (marching_threads) *marching_threads = L.A.box1.q > 0 ? L.A.box1.threads : 0;
    return SPARSH_OK;
}

int sparsh_set_box_exact_fma(sparsh_handle h, int mode)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (mode < 0 || mode > 1) return fail(SPARSH_EINVAL, "mode must be 0 (never) or 1 (where every off-diagonal constant of the level is 0 or +-2^k, k >= 0)");
    h->eng->set_box_exact_fma(mode);
    return SPARSH_OK;
}

int sparsh_level_box_exact_fma(sparsh_handle h, int level, int *on, int *rule)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevLevel &L = h->eng->level(level);
    if (on) *on = L.A.box_nx > 0 && L.A.box_fma ? 1 : 0;
    if (rule) *rule = L.A.box_nx > 0 && L.A.box_exact ? 1 : 0;
    return SPARSH_OK;
}

int sparsh_debug_box_exact_offdiag(const double *c)
{
    return c && box_exact_offdiag(c) ? 1 : 0;
}

int sparsh_debug_box_plan_candidates(int kernel, int nx, int ny, int nz, int part_cap, int cap, int *plans)
{
    if (kernel != 1 && kernel != 2) return -1;
    const std::vector<BoxPlan> c = box_plan_candidates(kernel, nx, ny, nz, part_cap);
    for (size_t i = 0; i < c.size() && (int)i < cap && plans; ++i) {
        plans[4 * i] = c[i].threads;
        plans[4 * i + 1] = c[i].q;
        plans[4 * i + 2] = c[i].ty;
        plans[4 * i + 3] = c[i].cz;
    }
    return (int)c.size();
}

int sparsh_set_constant_diagonal(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->kernel_cfg().const_diag = enable != 0;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_level_constant_diagonal(sparsh_handle h, int level, int *is_const, double *value)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevLevel &L = h->eng->level(level);
    if (is_const) *is_const = h->eng->diag_stream(L) == nullptr ? 1 : 0;
    if (value) *value = L.diag_const;
    return SPARSH_OK;
}

int sparsh_set_fused_prolongation(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->kernel_cfg().fuse_prolong = enable != 0;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_level_prolong_fused(sparsh_handle h, int level, int *fused)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    if (!fused) return fail(SPARSH_EINVAL, "null output");
    *fused = !h->eng->level_prolong_fused(level) ? 0 : (h->eng->level(level - 1).pair_aggregates ? 1 : 2);
    return SPARSH_OK;
}

int sparsh_set_paired_restriction(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->kernel_cfg().pair_restrict = enable != 0;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_level_paired(sparsh_handle h, int level, int *paired)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    if (!paired) return fail(SPARSH_EINVAL, "null output");
    *paired = h->eng->level_paired(level);
    return SPARSH_OK;
}

int sparsh_set_index_compression(sparsh_handle h, int mode)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (mode < 0 || mode > 2) return fail(SPARSH_EINVAL, "mode must be 0 (off), 1 (operators that stream from HBM through the CSR-stream kernel) or 2 (every operator)");
    h->eng->kernel_cfg().idx16 = mode;
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_level_index16(sparsh_handle h, int level, long *blocks16, long *blocks)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevCsr &A = h->eng->level(level).A;
    if (blocks16) *blocks16 = A.col16 ? A.nblk16 : 0;
    if (blocks) *blocks = A.nblk;
    return SPARSH_OK;
}

int sparsh_set_smoother(sparsh_handle h, int kind, int sweeps, int order)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    Engine &E = *h->eng;
    if (kind != SPARSH_SMOOTH_JACOBI && kind != SPARSH_SMOOTH_SOR && kind != SPARSH_SMOOTH_CHEBYSHEV)
        return fail(SPARSH_EINVAL, "kind must be SPARSH_SMOOTH_JACOBI (0), SPARSH_SMOOTH_SOR (1) or SPARSH_SMOOTH_CHEBYSHEV (3)");
    if (sweeps < 0) return fail(SPARSH_EINVAL, "sweeps < 0");
    if (order != SPARSH_SOR_FORWARD && order != SPARSH_SOR_SYMMETRIC)
        return fail(SPARSH_EINVAL, "order must be SPARSH_SOR_FORWARD (0) or SPARSH_SOR_SYMMETRIC (1)");
    if (kind == SPARSH_SMOOTH_CHEBYSHEV) {
        if (sweeps > kChebyMaxDegree) return fail(SPARSH_EINVAL, "the Chebyshev degree must be 1..16 (0: the default of 4)");
        if (order != 0) return fail(SPARSH_EINVAL, "the Chebyshev smoother has no order: pass 0");
        if (E.distributed() || (E.comm() && E.comm()->size > 1))
            return fail(SPARSH_EINVAL, "the Chebyshev smoother is not available on a partitioned (multi-GPU) handle");
        if ((E.host_ready() || E.ready()) && E.params().precond_fp32)
            return fail(SPARSH_EINVAL, "the Chebyshev smoother has no fp32 hierarchy: unset params.precond_fp32");
    }
    if (kind == SPARSH_SMOOTH_JACOBI && sweeps > 0 && E.ready() && E.distributed())
        return fail(SPARSH_EINVAL, "a partitioned handle sizes its ghost layers for the sweep count of its setup: change params.sweeps and call sparsh_setup");
    if (kind == SPARSH_SMOOTH_SOR) {
        if (E.distributed() || (E.comm() && E.comm()->size > 1))
            return fail(SPARSH_EINVAL, "the SOR smoother is not available on a partitioned (multi-GPU) handle");
        if ((E.host_ready() || E.ready()) && E.params().precond_fp32)
            return fail(SPARSH_EINVAL, "the SOR smoother has no fp32 hierarchy: unset params.precond_fp32");
    }
    E.set_smoother(kind, sweeps, order);
    return SPARSH_OK;
}

int sparsh_set_chebyshev(sparsh_handle h, double ratio, int lanczos_steps)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (!(ratio == 0.0 || (ratio > 1.0 && std::isfinite(ratio)))) return fail(SPARSH_EINVAL, "ratio must be > 1 (0: the default of 30)");
    if (lanczos_steps < 0 || lanczos_steps > kChebyMaxSteps) return fail(SPARSH_EINVAL, "lanczos_steps must be 1..64 (0: the default of 10)");
    h->eng->set_chebyshev(ratio == 0.0 ? kChebyDefaultRatio : ratio, lanczos_steps == 0 ? kChebyDefaultSteps : lanczos_steps);
    return SPARSH_OK;
}

int sparsh_set_chebyshev_lmax(sparsh_handle h, int level, double lmax)
{
    REQUIRE_HOST(h);
    REQUIRE_LEVEL(h, level);
    if (!(lmax >= 0.0 && std::isfinite(lmax))) return fail(SPARSH_EINVAL, "lmax must be > 0 and finite (0: the estimate)");
    h->eng->set_cheby_lmax(level, lmax);
    return SPARSH_OK;
}

int sparsh_level_chebyshev(sparsh_handle h, int level, double *lmax, double *lmin, double *gershgorin, double *lanczos)
{
    REQUIRE_HOST(h);
    REQUIRE_LEVEL(h, level);
    const ChebyLevel &c = h->eng->level_cheby(level);
    if (lmax) *lmax = c.lmax();
    if (lmin) *lmin = c.lmax() / h->eng->cheby_ratio();
    if (gershgorin) *gershgorin = c.est.gershgorin;
    if (lanczos) *lanczos = c.est.lanczos;
    return SPARSH_OK;
}

int sparsh_level_colors(sparsh_handle h, int level, int *ncolors, int *rows_per_color)
{
    REQUIRE_HOST(h);
    REQUIRE_LEVEL(h, level);
    const ColorClasses &cc = h->eng->level_colors(level);
    if (ncolors) *ncolors = cc.ncolors;
    if (rows_per_color)
        for (int c = 0; c < cc.ncolors; ++c) rows_per_color[c] = cc.start[c + 1] - cc.start[c];
    return SPARSH_OK;
}

int sparsh_level_color_of_rows(sparsh_handle h, int level, int *color)
{
    REQUIRE_HOST(h);
    REQUIRE_LEVEL(h, level);
    if (!color) return fail(SPARSH_EINVAL, "null color");
    const ColorClasses &cc = h->eng->level_colors(level);
    std::copy(cc.color.begin(), cc.color.end(), color);
    return SPARSH_OK;
}

int sparsh_set_sor_path(sparsh_handle h, int mode)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (mode < 0 || mode > 2) return fail(SPARSH_EINVAL, "mode must be 0 (level policy), 1 (per-colour launches) or 2 (one launch per leg)");
    h->eng->set_sor_path(mode);
    h->eng->config_changed();
    return SPARSH_OK;
}

int sparsh_level_sor_layout(sparsh_handle h, int level, int *ncolors, int *single_launch, long *bytes)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const SorLevel *S = h->eng->sor_level(level);
    if (!S) return fail(SPARSH_ESTATE, "the SOR layouts are not built (select SOR before sparsh_setup, or solve / call sparsh_op_sor)");
    if (ncolors) *ncolors = S->ncolors;
    if (single_launch) *single_launch = h->eng->sor_single(level) ? 1 : 0;
    if (bytes) *bytes = (long)S->bytes;
    return SPARSH_OK;
}

int sparsh_num_levels(sparsh_handle h)
{
    if (!h || !h->eng || !h->eng->host_ready()) return 0;
    return (int)h->eng->host().levels.size();
}

int sparsh_level_info(sparsh_handle h, int level, int *nrow, int *nnz, int *p_ncol, int *p_nnz)
{
    REQUIRE_HOST(h);
    REQUIRE_LEVEL(h, level);
    const HostLevel &L = h->eng->host().levels[level];
    if (nrow) *nrow = L.A.nrow;
    if (nnz) *nnz = L.A.nnz();
    if (p_ncol) *p_ncol = L.P.rowptr ? L.P.ncol : 0;
    if (p_nnz) *p_nnz = L.P.rowptr ? L.P.nnz() : 0;
    return SPARSH_OK;
}

int sparsh_level_csr(sparsh_handle h, int level, int which, int *rowptr, int *colindex, double *val)
{
    REQUIRE_HOST(h);
    REQUIRE_LEVEL(h, level);
    const HostLevel &L = h->eng->host().levels[level];
    if (which < 0 || which > 2) return fail(SPARSH_EINVAL, "which must be 0 (A), 1 (P) or 2 (R)");
    const HostCsr &M = (which == 0) ? L.A : (which == 1 ? L.P : L.R);
    if (!M.rowptr) return fail(SPARSH_EINVAL, "no such matrix on this level");
    std::memcpy(rowptr, M.rowptr, sizeof(int) * ((size_t)M.nrow + 1));
    std::memcpy(colindex, M.col, sizeof(int) * (size_t)M.nnz());
    std::memcpy(val, M.val, sizeof(double) * (size_t)M.nnz());
    return SPARSH_OK;
}

int sparsh_coarse_inverse(sparsh_handle h, double *inv)
{
    REQUIRE_HOST(h);
    const HostHierarchy &H = h->eng->host();
    if (!H.coarse_dense) return fail(SPARSH_ESTATE, "the coarsest level is above dense_limit: it is factored on the device (nested-dissection or block-tridiagonal form), no dense inverse exists");
    if (H.coarse_inverse.empty()) return fail(SPARSH_ESTATE, "host copy of the inverse was released by sparsh_setup; use sparsh_setup_host");
    std::memcpy(inv, H.coarse_inverse.data(), sizeof(double) * (size_t)H.nL * H.nL);
    return SPARSH_OK;
}

int sparsh_coarse_info(sparsh_handle h, int *info6, long *bytes)
{
    REQUIRE_HOST(h);
    const HostHierarchy &H = h->eng->host();
    const CoarseSolver &c = h->eng->coarse();
    const bool bt = c.ready() && !c.dense() && !c.nested();
    if (info6) {
        info6[0] = H.nL;
        info6[1] = H.coarse_dense ? 1 : 0;
        info6[2] = bt ? c.block() : 0;
        info6[3] = bt ? c.nblocks() : 0;
        info6[4] = bt ? c.bandwidth() : 0;
        info6[5] = H.extended ? 1 : 0;
    }
    if (bytes) *bytes = c.ready() ? (long)c.bytes() : 0;
    return SPARSH_OK;
}

int sparsh_set_coarse_interface(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->coarse_mut().set_allow_windowed(enable != 0);
    h->eng->coarse_mut().set_unrolled_chain(enable != 2);
    return SPARSH_OK;
}

int sparsh_set_coarse_form(sparsh_handle h, int form, int leaf, int merge_rows)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (form != 0 && form != 1) return fail(SPARSH_EINVAL, "form must be 0 (nested dissection) or 1 (block tridiagonal)");
    h->eng->coarse_mut().set_form(form);
    h->eng->coarse_mut().set_nd_params(leaf, merge_rows);
    return SPARSH_OK;
}

int sparsh_set_coarse_top_merge(sparsh_handle h, int top_merge_rows)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (top_merge_rows < 0) return fail(SPARSH_EINVAL, "top_merge_rows must be >= 0");
    h->eng->coarse_mut().set_nd_params(0, -1, top_merge_rows);
    return SPARSH_OK;
}

int sparsh_coarse_nd_info(sparsh_handle h, int *info6)
{
    REQUIRE_HOST(h);
    const CoarseSolver &c = h->eng->coarse();
    const bool nd = c.ready() && c.nested();
    if (info6) {
        info6[0] = nd ? 1 : 0;
        info6[1] = nd ? c.nd().nnodes() : 0;
        info6[2] = nd ? c.nd().nlevels() : 0;
        info6[3] = nd ? c.nd().max_pivot_rows() : 0;
        info6[4] = nd ? c.nd().launches_per_solve() : 0;
        info6[5] = nd ? c.nd().leaf() : 0;
    }
    return SPARSH_OK;
}

int sparsh_coarse_pivot_info(sparsh_handle h, int *out4)
{
    REQUIRE_HOST(h);
    if (!out4) return fail(SPARSH_EINVAL, "null output");
    h->eng->coarse().pivot_counts(out4);
    return SPARSH_OK;
}

int sparsh_set_coarse_block(sparsh_handle h, int rows)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (rows < 0) return fail(SPARSH_EINVAL, "rows must be >= 0 (0 = built-in rule)");
    h->eng->coarse_mut().set_block_hint(rows);
    return SPARSH_OK;
}

int sparsh_coarse_window(sparsh_handle h, int *window)
{
    REQUIRE_HOST(h);
    const CoarseSolver &c = h->eng->coarse();
    if (window) *window = (c.ready() && !c.dense() && c.windowed()) ? c.window() : 0;
    return SPARSH_OK;
}

double sparsh_setup_seconds(sparsh_handle h) { return (h && h->eng) ? h->eng->setup_seconds : 0.0; }

int sparsh_vcycle(sparsh_handle h, const double *b, double *x, int iterations, double *hist, int hist_cap, int *ncycles)
{
    REQUIRE_CYCLE_FITS(h, SPARSH_AMG);
    REQUIRE_READY(h);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.local_n0();  // multi-GPU: this rank's block of level 0
    DBuf db(E, n, b), dx(E, n, x);
    if (!db.p || !dx.p) return fail(SPARSH_ENODEV, E.error);
    int rc = E.amg_solve_dev(db.p, dx.p, iterations, hist, hist_cap, ncycles);
    dx.get(x);
    if (rc != SPARSH_OK) return fail(rc, E.error);
    return rc;
}

int sparsh_vcycle_dev(sparsh_handle h, const double *b_dev, double *x_dev, int iterations, double *hist, int hist_cap, int *ncycles)
{
    REQUIRE_CYCLE_FITS(h, SPARSH_AMG);
    REQUIRE_READY(h);
    int rc = h->eng->amg_solve_dev(b_dev, x_dev, iterations, hist, hist_cap, ncycles);
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

int sparsh_solve(sparsh_handle h, int method, const double *b, double *x, double *hist, int hist_cap, int *iters)
{
    REQUIRE_NOT_BLOCK_ONLY(method);
    REQUIRE_SMOOTHER_FITS(h, method);
    REQUIRE_CYCLE_FITS(h, method);
    REQUIRE_GMRES_FITS(h, method);
    REQUIRE_READY(h);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.local_n0();  // multi-GPU: this rank's block of level 0
    DBuf db(E, n, b), dx(E, n, x);
    if (!db.p || !dx.p) return fail(SPARSH_ENODEV, E.error);
    int rc = E.solve_dev(method, db.p, dx.p, 0, hist, hist_cap, iters, nullptr);
    dx.get(x);
    if (rc != SPARSH_OK) return fail(rc, E.error);
    return rc;
}

int sparsh_solve_dev(sparsh_handle h, int method, const double *b_dev, double *x_dev, int max_iters, double *hist, int hist_cap,
                     int *iters, double *seconds)
{
    REQUIRE_NOT_BLOCK_ONLY(method);
    REQUIRE_SMOOTHER_FITS(h, method);
    REQUIRE_CYCLE_FITS(h, method);
    REQUIRE_GMRES_FITS(h, method);
    REQUIRE_READY(h);
    int rc = h->eng->solve_dev(method, b_dev, x_dev, max_iters, hist, hist_cap, iters, seconds);
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

// ---- multi-GPU ----

int sparsh_set_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SPARSH_ENODEV, "no HIP device visible");
    if (hipSetDevice(device % n) != hipSuccess) return fail(SPARSH_ENODEV, "hipSetDevice failed");
    return SPARSH_OK;
}

int sparsh_comm_unique_id(char id128[128])
{
    std::string err;
    if (!rccl_unique_id(id128, err)) return fail(SPARSH_ECOMM, err);
    return SPARSH_OK;
}

int sparsh_comm_init_rccl(sparsh_handle h, const char id128[128], int rank, int nranks)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (rank < 0 || rank >= nranks) return fail(SPARSH_EINVAL, "rank out of range");
    std::string err;
    auto c = make_rccl_comm(id128, rank, nranks, err);
    if (!c) return fail(SPARSH_ECOMM, err);
    h->eng->set_comm(std::move(c));
    return SPARSH_OK;
}

int sparsh_comm_group_create(int nranks, void **group)
{
    if (nranks < 1 || !group) return fail(SPARSH_EINVAL, "bad arguments");
    *group = thread_group_create(nranks);
    return SPARSH_OK;
}

void sparsh_comm_group_destroy(void *group) { thread_group_destroy(static_cast<ThreadGroup *>(group)); }

int sparsh_comm_group_set_delay(void *group, double microseconds)
{
    if (!group || microseconds < 0.0) return fail(SPARSH_EINVAL, "bad group / delay");
    thread_group_set_delay(static_cast<ThreadGroup *>(group), microseconds);
    return SPARSH_OK;
}

int sparsh_set_comm_tuning(sparsh_handle h, int mode)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (mode != 0 && mode != 1) return fail(SPARSH_EINVAL, "mode must be 0 (replicate_rows / set_deep_halo decide) or 1 (measured)");
    h->eng->set_comm_tuning(mode);
    return SPARSH_OK;
}

int sparsh_plan_comm_schedule(sparsh_handle h, int nranks, const double *m7)
{
    REQUIRE_HOST(h);
    if (nranks < 2 || !m7) return fail(SPARSH_EINVAL, "nranks >= 2 and seven measured numbers are needed");
    Engine::CommMeasured m;
    m.exchange_us = m7[0];
    m.exchange_us_per_mb = m7[1];
    m.allreduce_us = m7[2];
    m.allgather_us = m7[3];
    m.allgather_us_per_mb = m7[4];
    m.sweep_floor_us = m7[5];
    m.sweep_us_per_mb = m7[6];
    h->eng->plan_comm_schedule(h->eng->params(), nranks, m);
    return SPARSH_OK;
}

int sparsh_comm_schedule(sparsh_handle h, int level, int *info4, double *cost_us3)
{
    REQUIRE_HOST(h);
    if (level < 0 || level >= (int)h->eng->host().levels.size()) return fail(SPARSH_EINVAL, "level out of range");
    const auto &sc = h->eng->comm_schedule();
    if (sc.empty()) return fail(SPARSH_ESTATE, "no measured schedule: one rank, tuning off, or replicate_rows given by the caller");
    const auto &c = sc[level];
    if (info4) {
        info4[0] = c.rows;
        info4[1] = c.halo_rows;
        info4[2] = c.partitioned ? 1 : 0;
        info4[3] = c.deep ? 1 : 0;
    }
    if (cost_us3) {
        cost_us3[0] = c.cost_deep_us;
        cost_us3[1] = c.cost_per_sweep_us;
        cost_us3[2] = c.cost_replicated_us;
    }
    return SPARSH_OK;
}

int sparsh_comm_measured(sparsh_handle h, double *m7)
{
    REQUIRE_HOST(h);
    const auto &m = h->eng->comm_measured();
    if (!m.valid) return fail(SPARSH_ESTATE, "the transport was not measured in this setup");
    if (m7) {
        m7[0] = m.exchange_us;
        m7[1] = m.exchange_us_per_mb;
        m7[2] = m.allreduce_us;
        m7[3] = m.allgather_us;
        m7[4] = m.allgather_us_per_mb;
        m7[5] = m.sweep_floor_us;
        m7[6] = m.sweep_us_per_mb;
    }
    return SPARSH_OK;
}

int sparsh_comm_group_fail_after(void *group, int ncalls)
{
    if (!group) return fail(SPARSH_EINVAL, "null group");
    thread_group_fail_after(static_cast<ThreadGroup *>(group), ncalls);
    return SPARSH_OK;
}

int sparsh_comm_init_group(sparsh_handle h, void *group, int rank)
{
    if (!h || !h->eng || !group) return fail(SPARSH_EINVAL, "bad arguments");
    h->eng->set_comm(make_thread_comm(static_cast<ThreadGroup *>(group), rank));
    return SPARSH_OK;
}

int sparsh_deep_info(sparsh_handle h, int level, int *info4)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevLevel &L = h->eng->level(level);
    info4[0] = L.deep ? L.K : 0;
    info4[1] = L.deep ? L.A.nrow : 0;
    info4[2] = L.deep ? L.A.ncol : 0;
    info4[3] = L.deep ? L.npad : 0;
    return SPARSH_OK;
}

int sparsh_deep_layer_end(sparsh_handle h, int level, int d, int *end)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    const DevLevel &L = h->eng->level(level);
    if (!L.deep || d < 0 || d > L.K) return fail(SPARSH_EINVAL, "not a deep-halo level / layer out of range");
    *end = L.layer_end[d];
    return SPARSH_OK;
}

int sparsh_deep_prefix_spmv(sparsh_handle h, int level, int rows, const double *x_ext, double *y)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    const DevLevel &L = E.level(level);
    if (!L.deep || rows < 0 || rows > L.A.nrow) return fail(SPARSH_EINVAL, "not a deep-halo level / bad prefix");
    DBuf dx(E, (size_t)L.A.ncol, x_ext), dy(E, (size_t)L.A.nrow + 64);
    if (!E.debug_prefix_spmv(level, rows, dx.p, dy.p)) return fail(SPARSH_ENODEV, E.error);
    if (hipMemcpy(y, dy.p, (size_t)rows * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(SPARSH_ENODEV, "D2H failed");
    return SPARSH_OK;
}

int sparsh_set_deep_halo(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->set_deep_halo(enable != 0);
    return SPARSH_OK;
}

long sparsh_exchanges_issued(sparsh_handle h) { return (h && h->eng) ? h->eng->exchanges_issued() : 0; }

int sparsh_set_overlap(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->set_overlap(enable != 0);
    return SPARSH_OK;
}

int sparsh_local_range(sparsh_handle h, int level, int *lo, int *hi, int *replicated)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    const Partition &p = E.partition(level);
    const int r = E.comm() ? E.comm()->rank : 0;
    if (lo) *lo = p.replicated ? 0 : p.lo(r);
    if (hi) *hi = p.replicated ? p.n : p.hi(r);
    if (replicated) *replicated = p.replicated ? 1 : 0;
    return SPARSH_OK;
}

// Host-only planning query (needs sparsh_setup_host): the part of operator `which` (0 A_l, 1 P_l,
// 2 R_l) that `rank` of `nranks` holds when no level is replicated, and its halo plan.
int sparsh_dist_local_op(sparsh_handle h, int level, int which, int rank, int nranks, int *sizes8)
{
    REQUIRE_HOST(h);
    REQUIRE_LEVEL(h, level);
    if (nranks < 1 || rank < 0 || rank >= nranks || which < 0 || which > 2) return fail(SPARSH_EINVAL, "bad arguments");
    const HostHierarchy &H = h->eng->host();
    const int nl = (int)H.levels.size();
    if (which != 0 && level + 1 >= nl) return fail(SPARSH_EINVAL, "no coarser level");
    std::vector<Partition> parts((size_t)nl);
    for (int l = 0; l <= std::min(level + 1, nl - 1); ++l)
        parts[l] = (l == 0) ? make_partition(H.levels[0].A.nrow, nranks) : coarse_partition(H.levels[l - 1].R, parts[l - 1]);
    const HostLevel &L = H.levels[level];
    if (which == 0)
        h->cached_op = extract_local(L.A, parts[level], parts[level], rank);
    else if (which == 1)
        h->cached_op = extract_local(L.P, parts[level], parts[level + 1], rank);
    else
        h->cached_op = extract_local(L.R, parts[level + 1], parts[level], rank);
    const LocalOp &o = h->cached_op;
    const Partition &rowsP = (which == 2) ? parts[level + 1] : parts[level];
    sizes8[0] = o.M.nrow;
    sizes8[1] = o.M.nnz();
    sizes8[2] = o.plan.nloc;
    sizes8[3] = o.plan.nhalo;
    sizes8[4] = (int)o.plan.send.size();
    sizes8[5] = (int)o.plan.recv.size();
    sizes8[6] = (int)o.plan.send_idx.size();
    sizes8[7] = rowsP.lo(rank);
    return SPARSH_OK;
}

int sparsh_dist_local_op_get(sparsh_handle h, int *rowptr, int *col, double *val, int *halo_global, int *send_idx, int *send_segs3,
                             int *recv_segs3)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    const LocalOp &o = h->cached_op;
    if (!o.M.rowptr) return fail(SPARSH_ESTATE, "call sparsh_dist_local_op first");
    std::memcpy(rowptr, o.M.rowptr, sizeof(int) * ((size_t)o.M.nrow + 1));
    std::memcpy(col, o.M.col, sizeof(int) * (size_t)o.M.nnz());
    std::memcpy(val, o.M.val, sizeof(double) * (size_t)o.M.nnz());
    std::copy(o.plan.halo_global.begin(), o.plan.halo_global.end(), halo_global);
    std::copy(o.plan.send_idx.begin(), o.plan.send_idx.end(), send_idx);
    for (size_t k = 0; k < o.plan.send.size(); ++k) {
        send_segs3[3 * k] = o.plan.send[k].peer;
        send_segs3[3 * k + 1] = o.plan.send[k].off;
        send_segs3[3 * k + 2] = o.plan.send[k].cnt;
    }
    for (size_t k = 0; k < o.plan.recv.size(); ++k) {
        recv_segs3[3 * k] = o.plan.recv[k].peer;
        recv_segs3[3 * k + 1] = o.plan.recv[k].off;
        recv_segs3[3 * k + 2] = o.plan.recv[k].cnt;
    }
    return SPARSH_OK;
}

int sparsh_dist_deep_op(sparsh_handle h, int level, int rank, int nranks, int K, int depth, int *sizes8)
{
    REQUIRE_HOST(h);
    REQUIRE_LEVEL(h, level);
    if (nranks < 2 || rank < 0 || rank >= nranks || K < 1 || depth < 1 || depth > K) return fail(SPARSH_EINVAL, "bad arguments");
    const HostHierarchy &H = h->eng->host();
    std::vector<Partition> parts((size_t)level + 1);
    for (int l = 0; l <= level; ++l)
        parts[l] = (l == 0) ? make_partition(H.levels[0].A.nrow, nranks) : coarse_partition(H.levels[l - 1].R, parts[l - 1]);
    h->cached_deep = extract_local_deep(H.levels[level].A, parts[level], rank, K, {depth});
    const DeepLocal &d = h->cached_deep;
    sizes8[0] = d.M.nrow;
    sizes8[1] = d.M.nnz();
    sizes8[2] = d.nloc;
    sizes8[3] = d.npad;
    sizes8[4] = (int)d.global_of.size();
    sizes8[5] = (int)d.plans[0].send.size();
    sizes8[6] = (int)d.plans[0].recv.size();
    sizes8[7] = (int)d.plans[0].send_idx.size();
    return SPARSH_OK;
}

int sparsh_dist_deep_op_get(sparsh_handle h, int *rowptr, int *col, double *val, int *global_of, int *layer_end, int *send_idx,
                            int *send_segs3, int *recv_pos, int *recv_segs3)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    const DeepLocal &d = h->cached_deep;
    if (!d.M.rowptr) return fail(SPARSH_ESTATE, "call sparsh_dist_deep_op first");
    const DeepPlan &pl = d.plans[0];
    std::memcpy(rowptr, d.M.rowptr, sizeof(int) * ((size_t)d.M.nrow + 1));
    std::memcpy(col, d.M.col, sizeof(int) * (size_t)d.M.nnz());
    std::memcpy(val, d.M.val, sizeof(double) * (size_t)d.M.nnz());
    std::copy(d.global_of.begin(), d.global_of.end(), global_of);
    std::copy(d.layer_end.begin(), d.layer_end.end(), layer_end);
    std::copy(pl.send_idx.begin(), pl.send_idx.end(), send_idx);
    std::copy(pl.recv_pos.begin(), pl.recv_pos.end(), recv_pos);
    for (size_t k = 0; k < pl.send.size(); ++k) {
        send_segs3[3 * k] = pl.send[k].peer;
        send_segs3[3 * k + 1] = pl.send[k].off;
        send_segs3[3 * k + 2] = pl.send[k].cnt;
    }
    for (size_t k = 0; k < pl.recv.size(); ++k) {
        recv_segs3[3 * k] = pl.recv[k].peer;
        recv_segs3[3 * k + 1] = pl.recv[k].off;
        recv_segs3[3 * k + 2] = pl.recv[k].cnt;
    }
    return SPARSH_OK;
}

int sparsh_krylov_init_dev(sparsh_handle h, int method, const double *b_dev, double *x_dev)
{
    REQUIRE_NOT_BLOCK_ONLY(method);
    REQUIRE_SMOOTHER_FITS(h, method);
    REQUIRE_CYCLE_FITS(h, method);
    REQUIRE_READY(h);
    if (method != SPARSH_CG && method != SPARSH_PCG) return fail(SPARSH_EINVAL, "stepwise interface covers SPARSH_CG and SPARSH_PCG");
    int rc = h->eng->pcg_init(b_dev, x_dev, method == SPARSH_PCG);
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

int sparsh_krylov_step_dev(sparsh_handle h, int nsteps, int *done, double *residual)
{
    REQUIRE_READY(h);
    int rc = h->eng->pcg_steps(nsteps, done);
    if (residual) *residual = h->eng->krylov_residual();
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

int sparsh_krylov_history(sparsh_handle h, double *hist, int hist_cap, int *iters)
{
    REQUIRE_READY(h);
    int c = h->eng->krylov_hist(hist, hist_cap);
    if (iters) *iters = c;
    return SPARSH_OK;
}

int sparsh_op_spmv(sparsh_handle h, int level, const double *x, double *y)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    const DevLevel &L = E.level(level);
    DBuf dx(E, (size_t)L.A.ncol, x), dy(E, (size_t)L.n);
    E.op_spmv(level, dx.p, dy.p);
    return done(E, dy.get(y));
}

int sparsh_op_jacobi(sparsh_handle h, int level, const double *b, double *x, int sweeps, int x_is_zero)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    if (sweeps < 0) return fail(SPARSH_EINVAL, "sweeps < 0");
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(level).n;
    DBuf db(E, n, b), dx(E, n, x), dt(E, n);
    E.op_jacobi(level, db.p, dx.p, dt.p, sweeps, x_is_zero != 0);
    return done(E, dx.get(x));
}

int sparsh_op_sor(sparsh_handle h, int level, const double *b, double *x, int sweeps, int reverse, int x_is_zero)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    if (sweeps < 0) return fail(SPARSH_EINVAL, "sweeps < 0");
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(level).n;
    DBuf db(E, n, b), dx(E, n, x);
    if (!db.p || !dx.p) return fail(SPARSH_ENODEV, E.error);
    if (!E.op_sor(level, db.p, dx.p, sweeps, reverse != 0, x_is_zero != 0)) return fail(E.fault() != SPARSH_OK ? E.fault() : SPARSH_ENODEV, E.error);
    return done(E, dx.get(x));
}

int sparsh_op_cheby(sparsh_handle h, int level, const double *b, double *x, int degree, int x_is_zero)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    if (degree < 0 || degree > kChebyMaxDegree) return fail(SPARSH_EINVAL, "degree must be 0..16");
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(level).n;
    DBuf db(E, n, b), dx(E, n, x), dt(E, n);
    if (!db.p || !dx.p || !dt.p) return fail(SPARSH_ENODEV, E.error);
    if (x_is_zero && degree == 0) launch_fill((int)n, 0.0, dx.p, E.stream());
    if (!E.op_cheby(level, db.p, dx.p, dt.p, degree, x_is_zero != 0)) return fail(E.fault() != SPARSH_OK ? E.fault() : SPARSH_ENUMERIC, E.error);
    return done(E, dx.get(x));
}

int sparsh_op_residual(sparsh_handle h, int level, const double *b, const double *x, double *r)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(level).n;
    DBuf db(E, n, b), dx(E, n, x), dr(E, n);
    E.op_residual(level, db.p, dx.p, dr.p);
    return done(E, dr.get(r));
}

int sparsh_op_resnorm(sparsh_handle h, int level, const double *b, const double *x, double *nrm)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(level).n;
    DBuf db(E, n, b), dx(E, n, x);
    *nrm = E.op_resnorm(level, db.p, dx.p);
    return SPARSH_OK;
}

int sparsh_op_spmv_dot(sparsh_handle h, int level, const double *x, double *y, double *dot)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    const DevLevel &L = E.level(level);
    DBuf dx(E, (size_t)L.A.ncol, x), dy(E, (size_t)L.n);
    if (!dx.p || !dy.p) return fail(SPARSH_ENODEV, E.error);
    const double d = E.op_spmv_dot(level, dx.p, dy.p);
    if (dot) *dot = d;
    return done(E, dy.get(y));
}

int sparsh_op_jacobi_dot(sparsh_handle h, int level, const double *b, const double *x, double *y, double *dot)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    const DevLevel &L = E.level(level);
    DBuf db(E, (size_t)L.n, b), dx(E, (size_t)L.A.ncol, x), dy(E, (size_t)L.n);
    if (!db.p || !dx.p || !dy.p) return fail(SPARSH_ENODEV, E.error);
    const double d = E.op_jacobi_dot(level, db.p, dx.p, dy.p);
    if (dot) *dot = d;
    return done(E, dy.get(y));
}

int sparsh_op_restrict(sparsh_handle h, int level, const double *r, double *bc)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    if (level + 1 >= h->eng->nlevels()) return fail(SPARSH_EINVAL, "no coarser level");
    Engine &E = *h->eng;
    DBuf dr(E, (size_t)E.level(level).n, r), dc(E, (size_t)E.level(level + 1).n);
    E.op_restrict(level, dr.p, dc.p);
    return done(E, dc.get(bc));
}

int sparsh_op_residual_restrict(sparsh_handle h, int level, const double *b, const double *x, double *bc, double *xc)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    if (!E.level_paired(level)) return fail(SPARSH_ESTATE, "the level does not take the fused residual + restriction launch (sparsh_level_paired)");
    DBuf db(E, (size_t)E.level(level).n, b), dx(E, (size_t)E.level(level).A.ncol, x);
    DBuf dc(E, (size_t)E.level(level + 1).n), dz(E, (size_t)E.level(level + 1).n);
    E.op_residual_restrict(level, db.p, dx.p, dc.p, dz.p);
    const int rc = done(E, dc.get(bc));
    return rc != SPARSH_OK ? rc : done(E, dz.get(xc));
}

int sparsh_op_jacobi_prolong(sparsh_handle h, int level, const double *b, const double *x, double *xf)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    if (!E.level_prolong_fused(level)) return fail(SPARSH_ESTATE, "the level's last post-sweep does not prolongate itself (sparsh_level_prolong_fused)");
    DBuf db(E, (size_t)E.level(level).n, b), dx(E, (size_t)E.level(level).A.ncol, x), df(E, (size_t)E.level(level - 1).n, xf);
    E.op_jacobi_prolong(level, db.p, dx.p, df.p);
    return done(E, df.get(xf));
}

int sparsh_op_prolong(sparsh_handle h, int level, const double *xc, double *xf)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    if (level + 1 >= h->eng->nlevels()) return fail(SPARSH_EINVAL, "no coarser level");
    Engine &E = *h->eng;
    DBuf dc(E, (size_t)E.level(level + 1).n, xc), df(E, (size_t)E.level(level).n, xf);
    E.op_prolong(level, dc.p, df.p);
    return done(E, df.get(xf));
}

int sparsh_op_coarse(sparsh_handle h, const double *b, double *x)
{
    REQUIRE_READY(h);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(E.nlevels() - 1).n;
    DBuf db(E, n, b), dx(E, n);
    E.op_coarse(db.p, dx.p);
    return done(E, dx.get(x));
}

int sparsh_op_precond_f32(sparsh_handle h, const double *r, double *z)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(0).n;
    DBuf dr(E, n, r), dz(E, n);
    if (!E.op_precond_f32(dr.p, dz.p)) return fail(SPARSH_ESTATE, E.error);
    return done(E, dz.get(z));
}

// ---- the steps of the fp32 cycle one at a time (Engine::f32_*): float vectors in and out, nothing converted on the way
}  // extern "C"

namespace {

// RAII device buffer of floats (DBuf's twin)
struct FBuf {
    Engine &E;
    float *p = nullptr;
    size_t n;
    FBuf(Engine &e, size_t count, const float *src = nullptr) : E(e), n(count)
    {
        p = static_cast<float *>(E.dalloc(std::max(count, (size_t)1) * sizeof(float)));
        if (p && src && count) (void)hipMemcpy(p, src, count * sizeof(float), hipMemcpyHostToDevice);
    }
    ~FBuf() { E.dfree(p); }
    bool get(float *dst, const float *from = nullptr)
    {
        (void)hipStreamSynchronize(E.stream());
        return n == 0 || hipMemcpy(dst, from ? from : p, n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
    }
};

// The checks that need no device come first, so that they answer the same on a host-only handle: the mode (SPARSH_ESTATE), then the
// level (SPARSH_EINVAL).  After the device checks, precond_fp32_active() covers a float hierarchy whose setup failed.
#define REQUIRE_F32_MODE(h)                                                                                                          \
    REQUIRE_HOST(h);                                                                                                                 \
    if (!(h)->eng->params().precond_fp32 || (h)->eng->host().levels.size() < 2) return fail(SPARSH_ESTATE, kF32NotBuilt)

#define REQUIRE_F32_DEVICE(h) \
    REQUIRE_READY(h);         \
    REQUIRE_SINGLE(h);        \
    if (!(h)->eng->precond_fp32_active()) return fail(SPARSH_ESTATE, kF32NotBuilt)

// a level with a float operator and transfer operators: every level but the coarsest
#define REQUIRE_F32_LEVEL(h, l)                                                                                             \
    REQUIRE_F32_MODE(h);                                                                                                    \
    REQUIRE_LEVEL(h, l);                                                                                                    \
    if ((l) + 1 >= (int)(h)->eng->host().levels.size())                                                                     \
        return fail(SPARSH_EINVAL, "the coarsest level has no float operator (sparsh_op_coarse_f32 solves on it)"); \
    REQUIRE_F32_DEVICE(h)

}  // namespace

extern "C" {

int sparsh_level_f32_layout(sparsh_handle h, int level, int *layout)
{
    REQUIRE_F32_MODE(h);
    REQUIRE_LEVEL(h, level);
    REQUIRE_F32_DEVICE(h);
    const Engine &E = *h->eng;
    if (layout) *layout = level + 1 >= E.nlevels() ? 0 : (E.level_f32_sdia(level) ? 1 : 2);
    return SPARSH_OK;
}

int sparsh_op_jacobi_f32(sparsh_handle h, int level, const float *b, float *x, int sweeps, int x_is_zero)
{
    REQUIRE_F32_LEVEL(h, level);
    if (sweeps < 0) return fail(SPARSH_EINVAL, "sweeps < 0");
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(level).n;
    FBuf db(E, n, b), dx(E, n, x), dt(E, n);
    if (!db.p || !dx.p || !dt.p) return fail(SPARSH_ENODEV, E.error);
    const float *res = E.op_jacobi_f32(level, db.p, dx.p, dt.p, sweeps, x_is_zero != 0);
    return done(E, dx.get(x, res));
}

int sparsh_op_residual_f32(sparsh_handle h, int level, const float *b, const float *x, float *r)
{
    REQUIRE_F32_LEVEL(h, level);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(level).n;
    FBuf db(E, n, b), dx(E, n, x), dr(E, n);
    if (!db.p || !dx.p || !dr.p) return fail(SPARSH_ENODEV, E.error);
    E.f32_residual(level, db.p, dx.p, dr.p);
    return done(E, dr.get(r));
}

int sparsh_op_restrict_f32(sparsh_handle h, int level, const float *r, float *bc)
{
    REQUIRE_F32_LEVEL(h, level);
    Engine &E = *h->eng;
    FBuf dr(E, (size_t)E.level(level).n, r), dc(E, (size_t)E.level(level + 1).n);
    if (!dr.p || !dc.p) return fail(SPARSH_ENODEV, E.error);
    E.f32_restrict(level, dr.p, dc.p);
    return done(E, dc.get(bc));
}

int sparsh_op_prolong_f32(sparsh_handle h, int level, const float *xc, float *xf)
{
    REQUIRE_F32_LEVEL(h, level);
    Engine &E = *h->eng;
    FBuf dc(E, (size_t)E.level(level + 1).n, xc), df(E, (size_t)E.level(level).n, xf);
    if (!dc.p || !df.p) return fail(SPARSH_ENODEV, E.error);
    E.f32_prolong(level, dc.p, df.p);
    return done(E, df.get(xf));
}

int sparsh_op_coarse_f32(sparsh_handle h, const float *b, float *x)
{
    REQUIRE_F32_MODE(h);
    REQUIRE_F32_DEVICE(h);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(E.nlevels() - 1).n;
    FBuf db(E, n, b), dx(E, n);
    if (!db.p || !dx.p) return fail(SPARSH_ENODEV, E.error);
    E.f32_coarse(db.p, dx.p);
    return done(E, dx.get(x));
}

int sparsh_op_cvt_f32(sparsh_handle h, long n, const double *in, float *out)
{
    REQUIRE_F32_MODE(h);
    if (n <= 0) return fail(SPARSH_EINVAL, "n <= 0");
    REQUIRE_F32_DEVICE(h);
    Engine &E = *h->eng;
    DBuf di(E, (size_t)n, in);
    FBuf dout(E, (size_t)n);
    if (!di.p || !dout.p) return fail(SPARSH_ENODEV, E.error);
    E.f32_cvt(n, di.p, dout.p);
    return done(E, dout.get(out));
}

int sparsh_op_cvt_f2d_dot(sparsh_handle h, int n, const float *z32, const double *r, double *z, double *dot)
{
    REQUIRE_F32_MODE(h);
    if (n <= 0) return fail(SPARSH_EINVAL, "n <= 0");
    REQUIRE_F32_DEVICE(h);
    Engine &E = *h->eng;
    FBuf dz32(E, (size_t)n, z32);
    DBuf dr(E, (size_t)n, r), dz(E, (size_t)n);
    if (!dz32.p || !dr.p || !dz.p) return fail(SPARSH_ENODEV, E.error);
    const double d = E.op_cvt_f2d_dot(n, dz32.p, dr.p, dz.p);
    if (dot) *dot = d;
    return done(E, dz.get(z));
}

int sparsh_op_precond(sparsh_handle h, const double *r, double *z)
{
    REQUIRE_CYCLE_FITS(h, SPARSH_AMG);
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(0).n;
    DBuf dr(E, n, r), dz(E, n);
    if (!dr.p || !dz.p) return fail(SPARSH_ENODEV, E.error);
    if (int rc = E.op_precond(dr.p, dz.p); rc != SPARSH_OK) return fail(rc, E.error);
    return done(E, dz.get(z));
}

int sparsh_set_cycle(sparsh_handle h, int kind, int stride)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (kind != SPARSH_CYCLE_V && kind != SPARSH_CYCLE_W && kind != SPARSH_CYCLE_K)
        return fail(SPARSH_EINVAL, "kind must be SPARSH_CYCLE_V (0), SPARSH_CYCLE_W (1) or SPARSH_CYCLE_K (2)");
    if (stride < 0 || stride > 8) return fail(SPARSH_EINVAL, "stride must be 1..8 (0: the default of 3)");
    h->eng->set_cycle(kind, stride == 0 ? Engine::kCycleDefaultStride : stride);
    return SPARSH_OK;
}

int sparsh_cycle_info(sparsh_handle h, int *kind, int *stride, int *nlevels_wk, long *level_visits, long *bytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    const Engine &E = *h->eng;
    if (kind) *kind = E.cycle_kind();
    if (stride) *stride = E.cycle_stride();
    if (nlevels_wk) *nlevels_wk = E.host_ready() ? E.wk_level_count() : 0;
    if (level_visits) *level_visits = E.host_ready() ? E.cycle_visits() : 0;
    if (bytes) *bytes = (long)E.wk_bytes();
    return SPARSH_OK;
}

int sparsh_level_cycle(sparsh_handle h, int level, int *is_wk, long *visits)
{
    REQUIRE_HOST(h);
    REQUIRE_LEVEL(h, level);
    if (is_wk) *is_wk = h->eng->wk_level(level) ? 1 : 0;
    if (visits) *visits = h->eng->level_visits(level);
    return SPARSH_OK;
}

int sparsh_op_kstep(sparsh_handle h, int level, const double *b, const double *c, const double *d, double *r, double *x, double *scal8)
{
    if (!b || !c || !d || !r || !x || !scal8) return fail(SPARSH_EINVAL, "null array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.level(level).n;
    DBuf db(E, n, b), dc(E, n, c), dd(E, n, d), dr(E, n), dx(E, n), ds(E, 8);
    if (!db.p || !dc.p || !dd.p || !dr.p || !dx.p || !ds.p) return fail(SPARSH_ENODEV, E.error);
    if (int rc = E.op_kstep(level, db.p, dc.p, dd.p, dr.p, dx.p, ds.p); rc != SPARSH_OK) return fail(rc, E.error);
    const bool ok = dr.get(r) && dx.get(x) && ds.get(scal8);
    return done(E, ok);
}

// ---- constant null space ----

int sparsh_set_nullspace(sparsh_handle h, int kind)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (kind != SPARSH_NULLSPACE_NONE && kind != SPARSH_NULLSPACE_CONSTANT)
        return fail(SPARSH_EINVAL, "null space kind must be SPARSH_NULLSPACE_NONE (0) or SPARSH_NULLSPACE_CONSTANT (1)");
    h->eng->set_nullspace(kind);
    return SPARSH_OK;
}

int sparsh_nullspace_info(sparsh_handle h, int *kind, int *pinned_row, double *row_defect, double *col_defect)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    const Engine &E = *h->eng;
    const bool on = E.nullspace_built() == SPARSH_NULLSPACE_CONSTANT;
    if (kind) *kind = E.nullspace_built();
    if (pinned_row) *pinned_row = on ? E.pinned_row() : -1;
    if (row_defect) *row_defect = on ? E.row_defect() : 0.0;
    if (col_defect) *col_defect = on ? E.col_defect() : 0.0;
    return SPARSH_OK;
}

// x -= mean(x) on a device vector of any 8-byte alignment (r_dev non-null: *dot = x.r of the projected x)
int sparsh_op_project_dev(sparsh_handle h, int n, double *x_dev, const double *r_dev, double *mean, double *dot)
{
    if (!h || !h->eng || !x_dev || n <= 0) return fail(SPARSH_EINVAL, "bad arguments");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    if (int rc = E.op_project(n, x_dev, r_dev, mean, dot); rc != SPARSH_OK) return fail(rc, E.error);
    return SPARSH_OK;
}

int sparsh_op_project(sparsh_handle h, int n, double *x, double *mean)
{
    if (!h || !h->eng || !x || n <= 0) return fail(SPARSH_EINVAL, "bad arguments");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    DBuf dx(E, (size_t)n, x);
    if (!dx.p) return fail(SPARSH_ENODEV, E.error);
    if (int rc = sparsh_op_project_dev(h, n, dx.p, nullptr, mean, nullptr); rc != SPARSH_OK) return rc;
    return done(E, dx.get(x));
}

int sparsh_op_project_dot(sparsh_handle h, int n, double *z, const double *r, double *mean, double *dot)
{
    if (!h || !h->eng || !z || !r || n <= 0) return fail(SPARSH_EINVAL, "bad arguments");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    DBuf dz(E, (size_t)n, z), dr(E, (size_t)n, r);
    if (!dz.p || !dr.p) return fail(SPARSH_ENODEV, E.error);
    if (int rc = sparsh_op_project_dev(h, n, dz.p, dr.p, mean, dot); rc != SPARSH_OK) return rc;
    return done(E, dz.get(z));
}

int sparsh_set_gmres(sparsh_handle h, int restart)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (int rc = h->eng->set_gmres(restart); rc != SPARSH_OK) return fail(rc, h->eng->error);
    return SPARSH_OK;
}

int sparsh_gmres_info(sparsh_handle h, int *restart, long *basis_bytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (restart) *restart = h->eng->gmres_restart();
    if (basis_bytes) *basis_bytes = (long)h->eng->gmres_basis_bytes();
    return SPARSH_OK;
}

int sparsh_set_gmres_basis(sparsh_handle h, int precision)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (int rc = h->eng->set_gmres_basis(precision); rc != SPARSH_OK) return fail(rc, h->eng->error);
    return SPARSH_OK;
}

int sparsh_gmres_basis(sparsh_handle h, int *precision)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (precision) *precision = h->eng->gmres_basis();
    return SPARSH_OK;
}

int sparsh_op_dot(sparsh_handle h, int n, const double *x, const double *y, double *out)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    if (n <= 0) return fail(SPARSH_EINVAL, "n <= 0");
    Engine &E = *h->eng;
    DBuf dx(E, (size_t)n, x), dy(E, (size_t)n, y);
    *out = E.op_dot(n, dx.p, dy.p);
    return SPARSH_OK;
}

int sparsh_op_nrm2(sparsh_handle h, int n, const double *x, double *out)
{
    double d = 0.0;
    int rc = sparsh_op_dot(h, n, x, x, &d);
    if (rc == SPARSH_OK) *out = std::sqrt(d);
    return rc;
}

int sparsh_op_axpby(sparsh_handle h, int n, double a, const double *x, double bcoef, double *y)
{
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    if (n <= 0) return fail(SPARSH_EINVAL, "n <= 0");
    Engine &E = *h->eng;
    DBuf dx(E, (size_t)n, x), dy(E, (size_t)n, y);
    launch_axpby(n, a, dx.p, bcoef, dy.p, E.stream());
    return done(E, dy.get(y));
}

// ---- operator-level hooks of the GMRES kernels (krylov_kernels.hip): the handle lends its stream and allocator only
}  // extern "C"

namespace {

// nv host vectors V[nv][n] (nullptr: none copied in) in the engine's basis layout (Engine::gmres_basis_alloc); fp32: rounded to float
// on the host, zero-padded
struct GsBasis {
    Engine &E;
    double *d = nullptr;
    float *f = nullptr;
    long stride = 0;
    bool ok = false;
    GsBasis(Engine &e, int n, int nv, int precision, const double *V) : E(e)
    {
        if (!E.gmres_basis_alloc(n, nv, precision, d, f, stride)) return;
        if (hipStreamSynchronize(E.stream()) != hipSuccess) return;  // (the zeroing runs on the stream, the copies below do not)
        if (!V) {
            ok = true;  // left as allocated
        } else if (f) {
            std::vector<float> host((size_t)nv * (size_t)stride, 0.f);
            for (int k = 0; k < nv; ++k)
                for (int i = 0; i < n; ++i) host[(size_t)k * stride + i] = (float)V[(size_t)k * n + i];
            ok = hipMemcpy(f, host.data(), host.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
        } else {
            ok = true;
            for (int k = 0; k < nv && ok; ++k)
                ok = hipMemcpy(d + (size_t)k * stride, V + (size_t)k * n, (size_t)n * 8, hipMemcpyHostToDevice) == hipSuccess;
        }
    }
    ~GsBasis()
    {
        E.dfree(d);
        E.dfree(f);
    }
};

// a vector of `stride` doubles: src (or `fill`) in rows [0, n), `fill` behind them
bool fill_padded(DBuf &b, int n, const double *src, double fill)
{
    std::vector<double> host(b.n, fill);
    if (src) std::copy(src, src + n, host.begin());
    return b.p && hipMemcpy(b.p, host.data(), b.n * 8, hipMemcpyHostToDevice) == hipSuccess;
}

int gs_args(sparsh_handle h, int n, int nv, int precision)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (n <= 0) return fail(SPARSH_EINVAL, "n <= 0");
    if (nv < 1 || nv > kGmresMaxRestart + 1) return fail(SPARSH_EINVAL, "nv must be in 1.." + std::to_string(kGmresMaxRestart + 1));
    if (precision != SPARSH_BASIS_FP64 && precision != SPARSH_BASIS_FP32)
        return fail(SPARSH_EINVAL, "basis precision must be SPARSH_BASIS_FP64 (0) or SPARSH_BASIS_FP32 (1)");
    return SPARSH_OK;
}

}  // namespace

extern "C" {

int sparsh_op_gs_dot(sparsh_handle h, int n, int nv, int precision, const double *V, const double *w, int want_ww, double *sums)
{
    if (int rc = gs_args(h, n, nv, precision); rc != SPARSH_OK) return rc;
    if (!V || !w || !sums) return fail(SPARSH_EINVAL, "null array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    const int g = gs_grid(n), cnt = nv + (want_ww ? 1 : 0);
    GsBasis B(E, n, nv, precision, V);
    DBuf dw(E, (size_t)B.stride), part(E, (size_t)(nv + 1) * g), out(E, (size_t)cnt);
    if (!B.ok || !part.p || !out.p || !fill_padded(dw, n, w, 0.0)) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    double *ww = want_ww ? part.p + (size_t)nv * g : nullptr;
    if (B.f) launch_gs_dot(n, B.stride, B.f, nv, dw.p, part.p, ww, E.stream());
    else launch_gs_dot(n, B.stride, B.d, nv, dw.p, part.p, ww, E.stream());
    launch_gs_finalize(part.p, g, cnt, out.p, E.stream());  // (w.w is row nv of the partial sums)
    return done(E, out.get(sums));
}

int sparsh_op_gs_update(sparsh_handle h, int n, int nv, int precision, const double *V, const double *coef, const double *w_in,
                        int in_place, int want_dots, int want_ww, double sentinel, double *w_out, double *sums, double *tail, int *ntail)
{
    if (int rc = gs_args(h, n, nv, precision); rc != SPARSH_OK) return rc;
    if (!V || !coef || !w_out || !sums || !tail || !ntail) return fail(SPARSH_EINVAL, "null array");
    if (in_place && !w_in) return fail(SPARSH_EINVAL, "an update in place needs w_in");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    const int g = gs_grid(n);
    GsBasis B(E, n, nv, precision, V);
    const size_t stride = (size_t)B.stride;
    DBuf dh(E, (size_t)nv, coef), din(E, (w_in && !in_place) ? stride : 1), dout(E, stride), part(E, (size_t)(nv + 1) * g), out(E, (size_t)nv + 1);
    if (!B.ok || !dh.p || !din.p || !part.p || !out.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    if (!fill_padded(dout, n, in_place ? w_in : nullptr, sentinel)) return fail(SPARSH_ENODEV, "H2D failed");
    if (w_in && !in_place && !fill_padded(din, n, w_in, sentinel)) return fail(SPARSH_ENODEV, "H2D failed");
    if (!fill_padded(out, 0, nullptr, 0.0)) return fail(SPARSH_ENODEV, "H2D failed");  // (sums not asked for read 0)
    const double *src = !w_in ? nullptr : in_place ? dout.p : din.p;
    double *dots = want_dots ? part.p : nullptr, *ww = want_ww ? part.p + (size_t)nv * g : nullptr;
    if (B.f) launch_gs_update(n, B.stride, B.f, nv, dh.p, src, dout.p, dots, ww, E.stream());
    else launch_gs_update(n, B.stride, B.d, nv, dh.p, src, dout.p, dots, ww, E.stream());
    if (want_dots) launch_gs_finalize(part.p, g, nv, out.p, E.stream());
    if (want_ww) launch_gs_finalize(ww, g, 1, out.p + nv, E.stream());
    std::vector<double> full(stride);
    if (!dout.get(full.data()) || !out.get(sums)) return done(E, false);
    std::copy(full.begin(), full.begin() + n, w_out);
    std::copy(full.begin() + n, full.end(), tail);
    *ntail = (int)(stride - (size_t)n);
    return done(E, true);
}

int sparsh_op_gs_scale(sparsh_handle h, int n, int precision, const double *w, double d, double *v, double *vd, double *tail, int *ntail)
{
    if (int rc = gs_args(h, n, 1, precision); rc != SPARSH_OK) return rc;
    if (!w || !v || !ntail) return fail(SPARSH_EINVAL, "null array");
    if (precision == SPARSH_BASIS_FP32 && (!vd || !tail)) return fail(SPARSH_EINVAL, "a float basis returns vd and the padding");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    GsBasis B(E, n, 1, precision, precision == SPARSH_BASIS_FP64 ? w : nullptr);  // a double vector is scaled in place
    const size_t stride = (size_t)B.stride;
    DBuf dd(E, 1, &d);
    if (!B.ok || !dd.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    *ntail = 0;
    if (!B.f) {
        launch_gs_scale(n, B.d, dd.p, E.stream());
        (void)hipStreamSynchronize(E.stream());
        return done(E, hipMemcpy(v, B.d, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess);
    }
    DBuf dw(E, stride), dvd(E, stride);
    if (!fill_padded(dw, n, w, 0.0) || !fill_padded(dvd, 0, nullptr, -1.0)) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");  // (vd: every row is to be written)
    launch_gs_scale(n, dw.p, B.f, dvd.p, dd.p, E.stream());
    std::vector<double> full(stride);
    std::vector<float> stored(stride);
    (void)hipStreamSynchronize(E.stream());
    if (!dvd.get(full.data()) || hipMemcpy(stored.data(), B.f, stride * 4, hipMemcpyDeviceToHost) != hipSuccess) return done(E, false);
    std::copy(full.begin(), full.begin() + n, vd);
    for (int i = 0; i < n; ++i) v[i] = (double)stored[i];
    for (size_t i = (size_t)n; i < stride; ++i) tail[i - (size_t)n] = (double)stored[i];
    *ntail = (int)(stride - (size_t)n);
    return done(E, true);
}

int sparsh_op_gmres_small(sparsh_handle h, int m, int nblk, const double *hcol, const double *ccol, const double *ww_partial, double beta,
                          int k, double *hist, double *R, double *cs, double *sn, double *g, double *ny)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (m < 1 || m > kGmresMaxRestart) return fail(SPARSH_EINVAL, "m must be in 1.." + std::to_string(kGmresMaxRestart));
    if (nblk < 1) return fail(SPARSH_EINVAL, "nblk < 1");
    if (k < 0 || k > m) return fail(SPARSH_EINVAL, "k must be in 0..m");
    if (!hcol || !ccol || !ww_partial || !hist || !R || !cs || !sn || !g || !ny) return fail(SPARSH_EINVAL, "null array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    const size_t tri = (size_t)m * (m + 1) / 2;
    DBuf dh(E, tri, hcol), dc(E, tri, ccol), dww(E, (size_t)m * nblk, ww_partial), dbeta(E, 1, &beta), dhist(E, (size_t)m);
    GmresState s;  // freshly zeroed, carved as the solver's
    DBuf state(E, s);
    if (!state.p || !dh.p || !dc.p || !dww.p || !dbeta.p || !dhist.p) return fail(SPARSH_ENODEV, "device allocation failed");
    hipStream_t st = E.stream();
    size_t off = 0;
    for (int j = 0; j < m; off += (size_t)j + 1, ++j) {  // the columns arrive as the finalize kernels leave them: j + 1 entries each
        E.note_hip(hipMemcpyAsync(s.hcol, dh.p + off, ((size_t)j + 1) * 8, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
        E.note_hip(hipMemcpyAsync(s.ccol, dc.p + off, ((size_t)j + 1) * 8, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
        launch_gmres_step(j, dww.p + (size_t)j * nblk, nblk, s, dbeta.p, dhist.p, j, st);
    }
    launch_gmres_solve(k, s, st);
    std::vector<double> all((size_t)kGmresStateDoubles);
    if (!state.get(all.data()) || !dhist.get(hist)) return done(E, false);
    auto take = [&](const double *dev, size_t count, double *dst) { std::copy(all.begin() + (dev - state.p), all.begin() + (dev - state.p) + count, dst); };
    take(s.R, (size_t)kGmresMaxRestart * kGmresMaxRestart, R);
    take(s.cs, kGmresMaxRestart, cs);
    take(s.sn, kGmresMaxRestart, sn);
    take(s.g, kGmresMaxRestart + 1, g);
    take(s.ny, kGmresMaxRestart, ny);
    return done(E, true);
}

int sparsh_bench_op(sparsh_handle h, int op, int level, int reps, double *avg_seconds)
{
    REQUIRE_READY(h);
    REQUIRE_LEVEL(h, level);
    if (reps <= 0 || !avg_seconds) return fail(SPARSH_EINVAL, "bad reps");
    Engine &E = *h->eng;
    const DevLevel &L = E.level(level);
    const size_t n = (size_t)L.n;
    const bool has_coarse = level + 1 < E.nlevels();
    if ((op == 3 || op == 4) && !has_coarse) return fail(SPARSH_EINVAL, "no coarser level");
    const size_t nc = has_coarse ? (size_t)E.level(level + 1).n : 1;
    // multi-GPU: operator inputs carry the halo behind the own entries
    const size_t xh = (size_t)std::max(L.planA.nhalo, L.planR.nhalo), ch = (size_t)L.planP.nhalo;
    DBuf x(E, n + xh), y(E, n), b(E, n), c(E, nc + ch);
    std::vector<double> ones(std::max(n, nc), 1.0);
    (void)hipMemcpy(x.p, ones.data(), n * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(b.p, ones.data(), n * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(y.p, ones.data(), n * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(c.p, ones.data(), nc * 8, hipMemcpyHostToDevice);
    hipStream_t st = E.stream();
    std::unique_ptr<DBuf> ns_part;  // op 18: the partial sums of launch_sum
    auto run = [&]() {
        switch (op) {
        case 0: E.op_spmv(level, x.p, y.p); break;
        case 1: {
            CsrArgs a;
            a.x = x.p;
            a.b = b.p;
            a.d = L.diag;
            a.y = y.p;
            a.omega = E.params().omega;
            launch_csr(L.A, OP_JACOBI, a, L.fine, st, E.kernel_cfg());
        } break;
        case 2: E.op_residual(level, b.p, x.p, y.p); break;
        case 3: E.op_restrict(level, x.p, c.p); break;
        case 4: E.op_prolong(level, c.p, y.p); break;
        case 5: E.op_coarse(E.level(E.nlevels() - 1).b ? E.level(E.nlevels() - 1).b : b.p, E.level(E.nlevels() - 1).r); break;
        case 6: {
            int nb = 0;
            launch_dot((int)n, x.p, b.p, E.level(0).r, &nb, st);
        } break;
        case 7: launch_axpby((int)n, 0.5, x.p, 0.5, y.p, st); break;
        case 8: launch_copy_int((int)n, L.A.rowptr, reinterpret_cast<int *>(y.p), st); break;  // n int32: reads 4n, writes 4n
        case 9:    // fused Jacobi sweeps the way a smoothing leg issues them: ping-pong between two vectors
        case 10: { // ... on the level's own resident buffers (x, x2, r as the right-hand side)
            static thread_local int flip = 0;
            double *xa = op == 9 ? x.p : L.x, *xb = op == 9 ? y.p : L.x2;
            CsrArgs a;
            a.x = (flip & 1) ? xb : xa;
            a.y = (flip & 1) ? xa : xb;
            a.b = op == 9 ? b.p : L.r;
            a.d = L.diag;
            a.omega = E.params().omega;
            a.reverse = csr_alternates(L.A, E.kernel_cfg()) && (flip & 1);
            ++flip;
            launch_csr(L.A, OP_JACOBI, a, L.fine, st, E.kernel_cfg());
        } break;
        case 12: E.sor_leg(level, L.r, L.x, 1, false); break;  // one SOR sweep, as a leg issues it
        case 11: {  // double sweeps (sdia_box2_kernel) ping-ponging on the level's resident buffers, as a smoothing leg issues them
            static thread_local int flip2 = 0;
            double *xa = (flip2 & 1) ? L.x2 : L.x, *xb = (flip2 & 1) ? L.x : L.x2;
            ++flip2;
            launch_box2(L.A, xa, L.r, xb, E.params().omega, L.fine, st);
        } break;
        case 16: {  // last post-sweep + dot through the plane-marching kernel (sdia_box1_kernel), same buffers
            static thread_local int flip3 = 0;
            CsrArgs a;
            a.x = (flip3 & 1) ? L.x2 : L.x;
            a.y = (flip3 & 1) ? L.x : L.x2;
            ++flip3;
            a.b = L.r;
            a.d = L.diag;
            a.omega = E.params().omega;
            a.partial = E.partials();
            launch_box1(L.A, 1, a, L.fine, st);
        } break;
        case 17: E.cheby_bench_step(level); break;
        case 18: {  // one projection with the dot (launch_sum + launch_project) on level 0's resident x and r
            int nb = 0;
            E.project_any(L.n, L.x, L.r, ns_part->p, E.partials(), &nb);
        } break;
        case 13: E.gmres_bench_step(true); break;
        case 14: E.gmres_bench_step(false); break;
        case 15: E.gmres_bench_step(true); break;  // (the handle's float basis)
        default: break;
        }
    };
    if (op < 0 || op > 18) return fail(SPARSH_EINVAL, "unknown op");
    if (op == 18) {
        if (level != 0 || E.distributed()) return fail(SPARSH_EINVAL, "the projection runs on level 0 of a single-GPU handle");
        ns_part.reset(new DBuf(E, (size_t)ns_grid(L.n)));
        if (!ns_part->p) return fail(SPARSH_ENODEV, E.error);
        launch_fill(L.n, 1.0, L.x, st);
    }
    if (op == 17 && (E.distributed() || !E.build_cheby_level(level))) return fail(SPARSH_ESTATE, "no Chebyshev bounds on this handle");
    if (op == 13 || op == 14 || op == 15) {
        if (level != 0 || E.distributed()) return fail(SPARSH_EINVAL, "the GMRES orthogonalisation step runs on level 0 of a single-GPU handle");
        if ((op == 15) != (E.gmres_basis() == SPARSH_BASIS_FP32))
            return fail(SPARSH_ESTATE, "ops 13 and 14 run on a double basis, op 15 on a float basis (sparsh_set_gmres_basis)");
        if (int rc = E.gmres_bench_prepare(); rc != SPARSH_OK) return fail(rc, E.error);
    }
    if (op == 12 && (E.distributed() || !E.build_sor_level(level))) return fail(SPARSH_ESTATE, "no SOR layout on this handle");
    if (op == 11 && (E.distributed() || !box2_applies(L.A, E.kernel_cfg()))) return fail(SPARSH_ESTATE, "the level does not run double sweeps (sparsh_level_double_sweep)");
    if (op == 16 && (E.distributed() || !box1_applies(L.A, E.kernel_cfg()))) return fail(SPARSH_ESTATE, "the level does not run the plane-marching kernel (sparsh_level_marching_ops)");
    // (the ops on the level's own buffers, 10, 11 and 16: ones as the right-hand side, as in Engine::tune_box_kernels -- on zeros every quotient
    // of div_const takes the plain-division branch)
    if (op == 10 || op == 11 || op == 16 || op == 17 || op == 18) launch_fill(L.n, 1.0, L.r, st);
    for (int i = 0; i < 3; ++i) run();
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, st);
    for (int i = 0; i < reps; ++i) run();
    (void)hipEventRecord(e1, st);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (op == 10 || op == 11 || op == 16 || op == 17 || op == 18) {
        (void)hipMemsetAsync(L.x, 0, n * 8, st);
        (void)hipMemsetAsync(L.x2, 0, n * 8, st);
        (void)hipMemsetAsync(L.r, 0, n * 8, st);
    }
    *avg_seconds = ms * 1e-3 / reps;
    return SPARSH_OK;
}

int sparsh_dev_alloc(sparsh_handle h, long nbytes, void **out)
{
    if (!h || !h->eng || !out || nbytes < 0) return fail(SPARSH_EINVAL, "bad arguments");
    *out = h->eng->dalloc((size_t)nbytes);
    return *out ? SPARSH_OK : fail(SPARSH_ENODEV, h->eng->error);
}

int sparsh_dev_free(sparsh_handle h, void *p)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    h->eng->dfree(p);
    return SPARSH_OK;
}

int sparsh_dev_fill(sparsh_handle h, double *dst_dev, long n, double value)
{
    if (!h || !h->eng || !h->eng->stream()) return fail(SPARSH_EINVAL, "null handle or no stream (call sparsh_setup first)");
    if (n < 0 || n > 0x7fffffffL) return fail(SPARSH_EINVAL, "bad length");
    launch_fill((int)n, value, dst_dev, h->eng->stream());
    return SPARSH_OK;
}

int sparsh_h2d(sparsh_handle h, void *dst_dev, const void *src, long nbytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (hipMemcpy(dst_dev, src, (size_t)nbytes, hipMemcpyHostToDevice) != hipSuccess) return fail(SPARSH_ENODEV, "H2D failed");
    return SPARSH_OK;
}

int sparsh_d2h(sparsh_handle h, void *dst, const void *src_dev, long nbytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (h->eng->stream()) (void)hipStreamSynchronize(h->eng->stream());
    if (hipMemcpy(dst, src_dev, (size_t)nbytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(SPARSH_ENODEV, "D2H failed");
    return SPARSH_OK;
}

int sparsh_sync(sparsh_handle h)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (h->eng->stream() && hipStreamSynchronize(h->eng->stream()) != hipSuccess) return fail(SPARSH_ENODEV, "sync failed");
    return SPARSH_OK;
}

int sparsh_profile(sparsh_handle h, int enable)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (enable) {
        h->eng->profile_begin();
        h->eng->prof.enabled = true;
    } else if (h->eng->prof.enabled) {
        h->eng->profile_collect();
        h->eng->prof.enabled = false;
    }
    return SPARSH_OK;
}

int sparsh_profile_read(sparsh_handle h, double *out4)
{
    REQUIRE_READY(h);
    out4[0] = h->eng->prof.launches;
    out4[1] = h->eng->prof.seconds;
    out4[2] = h->eng->level(0).n;
    out4[3] = h->eng->level(0).A.nnz;
    return SPARSH_OK;
}

// ---- block of up to SPARSH_MAX_RHS right-hand sides ----

// bad arguments and handles no setup can make fit are SPARSH_EINVAL with or without a device, so they are checked before readiness
#define REQUIRE_MULTI_ARGS(h, nrhs)                                                                               \
    if (!(h) || !(h)->eng) return fail(SPARSH_EINVAL, "null handle");                                             \
    if ((nrhs) < 1 || (nrhs) > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "nrhs must be 1 .. SPARSH_MAX_RHS (8)")

#define REQUIRE_MULTI_FITS(h) \
    if (const char *why_ = (h)->eng->multi_refusal()) return fail(SPARSH_EINVAL, why_)

}  // extern "C"

namespace {

int block_solve(Engine &E, int method, int nrhs, const double *B, long ldb, double *X, long ldx, int max_iters, double *hist, int hist_cap,
                int *iters, int *status, double *seconds)
{
    if (method == SPARSH_BCG) return E.solve_bcg_dev(nrhs, B, ldb, X, ldx, max_iters, hist, hist_cap, iters, status, seconds);
    if (method == SPARSH_MBICG) return E.solve_mbicg_dev(nrhs, B, ldb, X, ldx, max_iters, hist, hist_cap, iters, status, seconds);
    return E.solve_multi_dev(nrhs, B, ldb, X, ldx, max_iters, hist, hist_cap, iters, status, seconds);
}

}  // namespace

extern "C" {

int sparsh_solve_multi_dev(sparsh_handle h, int method, int nrhs, const double *B_dev, long ldb, double *X_dev, long ldx, int max_iters,
                           double *hist, int hist_cap, int *iters, int *status, double *seconds)
{
    REQUIRE_MULTI_ARGS(h, nrhs);
    if (method != SPARSH_PCG && method != SPARSH_BCG && method != SPARSH_MBICG)
        return fail(SPARSH_EINVAL, "block solves take SPARSH_PCG, SPARSH_BCG or SPARSH_MBICG only");
    if (!B_dev || !X_dev || !iters || !status || (hist_cap > 0 && !hist)) return fail(SPARSH_EINVAL, "NULL array");
    if (hist_cap < 0) return fail(SPARSH_EINVAL, "hist_cap < 0");
    if (ldb < h->eng->n0() || ldx < h->eng->n0()) return fail(SPARSH_EINVAL, "ldb and ldx must be at least the number of rows");
    REQUIRE_MULTI_FITS(h);
    REQUIRE_READY(h);
    int rc = block_solve(*h->eng, method, nrhs, B_dev, ldb, X_dev, ldx, max_iters, hist, hist_cap, iters, status, seconds);
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

int sparsh_solve_multi(sparsh_handle h, int method, int nrhs, const double *B, long ldb, double *X, long ldx, double *hist, int hist_cap,
                       int *iters, int *status)
{
    REQUIRE_MULTI_ARGS(h, nrhs);
    if (method != SPARSH_PCG && method != SPARSH_BCG && method != SPARSH_MBICG)
        return fail(SPARSH_EINVAL, "block solves take SPARSH_PCG, SPARSH_BCG or SPARSH_MBICG only");
    if (!B || !X || !iters || !status || (hist_cap > 0 && !hist)) return fail(SPARSH_EINVAL, "NULL array");
    if (hist_cap < 0) return fail(SPARSH_EINVAL, "hist_cap < 0");
    if (ldb < h->eng->n0() || ldx < h->eng->n0()) return fail(SPARSH_EINVAL, "ldb and ldx must be at least the number of rows");
    REQUIRE_MULTI_FITS(h);
    REQUIRE_READY(h);
    Engine &E = *h->eng;
    const size_t n = (size_t)E.n0();
    // the device copies are packed (leading dimension n): only the n rows of every column travel
    DBuf db(E, n * nrhs), dx(E, n * nrhs);
    if (!db.p || !dx.p) return fail(SPARSH_ENODEV, E.error);
    for (int c = 0; c < nrhs; ++c) {
        (void)hipMemcpy(db.p + (size_t)c * n, B + (size_t)c * ldb, n * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(dx.p + (size_t)c * n, X + (size_t)c * ldx, n * 8, hipMemcpyHostToDevice);
    }
    int rc = block_solve(E, method, nrhs, db.p, (long)n, dx.p, (long)n, 0, hist, hist_cap, iters, status, nullptr);
    (void)hipStreamSynchronize(E.stream());
    for (int c = 0; c < nrhs; ++c) (void)hipMemcpy(X + (size_t)c * ldx, dx.p + (size_t)c * n, n * 8, hipMemcpyDeviceToHost);
    if (rc != SPARSH_OK) return fail(rc, E.error);
    return rc;
}

int sparsh_multi_info(sparsh_handle h, int *width, long *bytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (width) *width = h->eng->multi_width_now();
    if (bytes) *bytes = (long)h->eng->multi_bytes();
    return SPARSH_OK;
}

namespace {

// the operator hooks: column-major host blocks in (b: rows_b x nrhs, x: rows_x x nrhs; either may be absent) and out (rows_y x nrhs;
// y_in: the output block is also an input)
int op_multi_host(sparsh_handle h, int which, int level, int nrhs, const double *b, const double *x, double *y, bool y_in, double *dots,
                  int sweeps, bool x_is_zero)
{
    Engine &E = *h->eng;
    const int last = E.nlevels() - 1;
    const int l = which == 5 ? last : (which == 6 ? 0 : level);
    if ((which == 3 || which == 4) && l >= last) return fail(SPARSH_EINVAL, "no coarser level");
    const size_t n = (size_t)E.level(l).n, nc = l < last ? (size_t)E.level(l + 1).n : 0;
    const size_t rows_x = which == 4 ? nc : n, rows_y = which == 3 ? nc : n;
    DBuf db(E, std::max<size_t>(n * nrhs, 1), nullptr), dx(E, std::max<size_t>(rows_x * nrhs, 1), nullptr), dy(E, rows_y * nrhs, y_in ? y : nullptr);
    if (!db.p || !dx.p || !dy.p) return fail(SPARSH_ENODEV, E.error);
    if (b) (void)hipMemcpy(db.p, b, n * nrhs * 8, hipMemcpyHostToDevice);
    if (x) (void)hipMemcpy(dx.p, x, rows_x * nrhs * 8, hipMemcpyHostToDevice);
    if (int rc = E.op_multi(which, l, nrhs, b ? db.p : nullptr, x ? dx.p : nullptr, dy.p, dots, sweeps, x_is_zero); rc != SPARSH_OK)
        return fail(rc, E.error);
    return done(E, dy.get(y));
}

}  // namespace

#define REQUIRE_MULTI_OP(h, nrhs)  \
    REQUIRE_MULTI_ARGS(h, nrhs);   \
    REQUIRE_READY(h);              \
    REQUIRE_SINGLE(h)

int sparsh_op_spmv_dot_multi(sparsh_handle h, int level, int nrhs, const double *X, double *Y, double *dots)
{
    REQUIRE_MULTI_OP(h, nrhs);
    REQUIRE_LEVEL(h, level);
    if (!X || !Y || !dots) return fail(SPARSH_EINVAL, "NULL array");
    return op_multi_host(h, 0, level, nrhs, nullptr, X, Y, false, dots, 0, false);
}

int sparsh_op_residual_multi(sparsh_handle h, int level, int nrhs, const double *B, const double *X, double *R)
{
    REQUIRE_MULTI_OP(h, nrhs);
    REQUIRE_LEVEL(h, level);
    if (!B || !X || !R) return fail(SPARSH_EINVAL, "NULL array");
    return op_multi_host(h, 1, level, nrhs, B, X, R, false, nullptr, 0, false);
}

int sparsh_op_jacobi_multi(sparsh_handle h, int level, int nrhs, const double *B, double *X, int sweeps, int x_is_zero)
{
    REQUIRE_MULTI_OP(h, nrhs);
    REQUIRE_LEVEL(h, level);
    if (!B || !X) return fail(SPARSH_EINVAL, "NULL array");
    if (sweeps < 0) return fail(SPARSH_EINVAL, "sweeps < 0");
    return op_multi_host(h, 2, level, nrhs, B, x_is_zero ? nullptr : X, X, false, nullptr, sweeps, x_is_zero != 0);
}

int sparsh_op_restrict_multi(sparsh_handle h, int level, int nrhs, const double *R, double *BC)
{
    REQUIRE_MULTI_OP(h, nrhs);
    REQUIRE_LEVEL(h, level);
    if (!R || !BC) return fail(SPARSH_EINVAL, "NULL array");
    return op_multi_host(h, 3, level, nrhs, nullptr, R, BC, false, nullptr, 0, false);
}

int sparsh_op_prolong_multi(sparsh_handle h, int level, int nrhs, const double *XC, double *XF)
{
    REQUIRE_MULTI_OP(h, nrhs);
    REQUIRE_LEVEL(h, level);
    if (!XC || !XF) return fail(SPARSH_EINVAL, "NULL array");
    return op_multi_host(h, 4, level, nrhs, nullptr, XC, XF, true, nullptr, 0, false);
}

int sparsh_op_coarse_multi(sparsh_handle h, int nrhs, const double *B, double *X)
{
    REQUIRE_MULTI_OP(h, nrhs);
    if (!B || !X) return fail(SPARSH_EINVAL, "NULL array");
    return op_multi_host(h, 5, 0, nrhs, B, nullptr, X, false, nullptr, 0, false);
}

int sparsh_op_precond_multi(sparsh_handle h, int nrhs, const double *R, double *Z)
{
    REQUIRE_MULTI_ARGS(h, nrhs);
    if (!R || !Z) return fail(SPARSH_EINVAL, "NULL array");
    REQUIRE_MULTI_FITS(h);
    REQUIRE_READY(h);
    return op_multi_host(h, 6, 0, nrhs, R, nullptr, Z, false, nullptr, 0, false);
}

int sparsh_bench_op_multi(sparsh_handle h, int op, int level, int nrhs, int reps, double *avg_seconds)
{
    REQUIRE_MULTI_ARGS(h, nrhs);
    if (op < 0 || op > 9 || op == 6) return fail(SPARSH_EINVAL, "unknown op");  // (6 is not assigned)
    if (reps <= 0 || !avg_seconds) return fail(SPARSH_EINVAL, "bad reps");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    REQUIRE_LEVEL(h, level);
    Engine &E = *h->eng;
    const bool con = op == 7;  // the projection of the constrained eigensolver: only on what a constrained solve has left resident
    const bool eig = op >= 2;  // the eigensolver's launches run on its own resident blocks (level 0)
    const bool ortho = op >= 8;        // 8, 9: the transform and the masked subtraction of the ortho basis, on the generalised solver's blocks
    const bool gen = op >= 4 && !con;  // 4, 5, 8, 9: the generalised solver's blocks beside them, and its B
    if (gen && !E.eig_b_set()) return fail(SPARSH_ESTATE, "sparsh_eig_set_b has not been called");
    if (ortho && E.eig_basis() != SPARSH_EIG_BASIS_ORTHO) return fail(SPARSH_ESTATE, "sparsh_set_eig_options has not selected SPARSH_EIG_BASIS_ORTHO");
    if (con) {
        if (E.eig_con_total() == 0 || E.eig_width_now() != multi_width(nrhs))
            return fail(SPARSH_ESTATE, "no constrained eigen solve of this width has reserved the constraint blocks");
    } else if (int rc = gen ? E.eig_reserve_gen(nrhs) : (eig ? E.eig_reserve(nrhs) : E.multi_reserve(nrhs)); rc != SPARSH_OK) {
        return fail(rc, E.error);
    }
    if (ortho)
        if (int rc = E.eig_ortho_reserve(); rc != SPARSH_OK) return fail(rc, E.error);
    hipStream_t st = E.stream();
    auto launch = [&]() {
        if (ortho) return E.bench_eig_ortho_launch(op);
        return con ? E.bench_eig_con_launch() : (eig ? E.bench_eig_launch(op) : E.bench_multi_launch(op, level));
    };
    for (int i = 0; i < 3; ++i) launch();
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, st);
    for (int i = 0; i < reps; ++i) launch();
    (void)hipEventRecord(e1, st);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_seconds = ms * 1e-3 / reps;
    return done(E, true);
}

// ---- lowest eigenpairs by LOBPCG on the block path ----

// like REQUIRE_MULTI_ARGS: what no setup can make valid is SPARSH_EINVAL with or without a device
#define REQUIRE_EIG_ARGS(h, nev, X, ldx, tol, lambda, hist, hist_cap, iters, status)                                          \
    if (!(h) || !(h)->eng) return fail(SPARSH_EINVAL, "null handle");                                                         \
    if ((nev) < 1 || (nev) > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "nev must be 1 .. SPARSH_MAX_RHS (8)");                 \
    if ((nev) > (h)->eng->n0()) return fail(SPARSH_EINVAL, "nev exceeds the number of rows");                                  \
    if ((h)->eng->eig_wanted() > (nev)) return fail(SPARSH_EINVAL, "wanted (sparsh_set_eig_options) exceeds nev"); \
    if (!(X) || !(lambda) || !(iters) || !(status) || ((hist_cap) > 0 && !(hist))) return fail(SPARSH_EINVAL, "NULL array"); \
    if ((hist_cap) < 0) return fail(SPARSH_EINVAL, "hist_cap < 0");                                                           \
    if ((ldx) < (h)->eng->n0()) return fail(SPARSH_EINVAL, "ldx must be at least the number of rows");                         \
    if (!std::isfinite(tol) || !((tol) > 0.0)) return fail(SPARSH_EINVAL, "tol must be finite and positive");                 \
    REQUIRE_MULTI_FITS(h)

int sparsh_eigs_dev(sparsh_handle h, int nev, double *X_dev, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap,
                    int *iters, int *status, double *seconds)
{
    REQUIRE_EIG_ARGS(h, nev, X_dev, ldx, tol, lambda, hist, hist_cap, iters, status);
    REQUIRE_READY(h);
    int rc = h->eng->eigs_dev(nev, X_dev, ldx, tol, max_iters, lambda, hist, hist_cap, iters, status, seconds);
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

namespace {

// sparsh_eigs and sparsh_eigs_gen on host arrays
int eigs_host(sparsh_handle h, bool gen, int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap,
              int *iters, int *status)
{
    REQUIRE_EIG_ARGS(h, nev, X, ldx, tol, lambda, hist, hist_cap, iters, status);
    REQUIRE_READY(h);
    Engine &E = *h->eng;
    if (gen && !E.eig_b_set()) return fail(SPARSH_ESTATE, "sparsh_eig_set_b has not been called: the generalised problem needs its B");
    const size_t n = (size_t)E.n0();
    DBuf dx(E, n * nev);  // packed (leading dimension n): only the n rows of every column travel
    if (!dx.p) return fail(SPARSH_ENODEV, E.error);
    for (int c = 0; c < nev; ++c) (void)hipMemcpy(dx.p + (size_t)c * n, X + (size_t)c * ldx, n * 8, hipMemcpyHostToDevice);
    int rc = gen ? E.eigs_gen_dev(nev, dx.p, (long)n, tol, max_iters, lambda, hist, hist_cap, iters, status, nullptr)
                 : E.eigs_dev(nev, dx.p, (long)n, tol, max_iters, lambda, hist, hist_cap, iters, status, nullptr);
    (void)hipStreamSynchronize(E.stream());
    if (rc == SPARSH_OK || rc == SPARSH_ENOCONV)
        for (int c = 0; c < nev; ++c) (void)hipMemcpy(X + (size_t)c * ldx, dx.p + (size_t)c * n, n * 8, hipMemcpyDeviceToHost);
    if (rc != SPARSH_OK) return fail(rc, E.error);
    return rc;
}

}  // namespace

int sparsh_eigs(sparsh_handle h, int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap,
                int *iters, int *status)
{
    return eigs_host(h, false, nev, X, ldx, tol, max_iters, lambda, hist, hist_cap, iters, status);
}

// ---- the generalised problem A x = lambda B x ----

namespace {

// what sparsh_eig_set_b refuses in B itself (nullptr: nothing); host only
const char *eig_b_defect(int n, const int *rp, const int *ci, const double *v)
{
    if (rp[0] != 0) return "B: rowptr[0] must be 0";
    for (int i = 0; i < n; ++i)
        if (rp[i + 1] < rp[i]) return "B: rowptr must be non-decreasing";
    double vmax = 0.0;
    for (int i = 0; i < n; ++i) {
        bool diag = false;
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            if (ci[p] < 0 || ci[p] >= n) return "B: column index out of range";
            if (p > rp[i] && ci[p] <= ci[p - 1]) return "B: the columns of a row must be strictly ascending";
            if (!std::isfinite(v[p])) return "B: a value is not finite";
            vmax = std::max(vmax, std::fabs(v[p]));
            if (ci[p] == i) {
                diag = true;
                if (!(v[p] > 0.0)) return "B: a diagonal entry is not positive";
            }
        }
        if (!diag) return "B: a row has no stored diagonal entry";
    }
    const double bound = 1e-12 * vmax;
    for (int i = 0; i < n; ++i)
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            const int j = ci[p];
            if (j == i) continue;
            const int *lo = ci + rp[j], *hi = ci + rp[j + 1];
            const int *q = std::lower_bound(lo, hi, i);
            const double t = (q != hi && *q == i) ? v[q - ci] : 0.0;  // a missing transpose entry counts as 0
            if (std::fabs(v[p] - t) > bound) return "B is not symmetric: some |b_ij - b_ji| > 1e-12 max|b|";
        }
    return nullptr;
}

}  // namespace

namespace {

// sparsh_eig_set_b and sparsh_eig_con_set_b: con lets a null-space handle through
int eig_set_b_checked(sparsh_handle h, const int *rowptr, const int *colindex, const double *val, bool con)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    Engine &E = *h->eng;
    if (!rowptr) {  // drop B: nothing to check, and nothing to drop before a setup
        if (E.eig_b_set()) (void)E.eig_set_b(nullptr, nullptr, nullptr);
        return SPARSH_OK;
    }
    if (!colindex || !val) return fail(SPARSH_EINVAL, "B: NULL colindex or val with a rowptr");
    if (const char *why = eig_b_defect(E.n0(), rowptr, colindex, val)) return fail(SPARSH_EINVAL, why);
    if (const char *why = con ? E.eig_con_refusal() : E.multi_refusal()) return fail(SPARSH_EINVAL, why);
    REQUIRE_READY(h);
    if (int rc = E.eig_set_b(rowptr, colindex, val); rc != SPARSH_OK) return fail(rc, E.error);
    return SPARSH_OK;
}

}  // namespace

int sparsh_eig_set_b(sparsh_handle h, const int *rowptr, const int *colindex, const double *val)
{
    return eig_set_b_checked(h, rowptr, colindex, val, false);
}

int sparsh_eig_con_set_b(sparsh_handle h, const int *rowptr, const int *colindex, const double *val)
{
    return eig_set_b_checked(h, rowptr, colindex, val, true);
}

int sparsh_eig_b_info(sparsh_handle h, int *is_set, long *nnz, long *bytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (is_set) *is_set = h->eng->eig_b_set() ? 1 : 0;
    if (nnz) *nnz = h->eng->eig_b_nnz();
    if (bytes) *bytes = (long)h->eng->eig_b_bytes();
    return SPARSH_OK;
}

int sparsh_eigs_gen_dev(sparsh_handle h, int nev, double *X_dev, long ldx, double tol, int max_iters, double *lambda, double *hist,
                        int hist_cap, int *iters, int *status, double *seconds)
{
    REQUIRE_EIG_ARGS(h, nev, X_dev, ldx, tol, lambda, hist, hist_cap, iters, status);
    REQUIRE_READY(h);
    int rc = h->eng->eigs_gen_dev(nev, X_dev, ldx, tol, max_iters, lambda, hist, hist_cap, iters, status, seconds);
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

int sparsh_eigs_gen(sparsh_handle h, int nev, double *X, long ldx, double tol, int max_iters, double *lambda, double *hist, int hist_cap,
                    int *iters, int *status)
{
    return eigs_host(h, true, nev, X, ldx, tol, max_iters, lambda, hist, hist_cap, iters, status);
}

int sparsh_eig_info(sparsh_handle h, int *width, long *bytes, int *restarts)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (width) *width = h->eng->eig_width_now();
    if (bytes) *bytes = (long)h->eng->eig_bytes();
    if (restarts) *restarts = h->eng->eig_restarts();
    return SPARSH_OK;
}

// ---- eigenpairs under constraints ----

// REQUIRE_EIG_ARGS with a null-space handle let through (it gets the constant vector as one more constraint), then the constraints
#define REQUIRE_EIG_CON_ARGS(h, gen, nev, X, ldx, ncon, Y, ldy, tol, lambda, hist, hist_cap, iters, status)                               \
    if (!(h) || !(h)->eng) return fail(SPARSH_EINVAL, "null handle");                                                                  \
    if ((nev) < 1 || (nev) > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "nev must be 1 .. SPARSH_MAX_RHS (8)");                          \
    if ((nev) > (h)->eng->n0()) return fail(SPARSH_EINVAL, "nev exceeds the number of rows");                                           \
    if ((h)->eng->eig_wanted() > (nev)) return fail(SPARSH_EINVAL, "wanted (sparsh_set_eig_options) exceeds nev"); \
    if (!(X) || !(lambda) || !(iters) || !(status) || ((hist_cap) > 0 && !(hist))) return fail(SPARSH_EINVAL, "NULL array");          \
    if ((hist_cap) < 0) return fail(SPARSH_EINVAL, "hist_cap < 0");                                                                    \
    if ((ldx) < (h)->eng->n0()) return fail(SPARSH_EINVAL, "ldx must be at least the number of rows");                                  \
    if (!std::isfinite(tol) || !((tol) > 0.0)) return fail(SPARSH_EINVAL, "tol must be finite and positive");                          \
    if (const char *why_ = (h)->eng->eig_con_refusal()) return fail(SPARSH_EINVAL, why_);                                              \
    if ((gen) != 0 && (gen) != 1) return fail(SPARSH_EINVAL, "gen must be 0 (A x = lambda x) or 1 (A x = lambda B x)");                \
    if ((ncon) < 0 || (ncon) > SPARSH_MAX_CON) return fail(SPARSH_EINVAL, "ncon must be 0 .. SPARSH_MAX_CON (16)");                     \
    if ((ncon) > 0 && !(Y)) return fail(SPARSH_EINVAL, "NULL array: Y with ncon > 0");                                                 \
    if ((ncon) > 0 && (ldy) < (h)->eng->n0()) return fail(SPARSH_EINVAL, "ldy must be at least the number of rows");                    \
    if ((nev) + (ncon) + ((h)->eng->ns_on() ? 1 : 0) > (h)->eng->n0())                                                                 \
    return fail(SPARSH_EINVAL, "nev and the constraints (the constant vector of a null-space handle included) exceed the number of rows")

int sparsh_eigs_con_dev(sparsh_handle h, int gen, int nev, double *X_dev, long ldx, int ncon, const double *Y_dev, long ldy, double tol,
                        int max_iters, double *lambda, double *hist, int hist_cap, int *iters, int *status, double *seconds)
{
    REQUIRE_EIG_CON_ARGS(h, gen, nev, X_dev, ldx, ncon, Y_dev, ldy, tol, lambda, hist, hist_cap, iters, status);
    REQUIRE_READY(h);
    int rc = h->eng->eigs_con_dev(gen != 0, nev, X_dev, ldx, ncon, Y_dev, ldy, tol, max_iters, lambda, hist, hist_cap, iters, status, seconds);
    if (rc != SPARSH_OK) return fail(rc, h->eng->error);
    return rc;
}

int sparsh_eigs_con(sparsh_handle h, int gen, int nev, double *X, long ldx, int ncon, const double *Y, long ldy, double tol, int max_iters,
                    double *lambda, double *hist, int hist_cap, int *iters, int *status)
{
    REQUIRE_EIG_CON_ARGS(h, gen, nev, X, ldx, ncon, Y, ldy, tol, lambda, hist, hist_cap, iters, status);
    REQUIRE_READY(h);
    Engine &E = *h->eng;
    if (gen && !E.eig_b_set()) return fail(SPARSH_ESTATE, "sparsh_eig_set_b has not been called: the generalised problem needs its B");
    const size_t n = (size_t)E.n0();
    DBuf dx(E, n * nev), dy(E, n * std::max(ncon, 1));  // packed (leading dimension n)
    if (!dx.p || !dy.p) return fail(SPARSH_ENODEV, E.error);
    for (int c = 0; c < nev; ++c) (void)hipMemcpy(dx.p + (size_t)c * n, X + (size_t)c * ldx, n * 8, hipMemcpyHostToDevice);
    for (int c = 0; c < ncon; ++c) (void)hipMemcpy(dy.p + (size_t)c * n, Y + (size_t)c * ldy, n * 8, hipMemcpyHostToDevice);
    int rc = E.eigs_con_dev(gen != 0, nev, dx.p, (long)n, ncon, ncon > 0 ? dy.p : nullptr, (long)n, tol, max_iters, lambda, hist, hist_cap, iters,
                            status, nullptr);
    (void)hipStreamSynchronize(E.stream());
    if (rc == SPARSH_OK || rc == SPARSH_ENOCONV)
        for (int c = 0; c < nev; ++c) (void)hipMemcpy(X + (size_t)c * ldx, dx.p + (size_t)c * n, n * 8, hipMemcpyDeviceToHost);
    if (rc != SPARSH_OK) return fail(rc, E.error);
    return rc;
}

int sparsh_eig_con_info(sparsh_handle h, int *ncon_total, int *implicit_constant, long *bytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    const int mt = h->eng->eig_con_total();
    if (ncon_total) *ncon_total = mt;
    if (implicit_constant) *implicit_constant = (mt > 0 && h->eng->ns_on()) ? 1 : 0;
    if (bytes) *bytes = (long)h->eng->eig_con_bytes();
    return SPARSH_OK;
}

int sparsh_op_eig_con_project(sparsh_handle h, int n, int k, int m, const double *Y, const double *BY, const double *Ginv, const double *V,
                              double *Vout, double *C)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (n <= 0) return fail(SPARSH_EINVAL, "n <= 0");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (m < 1 || m > kEigConMax) return fail(SPARSH_EINVAL, "m must be 1 .. 17");
    if (!Y || !BY || !Ginv || !V || !Vout || !C) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int W = multi_width(k), nblk = (m + W - 1) / W;
    const size_t len = (size_t)n * W;
    DBuf stage(E, (size_t)n * W), by(E, len * nblk), bby(E, len * nblk), bv(E, len), bo(E, len), dg(E, (size_t)m * m, Ginv),
        dc(E, (size_t)nblk * W * W), part(E, (size_t)nblk * W * W * eig_grid(n, W));
    if (!stage.p || !by.p || !bby.p || !bv.p || !bo.p || !dg.p || !dc.p || !part.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    bool ok = true;
    auto put = [&](const double *src, int first, int cols, double *blk) {  // columns first .. first + cols - 1 of a host array -> a block
        ok = ok && hipMemcpy(stage.p, src + (size_t)first * n, (size_t)n * cols * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) launch_interleave(n, cols, W, stage.p, n, blk, E.stream());
        ok = ok && hipStreamSynchronize(E.stream()) == hipSuccess;
    };
    for (int b = 0; b < nblk; ++b) {
        put(Y, b * W, std::min(W, m - b * W), by.p + b * len);
        put(BY, b * W, std::min(W, m - b * W), bby.p + b * len);
    }
    put(V, 0, k, bv.p);
    if (!ok) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    double *dst = Vout == V ? bv.p : bo.p;  // V == Vout on the host: in place on the device too
    launch_eig_con_project(n, W, m, by.p, bby.p, dg.p, bv.p, dst, dc.p, part.p, E.stream());
    // the padding columns of the block that comes back must still hold zeros (a lane stores both columns of its pair, so they cannot
    // carry a sentinel through the launch)
    std::vector<double> full(len), cfull((size_t)nblk * W * W);
    (void)hipStreamSynchronize(E.stream());
    ok = hipMemcpy(full.data(), dst, len * 8, hipMemcpyDeviceToHost) == hipSuccess && dc.get(cfull.data());
    if (!ok) return done(E, false);
    for (size_t i = 0; i < (size_t)n; ++i) {
        for (int c = 0; c < k; ++c) Vout[(size_t)c * n + i] = full[i * W + c];
        for (int c = k; c < W; ++c)
            if (full[i * W + c] != 0.0) return fail(SPARSH_ENUMERIC, "a padding column of the projected block is not zero");
    }
    for (int j = 0; j < m; ++j)
        for (int c = 0; c < k; ++c) C[j * k + c] = cfull[(size_t)j * W + c];
    return done(E, true);
}

int sparsh_debug_eig_small(int m, int k, const double *GA, const double *GB, double *theta, double *C)
{
    if (m < 1 || m > kEigSmallMax || k < 1 || k > m || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "m must be 1 .. 24 and k 1 .. min(m, 8)");
    if (!GA || !GB || !theta || !C) return fail(SPARSH_EINVAL, "NULL array");
    return eig_small(m, k, GA, GB, theta, C);
}

// ---- operator-level hooks of the eigensolver's kernels (eig_kernels.hip): the handle lends its stream and allocator only

#define REQUIRE_EIG_OP(h, n)                                          \
    if (!(h) || !(h)->eng) return fail(SPARSH_EINVAL, "null handle"); \
    if ((n) <= 0) return fail(SPARSH_EINVAL, "n <= 0");               \
    REQUIRE_READY(h);                                                 \
    REQUIRE_SINGLE(h)

int sparsh_op_gram_multi(sparsh_handle h, int n, int nu, const double *U, int nv, const double *V, double *G)
{
    REQUIRE_EIG_OP(h, n);
    if (nu < 1 || nu > SPARSH_MAX_RHS || nv < 1 || nv > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "nu and nv must be 1 .. SPARSH_MAX_RHS (8)");
    if (!U || !V || !G) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int W = multi_width(std::max(nu, nv));
    const size_t len = (size_t)n * W;
    DBuf du(E, (size_t)n * nu, U), dv(E, (size_t)n * nv, V), bu(E, len), bv(E, len), part(E, (size_t)W * W * eig_grid(n, W)), g(E, (size_t)W * W);
    if (!du.p || !dv.p || !bu.p || !bv.p || !part.p || !g.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_interleave(n, nu, W, du.p, n, bu.p, E.stream());
    launch_interleave(n, nv, W, dv.p, n, bv.p, E.stream());
    GramPairs prs{};
    prs.u[0] = bu.p;
    prs.v[0] = bv.p;
    launch_gram_multi(n, W, 1, prs, part.p, g.p, W, E.stream());
    std::vector<double> full((size_t)W * W);
    if (!g.get(full.data())) return done(E, false);
    for (int a = 0; a < nu; ++a)
        for (int b = 0; b < nv; ++b) G[a * nv + b] = full[(size_t)a * W + b];
    return done(E, true);
}

int sparsh_op_eig_residual(sparsh_handle h, int n, int k, const double *AX, const double *X, const double *theta, double *R, double *norms)
{
    REQUIRE_EIG_OP(h, n);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (!AX || !X || !theta || !R || !norms) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int W = multi_width(k);
    const size_t len = (size_t)n * W;
    std::vector<double> th(W, 0.0);
    std::copy(theta, theta + k, th.begin());
    DBuf dax(E, (size_t)n * k, AX), dx(E, (size_t)n * k, X), bax(E, len), bx(E, len), br(E, len), dth(E, (size_t)W, th.data()),
        part(E, (size_t)W * eig_grid(n, W)), dn(E, (size_t)W), dr(E, (size_t)n * k);
    if (!dax.p || !dx.p || !bax.p || !bx.p || !br.p || !dth.p || !part.p || !dn.p || !dr.p)
        return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_interleave(n, k, W, dax.p, n, bax.p, E.stream());
    launch_interleave(n, k, W, dx.p, n, bx.p, E.stream());
    launch_eig_residual(n, W, bax.p, bx.p, dth.p, br.p, part.p, dn.p, E.stream());
    launch_deinterleave(n, k, W, br.p, dr.p, n, E.stream());
    if (!dr.get(R) || !dn.get(th.data())) return done(E, false);
    std::copy(th.begin(), th.begin() + k, norms);
    return done(E, true);
}

int sparsh_op_eig_update(sparsh_handle h, int n, int k, const double *X, const double *W, const double *P, const double *AX, const double *AW,
                         const double *AP, const double *Cx, const double *Cw, const double *Cp, double *Xo, double *Po, double *AXo,
                         double *APo)
{
    REQUIRE_EIG_OP(h, n);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (!X || !W || !P || !AX || !AW || !AP || !Cx || !Cw || !Cp || !Xo || !Po || !AXo || !APo) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int Wd = multi_width(k);
    const size_t len = (size_t)n * Wd, cm = (size_t)n * k;
    // an output that is the array it replaces (Xo == X, ...) is updated in place on the device as well
    const double *in[6] = {X, W, P, AX, AW, AP};
    double *out[4] = {Xo, Po, AXo, APo};
    const int replaces[4] = {0, 2, 3, 5};
    std::vector<double> coef(3 * (size_t)Wd * Wd, 0.0);
    const double *cs[3] = {Cx, Cw, Cp};
    for (int m = 0; m < 3; ++m)
        for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b) coef[(size_t)m * Wd * Wd + a * Wd + b] = cs[m][a * k + b];
    DBuf stage(E, cm), dcoef(E, coef.size(), coef.data());
    std::vector<std::unique_ptr<DBuf>> bi, bo;
    bool ok = stage.p && dcoef.p;
    for (int i = 0; i < 6 && ok; ++i) {
        bi.emplace_back(new DBuf(E, len));
        ok = bi.back()->p && hipMemcpy(stage.p, in[i], cm * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) launch_interleave(n, k, Wd, stage.p, n, bi.back()->p, E.stream());
        if (ok) ok = hipStreamSynchronize(E.stream()) == hipSuccess;
    }
    double *dst[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int o = 0; o < 4 && ok; ++o) {
        if (out[o] == in[replaces[o]]) {
            dst[o] = bi[replaces[o]]->p;
        } else {
            bo.emplace_back(new DBuf(E, len));
            ok = bo.back()->p != nullptr;
            dst[o] = bo.back()->p;
        }
    }
    if (!ok) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_eig_update(n, Wd, k, bi[0]->p, bi[1]->p, bi[2]->p, bi[3]->p, bi[4]->p, bi[5]->p, dcoef.p, dst[0], dst[1], dst[2], dst[3], E.stream());
    for (int o = 0; o < 4 && ok; ++o) {
        launch_deinterleave(n, k, Wd, dst[o], stage.p, n, E.stream());
        ok = stage.get(out[o]);
    }
    return done(E, ok);
}

int sparsh_op_eig_b_multi(sparsh_handle h, int nrhs, const double *X, double *Y)
{
    REQUIRE_MULTI_ARGS(h, nrhs);
    if (!X || !Y) return fail(SPARSH_EINVAL, "NULL array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    if (!E.eig_b_set()) return fail(SPARSH_ESTATE, "sparsh_eig_set_b has not been called");
    const size_t cm = (size_t)E.n0() * nrhs;
    DBuf dx(E, cm, X), dy(E, cm);
    if (!dx.p || !dy.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    if (int rc = E.op_eig_b_multi(nrhs, dx.p, dy.p); rc != SPARSH_OK) return fail(rc, E.error);
    return done(E, dy.get(Y));
}

int sparsh_op_eig_residual_gen(sparsh_handle h, int n, int k, const double *AX, const double *BX, const double *theta, double *R,
                               double *rnorms, double *bnorms)
{
    REQUIRE_EIG_OP(h, n);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (!AX || !BX || !theta || !R || !rnorms || !bnorms) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int W = multi_width(k);
    const size_t len = (size_t)n * W;
    std::vector<double> th(W, 0.0), bn(W, 0.0);
    std::copy(theta, theta + k, th.begin());
    DBuf dax(E, (size_t)n * k, AX), dbx(E, (size_t)n * k, BX), bax(E, len), bbx(E, len), br(E, len), dth(E, (size_t)W, th.data()),
        part(E, (size_t)2 * W * eig_grid(n, W)), drn(E, (size_t)W), dbn(E, (size_t)W), dr(E, (size_t)n * k);
    if (!dax.p || !dbx.p || !bax.p || !bbx.p || !br.p || !dth.p || !part.p || !drn.p || !dbn.p || !dr.p)
        return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_interleave(n, k, W, dax.p, n, bax.p, E.stream());
    launch_interleave(n, k, W, dbx.p, n, bbx.p, E.stream());
    launch_eig_residual_gen(n, W, bax.p, bbx.p, dth.p, br.p, part.p, drn.p, dbn.p, E.stream());
    launch_deinterleave(n, k, W, br.p, dr.p, n, E.stream());
    if (!dr.get(R) || !drn.get(th.data()) || !dbn.get(bn.data())) return done(E, false);
    std::copy(th.begin(), th.begin() + k, rnorms);
    std::copy(bn.begin(), bn.begin() + k, bnorms);
    return done(E, true);
}

int sparsh_op_eig_update_gen(sparsh_handle h, int n, int k, const double *const in[9], const double *Cx, const double *Cw, const double *Cp,
                             double *const out[6])
{
    REQUIRE_EIG_OP(h, n);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (!in || !out || !Cx || !Cw || !Cp) return fail(SPARSH_EINVAL, "NULL array");
    for (int i = 0; i < 9; ++i)
        if (!in[i]) return fail(SPARSH_EINVAL, "NULL array");
    for (int o = 0; o < 6; ++o)
        if (!out[o]) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int Wd = multi_width(k);
    const size_t len = (size_t)n * Wd, cm = (size_t)n * k;
    const int replaces[6] = {0, 2, 3, 5, 6, 8};
    std::vector<double> coef(3 * (size_t)Wd * Wd, 0.0);
    const double *cs[3] = {Cx, Cw, Cp};
    for (int m = 0; m < 3; ++m)
        for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b) coef[(size_t)m * Wd * Wd + a * Wd + b] = cs[m][a * k + b];
    DBuf stage(E, cm), dcoef(E, coef.size(), coef.data());
    std::vector<std::unique_ptr<DBuf>> bi, bo;
    bool ok = stage.p && dcoef.p;
    for (int i = 0; i < 9 && ok; ++i) {
        bi.emplace_back(new DBuf(E, len));
        ok = bi.back()->p && hipMemcpy(stage.p, in[i], cm * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) launch_interleave(n, k, Wd, stage.p, n, bi.back()->p, E.stream());
        if (ok) ok = hipStreamSynchronize(E.stream()) == hipSuccess;
    }
    const double *src[9] = {nullptr};
    double *dst[6] = {nullptr};
    for (int i = 0; i < 9 && ok; ++i) src[i] = bi[i]->p;
    for (int o = 0; o < 6 && ok; ++o) {
        if (out[o] == in[replaces[o]]) {
            dst[o] = bi[replaces[o]]->p;
        } else {
            bo.emplace_back(new DBuf(E, len));
            ok = bo.back()->p != nullptr;
            dst[o] = bo.back()->p;
        }
    }
    if (!ok) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_eig_update_gen(n, Wd, k, src, dcoef.p, dst, E.stream());
    for (int o = 0; o < 6 && ok; ++o) {
        launch_deinterleave(n, k, Wd, dst[o], stage.p, n, E.stream());
        ok = stage.get(out[o]);
    }
    return done(E, ok);
}

// ---- the orthonormalised basis and the guard vectors of the eigensolver (SPARSH_EIG_BASIS_ORTHO; eig_ortho_kernels.hip, eig_chol.hpp) ----

int sparsh_set_eig_options(sparsh_handle h, int basis, int wanted)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (basis != SPARSH_EIG_BASIS_PLAIN && basis != SPARSH_EIG_BASIS_ORTHO)
        return fail(SPARSH_EINVAL, "basis must be SPARSH_EIG_BASIS_PLAIN (0) or SPARSH_EIG_BASIS_ORTHO (1)");
    if (wanted < 0 || wanted > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "wanted must be 0 .. SPARSH_MAX_RHS (8)");
    return h->eng->set_eig_options(basis, wanted);
}

int sparsh_eig_options(sparsh_handle h, int *basis, int *wanted)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (basis) *basis = h->eng->eig_basis();
    if (wanted) *wanted = h->eng->eig_wanted();
    return SPARSH_OK;
}

int sparsh_eig_ortho_info(sparsh_handle h, int *dropped_w, int *dropped_p, long *bytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (dropped_w) *dropped_w = h->eng->eig_dropped_w();
    if (dropped_p) *dropped_p = h->eng->eig_dropped_p();
    if (bytes) *bytes = (long)h->eng->eig_ortho_bytes();
    return SPARSH_OK;
}

int sparsh_debug_eig_chol(int m, const double *G, const int *mask_in, double *T, int *mask_out)
{
    if (m < 1 || m > kEigCholMax) return fail(SPARSH_EINVAL, "m must be 1 .. 8");
    if (!G || !mask_in || !T || !mask_out) return fail(SPARSH_EINVAL, "NULL array");
    double mi[kEigCholMax], mo[kEigCholMax], L[kEigCholMax * kEigCholMax] = {0.0}, d[kEigCholMax] = {0.0}, z[kEigCholMax] = {0.0};
    for (int i = 0; i < m; ++i) mi[i] = mask_in[i] ? 1.0 : 0.0;
    (void)eig_chol(m, G, m, mi, T, m, mo, L, d, z);
    for (int i = 0; i < m; ++i) mask_out[i] = mo[i] != 0.0 ? 1 : 0;
    return SPARSH_OK;
}

int sparsh_op_eig_chol_small(sparsh_handle h, int W, const double *G, const int *mask_in, double *T, int *mask_out)
{
    REQUIRE_EIG_OP(h, 1);
    if (W != 2 && W != 4 && W != 8) return fail(SPARSH_EINVAL, "W must be 2, 4 or 8");
    if (!G || !mask_in || !T || !mask_out) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    double m[kEigCholMax];
    for (int i = 0; i < W; ++i) m[i] = mask_in[i] ? 1.0 : 0.0;
    DBuf dg(E, (size_t)W * W, G), dm(E, (size_t)W, m), dt(E, (size_t)W * W);
    if (!dg.p || !dm.p || !dt.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_eig_chol_small(W, dg.p, dm.p, dt.p, dm.p, E.stream());  // the mask is replaced in place, as the second pass over W does
    if (!dt.get(T) || !dm.get(m)) return done(E, false);
    for (int i = 0; i < W; ++i) mask_out[i] = m[i] != 0.0 ? 1 : 0;
    return done(E, true);
}

int sparsh_op_eig_active_mask(sparsh_handle h, int k, int gen, double tol, const double *theta, const double *rn, const double *bn, int *mask)
{
    REQUIRE_EIG_OP(h, 1);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (!theta || !rn || !mask || (gen && !bn)) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int W = multi_width(k);
    std::vector<double> th(W, 0.0), r(W, 0.0), b(W, 0.0), m(3 * (size_t)W, -1.0);
    std::copy(theta, theta + k, th.begin());
    std::copy(rn, rn + k, r.begin());
    if (gen) std::copy(bn, bn + k, b.begin());
    DBuf dth(E, (size_t)W, th.data()), dr(E, (size_t)W, r.data()), db(E, (size_t)W, b.data()), dm(E, 3 * (size_t)W, m.data());
    if (!dth.p || !dr.p || !db.p || !dm.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_eig_active_mask(W, k, gen != 0, tol, dth.p, dr.p, db.p, dm.p, E.stream());
    if (!dm.get(m.data())) return done(E, false);
    for (int c = W; c < 3 * W; ++c)
        if (m[c] != 0.0) return fail(SPARSH_ENUMERIC, "the masks of W and P were not cleared");
    for (int c = k; c < W; ++c)
        if (m[c] != 0.0) return fail(SPARSH_ENUMERIC, "a padding column is active");
    for (int c = 0; c < k; ++c) mask[c] = m[c] != 0.0 ? 1 : 0;
    return done(E, true);
}

int sparsh_op_eig_transform(sparsh_handle h, int n, int k, int nb, double *const V[3], const double *T)
{
    REQUIRE_EIG_OP(h, n);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (nb < 1 || nb > 3) return fail(SPARSH_EINVAL, "nb must be 1 .. 3");
    if (!V || !T) return fail(SPARSH_EINVAL, "NULL array");
    for (int b = 0; b < nb; ++b)
        if (!V[b]) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int W = multi_width(k);
    const size_t len = (size_t)n * W, cm = (size_t)n * k;
    std::vector<double> tp((size_t)W * W, 0.0);
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) tp[(size_t)a * W + b] = T[a * k + b];
    DBuf stage(E, cm), dt(E, tp.size(), tp.data());
    std::vector<std::unique_ptr<DBuf>> blk;
    bool ok = stage.p && dt.p;
    double *dev[3] = {nullptr, nullptr, nullptr};
    for (int b = 0; b < nb && ok; ++b) {
        blk.emplace_back(new DBuf(E, len));
        ok = blk.back()->p && hipMemcpy(stage.p, V[b], cm * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) launch_interleave(n, k, W, stage.p, n, blk.back()->p, E.stream());
        if (ok) ok = hipStreamSynchronize(E.stream()) == hipSuccess;
        dev[b] = blk.back()->p;
    }
    if (!ok) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_eig_transform(n, W, k, nb, dev, dt.p, E.stream());
    std::vector<double> full(len);
    for (int b = 0; b < nb; ++b) {
        (void)hipStreamSynchronize(E.stream());
        if (hipMemcpy(full.data(), dev[b], len * 8, hipMemcpyDeviceToHost) != hipSuccess) return done(E, false);
        for (size_t i = 0; i < (size_t)n; ++i) {
            for (int c = 0; c < k; ++c) V[b][(size_t)c * n + i] = full[i * W + c];
            for (int c = k; c < W; ++c)  // (bitwise: a -0.0 or a NaN in a padding column is caught too)
                if (full[i * W + c] != 0.0 || std::signbit(full[i * W + c])) return fail(SPARSH_ENUMERIC, "a padding column of a transformed block is not zero");
        }
    }
    return done(E, true);
}

int sparsh_op_eig_ortho_apply(sparsh_handle h, int n, int k, const double *X, const double *C, const int *mask, const double *W0, double *Wout)
{
    REQUIRE_EIG_OP(h, n);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (!X || !C || !mask || !W0 || !Wout) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int W = multi_width(k);
    const size_t len = (size_t)n * W, cm = (size_t)n * k;
    std::vector<double> cp((size_t)W * W, 0.0), mk(W, 0.0);
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) cp[(size_t)a * W + b] = C[a * k + b];
    for (int c = 0; c < k; ++c) mk[c] = mask[c] ? 1.0 : 0.0;
    DBuf dx(E, cm, X), dw(E, cm, W0), bx(E, len), bw(E, len), bo(E, len), dc(E, cp.size(), cp.data()), dm(E, (size_t)W, mk.data());
    if (!dx.p || !dw.p || !bx.p || !bw.p || !bo.p || !dc.p || !dm.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_interleave(n, k, W, dx.p, n, bx.p, E.stream());
    launch_interleave(n, k, W, dw.p, n, bw.p, E.stream());
    double *dst = Wout == W0 ? bw.p : bo.p;  // W0 == Wout on the host: in place on the device too
    launch_eig_ortho_apply(n, W, k, bx.p, dc.p, dm.p, bw.p, dst, E.stream());
    std::vector<double> full(len);
    (void)hipStreamSynchronize(E.stream());
    if (hipMemcpy(full.data(), dst, len * 8, hipMemcpyDeviceToHost) != hipSuccess) return done(E, false);
    for (size_t i = 0; i < (size_t)n; ++i) {
        for (int c = 0; c < k; ++c) Wout[(size_t)c * n + i] = full[i * W + c];
        for (int c = k; c < W; ++c)
            if (full[i * W + c] != 0.0 || std::signbit(full[i * W + c])) return fail(SPARSH_ENUMERIC, "a padding column of the block that came back is not zero");
    }
    return done(E, true);
}

// ---- block CG (engine_bcg.cpp, bcg_kernels.hip, bcg_small.hpp) ----

int sparsh_bcg_info(sparsh_handle h, int *iterations, int *min_rank, int *dropped, long *bytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (iterations) *iterations = h->eng->bcg_iterations();
    if (min_rank) *min_rank = h->eng->bcg_min_rank();
    if (dropped) *dropped = h->eng->bcg_dropped();
    if (bytes) *bytes = (long)h->eng->bcg_bytes();
    return SPARSH_OK;
}

int sparsh_debug_bcg_small(int k, const double *G, const double *C, double sign, double *coef, int *keep)
{
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (!G || !C || !coef || !keep) return fail(SPARSH_EINVAL, "NULL array");
    double L[kBcgMax * kBcgMax] = {0.0}, d[kBcgMax] = {0.0}, y[kBcgMax];
    int kp[kBcgMax] = {0};
    const int rank = bcg_factor(k, G, k, L, d, kp);
    for (int c = 0; c < k; ++c) bcg_solve_column(k, L, d, kp, C, k, c, sign, coef, k, y);
    std::copy(kp, kp + k, keep);
    return rank;
}

int sparsh_op_bcg_small(sparsh_handle h, int W, int k, const double *G, const double *C, double sign, double *coef, int *keep)
{
    REQUIRE_EIG_OP(h, 1);
    if (W != 2 && W != 4 && W != 8) return fail(SPARSH_EINVAL, "W must be 2, 4 or 8");
    if (k < 1 || k > W) return fail(SPARSH_EINVAL, "k must be 1 .. W");
    if (!G || !C || !coef || !keep) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    std::vector<double> g((size_t)W * W, 0.0), c((size_t)W * W, 0.0), zeros((size_t)kBcgMax * kBcgMax, 0.0);
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) {
            g[(size_t)a * W + b] = G[a * k + b];
            c[(size_t)a * W + b] = C[a * k + b];
        }
    DBuf dg(E, g.size(), g.data()), dc(E, c.size(), c.data()), o1(E, g.size(), zeros.data()), o2(E, g.size(), zeros.data()),
        dl(E, zeros.size(), zeros.data()), dd(E, kBcgMax, zeros.data()), dres(E, kBcgMax, zeros.data()), dfl(E, BF_COUNT / 2, zeros.data());
    if (!dg.p || !dc.p || !o1.p || !o2.p || !dl.p || !dd.p || !dres.p || !dfl.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    BcgState s;
    s.L = dl.p;
    s.d = dd.p;
    s.res = dres.p;
    s.flags = reinterpret_cast<int *>(dfl.p);
    // the solve of an iteration's first call, then the second call's: the same G with the factor kept on the device
    launch_bcg_small(W, k, true, dg.p, dc.p, sign, s, o1.p, 0, E.stream());
    int flags[BF_COUNT];
    (void)hipStreamSynchronize(E.stream());
    bool ok = hipMemcpy(flags, dfl.p, sizeof(flags), hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && flags[BF_DONE]) {  // rank 0 ends a solve: lift the flag so that the second launch runs
        const int zero = 0;
        ok = hipMemcpy(s.flags + BF_DONE, &zero, sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    }
    launch_bcg_small(W, k, false, dg.p, dc.p, sign, s, o2.p, 0, E.stream());
    std::vector<double> f1(g.size()), f2(g.size());
    ok = ok && o1.get(f1.data()) && o2.get(f2.data());
    if (!ok) return done(E, false);
    if (std::memcmp(f1.data(), f2.data(), f1.size() * 8) != 0) return fail(SPARSH_ENUMERIC, "the kept factor gives other coefficients");
    for (int a = 0; a < W; ++a)
        for (int b = 0; b < W; ++b) {
            if (a < k && b < k) coef[a * k + b] = f1[(size_t)a * W + b];
            else if (f1[(size_t)a * W + b] != 0.0) return fail(SPARSH_ENUMERIC, "a padding entry of the coefficient matrix is not zero");
        }
    std::copy(flags + BF_KEEP, flags + BF_KEEP + k, keep);
    if (int rc = done(E, true); rc != SPARSH_OK) return rc;
    return flags[BF_RANK];
}

}  // extern "C"

namespace {

// host blocks (column-major, n x k) to interleaved device blocks of width W and back, through one staging buffer
bool bcg_put(Engine &E, int n, int k, int W, const double *src, DBuf &stage, double *blk)
{
    if (hipMemcpy(stage.p, src, (size_t)n * k * 8, hipMemcpyHostToDevice) != hipSuccess) return false;
    launch_interleave(n, k, W, stage.p, n, blk, E.stream());
    return hipStreamSynchronize(E.stream()) == hipSuccess;
}

// ... and back; a padding column that is not zero makes *padding_clean false
bool bcg_get(Engine &E, int n, int k, int W, const double *blk, double *dst, bool *padding_clean)
{
    std::vector<double> full((size_t)n * W);
    if (hipStreamSynchronize(E.stream()) != hipSuccess) return false;
    if (hipMemcpy(full.data(), blk, full.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (size_t i = 0; i < (size_t)n; ++i) {
        for (int c = 0; c < k; ++c) dst[(size_t)c * n + i] = full[i * W + c];
        for (int c = k; c < W; ++c)
            if (full[i * W + c] != 0.0) *padding_clean = false;
    }
    return true;
}

std::vector<double> bcg_pad_coef(int k, int W, const double *coef)
{
    std::vector<double> out((size_t)W * W, 0.0);
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) out[(size_t)a * W + b] = coef[a * k + b];
    return out;
}

}  // namespace

extern "C" {

int sparsh_op_bcg_update(sparsh_handle h, int n, int k, const double *X, const double *R, const double *P, const double *Q,
                         const double *alpha, double *Xo, double *Ro, double *norms)
{
    REQUIRE_EIG_OP(h, n);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (!X || !R || !P || !Q || !alpha || !Xo || !Ro || !norms) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int W = multi_width(k);
    const size_t len = (size_t)n * W;
    const std::vector<double> coef = bcg_pad_coef(k, W, alpha), zeros(kBcgMax * kBcgMax, 0.0);
    DBuf stage(E, (size_t)n * k), bx(E, len), br(E, len), bp(E, len), bq(E, len), bxo(E, len), bro(E, len), dcoef(E, coef.size(), coef.data()),
        part(E, (size_t)W * bcg_grid(n, W)), dl(E, zeros.size(), zeros.data()), dd(E, kBcgMax, zeros.data()), dres(E, kBcgMax, zeros.data()),
        dfl(E, BF_COUNT / 2, zeros.data());
    bool ok = stage.p && bx.p && br.p && bp.p && bq.p && bxo.p && bro.p && dcoef.p && part.p && dl.p && dd.p && dres.p && dfl.p;
    ok = ok && bcg_put(E, n, k, W, X, stage, bx.p) && bcg_put(E, n, k, W, R, stage, br.p) && bcg_put(E, n, k, W, P, stage, bp.p) &&
         bcg_put(E, n, k, W, Q, stage, bq.p);
    if (!ok) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    // an output that is the array it replaces (Xo == X, Ro == R) is updated in place on the device as well
    double *dxo = Xo == X ? bx.p : bxo.p, *dro = Ro == R ? br.p : bro.p;
    BcgState s;
    s.L = dl.p;
    s.d = dd.p;
    s.res = dres.p;
    s.flags = reinterpret_cast<int *>(dfl.p);
    const int nb = launch_bcg_update(n, W, k, s.flags + BF_DONE, bx.p, br.p, bp.p, bq.p, dcoef.p, dxo, dro, part.p, E.stream());
    launch_bcg_finalize(W, k, part.p, nb, s, 0.0, nullptr, 0, 0, E.stream());
    bool clean = true;
    double res[kBcgMax];
    ok = bcg_get(E, n, k, W, dxo, Xo, &clean) && bcg_get(E, n, k, W, dro, Ro, &clean) && dres.get(res);
    if (!ok) return done(E, false);
    if (!clean) return fail(SPARSH_ENUMERIC, "a padding column of an updated block is not zero");
    std::copy(res, res + k, norms);
    return done(E, true);
}

int sparsh_op_bcg_dir(sparsh_handle h, int n, int k, const double *Z, const double *P, const double *beta, double *Po)
{
    REQUIRE_EIG_OP(h, n);
    if (k < 1 || k > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "k must be 1 .. SPARSH_MAX_RHS (8)");
    if (!Z || !P || !beta || !Po) return fail(SPARSH_EINVAL, "NULL array");
    Engine &E = *h->eng;
    const int W = multi_width(k);
    const size_t len = (size_t)n * W;
    const std::vector<double> coef = bcg_pad_coef(k, W, beta);
    DBuf stage(E, (size_t)n * k), bz(E, len), bp(E, len), bpo(E, len), dcoef(E, coef.size(), coef.data());
    bool ok = stage.p && bz.p && bp.p && bpo.p && dcoef.p;
    ok = ok && bcg_put(E, n, k, W, Z, stage, bz.p) && bcg_put(E, n, k, W, P, stage, bp.p);
    if (!ok) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    double *dpo = Po == P ? bp.p : bpo.p;  // in place on the device too
    launch_bcg_dir(n, W, k, nullptr, bz.p, bp.p, dcoef.p, dpo, E.stream());
    bool clean = true;
    if (!bcg_get(E, n, k, W, dpo, Po, &clean)) return done(E, false);
    if (!clean) return fail(SPARSH_ENUMERIC, "a padding column of the new direction block is not zero");
    return done(E, true);
}

}  // extern "C"

// ---- operator-level hooks of the single-vector Krylov kernels and of finalize_kernel (kernels.hip): one launch through the loops' own
// launcher on device vectors of the call's own; the handle lends its stream and allocator
namespace {

static_assert(SPARSH_OP_SCALARS == S_COUNT, "sparsh_amg.h: SPARSH_OP_SCALARS is the number of scalar slots");
static_assert(SPARSH_OP_PARTIALS == kEwGridMax, "sparsh_amg.h: SPARSH_OP_PARTIALS is the cap of the elementwise grid");

// host arrays of one call on the device: a host array given twice is one device vector (the first registration allocates, so the
// padded -- written -- arguments are registered first)
struct OpVecs {
    Engine &E;
    struct Ent {
        const double *host;
        std::unique_ptr<DBuf> buf;
    };
    std::vector<Ent> v;
    bool ok = true, fits = true;
    explicit OpVecs(Engine &e) : E(e) {}
    double *dev(const double *host, size_t count)
    {
        if (!host) return nullptr;
        for (Ent &e : v)
            if (e.host == host) {
                if (e.buf->n < count) fits = false;
                return e.buf->p;
            }
        v.push_back(Ent{host, std::make_unique<DBuf>(E, count, host)});
        if (!v.back().buf->p) ok = false;
        return v.back().buf->p;
    }
    bool get(double *host)
    {
        if (!host) return true;
        for (Ent &e : v)
            if (e.host == host) return e.buf->get(host);
        return false;
    }
    int status() const
    {
        if (!fits) return fail(SPARSH_EINVAL, "an array given for a written and a read argument must be the padded one");
        return ok ? SPARSH_OK : fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    }
};

// a zeroed scalar block with the given slots set
struct OpScal {
    double host[S_COUNT] = {};
    OpScal &set(int slot, double v)
    {
        host[slot] = v;
        return *this;
    }
};

constexpr size_t kOpPartials = (size_t)SPARSH_OP_PARTIALS + SPARSH_OP_PAD;
inline size_t op_padded(int n) { return (size_t)n + SPARSH_OP_PAD; }

}  // namespace

#define REQUIRE_KRYLOV_OP(h, n)                                       \
    if (!(h) || !(h)->eng) return fail(SPARSH_EINVAL, "null handle"); \
    if ((n) <= 0) return fail(SPARSH_EINVAL, "n <= 0")

extern "C" {

int sparsh_op_dot2(sparsh_handle h, int n, const double *a, const double *b, const double *c, const double *d, double *p0, double *p1,
                   int *nblk)
{
    REQUIRE_KRYLOV_OP(h, n);
    if (!a || !b || !c || !d || !p0 || !p1 || !nblk || p0 == p1) return fail(SPARSH_EINVAL, "null array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    OpVecs V(E);
    double *dp0 = V.dev(p0, kOpPartials), *dp1 = V.dev(p1, kOpPartials);
    const double *da = V.dev(a, (size_t)n), *db = V.dev(b, (size_t)n), *dc = V.dev(c, (size_t)n), *dd = V.dev(d, (size_t)n);
    if (int rc = V.status(); rc != SPARSH_OK) return rc;
    launch_dot2(n, da, db, dc, dd, dp0, dp1, nblk, E.stream());
    return done(E, V.get(p0) && V.get(p1));
}

int sparsh_op_cg_update(sparsh_handle h, int n, double alpha, double nalpha, const double *p, const double *Ap, double *x, double *r,
                        double *partial, int *nblk, int zero, const double *d, double dconst, double omega, int nt, double *z0)
{
    REQUIRE_KRYLOV_OP(h, n);
    if (!p || !Ap || !r || !partial || !nblk) return fail(SPARSH_EINVAL, "null array");
    if (zero != 0 && zero != 1) return fail(SPARSH_EINVAL, "zero must be 0 or 1");
    if (nt != 0 && nt != 1) return fail(SPARSH_EINVAL, "nt must be 0 or 1");
    if (zero && !z0) return fail(SPARSH_EINVAL, "null array: the zero-guess form writes z0");
    if (x == r || (zero && (z0 == r || z0 == x))) return fail(SPARSH_EINVAL, "the written vectors must be distinct arrays");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    OpVecs V(E);
    OpScal s;
    s.set(S_ALPHA, alpha).set(S_NALPHA, nalpha);
    DBuf scal(E, (size_t)S_COUNT, s.host);
    double *dx = V.dev(x, op_padded(n)), *dr = V.dev(r, op_padded(n)), *dz0 = zero ? V.dev(z0, op_padded(n)) : nullptr;
    double *dpart = V.dev(partial, kOpPartials);
    const double *dp = V.dev(p, (size_t)n), *dAp = V.dev(Ap, (size_t)n), *dd = zero ? V.dev(d, (size_t)n) : nullptr;
    if (!scal.p) return fail(SPARSH_ENODEV, "device allocation failed");
    if (int rc = V.status(); rc != SPARSH_OK) return rc;
    if (zero) launch_cg_update_zero(n, scal.p, dp, dAp, dx, dr, dpart, nblk, dd, dconst, omega, dz0, E.stream(), nt != 0);
    else launch_cg_update(n, scal.p, dp, dAp, dx, dr, dpart, nblk, E.stream());
    return done(E, V.get(x) && V.get(r) && V.get(partial) && (!zero || V.get(z0)));
}

int sparsh_op_p_update(sparsh_handle h, int n, double beta, const double *z, double *p)
{
    REQUIRE_KRYLOV_OP(h, n);
    if (!z || !p) return fail(SPARSH_EINVAL, "null array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    OpVecs V(E);
    OpScal s;
    s.set(S_BETA, beta);
    DBuf scal(E, (size_t)S_COUNT, s.host);
    double *dp = V.dev(p, op_padded(n));
    const double *dz = V.dev(z, (size_t)n);
    if (!scal.p) return fail(SPARSH_ENODEV, "device allocation failed");
    if (int rc = V.status(); rc != SPARSH_OK) return rc;
    launch_p_update(n, scal.p, dz, dp, E.stream());
    return done(E, V.get(p));
}

int sparsh_op_xp_update(sparsh_handle h, int n, double alpha, double beta, const double *z, double *p, double *x)
{
    REQUIRE_KRYLOV_OP(h, n);
    if (!z || !p || !x || p == x) return fail(SPARSH_EINVAL, "null array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    OpVecs V(E);
    OpScal s;
    s.set(S_ALPHA, alpha).set(S_BETA, beta);
    DBuf scal(E, (size_t)S_COUNT, s.host);
    double *dp = V.dev(p, op_padded(n)), *dx = V.dev(x, op_padded(n));
    const double *dz = V.dev(z, (size_t)n);
    if (!scal.p) return fail(SPARSH_ENODEV, "device allocation failed");
    if (int rc = V.status(); rc != SPARSH_OK) return rc;
    launch_xp_update(n, scal.p, dz, dp, dx, E.stream());
    return done(E, V.get(p) && V.get(x));
}

int sparsh_op_bicg_s(sparsh_handle h, int n, double alpha, const double *r, const double *Ap, double *s)
{
    REQUIRE_KRYLOV_OP(h, n);
    if (!r || !Ap || !s) return fail(SPARSH_EINVAL, "null array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    OpVecs V(E);
    OpScal sc;
    sc.set(S_ALPHA, alpha);
    DBuf scal(E, (size_t)S_COUNT, sc.host);
    double *ds = V.dev(s, op_padded(n));
    const double *dr = V.dev(r, (size_t)n), *dAp = V.dev(Ap, (size_t)n);
    if (!scal.p) return fail(SPARSH_ENODEV, "device allocation failed");
    if (int rc = V.status(); rc != SPARSH_OK) return rc;
    launch_bicg_s(n, scal.p, dr, dAp, ds, E.stream());
    return done(E, V.get(s));
}

int sparsh_op_bicg_xr(sparsh_handle h, int n, double alpha, double omega1, const double *p1, const double *s1, const double *s,
                      const double *As, const double *r0, double *x, double *r, double *q0, double *q1, int *nblk)
{
    REQUIRE_KRYLOV_OP(h, n);
    if (!p1 || !s1 || !s || !As || !r0 || !x || !r || !q0 || !q1 || !nblk) return fail(SPARSH_EINVAL, "null array");
    if (x == r || q0 == q1) return fail(SPARSH_EINVAL, "the written vectors must be distinct arrays");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    OpVecs V(E);
    OpScal sc;
    sc.set(S_ALPHA, alpha).set(S_OMEGA1, omega1);
    DBuf scal(E, (size_t)S_COUNT, sc.host);
    double *dx = V.dev(x, op_padded(n)), *dr = V.dev(r, op_padded(n)), *dq0 = V.dev(q0, kOpPartials), *dq1 = V.dev(q1, kOpPartials);
    const double *dp1 = V.dev(p1, (size_t)n), *ds1 = V.dev(s1, (size_t)n), *ds = V.dev(s, (size_t)n), *dAs = V.dev(As, (size_t)n),
                 *dr0 = V.dev(r0, (size_t)n);
    if (!scal.p) return fail(SPARSH_ENODEV, "device allocation failed");
    if (int rc = V.status(); rc != SPARSH_OK) return rc;
    launch_bicg_xr(n, scal.p, dp1, ds1, ds, dAs, dr0, dx, dr, dq0, dq1, nblk, E.stream());
    return done(E, V.get(x) && V.get(r) && V.get(q0) && V.get(q1));
}

int sparsh_op_bicg_p(sparsh_handle h, int n, double beta, double omega1, const double *r, const double *Ap, double *p)
{
    REQUIRE_KRYLOV_OP(h, n);
    if (!r || !Ap || !p) return fail(SPARSH_EINVAL, "null array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    OpVecs V(E);
    OpScal sc;
    sc.set(S_BETA, beta).set(S_OMEGA1, omega1);
    DBuf scal(E, (size_t)S_COUNT, sc.host);
    double *dp = V.dev(p, op_padded(n));
    const double *dr = V.dev(r, (size_t)n), *dAp = V.dev(Ap, (size_t)n);
    if (!scal.p) return fail(SPARSH_ENODEV, "device allocation failed");
    if (int rc = V.status(); rc != SPARSH_OK) return rc;
    launch_bicg_p(n, scal.p, dr, dAp, dp, E.stream());
    return done(E, V.get(p));
}

int sparsh_op_finalize(sparsh_handle h, int code, int mode, const double *p0, int nblk, const double *p1, int nblk1, double *scal,
                       int slot_a, double *hist, int hist_cap, int it, int *iter_ctr, int repeat)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (code < FIN_STORE || code > FIN_FCG_BETA) return fail(SPARSH_EINVAL, "code must be one of the Fin codes 0..10");
    if (mode < 0 || mode > 2) return fail(SPARSH_EINVAL, "mode must be 0, 1 or 2");
    if (!scal || !iter_ctr || (mode != 2 && !p0)) return fail(SPARSH_EINVAL, "null array");
    if (nblk < 1 || (p1 && nblk1 < 1)) return fail(SPARSH_EINVAL, "nblk < 1");
    if (slot_a < 0 || slot_a >= S_COUNT) return fail(SPARSH_EINVAL, "slot out of range");
    if (hist && hist_cap < 1) return fail(SPARSH_EINVAL, "hist_cap < 1");
    if (*iter_ctr < 0) return fail(SPARSH_EINVAL, "the iteration counter must be >= 0");
    if (repeat < 1 || repeat > 64) return fail(SPARSH_EINVAL, "repeat must be in 1..64");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    OpVecs V(E);
    double *dscal = V.dev(scal, (size_t)S_COUNT), *dhist = hist ? V.dev(hist, op_padded(hist_cap)) : nullptr;
    const double *d0 = mode != 2 ? V.dev(p0, (size_t)nblk) : nullptr, *d1 = (mode != 2 && p1) ? V.dev(p1, (size_t)nblk1) : nullptr;
    int *dctr = static_cast<int *>(E.dalloc(2 * sizeof(int)));
    if (int rc = V.status(); rc != SPARSH_OK || !dctr) {
        E.dfree(dctr);
        return rc != SPARSH_OK ? rc : fail(SPARSH_ENODEV, "device allocation failed");
    }
    bool ok = hipMemcpy(dctr, iter_ctr, sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    // (mode 2 reads no partials: its sums are what S_SUM0 / S_SUM1 of the block hold, as after the all-reduce)
    for (int k = 0; ok && k < repeat; ++k)
        launch_finalize((Fin)code, d0, d1, nblk, dscal, slot_a, dhist, it, E.stream(), mode, dctr, hist ? hist_cap : 1, p1 ? nblk1 : -1);
    ok = ok && V.get(scal) && V.get(hist);
    ok = ok && hipMemcpy(iter_ctr, dctr, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    E.dfree(dctr);
    return done(E, ok);
}

}  // extern "C"

// ---- block BiCGStab (engine_mbicg.cpp, mbicg_kernels.hip): its info call and the operator-level hooks of its kernels.  A hook is one
// launch through the launcher the loop uses, on device blocks of the call's own; the handle lends its stream and allocator.
namespace {

static_assert(SPARSH_MBICG_SCALARS == MB_COUNT, "sparsh_amg.h: SPARSH_MBICG_SCALARS is the number of per-column scalar slots");
static_assert(SPARSH_MBICG_PARTIALS == kMultiGridMax, "sparsh_amg.h: SPARSH_MBICG_PARTIALS is the cap of the block kernels' grid");

// what the padding columns of a block a hook's launch may write hold before the launch: they must come back with these bits
constexpr double kMbicgPadding = -7.25e300;

// host blocks (column-major, n x nrhs) as interleaved device blocks of width W.  A host array given twice is one device block; the
// written arguments are registered first, with the sentinel in their padding columns (read-only blocks are padded with zeros).
struct MbBlocks {
    Engine &E;
    int n, nrhs, W;
    struct Ent {
        const double *host;
        std::unique_ptr<DBuf> buf;
    };
    std::vector<Ent> v;
    std::vector<double> stage;
    bool ok = true;
    MbBlocks(Engine &e, int n_, int nrhs_) : E(e), n(n_), nrhs(nrhs_), W(multi_width(nrhs_)), stage((size_t)n_ * multi_width(nrhs_)) {}
    double *dev(const double *host, bool written)
    {
        for (Ent &e : v)
            if (e.host == host) return e.buf->p;
        for (size_t i = 0; i < (size_t)n; ++i)
            for (int c = 0; c < W; ++c) stage[i * W + c] = c < nrhs ? host[(size_t)c * n + i] : (written ? kMbicgPadding : 0.0);
        v.push_back(Ent{host, std::make_unique<DBuf>(E, stage.size(), stage.data())});
        if (!v.back().buf->p) ok = false;
        return v.back().buf->p;
    }
    // the block back into its host array; *clean goes false if a padding column no longer holds the sentinel
    bool get(double *host, bool *clean)
    {
        for (Ent &e : v)
            if (e.host == host) {
                if (!e.buf->get(stage.data())) return false;
                for (size_t i = 0; i < (size_t)n; ++i) {
                    for (int c = 0; c < nrhs; ++c) host[(size_t)c * n + i] = stage[i * W + c];
                    for (int c = nrhs; c < W; ++c)
                        if (std::memcmp(&stage[i * W + c], &kMbicgPadding, 8) != 0) *clean = false;
                }
                return true;
            }
        return false;
    }
};

// the per-column state of a hook on the device: scal (MB_COUNT x 8, slot-major) and frozen / iters / status (8 ints each); the
// padding columns are frozen
struct MbState {
    DBuf scal, flags;
    MbicgState s;
    MbState(Engine &E, int nrhs, const double *scal_host, const int *frozen, const int *iters, const int *status)
        : scal(E, (size_t)MB_COUNT * kMultiMax), flags(E, (3 * kMultiMax + 1) / 2)
    {
        int f[3 * kMultiMax] = {};
        for (int c = 0; c < kMultiMax; ++c) {
            f[c] = c < nrhs ? (frozen && frozen[c] != 0) : 1;
            f[kMultiMax + c] = (c < nrhs && iters) ? iters[c] : 0;
            f[2 * kMultiMax + c] = (c < nrhs && status) ? status[c] : 0;
        }
        if (scal.p) (void)hipMemcpy(scal.p, scal_host, (size_t)MB_COUNT * kMultiMax * 8, hipMemcpyHostToDevice);
        if (flags.p) (void)hipMemcpy(flags.p, f, sizeof(f), hipMemcpyHostToDevice);
        s.scal = scal.p;
        s.frozen = reinterpret_cast<int *>(flags.p);
        s.iters = s.frozen + kMultiMax;
        s.status = s.frozen + 2 * kMultiMax;
    }
    bool ok() const { return scal.p && flags.p; }
};

// a zeroed scalar block with one or two slots set per column
struct MbScal {
    double host[MB_COUNT * kMultiMax] = {};
    MbScal &set(int slot, int nrhs, const double *v)
    {
        for (int c = 0; c < nrhs; ++c) host[slot * kMultiMax + c] = v[c];
        return *this;
    }
};

}  // namespace

#define REQUIRE_MBICG_OP(h, n, nrhs)                                                                                  \
    if (!(h) || !(h)->eng) return fail(SPARSH_EINVAL, "null handle");                                                 \
    if ((n) <= 0) return fail(SPARSH_EINVAL, "n <= 0");                                                               \
    if ((nrhs) < 1 || (nrhs) > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "nrhs must be 1 .. SPARSH_MAX_RHS (8)")

extern "C" {

int sparsh_mbicg_info(sparsh_handle h, int *iterations, long *bytes)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (iterations) *iterations = h->eng->mbicg_iterations();
    if (bytes) *bytes = (long)h->eng->mbicg_bytes();
    return SPARSH_OK;
}

int sparsh_op_dot2_multi(sparsh_handle h, int n, int nrhs, const double *a, const double *b, const double *c, const double *d, double *part0,
                         double *part1, int *nblk)
{
    REQUIRE_MBICG_OP(h, n, nrhs);
    if (!a || !b || !c || !d || !part0 || !part1 || !nblk || part0 == part1) return fail(SPARSH_EINVAL, "NULL array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    MbBlocks V(E, n, nrhs);
    const int W = V.W, g = mbicg_reduce_grid(n);
    const double *da = V.dev(a, false), *db = V.dev(b, false), *dc = V.dev(c, false), *dd = V.dev(d, false);
    DBuf p0(E, (size_t)W * g), p1(E, (size_t)W * g);
    if (!V.ok || !p0.p || !p1.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    *nblk = launch_dot2_multi(n, W, da, db, dc, dd, p0.p, p1.p, E.stream());
    return done(E, p0.get(part0) && p1.get(part1));
}

int sparsh_op_bicg_s_multi(sparsh_handle h, int n, int nrhs, const int *frozen, const double *alpha, const double *R, const double *AP,
                           double *S)
{
    REQUIRE_MBICG_OP(h, n, nrhs);
    if (!frozen || !alpha || !R || !AP || !S || S == R || S == AP) return fail(SPARSH_EINVAL, "NULL array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    MbBlocks V(E, n, nrhs);
    MbScal sc;
    MbState st(E, nrhs, sc.set(MB_ALPHA, nrhs, alpha).host, frozen, nullptr, nullptr);
    double *ds = V.dev(S, true);
    const double *dr = V.dev(R, false), *dap = V.dev(AP, false);
    if (!V.ok || !st.ok()) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_bicg_s_multi(n, V.W, st.s, dr, dap, ds, E.stream());
    bool clean = true;
    if (!V.get(S, &clean)) return done(E, false);
    if (!clean) return fail(SPARSH_ENUMERIC, "a padding column of the block was written");
    return done(E, true);
}

int sparsh_op_bicg_xr_multi(sparsh_handle h, int n, int nrhs, const int *frozen, const double *alpha, const double *omega, const double *P1,
                            const double *S1, const double *S, const double *AS, const double *R0, double *X, double *R, double *part0,
                            double *part1, int *nblk)
{
    REQUIRE_MBICG_OP(h, n, nrhs);
    if (!frozen || !alpha || !omega || !P1 || !S1 || !S || !AS || !R0 || !X || !R || !part0 || !part1 || !nblk) return fail(SPARSH_EINVAL, "NULL array");
    if (X == R || part0 == part1) return fail(SPARSH_EINVAL, "the written arrays must be distinct");
    for (const double *in : {P1, S1, S, AS, R0})
        if (in == X || in == R) return fail(SPARSH_EINVAL, "a written block may not be a read block");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    MbBlocks V(E, n, nrhs);
    MbScal sc;
    sc.set(MB_ALPHA, nrhs, alpha).set(MB_OMEGA1, nrhs, omega);
    MbState st(E, nrhs, sc.host, frozen, nullptr, nullptr);
    const int W = V.W, g = mbicg_reduce_grid(n);
    double *dx = V.dev(X, true), *dr = V.dev(R, true);
    const double *dp1 = V.dev(P1, false), *ds1 = V.dev(S1, false), *ds = V.dev(S, false), *das = V.dev(AS, false), *dr0 = V.dev(R0, false);
    DBuf p0(E, (size_t)W * g), p1(E, (size_t)W * g);
    if (!V.ok || !st.ok() || !p0.p || !p1.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    *nblk = launch_bicg_xr_multi(n, W, st.s, dp1, ds1, ds, das, dr0, dx, dr, p0.p, p1.p, E.stream());
    bool clean = true;
    if (!(V.get(X, &clean) && V.get(R, &clean) && p0.get(part0) && p1.get(part1))) return done(E, false);
    if (!clean) return fail(SPARSH_ENUMERIC, "a padding column of a block was written");
    return done(E, true);
}

int sparsh_op_bicg_p_multi(sparsh_handle h, int n, int nrhs, const int *frozen, const double *beta, const double *omega, const double *R,
                           const double *AP, double *P)
{
    REQUIRE_MBICG_OP(h, n, nrhs);
    if (!frozen || !beta || !omega || !R || !AP || !P || P == R || P == AP) return fail(SPARSH_EINVAL, "NULL array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    MbBlocks V(E, n, nrhs);
    MbScal sc;
    sc.set(MB_BETA, nrhs, beta).set(MB_OMEGA1, nrhs, omega);
    MbState st(E, nrhs, sc.host, frozen, nullptr, nullptr);
    double *dp = V.dev(P, true);
    const double *dr = V.dev(R, false), *dap = V.dev(AP, false);
    if (!V.ok || !st.ok()) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_bicg_p_multi(n, V.W, st.s, dr, dap, dp, E.stream());
    bool clean = true;
    if (!V.get(P, &clean)) return done(E, false);
    if (!clean) return fail(SPARSH_ENUMERIC, "a padding column of the block was written");
    return done(E, true);
}

int sparsh_op_mbicg_finalize(sparsh_handle h, int code, int nrhs, const double *part0, int n0, const double *part1, int n1, double *scal,
                             int *frozen, int *iters, int *status, double tol, double *hist, int hist_cap, int it)
{
    if (!h || !h->eng) return fail(SPARSH_EINVAL, "null handle");
    if (nrhs < 1 || nrhs > SPARSH_MAX_RHS) return fail(SPARSH_EINVAL, "nrhs must be 1 .. SPARSH_MAX_RHS (8)");
    if (code < MBFIN_INIT || code > MBFIN_BETA_RES) return fail(SPARSH_EINVAL, "code must be one of the finalise codes 0..3");
    if (!part0 || !scal || !frozen || !iters || !status) return fail(SPARSH_EINVAL, "NULL array");
    if (n0 < 1 || n0 > kMultiGridMax || (part1 && (n1 < 1 || n1 > kMultiGridMax))) return fail(SPARSH_EINVAL, "the partial counts must be 1 .. SPARSH_MBICG_PARTIALS");
    if (hist_cap < 0 || (hist_cap > 0 && !hist) || it < 0) return fail(SPARSH_EINVAL, "hist_cap < 0, it < 0 or no history array");
    REQUIRE_READY(h);
    REQUIRE_SINGLE(h);
    Engine &E = *h->eng;
    const int W = multi_width(nrhs);
    MbState st(E, nrhs, scal, frozen, iters, status);
    DBuf p0(E, (size_t)W * n0, part0), p1(E, (size_t)W * (part1 ? n1 : 1), part1);
    // the histories of all 8 columns at the stride hist_cap, as the loop keeps them (one entry more: never an empty allocation)
    std::vector<double> hh((size_t)kMultiMax * hist_cap + 1, 0.0);
    for (int c = 0; c < nrhs && hist_cap > 0; ++c) std::copy(hist + (size_t)c * hist_cap, hist + (size_t)(c + 1) * hist_cap, hh.begin() + (size_t)c * hist_cap);
    DBuf dh(E, hh.size(), hh.data());
    if (!st.ok() || !p0.p || !p1.p || !dh.p) return fail(SPARSH_ENODEV, "device allocation or H2D copy failed");
    launch_finalize_mbicg((MbicgFin)code, W, nrhs, p0.p, n0, part1 ? p1.p : nullptr, part1 ? n1 : 0, st.s, tol, hist_cap > 0 ? dh.p : nullptr,
                          hist_cap, it, E.stream());
    int f[3 * kMultiMax];
    bool ok = st.scal.get(scal) && dh.get(hh.data()) && hipMemcpy(f, st.flags.p, sizeof(f), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return done(E, false);
    for (int c = 0; c < nrhs; ++c) {
        frozen[c] = f[c];
        iters[c] = f[kMultiMax + c];
        status[c] = f[2 * kMultiMax + c];
        if (hist_cap > 0) std::copy(hh.begin() + (size_t)c * hist_cap, hh.begin() + (size_t)(c + 1) * hist_cap, hist + (size_t)c * hist_cap);
    }
    for (int c = nrhs; c < W; ++c)
        if (!f[c]) return fail(SPARSH_ENUMERIC, "a padding column came back running");
    return done(E, true);
}

}  // extern "C"
