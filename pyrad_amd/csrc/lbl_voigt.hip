// True Voigt line shape (include/pyrad_hip.h, "true Voigt line shape"): argument checking, staging and the launches of
// lbl_xsec_voigt_dev, lbl_xsec_voigt_dt_dev, lbl_voigt_function_dev and lbl_voigt_gradient_dev.  The kernels are K2v and K2v-T
// of lbl_kernels.hip; the context's internals are reached
// through the hooks at the end of lbl_api.hip, as lbl_kdist.hip reaches them.
#include "../../include/pyrad_hip.h"
#include "lbl_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>
#include <vector>

namespace lbl {
int comm_fail(lbl_ctx* ctx, int code, const char* msg);
int ctx_device(lbl_ctx* ctx);
hipStream_t ctx_stream(lbl_ctx* ctx);
lbl_ctx* buffer_ctx(lbl_buffer* buf);
int ctx_device_args(lbl_ctx* ctx, const void* host, size_t bytes, void** dptr);
int ctx_check_buffer(lbl_ctx* ctx, lbl_buffer* b, int64_t n, const char* what, bool required);
double* buffer_data(lbl_buffer* buf);
int ctx_check_grid(lbl_ctx* ctx, const lbl_grid* g);
int ctx_check_lines(lbl_ctx* ctx, const lbl_lines* lines, int at);
int64_t lines_count(const lbl_lines* lines);
void prep_job_fill(PrepJob* p, const lbl_lines* L, const lbl_iso_params* iso, const lbl_grid* grid);
int ctx_voigt_scratch(lbl_ctx* ctx, size_t bytes, void** dptr);
int ctx_regime_blocks(lbl_ctx* ctx, int n_lists, int blocks_per_list, unsigned int** d_counts);
void ctx_regime_batch(lbl_ctx* ctx, int n_lists, int blocks_per_list, const int* list_blocks);
void* ctx_profile_begin(lbl_ctx* ctx, int kind);
void ctx_profile_end(lbl_ctx* ctx, int kind, void* start);
}

using namespace lbl;

static int vg_fail(lbl_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return comm_fail(ctx, code, buf);
}

// no C++ exception crosses the C boundary (see lbl_api.hip)
#define LBL_GUARD_END(ctx_expr)                                                                                   \
    catch (const std::bad_alloc&) { return comm_fail((ctx_expr), LBL_ERR_OOM, "host allocation failed"); }        \
    catch (const std::length_error&) { return comm_fail((ctx_expr), LBL_ERR_OOM, "host allocation too large"); }  \
    catch (const std::exception& e) { return comm_fail((ctx_expr), LBL_ERR_STATE, e.what()); }                    \
    catch (...) { return comm_fail((ctx_expr), LBL_ERR_STATE, "unknown C++ exception"); }

// kernel classes of lbl_profile_read that a Voigt batch is timed under
enum { PROF_PREP = 0, PROF_ACCUM = 1, PROF_REGRID = 2 };

static size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
static bool needs_regrid(const lbl_grid& g) { return !(g.resolution == g.base_resolution && g.n_work == g.n_base); }

extern "C" int lbl_xsec_voigt_dev(lbl_ctx* ctx, int n_jobs, lbl_lines* const* lines, const lbl_iso_params* iso,
                                  const lbl_grid* grid, lbl_buffer* const* out) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    if (n_jobs < 0) return vg_fail(ctx, LBL_ERR_BAD_ARG, "negative job count");
    if (n_jobs > LBL_MAX_JOBS) return vg_fail(ctx, LBL_ERR_BAD_ARG, "at most %d jobs per batch", LBL_MAX_JOBS);
    if (n_jobs == 0) return LBL_OK;
    if (!lines || !iso || !grid || !out) return vg_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    int rc;
    // everything is checked before anything is enqueued; the scratch layout: records | centre indices | work grids
    std::vector<size_t> line_off(n_jobs), work_off(n_jobs);
    size_t tot_lines = 0, tot_work = 0;
    int64_t max_lines = 0;
    long long max_points = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (!out[j] || buffer_ctx(out[j]) != ctx) return vg_fail(ctx, LBL_ERR_STATE, "job %d: output buffer missing or from another context", j);
        if ((rc = ctx_check_grid(ctx, &grid[j]))) return rc;
        if ((rc = ctx_check_buffer(ctx, out[j], grid[j].n_base, "output buffer (n_base doubles)", true))) return rc;
        if ((rc = ctx_check_lines(ctx, lines[j], j))) return rc;
        if (!(iso[j].T > 0) || !(iso[j].P > 0) || !(iso[j].molmass > 0) || !(iso[j].Q_T > 0))
            return vg_fail(ctx, LBL_ERR_BAD_ARG, "line list %d: T, P, molmass and Q_T must be > 0", j);
        line_off[j] = tot_lines;
        tot_lines += (size_t)lines_count(lines[j]);
        max_lines = std::max(max_lines, lines_count(lines[j]));
        work_off[j] = tot_work;
        if (needs_regrid(grid[j])) tot_work += (size_t)grid[j].n_work;
        max_points = std::max<long long>(max_points, grid[j].shard_count > 0 ? grid[j].shard_count : grid[j].n_work);
    }
    const size_t rec_bytes = round256(std::max<size_t>(tot_lines, 1) * sizeof(VoigtRec));
    const size_t cidx_bytes = round256(std::max<size_t>(tot_lines, 1) * sizeof(int32_t));
    char* scratch = nullptr;
    if ((rc = ctx_voigt_scratch(ctx, rec_bytes + cidx_bytes + std::max<size_t>(tot_work, 1) * sizeof(double), (void**)&scratch))) return rc;
    const int blocks_per_list = (int)((max_lines + 255) / 256);
    unsigned int* d_counts = nullptr;
    if ((rc = ctx_regime_blocks(ctx, n_jobs, blocks_per_list, &d_counts))) return rc;
    VoigtRec* d_rec = (VoigtRec*)scratch;
    int32_t* d_cidx = (int32_t*)(scratch + rec_bytes);
    double* d_work = (double*)(scratch + rec_bytes + cidx_bytes);

    // the argument block: PrepJob[n_jobs], VoigtJob[n_jobs]
    const size_t prep_bytes = ((size_t)n_jobs * sizeof(PrepJob) + 15) & ~(size_t)15;
    std::vector<char> blk(prep_bytes + (size_t)n_jobs * sizeof(VoigtJob), 0);
    PrepJob* hp = (PrepJob*)blk.data();
    VoigtJob* hv = (VoigtJob*)(blk.data() + prep_bytes);
    std::vector<int> list_blocks(n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        prep_job_fill(&hp[j], lines[j], &iso[j], &grid[j]);
        hp[j].block_counts = d_counts + (size_t)j * blocks_per_list * 3;
        list_blocks[j] = (int)((lines_count(lines[j]) + 255) / 256);
        VoigtJob& v = hv[j];
        v.rec = d_rec + line_off[j];
        v.cidx = d_cidx + line_off[j];
        v.out = needs_regrid(grid[j]) ? d_work + work_off[j] : buffer_data(out[j]);
        v.n_lines = (int32_t)lines_count(lines[j]);
        v.H = (int32_t)std::max<long long>(grid[j].window - 2, 0);
        const long long first = grid[j].shard_count > 0 ? grid[j].shard_first : 0;
        const long long count = grid[j].shard_count > 0 ? grid[j].shard_count : grid[j].n_work;
        v.p_begin = (int32_t)first;
        v.p_end = (int32_t)(first + count);
    }
    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, blk.data(), blk.size(), &d_args))) return rc;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return vg_fail(ctx, LBL_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    const PrepJob* dp = (const PrepJob*)d_args;
    const VoigtJob* dv = (const VoigtJob*)((const char*)d_args + prep_bytes);
    hipStream_t s = ctx_stream(ctx);
    void* ev = ctx_profile_begin(ctx, PROF_PREP);
    launch_voigt_prep(dp, dv, n_jobs, (int)max_lines, s);
    ctx_profile_end(ctx, PROF_PREP, ev);
    ctx_regime_batch(ctx, n_jobs, blocks_per_list, list_blocks.data());
    ev = ctx_profile_begin(ctx, PROF_ACCUM);
    launch_voigt_accumulate(dv, n_jobs, max_points, s);
    ctx_profile_end(ctx, PROF_ACCUM, ev);
    for (int j = 0; j < n_jobs; ++j) {
        if (!needs_regrid(grid[j])) continue;
        ev = ctx_profile_begin(ctx, PROF_REGRID);
        launch_regrid(d_work + work_off[j], grid[j].n_work, buffer_data(out[j]), grid[j].n_base, grid[j].range_min, grid[j].range_max, s);
        ctx_profile_end(ctx, PROF_REGRID, ev);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return vg_fail(ctx, LBL_ERR_HIP, "Voigt kernels: %s", hipGetErrorString(e));
    return LBL_OK;
} LBL_GUARD_END(ctx)

extern "C" int lbl_voigt_function_dev(lbl_ctx* ctx, lbl_buffer* x, lbl_buffer* y, int64_t n, lbl_buffer* out) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    if (n < 0) return vg_fail(ctx, LBL_ERR_BAD_ARG, "negative n");
    int rc;
    if ((rc = ctx_check_buffer(ctx, x, n, "x", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, y, n, "y", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, out, n, "out", true))) return rc;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return vg_fail(ctx, LBL_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    launch_voigt_function(buffer_data(x), buffer_data(y), n, buffer_data(out), ctx_stream(ctx));
    e = hipGetLastError();
    if (e != hipSuccess) return vg_fail(ctx, LBL_ERR_HIP, "voigt function kernel: %s", hipGetErrorString(e));
    return LBL_OK;
} LBL_GUARD_END(ctx)

// d(sigma)/dT under the Voigt shape: lbl_xsec_voigt_dev's checks, scratch layout and launches with K2v-T's records (48 bytes)
// and kernels; no regime counters
extern "C" int lbl_xsec_voigt_dt_dev(lbl_ctx* ctx, int n_jobs, lbl_lines* const* lines, const lbl_iso_params* iso,
                                     const double* dlnw_dT, const lbl_grid* grid, lbl_buffer* const* out) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    if (n_jobs < 0) return vg_fail(ctx, LBL_ERR_BAD_ARG, "negative job count");
    if (n_jobs > LBL_MAX_JOBS) return vg_fail(ctx, LBL_ERR_BAD_ARG, "at most %d jobs per batch", LBL_MAX_JOBS);
    if (n_jobs == 0) return LBL_OK;
    if (!lines || !iso || !dlnw_dT || !grid || !out) return vg_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    int rc;
    std::vector<size_t> line_off(n_jobs), work_off(n_jobs);
    size_t tot_lines = 0, tot_work = 0;
    int64_t max_lines = 0;
    long long max_points = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (!out[j] || buffer_ctx(out[j]) != ctx) return vg_fail(ctx, LBL_ERR_STATE, "job %d: output buffer missing or from another context", j);
        if ((rc = ctx_check_grid(ctx, &grid[j]))) return rc;
        if ((rc = ctx_check_buffer(ctx, out[j], grid[j].n_base, "output buffer (n_base doubles)", true))) return rc;
        if ((rc = ctx_check_lines(ctx, lines[j], j))) return rc;
        if (!(iso[j].T > 0) || !(iso[j].P > 0) || !(iso[j].molmass > 0) || !(iso[j].Q_T > 0))
            return vg_fail(ctx, LBL_ERR_BAD_ARG, "line list %d: T, P, molmass and Q_T must be > 0", j);
        if (!std::isfinite(dlnw_dT[j])) return vg_fail(ctx, LBL_ERR_BAD_ARG, "line list %d: dlnw_dT must be finite", j);
        line_off[j] = tot_lines;
        tot_lines += (size_t)lines_count(lines[j]);
        max_lines = std::max(max_lines, lines_count(lines[j]));
        work_off[j] = tot_work;
        if (needs_regrid(grid[j])) tot_work += (size_t)grid[j].n_work;
        max_points = std::max<long long>(max_points, grid[j].shard_count > 0 ? grid[j].shard_count : grid[j].n_work);
    }
    const size_t rec_bytes = round256(std::max<size_t>(tot_lines, 1) * sizeof(VoigtDTRec));
    const size_t cidx_bytes = round256(std::max<size_t>(tot_lines, 1) * sizeof(int32_t));
    char* scratch = nullptr;
    if ((rc = ctx_voigt_scratch(ctx, rec_bytes + cidx_bytes + std::max<size_t>(tot_work, 1) * sizeof(double), (void**)&scratch))) return rc;
    VoigtDTRec* d_rec = (VoigtDTRec*)scratch;
    int32_t* d_cidx = (int32_t*)(scratch + rec_bytes);
    double* d_work = (double*)(scratch + rec_bytes + cidx_bytes);

    // the argument block: PrepJob[n_jobs], VoigtDTJob[n_jobs]
    const size_t prep_bytes = ((size_t)n_jobs * sizeof(PrepJob) + 15) & ~(size_t)15;
    std::vector<char> blk(prep_bytes + (size_t)n_jobs * sizeof(VoigtDTJob), 0);
    PrepJob* hp = (PrepJob*)blk.data();
    VoigtDTJob* hv = (VoigtDTJob*)(blk.data() + prep_bytes);
    for (int j = 0; j < n_jobs; ++j) {
        prep_job_fill(&hp[j], lines[j], &iso[j], &grid[j]);
        hp[j].block_counts = nullptr;                       // (K2v-T counts no regimes)
        VoigtDTJob& v = hv[j];
        v.rec = d_rec + line_off[j];
        v.cidx = d_cidx + line_off[j];
        v.out = needs_regrid(grid[j]) ? d_work + work_off[j] : buffer_data(out[j]);
        v.dlnw_dT = dlnw_dT[j];
        v.bx = -0.5 * hp[j].inv_T;
        v.n_lines = (int32_t)lines_count(lines[j]);
        v.H = (int32_t)std::max<long long>(grid[j].window - 2, 0);
        const long long first = grid[j].shard_count > 0 ? grid[j].shard_first : 0;
        const long long count = grid[j].shard_count > 0 ? grid[j].shard_count : grid[j].n_work;
        v.p_begin = (int32_t)first;
        v.p_end = (int32_t)(first + count);
    }
    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, blk.data(), blk.size(), &d_args))) return rc;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return vg_fail(ctx, LBL_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    const PrepJob* dp = (const PrepJob*)d_args;
    const VoigtDTJob* dv = (const VoigtDTJob*)((const char*)d_args + prep_bytes);
    hipStream_t s = ctx_stream(ctx);
    void* ev = ctx_profile_begin(ctx, PROF_PREP);
    launch_voigt_dT_prep(dp, dv, n_jobs, (int)max_lines, s);
    ctx_profile_end(ctx, PROF_PREP, ev);
    ev = ctx_profile_begin(ctx, PROF_ACCUM);
    launch_voigt_dT_accumulate(dv, n_jobs, max_points, s);
    ctx_profile_end(ctx, PROF_ACCUM, ev);
    for (int j = 0; j < n_jobs; ++j) {
        if (!needs_regrid(grid[j])) continue;
        ev = ctx_profile_begin(ctx, PROF_REGRID);
        launch_regrid(d_work + work_off[j], grid[j].n_work, buffer_data(out[j]), grid[j].n_base, grid[j].range_min, grid[j].range_max, s);
        ctx_profile_end(ctx, PROF_REGRID, ev);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return vg_fail(ctx, LBL_ERR_HIP, "Voigt derivative kernels: %s", hipGetErrorString(e));
    return LBL_OK;
} LBL_GUARD_END(ctx)

extern "C" int lbl_voigt_gradient_dev(lbl_ctx* ctx, lbl_buffer* x, lbl_buffer* y, int64_t n, lbl_buffer* K, lbl_buffer* GX,
                                      lbl_buffer* GY) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    if (n < 0) return vg_fail(ctx, LBL_ERR_BAD_ARG, "negative n");
    int rc;
    if ((rc = ctx_check_buffer(ctx, x, n, "x", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, y, n, "y", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, K, n, "K", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, GX, n, "GX", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, GY, n, "GY", true))) return rc;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return vg_fail(ctx, LBL_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    launch_voigt_gradient(buffer_data(x), buffer_data(y), n, buffer_data(K), buffer_data(GX), buffer_data(GY), ctx_stream(ctx));
    e = hipGetLastError();
    if (e != hipSuccess) return vg_fail(ctx, LBL_ERR_HIP, "voigt gradient kernel: %s", hipGetErrorString(e));
    return LBL_OK;
} LBL_GUARD_END(ctx)
