// k-distributions (include/pyrad_hip.h, "k-distributions"): argument checking and the launches of lbl_rank_order_dev and
// lbl_ranked_means_dev.  The kernels are K9 of lbl_kernels.hip; the context's internals are reached through the hooks at the
// end of lbl_api.hip, as lbl_instrument.hip reaches them.
#include "../../include/pyrad_hip.h"
#include "lbl_device.h"

#include <hip/hip_runtime.h>

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
int ctx_device_args(lbl_ctx* ctx, const void* host, size_t bytes, void** dptr);
int ctx_check_buffer(lbl_ctx* ctx, lbl_buffer* b, int64_t n, const char* what, bool required);
double* buffer_data(lbl_buffer* buf);
}

using namespace lbl;

static int kd_fail(lbl_ctx* ctx, int code, const char* fmt, ...) {
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
    catch (const std::exception& e) { return comm_fail((ctx_expr), LBL_ERR_STATE, e.what()); }                    \
    catch (...) { return comm_fail((ctx_expr), LBL_ERR_STATE, "unknown C++ exception"); }

static size_t round8(size_t b) { return (b + 7) & ~(size_t)7; }

// what both entry points check of their rows and bands; s_total: the length of a row's band-major output
static int check_rows_bands(lbl_ctx* ctx, int64_t n, int n_rows, int n_bands, const int64_t* band_first, const int64_t* band_count,
                            int64_t* s_total) {
    if (n < 1) return kd_fail(ctx, LBL_ERR_BAD_ARG, "n must be >= 1");
    if (n_rows < 1 || n_rows > kMaxKdistRows) return kd_fail(ctx, LBL_ERR_BAD_ARG, "1..%d rows", kMaxKdistRows);
    if (n_bands < 1 || n_bands > kMaxKdistBands) return kd_fail(ctx, LBL_ERR_BAD_ARG, "1..%d bands", kMaxKdistBands);
    if (!band_count) return kd_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    int64_t total = 0;
    for (int b = 0; b < n_bands; ++b) {
        const int64_t f = band_first ? band_first[b] : 0;
        if (f < 0 || band_count[b] < 1 || band_count[b] > n - f)
            return kd_fail(ctx, LBL_ERR_BAD_ARG, "band %d: empty or outside [0, n)", b);
        if (band_count[b] > INT32_MAX) return kd_fail(ctx, LBL_ERR_BAD_ARG, "band %d: more than 2^31 - 1 points", b);
        total += band_count[b];
    }
    *s_total = total;
    return LBL_OK;
}

static int check_row_buffers(lbl_ctx* ctx, int n_rows, lbl_buffer* const* buf, const int64_t* offset, int64_t len, const char* what) {
    for (int r = 0; r < n_rows; ++r) {
        if (!buf[r]) return kd_fail(ctx, LBL_ERR_BAD_ARG, "%s %d is NULL", what, r);
        if (offset[r] < 0 || offset[r] > INT64_MAX - len) return kd_fail(ctx, LBL_ERR_BAD_ARG, "%s %d: offset out of range", what, r);
        if (int rc = ctx_check_buffer(ctx, buf[r], offset[r] + len, what, true)) return rc;
    }
    return LBL_OK;
}

static bool needs_merge(int n_bands, const int64_t* band_count) {
    for (int b = 0; b < n_bands; ++b)
        if (band_count[b] > kKdistTile) return true;
    return false;
}

extern "C" int lbl_rank_order_workspace(int n_rows, int64_t n, int n_bands, const int64_t* band_count, int64_t* doubles) {
    int64_t s_total = 0;
    if (!doubles) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "doubles is NULL");
    if (int rc = check_rows_bands(nullptr, n, n_rows, n_bands, nullptr, band_count, &s_total)) return rc;
    // two sets of (8-byte key, 4-byte index) per point of the output, none when every band is sorted by one workgroup
    *doubles = needs_merge(n_bands, band_count) ? 3 * (int64_t)n_rows * s_total : 0;
    return LBL_OK;
}

extern "C" int lbl_rank_order_dev(lbl_ctx* ctx, int64_t n, int n_rows, lbl_buffer* const* src, const int64_t* src_offset,
                                  int n_bands, const int64_t* band_first, const int64_t* band_count,
                                  lbl_buffer* work, lbl_buffer* order, lbl_buffer* sorted) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    if (!src || !src_offset || !band_first || !band_count) return kd_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    int64_t s_total = 0;
    int rc;
    if ((rc = check_rows_bands(ctx, n, n_rows, n_bands, band_first, band_count, &s_total))) return rc;
    if ((rc = check_row_buffers(ctx, n_rows, src, src_offset, n, "row"))) return rc;
    const int64_t N = (int64_t)n_rows * s_total;
    const bool merge = needs_merge(n_bands, band_count);
    if ((rc = ctx_check_buffer(ctx, order, N, "order", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, sorted, N, "sorted", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, work, merge ? 3 * N : 0, "work", merge))) return rc;

    RankArgs a;
    memset(&a, 0, sizeof a);
    a.off_rows = (long long)round8(sizeof a);
    a.order = buffer_data(order);
    a.sorted = sorted ? buffer_data(sorted) : nullptr;
    if (merge) {
        unsigned long long* w = (unsigned long long*)buffer_data(work);
        a.keys[0] = w;
        a.keys[1] = w + N;
        a.idx[0] = (unsigned int*)(w + 2 * N);
        a.idx[1] = a.idx[0] + N;
    }
    a.s_total = s_total;
    a.n_rows = n_rows;
    a.n_bands = n_bands;
    int64_t at = 0;
    for (int b = 0; b < n_bands; ++b) {
        a.first[b] = band_first[b];
        a.count[b] = band_count[b];
        a.s_start[b] = at;
        at += band_count[b];
        int P = 0;
        while (((int64_t)kKdistTile << P) < band_count[b]) ++P;
        a.passes[b] = P;                                   // <= kKdistMaxPasses: a band holds less than 2^31 points
        const int32_t items = (int32_t)((band_count[b] + kKdistTile - 1) / kKdistTile);      // <= 2^20 a band
        a.item_start[0][b + 1] = a.item_start[0][b] + items;
        for (int p = 0; p < kKdistMaxPasses; ++p) a.item_start[p + 1][b + 1] = a.item_start[p + 1][b] + (P > p ? items : 0);
    }
    std::vector<char> blk((size_t)a.off_rows + (size_t)n_rows * sizeof(double*), 0);
    memcpy(blk.data(), &a, sizeof a);
    const double** rows = (const double**)(blk.data() + a.off_rows);
    for (int r = 0; r < n_rows; ++r) rows[r] = buffer_data(src[r]) + src_offset[r];

    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, blk.data(), blk.size(), &d_args))) return rc;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return kd_fail(ctx, LBL_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    launch_kdist_rank((const RankArgs*)d_args, a, ctx_stream(ctx));
    e = hipGetLastError();
    if (e != hipSuccess) return kd_fail(ctx, LBL_ERR_HIP, "kdist rank kernels: %s", hipGetErrorString(e));
    return LBL_OK;
} LBL_GUARD_END(ctx)

// the intervals of all bands, band after band, and the partial sums they need; fills `iv` (closed by one more entry) when given
static int check_intervals(lbl_ctx* ctx, int n_bands, const int64_t* band_count, const int32_t* n_intervals, const int64_t* edges,
                           const int64_t* s_start, std::vector<MeansInterval>* iv, int64_t* g_total, int64_t* n_chunks) {
    if (!n_intervals || !edges) return kd_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    int64_t g = 0, chunks = 0;
    const int64_t* e = edges;
    for (int b = 0; b < n_bands; ++b) {
        const int G = n_intervals[b];
        if (G < 1 || G > kMaxKdistIntervals) return kd_fail(ctx, LBL_ERR_BAD_ARG, "band %d: 1..%d intervals", b, kMaxKdistIntervals);
        if (e[0] != 0 || e[G] != band_count[b])
            return kd_fail(ctx, LBL_ERR_BAD_ARG, "band %d: the rank edges must run from 0 to the band's count", b);
        for (int i = 0; i < G; ++i) {
            if (e[i + 1] <= e[i]) return kd_fail(ctx, LBL_ERR_BAD_ARG, "band %d: rank edges not strictly increasing at %d", b, i);
            if (iv) iv->push_back(MeansInterval{(long long)((s_start ? s_start[b] : 0) + e[i]), (long long)(e[i + 1] - e[i]), b, (int32_t)chunks});
            chunks += (e[i + 1] - e[i] + kKdistTile - 1) / kKdistTile;
        }
        g += G;
        e += G + 1;
    }
    if (iv) iv->push_back(MeansInterval{0, 0, n_bands, (int32_t)chunks});
    *g_total = g;
    *n_chunks = chunks;                                    // <= 64 x (2^20 + 256)
    return LBL_OK;
}

extern "C" int lbl_ranked_means_workspace(int n_rows, int n_bands, const int64_t* band_count, const int32_t* n_intervals,
                                          const int64_t* edges, int64_t* doubles) {
    if (!doubles) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "doubles is NULL");
    if (n_rows < 1 || n_rows > kMaxKdistRows) return kd_fail(nullptr, LBL_ERR_BAD_ARG, "1..%d rows", kMaxKdistRows);
    if (n_bands < 1 || n_bands > kMaxKdistBands || !band_count) return kd_fail(nullptr, LBL_ERR_BAD_ARG, "1..%d bands", kMaxKdistBands);
    int64_t g_total = 0, n_chunks = 0;
    if (int rc = check_intervals(nullptr, n_bands, band_count, n_intervals, edges, nullptr, nullptr, &g_total, &n_chunks)) return rc;
    *doubles = (int64_t)n_rows * n_chunks;
    return LBL_OK;
}

extern "C" int lbl_ranked_means_dev(lbl_ctx* ctx, int64_t n, int n_rows, lbl_buffer* const* src, const int64_t* src_offset,
                                    lbl_buffer* const* order, const int64_t* order_offset,
                                    int n_bands, const int64_t* band_first, const int64_t* band_count,
                                    const int32_t* n_intervals, const int64_t* edges, lbl_buffer* work,
                                    lbl_buffer* mean, int64_t mean_offset, lbl_buffer* lower, int64_t lower_offset) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    if (!src || !src_offset || !order || !order_offset || !band_first || !band_count)
        return kd_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    int64_t s_total = 0, g_total = 0, n_chunks = 0;
    int rc;
    if ((rc = check_rows_bands(ctx, n, n_rows, n_bands, band_first, band_count, &s_total))) return rc;
    MeansArgs a;
    memset(&a, 0, sizeof a);
    int64_t at = 0, s_start[kMaxKdistBands];
    for (int b = 0; b < n_bands; ++b) {
        a.first[b] = band_first[b];
        a.count[b] = band_count[b];
        a.s_start[b] = s_start[b] = at;
        at += band_count[b];
    }
    std::vector<MeansInterval> iv;
    if ((rc = check_intervals(ctx, n_bands, band_count, n_intervals, edges, s_start, &iv, &g_total, &n_chunks))) return rc;
    if ((rc = check_row_buffers(ctx, n_rows, src, src_offset, n, "row"))) return rc;
    if ((rc = check_row_buffers(ctx, n_rows, order, order_offset, s_total, "order"))) return rc;
    const int64_t n_mean = (int64_t)n_rows * g_total, n_lower = (int64_t)n_rows * (g_total + n_bands);
    if (mean_offset < 0 || mean_offset > INT64_MAX - n_mean) return kd_fail(ctx, LBL_ERR_BAD_ARG, "mean: offset out of range");
    if (lower && (lower_offset < 0 || lower_offset > INT64_MAX - n_lower)) return kd_fail(ctx, LBL_ERR_BAD_ARG, "lower: offset out of range");
    if ((rc = ctx_check_buffer(ctx, mean, mean_offset + n_mean, "mean", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, lower, lower ? lower_offset + n_lower : 0, "lower", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, work, (int64_t)n_rows * n_chunks, "work", true))) return rc;

    // the argument block: header, rows, orders, intervals
    size_t off = round8(sizeof a);
    a.off_rows = (long long)off;      off += (size_t)n_rows * sizeof(double*);
    a.off_orders = (long long)off;    off += (size_t)n_rows * sizeof(double*);
    a.off_intervals = (long long)off; off += iv.size() * sizeof(MeansInterval);
    a.partial = buffer_data(work);
    a.mean = buffer_data(mean) + mean_offset;
    a.lower = lower ? buffer_data(lower) + lower_offset : nullptr;
    a.n_rows = n_rows;
    a.n_bands = n_bands;
    a.g_total = (int32_t)g_total;
    a.n_chunks = (int32_t)n_chunks;
    for (int b = 0; b < n_bands; ++b) a.g_start[b + 1] = a.g_start[b] + n_intervals[b];
    std::vector<char> blk(off, 0);
    memcpy(blk.data(), &a, sizeof a);
    const double** rows = (const double**)(blk.data() + a.off_rows);
    const double** orders = (const double**)(blk.data() + a.off_orders);
    for (int r = 0; r < n_rows; ++r) {
        rows[r] = buffer_data(src[r]) + src_offset[r];
        orders[r] = buffer_data(order[r]) + order_offset[r];
    }
    memcpy(blk.data() + a.off_intervals, iv.data(), iv.size() * sizeof(MeansInterval));

    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, blk.data(), blk.size(), &d_args))) return rc;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return kd_fail(ctx, LBL_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    launch_kdist_means((const MeansArgs*)d_args, a, ctx_stream(ctx));
    e = hipGetLastError();
    if (e != hipSuccess) return kd_fail(ctx, LBL_ERR_HIP, "kdist means kernels: %s", hipGetErrorString(e));
    return LBL_OK;
} LBL_GUARD_END(ctx)
