// Instrument channels (include/pyrad_hip.h, "instrument channels"): argument checking and the launch of lbl_ils_convolve_dev.
// The kernel is K8 of lbl_kernels.hip; the context's internals are reached through the hooks at the end of lbl_api.hip, as
// lbl_column_transport.hip reaches them.
#include "../../include/pyrad_hip.h"
#include "lbl_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <numeric>
#include <stdexcept>
#include <vector>

namespace lbl {
int comm_fail(lbl_ctx* ctx, int code, const char* msg);
int ctx_device(lbl_ctx* ctx);
hipStream_t ctx_stream(lbl_ctx* ctx);
int ctx_device_args(lbl_ctx* ctx, const void* host, size_t bytes, void** dptr);
int ctx_check_buffer(lbl_ctx* ctx, lbl_buffer* b, int64_t n, const char* what, bool required);
double* buffer_data(lbl_buffer* buf);
double grid_step(double lo, double hi, int64_t n);
}

using namespace lbl;

static int ils_fail(lbl_ctx* ctx, int code, const char* fmt, ...) {
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

extern "C" int lbl_ils_convolve_dev(lbl_ctx* ctx, double range_min, double range_max, int64_t n, int n_rows,
                                    lbl_buffer* const* src, const int64_t* src_offset, int64_t n_channels,
                                    const double* position, const double* width, const int64_t* first, const int64_t* count,
                                    int shape, int n_table, double table_half, const double* table, lbl_buffer* out) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    if (n < 0) return ils_fail(ctx, LBL_ERR_BAD_ARG, "negative n");
    if (n_rows < 1 || n_rows > kMaxIlsRows) return ils_fail(ctx, LBL_ERR_BAD_ARG, "1..%d rows", kMaxIlsRows);
    if (n_channels < 1 || n_channels > kMaxIlsChannels) return ils_fail(ctx, LBL_ERR_BAD_ARG, "1..%d channels", kMaxIlsChannels);
    if (shape < 0 || shape >= ILS_SHAPES) return ils_fail(ctx, LBL_ERR_BAD_ARG, "unknown line shape %d", shape);
    if (!src || !src_offset || !position || !first || !count) return ils_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    if (shape != ILS_TABLE && !width) return ils_fail(ctx, LBL_ERR_BAD_ARG, "NULL width");
    if (shape == ILS_TABLE) {
        if (n_table < 2 || n_table > kMaxIlsTable) return ils_fail(ctx, LBL_ERR_BAD_ARG, "a table of 2..%d values", kMaxIlsTable);
        if (!(table_half > 0)) return ils_fail(ctx, LBL_ERR_BAD_ARG, "table_half must be > 0");
        if (!table) return ils_fail(ctx, LBL_ERR_BAD_ARG, "NULL table");
    } else {
        n_table = 0;
    }
    for (int64_t c = 0; c < n_channels; ++c) {
        if (first[c] < 0 || count[c] < 1 || count[c] > n - first[c])
            return ils_fail(ctx, LBL_ERR_BAD_ARG, "channel %lld: support empty or outside [0, n)", (long long)c);
        if (shape != ILS_TABLE && !(width[c] > 0))
            return ils_fail(ctx, LBL_ERR_BAD_ARG, "channel %lld: width must be > 0", (long long)c);
    }
    int rc;
    for (int r = 0; r < n_rows; ++r) {
        if (!src[r]) return ils_fail(ctx, LBL_ERR_BAD_ARG, "row %d is NULL", r);
        if (src_offset[r] < 0 || src_offset[r] > INT64_MAX - n) return ils_fail(ctx, LBL_ERR_BAD_ARG, "row %d: offset out of range", r);
        if ((rc = ctx_check_buffer(ctx, src[r], src_offset[r] + n, "row", true))) return rc;
    }
    if ((rc = ctx_check_buffer(ctx, out, (int64_t)n_rows * n_channels, "out", true))) return rc;

    // the argument block: header, rows, position, width, first, count, order, table
    const size_t C = (size_t)n_channels;
    IlsArgs a;
    memset(&a, 0, sizeof a);
    size_t off = round8(sizeof a);
    a.off_rows = (long long)off;     off += (size_t)n_rows * sizeof(double*);
    a.off_position = (long long)off; off += C * sizeof(double);
    a.off_width = (long long)off;    off += C * sizeof(double);
    a.off_first = (long long)off;    off += C * sizeof(long long);
    a.off_count = (long long)off;    off += C * sizeof(long long);
    a.off_order = (long long)off;    off += round8(C * sizeof(int32_t));
    a.off_table = (long long)off;    off += (size_t)n_table * sizeof(double);
    a.out = buffer_data(out);
    a.step = grid_step(range_min, range_max, n);
    a.table_half = shape == ILS_TABLE ? table_half : 0.0;
    a.table_rdx = shape == ILS_TABLE ? (double)(n_table - 1) / (2.0 * table_half) : 0.0;
    a.n_channels = n_channels;
    a.n_rows = n_rows;
    a.n_table = n_table;
    a.chunk = (int32_t)((n_channels + 7) / 8);
    std::vector<char> blk(off, 0);
    memcpy(blk.data(), &a, sizeof a);
    const double** rows = (const double**)(blk.data() + a.off_rows);
    for (int r = 0; r < n_rows; ++r) rows[r] = buffer_data(src[r]) + src_offset[r];
    memcpy(blk.data() + a.off_position, position, C * sizeof(double));
    if (shape != ILS_TABLE) memcpy(blk.data() + a.off_width, width, C * sizeof(double));
    long long* f = (long long*)(blk.data() + a.off_first);
    long long* k = (long long*)(blk.data() + a.off_count);
    for (size_t c = 0; c < C; ++c) { f[c] = first[c]; k[c] = count[c]; }
    // neighbours in the dispatch order share most of their support (K8's XCD mapping)
    int32_t* order = (int32_t*)(blk.data() + a.off_order);
    std::iota(order, order + C, 0);
    std::stable_sort(order, order + C, [&](int32_t x, int32_t y) { return first[x] < first[y]; });
    if (n_table) memcpy(blk.data() + a.off_table, table, (size_t)n_table * sizeof(double));

    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, blk.data(), blk.size(), &d_args))) return rc;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return ils_fail(ctx, LBL_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    launch_ils_convolve((const IlsArgs*)d_args, shape, n_rows, n_channels, ctx_stream(ctx));
    e = hipGetLastError();
    if (e != hipSuccess) return ils_fail(ctx, LBL_ERR_HIP, "ils_convolve_kernel: %s", hipGetErrorString(e));
    return LBL_OK;
} LBL_GUARD_END(ctx)
