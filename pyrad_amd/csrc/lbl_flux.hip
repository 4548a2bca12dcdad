// Level fluxes of a column (include/pyrad_hip.h, "level fluxes"): argument checking and the launch sequence of
// lbl_column_flux_dev.  The kernels are K5c of lbl_kernels.hip; the context's internals are reached through the hooks at
// the end of lbl_api.hip, so that lbl_api.hip builds on its own (tests/host_shim) without this file's launcher.
#include "../../include/pyrad_hip.h"
#include "lbl_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <new>
#include <stdexcept>
#include <vector>

namespace lbl {
int comm_fail(lbl_ctx* ctx, int code, const char* msg);
int ctx_device(lbl_ctx* ctx);
hipStream_t ctx_stream(lbl_ctx* ctx);
bool ctx_sweep_ieee(lbl_ctx* ctx);
int ctx_device_args(lbl_ctx* ctx, const void* host, size_t bytes, void** dptr);
int ctx_reduction_scratch(lbl_ctx* ctx, size_t bytes, void** dptr);
int ctx_check_buffer(lbl_ctx* ctx, lbl_buffer* b, int64_t n, const char* what, bool required);
double* buffer_data(lbl_buffer* buf);
void planck_budget_constants(double T, double* pa, double* pbkT);
double grid_step(double lo, double hi, int64_t n);
}

using namespace lbl;

static int flux_fail(lbl_ctx* ctx, int code, const char* fmt, ...) {
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

#define FLUX_HIP_TRY(ctx, expr)                                                                                   \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return flux_fail(ctx, e_ == hipErrorOutOfMemory ? LBL_ERR_OOM : LBL_ERR_HIP, "%s: %s", #expr,         \
                             hipGetErrorString(e_));                                                              \
    } while (0)

extern "C" int lbl_column_flux_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                   const double* depth, double range_min, double range_max, int64_t n,
                                   lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top, int n_angles,
                                   const double* mu, const double* weight, int n_bands, const int64_t* band_first,
                                   const int64_t* band_count, lbl_buffer* level_flux, lbl_buffer* up_top,
                                   lbl_buffer* down_surface) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    if (n_layers < 0 || n_layers > kMaxLayers) return flux_fail(ctx, LBL_ERR_BAD_ARG, "at most %d layers", kMaxLayers);
    if (n < 0) return flux_fail(ctx, LBL_ERR_BAD_ARG, "negative n");
    if (n_layers > 0 && (!abs_coef || !T || !depth)) return flux_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    if (ctx_sweep_ieee(ctx))
        return flux_fail(ctx, LBL_ERR_BAD_ARG, "level fluxes exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)");
    if (n_angles < 1 || n_angles > kMaxFluxAngles) return flux_fail(ctx, LBL_ERR_BAD_ARG, "1..%d angles", kMaxFluxAngles);
    if (!mu || !weight) return flux_fail(ctx, LBL_ERR_BAD_ARG, "NULL angle set");
    if (n_bands < 1 || n_bands > kMaxFluxBands) return flux_fail(ctx, LBL_ERR_BAD_ARG, "1..%d bands", kMaxFluxBands);
    if (!band_first || !band_count) return flux_fail(ctx, LBL_ERR_BAD_ARG, "NULL band list");
    int rc;
    if ((rc = ctx_check_buffer(ctx, level_flux, (int64_t)n_bands * 2 * (n_layers + 1), "level_flux", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, I_surface, n, "I_surface", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, I_top, n, "I_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_top, n, "up_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, down_surface, n, "down_surface", false))) return rc;
    if (!I_surface && !(surface_T > 0)) return flux_fail(ctx, LBL_ERR_BAD_ARG, "need I_surface or surface_T > 0");
    for (int b = 0; b < n_bands; ++b)
        if (band_first[b] < 0 || band_count[b] < 1 || band_count[b] > n - band_first[b])
            return flux_fail(ctx, LBL_ERR_BAD_ARG, "band %d: empty or outside [0, n)", b);
    std::vector<char> blk(sizeof(FluxArgs), 0);
    FluxArgs* a = (FluxArgs*)blk.data();
    double pa = 0.0;
    for (int l = 0; l < n_layers; ++l) {
        if ((rc = ctx_check_buffer(ctx, abs_coef[l], n, "abs_coef", true))) return rc;
        if (!(T[l] > 0)) return flux_fail(ctx, LBL_ERR_BAD_ARG, "layer %d: T must be > 0", l);
        if (!(depth[l] >= 0)) return flux_fail(ctx, LBL_ERR_BAD_ARG, "layer %d: depth must be >= 0", l);
        a->abs_coef[l] = buffer_data(abs_coef[l]);
        a->depth[l] = depth[l];
        planck_budget_constants(T[l], &pa, &a->pbkT[l]);
        a->pbkT_min = l == 0 ? a->pbkT[l] : std::min(a->pbkT_min, a->pbkT[l]);
        a->pbkT_max = l == 0 ? a->pbkT[l] : std::max(a->pbkT_max, a->pbkT[l]);
    }
    for (int k = 0; k < n_angles; ++k) {
        if (!(mu[k] > 0 && mu[k] <= 1)) return flux_fail(ctx, LBL_ERR_BAD_ARG, "angle %d: mu must lie in (0, 1]", k);
        if (!std::isfinite(weight[k])) return flux_fail(ctx, LBL_ERR_BAD_ARG, "angle %d: weight must be finite", k);
        a->rmu[k] = 1.0 / mu[k];
        a->w[k] = weight[k];
    }
    planck_budget_constants(surface_T > 0 ? surface_T : 1.0, &pa, &a->pbk_surface);
    a->pa = pa;
    a->start = range_min; a->stop = range_max; a->step = grid_step(range_min, range_max, n);
    a->I_surface = I_surface ? buffer_data(I_surface) : nullptr;
    a->I_top = I_top ? buffer_data(I_top) : nullptr;
    a->up_top = up_top ? buffer_data(up_top) : nullptr;
    a->down_surface = down_surface ? buffer_data(down_surface) : nullptr;
    a->n = n;
    a->n_layers = n_layers; a->n_angles = n_angles;
    const int nv = 2 * (n_layers + 1);
    int64_t max_count = 0;
    for (int b = 0; b < n_bands; ++b) max_count = std::max(max_count, band_count[b]);
    void* partial = nullptr;
    if ((rc = ctx_reduction_scratch(ctx, (size_t)column_flux_partials(max_count) * nv * sizeof(double), &partial))) return rc;
    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, a, sizeof(FluxArgs), &d_args))) return rc;
    const hipStream_t s = ctx_stream(ctx);
    FLUX_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    // (points outside every band keep 0 in the spectra)
    if (up_top && n > 0) FLUX_HIP_TRY(ctx, hipMemsetAsync(a->up_top, 0, (size_t)n * sizeof(double), s));
    if (down_surface && n > 0) FLUX_HIP_TRY(ctx, hipMemsetAsync(a->down_surface, 0, (size_t)n * sizeof(double), s));
    // the bands one after another over one partial block: stream order keeps a band's final reduction ahead of the next band
    for (int b = 0; b < n_bands; ++b)
        launch_column_flux((const FluxArgs*)d_args, n_layers, n_angles, band_first[b], band_count[b], (double*)partial,
                           buffer_data(level_flux) + (size_t)b * nv, s);
    FLUX_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
} LBL_GUARD_END(ctx)
