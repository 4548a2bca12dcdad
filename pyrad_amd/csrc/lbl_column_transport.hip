// Column transport (include/pyrad_hip.h, "level fluxes", "Jacobians" and "ray paths"): argument checking and the launch
// sequences of lbl_column_flux_dev, lbl_column_jacobian_dev, lbl_ray_radiance_dev and lbl_ray_jacobian_dev, and of their
// variants over a reflecting surface, lbl_column_flux_surface_dev, lbl_ray_radiance_surface_dev, lbl_column_jacobian_surface_dev
// and lbl_ray_jacobian_surface_dev, of the linear-source variants lbl_column_flux_linear_dev and lbl_ray_radiance_linear_dev, and
// of their Jacobians lbl_column_jacobian_linear_dev and lbl_ray_jacobian_linear_dev, of the direct solar beam,
// lbl_column_solar_dev, of its two-stream multiple scattering, lbl_column_twostream_dev, of the thermal fluxes through
// scattering layers, lbl_column_flux_scatter_dev, of its Jacobians, lbl_column_jacobian_scatter_dev, and of the radiances
// through them, lbl_column_radiance_scatter_dev.
// The kernels are K5c, K5d, K5e, K5f, K5g, K5h, K5i, K5j, K5k, K5l, K5m, K5n, K5o and K5p of lbl_kernels.hip; the context's internals
// are reached through the hooks at the end of lbl_api.hip, so that lbl_api.hip builds on its own (tests/host_shim) without
// this file's launchers.
#include "../../include/pyrad_hip.h"
#include "lbl_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
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

static int column_fail(lbl_ctx* ctx, int code, const char* fmt, ...) {
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

#define COLUMN_HIP_TRY(ctx, expr)                                                                                 \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return column_fail(ctx, e_ == hipErrorOutOfMemory ? LBL_ERR_OOM : LBL_ERR_HIP, "%s: %s", #expr,       \
                               hipGetErrorString(e_));                                                            \
    } while (0)

// The arguments both entry points share (ctx non-NULL): checked in this order, then the ColumnRT part of the argument block
// filled.  `what` names the feature in the refusal under "sweep_ieee_divisions" 1.  With `pbkT_top` (the linear source) T holds
// two temperatures per layer, bottom and top edge, finite and > 0: pbkT receives the bottom edges, pbkT_top the top edges,
// and pbkT_min / pbkT_max cover both.
static int check_column(lbl_ctx* ctx, const char* what, ColumnRT* a, int n_layers, lbl_buffer* const* abs_coef,
                        const double* T, const double* depth, double range_min, double range_max, int64_t n,
                        lbl_buffer* I_surface, double surface_T, int n_angles, const double* mu, const double* weight,
                        int n_bands, const int64_t* band_first, const int64_t* band_count, double* pbkT_top = nullptr) {
    if (n_layers < 0 || n_layers > kMaxLayers) return column_fail(ctx, LBL_ERR_BAD_ARG, "at most %d layers", kMaxLayers);
    if (n < 0) return column_fail(ctx, LBL_ERR_BAD_ARG, "negative n");
    if (n_layers > 0 && (!abs_coef || !T || !depth)) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    if (ctx_sweep_ieee(ctx))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "%s exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)", what);
    if (n_angles < 1 || n_angles > kMaxFluxAngles) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d angles", kMaxFluxAngles);
    if (!mu || !weight) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL angle set");
    if (n_bands < 1 || n_bands > kMaxFluxBands) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d bands", kMaxFluxBands);
    if (!band_first || !band_count) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL band list");
    int rc;
    if ((rc = ctx_check_buffer(ctx, I_surface, n, "I_surface", false))) return rc;
    if (!I_surface && !(surface_T > 0)) return column_fail(ctx, LBL_ERR_BAD_ARG, "need I_surface or surface_T > 0");
    for (int b = 0; b < n_bands; ++b)
        if (band_first[b] < 0 || band_count[b] < 1 || band_count[b] > n - band_first[b])
            return column_fail(ctx, LBL_ERR_BAD_ARG, "band %d: empty or outside [0, n)", b);
    double pa = 0.0;
    for (int l = 0; l < n_layers; ++l) {
        if ((rc = ctx_check_buffer(ctx, abs_coef[l], n, "abs_coef", true))) return rc;
        const double Tl = pbkT_top ? T[2 * l] : T[l];
        if (pbkT_top && !(std::isfinite(Tl) && std::isfinite(T[2 * l + 1]) && Tl > 0 && T[2 * l + 1] > 0))
            return column_fail(ctx, LBL_ERR_BAD_ARG, "layer %d: both edge temperatures must be finite and > 0", l);
        if (!(Tl > 0)) return column_fail(ctx, LBL_ERR_BAD_ARG, "layer %d: T must be > 0", l);
        if (!(depth[l] >= 0)) return column_fail(ctx, LBL_ERR_BAD_ARG, "layer %d: depth must be >= 0", l);
        a->abs_coef[l] = buffer_data(abs_coef[l]);
        a->depth[l] = depth[l];
        planck_budget_constants(Tl, &pa, &a->pbkT[l]);
        a->pbkT_min = l == 0 ? a->pbkT[l] : std::min(a->pbkT_min, a->pbkT[l]);
        a->pbkT_max = l == 0 ? a->pbkT[l] : std::max(a->pbkT_max, a->pbkT[l]);
        if (pbkT_top) {
            planck_budget_constants(T[2 * l + 1], &pa, &pbkT_top[l]);
            a->pbkT_min = std::min(a->pbkT_min, pbkT_top[l]);
            a->pbkT_max = std::max(a->pbkT_max, pbkT_top[l]);
        }
    }
    for (int k = 0; k < n_angles; ++k) {
        if (!(mu[k] > 0 && mu[k] <= 1)) return column_fail(ctx, LBL_ERR_BAD_ARG, "angle %d: mu must lie in (0, 1]", k);
        if (!std::isfinite(weight[k])) return column_fail(ctx, LBL_ERR_BAD_ARG, "angle %d: weight must be finite", k);
        a->rmu[k] = 1.0 / mu[k];
        a->w[k] = weight[k];
    }
    planck_budget_constants(surface_T > 0 ? surface_T : 1.0, &pa, &a->pbk_surface);
    a->pa = pa;
    a->start = range_min; a->stop = range_max; a->step = grid_step(range_min, range_max, n);
    a->I_surface = I_surface ? buffer_data(I_surface) : nullptr;
    a->n = n;
    a->n_layers = n_layers; a->n_angles = n_angles;
    return LBL_OK;
}

// The launch sequence after every check: the argument block and the partial scratch for the widest band (`np` points per
// thread, nv values per partial), the optional spectra spec[0 .. NS) (spec_bytes each) and spec_n (n points) zeroed, then
// the bands one after another over one partial block: stream order keeps a band's final reduction ahead of the next band.
// launch_band(d_args, partial, b, s) enqueues band b.
template <class Args, size_t NS, class LaunchBand>
static int run_column(lbl_ctx* ctx, const Args* a, int np, int nv, int n_bands, const int64_t* band_count, double* const (&spec)[NS],
                      size_t spec_bytes, LaunchBand launch_band, double* spec_n = nullptr) {
    int64_t max_count = 0;
    for (int b = 0; b < n_bands; ++b) max_count = std::max(max_count, band_count[b]);
    void* partial = nullptr;
    int rc;
    if ((rc = ctx_reduction_scratch(ctx, (size_t)column_transport_partials(max_count, np) * nv * sizeof(double), &partial)))
        return rc;
    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, a, sizeof(Args), &d_args))) return rc;
    const hipStream_t s = ctx_stream(ctx);
    COLUMN_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    // (points outside every band keep 0 in the spectra)
    for (double* p : spec)
        if (p && spec_bytes) COLUMN_HIP_TRY(ctx, hipMemsetAsync(p, 0, spec_bytes, s));
    if (spec_n && a->n > 0) COLUMN_HIP_TRY(ctx, hipMemsetAsync(spec_n, 0, (size_t)a->n * sizeof(double), s));
    for (int b = 0; b < n_bands; ++b) launch_band((const Args*)d_args, (double*)partial, b, s);
    COLUMN_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
}

extern "C" int lbl_column_flux_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                   const double* depth, double range_min, double range_max, int64_t n,
                                   lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top, int n_angles,
                                   const double* mu, const double* weight, int n_bands, const int64_t* band_first,
                                   const int64_t* band_count, lbl_buffer* level_flux, lbl_buffer* up_top,
                                   lbl_buffer* down_surface) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    std::vector<char> blk(sizeof(FluxArgs), 0);
    FluxArgs* a = (FluxArgs*)blk.data();
    int rc;
    if ((rc = check_column(ctx, "level fluxes", a, n_layers, abs_coef, T, depth, range_min, range_max, n, I_surface,
                           surface_T, n_angles, mu, weight, n_bands, band_first, band_count)))
        return rc;
    const int nv = 2 * (n_layers + 1);
    if ((rc = ctx_check_buffer(ctx, level_flux, (int64_t)n_bands * nv, "level_flux", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, I_top, n, "I_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_top, n, "up_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, down_surface, n, "down_surface", false))) return rc;
    a->I_top = I_top ? buffer_data(I_top) : nullptr;
    a->up_top = up_top ? buffer_data(up_top) : nullptr;
    a->down_surface = down_surface ? buffer_data(down_surface) : nullptr;
    return run_column(ctx, a, 4, nv, n_bands, band_count, {a->up_top, a->down_surface}, (size_t)n * sizeof(double),
                      [&](const FluxArgs* d, double* partial, int b, hipStream_t s) {
        launch_column_flux(d, n_layers, n_angles, band_first[b], band_count[b], partial, buffer_data(level_flux) + (size_t)b * nv, s);
    });
} LBL_GUARD_END(ctx)

// The emissivity arguments of both surface entry points: a buffer of n points (its values are not read here) or one value
// in [0, 1].
static int check_emissivity(lbl_ctx* ctx, lbl_buffer* emissivity, double emissivity_all, int64_t n) {
    int rc;
    if ((rc = ctx_check_buffer(ctx, emissivity, n, "emissivity", false))) return rc;
    if (!emissivity && !(emissivity_all >= 0.0 && emissivity_all <= 1.0))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "emissivity_all must lie in [0, 1]");
    return LBL_OK;
}

// lbl_column_flux_surface_dev (Args = SurfaceFluxArgs, T per layer) and lbl_column_flux_linear_dev (Args = LinearFluxArgs, T
// the 2 n_layers edge temperatures): the same checks in the same order and the same launch sequence around launch(...).
template <class Args, class Launch>
static int surface_flux_call(lbl_ctx* ctx, double* pbkT_top, Args* a, Launch launch, int n_layers, lbl_buffer* const* abs_coef,
                             const double* T, const double* depth, double range_min, double range_max, int64_t n,
                             lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top, int n_angles, const double* mu,
                             const double* weight, int n_bands, const int64_t* band_first, const int64_t* band_count,
                             lbl_buffer* emissivity, double emissivity_all, int reflection, lbl_buffer* level_flux,
                             lbl_buffer* up_top, lbl_buffer* down_surface, lbl_buffer* up_surface) {
    int rc;
    if ((rc = check_column(ctx, "level fluxes", a, n_layers, abs_coef, T, depth, range_min, range_max, n, I_surface,
                           surface_T, n_angles, mu, weight, n_bands, band_first, band_count, pbkT_top)))
        return rc;
    const int nv = 2 * (n_layers + 1);
    if ((rc = ctx_check_buffer(ctx, level_flux, (int64_t)n_bands * nv, "level_flux", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, I_top, n, "I_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_top, n, "up_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, down_surface, n, "down_surface", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_surface, n, "up_surface", false))) return rc;
    if (reflection != 0 && reflection != 1)
        return column_fail(ctx, LBL_ERR_BAD_ARG, "reflection must be 0 (Lambertian) or 1 (specular)");
    if ((rc = check_emissivity(ctx, emissivity, emissivity_all, n))) return rc;
    double w_sum = 0.0;
    for (int k = 0; k < n_angles; ++k) w_sum += weight[k];
    if (!(w_sum > 0.0) || !std::isfinite(w_sum))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "the weights must add up to a finite sum > 0");
    a->I_top = I_top ? buffer_data(I_top) : nullptr;
    a->up_top = up_top ? buffer_data(up_top) : nullptr;
    a->down_surface = down_surface ? buffer_data(down_surface) : nullptr;
    a->emissivity = emissivity ? buffer_data(emissivity) : nullptr;
    a->emissivity_all = emissivity_all;
    a->w_sum = w_sum;
    a->up_surface = up_surface ? buffer_data(up_surface) : nullptr;
    a->reflection = reflection;
    return run_column(ctx, a, 4, nv, n_bands, band_count, {a->up_top, a->down_surface, a->up_surface}, (size_t)n * sizeof(double),
                      [&](const Args* d, double* partial, int b, hipStream_t s) {
        launch(d, n_layers, n_angles, band_first[b], band_count[b], partial, buffer_data(level_flux) + (size_t)b * nv, s);
    });
}

extern "C" int lbl_column_flux_surface_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                           const double* depth, double range_min, double range_max, int64_t n,
                                           lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top, int n_angles,
                                           const double* mu, const double* weight, int n_bands, const int64_t* band_first,
                                           const int64_t* band_count, lbl_buffer* emissivity, double emissivity_all,
                                           int reflection, lbl_buffer* level_flux, lbl_buffer* up_top,
                                           lbl_buffer* down_surface, lbl_buffer* up_surface) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    std::vector<char> blk(sizeof(SurfaceFluxArgs), 0);
    return surface_flux_call(ctx, nullptr, (SurfaceFluxArgs*)blk.data(), launch_surface_flux, n_layers, abs_coef, T, depth,
                             range_min, range_max, n, I_surface, surface_T, I_top, n_angles, mu, weight, n_bands, band_first,
                             band_count, emissivity, emissivity_all, reflection, level_flux, up_top, down_surface, up_surface);
} LBL_GUARD_END(ctx)

extern "C" int lbl_column_flux_linear_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T_edge,
                                          const double* depth, double range_min, double range_max, int64_t n,
                                          lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top, int n_angles,
                                          const double* mu, const double* weight, int n_bands, const int64_t* band_first,
                                          const int64_t* band_count, lbl_buffer* emissivity, double emissivity_all,
                                          int reflection, lbl_buffer* level_flux, lbl_buffer* up_top,
                                          lbl_buffer* down_surface, lbl_buffer* up_surface) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    std::vector<char> blk(sizeof(LinearFluxArgs), 0);
    LinearFluxArgs* a = (LinearFluxArgs*)blk.data();
    return surface_flux_call(ctx, a->pbkT_top, a, launch_linear_flux, n_layers, abs_coef, T_edge, depth, range_min, range_max,
                             n, I_surface, surface_T, I_top, n_angles, mu, weight, n_bands, band_first, band_count, emissivity,
                             emissivity_all, reflection, level_flux, up_top, down_surface, up_surface);
} LBL_GUARD_END(ctx)

// K5k: no temperatures and no surface source, so check_column does not fit; the checks follow its order.  The scratch is one
// reservation: F_down at the surface between the two walks (Lambertian, unless the caller's down_surface serves) and behind
// it the partials of the widest band.
extern "C" int lbl_column_solar_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* depth,
                                    double range_min, double range_max, int64_t n, lbl_buffer* S0, int n_beams,
                                    const double* beam_weight, const double* slant, int n_angles, const double* mu,
                                    const double* weight, int n_bands, const int64_t* band_first, const int64_t* band_count,
                                    lbl_buffer* emissivity, double emissivity_all, int reflection, lbl_buffer* level_flux,
                                    lbl_buffer* up_top, lbl_buffer* down_surface, lbl_buffer* up_surface) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    (void)range_min; (void)range_max;       // (the grid of the other column calls: nothing here depends on a wavenumber)
    std::vector<char> blk(sizeof(SolarArgs), 0);
    SolarArgs* a = (SolarArgs*)blk.data();
    if (n_layers < 0 || n_layers > kMaxLayers) return column_fail(ctx, LBL_ERR_BAD_ARG, "at most %d layers", kMaxLayers);
    if (n < 0) return column_fail(ctx, LBL_ERR_BAD_ARG, "negative n");
    if (n_layers > 0 && (!abs_coef || !depth || !slant)) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    if (ctx_sweep_ieee(ctx))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "%s exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)", "solar fluxes");
    if (n_beams < 1 || n_beams > kMaxFluxAngles) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d beams", kMaxFluxAngles);
    if (!beam_weight) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL beam set");
    if (reflection != 0 && reflection != 1)
        return column_fail(ctx, LBL_ERR_BAD_ARG, "reflection must be 0 (Lambertian) or 1 (specular)");
    if (n_angles < (reflection == 0 ? 1 : 0) || n_angles > kMaxFluxAngles)
        return column_fail(ctx, LBL_ERR_BAD_ARG, "%d..%d angles", reflection == 0 ? 1 : 0, kMaxFluxAngles);
    if (n_angles > 0 && (!mu || !weight)) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL angle set");
    if (n_bands < 1 || n_bands > kMaxFluxBands) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d bands", kMaxFluxBands);
    if (!band_first || !band_count) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL band list");
    const int nv = 2 * (n_layers + 1);
    int rc;
    if ((rc = ctx_check_buffer(ctx, S0, n, "S0", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, level_flux, (int64_t)n_bands * nv, "level_flux", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_top, n, "up_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, down_surface, n, "down_surface", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_surface, n, "up_surface", false))) return rc;
    if ((rc = check_emissivity(ctx, emissivity, emissivity_all, n))) return rc;
    int64_t max_count = 0;
    for (int b = 0; b < n_bands; ++b) {
        if (band_first[b] < 0 || band_count[b] < 1 || band_count[b] > n - band_first[b])
            return column_fail(ctx, LBL_ERR_BAD_ARG, "band %d: empty or outside [0, n)", b);
        max_count = std::max(max_count, band_count[b]);
    }
    for (int l = 0; l < n_layers; ++l) {
        if ((rc = ctx_check_buffer(ctx, abs_coef[l], n, "abs_coef", true))) return rc;
        if (!(depth[l] >= 0)) return column_fail(ctx, LBL_ERR_BAD_ARG, "layer %d: depth must be >= 0", l);
        a->abs_coef[l] = buffer_data(abs_coef[l]);
        a->depth[l] = depth[l];
    }
    for (int s = 0; s < n_beams; ++s) {
        if (!std::isfinite(beam_weight[s])) return column_fail(ctx, LBL_ERR_BAD_ARG, "beam %d: weight must be finite", s);
        a->beam_w[s] = beam_weight[s];
        for (int l = 0; l < n_layers; ++l) {
            const double v = slant[(size_t)s * n_layers + l];
            if (!(v >= 0) || !std::isfinite(v))
                return column_fail(ctx, LBL_ERR_BAD_ARG, "beam %d, layer %d: slant must be finite and >= 0", s, l);
            a->slant[s][l] = v;
        }
    }
    double w_sum = 0.0;
    for (int k = 0; k < n_angles; ++k) {
        if (!(mu[k] > 0 && mu[k] <= 1)) return column_fail(ctx, LBL_ERR_BAD_ARG, "angle %d: mu must lie in (0, 1]", k);
        if (!std::isfinite(weight[k])) return column_fail(ctx, LBL_ERR_BAD_ARG, "angle %d: weight must be finite", k);
        a->rmu[k] = 1.0 / mu[k];
        a->w[k] = weight[k];
        w_sum += weight[k];
    }
    if (reflection == 0 && (!(w_sum > 0.0) || !std::isfinite(w_sum)))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "the weights must add up to a finite sum > 0");
    a->w_sum = w_sum;
    a->S0 = buffer_data(S0);
    a->emissivity = emissivity ? buffer_data(emissivity) : nullptr;
    a->emissivity_all = emissivity_all;
    a->up_top = up_top ? buffer_data(up_top) : nullptr;
    a->down_surface = down_surface ? buffer_data(down_surface) : nullptr;
    a->up_surface = up_surface ? buffer_data(up_surface) : nullptr;
    a->n = n;
    a->n_layers = n_layers; a->n_beams = n_beams; a->n_angles = n_angles; a->reflection = reflection;

    // (f0 is read with the vector loads of the coefficients: it starts the reservation and the partials follow 32-byte aligned)
    const size_t f0_bytes = reflection == 0 && !down_surface ? ((size_t)n * sizeof(double) + 31) & ~(size_t)31 : 0;
    void* scratch = nullptr;
    if ((rc = ctx_reduction_scratch(ctx, f0_bytes + (size_t)column_transport_partials(max_count, 4) * nv * sizeof(double), &scratch)))
        return rc;
    a->f0 = reflection == 1 ? nullptr : down_surface ? a->down_surface : (double*)scratch;
    double* partial = (double*)((char*)scratch + f0_bytes);
    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, a, sizeof(SolarArgs), &d_args))) return rc;
    const hipStream_t s = ctx_stream(ctx);
    COLUMN_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    // (points outside every band keep 0 in the spectra)
    for (double* p : {a->up_top, a->down_surface, a->up_surface})
        if (p && n > 0) COLUMN_HIP_TRY(ctx, hipMemsetAsync(p, 0, (size_t)n * sizeof(double), s));
    for (int b = 0; b < n_bands; ++b)
        launch_solar((const SolarArgs*)d_args, n_layers, n_beams, n_angles, reflection, band_first[b], band_count[b], partial,
                     buffer_data(level_flux) + (size_t)b * nv, s);
    COLUMN_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
} LBL_GUARD_END(ctx)

// K5l, K5m, K5n: the doubles of a workspace that holds `points` points (rounded up to whole tiles, at least one) in one
// pass, `quantities` numbers per level and point; K5n's is K5m's (the layer quantities are recomputed)
static int scatter_workspace(int quantities, int n_layers, int64_t points, int64_t* doubles) {
    if (!doubles || n_layers < 0 || n_layers > kMaxLayers || points < 0 || points > (int64_t)1 << 40) return LBL_ERR_BAD_ARG;
    const int64_t tiles = std::max<int64_t>((points + kTwoStreamTile - 1) / kTwoStreamTile, 1);
    *doubles = (int64_t)quantities * (n_layers + 1) * tiles * kTwoStreamTile;
    return LBL_OK;
}
extern "C" int lbl_column_twostream_workspace(int n_layers, int64_t points, int64_t* doubles) {
    return scatter_workspace(kTwoStreamQuantities, n_layers, points, doubles);
}
extern "C" int lbl_column_flux_scatter_workspace(int n_layers, int64_t points, int64_t* doubles) {
    return scatter_workspace(kScatterFluxQuantities, n_layers, points, doubles);
}
extern "C" int lbl_column_radiance_scatter_workspace(int n_layers, int64_t points, int64_t* doubles) {
    return scatter_workspace(kScatterFluxQuantities, n_layers, points, doubles);
}
extern "C" int lbl_column_beam_radiance_workspace(int n_layers, int64_t points, int64_t* doubles) {
    return scatter_workspace(kTwoStreamQuantities, n_layers, points, doubles);      // (K5o's is K5l's)
}

// one of the three spectral numbers of the scatterers: a buffer of n points per scatterer, or the number beside it within
// [lo, hi] (the ends excluded where `open`)
static int check_scat_numbers(lbl_ctx* ctx, const char* what, int n_scat, int64_t n, lbl_buffer* const* bufs, const double* all,
                              double lo, double hi, bool open, const double** ptr, double* value) {
    for (int c = 0; c < n_scat; ++c) {
        lbl_buffer* b = bufs ? bufs[c] : nullptr;
        int rc;
        if ((rc = ctx_check_buffer(ctx, b, n, what, false))) return rc;
        if (b) { ptr[c] = buffer_data(b); continue; }
        if (!all) return column_fail(ctx, LBL_ERR_BAD_ARG, "scatterer %d: %s needs a buffer or a number", c, what);
        const double v = all[c];
        if (!(open ? v > lo && v < hi : v >= lo && v <= hi) || !std::isfinite(v))
            return column_fail(ctx, LBL_ERR_BAD_ARG, "scatterer %d: %s outside its range", c, what);
        value[c] = v;
    }
    return LBL_OK;
}

// the scatterers of K5l, K5m and K5n (n_scat within its limit, scat_amount there): every amount, then the three numbers of each
static int check_scatterers(lbl_ctx* ctx, ScatterPart* a, int n_layers, int64_t n, int n_scat, const double* scat_amount,
                            lbl_buffer* const* scat_ext, const double* scat_ext_all, lbl_buffer* const* scat_ssa,
                            const double* scat_ssa_all, lbl_buffer* const* scat_asym, const double* scat_asym_all) {
    int rc;
    for (int c = 0; c < n_scat; ++c)
        for (int l = 0; l < n_layers; ++l) {
            const double v = scat_amount[(size_t)c * n_layers + l];
            if (!(v >= 0) || !std::isfinite(v))
                return column_fail(ctx, LBL_ERR_BAD_ARG, "scatterer %d, layer %d: amount must be finite and >= 0", c, l);
            a->amount[c][l] = v;
        }
    if ((rc = check_scat_numbers(ctx, "extinction", n_scat, n, scat_ext, scat_ext_all, 0.0, HUGE_VAL, false, a->ext, a->ext_all))) return rc;
    if ((rc = check_scat_numbers(ctx, "single-scattering albedo", n_scat, n, scat_ssa, scat_ssa_all, 0.0, 1.0, false, a->ssa, a->ssa_all))) return rc;
    return check_scat_numbers(ctx, "asymmetry", n_scat, n, scat_asym, scat_asym_all, -1.0, 1.0, true, a->asym, a->asym_all);
}

// the caller's workspace of K5l and K5m, `quantities` numbers per level and point: at least one tile; *ws_points receives the
// points of one pass, a whole number of tiles
static int check_workspace(lbl_ctx* ctx, lbl_buffer* workspace, int quantities, int n_layers, int64_t* ws_points) {
    int rc;
    if ((rc = ctx_check_buffer(ctx, workspace, 0, "workspace", true))) return rc;
    int64_t ws_len = 0;
    lbl_buffer_size(workspace, &ws_len);
    const int64_t tile_doubles = (int64_t)quantities * (n_layers + 1) * kTwoStreamTile;
    if (ws_len < tile_doubles)
        return column_fail(ctx, LBL_ERR_BAD_ARG, "workspace: at least %lld doubles (one tile of %d points)", (long long)tile_doubles, kTwoStreamTile);
    *ws_points = ws_len / tile_doubles * kTwoStreamTile;
    return LBL_OK;
}

// the scatter part's fields that are not the scatterers' (those: check_scatterers), from checked arguments
static void fill_scatter_part(ScatterPart* a, lbl_buffer* emissivity, double emissivity_all, lbl_buffer* workspace,
                              int64_t ws_points, lbl_buffer* up_top, lbl_buffer* down_surface, lbl_buffer* up_surface,
                              int delta_scaling) {
    a->emissivity = emissivity ? buffer_data(emissivity) : nullptr;
    a->emissivity_all = emissivity_all;
    a->workspace = buffer_data(workspace);
    a->ws_points = ws_points;
    a->up_top = up_top ? buffer_data(up_top) : nullptr;
    a->down_surface = down_surface ? buffer_data(down_surface) : nullptr;
    a->up_surface = up_surface ? buffer_data(up_surface) : nullptr;
    a->delta_scaling = delta_scaling;
}

// The launch sequence of K5l and K5m on a checked argument block: the partial scratch, the block uploaded, the spectra zeroed,
// then every band in passes of as many points as the workspace holds, the band's partial slots zeroed first and reduced after
// its last pass.  `nv` values per band (K5l, K5m: the level sums; K5p: jac's rows); `variant` picks the downward kernel (K5l:
// n_beams; K5m, K5p: bool linear).
template <class Args, class Variant>
static int run_scatter_bands(lbl_ctx* ctx, const Args* a, Variant variant, int nv, int64_t n, int n_bands,
                             const int64_t* band_first, const int64_t* band_count, const std::vector<double*>& spectra,
                             lbl_buffer* level_flux) {
    const int64_t max_count = *std::max_element(band_count, band_count + n_bands);
    int rc;
    void* partial = nullptr;
    if ((rc = ctx_reduction_scratch(ctx, (size_t)twostream_partials(max_count) * nv * sizeof(double), &partial))) return rc;
    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, a, sizeof(Args), &d_args))) return rc;
    const hipStream_t s = ctx_stream(ctx);
    COLUMN_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    // (points outside every band keep 0 in the spectra)
    for (double* p : spectra)
        if (p && n > 0) COLUMN_HIP_TRY(ctx, hipMemsetAsync(p, 0, (size_t)n * sizeof(double), s));
    for (int b = 0; b < n_bands; ++b) {
        const int slots = twostream_partials(band_count[b]);
        COLUMN_HIP_TRY(ctx, hipMemsetAsync(partial, 0, (size_t)slots * nv * sizeof(double), s));
        for (int64_t done = 0; done < band_count[b]; done += a->ws_points)
            launch_scatter_pass((const Args*)d_args, variant, band_first[b], band_first[b] + done,
                                std::min<int64_t>(a->ws_points, band_count[b] - done), slots, (double*)partial, s);
        launch_scatter_final_values(nv, slots, (const double*)partial, buffer_data(level_flux) + (size_t)b * nv, s);
    }
    COLUMN_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
}

// The beam column of K5l and K5o, checked in two halves around each call's own checks (K5l's bands and level sums, K5o's
// views and radiances; the optional spectra and the emissivity in between).  Head: the column's extent, the sweeps'
// arithmetic, the beam and scatterer counts and the switch.
static int check_beam_column_head(lbl_ctx* ctx, const char* what, int n_layers, lbl_buffer* const* abs_coef, const double* depth,
                                  int64_t n, int n_beams, const double* beam_weight, const double* slant, int n_scat,
                                  const double* scat_amount, int delta_scaling) {
    if (n_layers < 0 || n_layers > kMaxLayers) return column_fail(ctx, LBL_ERR_BAD_ARG, "at most %d layers", kMaxLayers);
    if (n < 0) return column_fail(ctx, LBL_ERR_BAD_ARG, "negative n");
    if (n_layers > 0 && (!abs_coef || !depth || !slant)) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    if (ctx_sweep_ieee(ctx))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "%s exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)", what);
    if (n_beams < 1 || n_beams > kMaxFluxAngles) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d beams", kMaxFluxAngles);
    if (!beam_weight) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL beam set");
    if (n_scat < 0 || n_scat > kMaxScatterers) return column_fail(ctx, LBL_ERR_BAD_ARG, "0..%d scatterers", kMaxScatterers);
    if (n_scat > 0 && n_layers > 0 && !scat_amount) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL scatterer amounts");
    if (delta_scaling != 0 && delta_scaling != 1) return column_fail(ctx, LBL_ERR_BAD_ARG, "delta_scaling must be 0 or 1");
    return LBL_OK;
}

// Tail: the layers, the beams, the scatterers and the workspace; then the block (zeroed by the caller) filled from the
// buffers that the call checked itself.
static int check_beam_column_tail(lbl_ctx* ctx, TwoStreamArgs* a, int n_layers, lbl_buffer* const* abs_coef, const double* depth,
                                  int64_t n, lbl_buffer* S0, int n_beams, const double* beam_weight, const double* slant,
                                  int n_scat, const double* scat_amount, lbl_buffer* const* scat_ext,
                                  const double* scat_ext_all, lbl_buffer* const* scat_ssa, const double* scat_ssa_all,
                                  lbl_buffer* const* scat_asym, const double* scat_asym_all, int delta_scaling,
                                  lbl_buffer* emissivity, double emissivity_all, lbl_buffer* workspace, lbl_buffer* up_top,
                                  lbl_buffer* down_surface, lbl_buffer* direct_surface, lbl_buffer* up_surface) {
    int rc;
    for (int l = 0; l < n_layers; ++l) {
        if ((rc = ctx_check_buffer(ctx, abs_coef[l], n, "abs_coef", true))) return rc;
        if (!(depth[l] >= 0)) return column_fail(ctx, LBL_ERR_BAD_ARG, "layer %d: depth must be >= 0", l);
        a->abs_coef[l] = buffer_data(abs_coef[l]);
        a->depth[l] = depth[l];
    }
    for (int s = 0; s < n_beams; ++s) {
        if (!std::isfinite(beam_weight[s])) return column_fail(ctx, LBL_ERR_BAD_ARG, "beam %d: weight must be finite", s);
        a->beam_w[s] = beam_weight[s];
        for (int l = 0; l < n_layers; ++l) {
            const double v = slant[(size_t)s * n_layers + l];
            if (!(v > 0) || !std::isfinite(v))
                return column_fail(ctx, LBL_ERR_BAD_ARG, "beam %d, layer %d: slant must be finite and > 0", s, l);
            a->slant[s][l] = v;
            a->m[s][l] = 1.0 / v;
        }
    }
    if ((rc = check_scatterers(ctx, a, n_layers, n, n_scat, scat_amount, scat_ext, scat_ext_all, scat_ssa, scat_ssa_all,
                               scat_asym, scat_asym_all)))
        return rc;
    int64_t ws_points = 0;
    if ((rc = check_workspace(ctx, workspace, kTwoStreamQuantities, n_layers, &ws_points))) return rc;
    fill_scatter_part(a, emissivity, emissivity_all, workspace, ws_points, up_top, down_surface, up_surface, delta_scaling);
    a->S0 = buffer_data(S0);
    a->direct_surface = direct_surface ? buffer_data(direct_surface) : nullptr;
    a->n_layers = n_layers;
    return LBL_OK;
}

// K5l: lbl_column_solar_dev's checks in its order, the scatterers' and the workspace's behind them; then run_scatter_bands.
extern "C" int lbl_column_twostream_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* depth,
                                        double range_min, double range_max, int64_t n, lbl_buffer* S0, int n_beams,
                                        const double* beam_weight, const double* slant, int n_scat, const double* scat_amount,
                                        lbl_buffer* const* scat_ext, const double* scat_ext_all, lbl_buffer* const* scat_ssa,
                                        const double* scat_ssa_all, lbl_buffer* const* scat_asym, const double* scat_asym_all,
                                        int delta_scaling, int n_bands, const int64_t* band_first, const int64_t* band_count,
                                        lbl_buffer* emissivity, double emissivity_all, lbl_buffer* workspace,
                                        lbl_buffer* level_flux, lbl_buffer* up_top, lbl_buffer* down_surface,
                                        lbl_buffer* direct_surface, lbl_buffer* up_surface) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    (void)range_min; (void)range_max;       // (the grid of the other column calls: nothing here depends on a wavenumber)
    std::vector<char> blk(sizeof(TwoStreamArgs), 0);
    TwoStreamArgs* a = (TwoStreamArgs*)blk.data();
    int rc;
    if ((rc = check_beam_column_head(ctx, "two-stream fluxes", n_layers, abs_coef, depth, n, n_beams, beam_weight, slant, n_scat,
                                     scat_amount, delta_scaling)))
        return rc;
    if (n_bands < 1 || n_bands > kMaxFluxBands) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d bands", kMaxFluxBands);
    if (!band_first || !band_count) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL band list");
    const int nv = 3 * (n_layers + 1);
    if ((rc = ctx_check_buffer(ctx, S0, n, "S0", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, level_flux, (int64_t)n_bands * nv, "level_flux", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_top, n, "up_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, down_surface, n, "down_surface", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, direct_surface, n, "direct_surface", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_surface, n, "up_surface", false))) return rc;
    if ((rc = check_emissivity(ctx, emissivity, emissivity_all, n))) return rc;
    for (int b = 0; b < n_bands; ++b)
        if (band_first[b] < 0 || band_count[b] < 1 || band_count[b] > n - band_first[b])
            return column_fail(ctx, LBL_ERR_BAD_ARG, "band %d: empty or outside [0, n)", b);
    if ((rc = check_beam_column_tail(ctx, a, n_layers, abs_coef, depth, n, S0, n_beams, beam_weight, slant, n_scat, scat_amount,
                                     scat_ext, scat_ext_all, scat_ssa, scat_ssa_all, scat_asym, scat_asym_all, delta_scaling,
                                     emissivity, emissivity_all, workspace, up_top, down_surface, direct_surface, up_surface)))
        return rc;
    return run_scatter_bands(ctx, a, n_beams, nv, n, n_bands, band_first, band_count,
                             {a->up_top, a->down_surface, a->direct_surface, a->up_surface}, level_flux);
} LBL_GUARD_END(ctx)

// The thermal scattering column of K5m and K5n, checked in two halves around each call's own checks (its output buffer; K5n's
// views).  Head: check_column with the two-stream angle in place of an angle set (column, temperatures, surface source,
// bands), finite layer temperatures, and the scatterer count and switches.
static int check_scatter_column_head(lbl_ctx* ctx, const char* what, ScatterFluxArgs* a, int n_layers, lbl_buffer* const* abs_coef,
                                     const double* T, int planck_linear, const double* depth, double range_min,
                                     double range_max, int64_t n, lbl_buffer* I_surface, double surface_T, int n_scat,
                                     const double* scat_amount, int delta_scaling, int n_bands, const int64_t* band_first,
                                     const int64_t* band_count) {
    if (planck_linear != 0 && planck_linear != 1)
        return column_fail(ctx, LBL_ERR_BAD_ARG, "planck_linear must be 0 (layer temperatures) or 1 (edge temperatures)");
    const double mu = 0.5773502691896258, weight = kPi;      // 1 / sqrt(3) and pi: what the result corresponds to
    int rc;
    if ((rc = check_column(ctx, what, a, n_layers, abs_coef, T, depth, range_min, range_max, n, I_surface, surface_T, 1, &mu,
                           &weight, n_bands, band_first, band_count, planck_linear ? a->pbkT_top : nullptr)))
        return rc;
    for (int l = 0; l < n_layers && !planck_linear; ++l)
        if (!std::isfinite(T[l])) return column_fail(ctx, LBL_ERR_BAD_ARG, "layer %d: T must be finite and > 0", l);
    if (n_scat < 0 || n_scat > kMaxScatterers) return column_fail(ctx, LBL_ERR_BAD_ARG, "0..%d scatterers", kMaxScatterers);
    if (n_scat > 0 && n_layers > 0 && !scat_amount) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL scatterer amounts");
    if (delta_scaling != 0 && delta_scaling != 1) return column_fail(ctx, LBL_ERR_BAD_ARG, "delta_scaling must be 0 or 1");
    return LBL_OK;
}

// Tail: the optional buffers (up_surface: nullptr for K5n), the emissivity, K5l's scatterers and workspace (`quantities`
// numbers per level and point: K5p's has five); then I_top and the scatter part filled.
static int check_scatter_column_tail(lbl_ctx* ctx, ScatterFluxArgs* a, int n_layers, int64_t n, lbl_buffer* I_top, int n_scat,
                                     const double* scat_amount, lbl_buffer* const* scat_ext, const double* scat_ext_all,
                                     lbl_buffer* const* scat_ssa, const double* scat_ssa_all, lbl_buffer* const* scat_asym,
                                     const double* scat_asym_all, int delta_scaling, lbl_buffer* emissivity,
                                     double emissivity_all, lbl_buffer* workspace, lbl_buffer* up_top,
                                     lbl_buffer* down_surface, lbl_buffer* up_surface,
                                     int quantities = kScatterFluxQuantities) {
    int rc;
    if ((rc = ctx_check_buffer(ctx, I_top, n, "I_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_top, n, "up_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, down_surface, n, "down_surface", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_surface, n, "up_surface", false))) return rc;
    if ((rc = check_emissivity(ctx, emissivity, emissivity_all, n))) return rc;
    if ((rc = check_scatterers(ctx, a, n_layers, n, n_scat, scat_amount, scat_ext, scat_ext_all, scat_ssa, scat_ssa_all,
                               scat_asym, scat_asym_all)))
        return rc;
    int64_t ws_points = 0;
    if ((rc = check_workspace(ctx, workspace, quantities, n_layers, &ws_points))) return rc;
    a->I_top = I_top ? buffer_data(I_top) : nullptr;
    fill_scatter_part(a, emissivity, emissivity_all, workspace, ws_points, up_top, down_surface, up_surface, delta_scaling);
    return LBL_OK;
}

// K5m: the thermal scattering column's checks around the level sums' buffer; the launch sequence is K5l's.
extern "C" int lbl_column_flux_scatter_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                           int planck_linear, const double* depth, double range_min, double range_max,
                                           int64_t n, lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top, int n_scat,
                                           const double* scat_amount, lbl_buffer* const* scat_ext, const double* scat_ext_all,
                                           lbl_buffer* const* scat_ssa, const double* scat_ssa_all,
                                           lbl_buffer* const* scat_asym, const double* scat_asym_all, int delta_scaling,
                                           int n_bands, const int64_t* band_first, const int64_t* band_count,
                                           lbl_buffer* emissivity, double emissivity_all, lbl_buffer* workspace,
                                           lbl_buffer* level_flux, lbl_buffer* up_top, lbl_buffer* down_surface,
                                           lbl_buffer* up_surface) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    std::vector<char> blk(sizeof(ScatterFluxArgs), 0);
    ScatterFluxArgs* a = (ScatterFluxArgs*)blk.data();
    int rc;
    if ((rc = check_scatter_column_head(ctx, "scattering level fluxes", a, n_layers, abs_coef, T, planck_linear, depth, range_min,
                                        range_max, n, I_surface, surface_T, n_scat, scat_amount, delta_scaling, n_bands,
                                        band_first, band_count)))
        return rc;
    if ((rc = ctx_check_buffer(ctx, level_flux, (int64_t)n_bands * 2 * (n_layers + 1), "level_flux", true))) return rc;
    if ((rc = check_scatter_column_tail(ctx, a, n_layers, n, I_top, n_scat, scat_amount, scat_ext, scat_ext_all, scat_ssa,
                                        scat_ssa_all, scat_asym, scat_asym_all, delta_scaling, emissivity, emissivity_all,
                                        workspace, up_top, down_surface, up_surface)))
        return rc;
    return run_scatter_bands(ctx, a, planck_linear != 0, 2 * (n_layers + 1), n, n_bands, band_first, band_count,
                             {a->up_top, a->down_surface, a->up_surface}, level_flux);
} LBL_GUARD_END(ctx)

// the views of K5n and K5o: 1 .. kMaxViews cosines in (0, 1] with a direction each; the block's entries beyond n_views get
// mu = 1, up
static int check_views(lbl_ctx* ctx, ViewPart* a, int n_views, const double* view_mu, const int32_t* view_down) {
    if (n_views < 1 || n_views > kMaxViews) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d views", kMaxViews);
    if (!view_mu || !view_down) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL view list");
    for (int v = 0; v < kMaxViews; ++v) {
        if (v < n_views && !(view_mu[v] > 0 && view_mu[v] <= 1))
            return column_fail(ctx, LBL_ERR_BAD_ARG, "view %d: mu must lie in (0, 1]", v);
        if (v < n_views && view_down[v] != 0 && view_down[v] != 1)
            return column_fail(ctx, LBL_ERR_BAD_ARG, "view %d: the direction must be 0 (up) or 1 (down)", v);
        a->view_mu[v] = v < n_views ? view_mu[v] : 1.0;
        a->view_rmu[v] = 1.0 / a->view_mu[v];
        a->view_down[v] = v < n_views ? view_down[v] : 0;
    }
    return LBL_OK;
}

// K5n: the thermal scattering column's checks over one band, the whole grid, around the views' and the radiance buffer's;
// the passes are K5m's, without partial sums.
extern "C" int lbl_column_radiance_scatter_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                               int planck_linear, const double* depth, double range_min, double range_max,
                                               int64_t n, lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top,
                                               int n_scat, const double* scat_amount, lbl_buffer* const* scat_ext,
                                               const double* scat_ext_all, lbl_buffer* const* scat_ssa,
                                               const double* scat_ssa_all, lbl_buffer* const* scat_asym,
                                               const double* scat_asym_all, int delta_scaling, lbl_buffer* emissivity,
                                               double emissivity_all, int n_views, const double* view_mu,
                                               const int32_t* view_down, lbl_buffer* workspace, lbl_buffer* radiance,
                                               lbl_buffer* up_top, lbl_buffer* down_surface) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    std::vector<char> blk(sizeof(ScatterRadianceArgs), 0);
    ScatterRadianceArgs* a = (ScatterRadianceArgs*)blk.data();
    const int64_t band_first = 0, band_count = n;
    int rc;
    if ((rc = check_scatter_column_head(ctx, "scattering radiances", a, n_layers, abs_coef, T, planck_linear, depth, range_min,
                                        range_max, n, I_surface, surface_T, n_scat, scat_amount, delta_scaling, 1, &band_first,
                                        &band_count)))
        return rc;
    if ((rc = check_views(ctx, &a->views, n_views, view_mu, view_down))) return rc;
    if ((rc = ctx_check_buffer(ctx, radiance, (int64_t)n_views * n, "radiance", true))) return rc;
    if ((rc = check_scatter_column_tail(ctx, a, n_layers, n, I_top, n_scat, scat_amount, scat_ext, scat_ext_all, scat_ssa,
                                        scat_ssa_all, scat_asym, scat_asym_all, delta_scaling, emissivity, emissivity_all,
                                        workspace, up_top, down_surface, nullptr)))
        return rc;
    a->views.radiance = buffer_data(radiance);
    a->views.n_views = n_views;

    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, a, sizeof(ScatterRadianceArgs), &d_args))) return rc;
    const hipStream_t s = ctx_stream(ctx);
    COLUMN_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    for (int64_t done = 0; done < n; done += a->ws_points)
        launch_scatter_radiance_pass((const ScatterRadianceArgs*)d_args, planck_linear != 0, n_views, done,
                                     std::min<int64_t>(a->ws_points, n - done), s);
    COLUMN_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
} LBL_GUARD_END(ctx)

// K5o: K5l's checks of one beam over the whole grid around the views' and the radiance buffer's; the passes are K5n's.
extern "C" int lbl_column_beam_radiance_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* depth,
                                            double range_min, double range_max, int64_t n, lbl_buffer* S0, double beam_weight,
                                            const double* slant, int n_scat, const double* scat_amount,
                                            lbl_buffer* const* scat_ext, const double* scat_ext_all,
                                            lbl_buffer* const* scat_ssa, const double* scat_ssa_all,
                                            lbl_buffer* const* scat_asym, const double* scat_asym_all, int delta_scaling,
                                            lbl_buffer* emissivity, double emissivity_all, int n_views, const double* view_mu,
                                            const int32_t* view_down, lbl_buffer* workspace, lbl_buffer* radiance,
                                            lbl_buffer* up_top, lbl_buffer* down_surface, lbl_buffer* direct_surface) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    (void)range_min; (void)range_max;       // (as lbl_column_twostream_dev: nothing here depends on a wavenumber)
    std::vector<char> blk(sizeof(BeamViewArgs), 0);
    BeamViewArgs* a = (BeamViewArgs*)blk.data();
    int rc;
    if ((rc = check_beam_column_head(ctx, "scattered solar radiances", n_layers, abs_coef, depth, n, 1, &beam_weight, slant,
                                     n_scat, scat_amount, delta_scaling)))
        return rc;
    if (n < 1) return column_fail(ctx, LBL_ERR_BAD_ARG, "the grid is empty");
    if ((rc = check_views(ctx, &a->views, n_views, view_mu, view_down))) return rc;
    if ((rc = ctx_check_buffer(ctx, S0, n, "S0", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, radiance, (int64_t)n_views * n, "radiance", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, up_top, n, "up_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, down_surface, n, "down_surface", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, direct_surface, n, "direct_surface", false))) return rc;
    if ((rc = check_emissivity(ctx, emissivity, emissivity_all, n))) return rc;
    if ((rc = check_beam_column_tail(ctx, a, n_layers, abs_coef, depth, n, S0, 1, &beam_weight, slant, n_scat, scat_amount,
                                     scat_ext, scat_ext_all, scat_ssa, scat_ssa_all, scat_asym, scat_asym_all, delta_scaling,
                                     emissivity, emissivity_all, workspace, up_top, down_surface, direct_surface, nullptr)))
        return rc;
    a->views.radiance = buffer_data(radiance);
    a->n = n;
    a->views.n_views = n_views;

    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, a, sizeof(BeamViewArgs), &d_args))) return rc;
    const hipStream_t s = ctx_stream(ctx);
    COLUMN_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    for (int64_t done = 0; done < n; done += a->ws_points)
        launch_beam_view_pass((const BeamViewArgs*)d_args, n_views, done, std::min<int64_t>(a->ws_points, n - done), s);
    COLUMN_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
} LBL_GUARD_END(ctx)

// What lbl_column_jacobian_dev and lbl_column_jacobian_surface_dev check behind check_column, then the JacArgs part of the
// argument block filled; `head` values per band come before the layers' (2, or 3 with dF/de).  `edges` temperatures per
// layer in T, as many temperature values per layer and band and rows per layer in jac_T_spectra: 1, or 2 with the linear
// source (lbl_column_jacobian_linear_dev), where rT receives the bottom edges'.
// The terms and the outputs of every column Jacobian call (K5d, K5h, K5j, K5p), `nv0` values per band ahead of the terms': the
// term count, jac and the two optional spectra (`edges` temperature rows per layer), then every term; the terms sorted by layer (stable) into
// term_k, term_slot and layer_term (zeroed by the caller): layer l reads [layer_term[l], layer_term[l + 1]).
static int check_jacobian_terms(lbl_ctx* ctx, int nv0, int edges, int n_layers, int64_t n, int n_bands, int n_terms,
                                lbl_buffer* const* term_abs_coef, const int32_t* term_layer, lbl_buffer* jac,
                                lbl_buffer* jac_ln_tau_spectra, lbl_buffer* jac_T_spectra, const double** term_k,
                                int32_t* term_slot, int32_t* layer_term) {
    int rc;
    if (n_terms < 0 || n_terms > kMaxJacobianTerms)
        return column_fail(ctx, LBL_ERR_BAD_ARG, "at most %d molecule terms", kMaxJacobianTerms);
    if (n_terms > 0 && (!term_abs_coef || !term_layer)) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL term list");
    if ((rc = ctx_check_buffer(ctx, jac, (int64_t)n_bands * (nv0 + n_terms), "jac", true))) return rc;
    if ((rc = ctx_check_buffer(ctx, jac_ln_tau_spectra, (int64_t)n_layers * n, "jac_ln_tau_spectra", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, jac_T_spectra, (int64_t)edges * n_layers * n, edges == 1 ? "jac_T_spectra" : "jac_T_edge_spectra", false)))
        return rc;
    for (int t = 0; t < n_terms; ++t) {
        if (term_layer[t] < 0 || term_layer[t] >= n_layers)
            return column_fail(ctx, LBL_ERR_BAD_ARG, "term %d: layer %d outside [0, %d)", t, (int)term_layer[t], n_layers);
        if ((rc = ctx_check_buffer(ctx, term_abs_coef[t], n, "term_abs_coef", true))) return rc;
        ++layer_term[term_layer[t] + 1];
    }
    for (int l = 0; l < n_layers; ++l) layer_term[l + 1] += layer_term[l];
    std::vector<int32_t> fill(layer_term, layer_term + std::max(n_layers, 1));
    for (int t = 0; t < n_terms; ++t) {
        const int pos = fill[term_layer[t]]++;
        term_k[pos] = buffer_data(term_abs_coef[t]);
        term_slot[pos] = t;
    }
    return LBL_OK;
}

static int check_jacobian(lbl_ctx* ctx, JacArgs* a, int head, int n_layers, const double* T, int64_t n, double surface_T,
                          int n_angles, const double* weight, int n_bands, int n_terms, lbl_buffer* const* term_abs_coef,
                          const int32_t* term_layer, lbl_buffer* jac, lbl_buffer* jac_ln_tau_spectra,
                          lbl_buffer* jac_T_spectra, int edges = 1) {
    int rc;
    if ((rc = check_jacobian_terms(ctx, jacobian_slots(head, edges, n_layers, 0), edges, n_layers, n, n_bands, n_terms,
                                   term_abs_coef, term_layer, jac, jac_ln_tau_spectra, jac_T_spectra, a->term_k, a->term_slot,
                                   a->layer_term)))
        return rc;
    for (int l = 0; l < n_layers; ++l) a->rT[l] = 1.0 / T[edges * l];
    for (int k = 0; k < n_angles; ++k) a->wrmu[k] = weight[k] * a->rmu[k];
    a->r_surface_T = surface_T > 0 ? 1.0 / surface_T : 0.0;
    a->ln_tau_spec = jac_ln_tau_spectra ? buffer_data(jac_ln_tau_spectra) : nullptr;
    a->T_spec = jac_T_spectra ? buffer_data(jac_T_spectra) : nullptr;
    a->n_terms = n_terms;
    return LBL_OK;
}

extern "C" int lbl_column_jacobian_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                       const double* depth, double range_min, double range_max, int64_t n,
                                       lbl_buffer* I_surface, double surface_T, int n_angles, const double* mu,
                                       const double* weight, int n_bands, const int64_t* band_first,
                                       const int64_t* band_count, int n_terms, lbl_buffer* const* term_abs_coef,
                                       const int32_t* term_layer, lbl_buffer* jac, lbl_buffer* jac_ln_tau_spectra,
                                       lbl_buffer* jac_T_spectra) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    std::vector<char> blk(sizeof(JacArgs), 0);
    JacArgs* a = (JacArgs*)blk.data();
    int rc;
    if ((rc = check_column(ctx, "Jacobians", a, n_layers, abs_coef, T, depth, range_min, range_max, n, I_surface, surface_T,
                           n_angles, mu, weight, n_bands, band_first, band_count)))
        return rc;
    if ((rc = check_jacobian(ctx, a, 2, n_layers, T, n, surface_T, n_angles, weight, n_bands, n_terms, term_abs_coef,
                             term_layer, jac, jac_ln_tau_spectra, jac_T_spectra)))
        return rc;
    const int nv = jacobian_slots(2, 1, n_layers, n_terms);
    return run_column(ctx, a, 2, nv, n_bands, band_count, {a->ln_tau_spec, a->T_spec}, (size_t)n_layers * (size_t)n * sizeof(double),
                      [&](const JacArgs* d, double* partial, int b, hipStream_t s) {
        launch_column_jacobian(d, n_layers, n_angles, n_terms, band_first[b], band_count[b], partial, buffer_data(jac) + (size_t)b * nv, s);
    });
} LBL_GUARD_END(ctx)

// lbl_column_jacobian_surface_dev (Args = SurfaceJacArgs, T per layer, jac_T_spectra L x n) and lbl_column_jacobian_linear_dev
// (Args = LinearJacArgs, T the 2 n_layers edge temperatures, jac_T_spectra 2 L x n, `linear` its part of the block): the same
// checks in the same order and the same launch sequence around launch(...) at `np` points per thread.
template <class Args, class Launch>
static int surface_jacobian_call(lbl_ctx* ctx, Args* a, LinearJacArgs* linear, int np, Launch launch, int n_layers,
                                 lbl_buffer* const* abs_coef, const double* T, const double* depth, double range_min,
                                 double range_max, int64_t n, lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top,
                                 int n_angles, const double* mu, const double* weight, int n_bands, const int64_t* band_first,
                                 const int64_t* band_count, lbl_buffer* emissivity, double emissivity_all, int reflection,
                                 int n_terms, lbl_buffer* const* term_abs_coef, const int32_t* term_layer, lbl_buffer* jac,
                                 lbl_buffer* jac_ln_tau_spectra, lbl_buffer* jac_T_spectra, lbl_buffer* jac_e_spectrum) {
    const int edges = linear ? 2 : 1;
    int rc;
    if ((rc = check_column(ctx, "Jacobians", a, n_layers, abs_coef, T, depth, range_min, range_max, n, I_surface, surface_T,
                           n_angles, mu, weight, n_bands, band_first, band_count, linear ? linear->pbkT_top : nullptr)))
        return rc;
    if ((rc = check_jacobian(ctx, a, 3, n_layers, T, n, surface_T, n_angles, weight, n_bands, n_terms, term_abs_coef,
                             term_layer, jac, jac_ln_tau_spectra, jac_T_spectra, edges)))
        return rc;
    if ((rc = ctx_check_buffer(ctx, I_top, n, "I_top", false))) return rc;
    if ((rc = ctx_check_buffer(ctx, jac_e_spectrum, n, "jac_e_spectrum", false))) return rc;
    if (reflection != 0 && reflection != 1)
        return column_fail(ctx, LBL_ERR_BAD_ARG, "reflection must be 0 (Lambertian) or 1 (specular)");
    if ((rc = check_emissivity(ctx, emissivity, emissivity_all, n))) return rc;
    double w_sum = 0.0;
    for (int k = 0; k < n_angles; ++k) w_sum += weight[k];
    if (!(w_sum > 0.0) || !std::isfinite(w_sum))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "the weights must add up to a finite sum > 0");
    a->I_top = I_top ? buffer_data(I_top) : nullptr;
    a->emissivity = emissivity ? buffer_data(emissivity) : nullptr;
    a->emissivity_all = emissivity_all;
    a->w_sum = w_sum;
    a->e_spec = jac_e_spectrum ? buffer_data(jac_e_spectrum) : nullptr;
    a->reflection = reflection;
    double* T_spec_hi = nullptr;
    if (linear) {
        // (the edge spectra are one buffer of 2 L rows: zeroed as two halves of L rows; the kernel reads T_edge_spec alone)
        for (int l = 0; l < n_layers; ++l) linear->rT_top[l] = 1.0 / T[2 * l + 1];
        linear->T_edge_spec = a->T_spec;
        T_spec_hi = a->T_spec ? a->T_spec + (size_t)n_layers * (size_t)n : nullptr;
    }
    const int nv = jacobian_slots(3, edges, n_layers, n_terms);
    return run_column(ctx, a, np, nv, n_bands, band_count, {a->ln_tau_spec, a->T_spec, T_spec_hi},
                      (size_t)n_layers * (size_t)n * sizeof(double),
                      [&](const Args* d, double* partial, int b, hipStream_t s) {
        launch(d, n_layers, n_angles, n_terms, band_first[b], band_count[b], partial, buffer_data(jac) + (size_t)b * nv, s);
    }, a->e_spec);
}

extern "C" int lbl_column_jacobian_surface_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                               const double* depth, double range_min, double range_max, int64_t n,
                                               lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top, int n_angles,
                                               const double* mu, const double* weight, int n_bands,
                                               const int64_t* band_first, const int64_t* band_count, lbl_buffer* emissivity,
                                               double emissivity_all, int reflection, int n_terms,
                                               lbl_buffer* const* term_abs_coef, const int32_t* term_layer, lbl_buffer* jac,
                                               lbl_buffer* jac_ln_tau_spectra, lbl_buffer* jac_T_spectra,
                                               lbl_buffer* jac_e_spectrum) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    std::vector<char> blk(sizeof(SurfaceJacArgs), 0);
    return surface_jacobian_call(ctx, (SurfaceJacArgs*)blk.data(), nullptr, jacobian_points(n_angles),
                                 launch_surface_jacobian, n_layers, abs_coef, T, depth, range_min, range_max, n, I_surface,
                                 surface_T, I_top, n_angles, mu, weight, n_bands, band_first, band_count, emissivity,
                                 emissivity_all, reflection, n_terms, term_abs_coef, term_layer, jac, jac_ln_tau_spectra,
                                 jac_T_spectra, jac_e_spectrum);
} LBL_GUARD_END(ctx)

extern "C" int lbl_column_jacobian_linear_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T_edge,
                                              const double* depth, double range_min, double range_max, int64_t n,
                                              lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top, int n_angles,
                                              const double* mu, const double* weight, int n_bands,
                                              const int64_t* band_first, const int64_t* band_count, lbl_buffer* emissivity,
                                              double emissivity_all, int reflection, int n_terms,
                                              lbl_buffer* const* term_abs_coef, const int32_t* term_layer, lbl_buffer* jac,
                                              lbl_buffer* jac_ln_tau_spectra, lbl_buffer* jac_T_edge_spectra,
                                              lbl_buffer* jac_e_spectrum) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    std::vector<char> blk(sizeof(LinearJacArgs), 0);
    LinearJacArgs* a = (LinearJacArgs*)blk.data();
    return surface_jacobian_call(ctx, a, a, jacobian_points(n_angles), launch_linear_jacobian, n_layers, abs_coef,
                                 T_edge, depth, range_min, range_max, n, I_surface, surface_T, I_top, n_angles, mu, weight,
                                 n_bands, band_first, band_count, emissivity, emissivity_all, reflection, n_terms,
                                 term_abs_coef, term_layer, jac, jac_ln_tau_spectra, jac_T_edge_spectra, jac_e_spectrum);
} LBL_GUARD_END(ctx)

extern "C" int lbl_column_jacobian_scatter_workspace(int n_layers, int64_t points, int64_t* doubles) {
    return scatter_workspace(kScatterJacQuantities, n_layers, points, doubles);
}

// K5p: K5m's checks of the shared arguments around the terms' and the outputs' (check_jacobian_terms); the launch sequence
// is K5l's over jac's rows.  The spectra are zeroed row by row (n points each), as run_scatter_bands zeroes K5m's.
extern "C" int lbl_column_jacobian_scatter_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                               int planck_linear, const double* depth, double range_min, double range_max,
                                               int64_t n, lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top,
                                               int n_scat, const double* scat_amount, lbl_buffer* const* scat_ext,
                                               const double* scat_ext_all, lbl_buffer* const* scat_ssa,
                                               const double* scat_ssa_all, lbl_buffer* const* scat_asym,
                                               const double* scat_asym_all, int delta_scaling, int n_bands,
                                               const int64_t* band_first, const int64_t* band_count, lbl_buffer* emissivity,
                                               double emissivity_all, int n_terms, lbl_buffer* const* term_abs_coef,
                                               const int32_t* term_layer, lbl_buffer* workspace, lbl_buffer* jac,
                                               lbl_buffer* jac_ln_tau_spectra, lbl_buffer* jac_T_spectra,
                                               lbl_buffer* up_top) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    std::vector<char> blk(sizeof(ScatterJacArgs), 0);
    ScatterJacArgs* a = (ScatterJacArgs*)blk.data();
    int rc;
    if ((rc = check_scatter_column_head(ctx, "scattering Jacobians", a, n_layers, abs_coef, T, planck_linear, depth, range_min,
                                        range_max, n, I_surface, surface_T, n_scat, scat_amount, delta_scaling, n_bands,
                                        band_first, band_count)))
        return rc;
    const int edges = planck_linear ? 2 : 1;
    if ((rc = check_jacobian_terms(ctx, scatter_jacobian_slots(edges, n_layers, n_scat, 0), edges, n_layers, n, n_bands, n_terms,
                                   term_abs_coef, term_layer, jac, jac_ln_tau_spectra, jac_T_spectra, a->term_k, a->term_slot,
                                   a->layer_term)))
        return rc;
    if ((rc = check_scatter_column_tail(ctx, a, n_layers, n, I_top, n_scat, scat_amount, scat_ext, scat_ext_all, scat_ssa,
                                        scat_ssa_all, scat_asym, scat_asym_all, delta_scaling, emissivity, emissivity_all,
                                        workspace, up_top, nullptr, nullptr, kScatterJacQuantities)))
        return rc;
    for (int l = 0; l < n_layers; ++l) {
        a->rT[l] = 1.0 / T[edges * l];
        a->rT_top[l] = 1.0 / T[edges * l + edges - 1];
    }
    a->r_surface_T = surface_T > 0 ? 1.0 / surface_T : 0.0;
    a->ln_tau_spec = jac_ln_tau_spectra ? buffer_data(jac_ln_tau_spectra) : nullptr;
    a->T_spec = jac_T_spectra ? buffer_data(jac_T_spectra) : nullptr;
    a->n_terms = n_terms;
    a->n_scat = n_scat;
    std::vector<double*> spectra{a->up_top};
    for (int l = 0; l < n_layers; ++l) {
        if (a->ln_tau_spec) spectra.push_back(a->ln_tau_spec + (size_t)l * (size_t)n);
        for (int r = 0; r < edges && a->T_spec; ++r) spectra.push_back(a->T_spec + ((size_t)edges * l + r) * (size_t)n);
    }
    return run_scatter_bands(ctx, a, planck_linear != 0, scatter_jacobian_slots(edges, n_layers, n_scat, n_terms), n, n_bands,
                             band_first, band_count, spectra, jac);
} LBL_GUARD_END(ctx)

static size_t round8(size_t b) { return (b + 7) & ~(size_t)7; }

// What lbl_ray_radiance_dev, lbl_ray_jacobian_dev and lbl_ray_jacobian_rows (ctx NULL) check of the ray lists themselves.
// `markers`: a segment layer of kRaySurfaceMarker is no layer but the place where the ray meets the surface
// (lbl_ray_radiance_surface_dev, lbl_ray_jacobian_surface_dev and lbl_ray_jacobian_surface_rows).
static int check_ray_lists(lbl_ctx* ctx, int n_layers, int n_rays, const int32_t* ray_first, const int32_t* seg_layer,
                           bool markers) {
    if (n_layers < 1 || n_layers > kMaxLayers) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d layers", kMaxLayers);
    if (n_rays < 1 || n_rays > kMaxRayPaths) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d rays", kMaxRayPaths);
    if (!ray_first) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL ray list");
    if (ray_first[0] != 0) return column_fail(ctx, LBL_ERR_BAD_ARG, "ray_first[0] must be 0");
    for (int r = 0; r < n_rays; ++r)
        if (ray_first[r + 1] < ray_first[r]) return column_fail(ctx, LBL_ERR_BAD_ARG, "ray %d: ray_first decreases", r);
    const int n_seg = ray_first[n_rays];
    if (n_seg > kMaxRaySegments) return column_fail(ctx, LBL_ERR_BAD_ARG, "at most %d segments", kMaxRaySegments);
    if (n_seg > 0 && !seg_layer) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL segment list");
    for (int s = 0; s < n_seg; ++s)
        if ((seg_layer[s] < 0 || seg_layer[s] >= n_layers) && !(markers && seg_layer[s] == kRaySurfaceMarker))
            return column_fail(ctx, LBL_ERR_BAD_ARG, "segment %d: layer %d outside [0, %d)", s, (int)seg_layer[s], n_layers);
    return LBL_OK;
}

// Everything lbl_ray_radiance_dev and lbl_ray_jacobian_dev check of the arguments they share (ctx non-NULL), then the
// RayArgs part of the argument block filled - the tables start `header` bytes into the block, *bytes is where they end -
// and the dispatch order found.  `radiance` holds n_rays x n and may be NULL only where it is not `radiance_required`.
// `markers`: surface markers are allowed among the segment layers (check_ray_lists); their length must be 0 and a ray with
// one needs the surface source.  `seg_T` (the linear source; T is then not read): two temperatures per segment, entry and
// exit, finite and > 0 except a marker's pair; pbkT_min / pbkT_max are taken over them, *seg_pbkT receives their Planck
// exponents (0 for a marker's), and rays bundle only where they also share their segment temperatures.
static int check_rays(lbl_ctx* ctx, RayArgs* a, size_t header, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                      double range_min, double range_max, int64_t n, int n_rays, const int32_t* ray_first,
                      const int32_t* seg_layer, const double* seg_length, const int32_t* source_kind, lbl_buffer* I_source,
                      double source_T, lbl_buffer* radiance, bool radiance_required, lbl_buffer* transmittance, bool markers,
                      std::vector<int32_t>* order, size_t* bytes, const double* seg_T = nullptr,
                      std::vector<double>* seg_pbkT = nullptr) {
    const bool linear = seg_pbkT != nullptr;
    if (n_layers < 1 || n_layers > kMaxLayers) return column_fail(ctx, LBL_ERR_BAD_ARG, "1..%d layers", kMaxLayers);
    if (n < 1) return column_fail(ctx, LBL_ERR_BAD_ARG, "n must be >= 1");
    if (!abs_coef || (!linear && !T)) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL argument");
    if (ctx_sweep_ieee(ctx))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "%s exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)", "ray paths");
    int rc;
    if ((rc = check_ray_lists(ctx, n_layers, n_rays, ray_first, seg_layer, markers))) return rc;
    if (!source_kind) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL ray list");
    const int n_seg = ray_first[n_rays];
    if (n_seg > 0 && !seg_length) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL segment list");
    for (int s = 0; s < n_seg; ++s)
        if (!(seg_length[s] >= 0) || !std::isfinite(seg_length[s]))
            return column_fail(ctx, LBL_ERR_BAD_ARG, "segment %d: length must be finite and >= 0", s);
    if (linear && n_seg > 0 && !seg_T) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL segment list");
    for (int s = 0; linear && s < n_seg; ++s) {
        if (seg_layer[s] == kRaySurfaceMarker) continue;
        for (int e = 0; e < 2; ++e)
            if (!(std::isfinite(seg_T[2 * s + e]) && seg_T[2 * s + e] > 0))
                return column_fail(ctx, LBL_ERR_BAD_ARG, "segment %d: both temperatures must be finite and > 0", s);
    }
    if ((rc = ctx_check_buffer(ctx, I_source, n, "I_source", false))) return rc;
    for (int r = 0; markers && r < n_rays; ++r)
        for (int s = ray_first[r]; s < ray_first[r + 1]; ++s) {
            if (seg_layer[s] != kRaySurfaceMarker) continue;
            if (seg_length[s] != 0.0) return column_fail(ctx, LBL_ERR_BAD_ARG, "segment %d: a surface marker has length 0", s);
            if (!I_source && !(source_T > 0))
                return column_fail(ctx, LBL_ERR_BAD_ARG, "ray %d: a ray that meets the surface needs I_source or source_T > 0", r);
        }
    for (int r = 0; r < n_rays; ++r) {
        if (source_kind[r] != 0 && source_kind[r] != 1)
            return column_fail(ctx, LBL_ERR_BAD_ARG, "ray %d: source_kind must be 0 (space) or 1 (surface)", r);
        if (source_kind[r] == 1 && !I_source && !(source_T > 0))
            return column_fail(ctx, LBL_ERR_BAD_ARG, "ray %d: a surface source needs I_source or source_T > 0", r);
    }
    if (n > INT64_MAX / n_rays) return column_fail(ctx, LBL_ERR_BAD_ARG, "n_rays x n overflows");
    if ((rc = ctx_check_buffer(ctx, radiance, (int64_t)n_rays * n, "radiance", radiance_required))) return rc;
    if ((rc = ctx_check_buffer(ctx, transmittance, (int64_t)n_rays * n, "transmittance", false))) return rc;

    double pa = 0.0;
    for (int l = 0; l < n_layers; ++l) {
        if ((rc = ctx_check_buffer(ctx, abs_coef[l], n, "abs_coef", true))) return rc;
        a->abs_coef[l] = buffer_data(abs_coef[l]);
        if (linear) continue;
        if (!(T[l] > 0)) return column_fail(ctx, LBL_ERR_BAD_ARG, "layer %d: T must be > 0", l);
        planck_budget_constants(T[l], &pa, &a->pbkT[l]);
        a->pbkT_min = l == 0 ? a->pbkT[l] : std::min(a->pbkT_min, a->pbkT[l]);
        a->pbkT_max = l == 0 ? a->pbkT[l] : std::max(a->pbkT_max, a->pbkT[l]);
    }
    if (linear) {
        // (a call without a real segment forms no Planck value in a step: the bounds stay 0 and the general path runs)
        seg_pbkT->assign(2 * (size_t)n_seg, 0.0);
        bool any = false;
        for (int s = 0; s < n_seg; ++s) {
            if (seg_layer[s] == kRaySurfaceMarker) continue;
            for (int e = 0; e < 2; ++e) {
                double& v = (*seg_pbkT)[2 * (size_t)s + e];
                planck_budget_constants(seg_T[2 * s + e], &pa, &v);
                a->pbkT_min = any ? std::min(a->pbkT_min, v) : v;
                a->pbkT_max = any ? std::max(a->pbkT_max, v) : v;
                any = true;
            }
        }
    }
    planck_budget_constants(source_T > 0 ? source_T : 1.0, &pa, &a->pbk_surface);
    a->pa = pa;
    a->start = range_min; a->stop = range_max; a->step = grid_step(range_min, range_max, n);
    a->I_surface = I_source ? buffer_data(I_source) : nullptr;
    a->n = n;
    a->n_layers = n_layers;
    a->radiance = radiance ? buffer_data(radiance) : nullptr;
    a->transmittance = transmittance ? buffer_data(transmittance) : nullptr;
    a->n_rays = n_rays;
    // the tables: ray_first, seg_layer, seg_length, source_kind, order
    size_t off = round8(header);
    a->off_ray_first = (long long)off;   off += round8((size_t)(n_rays + 1) * sizeof(int32_t));
    a->off_seg_layer = (long long)off;   off += round8((size_t)n_seg * sizeof(int32_t));
    a->off_seg_length = (long long)off;  off += (size_t)n_seg * sizeof(double);
    a->off_source_kind = (long long)off; off += round8((size_t)n_rays * sizeof(int32_t));
    a->off_order = (long long)off;       off += round8((size_t)n_rays * sizeof(int32_t));
    *bytes = off;
    // Bundles: rays with one layer sequence (and at least one segment), kRayBundle at a time in the order they come; what
    // is left of every sequence, and the rays without segments, go one by one.  (A ray's arithmetic is the same either way.)
    std::vector<int32_t> single;
    order->clear();
    {
        // (the second key: the segments' Planck exponents with the linear source, empty otherwise)
        std::map<std::pair<std::vector<int32_t>, std::vector<double>>, std::vector<int32_t>> open;
        for (int r = 0; r < n_rays; ++r) {
            if (ray_first[r + 1] == ray_first[r]) { single.push_back(r); continue; }
            std::vector<double> temps;
            if (linear) temps.assign(seg_pbkT->begin() + 2 * (size_t)ray_first[r], seg_pbkT->begin() + 2 * (size_t)ray_first[r + 1]);
            auto& waiting = open[std::make_pair(std::vector<int32_t>(seg_layer + ray_first[r], seg_layer + ray_first[r + 1]),
                                                std::move(temps))];
            waiting.push_back(r);
            if ((int)waiting.size() == kRayBundle) {
                order->insert(order->end(), waiting.begin(), waiting.end());
                waiting.clear();
            }
        }
        for (auto& kv : open) single.insert(single.end(), kv.second.begin(), kv.second.end());
    }
    a->n_bundles = (int32_t)order->size() / kRayBundle;
    order->insert(order->end(), single.begin(), single.end());
    return LBL_OK;
}

// the tables check_rays laid out, copied into the block (whose header the caller copies)
static void fill_ray_tables(char* blk, const RayArgs& a, int n_rays, const int32_t* ray_first, const int32_t* seg_layer,
                            const double* seg_length, const int32_t* source_kind, const std::vector<int32_t>& order) {
    const int n_seg = ray_first[n_rays];
    memcpy(blk + a.off_ray_first, ray_first, (size_t)(n_rays + 1) * sizeof(int32_t));
    if (n_seg > 0) {
        memcpy(blk + a.off_seg_layer, seg_layer, (size_t)n_seg * sizeof(int32_t));
        memcpy(blk + a.off_seg_length, seg_length, (size_t)n_seg * sizeof(double));
    }
    memcpy(blk + a.off_source_kind, source_kind, (size_t)n_rays * sizeof(int32_t));
    memcpy(blk + a.off_order, order.data(), (size_t)n_rays * sizeof(int32_t));
}

extern "C" int lbl_ray_radiance_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                    double range_min, double range_max, int64_t n, int n_rays, const int32_t* ray_first,
                                    const int32_t* seg_layer, const double* seg_length, const int32_t* source_kind,
                                    lbl_buffer* I_source, double source_T, lbl_buffer* radiance,
                                    lbl_buffer* transmittance) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    // the argument block: header, ray_first, seg_layer, seg_length, source_kind, order
    RayArgs a;
    memset((void*)&a, 0, sizeof a);
    std::vector<int32_t> order;
    size_t bytes = 0;
    int rc;
    if ((rc = check_rays(ctx, &a, sizeof a, n_layers, abs_coef, T, range_min, range_max, n, n_rays, ray_first, seg_layer,
                         seg_length, source_kind, I_source, source_T, radiance, true, transmittance, false, &order, &bytes)))
        return rc;
    std::vector<char> blk(bytes, 0);
    memcpy(blk.data(), (const void*)&a, sizeof a);
    fill_ray_tables(blk.data(), a, n_rays, ray_first, seg_layer, seg_length, source_kind, order);

    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, blk.data(), blk.size(), &d_args))) return rc;
    COLUMN_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    launch_ray_radiance((const RayArgs*)d_args, n, n_rays, a.n_bundles, ctx_stream(ctx));
    COLUMN_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
} LBL_GUARD_END(ctx)

extern "C" int lbl_ray_radiance_surface_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                            double range_min, double range_max, int64_t n, int n_rays,
                                            const int32_t* ray_first, const int32_t* seg_layer, const double* seg_length,
                                            const int32_t* source_kind, lbl_buffer* I_source, double source_T,
                                            lbl_buffer* emissivity, double emissivity_all, lbl_buffer* surface_down,
                                            double surface_down_norm, lbl_buffer* radiance,
                                            lbl_buffer* transmittance) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    // the argument block: header, then K5e's tables
    RaySurfaceArgs a;
    memset((void*)&a, 0, sizeof a);
    std::vector<int32_t> order;
    size_t bytes = 0;
    int rc;
    if ((rc = check_rays(ctx, &a, sizeof a, n_layers, abs_coef, T, range_min, range_max, n, n_rays, ray_first, seg_layer,
                         seg_length, source_kind, I_source, source_T, radiance, true, transmittance, true, &order, &bytes)))
        return rc;
    if ((rc = check_emissivity(ctx, emissivity, emissivity_all, n))) return rc;
    if ((rc = ctx_check_buffer(ctx, surface_down, n, "surface_down", false))) return rc;
    if (surface_down && (!(surface_down_norm > 0.0) || !std::isfinite(surface_down_norm)))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "surface_down_norm must be finite and > 0");
    a.emissivity = emissivity ? buffer_data(emissivity) : nullptr;
    a.emissivity_all = emissivity_all;
    a.surface_down = surface_down ? buffer_data(surface_down) : nullptr;
    a.surface_down_norm = surface_down ? surface_down_norm : 1.0;
    std::vector<char> blk(bytes, 0);
    memcpy(blk.data(), (const void*)&a, sizeof a);
    fill_ray_tables(blk.data(), a, n_rays, ray_first, seg_layer, seg_length, source_kind, order);

    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, blk.data(), blk.size(), &d_args))) return rc;
    COLUMN_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    launch_ray_surface((const RaySurfaceArgs*)d_args, n, n_rays, a.n_bundles, ctx_stream(ctx));
    COLUMN_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
} LBL_GUARD_END(ctx)

extern "C" int lbl_ray_radiance_linear_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* seg_T,
                                           double range_min, double range_max, int64_t n, int n_rays,
                                           const int32_t* ray_first, const int32_t* seg_layer, const double* seg_length,
                                           const int32_t* source_kind, lbl_buffer* I_source, double source_T,
                                           lbl_buffer* emissivity, double emissivity_all, lbl_buffer* surface_down,
                                           double surface_down_norm, lbl_buffer* radiance,
                                           lbl_buffer* transmittance) try {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    // the argument block: header, K5e's tables, then the segments' Planck exponents
    LinearRayArgs a;
    memset((void*)&a, 0, sizeof a);
    std::vector<int32_t> order;
    std::vector<double> seg_pbkT;
    size_t bytes = 0;
    int rc;
    if ((rc = check_rays(ctx, &a, sizeof a, n_layers, abs_coef, nullptr, range_min, range_max, n, n_rays, ray_first, seg_layer,
                         seg_length, source_kind, I_source, source_T, radiance, true, transmittance, true, &order, &bytes,
                         seg_T, &seg_pbkT)))
        return rc;
    if ((rc = check_emissivity(ctx, emissivity, emissivity_all, n))) return rc;
    if ((rc = ctx_check_buffer(ctx, surface_down, n, "surface_down", false))) return rc;
    if (surface_down && (!(surface_down_norm > 0.0) || !std::isfinite(surface_down_norm)))
        return column_fail(ctx, LBL_ERR_BAD_ARG, "surface_down_norm must be finite and > 0");
    a.emissivity = emissivity ? buffer_data(emissivity) : nullptr;
    a.emissivity_all = emissivity_all;
    a.surface_down = surface_down ? buffer_data(surface_down) : nullptr;
    a.surface_down_norm = surface_down ? surface_down_norm : 1.0;
    a.off_seg_pbkT = (long long)bytes;
    bytes += seg_pbkT.size() * sizeof(double);
    std::vector<char> blk(bytes, 0);
    memcpy(blk.data(), (const void*)&a, sizeof a);
    fill_ray_tables(blk.data(), a, n_rays, ray_first, seg_layer, seg_length, source_kind, order);
    if (!seg_pbkT.empty()) memcpy(blk.data() + a.off_seg_pbkT, seg_pbkT.data(), seg_pbkT.size() * sizeof(double));

    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, blk.data(), blk.size(), &d_args))) return rc;
    COLUMN_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    launch_linear_ray((const LinearRayArgs*)d_args, n, n_rays, a.n_bundles, ctx_stream(ctx));
    COLUMN_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
} LBL_GUARD_END(ctx)

// The rows of lbl_ray_jacobian_dev (include/pyrad_hip.h): per ray the distinct layers it crosses in ascending order and
// the terms whose layer it crosses in term order; `head` rows come before the layers' (1, or 2 with dI/de: the surface entry
// points, whose markers are no layers and have no rows).  The lists are checked already.  `linear`
// (lbl_ray_jacobian_linear_dev): the c temperature rows of the layers give way to two rows per real segment in order of
// travel, seg_Trow names the first of each pair relative to the ray's first row, and the terms follow them.
struct RayRows {
    std::vector<int64_t> row_first;          // n_rays + 1
    std::vector<int32_t> crossed;            // per ray: c
    std::vector<int32_t> seg_slot;           // per segment: the rank of its layer among the ray's | kRayRowStore
    std::vector<int32_t> ray_terms;          // per ray: start of its table in term_row
    std::vector<int32_t> term_row;           // per set of crossed layers: the row of original term m, relative (-1: not crossed)
    std::vector<int32_t> seg_Trow;           // per segment (`linear`): the row of its dTa, relative; 0 for a marker
};
static void ray_rows(int n_layers, int n_rays, const int32_t* ray_first, const int32_t* seg_layer, int n_terms,
                     const int32_t* term_layer, int head, RayRows* R, bool linear = false) {
    R->row_first.assign(1, 0);
    R->crossed.clear(); R->ray_terms.clear(); R->term_row.clear();
    R->seg_slot.assign((size_t)ray_first[n_rays], 0);
    R->seg_Trow.assign(linear ? (size_t)ray_first[n_rays] : 0, 0);
    std::map<std::vector<int32_t>, int32_t> tables;
    std::vector<int32_t> rank(n_layers);
    for (int r = 0; r < n_rays; ++r) {
        std::fill(rank.begin(), rank.end(), -1);
        for (int s = ray_first[r]; s < ray_first[r + 1]; ++s)
            if (seg_layer[s] != kRaySurfaceMarker) rank[seg_layer[s]] = 0;
        std::vector<int32_t> set;
        for (int l = 0; l < n_layers; ++l)
            if (rank[l] == 0) { rank[l] = (int32_t)set.size(); set.push_back(l); }
        const int c = (int)set.size();
        // backward order: the last segment of a layer stores its rows, the earlier ones add
        std::vector<char> seen(n_layers, 0);
        for (int s = ray_first[r + 1] - 1; s >= ray_first[r]; --s) {
            if (seg_layer[s] == kRaySurfaceMarker) continue;
            R->seg_slot[s] = rank[seg_layer[s]] | (seen[seg_layer[s]] ? 0 : kRayRowStore);
            seen[seg_layer[s]] = 1;
        }
        // the rows between the head and the terms: 2 c, or c and two per real segment
        int body = 2 * c;
        if (linear) {
            body = c;
            for (int s = ray_first[r]; s < ray_first[r + 1]; ++s) {
                if (seg_layer[s] == kRaySurfaceMarker) continue;
                R->seg_Trow[s] = head + body;
                body += 2;
            }
            set.push_back(n_layers + body);          // (the terms' rows depend on the number of segments too)
        }
        int m_r = 0;
        for (int m = 0; m < n_terms; ++m) m_r += rank[term_layer[m]] >= 0;
        if (n_terms > 0) {
            auto it = tables.find(set);
            if (it == tables.end()) {
                it = tables.emplace(set, (int32_t)R->term_row.size()).first;
                int next = head + body;
                for (int m = 0; m < n_terms; ++m) R->term_row.push_back(rank[term_layer[m]] >= 0 ? next++ : -1);
            }
            R->ray_terms.push_back(it->second);
        } else {
            R->ray_terms.push_back(0);
        }
        R->crossed.push_back(c);
        R->row_first.push_back(R->row_first.back() + head + body + m_r);
    }
}

static int check_ray_terms(lbl_ctx* ctx, int n_layers, int n_terms, const int32_t* term_layer) {
    if (n_terms < 0 || n_terms > kMaxJacobianTerms)
        return column_fail(ctx, LBL_ERR_BAD_ARG, "at most %d terms", kMaxJacobianTerms);
    if (n_terms > 0 && !term_layer) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL term list");
    for (int t = 0; t < n_terms; ++t)
        if (term_layer[t] < 0 || term_layer[t] >= n_layers)
            return column_fail(ctx, LBL_ERR_BAD_ARG, "term %d: layer %d outside [0, %d)", t, (int)term_layer[t], n_layers);
    return LBL_OK;
}

static int ray_jacobian_rows(bool surface, int n_layers, int n_rays, const int32_t* ray_first, const int32_t* seg_layer,
                             int n_terms, const int32_t* term_layer, int64_t* row_first, int64_t* rows, bool linear = false) {
    int rc;
    if (!rows) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "rows is NULL");
    if ((rc = check_ray_lists(nullptr, n_layers, n_rays, ray_first, seg_layer, surface))) return rc;
    if ((rc = check_ray_terms(nullptr, n_layers, n_terms, term_layer))) return rc;
    RayRows R;
    ray_rows(n_layers, n_rays, ray_first, seg_layer, n_terms, term_layer, surface ? 2 : 1, &R, linear);
    if (row_first) memcpy(row_first, R.row_first.data(), (size_t)(n_rays + 1) * sizeof(int64_t));
    *rows = R.row_first.back();
    return LBL_OK;
}

extern "C" int lbl_ray_jacobian_rows(int n_layers, int n_rays, const int32_t* ray_first, const int32_t* seg_layer,
                                     int n_terms, const int32_t* term_layer, int64_t* row_first, int64_t* rows) try {
    return ray_jacobian_rows(false, n_layers, n_rays, ray_first, seg_layer, n_terms, term_layer, row_first, rows);
} LBL_GUARD_END(nullptr)

extern "C" int lbl_ray_jacobian_surface_rows(int n_layers, int n_rays, const int32_t* ray_first, const int32_t* seg_layer,
                                             int n_terms, const int32_t* term_layer, int64_t* row_first, int64_t* rows) try {
    return ray_jacobian_rows(true, n_layers, n_rays, ray_first, seg_layer, n_terms, term_layer, row_first, rows);
} LBL_GUARD_END(nullptr)

extern "C" int lbl_ray_jacobian_linear_rows(int n_layers, int n_rays, const int32_t* ray_first, const int32_t* seg_layer,
                                            int n_terms, const int32_t* term_layer, int64_t* row_first, int64_t* rows) try {
    return ray_jacobian_rows(true, n_layers, n_rays, ray_first, seg_layer, n_terms, term_layer, row_first, rows, true);
} LBL_GUARD_END(nullptr)

// lbl_ray_jacobian_dev, and with `surface` lbl_ray_jacobian_surface_dev: markers among the segment layers, the emissivity
// behind the header, one more row per ray.  With `linear` (and `surface`) lbl_ray_jacobian_linear_dev: T holds two
// temperatures per segment, their Planck exponents, reciprocals and rows follow the other tables.
static int ray_jacobian_call(lbl_ctx* ctx, bool surface, bool linear, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                             double range_min, double range_max, int64_t n, int n_rays, const int32_t* ray_first,
                             const int32_t* seg_layer, const double* seg_length, const int32_t* source_kind,
                             lbl_buffer* I_source, double source_T, lbl_buffer* emissivity, double emissivity_all,
                             int n_terms, lbl_buffer* const* term_abs_coef, const int32_t* term_layer, lbl_buffer* radiance,
                             lbl_buffer* jac) {
    if (!ctx) return comm_fail(nullptr, LBL_ERR_BAD_ARG, "ctx is NULL");
    // the argument block: header, K5e's tables, row_first, ray_crossed, seg_slot, ray_terms, term_row
    const size_t header = linear ? sizeof(LinearRayJacArgs) : surface ? sizeof(RaySurfaceJacArgs) : sizeof(RayJacArgs);
    std::vector<char> head(header, 0);
    RayJacArgs* a = (RayJacArgs*)head.data();
    std::vector<int32_t> order;
    std::vector<double> seg_pbkT;
    size_t off = 0;
    int rc;
    if ((rc = check_rays(ctx, a, header, n_layers, abs_coef, linear ? nullptr : T, range_min, range_max, n, n_rays, ray_first,
                         seg_layer, seg_length, source_kind, I_source, source_T, radiance, false, nullptr, surface, &order, &off,
                         linear ? T : nullptr, linear ? &seg_pbkT : nullptr)))
        return rc;
    if (surface) {
        if ((rc = check_emissivity(ctx, emissivity, emissivity_all, n))) return rc;
        RaySurfaceJacArgs* sa = (RaySurfaceJacArgs*)head.data();
        sa->emissivity = emissivity ? buffer_data(emissivity) : nullptr;
        sa->emissivity_all = emissivity_all;
    }
    if ((rc = check_ray_terms(ctx, n_layers, n_terms, term_layer))) return rc;
    if (n_terms > 0 && !term_abs_coef) return column_fail(ctx, LBL_ERR_BAD_ARG, "NULL term list");
    for (int t = 0; t < n_terms; ++t)
        if ((rc = ctx_check_buffer(ctx, term_abs_coef[t], n, "term_abs_coef", true))) return rc;
    RayRows R;
    ray_rows(n_layers, n_rays, ray_first, seg_layer, n_terms, term_layer, surface ? 2 : 1, &R, linear);
    const int64_t rows = R.row_first.back();
    if (n > INT64_MAX / rows) return column_fail(ctx, LBL_ERR_BAD_ARG, "rows x n overflows");
    if ((rc = ctx_check_buffer(ctx, jac, rows * n, "jac", true))) return rc;
    // the terms sorted by layer (stable), and every table of term rows re-ordered to match
    std::vector<int32_t> sorted(std::max(n_terms, 1), 0);
    for (int t = 0; t < n_terms; ++t) ++a->layer_term[term_layer[t] + 1];
    for (int l = 0; l < n_layers; ++l) a->layer_term[l + 1] += a->layer_term[l];
    {
        std::vector<int32_t> fill(a->layer_term, a->layer_term + n_layers);
        for (int t = 0; t < n_terms; ++t) {
            const int pos = fill[term_layer[t]]++;
            a->term_k[pos] = buffer_data(term_abs_coef[t]);
            sorted[pos] = t;
        }
    }
    std::vector<int32_t> term_row(R.term_row.size());
    for (size_t base = 0; base < term_row.size(); base += (size_t)n_terms)
        for (int pos = 0; pos < n_terms; ++pos) term_row[base + pos] = R.term_row[base + sorted[pos]];
    for (int l = 0; !linear && l < n_layers; ++l) a->rT[l] = 1.0 / T[l];
    a->r_source_T = source_T > 0 ? 1.0 / source_T : 0.0;
    a->jac = buffer_data(jac);
    a->n_terms = n_terms;
    const int n_seg = ray_first[n_rays];
    a->off_row_first = (long long)off;   off += (size_t)n_rays * sizeof(int64_t);
    a->off_ray_crossed = (long long)off; off += round8((size_t)n_rays * sizeof(int32_t));
    a->off_seg_slot = (long long)off;    off += round8((size_t)n_seg * sizeof(int32_t));
    a->off_ray_terms = (long long)off;   off += round8((size_t)n_rays * sizeof(int32_t));
    a->off_term_row = (long long)off;    off += round8(term_row.size() * sizeof(int32_t));
    if (linear) {
        LinearRayJacArgs* la = (LinearRayJacArgs*)head.data();
        la->off_seg_pbkT = (long long)off; off += 2 * (size_t)n_seg * sizeof(double);
        la->off_seg_rT = (long long)off;   off += 2 * (size_t)n_seg * sizeof(double);
        la->off_seg_Trow = (long long)off; off += round8((size_t)n_seg * sizeof(int32_t));
    }
    std::vector<char> blk(off, 0);
    memcpy(blk.data(), head.data(), head.size());
    fill_ray_tables(blk.data(), *a, n_rays, ray_first, seg_layer, seg_length, source_kind, order);
    memcpy(blk.data() + a->off_row_first, R.row_first.data(), (size_t)n_rays * sizeof(int64_t));
    memcpy(blk.data() + a->off_ray_crossed, R.crossed.data(), (size_t)n_rays * sizeof(int32_t));
    if (n_seg > 0) memcpy(blk.data() + a->off_seg_slot, R.seg_slot.data(), (size_t)n_seg * sizeof(int32_t));
    memcpy(blk.data() + a->off_ray_terms, R.ray_terms.data(), (size_t)n_rays * sizeof(int32_t));
    if (!term_row.empty()) memcpy(blk.data() + a->off_term_row, term_row.data(), term_row.size() * sizeof(int32_t));
    if (linear && n_seg > 0) {
        const LinearRayJacArgs* la = (const LinearRayJacArgs*)head.data();
        memcpy(blk.data() + la->off_seg_pbkT, seg_pbkT.data(), 2 * (size_t)n_seg * sizeof(double));
        double* rT = (double*)(blk.data() + la->off_seg_rT);
        for (int s = 0; s < n_seg; ++s)
            for (int e = 0; e < 2; ++e) rT[2 * s + e] = seg_layer[s] == kRaySurfaceMarker ? 0.0 : 1.0 / T[2 * s + e];
        memcpy(blk.data() + la->off_seg_Trow, R.seg_Trow.data(), (size_t)n_seg * sizeof(int32_t));
    }

    void* d_args = nullptr;
    if ((rc = ctx_device_args(ctx, blk.data(), blk.size(), &d_args))) return rc;
    COLUMN_HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
    if (linear) launch_linear_ray_jacobian((const LinearRayJacArgs*)d_args, n, n_rays, a->n_bundles, ctx_stream(ctx));
    else if (surface) launch_ray_surface_jacobian((const RaySurfaceJacArgs*)d_args, n, n_rays, a->n_bundles, n_terms, ctx_stream(ctx));
    else launch_ray_jacobian((const RayJacArgs*)d_args, n, n_rays, a->n_bundles, n_terms, ctx_stream(ctx));
    COLUMN_HIP_TRY(ctx, hipGetLastError());
    return LBL_OK;
}

extern "C" int lbl_ray_jacobian_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                    double range_min, double range_max, int64_t n, int n_rays, const int32_t* ray_first,
                                    const int32_t* seg_layer, const double* seg_length, const int32_t* source_kind,
                                    lbl_buffer* I_source, double source_T, int n_terms, lbl_buffer* const* term_abs_coef,
                                    const int32_t* term_layer, lbl_buffer* radiance, lbl_buffer* jac) try {
    return ray_jacobian_call(ctx, false, false, n_layers, abs_coef, T, range_min, range_max, n, n_rays, ray_first, seg_layer,
                             seg_length, source_kind, I_source, source_T, nullptr, 1.0, n_terms, term_abs_coef, term_layer,
                             radiance, jac);
} LBL_GUARD_END(ctx)

extern "C" int lbl_ray_jacobian_surface_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                            double range_min, double range_max, int64_t n, int n_rays,
                                            const int32_t* ray_first, const int32_t* seg_layer, const double* seg_length,
                                            const int32_t* source_kind, lbl_buffer* I_source, double source_T,
                                            lbl_buffer* emissivity, double emissivity_all, int n_terms,
                                            lbl_buffer* const* term_abs_coef, const int32_t* term_layer,
                                            lbl_buffer* radiance, lbl_buffer* jac) try {
    return ray_jacobian_call(ctx, true, false, n_layers, abs_coef, T, range_min, range_max, n, n_rays, ray_first, seg_layer,
                             seg_length, source_kind, I_source, source_T, emissivity, emissivity_all, n_terms, term_abs_coef,
                             term_layer, radiance, jac);
} LBL_GUARD_END(ctx)

extern "C" int lbl_ray_jacobian_linear_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* seg_T,
                                           double range_min, double range_max, int64_t n, int n_rays,
                                           const int32_t* ray_first, const int32_t* seg_layer, const double* seg_length,
                                           const int32_t* source_kind, lbl_buffer* I_source, double source_T,
                                           lbl_buffer* emissivity, double emissivity_all, int n_terms,
                                           lbl_buffer* const* term_abs_coef, const int32_t* term_layer,
                                           lbl_buffer* radiance, lbl_buffer* jac) try {
    return ray_jacobian_call(ctx, true, true, n_layers, abs_coef, seg_T, range_min, range_max, n, n_rays, ray_first, seg_layer,
                             seg_length, source_kind, I_source, source_T, emissivity, emissivity_all, n_terms, term_abs_coef,
                             term_layer, radiance, jac);
} LBL_GUARD_END(ctx)
