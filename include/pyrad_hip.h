/*
 * pyrad_hip.h — C ABI of the MI355X (gfx950) line-by-line absorption engine.
 *
 * The reference (bschrag620/PyRad) has no FFI: its seam is a Python method contract,
 * Isotope.createCrossSection() (pyradClasses.py:361-407) plus the property chain
 * absCoef -> transmittance -> transmission (pyradClasses.py:322-340, 581-606, 707-732,
 * 784-787) and pyradPlanck.planckWavenumber (pyradPlanck.py:38-44).  This header is the
 * C boundary a maintainer binds with ctypes in place of those bodies.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every function returns int
 *     (LBL_OK or a negative lbl_status); no C++ exception crosses the boundary.
 *   - lbl_last_error(ctx) returns a NUL-terminated description of the last failure
 *     on that context (ctx == NULL: last failure of a ctx-less call on this thread).
 *   - Host pointers are C-contiguous float64 arrays owned by the caller; the library
 *     never keeps a host pointer past return.
 *   - Device objects (lbl_lines, lbl_buffer, lbl_comm) belong to the context that made
 *     them and must be destroyed before it.
 *   - A context is bound to one HIP device and one HIP stream and is NOT thread-safe.
 *     "_dev" entry points only enqueue work on the context stream; lbl_sync() or any
 *     download drains it.  Host-pointer entry points are synchronous.
 *   - All arithmetic is IEEE fp64 (the reference is NumPy float64); grid indices int64.
 */
#ifndef PYRAD_HIP_H
#define PYRAD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBL_ABI_VERSION 5

typedef enum lbl_status {
    LBL_OK = 0,
    LBL_ERR_BAD_ARG = -1,     /* NULL pointer, negative size, unsorted lines, ... */
    LBL_ERR_NO_DEVICE = -2,   /* no HIP device / device index out of range */
    LBL_ERR_HIP = -3,         /* a HIP runtime call failed */
    LBL_ERR_RCCL = -4,        /* an RCCL call failed */
    LBL_ERR_OOM = -5,         /* device allocation failed */
    LBL_ERR_STATE = -6        /* object belongs to another context, comm not initialised, ... */
} lbl_status;

typedef struct lbl_ctx lbl_ctx;
typedef struct lbl_lines lbl_lines;     /* device-resident HITRAN line list (SoA, sorted by nu) */
typedef struct lbl_buffer lbl_buffer;   /* device-resident float64 array */
typedef struct lbl_comm lbl_comm;       /* RCCL communicator, one rank per process */

/* Per-isotopologue scalars read by Isotope.createCrossSection (pyradClasses.py:361-407):
 * layer.T, layer.P (mbar), molecule.concentration (volume fraction, the q of
 * Line.lorentzHW, pyradClasses.py:258), isotope.molmass (g/mol, pyradClasses.py:296),
 * isotope.q[layer.T] and isotope.q296 (pyradClasses.py:389). */
typedef struct lbl_iso_params {
    double T;
    double P;
    double q_frac;
    double molmass;
    double Q_T;
    double Q_296;
} lbl_iso_params;

/* Layer grid (pyradClasses.py:648-676, 698-705).  The host computes these with the
 * reference's own expressions so that the integer truncations agree:
 *   resolution      = layer.resolution                        (pyradClasses.py:659-662)
 *   n_work          = int((rangeMax-rangeMin)/resolution)      (pyradClasses.py:700)
 *   n_base          = int((rangeMax-rangeMin)/BASE_RESOLUTION) (pyradClasses.py:672)
 *   window          = len(arange(0, distanceFromCenter, resolution))  (pyradClasses.py:377)
 * Wing support of a line is centre +- (window-2) grid points (pyradClasses.py:394). */
typedef struct lbl_grid {
    double range_min;
    double range_max;
    double resolution;
    double base_resolution;
    int64_t n_work;
    int64_t n_base;
    int64_t window;
    /* Contiguous shard of the WORK grid this call computes: points
     * [shard_first, shard_first + shard_count).  shard_count == 0 means the whole grid.
     * Output buffers stay globally indexed (n_base long) so that the shards of all ranks
     * can be all-gathered in place.  A sharded call requires resolution == base_resolution. */
    int64_t shard_first;
    int64_t shard_count;
} lbl_grid;

/* ---- library / context ------------------------------------------------------------- */
int lbl_abi_version(void);
/* Fixed sizes of the library (ABI 5), so that a host can choose a route instead of running into LBL_ERR_BAD_ARG:
 *   "merged_lists_per_job"  line lists one merged layer job takes (lbl_layer_merged_step_dev, lbl_layers_merged_accumulate_dev): 64
 *   "arrays_per_layer"      cross-section arrays of lbl_layer_sweep_dev / line lists of lbl_layer_step_dev: 511 (the reference
 *                           sums however many isotopologues a layer holds, pyradClasses.py:566-571, 707-712; HITRAN has ~160)
 *   "arrays_per_sum"        inputs of lbl_sum_dev: 64 (a longer sum is chained: the partial sum first)
 *   "arrays_per_column"     terms of lbl_column_step_dev: 511      "layers_per_column": 128      "jobs_per_batch": LBL_MAX_JOBS
 *   "flux_angles"           angles of lbl_column_flux_dev: 8      "flux_bands": bands of lbl_column_flux_dev: 64
 *   "jacobian_terms"        molecule terms of lbl_column_jacobian_dev: 512
 *   "ils_rows"              rows of lbl_ils_convolve_dev: 512      "ils_channels": its channels: 65536
 *   "ils_table"             values of its tabulated line shape: 4096
 *   "kdist_rows"            rows of lbl_rank_order_dev / lbl_ranked_means_dev: 512
 *   "kdist_intervals"       rank intervals of one band of lbl_ranked_means_dev: 256
 *   "ray_paths"             rays of lbl_ray_radiance_dev: 512      "ray_segments": their segments, all rays together: 65536
 * Unknown name: LBL_ERR_BAD_ARG. */
int lbl_limit(const char* name, int64_t* value);
int lbl_device_count(int* count);
int lbl_ctx_create(int device, lbl_ctx** out);
int lbl_ctx_destroy(lbl_ctx* ctx);
const char* lbl_last_error(const lbl_ctx* ctx);
int lbl_sync(lbl_ctx* ctx);
/* Native hipStream_t of the context (as void*) so a host can order foreign work on it. */
int lbl_ctx_stream(lbl_ctx* ctx, void** stream);
/* Two contexts of one device as a software pipeline: the ACCUMULATE kernels of `ctx` wait for the accumulate
 * kernels `predecessor` has enqueued so far (an event on its stream), everything else of `ctx` - line prep
 * before them, the sweep after them - does not.  With A chained after B and B after A and steps dealt
 * alternately, the fp64-bound accumulate kernels run one after another, each alone on the chip, while the
 * line prep of the next step and the sweep of the previous one fill the cycles they leave; every step's
 * arrays are complete in step order.  predecessor = NULL ends the chaining.
 * Destroying a predecessor unlinks it: its successors simply stop waiting (any destroy order is safe).
 * A chained context (either end of a link) cannot capture a graph - the cross-context event waits do not
 * live in a captured sequence: lbl_capture_begin returns LBL_ERR_STATE on it, and a capturing context
 * cannot be chained. */
int lbl_ctx_chain_accumulate(lbl_ctx* ctx, lbl_ctx* predecessor);
/* Name of the device ("gfx950..."), CU count, HBM bytes. */
int lbl_device_info(lbl_ctx* ctx, char* name, int name_len, int* n_cu, int64_t* hbm_bytes);

/* Tuning knobs for A/B parity runs and benchmarking (no reference counterpart):
 *   "accum_variant"          0 the literal form: IEEE divide + exp per (line, grid point) pair, line records through
 *                            the scalar cache (slow; the on-device cross-check of the others) |
 *                            3 running fraction + Gaussian recurrence with wave-private LDS staging of the
 *                            records, every pair evaluated directly |
 *                            5 (default) = 3 with the fp64-exact far-field series for Lorentz lines
 *                            more than 4 half-spans away from a span of 64*R points.
 *                            (1, 2 and 4 - superseded comparison kernels - were measured and removed from every
 *                            build, docs/history/: LBL_ERR_BAD_ARG)
 *   "accum_points_per_lane"  0 (auto) | 1 | 2 | 4 | 8
 *   "accum_line_split"       0 (auto) | 1 | 2 | 4 | 8 waves of a workgroup share one span of points
 *                            and split its lines (variants 3 and 5)
 *   "accum_longest_first"    workgroups are dispatched from a cached (job, tile) worklist sorted by
 *                            decreasing cost: 3 bin-packed per CU when the launch is a single round of
 *                            workgroups, 2 every other tier of n_cu items reversed (snake), 1 plain |
 *                            0: positional order (waves then search their line ranges themselves) |
 *                            4 (default): as 3, and a launch of several rounds is XCD-partitioned: workgroup
 *                            i runs on XCD i mod 8, each XCD has its own L2, so every XCD gets 32 contiguous
 *                            chunks of the tile sequence (dealt round-robin, equal estimated cost), each
 *                            XCD's list longest-first - K2 fetches 33 MB instead of 110 MB on the
 *                            100-2500 cm^-1 cell at the same kernel time
 *   "accum_tile_order"       positional order only: 1 (default) natural | 0 one contiguous run of
 *                            tiles per XCD | 2 golden-ratio stride
 *   "accum_blocks_per_cu"    0 .. 8, checked and without effect: it sized the launch of the retired variant 4, and the
 *                            key stays for callers that still set it (bench.py --blocks-per-cu)
 *   "accum_skew"             1 (default) line lists whose window has no far line (narrower than 640 points) go
 *                            through the skewed-range kernel when they fill the chip | 0 the span kernel
 *                            (all-direct instantiation) | 2 EVERY job through the skewed-range kernel (parity tests)
 *   "accum_skew_points_per_lane"  1 | 2 | 4 | 8 (default)
 *   "accum_xcd_chunks"       XCD-partitioned order ("accum_longest_first" 4): contiguous chunks of the tile sequence per
 *                            XCD, 0 (default: about 29 workgroups per chunk, 10..32 chunks) .. 64; for a launch of one
 *                            round: the contiguous runs per XCD of "accum_xcd_pack" (default 1, at most 16)
 *   "accum_xcd_pack"         launches of one round (at most 4 workgroups per CU; device-built schedules): every XCD packs its own
 *                            tiles into its own CUs.  1 (default): where every wave owns a span (no line split) an XCD's tiles
 *                            are a contiguous run of the sequence worth an eighth of the cost (its L2 then holds that run's
 *                            records only), else every 8th tile of the longest-first order (waves that share spans AND are
 *                            neighbours in the spectrum queue for the same L2 lines: +9..17 % measured) | 2 always the run |
 *                            3 always the mix | 0 one packing over all CUs by one wave (round 4).  The dispatch list has idle
 *                            positions (workgroups that exit at once)
 *   "accum_xcd_tolerance"    a contiguous run is kept as long as the busiest CU of no XCD carries more than this many percent
 *                            (default 3; -1: any) above the mean of the eight by the cost model: an XCD whose run holds the
 *                            spectrum's expensive tiles cannot hand any to another XCD's CUs; the mix takes over
 *   "accum_skew_line_split"  0 (default: by the lines per grid point) | 1 | 2 | 4 waves of a workgroup share one span of the
 *                            skewed-range kernel and deal its records (dense, merged line lists: a chunk of records
 *                            then covers the span again)
 *   "accum_gauss_run"        far-field kernel, production shape (4 points per lane, unsplit spans): points a lane walks per Gaussian
 *                            run.  16: two exp per 16 points, 128 VGPRs, four waves per SIMD | 32: two exp per 32 points, 164-166
 *                            VGPRs, three waves per SIMD; in exact mode also the build whose far-field series starts at 3
 *                            half-spans instead of 4 (38 terms) | 0 (default): budget mode - 32 for launches of more than 16 waves
 *                            per SIMD, else 16; exact mode - 32 except for launches of 12-16 waves per SIMD (one round of the
 *                            chip's wave slots at four per SIMD, two at three).  Results of the two builds agree to ~1e-15
 *                            (different summation orders), each is reproducible bit for bit.
 *   "accum_reach_skip"       1 (default): the line prep keeps the largest Gaussian cut-off of every block of 256 records, and a
 *                            chunk of far lines that lies beyond the largest cut-off of its span's blocks skips the
 *                            per-record test "does the Gaussian part still reach the span" | 0: every chunk forms the test.
 *                            The results are the same bit for bit; the switch exists for A/B runs and the tests
 *   "accum_far_min_window"  windows below this many points take the skewed-range kernel even where the far-field
 *                            kernel could run them (0, the default: its own limit, 640; measured flat up to 1000)
 *   "debug_ablate"           ONLY in diagnostic builds of the library (make EXTRA=-DLBL_DIAG): timing experiments,
 *                            bits switch off parts of kernels, results are wrong.  The production library has no
 *                            such code in its kernels and answers LBL_ERR_BAD_ARG (unknown option)
 *   "accuracy"               0 (default) "exact": every array as close to the reference's fp64 values as the arithmetic allows
 *                            (measured 1e-14 at every grid point of every BASELINE configuration) |
 *                            1 "budget": <= 1e-9 relative on the absorption coefficient (BASELINE north_star asks for 1e-6),
 *                            everything still fp64: 18 / 12 / 9 / 7 far-field series terms by distance instead of
 *                            30 / 26 / 23 / 20 / 17 / 15 / 13 (remainder <= 5.9e-10 of a line's own term), the Gaussian part of a pseudo-Voigt
 *                            line dropped where it is below 2^-34 of the line's Lorentz part (exact: 2^-54).  Applies to the
 *                            batches enqueued after the call
 *   "sweep_ieee_divisions"   0 (default) the sweeps form the absorption coefficient as cross section x one host-computed
 *                            factor conc P / 1E4 / k / T, the Planck exponent as n x (100 h c / k / T), reciprocals by
 *                            rcp + Newton steps: a few 1e-16 from | 1 the reference's own chain of correctly rounded
 *                            divisions (k bit-identical to NumPy's crossSection * concentration * P / 1E4 / k / T on the
 *                            same cross section; 2.5x the instructions per point and layer)
 *   "schedule_build"         1 (default) span tables and dispatch order of a launch group are built on the device, in
 *                            stream, by the first batch that uses them (no host search, no copy, no wait) | 0 on the host
 *                            (one thread; 4 ms for the 100-2500 cm^-1 cell, 80 ms for a 30-layer column).  Same tables,
 *                            same results; other "accum_longest_first" values than 4 always build on the host
 *   "layer_step_fused"       1 (default) lbl_layer_step_dev folds the sweep of a single-line-list layer into the
 *                            accumulate kernel | 0 always accumulate launch + sweep launch (bit-identical; A/B)
 *   "debug_throw"            test hook: 1 / 2 / 3 raise std::bad_alloc / std::runtime_error /
 *                            std::length_error inside the library; the call must come back as
 *                            LBL_ERR_OOM / LBL_ERR_STATE / LBL_ERR_OOM (no exception crosses this boundary) */
int lbl_set_option(lbl_ctx* ctx, const char* key, int value);

/* Kernel timing with HIP events recorded on the context stream around every launch of a
 * kernel class (the stream the kernels run on; torch.cuda.Event would not see it).
 * kind: 0 line_prep, 1 xsec_accumulate, 2 regrid, 3 layer_sweep, 4 column_sweep, 5 all-gather.
 * `on` is a bit mask of kinds (bit k = kind k; 0x3F = all; <= 0 = off).
 * lbl_profile_read drains the stream, returns the number of launches recorded since the last
 * reset and their summed duration in milliseconds. */
int lbl_profile_enable(lbl_ctx* ctx, int on);
int lbl_profile_read(lbl_ctx* ctx, int kind, int64_t* launches, double* total_ms);
int lbl_profile_reset(lbl_ctx* ctx);
/* Create events ahead of time so that timed launches only record them (an event created on first
 * use costs the timed region ~10 us). */
int lbl_profile_reserve(lbl_ctx* ctx, int n_events);

/* ---- device buffers (float64) ------------------------------------------------------- */
int lbl_buffer_create(lbl_ctx* ctx, int64_t n, lbl_buffer** out);
int lbl_buffer_destroy(lbl_buffer* buf);
int lbl_buffer_size(const lbl_buffer* buf, int64_t* n);
int lbl_buffer_upload(lbl_buffer* buf, const double* host, int64_t n, int64_t dst_offset);
int lbl_buffer_download(lbl_buffer* buf, double* host, int64_t n, int64_t src_offset);
int lbl_buffer_fill(lbl_buffer* buf, double value);                    /* async */
/* Download that does not wait: ordered behind everything enqueued on the context stream so far, carried out on the
 * context's copy stream beside the kernels enqueued after it (pyrad_amd.model sends a column's outgoing spectrum -
 * Atmosphere.transmission, pyradClasses.py:784-787 over all layers - home in pieces while the next piece is folded).
 * `host` should be page-locked (lbl_host_alloc); the range must not be rewritten, nor `host` read, before
 * lbl_download_wait (lbl_sync waits for these copies too).  Not capturable. */
int lbl_buffer_download_async(lbl_buffer* buf, double* host, int64_t n, int64_t src_offset);
int lbl_download_wait(lbl_ctx* ctx);
/* Page-locked host memory for the arrays a caller keeps handing to upload / download: the copy then
 * runs at the link's DMA rate instead of through the runtime's staging of pageable memory (3-5x
 * faster for a spectrum of a few MB).  Plain memory otherwise; free it with lbl_host_free (ctx may be
 * NULL there if the context is already gone). */
int lbl_host_alloc(lbl_ctx* ctx, int64_t bytes, void** out);
int lbl_host_free(lbl_ctx* ctx, void* ptr);
int lbl_buffer_devptr(lbl_buffer* buf, void** devptr);                 /* for RCCL / interop */

/* ---- line lists ------------------------------------------------------------------- */
/* Upload the seven per-line HITRAN fields Line carries and uses (pyradClasses.py:237-263;
 * Einstein A is carried by the reference but never read).  nu must be non-decreasing. */
int lbl_lines_create(lbl_ctx* ctx, const double* nu, const double* sw, const double* elower,
                     const double* gamma_air, const double* gamma_self, const double* n_air,
                     const double* delta_air, int64_t n_lines, lbl_lines** out);
/* A view of `count` consecutive lines of a resident list, starting at line `first` (nu is sorted, so a wavenumber
 * window of a list - Layer.effectiveRangeMin/Max of pyradClasses.py:656-657, or the halo of a grid shard - is such a
 * range): no copy, the view shares the parent's device arrays.  A 30-layer column keeps ONE copy of every molecule's
 * lines and 30 views of it, and the line-prep kernels of all layers read the same addresses (they stay in cache).
 * A view is destroyed with lbl_lines_destroy; a list with live views cannot be destroyed (LBL_ERR_STATE). */
int lbl_lines_view(lbl_lines* parent, int64_t first, int64_t count, lbl_lines** out);
int lbl_lines_destroy(lbl_lines* lines);
int lbl_lines_count(const lbl_lines* lines, int64_t* n);

/* ---- the hot path: Isotope.createCrossSection (pyradClasses.py:361-407) ----------- */
/* One-shot, host in / host out: per-line half-widths (pyradClasses.py:252-263), regime
 * select (pyradClasses.py:378-387), profile (pyradLineshape.py:39, 52, 58-76), intensity
 * (pyradIntensity.py:30-32), centre index (pyradClasses.py:390), accumulate
 * (pyradClasses.py:392-400) and regrid to the base grid (pyradClasses.py:401-405).
 * xsec_out has n_base elements (cm^2/molecule); regime_counts = {gaussian, lorentz, voigt}
 * as printed at pyradClasses.py:406 (may be NULL). */
int lbl_xsec_accumulate(lbl_ctx* ctx, const double* nu, const double* sw, const double* elower,
                        const double* gamma_air, const double* gamma_self, const double* n_air,
                        const double* delta_air, int64_t n_lines, const lbl_iso_params* iso,
                        const lbl_grid* grid, double* xsec_out, int64_t regime_counts[3]);

#define LBL_MAX_JOBS 65536    /* jobs (isotopologue x layer) per batched call */
/* Device-resident, asynchronous, batched form: job j accumulates lines[j] under iso[j] /
 * grid[j] into out[j] (n_base doubles).  All jobs run in one launch sequence so that
 * isotopologues, molecules and layers fill the chip together. */
int lbl_xsec_accumulate_dev(lbl_ctx* ctx, int n_jobs, lbl_lines* const* lines,
                            const lbl_iso_params* iso, const lbl_grid* grid,
                            lbl_buffer* const* out);
/* Regime counters of the most recent lbl_xsec_accumulate_dev (drains the stream):
 * counts[3*j + {0,1,2}] = {gaussian, lorentz, voigt} of job j. */
int lbl_last_regime_counts(lbl_ctx* ctx, int n_jobs, int64_t* counts);
/* ---- true Voigt line shape (beyond the reference; ABI 5, backward compatible) ----------------------------------------------
 * lbl_xsec_accumulate_dev evaluates the reference's profile: a Gaussian below lhw / ghw = 0.01, a Lorentzian above 100, a
 * pseudo-Voigt between (pyradClasses.py:378-387).  lbl_xsec_voigt_dev takes the same jobs and evaluates for EVERY line
 *     A * K(|d| * xs, y) / (ghw * sqrt(pi)),   K(x, y) = Re w(x + i y),   xs = resolution / ghw,   y = lhw / ghw,
 * with w the Faddeeva function, A the corrected intensity (pyradIntensity.py:30-32), lhw / ghw the Lorentz and Doppler half
 * widths (pyradClasses.py:252-263) and d the integer offset of a work-grid point from the line's centre index
 * (pyradClasses.py:390).  The geometry is the reference's scatter (pyradClasses.py:390-400): the centre point once, both
 * wings for |d| = 1 .. window - 2, points outside [0, n_work) dropped; a work grid coarser than the base grid is regridded
 * as before (pyradClasses.py:401-405).  x is formed as (double)|d| * xs with xs one IEEE division.
 * K is accurate to 1e-6 relative (measured: 3e-10) for y == 0 or 1e-5 <= y <= 1e4 and never negative; for 0 < y < 1e-5 its
 * error grows like 1 / y where exp(-x^2) has died (2.5e-9 at 1e-6, 2.5e-7 at 1e-8); y is what the line list and the
 * conditions make it - nothing is refused or clamped.
 * Arguments, limits (LBL_MAX_JOBS), sharding (shard_first / shard_count) and conventions are those of
 * lbl_xsec_accumulate_dev: stream-ordered, all jobs in one launch sequence, everything checked before anything is enqueued
 * (same status codes; window < 1 is refused), the host arrays are not retained, LBL_ERR_STATE inside a capture if the call
 * would allocate or upload.  lbl_last_regime_counts afterwards reports the batch's counters with their meaning unchanged:
 * the lines per regime by the reference's thresholds.  The options "accuracy" and "accum_*" (and the dispatch schedules,
 * lbl_ctx_chain_accumulate) do not apply to it: there is one kernel and one arithmetic.
 * Determinism: every point is summed by one thread over the lines in list order, without atomics: two calls give the same
 * bits, a job's result does not depend on the other jobs of the batch, and a shard equals the same points of the whole. */
int lbl_xsec_voigt_dev(lbl_ctx* ctx, int n_jobs, lbl_lines* const* lines, const lbl_iso_params* iso,
                       const lbl_grid* grid, lbl_buffer* const* out);
/* out[i] = K(x[i], y[i]) for i < n, elementwise, by the device function the accumulate kernel inlines (tests).  x >= 0;
 * y == 0 or y > 0; NaN in, NaN out; where the true value is below 1e-290 the result lies in [0, 1e-290].  Stream-ordered.
 * LBL_ERR_BAD_ARG: a NULL argument, negative n, a buffer shorter than n; LBL_ERR_STATE: a buffer of another context. */
int lbl_voigt_function_dev(lbl_ctx* ctx, lbl_buffer* x, lbl_buffer* y, int64_t n, lbl_buffer* out);
/* ---- temperature derivative of the Voigt cross section (ABI 5, additions) ----------------------------------------------------
 * Under the Voigt shape every line is amp * K(x, y) with amp = A / (ghw sqrt(pi)), x = |d| * resolution / ghw, y = lhw / ghw:
 * smooth in T, while the centre index, the window and the pressure shift do not depend on T.  lbl_xsec_voigt_dt_dev takes
 * lbl_xsec_voigt_dev's jobs and writes, over the same geometry and through the same regrid (it is linear),
 *     d(sigma)/dT = sum over lines and offsets of  amp * (a * K + bx * GX + by * GY),   GX = x dK/dx,  GY = y dK/dy,
 *     a  = d ln amp / dT = dlnw_dT[job] + c2 E / T^2 - (c2 nu' / T^2) / expm1(c2 nu' / T) - 1 / (2 T),
 *          nu' = nu + delta_air P / p0 (Boltzmann factor, stimulated emission, the 1 / ghw of amp),
 *     bx = d ln x / dT = -1 / (2 T),      by = d ln y / dT = -(n_air + 1/2) / T.
 * dlnw_dT[j] (host array, n_jobs doubles) is the logarithmic T-derivative of everything that multiplies job j's intensities
 * and is not formed from T by the line preparation: -d ln Q / dT for a cross section (iso.Q_T is a number to the library,
 * its slope is the caller's), -d ln Q / dT - 1 / T for a result that will be weighted by a number density P / (k T).
 * K, GX, GY come from one device function (voigt_kgrad of lbl_voigt_func.h): |dK|, |dGX|, |dGY| <= 1e-6 K for y == 0 or
 * 1e-5 <= y <= 1e4 wherever K >= 1e-290; K is lbl_voigt_function_dev's value bit for bit.  The derivative of the reference's
 * profile does not exist at its regime switches and is not offered.
 * out[j]: n_base doubles (cm^2 / molecule / K).  Stream-ordered, nothing is synchronised; everything is checked before
 * anything is enqueued.  Errors as lbl_xsec_voigt_dev, and LBL_ERR_BAD_ARG for a NULL or non-finite dlnw_dT.  The regime
 * counters (lbl_last_regime_counts) are not touched; lbl_profile_read counts the kernels as prep, accumulate and regrid.
 * Determinism as lbl_xsec_voigt_dev: line order per point, no atomics, a shard equals the same points of the whole. */
int lbl_xsec_voigt_dt_dev(lbl_ctx* ctx, int n_jobs, lbl_lines* const* lines, const lbl_iso_params* iso,
                          const double* dlnw_dT, const lbl_grid* grid, lbl_buffer* const* out);
/* K[i], GX[i], GY[i] = K, x dK/dx, y dK/dy at (x[i], y[i]) for i < n, by the device function the derivative kernel inlines
 * (tests).  y == 0: GY = 0; GX <= 0; NaN in, NaN out.  Stream-ordered.  Errors as lbl_voigt_function_dev. */
int lbl_voigt_gradient_dev(lbl_ctx* ctx, lbl_buffer* x, lbl_buffer* y, int64_t n, lbl_buffer* K, lbl_buffer* GX, lbl_buffer* GY);

/* Introspection for tests: the k-th most recently used dispatch schedule of the context (0 = the last one an
 * accumulate batch used).  list receives 2 ints per workgroup (job of the launch group, tile of the job), tabs 8 ints
 * per span of 64 R points {iA, iB, iC, iD, iF1, iF2, 0, 0} (the lower bounds of the span's edge / interior / far lines
 * in the job's sorted centre indices).  Either array may be NULL; *n_items / *n_tab_ints are always set.
 * built_on_device: 1 when the schedule came from the in-stream device build ("schedule_build" 1, the default),
 * 0 from the host. */
int lbl_schedule_export(lbl_ctx* ctx, int k, int32_t* list, int64_t list_cap, int32_t* tabs, int64_t tabs_cap,
                        int64_t* n_items, int64_t* n_tab_ints, int32_t* built_on_device);

/* Parity aid: runs the real line preparation (K1) of this one job and reports, per line, the centre index
 * K1 wrote (pyradClasses.py:390; the very value the accumulate kernel works from, clamped to +-2e9), and the
 * Lorentz and Doppler half-widths (pyradClasses.py:256-263), the corrected intensity (pyradIntensity.py:30-32)
 * and the regime (0 Gaussian, 1 Lorentz, 2 pseudo-Voigt; pyradClasses.py:379-387) from the same device
 * expressions K1 evaluates (a separate reporting kernel: the timed kernels carry no debug stores).
 * Any output may be NULL. */
int lbl_line_quantities(lbl_ctx* ctx, lbl_lines* lines, const lbl_iso_params* iso,
                        const lbl_grid* grid, int64_t* index, double* lorentz_hw,
                        double* gauss_hw, double* intensity, int32_t* regime);

/* ---- fused layer sweep (pyradClasses.py:566-571, 581-587, 707-716, 784-787; pyradPlanck.py:38-44)
 * For every base-grid point j:
 *   xs_m   = sum of the isotopologue cross sections of molecule m        (pyradClasses.py:566-571)
 *   k      = sum_m xs_m * conc[m] * P / 1e4 / kB / T                      (pyradClasses.py:583, 707-712)
 *   trans  = exp(-k * depth)                                             (pyradClasses.py:716)
 *   I_out  = trans * I_in + (1 - trans) * B(nu_j, T)                      (pyradClasses.py:784-787)
 * nu_j is the reference's xAxis = linspace(range_min, range_max, n, endpoint=True)
 * (pyradClasses.py:702-705).  iso_mol[i] (non-decreasing, 0-based) maps isotopologue i to
 * its molecule.  I_in == NULL with surface_T > 0 uses I_in = B(nu_j, surface_T)
 * (pyradInteractive.py:400).  Any of abs_coef / trans / I_out may be NULL.
 * Only points [first, first+count) are swept (count == 0: all n); buffers are indexed by j. */
int lbl_layer_sweep_dev(lbl_ctx* ctx, int n_iso, lbl_buffer* const* xsec, const int32_t* iso_mol,
                        int n_mol, const double* conc, double P, double T, double depth,
                        double range_min, double range_max, int64_t n,
                        int64_t first, int64_t count,
                        lbl_buffer* I_in, double surface_T,
                        lbl_buffer* abs_coef, lbl_buffer* trans, lbl_buffer* I_out);

/* One step of a layer (the gas cell of pyradClasses.py:648 after its addMolecule calls):
 * lbl_xsec_accumulate_dev for the layer's n_iso line lists followed by lbl_layer_sweep_dev, in ONE
 * launch sequence.  A layer with one line list on the base grid has the sweep of a point in the
 * accumulate kernel's output stage, right after that point's cross section is final (same arithmetic,
 * bit-identical results, no sweep launch, no re-read of the cross section).  With several line lists
 * the sweep kernel follows the accumulate launch: both ways of folding it in were measured slower on
 * MI355X.  Molecule sums, absorption coefficient, transmittance, outgoing radiance:
 * pyradClasses.py:566-571, 583, 707-716, 784-787; xsec[i] always receives line list i's cross
 * sections.  All line lists share `grid` (axis, shard) and the layer's T and P (iso[i].T / .P must
 * equal iso[0]'s); iso_mol / n_mol / conc as in lbl_layer_sweep_dev; xsec[i] receives the cross
 * section of line list i.  lbl_set_option("layer_step_fused", 0) forces the two-call form. */
int lbl_layer_step_dev(lbl_ctx* ctx, int n_iso, lbl_lines* const* lines, const lbl_iso_params* iso,
                       const lbl_grid* grid, lbl_buffer* const* xsec, const int32_t* iso_mol, int n_mol,
                       const double* conc, double depth, lbl_buffer* I_in, double surface_T,
                       lbl_buffer* abs_coef, lbl_buffer* trans, lbl_buffer* I_out);

/* ---- the layer's absorption coefficient accumulated directly (ABI 4) -----------------------------------------
 * Layer.absCoef is sum over molecules m of (sum over isotopologues of crossSection) * conc_m * P / 1E4 / k / T
 * (pyradClasses.py:707-712, 581-583, 566-571), and the reference computes its parts lazily (progressCrossSection,
 * pyradClasses.py:32-88).  These entry points run ONE accumulate job per LAYER: the line preparation multiplies every
 * line's amplitude by its molecule's factor f_m = conc_m P / 1E4 / k / T (host, the reference's order of operations) and
 * writes the records of all the layer's line lists into one array in centre-index order (the merged order is built on
 * the device once per (line lists, grid), beside the dispatch schedule); the accumulate kernel then sums every
 * (line, grid point) contribution of the layer into the absorption coefficient itself - one pass over the grid instead
 * of one per line list, no per-line-list cross-section arrays written and read back.  Every contribution the
 * reference's loop adds (pyradClasses.py:392-400) is still evaluated.  A per-isotopologue cross section
 * (Isotope.crossSection) is produced on demand by lbl_xsec_accumulate_dev, as before.
 * Arithmetic: fp64; differs from the per-line-list path by the order of summation and one rounding per line (the
 * factor rides on the amplitude instead of on the sum): a few 1e-16 relative.  They exist in the sweeps' default arithmetic
 * only: with "sweep_ieee_divisions" 1 lbl_layer_merged_step_dev, lbl_column_fold_dev and lbl_column_transmission answer
 * LBL_ERR_BAD_ARG (ABI 5; until then the option was silently ignored there) - use the per-line-list entry points, which honour
 * it.  "accuracy" applies as usual.  At most 64 line lists per layer (lbl_limit "merged_lists_per_job").  Needs "accum_variant" 3 or 5 and the device schedule build (LBL_ERR_BAD_ARG otherwise: use the per-list step).
 *
 * lbl_layer_merged_step_dev: one layer (gas cell) - line prep, ONE accumulate job over the merged lists, and in its
 * output stage k, transmittance exp(-k depth) and outgoing radiance trans * I_in + (1 - trans) * B(nu, T)
 * (pyradClasses.py:714-716, 784-787; pyradPlanck.py:38-44).  Arguments as lbl_layer_step_dev without the xsec buffers;
 * any of abs_coef / trans / I_out may be NULL (not all).  A work grid coarser than the base grid (dynamic resolution)
 * is regridded (np.interp of pyradClasses.py:401-405 applied to k) and swept by the sweep kernel. */
int lbl_layer_merged_step_dev(lbl_ctx* ctx, int n_iso, lbl_lines* const* lines, const lbl_iso_params* iso,
                              const lbl_grid* grid, const int32_t* iso_mol, int n_mol, const double* conc,
                              double depth, lbl_buffer* I_in, double surface_T,
                              lbl_buffer* abs_coef, lbl_buffer* trans, lbl_buffer* I_out);
/* The same for a batch of layers (a column: every layer's merged job in ONE launch sequence, so that layers fill the
 * chip together): layer l owns n_iso[l] consecutive entries of lines / iso / iso_mol (molecule index 0-based inside the
 * layer, non-decreasing), n_mol[l] consecutive entries of conc, its own grid[l], and receives its absorption
 * coefficient in abs_coef[l] (n_base doubles). */
int lbl_layers_merged_accumulate_dev(lbl_ctx* ctx, int n_layers, const int32_t* n_iso, lbl_lines* const* lines,
                                     const lbl_iso_params* iso, const lbl_grid* grid, const int32_t* iso_mol,
                                     const int32_t* n_mol, const double* conc, lbl_buffer* const* abs_coef);
/* Column step from the layers' absorption coefficients (bottom to top): per grid point and layer
 * trans = exp(-k depth), I <- trans * I + (1 - trans) * B(nu_j, T_l), I_0 = I_in or B(nu_j, surface_T)
 * (pyradClasses.py:714-716, 784-787) in one pass over the n_layers arrays.  trans: NULL, or n_layers buffers of which
 * any may be NULL (that layer's transmittance is then not written). */
int lbl_column_fold_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                        const double* depth, double range_min, double range_max, int64_t n,
                        int64_t first, int64_t count, lbl_buffer* I_in, double surface_T,
                        lbl_buffer* const* trans, lbl_buffer* I_out);

/* ---- level fluxes (beyond the reference; ABI 5, backward compatible) -------------------------------------------------
 * pyrad_amd.model.Atmosphere.fluxes: upward and downward fluxes at every level of a column and, from them, heating rates.
 * Layers l = 0 .. n_layers-1 bottom to top, levels i = 0 .. n_layers (level i is the lower boundary of layer i, level 0
 * the surface, level n_layers the top).  At grid point nu_j = linspace(range_min, range_max, n)[j], for every angle k with
 * cosine mu_k in (0, 1] and weight W_k:
 *   t_lk  = exp(-k_l(nu_j) depth_l / mu_k)        k_l = abs_coef[l] (the layer's absorption coefficient)
 *   B_l   = B(nu_j, T_l)                          (pyradPlanck.py:38-44)
 *   up:    I_up[0]   = I_surface[j] or B(nu_j, surface_T)      I_up[l+1] = t_lk I_up[l] + (1 - t_lk) B_l
 *   down:  I_down[L] = I_top[j] or 0                          I_down[l] = t_lk I_down[l+1] + (1 - t_lk) B_l
 *   spectral flux F_up_i(nu_j) = sum_k W_k I_up[i]  (likewise F_down)
 *   level_flux[b][0][i] = sum over j in band b of nan_to_num(F_up_i(nu_j)), level_flux[b][1][i] likewise for F_down:
 *   n_bands x 2 x (n_layers + 1) doubles, band b = grid points [band_first[b], band_first[b] + band_count[b]).
 * The caller multiplies by the grid step to get W m^-2 (integrateSpectrum's convention).  up_top / down_surface (may be
 * NULL; n points each) receive F_up at the top and F_down at the surface at every point of every band, 0 elsewhere.
 * The surface is black (emissivity 1); I_surface / I_top are isotropic radiances in the units of lbl_column_fold_dev's I_in.
 * Arithmetic: lbl_column_fold_dev's (one Planck term per point and layer shared by all angles, exp(-tau / mu_k) as
 * exp(-tau * (1 / mu_k))), so with the one angle (1, pi) F_up at the top is pi times the fold's I_out, bit for bit wherever
 * the fold takes its one-exp-per-thread Planck path.  Sums in a fixed order, no atomics: the same inputs give the same bits.
 * At most lbl_limit("flux_angles") = 8 angles and lbl_limit("flux_bands") = 64 bands; "sweep_ieee_divisions" 1 gives
 * LBL_ERR_BAD_ARG, as for the fold.  Stream-ordered on the context's stream; nothing is synchronised. */
int lbl_column_flux_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T, const double* depth,
                        double range_min, double range_max, int64_t n,
                        lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top,
                        int n_angles, const double* mu, const double* weight,
                        int n_bands, const int64_t* band_first, const int64_t* band_count,
                        lbl_buffer* level_flux, lbl_buffer* up_top, lbl_buffer* down_surface);

/* ---- Jacobians of the outgoing flux (beyond the reference; ABI 5, backward compatible) --------------------------------
 * pyrad_amd.model.Atmosphere.jacobians: analytic sensitivities of the upward flux at the top to every layer's optical
 * depth, every molecule's amount and every layer's (Planck) temperature, in one pass.  Column, layer order, grid, angle
 * set, bands, nan_to_num and conventions of lbl_column_flux_dev.  At grid point nu_j and angle k (mu_k, W_k):
 *   tau_l = k_l(nu_j) depth_l      t_lk = exp(-tau_l / mu_k)      B_l = B(nu_j, T_l)
 *   I_0k  = I_surface[j] or B(nu_j, surface_T)      I_(l+1)k = t_lk I_lk + (1 - t_lk) B_l
 *   A_lk  = prod_{i>l} t_ik  (A_(L-1)k = 1)          A_(-1)k = prod_i t_ik
 *   F(nu_j)           = sum_k W_k I_Lk                                              upward spectral flux at the top
 *   dF/d ln tau_l     = sum_k W_k (tau_l / mu_k) A_lk t_lk (B_l - I_lk)             all absorbers of layer l scaled
 *   dF/d ln n_m       = sum_k W_k (k_m depth_l / mu_k) A_lk t_lk (B_l - I_lk)       term m: term_abs_coef[m] in layer
 *                                                                                   term_layer[m], line shapes held fixed
 *   dF/dT_l (Planck)  = sum_k W_k A_lk (1 - t_lk) dB_l/dT                           absorption coefficients held fixed
 *   dF/dT_s           = sum_k W_k A_(-1)k dB(nu_j, surface_T)/dT                    0 when I_surface is given
 * jac[b] = [F, dF/dT_s, dF/d ln tau_0..L-1, dF/dT_0..L-1, dF/d ln n_0..n_terms-1], each summed over band b's points with
 * nan_to_num: n_bands x (2 + 2 n_layers + n_terms) doubles (the caller multiplies by the grid step).  jac_ln_tau_spectra /
 * jac_T_spectra (may be NULL; n_layers x n doubles, layer-major) receive the spectral dF/d ln tau_l and dF/dT_l at every
 * point of every band, 0 elsewhere.  The molecule terms are sensitivities at fixed line shapes (the self-broadening fraction
 * of the Lorentz width is not differentiated); the temperature terms are the Planck part only.  The absorption part of
 * dF/dT_l is a term like any other: pass dk_l/dT (lbl_xsec_voigt_dt_dev, weighted as k_l is) as term_abs_coef[m] with
 * term_layer[m] = l; the term sums are linear in the term and do not depend on its sign.
 * Arithmetic: the upward pass is lbl_column_flux_dev's; the downward pass keeps A and E_lk = sum_{i>l} A_ik (1 - t_ik) B_i
 * and evaluates A_lk t_lk (B_l - I_lk) as A_lk B_l + E_lk - I_Lk, clamped to [-A_lk t_lk max_i I_ik, A_lk t_lk B_l] (exact
 * bounds for non-negative sources), so that no per-level radiance is stored.  Sums in a fixed order, no atomics: the same
 * inputs give the same bits.  At most 8 angles, 64 bands and lbl_limit("jacobian_terms") = 512 terms; "sweep_ieee_divisions"
 * 1 gives LBL_ERR_BAD_ARG.  Everything is checked before anything is enqueued.  Stream-ordered; nothing is synchronised. */
int lbl_column_jacobian_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T, const double* depth,
                            double range_min, double range_max, int64_t n,
                            lbl_buffer* I_surface, double surface_T,
                            int n_angles, const double* mu, const double* weight,
                            int n_bands, const int64_t* band_first, const int64_t* band_count,
                            int n_terms, lbl_buffer* const* term_abs_coef, const int32_t* term_layer,
                            lbl_buffer* jac, lbl_buffer* jac_ln_tau_spectra, lbl_buffer* jac_T_spectra);

/* ---- ray paths (beyond the reference; ABI 5, backward compatible) -----------------------------------------------------
 * pyrad_amd.model.Atmosphere.radiance: the radiance that arrives along arbitrary lines of sight through the column - upward
 * looking, slant from a level inside it, limb - many rays per call.  Layers, abs_coef, T and the grid as lbl_column_flux_dev
 * takes them.  Ray r owns the segments s = ray_first[r] .. ray_first[r + 1] - 1 in the order the light travels (the first
 * segment is the one farthest from the observer); segment s crosses seg_length[s] cm of layer seg_layer[s].  A layer may be
 * skipped, or crossed more than once.  At grid point nu_j:
 *   I    = source_kind[r] == 1 ? (I_source[j] or B(nu_j, source_T)) : 0        (0: cold space, 1: the surface source)
 *   Ttot = 1
 *   per segment, l = seg_layer[s]:   tau = k_l(nu_j) * seg_length[s]      t = exp(-tau)      B = B(nu_j, T_l)
 *                                    I <- t I + (1 - t) B                  Ttot <- Ttot t
 *   radiance[r * n + j] = I          transmittance[r * n + j] = Ttot       (transmittance may be NULL)
 * A ray without segments returns its source and transmittance 1.
 * Arithmetic: lbl_column_flux_dev's step (the same Planck term, exp and update), so a ray through the layers 0 .. L-1 once,
 * bottom to top, with seg_length = depth_l and the surface source gives that call's up_top for the angle set {(1, 1.0)} bit
 * for bit.  Nothing is summed: no reductions and no atomics, the same inputs give the same bits, and a ray's result does not
 * depend on the other rays of the call.
 * LBL_ERR_BAD_ARG: a NULL ctx, list or radiance; n_layers outside 1..lbl_limit("layers_per_column"); n < 1; n_rays outside
 * 1..lbl_limit("ray_paths") = 512 (= "ils_rows": every ray can be a row of one lbl_ils_convolve_dev call); ray_first[0] != 0
 * or a ray_first that decreases; more than lbl_limit("ray_segments") = 65536 segments in all; a segment layer outside
 * [0, n_layers); a length that is negative, NaN or infinite; T[l] not > 0; a source_kind other than 0 or 1; a ray of kind 1
 * with neither I_source nor source_T > 0; a buffer too short (radiance and transmittance hold n_rays x n);
 * "sweep_ieee_divisions" 1, as for the fold.  Everything is checked before anything is enqueued; the host arrays are copied
 * and not retained.  Stream-ordered on the context's stream; nothing is synchronised. */
int lbl_ray_radiance_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                         double range_min, double range_max, int64_t n,
                         int n_rays, const int32_t* ray_first,      /* n_rays + 1, ray_first[0] = 0, non-decreasing */
                         const int32_t* seg_layer, const double* seg_length,   /* ray_first[n_rays] each; cm */
                         const int32_t* source_kind,                /* per ray: 0 cold space (I = 0), 1 surface source */
                         lbl_buffer* I_source, double source_T,
                         lbl_buffer* radiance, lbl_buffer* transmittance /* may be NULL */);

/* ---- reflecting surface (beyond the reference; ABI 5, backward compatible) --------------------------------------------
 * pyrad_amd.model.Atmosphere.fluxes and radiance with ``emissivity``: the lower boundary is a surface of emissivity e(nu) that
 * emits e Is and reflects (1 - e) of what comes down, instead of the black surface of lbl_column_flux_dev and
 * lbl_ray_radiance_dev.  e = emissivity[j] (n points; may be NULL) or emissivity_all at every point.  The values inside an
 * emissivity buffer are not read on the host: a value outside [0, 1] gives the arithmetic result of the expressions below.
 *
 * lbl_column_flux_surface_dev: the arguments, grid, layers, levels, angles, bands, nan_to_num, partial sums and level_flux
 * layout of lbl_column_flux_dev, and at grid point nu_j, for every angle k:
 *   down:   exactly lbl_column_flux_dev's downward walk (I_down[L] = I_top[j] or 0), run FIRST
 *   D_k   = I_down[0] of angle k                     F0 = sum_k W_k D_k   (angle 0 first, as every spectral flux)
 *   R_k   = reflection == 0 ? F0 / Wsum : D_k        0 Lambertian, 1 specular; Wsum = W_0 + W_1 + ... added in angle order
 *   Is    = I_surface[j] or B(nu_j, surface_T)
 *   I_up[0] of angle k = e * Is + (1 - e) * R_k      (every operation rounded: two products, one difference, one sum)
 *   up:     exactly lbl_column_flux_dev's upward walk from there
 * up_surface (may be NULL; n points) receives F_up at level 0, in the layout of up_top / down_surface.
 * Dividing by Wsum - pi for Gauss-Legendre angles on mu in [0, 1], anything for an explicit angle set - makes the reflected
 * upward flux sum_k W_k (1 - e) R_k = (1 - e) F0 under the quadrature itself: the Lambertian surface conserves energy in the
 * discrete scheme whatever the angle set.
 * Identity: with e == 1 at every point and finite downward radiances at the surface, level_flux, up_top and down_surface are
 * lbl_column_flux_dev's bit for bit (1 * Is + 0 * R == Is, and every level's sum receives the same terms in the same order).
 * Emissivity 1 is not a special case of the code.
 * LBL_ERR_BAD_ARG: everything lbl_column_flux_dev refuses; reflection not 0 or 1; emissivity NULL with emissivity_all outside
 * [0, 1] or NaN; an emissivity or up_surface buffer shorter than n; weights whose sum is not finite and > 0;
 * "sweep_ieee_divisions" 1.  Everything is checked before anything is enqueued.  Stream-ordered; nothing is synchronised.
 *
 * lbl_ray_radiance_surface_dev: the arguments and semantics of lbl_ray_radiance_dev, and two things more:
 *   - seg_layer[s] == -1 is a surface marker, not a layer: the ray meets the surface there and is reflected specularly.  Its
 *     seg_length must be 0.  With Is = I_source[j] or B(nu_j, source_T):
 *         I <- e * Is + (1 - e) * I          Ttot <- Ttot * (1 - e)
 *     Any number of markers, anywhere: first, last, adjacent.  A ray of one marker alone returns e Is from cold space.
 *   - a ray that starts at the surface (source_kind 1) starts with I = e * Is + (1 - e) * Rd, Rd = surface_down[j] /
 *     surface_down_norm where surface_down (may be NULL; n points: a hemispheric downward flux at the surface, for example
 *     lbl_column_flux_dev's down_surface, and surface_down_norm the Wsum it was formed with) is given, else 0: the diffuse
 *     (Lambertian) reflection of the downwelling.  Ttot starts at 1 as before.
 * Identities: rays without markers, with e == 1 and without surface_down, return lbl_ray_radiance_dev's bits.  The ray down
 * through the layers L-1 .. 0 over depth_l, a marker, and up through 0 .. L-1 returns lbl_column_flux_surface_dev's up_top for
 * reflection 1 and the angle set {(1, 1.0)}, bit for bit.  A ray's bits do not depend on the other rays of the call.
 * LBL_ERR_BAD_ARG: everything lbl_ray_radiance_dev refuses except a segment layer of -1; a marker whose length is not 0; a
 * ray with a marker when neither I_source nor source_T > 0 is given; emissivity NULL with emissivity_all outside [0, 1] or NaN;
 * an emissivity or surface_down buffer shorter than n; surface_down given with a norm that is not finite and > 0.  Everything
 * is checked before anything is enqueued; the host arrays are copied and not retained.  Stream-ordered; nothing is
 * synchronised.  (lbl_ray_radiance_dev and lbl_ray_jacobian_dev go on refusing a segment layer of -1.) */
int lbl_column_flux_surface_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T, const double* depth,
                                double range_min, double range_max, int64_t n,
                                lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top,
                                int n_angles, const double* mu, const double* weight,
                                int n_bands, const int64_t* band_first, const int64_t* band_count,
                                lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                int reflection /* 0 Lambertian, 1 specular */,
                                lbl_buffer* level_flux, lbl_buffer* up_top, lbl_buffer* down_surface,
                                lbl_buffer* up_surface /* may be NULL */);
int lbl_ray_radiance_surface_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                 double range_min, double range_max, int64_t n,
                                 int n_rays, const int32_t* ray_first,
                                 const int32_t* seg_layer /* -1: surface marker */, const double* seg_length,
                                 const int32_t* source_kind, lbl_buffer* I_source, double source_T,
                                 lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                 lbl_buffer* surface_down /* may be NULL */, double surface_down_norm,
                                 lbl_buffer* radiance, lbl_buffer* transmittance /* may be NULL */);

/* ---- linear-in-optical-depth Planck source (beyond the reference; ABI 5, backward compatible) ---------------------------
 * pyrad_amd.model.Atmosphere.fluxes and radiance with planck="linear": the Planck function is not one value per layer but
 * runs linearly in optical depth between two temperatures, which removes the first-order error of the isothermal layer on a
 * column with a lapse rate.  A ray crosses a piece of a layer with optical depth tau along the ray; Ta is the temperature
 * where the light enters the piece and Tb where it leaves, Ba = B(nu, Ta), Bb = B(nu, Tb):
 *     t = exp(-tau)
 *     I <- t I + (1 - t) Ba + g(tau) (Bb - Ba)          Ttot <- Ttot t
 *     g(tau) = 1 - (1 - t) / tau      (-> tau/2 as tau -> 0, -> 1 as tau -> inf)
 * The first two terms are the isothermal step of lbl_column_flux_dev with its rounding, the third is added afterwards: with
 * Ta == Tb it is g * 0 and the step returns the isothermal one's bits.  g (pyrad_amd/csrc/lbl_linear_source.h, one text for
 * the device and the host) is the expression itself for tau >= tau_0 = 0.25 and the Taylor series tau (1/2 - tau (1/6 - tau
 * (1/24 - ...))) with 11 terms below: truncation below 2^-53 relative, and 2 / tau_0^2 = 32 times a one-ulp error of t above.
 * g(0) = 0 exactly, g(+inf) = 1, NaN stays NaN.
 *
 * lbl_column_flux_linear_dev: lbl_column_flux_surface_dev's arguments and semantics - the downward walk first, the surface
 * with emissivity and reflection, the upward walk, level_flux, the spectra - with T replaced by T_edge, two temperatures per
 * layer: T_edge[2 l] at its bottom edge, T_edge[2 l + 1] at its top edge.  Going up Ta is the bottom edge and Tb the top
 * edge, going down the other way round; tau = k_l depth_l / mu_k.  The surface source stays surface_T or I_surface: a skin
 * temperature may differ from the lowest edge.  A black surface is emissivity NULL with emissivity_all 1.
 *
 * lbl_ray_radiance_linear_dev: lbl_ray_radiance_surface_dev's arguments and semantics - markers, the diffuse start term -
 * with T replaced by seg_T, two temperatures per segment in the light's direction of travel: seg_T[2 s] where it enters
 * segment s, seg_T[2 s + 1] where it leaves.  A marker's pair is ignored.  Rays are carried together where they share their
 * layer sequence AND their segment temperatures (nadir paths at different cosines still do); a ray's bits do not depend on
 * the other rays of the call.
 *
 * The one-exp-per-thread Planck path is chosen as for the fold, with the smallest and largest of ALL edge (segment)
 * temperatures of the call; each of a step's two Planck values then comes from one exp per thread.
 * Identities: with both temperatures of every layer or segment equal to the layer's temperature T_l, every result is the
 * surface variant's bit for bit, and hence the black-surface call's at e == 1.  The ray down through the layers L-1 .. 0 over
 * depth_l, a marker, and up through 0 .. L-1, each segment with its layer's edge temperatures in the direction of travel,
 * returns lbl_column_flux_linear_dev's up_top for reflection 1 and the angle set {(1, 1.0)}, bit for bit.
 * LBL_ERR_BAD_ARG: everything the surface variant refuses; an edge or segment temperature that is not finite and > 0 (a
 * marker's pair excepted); "sweep_ieee_divisions" 1.  Everything is checked before anything is enqueued; the host arrays are
 * copied and not retained.  Stream-ordered; nothing is synchronised. */
int lbl_column_flux_linear_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef,
                               const double* T_edge /* 2 n_layers: bottom, top of layer l */, const double* depth,
                               double range_min, double range_max, int64_t n,
                               lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top,
                               int n_angles, const double* mu, const double* weight,
                               int n_bands, const int64_t* band_first, const int64_t* band_count,
                               lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                               int reflection /* 0 Lambertian, 1 specular */,
                               lbl_buffer* level_flux, lbl_buffer* up_top, lbl_buffer* down_surface,
                               lbl_buffer* up_surface /* may be NULL */);
int lbl_ray_radiance_linear_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef,
                                const double* seg_T /* 2 per segment: entry, exit; a marker's pair is ignored */,
                                double range_min, double range_max, int64_t n,
                                int n_rays, const int32_t* ray_first,
                                const int32_t* seg_layer /* -1: surface marker */, const double* seg_length,
                                const int32_t* source_kind, lbl_buffer* I_source, double source_T,
                                lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                lbl_buffer* surface_down /* may be NULL */, double surface_down_norm,
                                lbl_buffer* radiance, lbl_buffer* transmittance /* may be NULL */);

/* ---- direct solar beam (beyond the reference; ABI 5, backward compatible) ------------------------------------------------
 * pyrad_amd.model.Atmosphere.solarFluxes: collimated beams (suns) that enter at the top, are attenuated along their slant
 * paths, and are reflected by the surface; the gas absorbs and nothing emits.  Without scattering the problem is linear: a
 * sunlit column's fluxes are lbl_column_flux_dev's (or a variant's) plus these, level by level.
 * Column, layer order, levels, grid, bands, nan_to_num, partial sums and the level_flux layout are lbl_column_flux_dev's
 * (range_min / range_max are taken for symmetry: no wavenumber enters).  At grid point nu_j, for beams s = 0 .. n_beams-1 and
 * diffuse angles k = 0 .. n_angles-1 with (mu_k, W_k):
 *   tau_l  = k_l(nu_j) * depth_l
 *   d_sl   = exp(-tau_l * slant[s * n_layers + l])       slant >= 0: path length through layer l per unit depth
 *   down:   S_s[L] = S0[j]                               S_s[l]   = d_sl * S_s[l+1]
 *           F_down_i(nu_j) = sum_s beam_weight[s] * S_s[i]          (beam 0 first: w_0 S_0, then fma(w_s, S_s, .) in order)
 *   surface (e = emissivity[j] or emissivity_all, as lbl_column_flux_surface_dev takes it; albedo 1 - e), F0 = F_down_0(nu_j):
 *     reflection 0 (Lambertian): I_k[0] = ((1 - e) * F0) / Wsum     I_k[l+1] = exp(-tau_l * (1 / mu_k)) * I_k[l]
 *                                F_up_i = sum_k W_k I_k[i]          Wsum = W_0 + W_1 + ... added in angle order
 *     reflection 1 (specular):   U_s[0] = (1 - e) * S_s[0]          U_s[l+1] = d_sl * U_s[l]
 *                                F_up_i = sum_s beam_weight[s] * U_s[i]
 *   level_flux[b][0][i] = sum over j in band b of nan_to_num(F_up_i(nu_j)), level_flux[b][1][i] likewise for F_down_i.
 * No thermal emission enters anywhere and no temperature is an argument.  S0 (n points) is the beams' irradiance on a plane
 * normal to them, W m^-2 per cm^-1; beam_weight[s] is what the host makes of weight_s * mu0_s (the projection onto the
 * horizontal).  up_top, down_surface and up_surface (may be NULL; n points each) receive F_up at the top, F_down at the
 * surface and F_up at the surface at every point of every band, 0 elsewhere.  exp is the flux kernels' (x > 800 gives
 * exp(-800) = 0, a NaN stays a NaN), every operation is rounded on its own (no contraction beside the fma chain named
 * above), sums run in a fixed order without atomics: the same inputs and launch give the same bits.  A beam's operations do
 * not depend on the other beams of the call.
 * At most lbl_limit("flux_angles") = 8 beams and 8 angles, lbl_limit("flux_bands") bands and lbl_limit("layers_per_column")
 * layers; n_angles may be 0 (mu and weight are then not read) when reflection == 1.
 * LBL_ERR_BAD_ARG, all before anything is enqueued: a NULL array or a negative count; a count beyond its limit; S0,
 * level_flux (n_bands x 2 x (n_layers + 1)), an abs_coef, emissivity or a spectrum shorter than n; an empty band or one outside
 * [0, n); a depth that is negative or NaN; a slant that is negative or not finite; a beam weight that is not finite; a mu
 * outside (0, 1] or an angle weight that is not finite; reflection not 0 or 1; emissivity NULL with emissivity_all outside
 * [0, 1] or NaN; reflection 0 with no angle or with weights whose sum is not finite and > 0; "sweep_ieee_divisions" 1, as
 * for lbl_column_flux_dev.  The host arrays are copied and not retained.  Stream-ordered; nothing is synchronised. */
int lbl_column_solar_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* depth,
                         double range_min, double range_max, int64_t n,
                         lbl_buffer* S0, int n_beams, const double* beam_weight,
                         const double* slant /* n_beams x n_layers */,
                         int n_angles, const double* mu, const double* weight,
                         int n_bands, const int64_t* band_first, const int64_t* band_count,
                         lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                         int reflection /* 0 Lambertian, 1 specular */,
                         lbl_buffer* level_flux, lbl_buffer* up_top, lbl_buffer* down_surface,
                         lbl_buffer* up_surface /* may be NULL */);

/* ---- two-stream multiple scattering of the solar beam (beyond the reference; ABI 5, backward compatible) ----------------
 * pyrad_amd.model.Atmosphere.solarFluxesTwoStream: lbl_column_solar_dev's beams through a column whose layers also scatter -
 * a delta-two-stream (quadrature) solution per layer and grid point, the layers joined by the adding method, the surface
 * Lambertian.  Nothing emits.  Column, layer order, levels, bands, nan_to_num and S0 / beam_weight / slant are
 * lbl_column_solar_dev's, except that every slant must be > 0.  Scatterer c < n_scat has one amount per layer,
 * scat_amount[c * n_layers + l], and three numbers per grid point, each from scat_X[c][j] or, where scat_X or scat_X[c] is NULL,
 * from scat_X_all[c]: extinction ext_c (per unit amount), single-scattering albedo ssa_c and asymmetry g_c.
 * Per point, with f_c = g_c^2 if delta_scaling else 0:
 *   alpha_c = ext_c (1 - ssa_c)      sigma_c = (ext_c ssa_c) (1 - f_c)      eta_c = (ext_c ssa_c) (g_c - f_c)
 * Layer l (sums in scatterer order, every operation rounded on its own):
 *   ta = k_l depth_l + sum_c amount_cl alpha_c     ts = sum_c amount_cl sigma_c     tsg = sum_c amount_cl eta_c     t = ta + ts
 *   t == 0: R = 0, T = 1, Td_s = 1, Rb_s = Tb_s = 0.  Otherwise, with D = sqrt(3):
 *   a = ta / t    b = (t - tsg) / t    w = ts / t    g = tsg / ts (0 when ts == 0)
 *   g1 = (D b + D a) / 2    g2 = (D b - D a) / 2    lam = sqrt((D a) (D b))
 *   diffuse:  E = exp(-lam t)    Gam = g2 / (g1 + lam)    oG = (D a + lam) (D b + lam) / (g1 + lam)^2    oE = -expm1(-2 lam t)
 *             den = oG + Gam^2 oE    R = Gam oE / den    T = E oG / den
 *             den == 0 (exactly conservative): R = g1 t / (1 + g1 t), T = 1 / (1 + g1 t)
 *             Ab = (-expm1(-lam t) ((D a + lam) / (g1 + lam))) (1 - Gam E) / den, 0 when den == 0: the layer's diffuse absorptance
 *             1 - R - T, without cancellation
 *   beam s, per unit flux through the horizontal at the layer's top:
 *             m = 1 / slant_sl    Td = exp(-t slant_sl)    g3 = (1 - D g m) / 2    g4 = 1 - g3
 *             a2 = g1 g3 + g2 g4    Tdm = Td
 *             if |1 - lam m| < 1e-6 (the particular solution's pole): m = (1 - 1e-6) / lam and Tdm = exp(-t / m) from here on
 *             Cp = w (g3 - a2 m) / ((1 - lam m) (1 + lam m))     u = w (1 + (D a) (g4 - g3) m) / ((1 - lam m) (1 + lam m))
 *             Y = (Cp T) (1 - Tdm)     Rb = Y + (R u + Cp Ab)     Tb = (u (T - Tdm) + (Cp Tdm) Ab) - Y
 *             This is the particular solution Cp, Cm = Cp - u (= -w (g4 + a1 m) / ..., a1 = g1 g4 + g2 g3) with the homogeneous
 *             one subtracted, Rb = Cp - R Cm - T Cp Tdm, Tb = Cm Tdm - T Cm - R Cp Tdm, regrouped with 1 - R - T = Ab so that
 *             without absorption (Ab = 0, u = 1) Y cancels and Rb + Tb + Td = R + T to rounding.
 * Column: S_s[L] = S0[j], S_s[l] = Td_sl S_s[l+1], Fd_s[i] = beam_weight[s] S_s[i]; direct_i = sum_s beam_weight[s] S_s[i]
 * (beam 0 first, then fma in order, as lbl_column_solar_dev sums); P_l = sum_s Rb_sl Fd_s[l+1], Q_l = sum_s Tb_sl Fd_s[l+1]
 * likewise.  The layer relations
 *   up_(l+1) = T_l up_l + R_l dn_(l+1) + P_l      dn_l = T_l dn_(l+1) + R_l up_l + Q_l      dn_L = 0
 *   up_0 = (1 - e) (dn_0 + direct_0)              e = emissivity[j] or emissivity_all
 * are solved by adding from the top, dn_i = Rs_i up_i + Ds_i with Rs_L = Ds_L = 0 and, c = 1 - R_l Rs_(l+1):
 *   U1 = T_l / c    U0 = (R_l Ds_(l+1) + P_l) / c    Rs_l = R_l + (T_l U1) Rs_(l+1)    Ds_l = Q_l + T_l ((Ds_(l+1) + Rs_(l+1) P_l) / c)
 * then from the surface: up_0 = ((1 - e) (Ds_0 + direct_0)) / (1 - (1 - e) Rs_0), up_(l+1) = U1 up_l + U0, dn_i = Rs_i up_i + Ds_i.
 * level_flux is n_bands x 3 x (n_layers + 1): [band][up, diffuse down, direct][level], band sums of nan_to_num.  up_top,
 * down_surface (diffuse), direct_surface and up_surface (may be NULL; n points each) receive the spectral values at every
 * point of every band, 0 elsewhere.  A point where some layer's t is not finite has NaN in all four and counts as 0 in
 * every band sum; every other point keeps its bits.  exp is the flux kernels'; no contraction beside the fma chains named;
 * sums run in a fixed order without atomics.
 * The first of two kernels writes 5 numbers per level and point into `workspace` (laid out [number][level][point]), the
 * second reads them.  The call works through each band in passes of as many points as the workspace holds: a whole number
 * of tiles of 256 points, at least one; lbl_column_twostream_workspace gives the doubles that hold `points` points in one
 * pass.  The partial sums are laid out by tile of the band, not of the pass: the bits do not depend on the workspace's size.
 * At most lbl_limit("scatterers") = 4 scatterers, lbl_limit("flux_angles") = 8 beams; the other limits are
 * lbl_column_solar_dev's.
 * LBL_ERR_BAD_ARG, all before anything is enqueued: what lbl_column_solar_dev refuses of these arguments (level_flux is
 * n_bands x 3 x (n_layers + 1)); n_scat outside 0 .. 4 or scat_amount NULL with n_scat and n_layers > 0; an amount that is
 * negative or not finite; a scat_X[c] shorter than n; with no buffer, an ext_all that is negative or not finite, an ssa_all
 * outside [0, 1] or an asym_all outside (-1, 1); a slant that is not finite and > 0; delta_scaling not 0 or 1; a
 * workspace of fewer than lbl_column_twostream_workspace(n_layers, 1) doubles.  Stream-ordered; nothing is synchronised. */
int lbl_column_twostream_workspace(int n_layers, int64_t points, int64_t* doubles);
int lbl_column_twostream_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* depth,
                             double range_min, double range_max, int64_t n,
                             lbl_buffer* S0, int n_beams, const double* beam_weight,
                             const double* slant /* n_beams x n_layers */,
                             int n_scat, const double* scat_amount /* n_scat x n_layers */,
                             lbl_buffer* const* scat_ext /* may be NULL, and every entry */, const double* scat_ext_all,
                             lbl_buffer* const* scat_ssa, const double* scat_ssa_all,
                             lbl_buffer* const* scat_asym, const double* scat_asym_all, int delta_scaling,
                             int n_bands, const int64_t* band_first, const int64_t* band_count,
                             lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                             lbl_buffer* workspace, lbl_buffer* level_flux, lbl_buffer* up_top,
                             lbl_buffer* down_surface, lbl_buffer* direct_surface,
                             lbl_buffer* up_surface /* may be NULL */);

/* ---- thermal fluxes through scattering layers (beyond the reference; ABI 5, backward compatible) --------------------------
 * pyrad_amd.model.Atmosphere.fluxesTwoStream: lbl_column_flux_surface_dev's (or _linear_dev's) thermal fluxes through a column
 * whose layers also scatter.  The layer solution - scatterers, delta scaling, ta, ts, tsg, t, a, b, g1, g2, lam, R, T, Ab, the
 * den == 0 and t == 0 branches - and the adding recurrences are lbl_column_twostream_dev's, unchanged; there are no beams.
 * Fluxes are hemispheric: an isotropic radiance I is the flux pi I, and the result corresponds to the angle set
 * {(1 / sqrt(3), pi)} of the other flux calls.  B is the fold's general Planck expression, pa nu^3 / (exp(nu pbkT) - 1).
 * Layer l at nu_j, with Bt = pi B(nu_j, T at the layer's top edge), Bb likewise at its bottom edge, d = Bb - Bt, D = sqrt(3):
 * the two-stream equations with the source (g1 - g2) pi B(tau), B linear in optical depth, have the particular solution
 * F+- = pi B(tau) +- c, c = d / ((g1 + g2) t) = d / (D (t - tsg)) (Toon et al. 1989); with the homogeneous response
 * subtracted the layer emits upward at its top P = (Bt + c) - R (Bt - c) - T (Bb + c) and downward at its bottom
 * Q = (Bb - c) - R (Bb + c) - T (Bt - c), evaluated with 1 - R - T = Ab and 1 + R - T = Ab + 2 R as
 *   h = (Ab + 2 R) / (D (t - tsg)) - T
 *   P = Bt Ab + d h          Q = Bb Ab - d h
 *   t == 0: P = Q = 0;  ta == 0 or den == 0 (nothing absorbs): P = Q = 0 exactly.
 * planck_linear 0: T holds n_layers layer temperatures, Bt = Bb = pi B(nu_j, T_l), so P = Q = Bb Ab and no h is formed.
 * planck_linear 1: T holds 2 n_layers edge temperatures in lbl_column_flux_linear_dev's order, T[2 l] at the bottom edge and
 * T[2 l + 1] at the top edge of layer l; with both equal to T_l every result is planck_linear 0's bit for bit.
 * Column, with lbl_column_twostream_dev's relations and recurrences (Rs, Ds, U1, U0, c = 1 - R Rs):
 *   top:      Rs_L = 0,  Ds_L = pi I_top[j]  or 0 (I_top NULL)
 *   surface:  Es = pi (I_surface[j] or B(nu_j, surface_T)),  e = emissivity[j] or emissivity_all, Lambertian
 *             up_0 = (e Es + (1 - e) Ds_0) / (1 - (1 - e) Rs_0)
 *   then      up_(l+1) = U1 up_l + U0,   dn_i = Rs_i up_i + Ds_i
 * level_flux is n_bands x 2 x (n_layers + 1): [band][up, down][level], band sums of nan_to_num.  up_top, down_surface and
 * up_surface (may be NULL; n points each) receive the spectral values at every point of every band, 0 elsewhere.  A point
 * where some layer's t is not finite has NaN in all three and counts as 0 in every band sum; every other point keeps its bits.
 * The first of two kernels writes 4 numbers per level and point into `workspace` ([number][level][point]), the second reads
 * them; passes, tiles of 256 points and the partial sums by tile of the band are lbl_column_twostream_dev's, so the bits do not
 * depend on the workspace's size.  lbl_column_flux_scatter_workspace gives the doubles that hold `points` points in one pass:
 * 4 (n_layers + 1) per point, whole tiles, at least one.  Every operation is rounded on its own; no atomics.
 * Without scatterers R = 0, T = exp(-D ta), and the result is lbl_column_flux_surface_dev's (_linear_dev's) with the angle
 * set {(1 / sqrt(3), pi)} and Lambertian reflection to rounding: P is (1 - t) Ba + g(tau) (Bb - Ba) at tau = D ta.
 * LBL_ERR_BAD_ARG, all before anything is enqueued: what lbl_column_flux_surface_dev (planck_linear 1: _linear_dev) refuses of
 * the column, the surface source, I_top, the bands, the emissivity and the outputs; what lbl_column_twostream_dev refuses of
 * the scatterers, delta_scaling and the workspace (here lbl_column_flux_scatter_workspace(n_layers, 1) doubles); a
 * temperature that is not finite and > 0; planck_linear not 0 or 1.  The host arrays are copied and not retained.
 * Stream-ordered; nothing is synchronised. */
int lbl_column_flux_scatter_workspace(int n_layers, int64_t points, int64_t* doubles);
int lbl_column_flux_scatter_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef,
                                const double* T /* n_layers, or 2 n_layers: bottom, top of layer l */, int planck_linear,
                                const double* depth, double range_min, double range_max, int64_t n,
                                lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top,
                                int n_scat, const double* scat_amount /* n_scat x n_layers */,
                                lbl_buffer* const* scat_ext /* may be NULL, and every entry */, const double* scat_ext_all,
                                lbl_buffer* const* scat_ssa, const double* scat_ssa_all,
                                lbl_buffer* const* scat_asym, const double* scat_asym_all, int delta_scaling,
                                int n_bands, const int64_t* band_first, const int64_t* band_count,
                                lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                lbl_buffer* workspace, lbl_buffer* level_flux, lbl_buffer* up_top,
                                lbl_buffer* down_surface, lbl_buffer* up_surface /* may be NULL */);

/* ---- Jacobians of the outgoing flux through scattering layers (beyond the reference; ABI 5, backward compatible) -----------
 * pyrad_amd.model.Atmosphere.jacobiansTwoStream: the analytic derivatives of F = up_L, lbl_column_flux_scatter_dev's upward
 * flux at the top, per grid point.  The forward model is that call's, unchanged: scatterers, delta scaling, ta, ts, tsg, t, the
 * layer's R, T, Ab, the sources P, Q of planck_linear 0 and 1, the t == 0, den == 0 and ta == 0 branches, Rs, Ds, U1, U0, the
 * emitting Lambertian surface and I_top.  The level relations are linear in the fluxes, so one adjoint pass gives every row:
 *   above level i:   up_L = Tu_i up_i + ...,   Tu_L = 1,  Tu_i = Tu_(i+1) U1_(i+1)          (the downward walk, with U1)
 *   below level l:   the surface and layers 0 .. l-1 reflect A_l:  A_0 = 1 - e,  A_(l+1) = R_l + T_l^2 A_l / (1 - A_l R_l)
 *   layer l alone changed, with up = up_l, dn' = dn_(l+1), Rs' = Rs_(l+1), Tu' = Tu_(l+1):
 *     w1 = Tu' / ((1 - R Rs') - T^2 A_l Rs' / (1 - R A_l))        w2 = w1 T A_l / (1 - R A_l)
 *     dF = w1 (dT up + dR dn' + dP) + w2 (dT dn' + dR up + dQ)
 *   surface, c0 = 1 - (1 - e) Rs_0:   dF/dEs = Tu_0 e / c0  (times pi dB/dT at surface_T: dF/dT_s; 0 with I_surface),
 *                                     dF/de = Tu_0 (Es - dn_0) / c0
 * The layer depends on its three depths through p = D ta and q = D (t - tsg) alone (D = sqrt(3)): with r = sqrt(p), s = sqrt(q),
 * x = r s, E = exp(-x), Gam = (s - r) / (s + r), G = r s / (s + r)^2 = (1 - Gam^2) / 4, oE = 1 - E^2, N = 4 G + Gam^2 oE
 *   R = Gam oE / N      T = 4 G E / N      Ab = 1 - R - T      h = (Ab + 2 R) / q - T
 *   p R_p  = G (4 x Gam E^2 - oE (1 + Gam^2 E^2)) / N^2        q R_q  = G (4 x Gam E^2 + oE (1 + Gam^2 E^2)) / N^2
 *   p T_p  = 2 G E (Gam oE - x (1 + Gam^2 E^2)) / N^2          q T_q  = -2 G E (Gam oE + x (1 + Gam^2 E^2)) / N^2
 *   p Ab_p = G (oE + 2 x E) / (1 + Gam E)^2                    q Ab_q = -G (oE - 2 x E) / (1 + Gam E)^2
 *   p h_p  = (p Ab_p + 2 p R_p) / q - p T_p                    q h_q  = (q Ab_q + 2 q R_q - (Ab + 2 R)) / q - q T_q
 * R and T are even in r, so they are smooth in p; the products p X_p and q X_q are formed directly and nothing is divided by
 * sqrt(ta) or sqrt(q) (G / N <= 1 / 4).  den == 0: the branch's R = y / (1 + y), T = 1 / (1 + y), y = (p + q) / 2, Ab = 0;
 * t == 0: every derivative is 0.  Sources: planck_linear 0, P = Q = B Ab: dP = dQ = B dAb, dP/dB = dQ/dB = Ab;
 * planck_linear 1: dP = Bt dAb + d dh, dQ = Bb dAb - d dh, dP/dBt = dQ/dBb = Ab - h, dP/dBb = dQ/dBt = h; where P = Q = 0
 * by a branch (t == 0, den == 0, ta == 0) their derivatives are 0.  With p F_p and q F_q the two sums dF above,
 *   fa = p F_p / ta  (0 at ta == 0),   fq = q F_q / (t - tsg)  (0 at t == tsg):   dF/dta = fa + fq,  dF/dts = fq,  dF/dtsg = -fq
 * so the logarithmic derivative of an amount that is 0 is exactly 0, and a term of a layer whose ta is 0 at a point sees fq alone.
 * jac is n_bands x (3 + (1 + NT + n_scat) n_layers + n_terms), band sums of nan_to_num, NT = 1 (planck_linear 0) or 2:
 *   F, dF/dT_s, dF/de,
 *   dF/d ln tau_l        l = 0 .. L-1                 the gas of layer l:  k_l depth_l dF/dta_l
 *   dF/dT                NT per layer, layer by layer  NT = 1: the layer's temperature, (w1 + w2) Ab pi dB/dT; NT = 2: bottom
 *                                                      edge (w1 h + w2 (Ab - h)) pi dB/dT_b, then top edge (w1 (Ab - h) + w2 h)
 *                                                      pi dB/dT_t  (lbl_column_jacobian_linear_dev's order)
 *   dF/d ln amount_cl    c = 0 .. n_scat-1, l = 0 .. L-1:  amount_cl (al_c dF/dta + si_c dF/dts + et_c dF/dtsg) of layer l
 *   dF/d ln n_m          m = 0 .. n_terms-1, lbl_column_jacobian_dev's terms:  term_abs_coef[m] depth_l dF/dta_l, l = term_layer[m]
 * The temperature rows are the Planck part; the absorption part is a term (dk/dT), as for lbl_column_jacobian_dev.
 * jac_ln_tau_spectra (L x n) and jac_T_spectra (NT L x n; both may be NULL) receive the spectral rows, 0 outside every band.
 * up_top (may be NULL) receives lbl_column_flux_scatter_dev's spectrum bit for bit, and the band's F is that call's up at
 * level L bit for bit.  A point where some layer's t is not finite is NaN in the spectra and counts as 0 in every sum.
 * Not differentiated: the scatterers' albedo and asymmetry, and the downward flux at the surface.
 * The first of two kernels writes 5 numbers per level and point into `workspace` ([number][level][point]: that call's four
 * and Tu), the second recomputes each layer; passes, tiles and the partial sums by tile of the band are
 * lbl_column_twostream_dev's: the bits do not depend on the workspace's size, and there are no atomics.
 * lbl_column_jacobian_scatter_workspace gives the doubles that hold `points` points in one pass.
 * LBL_ERR_BAD_ARG, all before anything is enqueued: what lbl_column_flux_scatter_dev refuses of the shared arguments; what
 * lbl_column_jacobian_dev refuses of the terms, jac and the spectra (more than lbl_limit("jacobian_terms") terms, a term
 * layer out of range, a short buffer); a workspace of fewer than lbl_column_jacobian_scatter_workspace(n_layers, 1) doubles;
 * "sweep_ieee_divisions" 1.  The host arrays are copied and not retained.  Stream-ordered; nothing is synchronised. */
int lbl_column_jacobian_scatter_workspace(int n_layers, int64_t points, int64_t* doubles);
int lbl_column_jacobian_scatter_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef,
                                    const double* T /* n_layers, or 2 n_layers: bottom, top of layer l */, int planck_linear,
                                    const double* depth, double range_min, double range_max, int64_t n,
                                    lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top,
                                    int n_scat, const double* scat_amount /* n_scat x n_layers */,
                                    lbl_buffer* const* scat_ext /* may be NULL, and every entry */, const double* scat_ext_all,
                                    lbl_buffer* const* scat_ssa, const double* scat_ssa_all,
                                    lbl_buffer* const* scat_asym, const double* scat_asym_all, int delta_scaling,
                                    int n_bands, const int64_t* band_first, const int64_t* band_count,
                                    lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                    int n_terms, lbl_buffer* const* term_abs_coef, const int32_t* term_layer,
                                    lbl_buffer* workspace, lbl_buffer* jac, lbl_buffer* jac_ln_tau_spectra /* may be NULL */,
                                    lbl_buffer* jac_T_spectra /* may be NULL */, lbl_buffer* up_top /* may be NULL */);

/* ---- radiances through scattering layers (beyond the reference; ABI 5, backward compatible) -------------------------------
 * pyrad_amd.model.Atmosphere.radianceTwoStream: what an instrument sees of lbl_column_flux_scatter_dev's column, by the
 * two-stream source function technique (Toon et al. 1989).  Everything about the column is that call's, unchanged: layers,
 * scatterers and delta scaling, ta, ts, tsg, t, a, b, g1, g2, lam, R, T, Ab, the t == 0 and den == 0 branches, the sources P
 * and Q, the adding recurrences, the surface and I_top; they define the hemispheric fluxes up_i and dn_i at every level over
 * the whole grid [0, n) (there are no bands).  Up to lbl_limit("scatter_views") = 16 views: view v is a cosine view_mu[v] in
 * (0, 1] and a direction, view_down[v] 0: the radiance leaving the top of the column upward; 1: the radiance arriving at the
 * surface downward.
 * Within layer l let s in [0, t] be the scaled optical depth from the layer's top, w = ts / t, g = tsg / ts (0 when ts == 0),
 * a = ta / t, D = sqrt(3), Bs(s) = Bt + (Bb - Bt) s / t (Bt, Bb = pi B at the top and bottom edge as in
 * lbl_column_flux_scatter_dev; equal for planck_linear 0).  F+(s), F-(s) are the two-stream fluxes inside the layer:
 *   dF+/ds =  g1 F+ - g2 F- - (g1 - g2) Bs(s)        F-(0) = dn_(l+1)
 *   dF-/ds =  g2 F+ - g1 F- + (g1 - g2) Bs(s)        F+(t) = up_l           (so F+(0) = up_(l+1), F-(t) = dn_l)
 * The source function in direction +-mu is
 *   S+-(s, mu) = ( a Bs(s) + (w / 2) [ (1 +- D g mu) F+(s) + (1 -+ D g mu) F-(s) ] ) / pi
 * and the radiances are
 *   up view:    Iu_0 = up_0 / pi   (the Lambertian surface: e Es + (1 - e) dn_0 = up_0)
 *               Iu_(l+1) = Iu_l exp(-t / mu) + integral_0^t S+(s, mu) exp(-s / mu) ds / mu            result Iu_L
 *   down view:  Id_L = I_top[j] or 0
 *               Id_l = Id_(l+1) exp(-t / mu) + integral_0^t S-(s, mu) exp(-(t - s) / mu) ds / mu      result Id_0
 *   t == 0:     the layer changes nothing.
 * Evaluation (every operation rounded on its own, exp the flux kernels').  With sigma = F+ + F- - 2 Bs, Delta = F+ - F-,
 * c = (Bb - Bt) / (D (t - tsg)) (0 where ta == 0) and a + w = 1:  pi S+- = Bs + (w / 2) sigma +- (w D g mu / 2) Delta, and
 * sigma and Delta - 2 c solve y'' = lam^2 y, so each is y(0) r0(s) + y(t) r1(s) with r1 = sinh(lam s) / sinh(lam t),
 * r0 = sinh(lam (t - s)) / sinh(lam t) and the edge values from up and dn of the two levels: the linear interpolation at
 * lam == 0 (den == 0 needs no branch), weights in [0, 1] at any thickness.  With u = lam t, tau = t / mu, E = exp(-u),
 * Tv = exp(-tau), x = (1 - lam mu) tau the integrals of 1, r0 + r1 and r1 against exp(-s / mu) ds / mu are
 *   W  = -expm1(-tau)
 *   Wp = (A1 + A2) / (1 + E),  A1 = (x >= 0 ? E : Tv) (-expm1(-|x|)) / |1 - lam mu|  (tau E at x == 0),
 *                              A2 = -expm1(-(tau + u)) / (1 + lam mu)
 *   W1 = (m2 (A1 / tau) - Tv) / (1 + lam mu),  m2 = min(2 u, 2000) / -expm1(-2 u)  (1 at u == 0)
 * and a layer adds, for an up view (a down view: Bt and Bb, and the two edges, exchanged, and the Delta term negated),
 *   pi J = Bb W + g(tau) (Bt - Bb) + (w / 2) (sigma(0) Wp + (sigma(t) - sigma(0)) W1)
 *          + (w D g mu / 2) (2 c (W - Wp) + Delta(0) Wp + (Delta(t) - Delta(0)) W1)
 * with g of lbl_ray_radiance_linear_dev.  A1 is smooth through lam mu == 1 - no point is left out and no mu is moved - and
 * no exponential has a positive argument; a thin layer adds (t / mu) S.
 * Identities.  At mu = 1 / sqrt(3), I = F+- / pi satisfies the transfer equation, so pi Iu_L == up_L and pi Id_0 == dn_0 to
 * rounding.  Without scatterers S = B and the result is lbl_ray_radiance_surface_dev's (_linear_dev's) for the same cosine
 * to rounding.  With one temperature everywhere, the sky included, I = B(T0) for every view.
 * Known limit of the two-term phase function: 1 - D g mu is negative for g mu > 1 / sqrt(3), which delta scaling
 * (g -> g / (1 + g)) avoids; nothing is clamped.
 * radiance is n_views x n.  up_top and down_surface (may be NULL; n points each) receive lbl_column_flux_scatter_dev's
 * spectra bit for bit.  A point where some layer's t is not finite is NaN in every output; every other point keeps its bits.
 * The workspace is lbl_column_flux_scatter_dev's (4 numbers per level and point; the second kernel recomputes the layer
 * from the coefficients); the grid runs in passes of whole 256-point tiles and the bits do not depend on the workspace's
 * size, nor a view's on the other views of the call.  No atomics.
 * LBL_ERR_BAD_ARG, all before anything is enqueued: what lbl_column_flux_scatter_dev refuses of the shared arguments (n == 0
 * among them); n_views outside 1 .. lbl_limit("scatter_views"); NULL view_mu or view_down; a mu outside (0, 1] or NaN; a
 * view_down not 0 or 1; a radiance buffer shorter than n_views * n; a short workspace; "sweep_ieee_divisions" 1.
 * Stream-ordered; nothing is synchronised. */
int lbl_column_radiance_scatter_workspace(int n_layers, int64_t points, int64_t* doubles);
int lbl_column_radiance_scatter_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef,
                                    const double* T /* n_layers, or 2 n_layers: bottom, top of layer l */, int planck_linear,
                                    const double* depth, double range_min, double range_max, int64_t n,
                                    lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top,
                                    int n_scat, const double* scat_amount /* n_scat x n_layers */,
                                    lbl_buffer* const* scat_ext /* may be NULL, and every entry */, const double* scat_ext_all,
                                    lbl_buffer* const* scat_ssa, const double* scat_ssa_all,
                                    lbl_buffer* const* scat_asym, const double* scat_asym_all, int delta_scaling,
                                    lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                    int n_views, const double* view_mu, const int32_t* view_down /* 0 up at the top, 1 down at the surface */,
                                    lbl_buffer* workspace, lbl_buffer* radiance /* n_views x n */,
                                    lbl_buffer* up_top, lbl_buffer* down_surface /* may be NULL */);

/* ---- scattered sunlight along a view (beyond the reference; ABI 5, backward compatible) -----------------------------------
 * pyrad_amd.model.Atmosphere.solarRadianceTwoStream: what an instrument sees of lbl_column_twostream_dev's column in
 * sunlight, by lbl_column_radiance_scatter_dev's source function technique with the beam's single scattering in the source.
 * Everything about the column is lbl_column_twostream_dev's, unchanged: layers, scatterers and delta scaling, ta, ts, tsg, t,
 * w, g, Da, g1, g2, lam, R, T, Ab, the t == 0 and den == 0 branches, the beam's m = 1 / slant_l, g3, g4, a2, Cp, u (Cm = Cp - u)
 * and Td, the move of m to (1 - 1e-6) / lam with Tdm where |1 - lam m| < 1e-6, the sources Rb and Tb, the adding recurrences
 * and the Lambertian surface; they define the hemispheric fluxes up_i, dn_i (diffuse) and the beam's flux through the
 * horizontal Fd_i = beam_weight S_i at every level over the whole grid [0, n) (there are no bands).  One sun per call
 * (n_beams is 1: an instrument sees one sun, and a mean over suns of radiances along a fixed view means nothing): one
 * beam_weight and one slant per layer.  Nothing emits.  Up to lbl_limit("beam_views") = 16 views, view_mu and view_down as
 * lbl_column_radiance_scatter_dev takes them.
 * Within layer l let s in [0, t] be the scaled optical depth from the layer's top, D = sqrt(3), Fd = Fd_(l+1).  F+(s), F-(s)
 * are the two-stream fluxes inside the layer, the system that Cp and Cm are the particular solution of:
 *   dF+/ds =  g1 F+ - g2 F- - w g3 (Fd / m) exp(-s / m)        F-(0) = dn_(l+1)
 *   dF-/ds =  g2 F+ - g1 F- + w g4 (Fd / m) exp(-s / m)        F+(t) = up_l       (so F+(0) = up_(l+1), F-(t) = dn_l)
 * The source function in direction +-mu is
 *   pi S+-(s, mu) = (w / 2) [ (1 +- D g mu) F+(s) + (1 -+ D g mu) F-(s) ]
 *                 + (w / (2 D m)) (1 -+ 3 g mu m) Fd exp(-s / m)
 * The first line is lbl_column_radiance_scatter_dev's scattering term.  The second is the singly scattered beam: the two-term
 * phase function 1 + 3 g cos(Theta) averaged over azimuth, cos(Theta) -> -+ mu m (a plane-parallel beam of cosine m in the
 * layer; the radiance is the azimuthal mean, there is no azimuth argument).  Its normalisation w / (2 D m) per unit Fd is
 * that of the quadrature scheme, not of an exact single-scattering calculation (w / (4 m) per unit Fd, i.e. 2 / sqrt(3)
 * times smaller): it is the one with which I = F+- / pi satisfies the transfer equation at mu = 1 / sqrt(3), a known property
 * of the two-stream source function technique, and what makes the first identity below hold.
 *   up view:    Iu_0 = up_0 / pi   (the Lambertian surface reflects diffuse and direct light alike)
 *               Iu_(l+1) = Iu_l exp(-t / mu) + integral_0^t S+(s, mu) exp(-s / mu) ds / mu            result Iu_L
 *   down view:  Id_L = 0   (the diffuse sky: the solar disc itself is not in it)
 *               Id_l = Id_(l+1) exp(-t / mu) + integral_0^t S-(s, mu) exp(-(t - s) / mu) ds / mu      result Id_0
 *   t == 0:     the layer changes nothing.
 * Where m is moved (the pole lam m = 1), every in-layer beam term - Cp, u, exp(-s / m), the 1 / m and m of the second line -
 * uses the moved m, and the beam's value at the layer's bottom is Fd Tdm: F+-(s) is the solution whose edge values the
 * adding used.  g3, g4 and a2 keep the unmoved m, as in lbl_column_twostream_dev.
 * Evaluation (every operation rounded on its own, exp the flux kernels').  sigma = F+ + F- - (2 Cp - u) Fd exp(-s / m) and
 * Delta = F+ - F- - u Fd exp(-s / m) solve y'' = lam^2 y, so each is y(0) r0(s) + y(t) r1(s) with
 * lbl_column_radiance_scatter_dev's r0, r1 and the edge values
 *   sigma(0) = (up_(l+1) + dn_(l+1)) - (2 Cp - u) Fd          sigma(t) = (up_l + dn_l) - (2 Cp - u) (Fd Tdm)
 *   Delta(0) = (up_(l+1) - dn_(l+1)) - u Fd                   Delta(t) = (up_l - dn_l) - u (Fd Tdm)
 * integrated by that call's Wp and W1 (u there is lam t), unchanged.  With tau = t / mu, Tv = exp(-tau), the beam
 * exponential integrates against exp(-s / mu) ds / mu and exp(-(t - s) / mu) ds / mu to
 *   Xu = -expm1(-(tau + t / m)) / (1 + mu / m)
 *   Xd = (x >= 0 ? Tdm : Tv) (-expm1(-|x|)) / |1 - mu / m|,  x = (1 - mu / m) tau   (tau Tv at x == 0)
 * (1 / m is slant_l, or 1 / (the moved m)), and a layer adds, for an up view,
 *   pi J = (w / 2) (sigma(0) Wp + (sigma(t) - sigma(0)) W1) + (w D g mu / 2) (Delta(0) Wp + (Delta(t) - Delta(0)) W1)
 *        + (Fd Xu) [ (w / 2) (2 Cp - u) + (w D g mu / 2) u + ((w / 2) / D) (1 / m - 3 g mu) ]
 * and for a down view the same with the two edges exchanged, the two w D g mu / 2 terms negated, Xd for Xu and 1 / m + 3 g mu.
 * Xd is smooth through mu == m, Wp and W1 through lam mu == 1: no point is left out and no mu is moved; no exponential has a
 * positive argument and no branch fires at lam == 0 or den == 0; a thin layer adds (t / mu) S.  Near the pole Cp and u reach
 * 1e6 and cancel against sigma and Delta: there the result loses digits (measured within 1.4e-12 of S0 / pi of a float64
 * restatement that is itself within 7.4e-13 of 50 digits; DESIGN.md "K5o"), elsewhere it is good to rounding.
 * Identities.  At mu = 1 / sqrt(3), pi Iu_L == up_L and pi Id_0 == dn_0 to rounding, lbl_column_twostream_dev's own spectra.
 * Without scatterers w = 0 and every J is exactly 0: an up view is lbl_column_solar_dev's Lambertian up_top / pi with the
 * single angle (mu, pi), a down view exactly 0.  A layer split into two of half the amounts and depth gives the same radiances.
 * Known limit of the two-term phase function: 1 - 3 g mu m is negative for g mu m > 1 / 3 (the forward peak seen against the
 * sun), which delta scaling (g -> g / (1 + g)) eases but does not exclude; nothing is clamped.
 * radiance is n_views x n.  up_top, down_surface (diffuse) and direct_surface (may be NULL; n points each) receive
 * lbl_column_twostream_dev's spectra bit for bit.  A point where some layer's t is not finite is NaN in every output; every
 * other point keeps its bits.  The workspace is lbl_column_twostream_dev's (5 numbers per level and point; the second kernel
 * recomputes the layer from the coefficients): lbl_column_beam_radiance_workspace is lbl_column_twostream_workspace.  The
 * grid runs in passes of whole 256-point tiles and the bits do not depend on the workspace's size, nor a view's on the other
 * views of the call.  No atomics.
 * LBL_ERR_BAD_ARG, all before anything is enqueued: what lbl_column_twostream_dev refuses of the shared arguments (one beam:
 * a beam_weight that is not finite, a slant that is not finite and > 0); n < 1; what lbl_column_radiance_scatter_dev refuses
 * of the views (the limit is lbl_limit("beam_views")), the radiance buffer and the workspace; "sweep_ieee_divisions" 1.
 * The host arrays are copied and not retained.  Stream-ordered; nothing is synchronised. */
int lbl_column_beam_radiance_workspace(int n_layers, int64_t points, int64_t* doubles);
int lbl_column_beam_radiance_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* depth,
                                 double range_min, double range_max, int64_t n,
                                 lbl_buffer* S0, double beam_weight, const double* slant /* n_layers */,
                                 int n_scat, const double* scat_amount /* n_scat x n_layers */,
                                 lbl_buffer* const* scat_ext /* may be NULL, and every entry */, const double* scat_ext_all,
                                 lbl_buffer* const* scat_ssa, const double* scat_ssa_all,
                                 lbl_buffer* const* scat_asym, const double* scat_asym_all, int delta_scaling,
                                 lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                 int n_views, const double* view_mu, const int32_t* view_down /* 0 up at the top, 1 down at the surface */,
                                 lbl_buffer* workspace, lbl_buffer* radiance /* n_views x n */,
                                 lbl_buffer* up_top, lbl_buffer* down_surface, lbl_buffer* direct_surface /* may be NULL */);

/* ---- ray-path Jacobians (beyond the reference; ABI 5, backward compatible) --------------------------------------------
 * pyrad_amd.model.Atmosphere.pathJacobians: the weighting functions of the radiance lbl_ray_radiance_dev computes - its
 * analytic derivatives to every crossed layer's optical depth and (Planck) temperature, to the source temperature and to any
 * number of absorber terms - per ray and grid point, in one pass.  Column, grid, rays, segments and sources as
 * lbl_ray_radiance_dev takes them, and its arithmetic on the way out: radiance (may be NULL; n_rays x n) receives that call's
 * radiance bit for bit.  For ray r at grid point nu_j, with I_s the radiance entering segment s (I_s0 the source), t_s =
 * exp(-tau_s), tau_s = k_l(nu_j) seg_length[s], l = seg_layer[s], B_s = B(nu_j, T_l) and A_s = the product of t_i over the
 * segments i after s (1 for the last):
 *   dI/d ln tau_l     = sum over the ray's segments s in layer l of tau_s A_s t_s (B_s - I_s)     all absorbers of l scaled
 *   dI/dT_l (Planck)  = sum over the same segments of A_s (1 - t_s) dB(nu_j, T_l)/dT              k_l held fixed
 *   term m            = sum over the ray's segments s in layer term_layer[m] of term_abs_coef[m][j] seg_length[s] A_s t_s (B_s - I_s)
 *   dI/dT_source      = (the product of all t_s) dB(nu_j, source_T)/dT for source_kind 1 without I_source, else 0
 * The terms are lbl_column_jacobian_dev's: pass a molecule's own absorption coefficient for dI/d ln n_m at fixed line shapes,
 * dk_l/dT (lbl_xsec_voigt_dt_dev) for the absorption part of dI/dT_l; the sums are linear in the term whatever its sign.
 * Rows.  Only the layers a ray crosses have rows (the other derivatives are 0).  Ray r crosses c_r distinct layers
 * l_0 < l_1 < ... and m_r of the terms lie in one of them; it owns the 1 + 2 c_r + m_r consecutive rows from row_first[r]
 * = the sum of the counts of the rays before it:
 *   row 0: dI/dT_source;   rows 1 .. c_r: dI/d ln tau of l_0, l_1, ...;   rows c_r + 1 .. 2 c_r: dI/dT of l_0, l_1, ...;
 *   then its m_r terms in the order of the term list.            jac[row * n + j] is the value at grid point j.
 * lbl_ray_jacobian_rows returns that layout - row_first (n_rays + 1 values, the last one the total; may be NULL) and the
 * total *rows - without a context; it refuses (LBL_ERR_BAD_ARG) the ray lists and term layers lbl_ray_jacobian_dev refuses.
 * Arithmetic: the forward walk keeps the running maximum Imax of I over the source and every segment end; the segments
 * are then walked last to first with A and D = E - I, E = the emission of the later segments that reaches the observer, and
 * A_s t_s (B_s - I_s) is evaluated as A_s B_s + D_s clamped to [-A_s t_s Imax, A_s t_s B_s] (lbl_column_jacobian_dev's form:
 * exact bounds for non-negative sources, no stored radiances).  A layer crossed more than once: its last segment stores the
 * layer's rows, every earlier one adds to them in that fixed order, the same thread each time.  No atomics and nothing
 * zeroed beforehand: the same inputs give the same bits, and a ray's rows do not depend on the other rays of the call.
 * LBL_ERR_BAD_ARG: everything lbl_ray_radiance_dev refuses (radiance may be NULL here); n_terms outside
 * 0..lbl_limit("jacobian_terms") = 512; a NULL term or term list; a term layer outside [0, n_layers); a term buffer shorter
 * than n; jac NULL or shorter than rows x n; rows x n beyond int64.  Everything is checked before anything is enqueued; the
 * host arrays are copied and not retained.  Stream-ordered on the context's stream; nothing is synchronised. */
int lbl_ray_jacobian_rows(int n_layers, int n_rays, const int32_t* ray_first, const int32_t* seg_layer,
                          int n_terms, const int32_t* term_layer,
                          int64_t* row_first /* n_rays + 1, may be NULL */, int64_t* rows);
int lbl_ray_jacobian_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                         double range_min, double range_max, int64_t n,
                         int n_rays, const int32_t* ray_first, const int32_t* seg_layer, const double* seg_length,
                         const int32_t* source_kind, lbl_buffer* I_source, double source_T,
                         int n_terms, lbl_buffer* const* term_abs_coef, const int32_t* term_layer,
                         lbl_buffer* radiance /* n_rays x n, may be NULL */, lbl_buffer* jac /* rows x n */);

/* ---- Jacobians over a reflecting surface (beyond the reference; ABI 5, backward compatible) ----------------------------
 * pyrad_amd.model.Atmosphere.jacobians, pathJacobians and observe with ``emissivity``: the derivatives of what
 * lbl_column_flux_surface_dev and lbl_ray_radiance_surface_dev compute, the emissivity among the variables.
 *
 * lbl_column_jacobian_surface_dev: the arguments of lbl_column_jacobian_dev, plus I_top (may be NULL: 0), emissivity /
 * emissivity_all / reflection as lbl_column_flux_surface_dev takes them, and jac_e_spectrum.  Forward, at grid point nu_j,
 * exactly lbl_column_flux_surface_dev: the downward walk from I_top gives Id_(l+1)k, the radiance entering layer l from
 * above, and D_k = Id_0k; R_k = F0 / Wsum (Lambertian, F0 = sum_k W_k D_k) or D_k (specular); Iu_0k = e Is + (1 - e) R_k;
 * the upward walk gives Iu_lk and F = sum_k W_k Iu_Lk.  With A_lk = prod_{i>l} t_ik, C_lk = prod_{i<l} t_ik, Ttot_k =
 * prod_i t_ik and Q_k = (1 - e) W_k (sum_k' W_k' Ttot_k') / Wsum (Lambertian) or (1 - e) W_k Ttot_k (specular):
 *   gu_lk = A_lk t_lk (B_l - Iu_lk)                upward leg: lbl_column_jacobian_dev's term, the reflecting boundary in Iu
 *   gd_lk = C_lk t_lk (B_l - Id_(l+1)k)            downward leg, seen through the surface
 *   dF/d ln tau_l     = sum_k (tau_l / mu_k) (W_k gu_lk + Q_k gd_lk)
 *   term m (layer l)  = sum_k (term_abs_coef[m][j] depth_l / mu_k) (W_k gu_lk + Q_k gd_lk)
 *   dF/dT_l (Planck)  = sum_k (W_k A_lk + Q_k C_lk) (1 - t_lk) dB_l/dT
 *   dF/dT_s           = e sum_k W_k Ttot_k dB(nu_j, surface_T)/dT                  0 when I_surface is given
 *   dF/de             = sum_k W_k Ttot_k (Is - R_k)
 * jac[b] = [F, dF/dT_s, dF/de, dF/d ln tau_0..L-1, dF/dT_0..L-1, terms]: n_bands x (3 + 2 n_layers + n_terms) doubles, band
 * sums with nan_to_num (of each leg's spectral value), as lbl_column_jacobian_dev.  jac_ln_tau_spectra / jac_T_spectra
 * (may be NULL; n_layers x n) and jac_e_spectrum (may be NULL; n) receive the spectral values at every point of every band, 0
 * elsewhere.  The terms are lbl_column_jacobian_dev's (dk_l/dT as a term gives the absorption part of dF/dT_l).
 * Arithmetic: three walks - down (Id, its running maximum Dmax over the levels, Ttot), up (lbl_column_jacobian_dev's upward
 * walk, and beside it gd_lk = C_lk B_l + D'_lk clamped to [-C_lk t_lk Dmax, C_lk t_lk B_l], D' = (the emission of the layers
 * below l that reaches the surface) - D: lbl_column_jacobian_dev's identity upside down), down (lbl_column_jacobian_dev's
 * downward pass).  No level radiance is stored; sums in a fixed order, no atomics: the same inputs give the same bits.
 * Identity: with e == 1 everywhere and finite downward radiances, for one and two angles every value other than dF/de is
 * lbl_column_jacobian_dev's bit for bit (the reflected leg adds zeros); with more angles the two calls group the points of
 * a thread differently and agree to rounding.
 * LBL_ERR_BAD_ARG: everything lbl_column_jacobian_dev or lbl_column_flux_surface_dev refuses (with jac holding n_bands x (3 +
 * 2 n_layers + n_terms)); a jac_e_spectrum shorter than n; "sweep_ieee_divisions" 1.  Everything is checked before anything
 * is enqueued.  Stream-ordered; nothing is synchronised.
 *
 * lbl_ray_jacobian_surface_dev: the arguments of lbl_ray_jacobian_dev with the rays, markers (seg_layer == -1, length 0) and
 * sources of lbl_ray_radiance_surface_dev without surface_down - a ray that starts at the surface starts with e Is - and that
 * call's radiance bit for bit.  An element of a ray is a segment or a marker; A is the product, over every element after
 * one, of t_s for segments and (1 - e) for markers; A_0 the product over every element of the ray:
 *   dI/d ln tau_l, dI/dT_l, the terms: lbl_ray_jacobian_dev's sums with that A
 *   dI/dT_source = e dBs/dT (sum over the markers m of A_m + [source_kind 1] A_0)          0 when I_source is given
 *   dI/de        = sum over the markers m of A_m (Is - I_m) + [source_kind 1] A_0 Is        I_m: what arrives at the marker
 * Ray r owns 2 + 2 c_r + m_r rows: row 0 dI/dT_source, row 1 dI/de, then lbl_ray_jacobian_dev's order; markers are no
 * layers and have no rows.  lbl_ray_jacobian_surface_rows returns that layout without a context.
 * Arithmetic: lbl_ray_jacobian_dev's two walks; dI/de is carried forward (S <- t S per segment, S <- (Is - I) + (1 - e) S at
 * a marker), Imax includes the markers' results, and on the way back a marker adds A e Is to D and A e dBs/dT to row 0,
 * then A <- A (1 - e).  Rays without a marker, with e == 1, give lbl_ray_jacobian_dev's rows and radiance bit for bit.
 * LBL_ERR_BAD_ARG: everything lbl_ray_jacobian_dev refuses except a segment layer of -1, and what
 * lbl_ray_radiance_surface_dev refuses of markers and emissivity.  Everything is checked before anything is enqueued; the
 * host arrays are copied and not retained.  Stream-ordered; nothing is synchronised.
 * (lbl_ray_jacobian_dev and lbl_ray_jacobian_rows go on refusing a segment layer of -1.) */
int lbl_column_jacobian_surface_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                    const double* depth, double range_min, double range_max, int64_t n,
                                    lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top /* may be NULL */,
                                    int n_angles, const double* mu, const double* weight,
                                    int n_bands, const int64_t* band_first, const int64_t* band_count,
                                    lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                    int reflection /* 0 Lambertian, 1 specular */,
                                    int n_terms, lbl_buffer* const* term_abs_coef, const int32_t* term_layer,
                                    lbl_buffer* jac, lbl_buffer* jac_ln_tau_spectra, lbl_buffer* jac_T_spectra,
                                    lbl_buffer* jac_e_spectrum /* n, may be NULL */);
int lbl_ray_jacobian_surface_rows(int n_layers, int n_rays, const int32_t* ray_first,
                                  const int32_t* seg_layer /* -1: surface marker */,
                                  int n_terms, const int32_t* term_layer,
                                  int64_t* row_first /* n_rays + 1, may be NULL */, int64_t* rows);
int lbl_ray_jacobian_surface_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef, const double* T,
                                 double range_min, double range_max, int64_t n,
                                 int n_rays, const int32_t* ray_first,
                                 const int32_t* seg_layer /* -1: surface marker */, const double* seg_length,
                                 const int32_t* source_kind, lbl_buffer* I_source, double source_T,
                                 lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                 int n_terms, lbl_buffer* const* term_abs_coef, const int32_t* term_layer,
                                 lbl_buffer* radiance /* n_rays x n, may be NULL */, lbl_buffer* jac /* rows x n */);

/* ---- Jacobians of the linear-in-optical-depth Planck source (beyond the reference; ABI 5, backward compatible) -----------
 * pyrad_amd.model.Atmosphere.jacobiansLinear, pathJacobiansLinear and observeLinear: the derivatives of what
 * lbl_column_flux_linear_dev and lbl_ray_radiance_linear_dev compute, the temperatures of the layers' edges and of the
 * segments' ends among the variables.  The step through a piece of optical depth tau, t = exp(-tau), Ba where the light
 * enters and Bb where it leaves, is I_out = t I_in + (1 - t) Ba + g(tau) (Bb - Ba) = t I_in + h(tau) Ba + g(tau) Bb with
 *   h(tau) = (1 - t) - g(tau) = tau g'(tau),   g'(tau) = (1 - t (1 + tau)) / tau^2      (-> 1/2 as tau -> 0, -> 0 as tau -> inf)
 * so that dI_out/d ln tau = tau t (Ba - I_in) + h (Bb - Ba), dI_out/dTa = h dB(Ta)/dT, dI_out/dTb = g dB(Tb)/dT, and for an
 * absorber term k_m over the length x: dI_out = k_m x [t (Ba - I_in) + g'(tau) (Bb - Ba)] - no division by tau, a point
 * without absorption stays finite.  g' is lbl::linear_source_dg of pyrad_amd/csrc/lbl_linear_source.h (the closed form from
 * tau = 3/8 on, its Taylor series below; within 1e-14 relative for a t good to 2 ulp), h is formed as tau g'.
 *
 * lbl_column_jacobian_linear_dev: the arguments of lbl_column_jacobian_surface_dev with T replaced by T_edge (2 per layer:
 * T_edge[2 l] the bottom edge of layer l, T_edge[2 l + 1] its top edge, as lbl_column_flux_linear_dev) and jac_T_spectra by
 * jac_T_edge_spectra (2 n_layers x n: rows 2 l and 2 l + 1 are the bottom and top edge of layer l).  emissivity NULL with
 * emissivity_all 1 is the black surface.  Forward, at grid point nu_j, exactly lbl_column_flux_linear_dev; with that call's
 * Id_(l+1)k, Iu_lk and lbl_column_jacobian_surface_dev's A_lk, C_lk, Ttot_k, Q_k, R_k and Is formed from them, x = k_l
 * depth_l / mu_k, t = exp(-x), Bbot = B(T_edge[2 l]), Btop = B(T_edge[2 l + 1]):
 *   gu_lk = A_lk [x t (Bbot - Iu_lk)     + h(x) (Btop - Bbot)]          upward leg
 *   gd_lk = C_lk [x t (Btop - Id_(l+1)k) + h(x) (Bbot - Btop)]          downward leg, seen through the surface
 *   dF/d ln tau_l     = sum_k (W_k gu_lk + Q_k gd_lk)
 *   term m (layer l)  = sum_k (term_abs_coef[m][j] depth_l / mu_k) (W_k A_lk [t (Bbot - Iu_lk) + g'(x) (Btop - Bbot)]
 *                                                                 + Q_k C_lk [t (Btop - Id_(l+1)k) + g'(x) (Bbot - Btop)])
 *   dF/dT_bottom(l)   = dB(T_edge[2 l])/dT     sum_k (W_k A_lk h(x) + Q_k C_lk g(x))
 *   dF/dT_top(l)      = dB(T_edge[2 l + 1])/dT sum_k (W_k A_lk g(x) + Q_k C_lk h(x))
 *   dF/dT_s, dF/de    : lbl_column_jacobian_surface_dev's expressions
 * jac[b] = [F, dF/dT_s, dF/de, dF/d ln tau_0..L-1, dF/dT_edge_0..2L-1, terms]: n_bands x (3 + 3 n_layers + n_terms) doubles,
 * band sums with nan_to_num (of each leg's spectral value), as lbl_column_jacobian_surface_dev; the spectra likewise.  The
 * derivative with respect to a level temperature that two layers share is the sum of the two edge values.
 * Arithmetic: lbl_column_jacobian_surface_dev's three walks with lbl_column_flux_linear_dev's step.  With A the
 * transmittance behind a step and D = (the emission behind it that reaches the end) - I_end,
 *   A t (Ba - I_in) = A (Ba + g (Bb - Ba)) + D,   clamped to [-A t Imax, A t Ba]
 * so no level radiance is stored; sums in a fixed order, no atomics: the same inputs give the same bits.  F agrees with
 * lbl_column_flux_linear_dev's upward flux at the top to rounding, not to the bit: the two calls group the points of a
 * thread differently (4, or 2 beyond two angles, against 4).
 * LBL_ERR_BAD_ARG: everything lbl_column_jacobian_surface_dev or lbl_column_flux_linear_dev refuses (an edge temperature
 * that is not finite and > 0 among it), with jac holding n_bands x (3 + 3 n_layers + n_terms) and jac_T_edge_spectra 2
 * n_layers x n; "sweep_ieee_divisions" 1.  Everything is checked before anything is enqueued.  Stream-ordered.
 *
 * lbl_ray_jacobian_linear_dev: the arguments of lbl_ray_jacobian_surface_dev with T replaced by seg_T (2 per segment:
 * seg_T[2 s] where the light enters segment s, seg_T[2 s + 1] where it leaves; a marker's pair is ignored), the forward
 * model of lbl_ray_radiance_linear_dev without surface_down, and that call's radiance bit for bit (the same step on the same
 * groups of points).  With lbl_ray_jacobian_surface_dev's A_s (the product over the elements after s):
 *   dI/d ln tau_l = sum over the ray's segments s in l of A_s [tau_s t_s (Ba_s - I_s) + h(tau_s) (Bb_s - Ba_s)]
 *   term m        = sum over the same segments of term_abs_coef[m][j] seg_length[s] A_s [t_s (Ba_s - I_s) + g'(tau_s) (Bb_s - Ba_s)]
 *   dI/dTa_s      = A_s h(tau_s) dB(Ta_s)/dT,   dI/dTb_s = A_s g(tau_s) dB(Tb_s)/dT        per segment, not per layer
 *   dI/dT_source, dI/de: lbl_ray_jacobian_surface_dev's
 * Ray r, with c_r crossed layers, s_r segments that are not markers and m_r terms, owns 2 + c_r + 2 s_r + m_r rows: row 0
 * dI/dT_source, row 1 dI/de, the c_r rows d ln tau in ascending layer order, then for each segment that is no marker, in
 * order of travel, dI/dTa_s and dI/dTb_s, then the terms.  A segment's two rows are stored once and never added to; the
 * layer rows and the terms keep lbl_ray_jacobian_dev's rule (the last segment stores, the earlier ones add).
 * lbl_ray_jacobian_linear_rows returns that layout without a context.  A ray's rows and radiance do not depend on the rays
 * it travels with, and the same inputs give the same bits.
 * LBL_ERR_BAD_ARG: everything lbl_ray_jacobian_surface_dev or lbl_ray_radiance_linear_dev refuses (a segment temperature
 * that is not finite and > 0, a marker's pair excepted), with jac holding the rows of this layout; "sweep_ieee_divisions" 1.
 * Everything is checked before anything is enqueued; the host arrays are copied and not retained.  Stream-ordered. */
int lbl_column_jacobian_linear_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef,
                                   const double* T_edge /* 2 n_layers: bottom, top */,
                                   const double* depth, double range_min, double range_max, int64_t n,
                                   lbl_buffer* I_surface, double surface_T, lbl_buffer* I_top /* may be NULL */,
                                   int n_angles, const double* mu, const double* weight,
                                   int n_bands, const int64_t* band_first, const int64_t* band_count,
                                   lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                   int reflection /* 0 Lambertian, 1 specular */,
                                   int n_terms, lbl_buffer* const* term_abs_coef, const int32_t* term_layer,
                                   lbl_buffer* jac, lbl_buffer* jac_ln_tau_spectra,
                                   lbl_buffer* jac_T_edge_spectra /* 2 n_layers x n, may be NULL */,
                                   lbl_buffer* jac_e_spectrum /* n, may be NULL */);
int lbl_ray_jacobian_linear_rows(int n_layers, int n_rays, const int32_t* ray_first,
                                 const int32_t* seg_layer /* -1: surface marker */,
                                 int n_terms, const int32_t* term_layer,
                                 int64_t* row_first /* n_rays + 1, may be NULL */, int64_t* rows);
int lbl_ray_jacobian_linear_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* abs_coef,
                                const double* seg_T /* 2 per segment: entry, exit */,
                                double range_min, double range_max, int64_t n,
                                int n_rays, const int32_t* ray_first,
                                const int32_t* seg_layer /* -1: surface marker */, const double* seg_length,
                                const int32_t* source_kind, lbl_buffer* I_source, double source_T,
                                lbl_buffer* emissivity /* may be NULL */, double emissivity_all,
                                int n_terms, lbl_buffer* const* term_abs_coef, const int32_t* term_layer,
                                lbl_buffer* radiance /* n_rays x n, may be NULL */, lbl_buffer* jac /* rows x n */);

/* ---- instrument channels (beyond the reference; ABI 5, backward compatible) -------------------------------------------
 * pyrad_amd.model.convolve / Atmosphere.observe: n_rows device-resident spectra on the base grid linspace(range_min,
 * range_max, n) convolved with an instrument line shape (ILS) onto n_channels channels, so that channel radiances and channel
 * weighting functions come down instead of spectra.  Row r is the n doubles at src[r] + src_offset[r] (several rows may
 * share a buffer).  Channel c has a centre position[c] in grid-index units ((centre - range_min) / step, fractional), a
 * width[c] in cm^-1 and the support [first[c], first[c] + count[c]) of grid points.  With step = (range_max - range_min) /
 * (n - 1), the step the other entry points use:
 *   x_cj = ((double)j - position[c]) * step      t_cj = x_cj / width[c]      w_cj = shape(t_cj)
 *   out[r * n_channels + c] = (sum_{j in support} w_cj S_r[j]) / (sum_{j in support} w_cj)
 *   shape 0 gaussian  exp(-4 ln2 t^2)                      width = FWHM
 *         1 triangle  max(0, 1 - |t|)                      width = FWHM = half the base
 *         2 boxcar    1 for |t| <= 0.5, else 0             width = full width
 *         3 sinc      sin(pi t) / (pi t), 1 at t = 0       width = centre to first zero = 1 / (2 OPD)
 *         4 table     table[0 .. n_table) sampled uniformly over x in [-table_half, +table_half], 0 outside; at x_cj:
 *                     u = (x + table_half) * ((n_table - 1) / (2 table_half)), i = min(floor(u), n_table - 2),
 *                     w = table[i] + (u - i) * (table[i + 1] - table[i]); width is ignored (may be NULL)
 * Nothing is renormalised beyond the division above: a support cut short changes the channel, it is the caller's to choose
 * (pyrad_amd.model.Instrument.support).  A sum of weights of 0 gives the IEEE result of the division.
 * Arithmetic: numerators and the normaliser are accumulated as unevaluated fp64 pairs (exact products, two-sum) in one fixed
 * order - per thread, per wave, the workgroup's four waves - without atomics: the same inputs give the same bits, a row's
 * result does not depend on the other rows of the call, and a constant row returns its constant bit for bit.
 * LBL_ERR_BAD_ARG: n_rows outside 1..lbl_limit("ils_rows") = 512; n_channels outside 1..lbl_limit("ils_channels") = 65536;
 * count[c] < 1, first[c] < 0 or first[c] + count[c] > n; width[c] not > 0 (shapes 0-3); an unknown shape; shape 4 with
 * n_table outside 2..lbl_limit("ils_table") = 4096 or table_half not > 0; a NULL src[r] or out; a row that does not fit its
 * buffer; out shorter than n_rows x n_channels.  Everything is checked before anything is enqueued; the host arrays are
 * copied and not retained.  Stream-ordered; nothing is synchronised. */
int lbl_ils_convolve_dev(lbl_ctx* ctx, double range_min, double range_max, int64_t n,
                         int n_rows, lbl_buffer* const* src, const int64_t* src_offset,
                         int64_t n_channels, const double* position, const double* width,
                         const int64_t* first, const int64_t* count,
                         int shape, int n_table, double table_half, const double* table,
                         lbl_buffer* out);

/* ---- k-distributions (beyond the reference; ABI 5, backward compatible) -------------------------------------------------
 * pyrad_amd.model.kDistribution / Atmosphere.kDistribution: the points of a band re-ordered by the size of a row (an
 * absorption coefficient, usually) and rows averaged over intervals of that rank, so that the tables correlated-k schemes are
 * built from come down instead of spectra.
 * Rows and bands.  Row r is the n doubles at src[r] + src_offset[r] on the base grid (several rows may share a buffer).
 * Band b is the index range [band_first[b], band_first[b] + band_count[b]); there are 1..lbl_limit("flux_bands") = 64 of
 * them, they may overlap, and each holds at most 2^31 - 1 points.  Every per-point output is laid out band after band: band
 * b occupies [S_b, S_b + band_count[b]) with S_b the sum of the counts of the bands before it; a row's output is S_total =
 * sum_b band_count[b] long, and row r's starts at r * S_total.
 * Order.  The order of row x in band b is exactly first_b + numpy.argsort(x[first_b : first_b + count_b], kind="stable"):
 * ascending; -0.0 and +0.0 tie; every NaN of either sign sorts after +inf; ties keep grid order.  (The pairs (key, index
 * in the band) are ranked, key = the value's bits in sign-magnitude order after -0 -> +0 and NaN -> all ones: all pairs are
 * distinct, so the result does not depend on the sorting algorithm.)  order[r * S_total + S_b + j] is the grid index of the
 * j-th smallest point as a double, as centre indices travel elsewhere in this library; sorted[...] is the row's value there,
 * bit for bit (payloads and signs of zero included).
 *
 * lbl_rank_order_dev ranks all bands of all rows in one call: tiles of 2,048 points are sorted in LDS by one launch, and a
 * band of more points takes ceil(log2(count / 2048)) merge passes over the work space `work`, which holds
 * lbl_rank_order_workspace(...) doubles: 0 when no band is longer than 2,048 points (work may then be NULL), else
 * 3 * n_rows * S_total.  `sorted` may be NULL.  The outputs must not overlap the rows or the work space.
 * LBL_ERR_BAD_ARG: a NULL argument; n < 1; n_rows outside 1..lbl_limit("kdist_rows") = 512; n_bands outside 1..64; a band
 * that is empty, longer than 2^31 - 1 or not inside [0, n); a row that does not fit its buffer; order or sorted shorter than
 * n_rows * S_total; work shorter than the work space.  lbl_rank_order_workspace needs no context and refuses the same row
 * and band counts. */
int lbl_rank_order_workspace(int n_rows, int64_t n, int n_bands, const int64_t* band_count, int64_t* doubles);
int lbl_rank_order_dev(lbl_ctx* ctx, int64_t n, int n_rows, lbl_buffer* const* src, const int64_t* src_offset,
                       int n_bands, const int64_t* band_first, const int64_t* band_count,
                       lbl_buffer* work, lbl_buffer* order, lbl_buffer* sorted);
/* lbl_ranked_means_dev averages n_rows rows over intervals of a rank.  Row r is ranked by the S_total doubles at order[r] +
 * order_offset[r] - one row of an `order` output of lbl_rank_order_dev for the same bands; several rows may name the same
 * one.  Band b has G_b = n_intervals[b] intervals, 1..lbl_limit("kdist_intervals") = 256, given by G_b + 1 rank edges
 * 0 = e_0 < e_1 < ... < e_G = band_count[b]; `edges` holds the bands' edges one band after the other (sum_b (G_b + 1)
 * values).  With G_total = sum_b G_b and Gs_b the sum of G of the bands before b:
 *   mean [mean_offset  + r * G_total             + Gs_b     + i] = (sum_{q = e_i}^{e_(i+1) - 1} x_r[order_r[S_b + q]]) / (e_(i+1) - e_i)
 *   lower[lower_offset + r * (G_total + n_bands) + Gs_b + b + i] = x_r[order_r[S_b + e_i]]            for i < G_b
 *                                                                  x_r[order_r[S_b + count_b - 1]]    for i = G_b
 * (lower may be NULL): the order statistics at the edges, bit-exact when the row is ranked by its own order.  An interval of
 * one rank returns its value bit for bit.  Every sum is taken in one fixed order - 2,048 ranks per workgroup: per thread,
 * the wave's 64 by a fixed tree, the four waves in order; then the interval's partial sums the same way - without atomics:
 * two calls give the same bits and a row's result does not depend on the rows beside it.  Inf and NaN pass through as IEEE
 * arithmetic gives them.  An order value that is no grid index of its band is clamped into the band (NaN: its first point),
 * so no read leaves the row.  `work` holds lbl_ranked_means_workspace(...) doubles: n_rows * sum over all intervals of
 * ceil((e_(i+1) - e_i) / 2048).
 * LBL_ERR_BAD_ARG: a NULL argument other than lower; rows and bands as above; G_b outside 1..256; edges that do not start
 * at 0, do not end at band_count[b] or are not strictly increasing; a row or an order that does not fit its buffer; a
 * negative offset; mean, lower or work too short.
 * Both entry points check everything before anything is enqueued; the host arrays are copied and not retained.
 * Stream-ordered; nothing is synchronised. */
int lbl_ranked_means_workspace(int n_rows, int n_bands, const int64_t* band_count, const int32_t* n_intervals,
                               const int64_t* edges, int64_t* doubles);
int lbl_ranked_means_dev(lbl_ctx* ctx, int64_t n, int n_rows, lbl_buffer* const* src, const int64_t* src_offset,
                         lbl_buffer* const* order, const int64_t* order_offset,
                         int n_bands, const int64_t* band_first, const int64_t* band_count,
                         const int32_t* n_intervals, const int64_t* edges, lbl_buffer* work,
                         lbl_buffer* mean, int64_t mean_offset, lbl_buffer* lower, int64_t lower_offset);

/* ---- resident column (ABI 5) ---------------------------------------------------------------------------------------
 * The argument blocks of a column's merged accumulate jobs (lbl_layers_merged_accumulate_dev) and of its fold
 * (lbl_column_fold_dev) kept on the C side between calls, so that a host's per-call work does not grow with layers x line
 * lists: pyrad_amd.model.Atmosphere.transmission (the fold of pyradClasses.py:784-787 over the layers' absorption
 * coefficients, pyradClasses.py:707-712) is ONE call of lbl_column_transmission and one lbl_download_wait.
 *   lbl_column_create        arguments as lbl_layers_merged_accumulate_dev plus the layers' depths; all layers share one
 *                            wavenumber range and base grid.  The handle owns nothing on the device: line lists and buffers stay
 *                            the caller's and must outlive it (or be replaced with lbl_column_set_layer first).
 *   lbl_column_set_layer     replaces one layer's line lists / parameters / grid / volume fractions / depth / buffer (what a
 *                            mutator of the reference changes: changeTemperature, changePressure, changeRange, changeDepth,
 *                            setPPM ...; the layer keeps its numbers of line lists and molecules)
 *   lbl_column_transmission  due[l] != 0 (due == NULL: every layer): layer l's absorption coefficient is recomputed (ONE merged
 *                            accumulate job per due layer, all in one launch sequence); then the fold bottom to top,
 *                            I <- T_l I + (1 - T_l) B(nu, T_l) with I_0 = I_in or B(nu, surface_T), in `pieces` pieces of the
 *                            grid, each piece's part of I_out copied to host_out (page-locked, lbl_host_alloc; may be NULL: no
 *                            download) while the next piece is folded.  Returns when everything is ENQUEUED:
 *                            lbl_download_wait(ctx) before host_out is read.  The sweeps' default arithmetic only
 *                            ("sweep_ieee_divisions" 1: LBL_ERR_BAD_ARG).  Every argument is checked before anything is
 *                            enqueued: a refused call has not started the due layers' jobs either. */
typedef struct lbl_column lbl_column;
int lbl_column_create(lbl_ctx* ctx, int n_layers, const int32_t* n_iso, lbl_lines* const* lines, const lbl_iso_params* iso,
                      const lbl_grid* grid, const int32_t* iso_mol, const int32_t* n_mol, const double* conc,
                      const double* depth, lbl_buffer* const* abs_coef, lbl_column** out);
int lbl_column_destroy(lbl_column* column);
int lbl_column_set_layer(lbl_column* column, int layer, lbl_lines* const* lines, const lbl_iso_params* iso,
                         const lbl_grid* grid, const double* conc, double depth, lbl_buffer* abs_coef);
int lbl_column_transmission(lbl_column* column, const uint8_t* due, lbl_buffer* I_in, double surface_T, lbl_buffer* I_out,
                            double* host_out, int pieces);

/* Column fold of Layer.transmission over layers bottom to top (pyradClasses.py:784-787):
 *   I <- trans_l * I + (1 - trans_l) * B(nu_j, layer_T[l]),  I_0 = I_in or B(nu_j, surface_T). */
int lbl_column_sweep_dev(lbl_ctx* ctx, int n_layers, lbl_buffer* const* trans, const double* layer_T,
                         double range_min, double range_max, int64_t n,
                         int64_t first, int64_t count,
                         lbl_buffer* I_in, double surface_T, lbl_buffer* I_out);

/* Column step straight from the cross sections: for every grid point, layer after layer (bottom
 * to top), the absorption coefficient and transmittance exactly as lbl_layer_sweep_dev computes
 * them, then the fold of lbl_column_sweep_dev - one pass over the cross sections instead of one
 * sweep launch per layer plus the fold.  Flattened per-layer inputs: layer l owns n_iso[l]
 * consecutive entries of xsec / iso_mol (molecule index 0-based inside the layer, non-decreasing)
 * and n_mol[l] consecutive entries of conc.  abs_coef / trans: NULL, or arrays of n_layers buffers
 * of which any entry may be NULL (that layer's array is then not written). */
int lbl_column_step_dev(lbl_ctx* ctx, int n_layers, const int32_t* n_iso, lbl_buffer* const* xsec,
                        const int32_t* iso_mol, const int32_t* n_mol, const double* conc,
                        const double* P, const double* T, const double* depth,
                        double range_min, double range_max, int64_t n, int64_t first, int64_t count,
                        lbl_buffer* I_in, double surface_T,
                        lbl_buffer* const* abs_coef, lbl_buffer* const* trans, lbl_buffer* I_out);

/* Elementwise optical properties of a transmittance array (pyradClasses.py:73-76, 330-340,
 * 596-606, 718-732): kind 0 emissivity/emittance = 1 - T; 1 absorbance = log10(1/T);
 * 2 optical depth = -ln T. */
int lbl_optical_dev(lbl_ctx* ctx, lbl_buffer* trans, int64_t n, int kind, lbl_buffer* out);

/* out[j] = 0 + in[0][j] + in[1][j] + ... in list order: the aggregation of
 * Molecule.createCrossSection / Layer.createCrossSection (pyradClasses.py:566-571, 684-689). */
int lbl_sum_dev(lbl_ctx* ctx, int n_in, lbl_buffer* const* in, int64_t n, lbl_buffer* out);

/* Planck radiance on the layer axis (pyradPlanck.py:38-44 via pyradClasses.py:781-782). */
int lbl_planck_dev(lbl_ctx* ctx, double range_min, double range_max, int64_t n, double T,
                   lbl_buffer* out);

/* integrateSpectrum (pyradClasses.py:26-29): sum(nan_to_num(y)) * unit_angle * res.
 * Deterministic fixed-tree reduction; synchronous (returns the scalar). */
int lbl_band_integral(lbl_ctx* ctx, lbl_buffer* spectrum, int64_t n, double unit_angle, double res,
                      double* result);

/* Line survey histogram, Isotope.createLineSurvey (pyradClasses.py:409-428): raw S summed
 * into the bin of each line's centre index; out has n_base elements. */
int lbl_line_survey_dev(lbl_ctx* ctx, lbl_lines* lines, const lbl_grid* grid, lbl_buffer* out);

/* ---- graph capture ------------------------------------------------------------------ */
/* A step that repeats (same line lists, grid, buffers) can be captured once and replayed as ONE
 * hipGraph launch: the host then spends microseconds per step instead of rebuilding and checking the
 * launch sequence, which is what bounds a small shard's step on 8 GPUs.
 *   run the sequence once (allocates scratch, builds schedules, uploads descriptors);
 *   lbl_capture_begin(ctx);  the same "_dev" calls again (nothing runs, kernels are recorded);
 *   lbl_capture_end(ctx, &g);   then lbl_graph_launch(g) per step.
 * Inside a capture only kernel launches are possible: a call that would allocate, upload or
 * synchronise returns LBL_ERR_STATE (and the capture must still be ended).  The all-gather is not
 * captured (lbl_allgather_* return LBL_ERR_STATE inside a capture): enqueue it after the graph.  A graph
 * holds pointers into the context's scratch and caches and to the buffers and line lists of the captured
 * calls; lbl_graph_launch returns LBL_ERR_STATE once one of them may have changed (another batch grew a
 * scratch buffer or took a descriptor slot, or ANY buffer or line list of the context was destroyed): capture
 * again.  Page-locked host blocks (lbl_host_alloc) are never captured. */
typedef struct lbl_graph lbl_graph;
int lbl_capture_begin(lbl_ctx* ctx);
int lbl_capture_end(lbl_ctx* ctx, lbl_graph** out);
int lbl_graph_launch(lbl_graph* graph);
int lbl_graph_destroy(lbl_graph* graph);

/* ---- multi-GPU: one process per GPU, grid sharded by contiguous range --------------- */
#define LBL_UNIQUE_ID_BYTES 128
/* Rank 0 calls lbl_comm_unique_id and hands the 128 bytes to every rank out of band
 * (file, env, torch.distributed store, MPI ...); then every rank calls lbl_comm_create. */
int lbl_comm_unique_id(char id[LBL_UNIQUE_ID_BYTES]);
int lbl_comm_create(lbl_ctx* ctx, const char id[LBL_UNIQUE_ID_BYTES], int world_size, int rank,
                    lbl_comm** out);
int lbl_comm_destroy(lbl_comm* comm);
/* The single RCCL all-gather of the path: every rank contributes count doubles starting at
 * send_offset of `send`, and receives world_size*count doubles into `recv` (rank order).
 * Enqueued on the context stream (send may alias recv at its own slot: in-place). */
int lbl_allgather_dev(lbl_comm* comm, lbl_buffer* send, int64_t send_offset, int64_t count,
                      lbl_buffer* recv);
/* Same collective, but the context stream does not wait for it: kernels enqueued afterwards
 * (the next step, on OTHER buffers) overlap the transfer.  `slot` (0..6) names the completion
 * event; lbl_comm_fence_dev(comm, slot) makes the context stream wait (no host sync) for the
 * collective issued with that slot, slot -1 for all of them: call it before send/recv of that
 * collective are touched again.  Collectives run, in issue order, on a stream the communicator owns.
 * "The context stream" is the stream of the context that owns send/recv (both the same, any context of
 * the communicator's device): several contexts of one process - independent steps in flight on streams
 * of their own - share ONE communicator, whose order of collectives stays the same on every rank.  A
 * slot belongs to the context that used it last; reusing it from another context before its fence is
 * LBL_ERR_STATE. */
int lbl_allgather_overlap_dev(lbl_comm* comm, lbl_buffer* send, int64_t send_offset, int64_t count,
                              lbl_buffer* recv, int slot);
int lbl_comm_fence_dev(lbl_comm* comm, int slot);
/* Fewer, larger collectives: stage the shards of several consecutive steps side by side in one batch
 * buffer (rank r, step b of B at [(r*B + b)*S, +S)) and send them with ONE all-gather of B*S doubles per
 * rank.  This is the staging copy: dst[dst_offset .. +n) = src[src_offset .. +n), device to device, async
 * on the stream of the context that owns dst. */
int lbl_gather_stage_dev(lbl_buffer* dst, int64_t dst_offset, lbl_buffer* src, int64_t src_offset, int64_t n);
/* Cost-balanced (unequal) shards: every rank sends `slot` doubles starting at its own first point,
 * so the gathered buffer holds rank r's shard in the first count[r] entries of slot r.  This puts
 * it back in grid order: out[first[r] + i] = gathered[r * slot + i], i < count[r], r < world_size
 * (first / count: host arrays of world_size entries; out at least max(first[r] + count[r]) long). */
int lbl_gather_compact_dev(lbl_ctx* ctx, lbl_buffer* gathered, int world_size, int64_t slot,
                           const int64_t* first, const int64_t* count, lbl_buffer* out);

#ifdef __cplusplus
}
#endif
#endif /* PYRAD_HIP_H */
