// Shared host/device structures of the MI355X line-by-line engine (internal; the public
// boundary is include/pyrad_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lbl_launch_shapes.h"

namespace lbl {

// physical constants exactly as the reference spells them (pyradClasses.py:15-23,
// pyradLineshape.py:14-19, pyradIntensity.py:3-13, pyradPlanck.py:4-9)
constexpr double kB = 1.38064852E-23;
constexpr double cLight = 299792458.0;
constexpr double hPlanck = 6.62607004e-34;
constexpr double kPi = 3.141592653589793;
constexpr double kInvPi = 0.3183098861837907;            // 1/pi
constexpr double kInvSqrtPi = 0.5641895835477563;        // 1/sqrt(pi)
constexpr double t0 = 296.0;
constexpr double p0 = 1013.25;
constexpr double avo = 6.022140857E23;

// One prepared spectral line, in work-grid units, split into the part every (wave, line)
// pair reads (hot, 32 B) and the Gaussian part only pairs near the line centre read (cold,
// 32 B).  The contribution of the line to the grid point at integer offset d from its centre
// ci is
//     KL / (d*d + a2)  +  KG * exp(-b*d*d)          for |d| <= H = window-2,
// which restates pyradLineshape.py:39 (Gaussian), :52 (Lorentz) and :72-74 (pseudo-Voigt)
// times the corrected intensity of pyradIntensity.py:30-32 with x = d*resolution.
struct __attribute__((aligned(32))) HotRec {
    double cf;      // centre index (pyradClasses.py:390) as a double (exact: |ci| <= 2e9)
    double a2;      // (hw / res)^2
    double KL;      // Lorentz amplitude / res^2   (0 for a pure Gaussian line)
    int32_t dgi;    // |d| >= dgi: the Gaussian term cannot change the fp64 value of the sum
    int32_t flags;  // REC_DIRECT_DIV: denominator outside the running-fraction range
};
struct __attribute__((aligned(32))) ColdRec {
    double KG;      // Gaussian amplitude           (0 for a pure Lorentz line)
    double b;       // (res / hw)^2
    double q2;      // exp(-2 b): ratio step of the Gaussian recurrence; < 0: evaluate directly
    double KLd;     // copy of HotRec.KL for the plain-divide pass of REC_DIRECT_DIV lines
};
static_assert(sizeof(HotRec) == 32 && sizeof(ColdRec) == 32, "record halves must be 32 bytes");

enum : int32_t {
    REC_DIRECT_DIV = 1,   // Lorentz denominator outside the running-fraction range: plain divide
    REC_NO_RECUR = 2,     // Gaussian too narrow for the two-exp recurrence (b > 4): one exp per point
    REC_LONG_RUN = 4,     // Gaussian wide enough (b <= 1) for the 16-point runs of the transposed pass: a run that
                          // starts from an underflowed seed cannot reach a point where the term still matters
    REC_LONG_RUN32 = 8    // ... and for its 32-point runs (b <= 0.3)
};

// One accumulate job = one isotopologue of one layer (Isotope.createCrossSection).
// Sweep of a layer fused into the accumulate kernel's output stage (lbl_layer_step_dev): the
// arithmetic of layer_sweep_kernel; per-molecule volume fractions travel with the chain's jobs.
struct FusedSweep {
    double P, T, depth;
    double rT, r_surface_T;         // RN(1/T), RN(1/surface_T) for div_uniform (0: plain divide)
    double start, stop, step;       // xAxis = linspace(start, stop, n)
    double pa, pb, surface_T;
    const double* I_in;
    double* abs_coef; double* trans; double* I_out;
    long long n;
    int32_t on, budget;             // on: 1 the job's sum is a cross section (fold with `factor` / the IEEE chain first); 2 (merged layer job,
                                    // lbl_layer_merged_step_dev) it IS the absorption coefficient.  budget: the sweeps' default arithmetic
                                    // ("sweep_ieee_divisions" 0; see lbl_kernels.hip)
    double factor, pbkT, pbk_surface;   // for it: conc * P / 1E4 / k / T; 100 h c / k / T; 100 h c / k / surface_T
};

struct AccumJob {
    const HotRec* hot;
    const ColdRec* cold;
    const int32_t* cidx;   // centre indices, non-decreasing
    double* out;           // work grid, n_work doubles (NULL: not stored - a merged layer job whose sweep is fused in)
    int32_t n_lines;
    int32_t n_work;
    int32_t H;             // wing support in points = max(window-2, 0)
    int32_t n_tiles;
    int32_t p_begin;       // shard of the work grid computed by this job: [p_begin, p_end)
    int32_t p_end;
    int32_t flush_every;   // lines per running-fraction block: 32, or 16 for very wide windows
    int32_t pad;           // LS variant: tile order (0 XCD-chunked, 1 natural)
    int32_t reserved[2];   // always 0 (the span numbering of the retired variant 4): keeps the offsets of what follows, and so the kernels' code
    // LDS variants with a host schedule: line ranges of every span of 64*R points of this job's
    // shard, 8 ints per span {iA, iB, iC, iD, iF1, iF2, 0, 0} (see wave_line_ranges[_far]); NULL:
    // the wave searches the centre indices itself
    const int32_t* span_tab;
    // Fused layer step of a single-line-list layer (lbl_layer_step_dev): the sweep of a point runs in
    // this job's output stage with the molecule's volume fraction `conc`.
    int32_t chain_flags;
    int32_t ablate;        // LBL_DIAG builds only (lbl_set_option debug_ablate, scripts/ablate.sh): timing-only runs skip parts of the kernel; else 0 and never read
    double conc;
    // Every sum leaves the kernel multiplied by out_scale: 1.0 for a line list's cross section (x * 1.0 is exact), and the
    // power of two 2^e that a merged layer job's record weights were divided by (exact as well), see PrepJob.weight.
    double out_scale;
    // The largest Gaussian cut-off (HotRec.dgi) of every block of 256 records of this job, written by the line prep of the
    // same batch: the far loop skips the per-record reach test of chunks that lie beyond the largest cut-off of the span's
    // blocks.  NULL (lbl_set_option "accum_reach_skip" 0, or records not prepared in this form): every chunk forms the test.
    const int32_t* block_reach;
    FusedSweep fuse;       // fuse.on: sweep every point right after its sum is final
};
enum : int32_t { CHAIN_MOL_FIRST = 1, CHAIN_MOL_LAST = 2 };

// (the span record of the retired variant 4: the name alone, no definition and no user in the library, so that a host-shim
// mock written against the earlier header - it stubbed variant 4's launcher by pointer - still compiles against this one)
struct SpanRec;

struct PrepJob {
    const double* nu; const double* sw; const double* elower; const double* gamma_air;
    const double* gamma_self; const double* n_air; const double* delta_air;
    HotRec* hot; ColdRec* cold; int32_t* cidx;
    unsigned int* block_counts;           // [blocks of 256 lines][3]: per-block regime counts, no atomics
    double T, P, q_frac, molmass, Q_T, Q_296;
    double range_min, resolution;
    double log_t0_over_T;   // ln(296/T), computed once per job on the host
    // per-job constants of the reference's expressions, evaluated once on the host in the reference's
    // operation order (same IEEE results as on the device), and reciprocals of the per-job divisors
    double P_over_p0;       // P / p0                                   (cls:254, 258)
    double ghw_factor;      // sqrt(2 k T / m / c^2), m = molmass/1000/avo (cls:263, 296)
    double q_ratio;         // Q_296 / Q_T                              (int:30-32)
    double inv_T, inv_res, inv_res2;
    double gauss_cut;       // 2^54: the Gaussian part of a pseudo-Voigt line is evaluated until it cannot change the fp64 value of
                            // the line's sum; budget mode 2^34: until it is below 2^-34 (5.8e-11) of the line's own Lorentz term
    int32_t n_lines;
    int32_t pad;
    // Merged layer job (lbl_layer_merged_step_dev, lbl_layers_merged_accumulate_dev): the records of ALL line lists of a layer go
    // into ONE array in centre-index order, each list's amplitudes KL, KG pre-multiplied by weight = conc P / 1E4 / k / T of
    // its molecule (pyradClasses.py:583) over a power of two common to the layer, so that the accumulate kernel's sum is the
    // layer's absorption coefficient sum_m f_m sum_iso xs_iso (pyradClasses.py:707-712, 566-571) up to that exact factor.
    // merged != 0: the list belongs to a job of several lists and is prepared by that job's merged-order launch
    // (line_prep_merged_kernel), which only reads this block's constants and field pointers; weight 1.0 leaves every bit as
    // it was (x * 1.0).
    int32_t merged;
    int32_t pad2;
    double weight;
    // [blocks of 256 lines]: the largest HotRec.dgi of every block, one plain store per block (a list of a merged job: not
    // used, its job's MergedPrep carries the array in merged order); NULL: not written
    int32_t* block_reach;
};

static_assert(sizeof(PrepJob) % 8 == 0, "line_prep_merged_kernel copies PrepJob blocks to LDS in 8-byte words");

// K1 in merged order: one per accumulate job of several line lists
struct MergedPrep {
    const int32_t* src;        // merged position -> (list within the job << 26) | line within the list
    HotRec* hot; ColdRec* cold; int32_t* cidx;       // the job's record arrays
    int32_t first_list, n_lists;                     // the job's lists in the PrepJob array
    int32_t n_total, blocks;                         // lines of all its lists; ceil(n_total / 256)
    int32_t* block_reach;                            // [blocks]: the largest HotRec.dgi of every 256 merged positions; NULL: not written
};
void launch_line_prep_merged(const PrepJob* d_lists, const MergedPrep* d_jobs, int n_jobs, int max_total, hipStream_t s);

// Merge of a layer's sorted centre-index lists (once per window, beside the schedule build): list `a` of a job holds lines
// whose centre indices (tmp_cidx, written by centre_index_kernel with K1's own expression) are non-decreasing; line i of it
// goes to  i + sum_{b < a} #{c_b <= c} + sum_{b > a} #{c_b < c}  - the stable merge, ties by list order - and what is kept is
// the inverse map of the job: src_of_job[position] = (list within the job << 26) | line.
struct MergeList {
    const double* nu;
    int32_t* tmp_cidx;     // this list's centre indices (scratch)
    int32_t* src_of_job;   // out: the job's inverse map (kept with the schedule); the same pointer in all lists of a job
    double range_min, resolution;
    int32_t n_lines;
    int32_t job_first, job_count;     // the lists [job_first, job_first + job_count) of the MergeList array form this list's job
    int32_t pad;
};
void launch_merge_ranks(const MergeList* d_lists, int n_lists, int max_lines, hipStream_t s);

// Device-side schedule build (lbl_kernels.hip "Schedule of a launch group"): one per job of the group
struct SchedJob {
    const int32_t* cidx;   // centre indices K1 wrote for this job in the current batch
    int32_t n_lines, H;
    int32_t p_begin, p_end;
    int32_t span_first;    // first span of this job in the group's span table
    int32_t tile_first;    // first (job, tile) item of this job in the group's positional item list
};
void launch_schedule_build(const SchedJob* d_jobs, int n_jobs, int total_spans, int total_tiles, int R, int spans_per_tile,
                           long long far_reach, double cost_near, double cost_edge, double cost_far, double cost_fixed,
                           int n_cu, int32_t* tabs, void* scratch, int2* worklist, hipStream_t s, int xcd_chunks = 32, bool xcd_pack = true,
                           int single_round_chunks = 1, int xcd_tol = 3, int xcd_local = -1);

// ---- fused sweep arguments (passed by value / by pointer to the sweep kernels) ----------
// line lists of one MERGED accumulate job (6 bits of the merged-order map, PrepJob blocks in K1's LDS) and arrays a layer
// sweep takes as a kernel argument; a layer with more arrays is swept by the column-step kernel, whose term list lives in
// device memory (kMaxColumnIso), so a layer holds up to kMaxColumnIso - 1 line lists (HITRAN knows ~160 isotopologues)
constexpr int kMaxIso = 64;
// A sweep walks a flat list of terms, one per cross-section array, molecule after molecule (and, in a column,
// layer after layer from the bottom): the flags say where a molecule's isotopologue sum is complete
// (pyradClasses.py:566-571 -> 583) and where a layer's molecules are (pyradClasses.py:707-716).
enum : int32_t { TERM_LAST_MOL = 1, TERM_LAST_LAYER = 2 };
struct SweepArgs {
    const double* xsec[kMaxIso];
    double term_conc[kMaxIso];      // volume fraction of the term's molecule
    int32_t term_flags[kMaxIso];
    double term_factor[kMaxIso];    // default arithmetic: conc * P / 1E4 / k / T of the term's molecule (host, the reference's order)
    double pbkT, pbk_surface;       // default arithmetic: 100 h c / k / T, 100 h c / k / surface_T
    int32_t n_iso, n_mol;
    int32_t variant, budget;         // 1: streaming (non-temporal) loads and stores (0 in LBL_DIAG builds with debug_ablate bit 64, for A/B)
    double P, T, depth;
    double rT, r_surface_T;         // RN(1/T), RN(1/surface_T) for div_uniform (0: plain divide)
    double start, stop, step;       // xAxis = linspace(start, stop, n)
    double pa, pb;                  // Planck constants 2E8*h*c**2 and 100*h*c
    double surface_T;               // used when I_in == nullptr
    const double* I_in;
    double* abs_coef; double* trans; double* I_out;
    long long n;
    long long first, count;         // swept sub-range
};
constexpr int kMaxLayers = 128;
constexpr int kMaxColumnIso = 512;      // cross-section arrays (terms) of a whole column
// Column step from the cross sections: per layer the arithmetic of layer_sweep_kernel (absorption
// coefficient, transmittance), folded bottom to top like column_sweep_kernel, in one pass.
struct ColumnStepArgs {
    const double* xsec[kMaxColumnIso];  // (a layer without line lists: one term reading the context's array of zeros)
    double term_conc[kMaxColumnIso];
    // the layer's scalars repeated per term, so that every load of a batch of terms has an address that depends
    // on the term index only (the kernel fetches them with wide scalar loads ahead of the arithmetic)
    double term_P[kMaxColumnIso], term_T[kMaxColumnIso], term_rT[kMaxColumnIso], term_depth[kMaxColumnIso];   // rT = RN(1/T) (0: plain divide)
    double term_factor[kMaxColumnIso], term_pbkT[kMaxColumnIso];     // default arithmetic (see SweepArgs)
    double pbk_surface;
    double pbkT_min, pbkT_max;          // smallest / largest term_pbkT of the column (the kernel's test for its one-exp-per-thread Planck path)
    int32_t term_flags[kMaxColumnIso];
    int32_t n_terms, n_layers;
    int32_t ablate;                     // LBL_DIAG builds only (lbl_set_option debug_ablate, scripts/ablate.sh): timing-only variants; else 0 and never read
    int32_t layer_arrays;               // any of trans[] / abs_coef[] set
    double r_surface_T;
    double* trans[kMaxLayers];          // optional per-layer transmittance outputs
    double* abs_coef[kMaxLayers];       // optional per-layer absorption coefficients
    double start, stop, step, pa, pb, surface_T;
    const double* I_in; double* I_out;
    long long n;
    long long first, count;
};
// Column transport (lbl_column_transport.hip: lbl_column_flux_dev, lbl_column_jacobian_dev): the fold's arithmetic over the
// layers' absorption coefficients for several angles.  One argument block per call; every band is its own launch over the
// same partial-sum scratch, then column_flux_final_kernel adds the partials in a fixed order.
constexpr int kMaxFluxAngles = 8;
constexpr int kMaxFluxBands = 64;
constexpr int kFluxMaxBlocks = 1024;      // workgroups of one band launch (grid-stride beyond): the partials stay bounded
// what both kernels read: the column, its grid, the angle set and the surface source
struct ColumnRT {
    const double* abs_coef[kMaxLayers];
    double depth[kMaxLayers];
    double pbkT[kMaxLayers];            // 100 h c / k / T_l (the budget Planck exponent per wavenumber)
    double pbkT_min, pbkT_max;          // smallest / largest of them (the fold's test for its one-exp-per-thread Planck path)
    double pbk_surface;                 // 100 h c / k / surface_T (used when I_surface == nullptr)
    double rmu[kMaxFluxAngles];         // 1 / mu_k
    double w[kMaxFluxAngles];           // W_k
    double start, stop, step, pa;
    const double* I_surface;            // upward radiance entering at the surface, or nullptr: B(nu, surface_T)
    long long n;
    int32_t n_layers, n_angles;
};
// Level fluxes (K5c): the fold upward from the surface and downward from the top, each level's angle-weighted radiance summed
// over a band of grid points.  Values per band: [up, down][level 0 .. L].
struct FluxArgs : ColumnRT {
    const double* I_top;                // downward radiance entering at the top, or nullptr: 0
    double* up_top;                     // optional: spectral flux F_up at the top
    double* down_surface;               // optional: spectral flux F_down at the surface
};
// Jacobians of the outgoing flux (K5d): K5c's upward fold, then a downward pass that keeps per angle the transmittance to the
// top A and D = E - I_top (E: emission of the layers above that reaches the top), so that A_l t_l (B_l - I_l) = A_l B_l + D_l
// needs no stored radiance.  Values per band: [F_top, dF/dT_s, L x d ln tau, L x dT (Planck part), n_terms x d ln n].
constexpr int kMaxJacobianTerms = kMaxColumnIso;
// Values per band of a column Jacobian call: `head` leading values (K5d: F_top, dT_s; K5h and K5j: and de), per layer one
// d ln tau and `edges` temperature values (1; K5j, the layer's two edges: 2), then the terms.  The kernels' slots in LDS and
// their partials, the launchers' final reductions and the checks of `jac` are all sized by it.
constexpr int jacobian_slots(int head, int edges, int n_layers, int n_terms) { return head + (1 + edges) * n_layers + n_terms; }
struct JacArgs : ColumnRT {
    double rT[kMaxLayers];              // 1 / T_l (dB/dT = B b e^b / ((e^b - 1) T), b = nu pbkT)
    double r_surface_T;                 // 1 / surface_T (used when I_surface == nullptr)
    double wrmu[kMaxFluxAngles];        // W_k / mu_k
    double* ln_tau_spec;                // optional: L x n spectral dF/d ln tau_l
    double* T_spec;                     // optional: L x n spectral dF/dT_l
    const double* term_k[kMaxJacobianTerms];   // the molecule terms sorted by layer (stable)
    int32_t term_slot[kMaxJacobianTerms];      // ... and each one's index in the caller's list
    int32_t layer_term[kMaxLayers + 1];        // terms of layer l: [layer_term[l], layer_term[l + 1])
    int32_t n_terms, pad;
};
// partial blocks one band of `count` points needs at `np` points per thread (the head and tail workgroup included)
int column_transport_partials(long long count, int np);
// one band [first, first + count): partials, then the fixed-order reduction into level_flux[0 .. 2 (n_layers + 1)) /
// jac[0 .. 2 + 2 L + n_terms)
void launch_column_flux(const FluxArgs* d_args, int n_layers, int n_angles, long long first, long long count, double* partial,
                        double* level_flux, hipStream_t s);
void launch_column_jacobian(const JacArgs* d_args, int n_layers, int n_angles, int n_terms, long long first, long long count,
                            double* partial, double* jac, hipStream_t s);

// Ray paths (K5e, lbl_column_transport.hip: lbl_ray_radiance_dev): the fold along an ordered list of (layer, path length)
// segments per ray.  One argument block per call: this header (of ColumnRT the layers' abs_coef and pbkT, the grid and the
// surface source are used), then the tables it names by their byte offset from the block's start, as IlsArgs does.
constexpr int kMaxRayPaths = 512;            // = kMaxIlsRows: every ray can be a row of one lbl_ils_convolve_dev call
constexpr int kMaxRaySegments = 65536;        // of all rays of a call together
constexpr int kRayBundle = 4;                 // rays with one layer sequence that a workgroup carries in registers
struct RayArgs : ColumnRT {
    long long off_ray_first;            // (n_rays + 1) x int32: ray r owns the segments [ray_first[r], ray_first[r + 1])
    long long off_seg_layer;            // n_segments x int32
    long long off_seg_length;           // n_segments doubles, cm
    long long off_source_kind;          // n_rays x int32: 0 cold space, 1 the surface source
    long long off_order;                // n_rays x int32: the rays in dispatch order - kRayBundle n_bundles rays bundle after
                                        // bundle (the rays of a bundle cross the same layers in the same order), then the rest
    double* radiance;                   // n_rays x n, row-major
    double* transmittance;              // likewise, or nullptr
    int32_t n_rays, n_bundles;
};
void launch_ray_radiance(const RayArgs* d_args, long long n, int n_rays, int n_bundles, hipStream_t s);

// Reflecting surface (K5g, lbl_column_transport.hip: lbl_column_flux_surface_dev, lbl_ray_radiance_surface_dev): K5c's two
// walks in the other order - downward first, then upward from I_up[0] = e Is + (1 - e) R - and K5e's walk with surface
// markers (a segment layer of kRaySurfaceMarker) and the diffuse term at a path's start at the surface.  The partials,
// their count and the final reduction are K5c's; the ray tables and the dispatch order K5e's.
constexpr int32_t kRaySurfaceMarker = -1;
struct SurfaceFluxArgs : FluxArgs {
    const double* emissivity;           // n points, or nullptr: emissivity_all
    double emissivity_all;
    double w_sum;                       // W_0 + W_1 + ..., added on the host in angle order (> 0 and finite)
    double* up_surface;                 // optional: spectral flux F_up at the surface
    int32_t reflection, pad;            // 0 Lambertian: R_k = F_down(0) / w_sum; 1 specular: R_k = I_down_k(0)
};
void launch_surface_flux(const SurfaceFluxArgs* d_args, int n_layers, int n_angles, long long first, long long count,
                         double* partial, double* level_flux, hipStream_t s);
struct RaySurfaceArgs : RayArgs {
    const double* emissivity;           // n points, or nullptr: emissivity_all
    double emissivity_all;
    const double* surface_down;         // optional: hemispheric downward flux at the surface, n points
    double surface_down_norm;           // ... and the sum of the weights it was formed with
};
void launch_ray_surface(const RaySurfaceArgs* d_args, long long n, int n_rays, int n_bundles, hipStream_t s);

// Linear-in-optical-depth Planck source (K5i, lbl_column_transport.hip: lbl_column_flux_linear_dev,
// lbl_ray_radiance_linear_dev): K5g's two kernels with two temperatures per layer or segment, the step
// I <- t I + (1 - t) Ba + g(tau) (Bb - Ba) (lbl_linear_source.h).  pbkT_min / pbkT_max are taken over every edge or segment
// temperature of the call.  Partials, ray tables and dispatch order are K5c's and K5e's; the rays of a bundle also share
// their segment temperatures.
struct LinearFluxArgs : SurfaceFluxArgs {
    double pbkT_top[kMaxLayers];        // 100 h c / k / T at the top edge of layer l; ColumnRT's pbkT holds the bottom edge
};
void launch_linear_flux(const LinearFluxArgs* d_args, int n_layers, int n_angles, long long first, long long count,
                        double* partial, double* level_flux, hipStream_t s);
struct LinearRayArgs : RaySurfaceArgs {
    long long off_seg_pbkT;             // 2 n_segments doubles: 100 h c / k / T where the light enters and leaves the segment
                                        // (a marker's pair is 0 and never read); ColumnRT's pbkT is not used
};
void launch_linear_ray(const LinearRayArgs* d_args, long long n, int n_rays, int n_bundles, hipStream_t s);

// Direct solar beam (K5k, lbl_column_transport.hip: lbl_column_solar_dev): collimated beams attenuated down the column along
// their slant paths, reflected by the surface, and the reflected light attenuated on its way up.  No emission anywhere, so
// no temperatures and no grid (a point's wavenumber is never formed).  A block of its own: the beams' slants per layer are
// workgroup-uniform tables.  Values per band as K5c's: [up, down][level 0 .. L]; partials and final reduction are K5c's.
struct SolarArgs {
    const double* abs_coef[kMaxLayers];
    double depth[kMaxLayers];
    double slant[kMaxFluxAngles][kMaxLayers];   // beam s, layer l: path length through the layer per unit depth
    double beam_w[kMaxFluxAngles];      // what multiplies beam s in a level's flux (weight_s mu0_s)
    double rmu[kMaxFluxAngles];         // 1 / mu_k of the diffuse angles (Lambertian reflection)
    double w[kMaxFluxAngles];           // W_k
    double w_sum;                       // W_0 + W_1 + ..., added on the host in angle order (Lambertian: > 0 and finite)
    const double* S0;                   // the beams' irradiance at the top, n points
    const double* emissivity;           // n points, or nullptr: emissivity_all
    double emissivity_all;
    double* f0;                         // Lambertian: F_down at the surface between the two walks, n points - down_surface
                                        // itself where the caller asked for it, else scratch; specular: nullptr
    double* up_top;                     // optional spectra, as SurfaceFluxArgs'
    double* down_surface;
    double* up_surface;
    long long n;
    int32_t n_layers, n_beams, n_angles, reflection;
};
// one band [first, first + count): the downward walk (with the upward one behind it where the reflection is specular), the
// Lambertian upward walk from f0, and the fixed-order reductions into level_flux[0 .. 2 (n_layers + 1))
void launch_solar(const SolarArgs* d_args, int n_layers, int n_beams, int n_angles, int reflection, long long first,
                  long long count, double* partial, double* level_flux, hipStream_t s);

// Two-stream multiple scattering for collimated beams (K5l, lbl_column_transport.hip: lbl_column_twostream_dev): a
// delta-two-stream layer solution per grid point, the layers joined by adding from the top.  Two kernels: the first walks
// down from the top with the direct beams at hand and writes five numbers per level and point into the caller's workspace,
// the second walks up from the surface through those numbers alone and forms every sum.  One point per thread; a tile is the
// kTwoStreamTile points of one workgroup.
constexpr int kMaxScatterers = 4;
constexpr int kTwoStreamTile = 256;
// What the family's argument blocks (K5l here, K5m and K5n below) hold alike: the scatterers, the reflecting surface, the
// workspace and the optional spectra.  The device functions and the host's checks of these fields take this part.
struct ScatterPart {
    double amount[kMaxScatterers][kMaxLayers];  // scatterer c, layer l; 0 for c >= n_scat
    const double* ext[kMaxScatterers];          // n points each, or nullptr: the number beside it (0 for c >= n_scat)
    const double* ssa[kMaxScatterers];
    const double* asym[kMaxScatterers];
    double ext_all[kMaxScatterers], ssa_all[kMaxScatterers], asym_all[kMaxScatterers];
    const double* emissivity;           // n points, or nullptr: emissivity_all
    double emissivity_all;
    double* workspace;                  // quantities x (n_layers + 1) x ws_points
    long long ws_points;                // points of one pass: a whole number of tiles
    double* up_top;                     // optional spectra
    double* down_surface;
    double* up_surface;
    int32_t delta_scaling, pad_scatter;
};
constexpr int kTwoStreamQuantities = 5;    // workspace[q][level][point]: R*, D*, U1, U0 (levels 1 .. L), direct flux
struct TwoStreamArgs : ScatterPart {
    const double* abs_coef[kMaxLayers];
    double depth[kMaxLayers];
    double slant[kMaxFluxAngles][kMaxLayers];   // beam s, layer l: path length through the layer per unit depth, > 0
    double m[kMaxFluxAngles][kMaxLayers];       // 1 / slant, from the host
    double beam_w[kMaxFluxAngles];
    const double* S0;                   // the beams' irradiance at the top, n points
    double* direct_surface;             // optional spectrum, beside ScatterPart's
    int32_t n_layers, pad;
};
// partial-sum slots of a band of `count` points: one per tile up to kFluxMaxBlocks, tile t adds into slot t % slots
int twostream_partials(long long count);
// one pass over the points [first, first + count) of the band that starts at band_first: first - band_first is a multiple of
// the tile and count <= ws_points; the second kernel adds the pass's tiles into their slots of `partial` (zeroed by the
// caller before the band's first pass)
void launch_scatter_pass(const TwoStreamArgs* d_args, int n_beams, long long band_first, long long first, long long count,
                         int slots, double* partial, hipStream_t s);
// the fixed-order reduction of a band's slots into level_flux[0 .. rows (n_layers + 1)): 3 rows for K5l, 2 for K5m
void launch_scatter_final(int rows, int n_layers, int slots, const double* partial, double* level_flux, hipStream_t s);

// Thermal fluxes through scattering layers (K5m, lbl_column_transport.hip: lbl_column_flux_scatter_dev): K5l's layer solution,
// adding, workspace, tiles and partial slots, with the layers' Planck emission as the source, an emitting Lambertian surface
// and a downward flux at the top.  Of ColumnRT the angle set is not used (the two-stream angle is built in).  Values per band
// as K5c's.
constexpr int kScatterFluxQuantities = 4;  // workspace[q][level][point]: R*, D*, U1, U0 (levels 1 .. L)
struct ScatterFluxArgs : ColumnRT, ScatterPart {
    double pbkT_top[kMaxLayers];        // planck_linear: 100 h c / k / T at the top edge of layer l; pbkT holds the bottom edge
    const double* I_top;                // downward radiance entering at the top, or nullptr: 0
};
// K5m's pass (`linear`: two edge temperatures per layer); the slots are twostream_partials', the final is launch_scatter_final
void launch_scatter_pass(const ScatterFluxArgs* d_args, bool linear, long long band_first, long long first, long long count,
                         int slots, double* partial, hipStream_t s);

// Jacobians of the outgoing flux through scattering layers (K5p, lbl_column_transport.hip: lbl_column_jacobian_scatter_dev):
// K5m's downward walk, which also writes Tu (up_L = Tu_i up_i + ...) as a fifth number per level, then one upward walk that
// recomputes each layer, differentiates it and forms every row.  Values per band: [F, dF/dT_s, dF/de, L x d ln tau,
// edges L x dT (layer by layer), n_scat x L d ln amount, n_terms x d ln n].
constexpr int kScatterJacQuantities = 5;   // workspace[q][level][point]: K5m's four, Tu
constexpr int scatter_jacobian_slots(int edges, int n_layers, int n_scat, int n_terms) {
    return 3 + (1 + edges + n_scat) * n_layers + n_terms;
}
constexpr int kScatterJacMaxSlots = scatter_jacobian_slots(2, kMaxLayers, kMaxScatterers, kMaxJacobianTerms);
struct ScatterJacArgs : ScatterFluxArgs {
    double rT[kMaxLayers];              // 1 / T_l (planck_linear: at the bottom edge)
    double rT_top[kMaxLayers];          // planck_linear: 1 / T at the top edge
    double r_surface_T;                 // 1 / surface_T (used when I_surface == nullptr)
    double* ln_tau_spec;                // optional: L x n spectral dF/d ln tau_l
    double* T_spec;                     // optional: edges L x n spectral dF/dT
    const double* term_k[kMaxJacobianTerms];   // the molecule terms sorted by layer (stable), as JacArgs'
    int32_t term_slot[kMaxJacobianTerms];
    int32_t layer_term[kMaxLayers + 1];
    int32_t n_terms, n_scat;
};
// K5p's pass and final reduction: the slots are twostream_partials', nv = scatter_jacobian_slots(...)
void launch_scatter_pass(const ScatterJacArgs* d_args, bool linear, long long band_first, long long first, long long count,
                         int slots, double* partial, hipStream_t s);
void launch_scatter_final_values(int nv, int slots, const double* partial, double* values, hipStream_t s);

// Radiances through scattering layers (K5n, lbl_column_transport.hip: lbl_column_radiance_scatter_dev): K5m's column, whose
// first kernel runs as it stands on the ScatterFluxArgs part of this block (the workspace is K5m's, four numbers per level),
// then one upward walk that integrates the two-stream source function along every view.  No band sums: up_surface stays
// nullptr, and the band fields of ColumnRT are not used.
constexpr int kMaxViews = 16;
constexpr int kMaxScatterViews = kMaxViews, kMaxBeamViews = kMaxViews;     // (lbl_limit's scatter_views and beam_views)
struct ViewPart {                       // the views of K5n and K5o
    double view_mu[kMaxViews];          // the viewing cosines, in (0, 1]; 1 beyond n_views
    double view_rmu[kMaxViews];         // 1 / mu_v, from the host
    int32_t view_down[kMaxViews];       // 0: upward at the top of the column; 1: downward at the surface
    double* radiance;                   // n_views x n
    int32_t n_views, pad_views;
};
struct ScatterRadianceArgs : ScatterFluxArgs { ViewPart views; };
// one pass over the points [first, first + count): first is a multiple of the tile and count <= ws_points
void launch_scatter_radiance_pass(const ScatterRadianceArgs* d_args, bool linear, int n_views, long long first, long long count,
                                  hipStream_t s);

// Scattered sunlight along a view (K5o, lbl_column_transport.hip: lbl_column_beam_radiance_dev): K5l's column with one beam,
// whose first kernel runs as it stands on the TwoStreamArgs part of this block (the workspace is K5l's, five numbers per
// level), then one upward walk that integrates the two-stream source function with the beam's single scattering along every
// view.  No band sums: up_surface stays nullptr.
struct BeamViewArgs : TwoStreamArgs {
    ViewPart views;
    long long n;                        // points of the grid: a view's row of `radiance`
};
// one pass over the points [first, first + count): first is a multiple of the tile and count <= ws_points
void launch_beam_view_pass(const BeamViewArgs* d_args, int n_views, long long first, long long count, hipStream_t s);

// Ray-path Jacobians (K5f, lbl_column_transport.hip: lbl_ray_jacobian_dev): K5e's walk, then the segments last to first
// with K5d's transmittance-and-emission recurrence, one output row per ray, kind and crossed layer.  RayArgs' block with
// more tables behind it; `radiance` may be nullptr here and `transmittance` is not used.  A ray's rows start at row_first[r]:
// [dT_source, c x d ln tau, c x dT, its terms] with c the number of distinct layers it crosses (include/pyrad_hip.h).
constexpr int32_t kRayRowStore = 1 << 30;     // flag of a seg_slot entry: the segment is its layer's first in backward order
struct RayJacArgs : RayArgs {
    double rT[kMaxLayers];              // 1 / T_l
    double r_source_T;                  // 1 / source_T (used when I_surface == nullptr)
    long long off_row_first;            // n_rays x int64: the ray's first row
    long long off_ray_crossed;          // n_rays x int32: c, the distinct layers the ray crosses
    long long off_seg_slot;             // n_segments x int32: rank of the segment's layer among the ray's distinct layers,
                                        // | kRayRowStore where the row is stored, not added to
    long long off_ray_terms;            // n_rays x int32: where the ray's term rows start in the table at off_term_row
    long long off_term_row;             // int32 per sorted term: its row relative to the ray's first (rays that cross the
                                        // same set of layers share one table; entries of layers not crossed are never read)
    double* jac;                        // rows x n, row-major
    const double* term_k[kMaxJacobianTerms];   // the terms sorted by layer (stable)
    int32_t layer_term[kMaxLayers + 1];        // terms of layer l: [layer_term[l], layer_term[l + 1])
    int32_t n_terms, pad;
};
void launch_ray_jacobian(const RayJacArgs* d_args, long long n, int n_rays, int n_bundles, int n_terms, hipStream_t s);

// Jacobians over a reflecting surface (K5h, lbl_column_transport.hip: lbl_column_jacobian_surface_dev,
// lbl_ray_jacobian_surface_dev): K5d's passes behind K5g's downward walk, with the downward leg's derivative carried up
// through the surface, and K5f's walks with surface markers.  Values per band: [F_top, dF/dT_s, dF/de, L x d ln tau, L x dT
// (Planck part), n_terms x term]; a ray's rows: [dT_source, de, c x d ln tau, c x dT, its terms].  Partials, their count and
// the final reduction are K5c's; the ray tables, the dispatch order and the row tables K5e's and K5f's.
struct SurfaceJacArgs : JacArgs {
    const double* I_top;                // downward radiance entering at the top, or nullptr: 0
    const double* emissivity;           // n points, or nullptr: emissivity_all
    double emissivity_all;
    double w_sum;                       // W_0 + W_1 + ..., added on the host in angle order (> 0 and finite)
    double* e_spec;                     // optional: n spectral dF/de
    int32_t reflection, pad2;           // 0 Lambertian, 1 specular (SurfaceFluxArgs)
};
// the points per thread of surface_jacobian_kernel and linear_jacobian_kernel for n_angles (their partials are sized by it)
int jacobian_points(int n_angles);
void launch_surface_jacobian(const SurfaceJacArgs* d_args, int n_layers, int n_angles, int n_terms, long long first,
                             long long count, double* partial, double* jac, hipStream_t s);
struct RaySurfaceJacArgs : RayJacArgs {
    const double* emissivity;           // n points, or nullptr: emissivity_all
    double emissivity_all;
};
void launch_ray_surface_jacobian(const RaySurfaceJacArgs* d_args, long long n, int n_rays, int n_bundles, int n_terms,
                                 hipStream_t s);

// Jacobians of the linear-in-optical-depth Planck source (K5j, lbl_column_transport.hip: lbl_column_jacobian_linear_dev,
// lbl_ray_jacobian_linear_dev): K5h's walks with K5i's step, d/d ln tau through g' and one temperature row per layer edge
// or segment end.  Values per band: [F_top, dF/dT_s, dF/de, L x d ln tau, 2 L x dT_edge (bottom, top per layer), n_terms x
// term]; a ray's rows: [dT_source, de, c x d ln tau, 2 per real segment in order of travel (dTa, dTb), its terms].  JacArgs'
// rT holds 1 / T of the bottom edges and T_spec is not used.
struct LinearJacArgs : SurfaceJacArgs {
    double pbkT_top[kMaxLayers];        // 100 h c / k / T at the top edge of layer l; ColumnRT's pbkT holds the bottom edge
    double rT_top[kMaxLayers];          // 1 / T at the top edge
    double* T_edge_spec;                // optional: 2 L x n spectral dF/dT_edge
};
void launch_linear_jacobian(const LinearJacArgs* d_args, int n_layers, int n_angles, int n_terms, long long first,
                            long long count, double* partial, double* jac, hipStream_t s);
struct LinearRayJacArgs : RaySurfaceJacArgs {
    long long off_seg_pbkT;             // 2 n_segments doubles: 100 h c / k / T where the light enters and leaves the segment
    long long off_seg_rT;               // 2 n_segments doubles: 1 / T likewise (a marker's pairs are 0 and never read)
    long long off_seg_Trow;             // n_segments x int32: the row of the segment's dTa relative to the ray's first row
};
void launch_linear_ray_jacobian(const LinearRayJacArgs* d_args, long long n, int n_rays, int n_bundles, hipStream_t s);

// Instrument channels (K8, lbl_instrument.hip: lbl_ils_convolve_dev): n_rows spectra on the base grid convolved with an
// instrument line shape onto n_channels channels.  One argument block per call: this header, then the arrays it names by
// their byte offset from the block's start (the block's device address is known only after it is uploaded).
constexpr int kMaxIlsRows = 512;
static_assert(kMaxRayPaths == kMaxIlsRows, "every ray of a call is a row of one convolve call");
constexpr int kMaxIlsChannels = 65536;
constexpr int kMaxIlsTable = 4096;
constexpr int kIlsRowBlock = 8;         // rows one workgroup carries in registers beside the normaliser
enum : int32_t { ILS_GAUSSIAN = 0, ILS_TRIANGLE = 1, ILS_BOXCAR = 2, ILS_SINC = 3, ILS_TABLE = 4, ILS_SHAPES = 5 };
struct IlsArgs {
    long long off_rows;                 // n_rows x const double*: the rows
    long long off_position, off_width;  // n_channels doubles each: centre in grid-index units, width in cm^-1
    long long off_first, off_count;     // n_channels x long long: the support [first, first + count)
    long long off_order;                // n_channels x int32: the channels by ascending `first` (the dispatch order)
    long long off_table;                // n_table doubles (ILS_TABLE)
    double* out;                        // n_rows x n_channels, row-major
    double step;                        // the grid step
    double table_half, table_rdx;       // ILS_TABLE: half extent in cm^-1 and (n_table - 1) / (2 table_half)
    long long n_channels;
    int32_t n_rows, n_table;
    int32_t chunk, pad;                 // channels dealt to one XCD: ceil(n_channels / 8)
};
void launch_ils_convolve(const IlsArgs* d_args, int shape, int n_rows, long long n_channels, hipStream_t s);

// k-distributions (K9, lbl_kdist.hip: lbl_rank_order_dev, lbl_ranked_means_dev): every (row, band) segment of n_rows rows
// on the base grid ranked by (key, index), then averaged over intervals of the rank.  One argument block per call.
constexpr int kMaxKdistRows = 512;
constexpr int kMaxKdistIntervals = 256;  // per band
constexpr int kMaxKdistBands = kMaxFluxBands;
constexpr int kKdistTile = 2048;         // pairs one workgroup sorts / merges in LDS (256 threads x 8), and ranks per partial sum
constexpr int kKdistMaxPasses = 20;      // merge passes of the longest band the 32-bit band-local index allows: 2048 << 20 = 2^31
struct RankArgs {
    long long off_rows;                 // n_rows x const double*: the rows (byte offset from the block's start, as IlsArgs)
    double* order; double* sorted;      // n_rows x s_total each (sorted may be nullptr)
    unsigned long long* keys[2];        // ping-pong of the merge passes: n_rows x s_total keys ...
    unsigned int* idx[2];               // ... and band-local indices (nullptr when no band is longer than a tile)
    long long s_total;
    long long first[kMaxKdistBands], count[kMaxKdistBands], s_start[kMaxKdistBands];
    int32_t passes[kMaxKdistBands];     // merge passes of the band: the smallest P with kKdistTile << P >= count
    // work items of one row per launch, as a prefix over the bands: launch 0 sorts tiles, launch p + 1 is merge pass p (over
    // the bands with passes > p, one item per kKdistTile outputs)
    int32_t item_start[kKdistMaxPasses + 1][kMaxKdistBands + 1];
    int32_t n_rows, n_bands;
};
struct MeansInterval {
    long long lo, len;                  // ranks [lo, lo + len) of a row's band-major order: lo = s_start[band] + e_i
    int32_t band, chunk_start;          // first partial sum of the interval (one per kKdistTile ranks)
};
struct MeansArgs {
    long long off_rows, off_orders;     // n_rows x const double* each: the rows, and the order every row is averaged by
    long long off_intervals;            // (g_total + 1) x MeansInterval, band after band; the last one closes chunk_start
    double* partial;                    // n_rows x n_chunks
    double* mean;                       // n_rows x g_total
    double* lower;                      // n_rows x (g_total + n_bands), or nullptr
    long long first[kMaxKdistBands], count[kMaxKdistBands], s_start[kMaxKdistBands];
    int32_t g_start[kMaxKdistBands + 1];   // first interval of every band
    int32_t n_rows, n_bands, g_total, n_chunks;
};
void launch_kdist_rank(const RankArgs* d_args, const RankArgs& host, hipStream_t s);
void launch_kdist_means(const MeansArgs* d_args, const MeansArgs& host, hipStream_t s);

// True Voigt line shape (K2v, lbl_voigt.hip: lbl_xsec_voigt_dev): one prepared line.  Its contribution to the work-grid point
// at integer offset d from its centre index is  amp * voigt_k(|d| * xs, y)  for |d| <= H = max(window - 2, 0), with
// voigt_k(x, y) = Re w(x + i y) of lbl_voigt_func.h.
struct __attribute__((aligned(32))) VoigtRec {
    double cf;      // centre index (pyradClasses.py:390) as a double, clamped as K1 clamps it
    double xs;      // resolution / ghw: one IEEE division
    double y;       // lhw / ghw
    double amp;     // A * (1 / (ghw * sqrt(pi)))
};
static_assert(sizeof(VoigtRec) == 32, "a lane stages one record with two 16-byte loads");
// One job of a Voigt batch, beside its PrepJob (same index): PrepJob carries the line fields, the job's physical constants
// and the regime counters' block; its hot / cold / cidx are not used.
struct VoigtJob {
    VoigtRec* rec;
    int32_t* cidx;         // centre indices, non-decreasing
    double* out;           // work grid, n_work doubles
    int32_t n_lines;
    int32_t H;             // wing support in points = max(window - 2, 0)
    int32_t p_begin;       // shard of the work grid computed by this job: [p_begin, p_end)
    int32_t p_end;
};
constexpr int kVoigtR = 2;                       // consecutive work-grid points a lane owns
constexpr int kVoigtChunk = 64;                  // records a wave parks in its LDS at a time (2 KB)
constexpr int kVoigtTile = 256 * kVoigtR;        // points of a workgroup
void launch_voigt_prep(const PrepJob* d_prep, const VoigtJob* d_jobs, int n_jobs, int max_lines, hipStream_t s);
void launch_voigt_accumulate(const VoigtJob* d_jobs, int n_jobs, long long max_points, hipStream_t s);
void launch_voigt_function(const double* x, const double* y, long long n, double* out, hipStream_t s);

// Temperature derivative of the Voigt cross section (K2v-T, lbl_voigt.hip: lbl_xsec_voigt_dt_dev): K2v's record and two
// logarithmic derivatives.  The line's contribution at integer offset d is
//     amp * (a * K + bx * GX + by * GY),  (K, GX, GY) = voigt_kgrad(|d| * xs, y),  bx = -1 / (2 T) of the job.
struct __attribute__((aligned(16))) VoigtDTRec {
    double cf, xs, y, amp;      // as VoigtRec
    double a;                   // d ln amp / dT
    double by;                  // d ln y / dT = -(n_air + 1/2) / T
};
static_assert(sizeof(VoigtDTRec) == 48, "a lane stages one record with three 16-byte loads");
struct VoigtDTJob {
    VoigtDTRec* rec;
    int32_t* cidx;
    double* out;           // work grid, n_work doubles
    double dlnw_dT;        // the caller's part of d ln amp / dT (what multiplies the intensities beside line_physics' factors)
    double bx;             // d ln x / dT = -1 / (2 T)
    int32_t n_lines, H, p_begin, p_end;     // as VoigtJob
};
void launch_voigt_dT_prep(const PrepJob* d_prep, const VoigtDTJob* d_jobs, int n_jobs, int max_lines, hipStream_t s);
void launch_voigt_dT_accumulate(const VoigtDTJob* d_jobs, int n_jobs, long long max_points, hipStream_t s);
void launch_voigt_gradient(const double* x, const double* y, long long n, double* K, double* GX, double* GY, hipStream_t s);

struct ColumnArgs {
    const double* trans[kMaxLayers];
    double layer_T[kMaxLayers];
    double r_layer_T[kMaxLayers];       // RN(1/layer_T[l]) (0: plain divide)
    double pbkT[kMaxLayers], pbk_surface;   // default arithmetic: 100 h c / k / T per layer and for the surface
    double r_surface_T;
    int32_t n_layers;
    double start, stop, step, pa, pb, surface_T;
    const double* I_in; double* I_out;
    long long n;
    long long first, count;
};

// ---- launchers (lbl_kernels.hip) ---------------------------------------------------------
void launch_line_prep(const PrepJob* d_jobs, int n_jobs, int max_lines, hipStream_t s);
void launch_line_quantities(const PrepJob* d_job, int n_lines, long long* index, double* lhw, double* ghw, double* intensity,
                            int32_t* regime, hipStream_t s);
void launch_accumulate(const AccumJob* d_jobs, int n_jobs, int max_tiles, int R, int LS, int variant,
                       const int2* worklist, int total_tiles, hipStream_t s, int budget = 0, int gauss_run = 16);
// narrow windows: every lane walks the lines that reach its own R points (skewed ranges); tiles of 256 R points
void launch_accumulate_skew(const AccumJob* d_jobs, int n_jobs, int max_tiles, int R, const int2* worklist, int total_tiles,
                            hipStream_t s, int LS = 1);      // LS 2 | 4: R = 8 only (waves of a workgroup share a span and deal its records)
void accumulate_far_field_params(int R, int* far_half_spans, double* far_cost, int budget = 0);
void launch_regrid(const double* work, long long n_work, double* out, long long n_base, double start, double stop,
                   hipStream_t s);
void launch_layer_sweep(const SweepArgs& a, hipStream_t s);
// kfold: every term is a whole layer with factor 1 (the fold over absorption coefficients): the kernel then skips the per-molecule sums
void launch_column_step(const ColumnStepArgs* d_args, long long first, long long count, hipStream_t s, int budget = 0, int kfold = 0);
void launch_column_sweep(const ColumnArgs* d_args, long long n, hipStream_t s, int budget = 0);
void launch_planck(double* out, long long n, double start, double stop, double T, double rT, double pa, double pb, hipStream_t s);
void launch_band_integral(const double* y, long long n, double* partial, double* result, hipStream_t s);
struct SumArgs { const double* in[kMaxIso]; int32_t n_in; double* out; long long n; };
void launch_sum(const SumArgs& a, hipStream_t s);
constexpr int kMaxRanks = 64;
struct CompactArgs { const double* gathered; double* out; long long slot; long long first[kMaxRanks]; long long count[kMaxRanks]; int32_t world; };
void launch_gather_compact(const CompactArgs& a, long long max_count, hipStream_t s);
void launch_optical(const double* trans, long long n, int kind, double* out, hipStream_t s);
void launch_line_survey(const double* nu, const double* sw, int n_lines, double range_min, double resolution,
                        double* out, long long n_base, hipStream_t s);

}  // namespace lbl
