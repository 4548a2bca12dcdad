// Hand-written CDNA4 (gfx950) kernels of the line-by-line absorption engine.
//
//   K1 line_prep_kernel        pyradClasses.py:252-263, 378-390; pyradLineshape.py:59-71;
//                              pyradIntensity.py:16-32
//   K2 xsec_accumulate_*       pyradLineshape.py:39, 52, 72-74 and the scatter loop
//                              pyradClasses.py:392-400, restated as an owner-computes gather
//   K2v voigt_prep_kernel, voigt_accumulate_kernel   the true Voigt profile Re w((x + i lhw) / ghw) / (ghw sqrt(pi)) over the
//                              same scatter geometry (lbl_xsec_voigt_dev; beyond the reference, see "K2v" below)
//   K2v-T voigt_dT_prep_kernel, voigt_dT_accumulate_kernel   its temperature derivative, term by term (lbl_xsec_voigt_dt_dev)
//   K3 regrid_kernel           np.interp of pyradClasses.py:401-405 (only when res != BASE)
//   K4 layer_sweep_kernel      pyradClasses.py:566-571, 583, 707-716, 784-787; pyradPlanck.py:38-44
//   K5 column_sweep_kernel     fold of pyradClasses.py:784-787 over layers
//   K5b column_step_kernel     K4's arithmetic per layer + that fold, straight from the cross sections
//   K6 band_integral kernels   pyradClasses.py:26-29
//   K5c column_flux_kernel     K5b's fold over absorption coefficients for several angles, upward and downward,
//                              reduced to level fluxes (Atmosphere.fluxes; beyond the reference)
//   K5d column_jacobian_kernel K5c's upward fold + a downward pass: analytic derivatives of the outgoing flux
//                              (Atmosphere.jacobians; beyond the reference)
//   K5e ray_radiance_kernel    K5c's step along ordered (layer, path length) segments: limb, slant and zenith rays
//                              (Atmosphere.radiance; beyond the reference)
//   K5f ray_jacobian_kernel    K5e's walk + K5d's downward pass along the segments: weighting functions of the radiance
//                              along a ray (Atmosphere.pathJacobians; beyond the reference)
//   K5g surface_flux_kernel, ray_surface_kernel   K5c and K5e over a reflecting surface: emissivity, Lambertian or specular
//                              reflection, rays that bounce (fluxes() and radiance() with an emissivity; beyond the reference)
//   K5h surface_jacobian_kernel, ray_surface_jacobian_kernel   K5d and K5f over that surface: the reflected leg's derivatives
//                              and d/d emissivity (jacobians(), pathJacobians(), observe() with an emissivity; beyond the reference)
//   K5i linear_flux_kernel, linear_ray_kernel   K5g's two kernels with a Planck source linear in optical depth between two
//                              temperatures per layer or segment (fluxes() and radiance() with planck="linear"; beyond the reference)
//   K5j linear_jacobian_kernel, ray_linear_jacobian_kernel   K5h's two kernels with K5i's step: d ln tau through g', one
//                              temperature row per layer edge or segment end (jacobiansLinear(), pathJacobiansLinear(),
//                              observeLinear(); beyond the reference)
//   K5k solar_beam_kernel, solar_diffuse_kernel   K5c's walks without emission: collimated beams attenuated along their slant
//                              paths, reflected by the surface (Atmosphere.solarFluxes; beyond the reference)
//   K5l twostream_down_kernel, twostream_up_kernel   the beams through scattering layers: a delta-two-stream solution per
//                              layer, joined by adding through a workspace (Atmosphere.solarFluxesTwoStream; beyond the reference)
//   K5m scatter_flux_down_kernel, scatter_flux_up_kernel   K5l with the layers' thermal emission as the source and an emitting
//                              surface (Atmosphere.fluxesTwoStream; beyond the reference)
//   K5n scatter_radiance_up_kernel   K5m's column seen along up to 16 views: the two-stream source function integrated in
//                              closed form per layer and view (Atmosphere.radianceTwoStream; beyond the reference)
//   K5o beam_view_kernel      K5l's column with one sun seen along up to 16 views: K5n's integrals with the beam's single
//                              scattering in the source function (Atmosphere.solarRadianceTwoStream; beyond the reference)
//   K5p scatter_jacobian_down_kernel, scatter_jacobian_up_kernel   the derivatives of K5m's upward flux at the top: its
//                              downward walk with one more number per level, then one adjoint walk that recomputes and
//                              differentiates every layer (Atmosphere.jacobiansTwoStream; beyond the reference)
//   K7 line_survey_kernel     pyradClasses.py:409-428
//
// Design notes (DESIGN.md has the long form).  The reference snaps every line centre to a
// grid index and samples the half-profile at integer multiples of the resolution, so the
// contribution of line l to grid point j depends only on |j - c_l|.  That makes the gather
// form exact: every lane owns R consecutive grid points in registers, a wavefront walks the
// (sorted) lines whose support reaches its 64*R points, and each grid point is written once
// with a plain coalesced store.  No atomics, and a fixed summation order per grid point, so two
// runs are bit-identical.
//
// K2 variants (lbl_set_option "accum_variant"; 1, 2 and 4 - the scalar-cache running fraction / recurrence kernels and the
// balanced single-round partition - were measured, superseded and removed: docs/history/):
//   0    xsec_accumulate_kernel      the literal form: IEEE divide + exp per pair, records through the scalar cache (on-device cross-check)
//   3    xsec_accumulate_lds_kernel  records streamed through wave-private LDS, every pair direct
//   5    xsec_accumulate_lds_kernel<.., FF = true>  (default) 3 + far-field series for distant
//        Lorentz lines; optionally the layer sweep of a single-line-list layer in the output stage;
//        round 3: its edge lines (support ends inside the span) take the skewed walk (skew_edges), and
//        line lists whose window is too narrow for any far line (< 640 points: the upper layers of a
//        column) run xsec_accumulate_skew_kernel, in which every LANE walks the lines that reach its
//        own points (lbl_set_option "accum_skew")
//
// Round 5: an accumulate job may hold ALL line lists of a layer (merged layer job: lbl_layer_merged_step_dev,
// lbl_layers_merged_accumulate_dev).  K1 (line_prep_merged_kernel) then writes the lists' records into one array in
// centre-index order with every amplitude times its molecule's conc P / 1E4 / k / T over a power of two, and the same K2
// kernels accumulate the layer's absorption coefficient sum_m f_m sum_iso xs_iso (pyradClasses.py:707-712, 581-583, 566-571)
// directly - the "shared wavenumber-grid absorption-coefficient array" - with the sweep in the output stage (output_point).
//
// K2 is fp64-VALU bound, not HBM bound: its compulsory traffic is 56 B per line and 8 B per grid
// point against 5 fp64 instructions per directly evaluated (line, grid point) pair.
#include "lbl_device.h"
#include "lbl_launch_shapes.h"
#include "lbl_linear_source.h"
#include "lbl_voigt_func.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace lbl {

// Timing-only ablations (parts of a kernel switched off: WRONG results) exist in diagnostic builds only
// (make EXTRA=-DLBL_DIAG, scripts/make_diag_lib.sh); the production library carries none of them.
#ifdef LBL_DIAG
#define LBL_ABLATE(obj, bit) (((obj).ablate & (bit)) != 0)
#else
#define LBL_ABLATE(obj, bit) false
#endif

// ----------------------------------------------------------------------------------------
// small helpers
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ int uniform_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Prepared line records are written by K1 and only read by K2.  The scalar-cache variants
// view them through the constant address space (invariant memory -> s_load with a uniform
// index); the LDS variant streams them with coalesced vector loads.
typedef const double __attribute__((address_space(4)))* ConstF64;
typedef const int32_t __attribute__((address_space(4)))* ConstI32;

// working copy of one line (hot + cold halves) in registers
struct Rec {
    double cf, a2, KL, KG, b, q2;
    int32_t ci, dgi, flags;
};

__device__ __forceinline__ Rec load_rec_scalar(const HotRec* hot, const ColdRec* cold, int i, bool want_cold) {
    ConstF64 h = (ConstF64)(unsigned long long)hot + (long long)i * 4;
    ConstI32 hi = (ConstI32)(h + 3);
    Rec r;
    r.cf = h[0]; r.a2 = h[1]; r.KL = h[2]; r.dgi = hi[0]; r.flags = hi[1];
    r.ci = (int32_t)r.cf;
    r.KG = 0.0; r.b = 0.0; r.q2 = -1.0;
    if (want_cold) {
        ConstF64 c = (ConstF64)(unsigned long long)cold + (long long)i * 4;
        r.KG = c[0]; r.b = c[1]; r.q2 = c[2];
    }
    return r;
}

// xAxis element j of np.linspace(start, stop, n, endpoint=True) (pyradClasses.py:702-705):
// NumPy computes arange(n) * step + start with a separate multiply and add and then
// overwrites the last element with `stop`, so contraction to an FMA is switched off here.
__device__ __forceinline__ double linspace_at(long long j, long long n, double start, double stop, double step) {
#pragma clang fp contract(off)
    if (n > 1 && j == n - 1) return stop;
    double y = (double)j * step;
    return y + start;
}

// pyradPlanck.planckWavenumber (pyradPlanck.py:38-44): a / (exp(b) - 1),
// a = 2E8*h*c**2 * n**3, b = 100*h*c*n/k/T.  pa = 2E8*h*c**2 and pb = 100*h*c come from the
// host in the reference's association order.
// x / c for a launch-uniform divisor, bit for bit the IEEE quotient the reference's NumPy expression
// produces, in 5 instructions instead of the ~14 of the general divide (the sweeps are ALU bound on
// these: 15 fp64 divisions per grid point).  rc = RN(1/c) from the host.  q0 = RN(x rc) is within
// (1 + 2^-52) ulp of x/c; r = x - q c is formed by one fma; q1 = RN(q0 + r rc) is a faithful
// quotient; by Markstein's theorem one more correction with an exact residual gives RN(x/c) for every
// x whenever rc is the correctly rounded reciprocal of a c whose significand is not all ones.  The host
// passes rc = 0 for such a c (or a subnormal / non-finite one) and the plain divide is taken instead.
// Range: the proof needs the residual x - q c to be exact, i.e. not to fall below the subnormal grid:
// |x| >= 2^-969 (about 1e-292) for the divisors used here; below that the quotient can be off by one ulp
// of a number that is itself below 1e-270, and x = +-inf gives NaN (inf - inf) where IEEE gives +-inf.
// Cross sections times volume fractions times pressures are many orders of magnitude inside the range
// (the smallest non-zero cross section a line list produces here is ~1e-200: Gaussian tails underflow to
// exact zeros first, and 0 is handled exactly); a guard per call would cost the sweeps 6 % of their
// instructions.  tests/test_gpu_abi.py::test_sweep_divisions_are_ieee_exact covers 1e-270 .. 1e+250 and 0.
__device__ __forceinline__ double div_uniform(double x, double c, double rc) {
    if (rc == 0.0) return x / c;
    double q = x * rc;
    double r = fma(-q, c, x);
    q = fma(r, rc, q);
    r = fma(-q, c, x);
    return fma(r, rc, q);
}
constexpr double kRcp1E4 = 1.0 / 1E4;      // correctly rounded by the compiler; neither significand is all ones
constexpr double kRcpKB = 1.0 / kB;

// exp(x) for x <= 700 without the range tests of the library routine (22 -> 17 instructions); exact
// to the library's accuracy for x >= -745, 0 (through v_ldexp_f64) below, finite garbage-free
// down to about -1e18, so callers clamp only when their argument can be more extreme:
// n = rint(x log2 e), r = x - n ln2 (two-part), degree-11 polynomial on |r| <= ln2/2 (the
// coefficients of the ROCm device library's double-precision exp), scaled by 2^n with v_ldexp_f64,
// which also delivers the gradual underflow.  Callers clamp the argument.
__device__ __forceinline__ double exp_clamped(double x) {
    const double n = __builtin_rint(x * 0x1.71547652b82fep+0);
    double r = fma(n, -0x1.62e42fefa39efp-1, x);
    r = fma(n, -0x1.abc9e3b39803fp-56, r);
    double p = fma(0x1.ade156a5dcb37p-26, r, 0x1.28af3fca7ab0cp-22);
    p = fma(p, r, 0x1.71dee623fde64p-19);
    p = fma(p, r, 0x1.a01997c89e6b0p-16);
    p = fma(p, r, 0x1.a01a014761f6ep-13);
    p = fma(p, r, 0x1.6c16c1852b7b0p-10);
    p = fma(p, r, 0x1.1111111122322p-7);
    p = fma(p, r, 0x1.55555555502a1p-5);
    p = fma(p, r, 0x1.5555555555511p-3);
    p = fma(p, r, 0x1.000000000000bp-1);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

// the part that depends on the grid point only (a, and pb * n / kB): hoisted out of loops over temperatures
__device__ __forceinline__ void planck_point(double n, double pa, double pb, double& a, double& bn) {
    a = pa * (n * n * n);
    bn = div_uniform(pb * n, kB, kRcpKB);
}
__device__ __forceinline__ double planck_at(double a, double bn, double T, double rT) {
    const double b = div_uniform(bn, T, rT);                              // pb * n / kB / T
    return a / (exp(b) - 1.0);
}
__device__ __forceinline__ double planck_wn(double n, double T, double rT, double pa, double pb) {
    double a, bn;
    planck_point(n, pa, pb, a, bn);
    return planck_at(a, bn, T, rT);
}

// xs * conc * P / 1E4 / kB / T (pyradClasses.py:583), left to right like the reference
__device__ __forceinline__ double abs_coef_term(double xs, double conc, double P, double T, double rT) {
#pragma clang fp contract(off)
    return div_uniform(div_uniform(div_uniform(xs * conc * P, 1E4, kRcp1E4), kB, kRcpKB), T, rT);
}

// ---- the sweeps' default arithmetic (lbl_set_option "sweep_ieee_divisions" 0; flag `budget` in the argument blocks) ----
// The reference's NumPy expressions round nine times per point and layer where it does not matter: crossSection *
// concentration * P / 1E4 / k / T is three correctly rounded divisions (51 of the column step's 161 instructions with
// div_uniform), and the Planck function two more plus the library exp.  The cross section entering them already differs
// from NumPy's in its last bits (K2 is 1e-14, not bit-exact), so the chain buys nothing a comparison with the reference can
// see.  By default the molecule's factor conc * P / 1E4 / k / T comes from the host (evaluated there in the reference's
// order) and meets the cross section in ONE multiplication; the Planck exponent is n * (100 h c / k / T) with the bracket
// from the host; reciprocals by v_rcp_f64 + two Newton steps; exp without the library's range tests.  Each result is within
// a few 1e-16 of the chain's (tests/test_gpu_abi.py::test_sweep_divisions_are_ieee_exact checks both).  "sweep_ieee_divisions"
// 1 selects the chain: k is then bit-identical to NumPy's expression applied to the same cross section.
__device__ __forceinline__ double rcp_newton(double x) {           // x finite, positive, normal
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    return fma(fma(-x, r, 1.0), r, r);
}
// (a NaN exponent must stay a NaN, as in np.exp(nan): fmin / fmax drop it, so it is put back explicitly - advisor, round 4)
__device__ __forceinline__ double planck_budget(double n, double pa, double pbkT) {
    const double b = n * pbkT;
    const double e = exp_clamped(fmin(b, 700.0)) - 1.0;
    const double v = (pa * (n * n * n)) * rcp_newton(fmax(e, 1e-300));
    const double r = (b > 700.0 || !(e > 0.0)) ? ((b > 700.0) ? 0.0 : (pa * (n * n * n)) / e) : v;     // (n = 0: 0/0 like the reference)
    return b != b ? b : r;
}
__device__ __forceinline__ double exp_neg_budget(double x) {       // exp(-x), x >= 0 (optical depth)
    // (the clamp as a select, not as fmax, which would drop a NaN: a NaN argument then runs through exp_clamped as a NaN -
    // rint, fma, ldexp all pass it on - and needs no test of its own; x = +inf gives 0 like the reference's exp(-inf))
    return exp_clamped(x > 800.0 ? -800.0 : -x);
}

// ----------------------------------------------------------------------------------------
// K1: per-line preparation
// ----------------------------------------------------------------------------------------
// What the reference computes per line before it touches the grid (pyradClasses.py:252-263, 378, 388-390;
// pyradIntensity.py:16-32): shared by K1 and by the kernel behind lbl_line_quantities, which only reports them.
struct LinePhysics {
    double broadened, lhw, ghw, ratio, A, fidx;
};
__device__ __forceinline__ LinePhysics line_physics(const PrepJob& J, int i) {
    LinePhysics L;
    const double nu = J.nu[i];
    const double q = J.q_frac;
    const double Pp0 = J.P_over_p0;                                   // P / p0, evaluated on the host
    // Line.broadenedLine (pyradClasses.py:252-254)
    L.broadened = nu + J.delta_air[i] * J.P / p0;
    // Line.lorentzHW (pyradClasses.py:256-259)
    // (t0/T)**n evaluated as exp(n ln(t0/T)) with the logarithm hoisted to the host (one per job)
    L.lhw = ((1.0 - q) * J.gamma_air[i] + q * J.gamma_self[i]) * Pp0 * exp(J.n_air[i] * J.log_t0_over_T);
    // Isotope.molMass (pyradClasses.py:294-296), Line.gaussianHW (pyradClasses.py:261-263): the
    // square root depends on the job only (host)
    L.ghw = L.broadened * J.ghw_factor;
    L.ratio = L.lhw / L.ghw;                                          // pyradClasses.py:378
    // pyradIntensity.intensityFactor (pyradIntensity.py:16-32) at the SHIFTED wavenumber
    // (pyradClasses.py:388).  Divisions by the per-job T and t0 are multiplications by their
    // reciprocals: at most one ulp in an exponent of order 1-50.
    const double c2 = cLight * hPlanck * 100.0 / kB;                  // pyradIntensity.py:13
    const double E = J.elower[i];
    const double stim = (1.0 - exp(-c2 * L.broadened * J.inv_T)) / (1.0 - exp(-c2 * L.broadened * (1.0 / t0)));
    // exp(-c2 E/T) / exp(-c2 E/t0) as one exponential of the difference (exactly 1 at T = t0,
    // like the quotient; elsewhere within |c2 E (1/T - 1/t0)| ulps of it, < 1e-14 relative)
    const double boltz = exp(c2 * E * (1.0 / t0) - c2 * E * J.inv_T);
    L.A = J.sw[i] * J.q_ratio * stim * boltz;
    // centre index from the UNSHIFTED wavenumber, truncation toward zero (pyradClasses.py:390)
    L.fidx = (nu - J.range_min) / J.resolution;
    return L;
}
__device__ __forceinline__ int line_regime(double ratio) {          // pyradClasses.py:379-387
    return ratio < .01 ? 0 : (ratio > 100.0 ? 1 : 2);
}

// One line's records (hot, cold), centre index and regime from its list's job constants: shared by the per-list K1 and
// the merged-order K1 below.
__device__ __forceinline__ void prep_one_line(const PrepJob& J, int i, HotRec& r, ColdRec& rc, long long& idx, int& regime) {
    const LinePhysics L = line_physics(J, i);
    // (merged layer job: the molecule's conc P / 1E4 / k / T over a power of two rides on the intensity; 1.0 otherwise: exact)
    const double lhw = L.lhw, ghw = L.ghw, ratio = L.ratio, A = L.A * J.weight;
    idx = (long long)L.fidx;
    if (idx > 2000000000LL) idx = 2000000000LL;
    if (idx < -2000000000LL) idx = -2000000000LL;

    double hw, KL, KG;
    if (ratio < .01) {                // Gaussian only (pyradClasses.py:379-381)
        regime = 0;
        hw = ghw;
        KL = 0.0;
        KG = A / hw * kInvSqrtPi;                                     // pyradLineshape.py:39 (/ sqrt(pi) as a product)
    } else if (ratio > 100.0) {       // Lorentz only (pyradClasses.py:382-384)
        regime = 1;
        hw = lhw;
        KL = A * (hw * kInvPi);                                       // pyradLineshape.py:52 (/ pi as a product)
        KG = 0.0;
    } else {                          // pseudo-Voigt (pyradClasses.py:385-387, pyradLineshape.py:58-76)
        regime = 2;
        const double g = 2.0 * ghw, l = 2.0 * lhw;
        const double g2 = g * g, l2 = l * l;
        const double f5 = g2 * g2 * g + 2.69269 * g2 * g2 * l + 2.42843 * g2 * g * l2 +
                          4.47163 * g2 * l2 * l + .07842 * g * l2 * l2 + l2 * l2 * l;
        const double f = exp(.2 * log(f5));                                 // f5 ** .2
        const double x = l / f;
        const double eta = 1.36603 * x - .47719 * x * x + .11116 * x * x * x;
        hw = f / 2.0;
        KL = eta * (A * (hw * kInvPi));
        KG = (1.0 - eta) * (A / hw * kInvSqrtPi);
    }
    const double a = hw * J.inv_res;
    r.cf = (double)idx;
    r.a2 = a * a;
    r.KL = KL * J.inv_res2;
    rc.KG = KG;
    rc.b = 1.0 / r.a2;
    r.flags = 0;
    // running-fraction accumulation multiplies up to 32 denominators d*d + a2 with
    // |d| <= H + 512 <= 4e4 (else 16, see AccumJob.flush_every): keep a2 in [1e-9, 1e8] so
    // the product stays within 1e-288 .. 1e296; anything else takes the plain-divide path
    if (!(r.a2 > 1e-9 && r.a2 < 1e8)) r.flags |= REC_DIRECT_DIV;
    // Gaussian term: where can it still change the fp64 value of the line's sum?
    double dg = 0.0;
    if (KG != 0.0) {
        const double u2_under = 745.2;           // exp(-745.2) == 0 in fp64
        double u2 = u2_under;
        if (KL != 0.0) {
            // ratio Gauss/Lorentz at offset u = d/a:  C (1+u^2) exp(-u^2);  solve = 2^-54 (budget mode: 2^-34) for u^2 = v + 1,
            // v = ln C + ln(1 + v).  The cut-off only has to err on the far side, so single precision
            // with a margin does: ln C from the exponent and a hardware log2 of the mantissa, three
            // fixed-point steps (each contracts by 1/(1+v)), +0.01 for the float roundings and the
            // remaining contraction (4 double-precision logs were a fifth of this kernel's instructions).
            const double C = fabs(KG / (r.KL * rc.b)) * J.gauss_cut;        // 2^54 (exact mode) or 2^34 (budget mode)
            if (C <= 1.0) {
                u2 = 0.0;
            } else {
                int ex;
                const float mant = (float)frexp(C, &ex);                               // C = mant 2^ex, mant in [0.5, 1)
                const float lnC = ((float)ex + __log2f(mant)) * 0.69314718f;
                float v = lnC;
                for (int it = 0; it < 3; ++it) v = lnC + __log2f(1.0f + v) * 0.69314718f;
                u2 = fmin((double)(v * 1.00001f + 1.01f), u2_under);
            }
        }
        dg = (u2 > 0.0) ? (double)(__fsqrt_rn((float)u2) * 1.000001f) * a + 2.0 : 0.0;
    }
    r.dgi = (dg < 2.0e9) ? (int32_t)dg : 2000000000;
#ifdef LBL_DIAG
    if (J.pad & 1024) r.dgi = 0;               // (timing only, debug_ablate 1024: no Gaussian part anywhere)
#endif
    // Gaussian recurrence along a lane's consecutive points: only for b <= 4 (see gauss_term);
    // narrower profiles take one exp per point
    rc.q2 = (rc.b <= 4.0) ? exp(-2.0 * rc.b) : -1.0;
    if (!(rc.b <= 4.0)) r.flags |= REC_NO_RECUR;
    // 16-point runs (gauss_runs): a lane walks 15 steps from its first point, possibly TOWARDS the centre.
    // If its seed KG exp(-b d0^2) has underflowed (b d0^2 > T, T = 745 - ln(1/KG) >= ~600 for any KG down
    // to 1e-60) the run's values stay 0; that is harmless as long as no point of the run can matter: the
    // nearest one has b d^2 > b (sqrt(T/b) - 15)^2, which exceeds the 45 beyond which the term is below
    // 2^-54 of the line's Lorentz part whenever sqrt(b) < (sqrt(600) - sqrt(45)) / 15 = 1.19.  b <= 1
    // (profiles at least one grid point wide) keeps a margin.  (Seeds that are tiny but normal keep the
    // recurrence exact; a clamped r only lowers a value that is negligible anyway.)  Pure-Gaussian lines
    // (no Lorentz part to be negligible against: their term counts until it underflows) keep the 4-point pass.
    if (rc.b <= 1.0 && KL != 0.0) r.flags |= REC_LONG_RUN;
    // 32-point runs (round 6, the three-waves-per-SIMD build of the far-field kernel): 31 steps towards the centre need
    // sqrt(b) < (sqrt(600) - sqrt(45)) / 31 = 0.57; b <= 0.3 keeps the same margin
    if (rc.b <= 0.3 && KL != 0.0) r.flags |= REC_LONG_RUN32;
    rc.KLd = r.KL;
}

__device__ __forceinline__ int wave_max_i32(int v);

// The largest Gaussian cut-off dgi of a block of 256 prepared positions, for the far loop of the accumulate kernel: a far
// chunk farther from its span than the largest cut-off of the span's blocks cannot hold a record whose Gaussian part
// reaches the span, and skips the per-record test (far_field_lines).  A wave maximum, the block's LDS and one plain store
// per block, like the regime counters; called by every thread of the block between two barriers of its caller's.
__device__ __forceinline__ void block_reach_stage(int dgi, int* s_reach) {
    const int m = wave_max_i32(dgi);
    if ((threadIdx.x & 63) == 0) s_reach[threadIdx.x >> 6] = m;
}
__device__ __forceinline__ int block_reach_value(const int* s_reach) {
    return max(max(s_reach[0], s_reach[1]), max(s_reach[2], s_reach[3]));
}

__global__ __launch_bounds__(256) void line_prep_kernel(const PrepJob* __restrict__ jobs) {
    const PrepJob& J = jobs[blockIdx.y];
    if (J.merged) return;                       // (its job's merged-order launch prepares this list)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int regime = -1, dgi = 0;
    if (i < J.n_lines) {
        HotRec r;
        ColdRec rc;
        long long idx;
        prep_one_line(J, i, r, rc, idx, regime);
        J.hot[i] = r;
        J.cold[i] = rc;
        J.cidx[i] = (int32_t)idx;
        dgi = r.dgi;
    }
    __shared__ int s_reach[4];
    block_reach_stage(dgi, s_reach);
    // regime counters (pyradClasses.py:368-370, 406).  One plain store per block: thousands of
    // atomics on one cache line cost ~12 ns each and made this kernel 3x longer than its arithmetic.
    __shared__ unsigned int s_cnt[4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < 3; ++k) {
        const unsigned long long m = __ballot(regime == k);
        if (lane == 0) s_cnt[wave][k] = (unsigned int)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < 3)
        J.block_counts[blockIdx.x * 3 + threadIdx.x] =
            s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
    if (threadIdx.x == 64 && J.block_reach) J.block_reach[blockIdx.x] = block_reach_value(s_reach);
}

// K1 of a merged layer job, in MERGED order: thread t prepares the line that belongs at position t of the layer's record
// array (src[t] = list within the job << 26 | line within the list, built once per window by merge_rank_kernel), so the
// records are written with coalesced stores; the seven HITRAN fields are gathered from the job's lists, each of which
// is walked in increasing order.  (The first version had every list scatter its records through the inverse map: the
// interleaved 32-byte stores of 90 lists made K1 of the 30-layer column twice as long, 0.39 against 0.20 ms.)
__global__ __launch_bounds__(256) void line_prep_merged_kernel(const PrepJob* __restrict__ lists, const MergedPrep* __restrict__ jobs) {
    const MergedPrep& M = jobs[blockIdx.y];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if ((int)blockIdx.x >= M.blocks) return;
    // the job's per-list constants and field pointers, staged in LDS: every lane picks its own list's block (neighbouring
    // merged positions belong to different lists), which as global loads were ~25 divergent fetches per line
    __shared__ PrepJob s_lists[kMaxIso];            // (a merged job holds at most kMaxIso lists: enqueue_accumulate)
    {
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(lists + M.first_list);
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(s_lists);
        const int words = M.n_lists * (int)(sizeof(PrepJob) / 8);
        for (int w = threadIdx.x; w < words; w += blockDim.x) dst[w] = src[w];
        __syncthreads();
    }
    int regime = -1, list = -1, dgi = 0;
    if (t < M.n_total) {
        const int s = M.src[t];
        list = (int)((unsigned int)s >> 26);
        const PrepJob& J = s_lists[list];
        HotRec r;
        ColdRec rc;
        long long idx;
        prep_one_line(J, s & ((1 << 26) - 1), r, rc, idx, regime);
        M.hot[t] = r;
        M.cold[t] = rc;
        M.cidx[t] = (int32_t)idx;
        dgi = r.dgi;
    }
    // the largest Gaussian cut-off of the block's 256 merged positions
    __shared__ int s_reach[4];
    block_reach_stage(dgi, s_reach);
    // regime counters per list and block of 256 merged positions
    __shared__ unsigned int s_cnt[4][kMaxIso][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int l = 0; l < M.n_lists; ++l)
        for (int k = 0; k < 3; ++k) {
            const unsigned long long m = __ballot(list == l && regime == k);
            if (lane == 0) s_cnt[wave][l][k] = (unsigned int)__popcll(m);
        }
    __syncthreads();
    for (int q = threadIdx.x; q < M.n_lists * 3; q += blockDim.x) {
        const int l = q / 3, k = q % 3;
        lists[M.first_list + l].block_counts[blockIdx.x * 3 + k] = s_cnt[0][l][k] + s_cnt[1][l][k] + s_cnt[2][l][k] + s_cnt[3][l][k];
    }
    if (threadIdx.x == 64 && M.block_reach) M.block_reach[blockIdx.x] = block_reach_value(s_reach);
}

// lbl_line_quantities: the per-line numbers of the reference (Line.lorentzHW / gaussianHW, the corrected intensity,
// the regime) from the same expressions K1 evaluates, and the centre index K1 itself wrote (the one K2 works
// from; K1 clamps it to +-2e9).  Never part of a step.
__global__ __launch_bounds__(256) void line_quantities_kernel(const PrepJob* __restrict__ jobs, long long* __restrict__ index,
                                                              double* __restrict__ lhw, double* __restrict__ ghw,
                                                              double* __restrict__ intensity, int32_t* __restrict__ regime) {
    const PrepJob& J = jobs[0];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= J.n_lines) return;
    const LinePhysics L = line_physics(J, i);
    index[i] = (long long)J.cidx[i];
    lhw[i] = L.lhw; ghw[i] = L.ghw; intensity[i] = L.A;
    regime[i] = line_regime(L.ratio);
}

// Merged layer jobs: which line of which list belongs at every position of the layer's one record array (centre-index
// order, ties by list).  Built once per (line lists, grid) beside the dispatch schedule and kept with it; K1 then runs in
// merged order (line_prep_merged_kernel) in every step.  centre_index_kernel evaluates K1's own expression (line_physics / line_prep_kernel:
// (nu - range_min) / resolution, truncated, clamped), so the order is the order of the very indices K1 will write.
__global__ __launch_bounds__(256) void centre_index_kernel(const MergeList* __restrict__ lists) {
    const MergeList& M = lists[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M.n_lines) return;
    long long idx = (long long)((M.nu[i] - M.range_min) / M.resolution);
    if (idx > 2000000000LL) idx = 2000000000LL;
    if (idx < -2000000000LL) idx = -2000000000LL;
    M.tmp_cidx[i] = (int32_t)idx;
}

__global__ __launch_bounds__(256) void merge_rank_kernel(const MergeList* __restrict__ lists) {
    const MergeList& M = lists[blockIdx.y];
    const int i0 = blockIdx.x * blockDim.x;
    if (i0 >= M.n_lines) return;                                  // (whole workgroup)
    const int i = i0 + threadIdx.x;
    const int me = (int)blockIdx.y;
    // lists ahead of this one win ties (count their lines with c_b <= c), lists behind lose them (c_b < c).
    // Round 6: the workgroup's 256 lines are consecutive in a sorted list, so their places in another list lie between the
    // places of its first and of its last line.  Those two are found by two THREADS per other list, side by side (one search
    // deep, not two); the window between them - a few hundred entries - is staged in LDS with coalesced loads and searched
    // there.  Before: 34 scattered loads per line and other list, 400 M for a column, at the rate the L2 serves them (0.26 ms).
    constexpr int WIN = 2048;
    __shared__ int s_lo[kMaxIso], s_hi[kMaxIso];
    __shared__ int32_t s_win[WIN];
    auto search = [&](const int32_t* __restrict__ a, long long target, int lo, int hi) {
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((long long)a[mid] < target) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    {
        const int u = (int)threadIdx.x & 63, which = (int)threadIdx.x >> 6;          // which 0: the first line's place, 1: the last line's
        const int b = M.job_first + u;
        if (which < 2 && u < M.job_count && b != me) {
            const MergeList& O = lists[b];
            const int i1 = min(i0 + (int)blockDim.x, M.n_lines) - 1;
            const long long tie = b < me ? 1 : 0;
            const int r = search(O.tmp_cidx, (long long)M.tmp_cidx[which ? i1 : i0] + tie, 0, O.n_lines);
            if (which) s_hi[u] = r; else s_lo[u] = r;
        }
    }
    __syncthreads();
    const bool mine = i < M.n_lines;
    const long long c = mine ? (long long)M.tmp_cidx[i] : 0;
    int pos = i;
    for (int b = M.job_first; b < M.job_first + M.job_count; ++b) {
        if (b == me) continue;
        const MergeList& O = lists[b];
        const int lo = s_lo[b - M.job_first], hi = s_hi[b - M.job_first];          // (uniform over the workgroup)
        const long long target = b < me ? c + 1 : c;
        if (hi - lo <= WIN) {
            __syncthreads();
            for (int k = threadIdx.x; k < hi - lo; k += blockDim.x) s_win[k] = O.tmp_cidx[lo + k];
            __syncthreads();
            if (mine) pos += lo + search(s_win, target, 0, hi - lo);
        } else if (mine) {
            pos += search(O.tmp_cidx, target, lo, hi);
        }
    }
    if (mine) M.src_of_job[pos] = (int32_t)(((unsigned int)(me - M.job_first) << 26) | (unsigned int)i);
}

void launch_merge_ranks(const MergeList* d_lists, int n_lists, int max_lines, hipStream_t s) {
    if (n_lists <= 0 || max_lines <= 0) return;
    dim3 grid((max_lines + 255) / 256, n_lists);
    hipLaunchKernelGGL(centre_index_kernel, grid, dim3(256), 0, s, d_lists);
    hipLaunchKernelGGL(merge_rank_kernel, grid, dim3(256), 0, s, d_lists);
}

// ----------------------------------------------------------------------------------------
// K2: owner-computes accumulation
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ int lower_bound_i32(const int32_t* __restrict__ a, int n, long long target) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)a[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Gaussian part of one line for a lane's R consecutive points (d0 = offset of the lane's
// first point from the line centre), masked to the line's support |d| <= H.
//   GM == 0: one exp per point.
//   GM == 1: two exps per lane, then g(d+1) = g(d) r(d), r(d+1) = r(d) q2 with
//            r(d) = exp(-b (2d+1)), q2 = exp(-2b): 2 multiplies per further point.
// The recurrence keeps full relative precision while g(d0) is a normal number.  Walking
// TOWARDS the centre the terms grow by at most exp(b (R-1) (2|d0| - R + 1)); K1 enables the
// recurrence only for b <= 4 (q2 >= 0), for which a lane whose first point has underflowed
// (b d0^2 > 708) cannot reach a point where the term still matters (b d^2 < ~45) within R <= 8
// steps: there  b (d0^2 - d^2) <= 14 sqrt(45 b) + 49 b < 400.  The exponent of r is clamped so
// that a far lane computes 0 * finite = 0, never 0 * inf.
template <int R, int GM, bool MASKED = true>
__device__ __forceinline__ void gauss_term(double KG, double b, bool recur, double d0, double Hf, double q2,
                                           double (&acc)[R]) {
    if (GM == 0 || !recur || R < 4) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const double d = d0 + (double)k;
            const double t = KG * exp_clamped(fmax(-b * (d * d), -800.0));
            acc[k] += (!MASKED || fabs(d) <= Hf) ? t : 0.0;
        }
    } else {
        // b <= 4 and |d0| < 2^31 here: the arguments stay far inside the range where the reduction of
        // exp_clamped is finite (a hopeless argument only has to underflow to 0); only the growth of r
        // towards the centre needs its cap
        double g = KG * exp_clamped(-b * (d0 * d0));
        double rr = exp_clamped(fmin(-b * (2.0 * d0 + 1.0), 700.0));
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (MASKED) {
                const double d = d0 + (double)k;
                acc[k] += (fabs(d) <= Hf) ? g : 0.0;
            } else {
                acc[k] += g;
            }
            g *= rr;
            rr *= q2;
        }
    }
}

// Per-wave accumulator state.  acc: finished sums.  N/D: running fraction of the Lorentz
// terms of the last `cnt` (< 16) lines:  sum_i K_i/den_i = N/D with
//     N <- N*den + K*D,   D <- D*den        (3 fp64 ops + 2 for den instead of a divide)
// flushed into acc with one IEEE divide per point every `every` lines (32; 16 when the
// window is wider than 4e4 points).  K1 routes lines with a2 outside [1e-9, 1e8] to the
// plain-divide path, so the product of denominators stays within 1e-288 .. 1e296.
template <int R>
struct WaveAcc {
    double acc[R], N[R], D[R];
    int cnt, every;
    __device__ __forceinline__ void init(int flush_every) {
#pragma unroll
        for (int k = 0; k < R; ++k) { acc[k] = 0.0; N[k] = 0.0; D[k] = 1.0; }
        cnt = 0;
        every = flush_every;
    }
    // N/D by reciprocal + two Newton steps + one residual correction of the quotient (7 fp64
    // instructions instead of the 12 of an IEEE divide; D is a product of finite positive
    // denominators in [1e-288, 1e296], so no special cases; the quotient is within 1 ulp)
    __device__ __forceinline__ void flush() {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double r = __builtin_amdgcn_rcp(D[k]);
            r = fma(fma(-D[k], r, 1.0), r, r);
            r = fma(fma(-D[k], r, 1.0), r, r);
            double q = N[k] * r;
            q = fma(fma(-D[k], q, N[k]), r, q);
            acc[k] += q;
            N[k] = 0.0; D[k] = 1.0;
        }
        cnt = 0;
    }
};

// One line against a lane's R points: an IEEE divide per pair.
template <int R, bool MASKED>
__device__ __forceinline__ void lorentz_term(double a2, double KL, double d0, double Hf, WaveAcc<R>& S) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const double d = d0 + (double)k;
        double t = KL / fma(d, d, a2);
        if (MASKED) t = (fabs(d) <= Hf) ? t : 0.0;
        S.acc[k] += t;
    }
}

// ---- variant 0: line records through the scalar cache (one s_load per wave and line) ----
template <int R, bool MASKED>
__device__ __forceinline__ void process_lines_scalar(const HotRec* hot, const ColdRec* cold, int i0, int i1, double x0,
                                                     int wlo, int whi, double Hf, WaveAcc<R>& S) {
    for (int i = i0; i < i1; ++i) {
        Rec r = load_rec_scalar(hot, cold, i, false);
        const double d0 = x0 - r.cf;
        lorentz_term<R, MASKED>(r.a2, r.KL, d0, Hf, S);
        const int dist = max(0, max(r.ci - whi, wlo - r.ci));
        if (dist < r.dgi) {
            r = load_rec_scalar(hot, cold, i, true);
            gauss_term<R, 0>(r.KG, r.b, r.q2 >= 0.0, d0, Hf, r.q2, S.acc);
        }
    }
}

// Line ranges of a wave whose points span [wlo, whi] (cidx is sorted):
//   [iA, iB)  left-edge lines,   c in [wlo-H, whi-H)      -> masked
//   [iB, iC)  interior lines,    c in [whi-H, wlo+H]      -> every point inside the support
//   [iC, iD)  right-edge lines,  c in (wlo+H, whi+H]      -> masked
// Four lower bounds at once: lane group q = lane/16 searches target q with a 16-ary search
// (16 probes per step, range / 17 per step): 4-5 dependent loads for 10^5..10^6 lines instead
// of the 17-19 of a binary search, which cost a third of a short wave's lifetime.
__device__ __forceinline__ void wave_line_ranges(const int32_t* __restrict__ cidx, int n_lines, int wlo, int whi, int H,
                                                 int lane, int& iA, int& iB, int& iC, int& iD) {
    const long long tA = (long long)wlo - H, tB = (long long)whi - H;
    const long long tC = (long long)wlo + H + 1, tD = (long long)whi + H + 1;
    const int q = lane >> 4, jj = lane & 15;
    const long long tgt = q == 0 ? tA : q == 1 ? tB : q == 2 ? tC : tD;
    const unsigned long long gmask = 0xFFFFull << (q * 16);
    int lo = 0, hi = n_lines;                       // answer a = first i with cidx[i] >= tgt, a in [lo, hi]
    while (__any(hi > lo)) {
        const long long len = (long long)hi - lo;
        const int pos = lo + (int)(((long long)(jj + 1) * len) / 17);       // < hi whenever len > 0
        const bool below = (len > 0) && ((long long)cidx[len > 0 ? pos : 0] < tgt);
        const int k = __popcll(__ballot(below) & gmask);                     // probes are sorted: the first k are below
        if (len > 0) {
            const int p_k = lo + (int)(((long long)(k + 1) * len) / 17);
            const int p_km1 = lo + (int)(((long long)k * len) / 17);
            const int new_lo = k > 0 ? p_km1 + 1 : lo;
            const int new_hi = k < 16 ? p_k : hi;
            lo = new_lo; hi = new_hi;
        }
    }
    iA = __builtin_amdgcn_readlane(lo, 0);
    iB = __builtin_amdgcn_readlane(lo, 16);
    iC = __builtin_amdgcn_readlane(lo, 32);
    iD = __builtin_amdgcn_readlane(lo, 48);
    if (tB >= tC) { iB = iD; iC = iD; }      // span wider than the support: no interior line
}

// The far-field variant also needs the two indices that bound the NEAR lines, so six lower
// bounds: lane group q = lane/8 searches target q with a 9-way split per step (8 probes).
//   [iB, iF1)  far-left interior lines,  c <= fl      [iF2, iC)  far-right interior lines,  c >= fr
__device__ __forceinline__ void wave_line_ranges_far(const int32_t* __restrict__ cidx, int n_lines, int wlo, int whi, int H,
                                                     long long fl, long long fr, int lane, int& iA, int& iB, int& iC,
                                                     int& iD, int& iF1, int& iF2, int& iN1, int& iN2, long long nl, long long nr) {
    const long long tA = (long long)wlo - H, tB = (long long)whi - H;
    const long long tC = (long long)wlo + H + 1, tD = (long long)whi + H + 1;
    const int q = lane >> 3, jj = lane & 7;
    const long long tgt = q == 0 ? tA : q == 1 ? tB : q == 2 ? tC : q == 3 ? tD : q == 4 ? fl + 1 : q == 5 ? fr : q == 6 ? nl + 1 : nr;
    const unsigned long long gmask = 0xFFull << (q * 8);
    int lo = 0, hi = n_lines;
    while (__any(hi > lo)) {
        const long long len = (long long)hi - lo;
        const int pos = lo + (int)(((long long)(jj + 1) * len) / 9);
        const bool below = (len > 0) && ((long long)cidx[len > 0 ? pos : 0] < tgt);
        const int k = __popcll(__ballot(below) & gmask);
        if (len > 0) {
            const int p_k = lo + (int)(((long long)(k + 1) * len) / 9);
            const int p_km1 = lo + (int)(((long long)k * len) / 9);
            const int new_lo = k > 0 ? p_km1 + 1 : lo;
            const int new_hi = k < 8 ? p_k : hi;
            lo = new_lo; hi = new_hi;
        }
    }
    iA = __builtin_amdgcn_readlane(lo, 0);
    iB = __builtin_amdgcn_readlane(lo, 8);
    iC = __builtin_amdgcn_readlane(lo, 16);
    iD = __builtin_amdgcn_readlane(lo, 24);
    iF1 = __builtin_amdgcn_readlane(lo, 32);
    iF2 = __builtin_amdgcn_readlane(lo, 40);
    if (tB >= tC) { iB = iD; iC = iD; }
    iF1 = min(max(iF1, iB), iC);
    iF2 = min(max(iF2, iF1), iC);
    iN1 = min(max(__builtin_amdgcn_readlane(lo, 48), iF1), iF2);       // the bounds at FF_MID half-spans, inside [iF1, iF2]
    iN2 = min(max(__builtin_amdgcn_readlane(lo, 56), iN1), iF2);
}

// XCD-aware tile order: blocks b and b+8 share an XCD (and its L2), so each XCD gets a
// contiguous run of tiles: neighbouring tiles read almost the same line records.
__device__ __forceinline__ int xcd_tile(int b, int n_tiles, int natural = 0) {
    if (natural == 1) return b < n_tiles ? b : -1;
    if (natural >= 2) {
        // low-discrepancy order: step through the tiles with a stride near n_tiles/phi (made coprime
        // to n_tiles), so that at any time the resident workgroups sample the whole grid evenly and
        // the last ones to start are a random draw instead of one dense region
        if (b >= n_tiles) return -1;
        int stride = (int)(0.6180339887498949 * (double)n_tiles) | 1;
        auto gcd = [](int a, int c) { while (c) { const int t = a % c; a = c; c = t; } return a; };
        while (stride > 1 && gcd(stride, n_tiles) != 1) stride += 2;
        if (stride >= n_tiles) stride = 1;
        return (int)(((long long)b * stride) % n_tiles);
    }
    const int chunk = (n_tiles + 7) >> 3;
    const int slot = b >> 3;
    if (slot >= chunk) return -1;
    const int tile = (b & 7) * chunk + slot;
    return tile < n_tiles ? tile : -1;
}

template <int R>
__device__ __forceinline__ void store_points(double* __restrict__ out, int p0, int n_end, const double (&acc)[R]) {
    if (p0 + R <= n_end) {
        if (R >= 2) {
#pragma unroll
            for (int k = 0; k < R; k += 2) {
                double2 v; v.x = acc[k]; v.y = acc[k + (R >= 2 ? 1 : 0)];
                *reinterpret_cast<double2*>(out + p0 + k) = v;
            }
        } else {
            out[p0] = acc[0];
        }
    } else {
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (p0 + k < n_end) out[p0 + k] = acc[k];
    }
}

template <int R>
__global__ __launch_bounds__(256) void xsec_accumulate_kernel(const AccumJob* __restrict__ jobs) {
    const AccumJob& J = jobs[blockIdx.y];
    const int tile = xcd_tile(blockIdx.x, J.n_tiles);
    if (tile < 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = uniform_i32(threadIdx.x >> 6);
    const int n_end = J.p_end;          // this job computes work-grid points [p_begin, p_end)
    const long long wave_lo_ll = (long long)J.p_begin + (long long)tile * (256LL * R) + (long long)wave * (64LL * R);
    if (wave_lo_ll >= n_end) return;
    const int wlo = (int)wave_lo_ll;
    const int whi = min(wlo + 64 * R - 1, n_end - 1);
    const int H = J.H;
    int iA, iB, iC, iD;
    wave_line_ranges(J.cidx, J.n_lines, wlo, whi, H, lane, iA, iB, iC, iD);

    const int p0 = wlo + lane * R;
    const double x0 = (double)p0;
    const double Hf = (double)H;
    WaveAcc<R> S;
    S.init(J.flush_every);
    process_lines_scalar<R, true>(J.hot, J.cold, iA, iB, x0, wlo, whi, Hf, S);
    process_lines_scalar<R, false>(J.hot, J.cold, iB, iC, x0, wlo, whi, Hf, S);
    process_lines_scalar<R, true>(J.hot, J.cold, iC, iD, x0, wlo, whi, Hf, S);
    S.flush();
    store_points<R>(J.out, p0, n_end, S.acc);
}

// ---- variant 3: wave-private LDS staging of the line records --------------------------------
// The scalar cache is not a streaming path: with one dependent s_load per (wave, line) the
// kernel ran at a tenth of the fp64 rate.  Here each wave streams its line range in chunks of
// 64 records with coalesced 16-byte vector loads (lane l fetches record c0+l), parks the chunk
// in its own 4 KB of LDS and reads every record back as a broadcast (all lanes, one address:
// conflict-free).  The next chunk's global loads are in flight while the current chunk is
// consumed, so neither HBM/L2 latency nor LDS latency is exposed, and no workgroup barrier is
// needed: waves stay independent.
//
// LS waves of a workgroup can share the same 64*R grid points and split that span's line range
// between them (small grids: more wavefronts without shrinking R); their partial sums meet in
// LDS in a fixed order, so results stay deterministic.
struct HotVals {
    double cf, a2, KL;
};

__device__ __forceinline__ HotVals lds_hot(const double* __restrict__ lh, int j) {
    const double* h = lh + j * 4;
    HotVals v;
    v.cf = h[0]; v.a2 = h[1]; v.KL = h[2];
    return v;
}

// Lorentz terms of records j0..j1-1 of the chunk parked in this wave's LDS, as a branch-free
// running-fraction loop: per point  d = d0+k, den = d*d+a2, t = K*D, N = N*den+t, D = D*den.
// The NEXT record's broadcast read is issued before the current record's arithmetic, so the LDS
// latency hides under the 5*R fp64 instructions (at the chunk end that read lands in the cold records behind slot 63 - at most
// `step` slots further, inside the wave's staging area - and is dropped: no clamp, the address just counts up).
// The flush test sits outside the inner loop (blocks of at most `every` lines), and Gaussian /
// plain-divide lines are handled after the chunk from bit masks, so the hot loop has no branch.
template <int R, bool MASKED>
__device__ __forceinline__ void rf_segment(const double* __restrict__ lh, int j0, int j1, double x0, double Hf,
                                           WaveAcc<R>& S, int step = 1, int phase = 0) {
    // records j0 <= j < j1 with j % step == phase (step = line split of the span, a power of two)
    int j = j0 + ((phase - j0) & (step - 1));
    while (j < j1) {
        const int left = (j1 - j + step - 1) / step;
        const int nb = min(S.every - S.cnt, left);
        HotVals nxt = lds_hot(lh, j);
#pragma unroll 2
        for (int t = 0; t < nb; ++t) {
            const HotVals cur = nxt;
            nxt = lds_hot(lh, j + (t + 1) * step);      // (past the chunk's last record: words of the cold records, read and never used)
            const double d0 = x0 - cur.cf;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const double d = d0 + (double)k;
                const double den = fma(d, d, cur.a2);
                double K = cur.KL;
                if (MASKED) K = (fabs(d) <= Hf) ? K : 0.0;
                const double tt = K * S.D[k];
                S.N[k] = fma(S.N[k], den, tt);
                S.D[k] *= den;
            }
        }
        j += nb * step;
        S.cnt += nb;
        if (S.cnt >= S.every) S.flush();
    }
}

// Rare per-record work of a chunk, driven by the masks computed when the chunk was staged:
// gmask bit j: record j's Gaussian term can matter for some point of this wave;
// dmask bit j: record j's denominator is outside the running-fraction range -> plain divide
// (its LDS copy carries K = 0, a2 = 1 so the hot loop adds nothing for it).
// LDS slot of grid-point offset o within a wave's span (padded so that a lane writing its R
// consecutive points and a lane reading every 64th point are both nearly conflict-free)
__device__ __forceinline__ int span_slot(int o) { return o + (o >> 4); }

// Transposed Gaussian pass: FOUR records at once, lane group q = lane/16 takes one of them and lane t =
// lane%16 of the group walks the 16 consecutive points 16t .. 16t+15 of the span with the recurrence
// g(d+1) = g(d) r(d), r(d+1) = r(d) q2: two exp per 16 points instead of per 4 (25 instead of 51 wave
// instructions per record).  Sums go to G[16] per lane (point 16t+k of the span, partial over this
// group's records); gauss_runs_fold adds the four groups' partial sums to the owners of the points
// in a fixed order.  Lines flagged REC_LONG_RUN by K1 come here; MASKED for those whose support ends
// inside the span.
// RUN = 16 points per lane: 16 lanes per record, four records per pass (the description above).  RUN = 32 (round 6, the
// three-waves-per-SIMD build of the far-field kernel: -DLBL_FF_WPS=3 -DLBL_GAUSS_RUN=32): 8 lanes per record, eight records
// per pass, two exp per 32 points - 142 instead of 92 wave-instructions per pass for twice the records - and 64 instead of
// 32 registers of sums.
template <int RUN, bool MASKED>
__device__ __forceinline__ void gauss_runs(const double* __restrict__ lh, const double* __restrict__ lc,
                                           unsigned long long m, double xrun, double Hf, int lane, double (&G)[RUN]) {
    constexpr int LPR = 256 / RUN, NREC = 64 / LPR;       // lanes per record, records per pass
    const int q = lane / LPR;
    // The records of the mask as a list of bytes in the wave's LDS (behind the staged records), built once: every pass then
    // reads its four record numbers (one ds_read_u8 per lane) instead of scanning the mask with ~32 scalar instructions -
    // which are not free: each takes an issue slot of its wave (round 5: merged C3 K2 243.5 -> 238.7 us, bit-identical).
    unsigned char* list = reinterpret_cast<unsigned char*>(const_cast<double*>(lh) + 512);
    const int cnt = __popcll(m);
    __builtin_amdgcn_wave_barrier();
    if ((m >> lane) & 1ull)
        list[__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u))] = (unsigned char)lane;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int j_first = __builtin_ctzll(m);
    for (int p = 0; p < cnt; p += NREC) {
        const int slot = p + q;
        const int j = slot < cnt ? (int)list[slot] : -1;
        const int jj = j < 0 ? j_first : j;
        const double cf = lh[jj * 4];
        const double* c = lc + jj * 4;
        const double KG = j < 0 ? 0.0 : c[0], b = c[1], q2 = c[2];
        const double d0 = xrun - cf;
        double g = KG * exp_clamped(-b * (d0 * d0));
        double rr = exp_clamped(fmin(-b * (2.0 * d0 + 1.0), 700.0));
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            if (MASKED) G[k] += (fabs(d0 + (double)k) <= Hf) ? g : 0.0;      // support ends inside the span (cls:394)
            else G[k] += g;
            g *= rr;
            rr *= q2;
        }
    }
}

// G (lane (q, t): points RUN t .. RUN t + RUN-1, partial sums of group q) -> acc (lane l: points R l .. R l + R-1), through
// the wave's LDS scratch.  RUN = 16: 2 KB, one group per round, groups added in the order 0..3.  RUN = 32: four regions of
// 272 doubles, four groups per round (group q in region q % 4), two rounds; groups added in the order 0..7.
template <int R, int RUN>
__device__ __forceinline__ void gauss_runs_fold(const double (&G)[RUN], double* scratch, int lane, double (&acc)[R]) {
    constexpr int LPR = 256 / RUN, NREC = 64 / LPR, NREG = RUN / 8, REGION = 272;      // regions in use at once: 2 (RUN 16: one suffices, kept at 1 below) / 4
    const int q = lane / LPR, t = lane % LPR;
    if (RUN == 16) {
#pragma unroll
        for (int round = 0; round < 4; ++round) {
            __builtin_amdgcn_wave_barrier();
            if (q == round) {
#pragma unroll
                for (int k = 0; k < RUN; ++k) scratch[span_slot(16 * t + k)] = G[k];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < R; ++k) acc[k] += scratch[span_slot(lane * R + k)];
        }
    } else {
#pragma unroll
        for (int round = 0; round < NREC / NREG; ++round) {
            __builtin_amdgcn_wave_barrier();
            if (q / NREG == round) {
                double* reg = scratch + (q % NREG) * REGION;
#pragma unroll
                for (int k = 0; k < RUN; ++k) reg[span_slot(RUN * t + k)] = G[k];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int g = 0; g < NREG; ++g) {
#pragma unroll
                for (int k = 0; k < R; ++k) acc[k] += scratch[g * REGION + span_slot(lane * R + k)];
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
}

template <int R, int LONGG = 0, int RUN = 16>
__device__ __forceinline__ void chunk_extras(const double* __restrict__ lh, const double* __restrict__ lc,
                                             unsigned long long gmask, unsigned long long emask,
                                             unsigned long long dmask, unsigned long long imask, double x0, double Hf,
                                             WaveAcc<R>& S, unsigned long long lmask, double xrun, int lane,
                                             double (&G16)[RUN]) {
    // emask bit j: record j must use one exp per point (profile too narrow for the recurrence)
    // imask bit j: record j is an interior line (every point of the wave inside its support): no masking
    // lmask bit j: record j may take the transposed 16-point runs (LONGG kernels, R = 4)
    if (LONGG && R == 4) {
        // LONGG 1: interior lines only (far-field kernel: its spans see few masked Gaussian records, and the
        // masked instantiation costs it 1 % in registers and code); 2: masked ones too (all-direct kernel,
        // i.e. the narrow-window layers of a column, where most records end inside the span)
        const unsigned long long ml = gmask & ~emask & lmask & (LONGG >= 2 ? ~0ull : imask);
        if (ml & imask) gauss_runs<RUN, false>(lh, lc, ml & imask, xrun, Hf, lane, G16);
        if (LONGG >= 2 && (ml & ~imask)) gauss_runs<RUN, true>(lh, lc, ml & ~imask, xrun, Hf, lane, G16);
        gmask &= ~ml;
    }
    unsigned long long m = gmask & ~emask & imask;
    while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const double d0 = x0 - lh[j * 4];
        const double* c = lc + j * 4;
        gauss_term<R, 1, false>(c[0], c[1], true, d0, Hf, c[2], S.acc);
    }
    m = gmask & ~emask & ~imask;
    while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const double d0 = x0 - lh[j * 4];
        const double* c = lc + j * 4;
        gauss_term<R, 1, true>(c[0], c[1], true, d0, Hf, c[2], S.acc);
    }
    m = gmask & emask;
    while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const double d0 = x0 - lh[j * 4];
        const double* c = lc + j * 4;
        gauss_term<R, 0>(c[0], c[1], false, d0, Hf, 0.0, S.acc);
    }
    while (dmask) {
        const int j = __builtin_ctzll(dmask);
        dmask &= dmask - 1;
        const double d0 = x0 - lh[j * 4];
        const double* c = lc + j * 4;
        const double a2 = 1.0 / c[1], KL = c[3];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const double d = d0 + (double)k;
            const double t = KL / fma(d, d, a2);
            S.acc[k] += (fabs(d) <= Hf) ? t : 0.0;
        }
    }
}

// Lines of one job against the 64*R points of a wave (wlo..whi; x0 = this lane's first point):
// the 64-line chunks [c0, c0+64) for c0 = mA, mA+stride, ... below mD.  stride = 64 walks a
// contiguous range; stride = 64*LS deals the chunks of a span round-robin to the LS waves that
// share it, so each wave gets its share of the expensive lines near the span (Gaussian passes):
// with contiguous quarters the two middle waves did ~1.8x the work of the outer two.
// Lines below iB or from iC on end inside the wave's span and are masked per point.
// The wave streams the records in chunks of 64 through its own LDS (lh: hot halves, lc: cold
// halves), with the next chunk's loads in flight while the current one is consumed.
template <int R, int LONGG = 0, int RUN = 16>
__device__ __forceinline__ void accumulate_lines(const HotRec* hot, const ColdRec* cold, int mA, int mD, int iB, int iC,
                                                 int wlo, int whi, double x0, double Hf, double* lh, double* lc, int lane,
                                                 WaveAcc<R>& S, double (&G16)[RUN], int stride = 64, int step = 1, int phase = 0,
                                                 int nL = 0, int nR = 0x7fffffff) {
    // [nL, nR): the records whose LORENTZ term this walk adds (round 6: the lines between FF_MID and FF_FAR half-spans take
    // their Lorentz term from the series and only their Gaussian part from this walk)
    // step > 1 (with stride = 64): every wave of the span walks ALL chunks but takes only the records
    // j % step == phase of each, so the split is exact to a line.  Dealing whole chunks left one wave
    // of a two-way split with 128 of a span's ~210 near lines and the other with 82.
    const unsigned long long stripe = step == 1 ? ~0ull : step == 2 ? (0x5555555555555555ull << phase)
                                    : step == 4 ? (0x1111111111111111ull << phase) : (0x0101010101010101ull << phase);
    // global address space made explicit: a flat load would also count on lgkmcnt and every
    // LDS wait would then drain the prefetch of the next chunk
    typedef double v2f64 __attribute__((ext_vector_type(2)));
    typedef const v2f64 __attribute__((address_space(1)))* GlobalF64x2;
    const GlobalF64x2 gh = (GlobalF64x2)(unsigned long long)hot;
    const GlobalF64x2 gc = (GlobalF64x2)(unsigned long long)cold;
    // software pipeline: registers hold the NEXT chunk's hot halves while LDS holds the current one
    v2f64 h0 = {0, 0}, h1 = {0, 0};
    if (mA + lane < mD) {
        const long long r = (long long)(mA + lane) * 2;
        h0 = gh[r]; h1 = gh[r + 1];
    }
    for (int c0 = mA; c0 < mD; c0 += stride) {
        const int c1 = min(c0 + 64, mD);
        __builtin_amdgcn_wave_barrier();
        // per-record branch decisions for the whole chunk, one lane per record
        const int ci = (int)h0.x;
        const int dgi = __double2loint(h1.y), fl = __double2hiint(h1.y);
        const bool valid = c0 + lane < c1;
        const bool mine = (stripe >> lane) & 1ull;
        const bool gauss = valid && mine && max(0, max(ci - whi, wlo - ci)) < dgi;
        const bool direct = valid && (fl & REC_DIRECT_DIV) != 0;
        const unsigned long long gmask = __ballot(gauss);
        const unsigned long long dmask = __ballot(direct && c0 + lane >= nL && c0 + lane < nR) & stripe;
        const unsigned long long emask = __ballot((fl & REC_NO_RECUR) != 0);
        const unsigned long long lmask = LONGG ? __ballot((fl & (RUN == 32 ? REC_LONG_RUN32 : REC_LONG_RUN)) != 0) : 0ull;
        v2f64 w0 = h0, w1 = h1;
        if (direct) { w0.y = 1.0; w1.x = 0.0; }          // a2 = 1, KL = 0 in the hot loop's copy
        reinterpret_cast<v2f64*>(lh)[lane * 2] = w0;
        reinterpret_cast<v2f64*>(lh)[lane * 2 + 1] = w1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // cold halves only for the records that will use them (about one in eight); they
        // land while the Lorentz loop below runs
        v2f64 c0v = {0, 0}, c1v = {0, 0};
        if (gauss || (direct && mine)) {
            const long long r = (long long)(c0 + lane) * 2;
            c0v = gc[r]; c1v = gc[r + 1];
        }
        if (c0 + stride + lane < mD && lane < 64) {
            const long long r = (long long)(c0 + stride + lane) * 2;
            h0 = gh[r]; h1 = gh[r + 1];
        }
        // the three classes of lines inside this chunk, as offsets into the chunk
        const int a1 = max(min(iB, c1), c0) - c0;
        const int b1 = max(min(iC, c1), c0) - c0;
        const int n0 = max(min(nL, c1), c0) - c0, n1 = max(min(nR, c1), c0) - c0;     // the chunk's share of [nL, nR)
        rf_segment<R, true>(lh, n0, min(a1, n1), x0, Hf, S, step, phase);
        rf_segment<R, false>(lh, max(a1, n0), min(b1, n1), x0, Hf, S, step, phase);
        rf_segment<R, true>(lh, max(b1, n0), n1, x0, Hf, S, step, phase);
        if (gmask | dmask) {
            if (gauss || (direct && mine)) {
                reinterpret_cast<v2f64*>(lc)[lane * 2] = c0v;
                reinterpret_cast<v2f64*>(lc)[lane * 2 + 1] = c1v;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // records a1..b1-1 of the chunk are interior lines
            const unsigned long long imask = (b1 > a1) ? ((b1 - a1 >= 64 ? ~0ull : ((1ull << (b1 - a1)) - 1ull)) << a1) : 0ull;
            chunk_extras<R, LONGG, RUN>(lh, lc, gmask, emask, dmask, imask, x0, Hf, S, lmask,
                                        (double)(wlo + RUN * (lane % (256 / RUN))), lane, G16);
        }
    }
}

// ---- variant 5: far-field series for distant Lorentz lines -------------------------------------
// Most (line, span) pairs are far apart: with a +-5 cm^-1 window at 0.001 cm^-1 a line reaches
// 40 spans of 256 points and is more than 8 half-spans away from 75 % of them.  For such a line
// (centre c, delta = c - xc from the span centre xc, s = delta^2 + a^2) the Lorentz term is a
// smooth function of u = x - xc over the whole span and its generating function is that of the
// Chebyshev polynomials of the second kind:
//     K / ((u - delta)^2 + a^2) = (K/s) / (1 - 2 X t + t^2) = (K/s) sum_n U_n(X) t^n,
//     X = delta / sqrt(s),  t = u / sqrt(s),  |t| <= rho = h / |delta| <= 1 / FF_FAR.
// In the scaled variable tau = u/h the coefficients q_n = (K/s) U_n(X) (h/sqrt(s))^n obey
//     q_0 = K beta,  q_1 = alpha q_0,  q_{n+1} = alpha q_n - beta' q_{n-1},
//     beta = 1/s,  alpha = 2 h delta beta,  beta' = h^2 beta,
// i.e. three fp64 instructions per order and LINE instead of five per line and POINT.  One lane
// takes one line, adds its q_n to per-lane sums C_n; the 64 lanes' sums are then reduced once per
// span and the polynomial is evaluated at every lane's R points (Horner in tau, |tau| < 1).
// Truncation after FF_NT terms: |sum_{n>=NT} U_n t^n| <= rho^NT (NT (1-rho) + 1) / (1-rho)^2,
// relative to a term that is >= (K/s) / (1+rho)^2: with rho = 1/4 and NT = 30 that is 5.7e-17,
// below half an ulp (measured sweep of threshold/terms: 4/30 beat 8/20, 6/24, 3/40 and 12/16), so the series is as exact as the sum it replaces (it carries fewer roundings:
// measured 2e-16 against a long-double sum where the direct fp64 sum has 7e-16).
// Edge lines (support ends inside the span) and near lines keep the direct path; a far line whose
// Gaussian part still matters on the span (wide Doppler cores) gets its Gaussian pass as usual.
#ifndef LBL_FF_FAR
#define LBL_FF_FAR 4
#define LBL_FF_NT 30
#endif
constexpr int FF_FAR = LBL_FF_FAR;   // a line is far when |c - xc| >= FF_FAR * (32 R)
constexpr int FF_NT = LBL_FF_NT;     // series terms (exact mode: remainder below half an ulp)
// Budget mode (lbl_set_option "accuracy" 1: <= 1e-9 relative on the absorption coefficient instead of the last bits;
// BASELINE north_star asks for 1e-6).  The remainder after NT terms is at most
// rho^NT (NT (1 - rho) + 1) (1 + rho)^2 / (1 - rho)^2 of the line's own smallest term on the span; every term of the sum
// is positive, so the sum's relative error is below the worst line's.  At rho <= 1/4: 5.9e-10 with 18 terms, falling by
// 4x per further half-span.
constexpr int FF_NT_BUDGET = 18;
// (Measured and dropped: far from 3 half-spans on in budget mode - rho <= 1/3, 24 terms leave 2.4e-10 - takes a quarter of
// the near lines out of the direct loop but lengthens the reduction and the polynomial: C3 K2 231.9 vs 230.5 us, C2 55.1 vs
// 50.2, the column 3.78 vs 3.90 ms: no gain overall.  The threshold stays a template constant per mode.)
constexpr int FF_FAR_BUDGET = 4;
template <int NT> struct FarThreshold { static constexpr int value = NT == FF_NT_BUDGET ? FF_FAR_BUDGET : FF_FAR; };
// Round 6, the three-waves-per-SIMD build of the exact mode (32-point Gaussian runs, 168 VGPRs): the series takes the
// Lorentz terms from FF_MID = 3 half-spans on, with FF_NT_MID = 38 terms for the chunks nearer than 4 (rho <= 1/3: remainder
// <= rho^38 (38 (1 - rho) + 1) (1 + rho)^2 / (1 - rho)^2 = 7.8e-17 of a line's own smallest term on the span, below half an ulp).
// The lines between 3 and 4 half-spans - a quarter of what the running fraction used to walk - keep their Gaussian parts in
// the near walk's runs (the span table carries both bounds: slots 4, 5 at FF_FAR, slots 6, 7 at FF_MID).  Measured with the
// Gaussian parts switched off (diagnostic builds, same box): K2 165 -> 151.5 us on the merged 100-2500 cm^-1 cell.
constexpr int FF_MID = 3;
constexpr int FF_NT_MID = 38;
template <int NT> struct LorentzNear { static constexpr int value = NT == FF_NT_MID ? FF_MID : FarThreshold<NT>::value; };

template <int CTRL>
__device__ __forceinline__ double dpp_move_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    // (bound_ctrl with full row and bank masks: a lane without a source reads 0 and the compiler needs no preset of the
    // destination - with bound_ctrl off every 64-bit move cost two extra v_mov_b32 0; round 6)
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// sum over the 64 lanes, same value (and same summation tree) in every lane; all lanes must be active
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp_move_f64<0xB1>(v);       // quad_perm [1,0,3,2]
    v += dpp_move_f64<0x4E>(v);       // quad_perm [2,3,0,1]
    v += dpp_move_f64<0x141>(v);      // row_half_mirror
    v += dpp_move_f64<0x140>(v);      // row_mirror: every lane of a row holds the row's sum
    return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// Sums over the 64 lanes of NT per-lane values, eight at a time through the wave's LDS scratch
// (8 rows of 72 doubles): every lane parks its 8 values (row n, column lane, one pad per 8 lanes),
// lane (n, j) = (l >> 3, l & 7) adds the 8 entries of segment j of row n, three DPP steps add the
// 8 segments, and the row total is read back as a wave-uniform value.  About 50 instructions per
// 8 values instead of 23 per value for the all-lanes butterfly; fixed summation tree.
template <int NT>
__device__ __forceinline__ void wave_sum_rows(double (&C)[NT], double* scratch, int lane) {
    const int wr = lane + (lane >> 3);                       // column of this lane inside a row
    const int rd = (lane >> 3) * 72 + (lane & 7) * 9;        // first entry of this lane's segment
#pragma unroll
    for (int base = 0; base < NT; base += 8) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int n = 0; n < 8; ++n)
            if (base + n < NT) scratch[n * 72 + wr] = C[base + n];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        double t = 0.0;
        if (base + (lane >> 3) < NT) {
            const double* seg = scratch + rd;
            t = ((seg[0] + seg[1]) + (seg[2] + seg[3])) + ((seg[4] + seg[5]) + (seg[6] + seg[7]));
        }
        t += dpp_move_f64<0xB1>(t);
        t += dpp_move_f64<0x4E>(t);
        t += dpp_move_f64<0x141>(t);
#pragma unroll
        for (int n = 0; n < 8; ++n)
            if (base + n < NT) C[base + n] = readlane_f64(t, n * 8);
    }
    __builtin_amdgcn_wave_barrier();
}

// Terms a chunk of far lines needs, by the distance d (in half-spans) of its NEAREST line from the span centre:
// rho <= 1/d, and the remainder bound above falls fast with d.  Exact mode (remainder below 7.8e-17, half an ulp of the
// line's own smallest term on the span, which the 38 terms from 3 half-spans on meet): one class per distinct count, each
// starting at the first whole d whose bound admits that count - the staircase 38 / 30 / 26 / 23 / 21 / 20 / 19 / 18 from
// d = 3 .. 10, then 17 from 11, 16 from 13, 15 from 15, 14 from 18, 13 from 22, 12 from 28 and 11 from 37 on (the window of a
// one-atmosphere cell ends at 39).  Budget mode (NT = 18, 5.9e-10) keeps four classes: d >= 8: 12 (2.8e-10), d >= 16: 9
// (1.8e-10), d >= 32: 7 (2.6e-10).
// The classes as {d, terms} pairs, nearest first: the only place a count lives (far_chunk's descent and the edge series'
// count take theirs from the table of the build's mode).  tests/test_far_terms_cpu.py reads these two lines and holds
// every pair to the remainder bound of its mode; tests/test_far_classes_cpu.py holds the exact table to the minimal count
// at every whole d:
constexpr int kFarClassExact[15][2] = {{3, 38}, {4, 30}, {5, 26}, {6, 23}, {7, 21}, {8, 20}, {9, 19}, {10, 18}, {11, 17}, {13, 16}, {15, 15}, {18, 14}, {22, 13}, {28, 12}, {37, 11}};
constexpr int kFarClassBudget[4][2] = {{4, 18}, {8, 12}, {16, 9}, {32, 7}};
static_assert(kFarClassExact[0][0] == FF_MID && kFarClassExact[0][1] == FF_NT_MID && kFarClassExact[1][0] == FF_FAR && kFarClassExact[1][1] == FF_NT &&
              kFarClassBudget[0][0] == FF_FAR_BUDGET && kFarClassBudget[0][1] == FF_NT_BUDGET, "the nearest classes are the builds' own thresholds and term counts");
constexpr int FF_EDGE_MIN = 8;       // the edge series is entered from this many half-spans on (series_edges)
// Where far_chunk's descent stops, exact mode: the distances (half-spans, nearest first) at which a chunk may leave the
// chain; a chunk takes the count of the table class of the last stop at or below its distance, so a chunk between two
// stops runs up to three terms more than its own class needs (never fewer: the bound holds).  Not every class is a stop,
// because a stop is not free: one scalar compare and one branch for every chunk that comes by, measured at about
// what ONE term costs (three dependent fp64 instructions) - with all 15 classes as stops a merged 100-2500 cm^-1 launch ran
// 1.8e6 fewer vector and 0.7e6 more scalar instructions in the same time as with the five stops 3 / 4 / 8 / 16 / 32 before.
// A stop pays where (the share of the passing chunks that leave) x (the terms they shed) exceeds that.  With a chunk's
// distance spread evenly over 3 .. 38 half-spans: five stops 18.0 terms and 2.3 compares per chunk, all fifteen 16.0 and
// 5.3, these eight (38 / 30 / 26 / 23 / 20 / 17 / 15 / 13 terms) 16.6 and 2.4 - the least cost for a compare worth 0.8 of
// a term, and within 1 % of it from 0.5 to 1.1.  The edge series pays its compares once per span and takes the count of
// its own class.  (LBL_FAR_STOPS: A/B builds, scripts/make_variant_lib.sh.)
#ifndef LBL_FAR_STOPS
#define LBL_FAR_STOPS {3, 4, 5, 6, 8, 11, 15, 22}
#endif
constexpr int kFarStopsExact[] = LBL_FAR_STOPS;
static_assert(kFarStopsExact[0] == FF_MID && kFarStopsExact[1] == FF_FAR, "the nearest stops are the builds' own thresholds");
// The classes and stops of one build: NT == FF_NT_MID walks the exact mode's stops from the first (3 half-spans), NT == FF_NT
// from the second (that build's series starts at FF_FAR and never enters the d = 3 segment); NT == FF_NT_BUDGET stops at
// every class of the budget table; any other NT (diagnostic builds) is one class of NT terms.
template <int NT> struct FarTerms {
    static constexpr bool exact = NT == FF_NT || NT == FF_NT_MID, budget = NT == FF_NT_BUDGET;
    static constexpr int first = exact && NT != FF_NT_MID ? 1 : 0;
    static constexpr int count = exact ? (int)(sizeof(kFarClassExact) / sizeof(kFarClassExact[0])) : (budget ? (int)(sizeof(kFarClassBudget) / sizeof(kFarClassBudget[0])) : 1);
    static constexpr int dist(int i) { return exact ? kFarClassExact[i][0] : (budget ? kFarClassBudget[i][0] : 0); }
    static constexpr int terms(int i) { return exact ? kFarClassExact[i][1] : (budget ? kFarClassBudget[i][1] : NT); }
    static constexpr int edge_first() { int i = first; while (i + 1 < count && dist(i) < FF_EDGE_MIN) ++i; return i; }
    static constexpr int terms_at(int d) { int i = 0; while (i + 1 < count && dist(i + 1) <= d) ++i; return terms(i); }
    static constexpr int stops = exact ? (int)(sizeof(kFarStopsExact) / sizeof(kFarStopsExact[0])) : count;
    static constexpr int stop_dist(int s) { return exact ? kFarStopsExact[s] : dist(s); }
    static constexpr int stop_terms(int s) { return exact ? terms_at(kFarStopsExact[s]) : terms(s); }
    // terms of the class that a distance of dmin points falls into, among the classes from FF_EDGE_MIN half-spans on (the
    // edge series: once per span, scalar compares against compile-time limits, farthest class first)
    template <int R, int I = count - 1> static __device__ __forceinline__ int edge_terms(int dmin) {
        if constexpr (I > edge_first()) return dmin >= dist(I) * 32 * R ? terms(I) : edge_terms<R, I - 1>(dmin);
        else return terms(I);
    }
};

// q_N0 .. q_{N1-1} of one line per lane added to the per-lane sums (qa, qb: q_{N0-2}, q_{N0-1}; carried on)
template <int N0, int N1, int NT>
__device__ __forceinline__ void series_terms(double al, double bp, double& qa, double& qb, double (&C)[NT]) {
#pragma unroll
    for (int n = N0; n < N1; ++n) {
        const double qn = fma(al, qb, -(bp * qa));
        C[n] += qn;
        // (an empty statement the scheduler may not move code across: without it the compiler runs the whole chain of
        // q_n first and sinks the additions behind the term-count branches - 20 more live values, spilled in the loop)
        // (also after a segment's last term: the one-term segments of the distance classes would otherwise have none)
        if ((n & 1) == 1 || n == N1 - 1) asm volatile("" : "+v"(C[n]));
        qa = qb; qb = qn;
    }
}

// The terms beyond those of stop I (already added), for a chunk whose nearest line is dmin2 / 2 points from the span
// centre: while the chunk lies nearer than stop I, the segment up to the next nearer stop's count, farthest stop first -
// a distant chunk (most of them) leaves after one or two scalar compares, only a span's two or three nearest walk the whole
// chain.  Integer compares against compile-time limits (stop I lies at stop_dist(I) half-spans = 32 R stop_dist(I) points).
template <int R, int NT, int I>
__device__ __forceinline__ void far_descent(int dmin2, double al, double bp, double& qa, double& qb, double (&C)[NT]) {
    typedef FarTerms<NT> FT;
    if constexpr (I > FT::first) {
        if (dmin2 < 2 * FT::stop_dist(I) * 32 * R) {
            series_terms<FT::stop_terms(I), FT::stop_terms(I - 1), NT>(al, bp, qa, qb, C);
            far_descent<R, NT, I - 1>(dmin2, al, bp, qa, qb, C);
        }
    }
}

// A far line's Gaussian part that still reaches the span.  At 1 atm and 0.001 cm^-1 that is no rare case: a pseudo-Voigt
// profile is a = 50-100 points wide and K1's cut-off dgi 290-580 points, while the far class begins 384 points from the
// span's edge - a merged 100-2500 cm^-1 span has 20 such records (median 14, at most 78) beside the 136 of its near walk.
// The four-point pass of chunk_extras costs them 51 wave-instructions each (two exp per four points) where the transposed
// runs of the near walk cost 142 per eight records.  So on the production shape (GROUTE: unsplit spans, one wave walks all
// of a span's records) a far record nearer than FF_GAUSS_CAP half-spans is only NOTED here - [g_lo, g_hi) grows to hold
// it - and the near walk, which forms the same predicate per record, is extended over that range: records are sorted by
// centre, so the noted ones and everything between them and the near lines are one index interval, and every (record, span)
// pair is still evaluated exactly once with the same cut-off.  The cap bounds what the near walk may have to stage beyond its
// own range (2 x 4 half-spans of records); 8 holds the whole class of a 1 atm cell (largest reach 582 + 128 points < 1,024).
// A record beyond the cap (several atmospheres, finer grids) keeps the four-point pass here.
constexpr int FF_GAUSS_CAP = 8;

// One chunk of far_field_lines: 64 records (PARTIAL: the nv = m1 - c0 < 64 first lanes; the others hold a copy of the call's
// last record and count for nothing), one per lane, in w0, w1.
template <int R, int NT, bool GROUTE, bool PARTIAL>
__device__ __forceinline__ void far_chunk(const double __attribute__((ext_vector_type(2))) w0, const double __attribute__((ext_vector_type(2))) w1,
                                          const ColdRec* cold, int c0, int m1, int reach_lim, double xc, int wlo, int whi,
                                          double x0, double Hf, double* lh, double* lc, int lane, double (&C)[NT], WaveAcc<R>& S,
                                          int& g_lo, int& g_hi) {
    // (every fused multiply-add of the series is spelled fma(); the products and sums beside them stay two roundings in
    // both copies of this body, whatever the compiler would make of each: the copies must agree to the last bit)
#pragma clang fp contract(off)
    typedef double v2f64 __attribute__((ext_vector_type(2)));
    typedef const v2f64 __attribute__((address_space(1)))* GlobalF64x2;
    const double hh = 32.0 * R;
    const int ci = (int)w0.x;
    // the chunk's nearest line (centres are sorted and a call stays on one side of the span: the first or the last
    // valid lane) decides how many terms the whole chunk takes; wave-uniform branches.  In integers (a centre is an
    // integer, xc = wlo + 32 R - 1/2): dmin2 = 2 |c - xc| from two v_readlane and scalar arithmetic instead of four
    // v_readlane and six fp64 vector instructions; the class limits are d half-spans = 32 R d points.
    const int nv = PARTIAL ? m1 - c0 : 64;
    const int ca = __builtin_amdgcn_readlane(ci, 0), cb = __builtin_amdgcn_readlane(ci, nv - 1);
    const int dmin2 = min(abs(2 * (ca - wlo) - (64 * R - 1)), abs(2 * (cb - wlo) - (64 * R - 1)));
    // Gaussian parts that still reach the span.  A record reaches it only if its distance from the span's nearest point,
    // at least dmin2 / 2 - 32 R + 1/2 for every record of the chunk, is below its cut-off dgi <= reach: a chunk with
    // dmin2 >= reach_lim = 2 (reach + 32 R) + 1 has none and forms neither the per-lane test nor its ballot.
    if (dmin2 < reach_lim) {
        const int dgi = __double2loint(w1.y), fl = __double2hiint(w1.y);
        bool gauss = (!PARTIAL || lane < nv) && max(0, max(ci - whi, wlo - ci)) < dgi;
        unsigned long long gmask = __ballot(gauss);
        if (GROUTE && gmask) {                         // (a chunk without such a record - most of them - pays the one ballot)
            // inside the cap: 2 |c - xc| < 2 * FF_GAUSS_CAP half-spans, in integers as dmin2 above (the left side is odd: no tie)
            const bool routed = abs(2 * (ci - wlo) - (64 * R - 1)) < 2 * FF_GAUSS_CAP * 32 * R;
            const unsigned long long rmask = __ballot(gauss && routed);      // wave-uniform, like c0: scalar registers
            if (rmask) {
                g_lo = min(g_lo, c0 + (int)__builtin_ctzll(rmask));
                g_hi = max(g_hi, c0 + 64 - (int)__builtin_clzll(rmask));
            }
            gauss = gauss && !routed;
            gmask &= ~rmask;
        }
        if (gmask) {                                   // (GROUTE: beyond the cap only - very wide profiles)
            const unsigned long long emask = __ballot((fl & REC_NO_RECUR) != 0);
            const GlobalF64x2 gc = (GlobalF64x2)(unsigned long long)cold;
            v2f64 c0v = {0, 0}, c1v = {0, 0};
            if (gauss) {
                const long long r = (long long)(c0 + lane) * 2;
                c0v = gc[r]; c1v = gc[r + 1];
            }
            __builtin_amdgcn_wave_barrier();
            reinterpret_cast<v2f64*>(lh)[lane * 2] = w0;
            reinterpret_cast<v2f64*>(lh)[lane * 2 + 1] = w1;
            reinterpret_cast<v2f64*>(lc)[lane * 2] = c0v;
            reinterpret_cast<v2f64*>(lc)[lane * 2 + 1] = c1v;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            double unused[16];
            chunk_extras<R, 0>(lh, lc, gmask, emask, 0ull, ~0ull, x0, Hf, S, 0ull, 0.0, lane, unused);
            __builtin_amdgcn_wave_barrier();
        }
    }
    const double dl = w0.x - xc;
    const double sq = fma(dl, dl, w0.y);
    double be = __builtin_amdgcn_rcp(sq);
    be = fma(fma(-sq, be, 1.0), be, be);
    be = fma(fma(-sq, be, 1.0), be, be);
    const double al = (dl * (2.0 * hh)) * be;
    const double bp = (hh * hh) * be;
    double qa = (PARTIAL ? (lane < nv ? w1.x : 0.0) : w1.x) * be;       // (only a call's last chunk can have lanes without a record)
    C[0] += qa;
    double qb = al * qa;
    C[1] += qb;
    typedef FarTerms<NT> FT;
    static_assert(FT::stop_terms(FT::first) == NT && FT::stop_terms(FT::stops - 1) >= 2, "a build's nearest class takes the build's own term count");
    static_assert(FT::count == 1 || FT::dist(FT::edge_first()) == FF_EDGE_MIN, "a class starts where the edge series is entered");
    series_terms<2, FT::stop_terms(FT::stops - 1), NT>(al, bp, qa, qb, C);
    far_descent<R, NT, FT::stops - 1>(dmin2, al, bp, qa, qb, C);
}

// Series coefficients of the far lines m0, m0+stride*k.. (chunks of 64, one line per lane) below m1.  stride: 64 LS, LS a
// power of two up to 8.  reach_lim: see far_chunk (INT_MAX: no bound on the records' cut-offs is known).
// The full chunks run without a validity mask; the call's last chunk, if partial, is a copy of the loop body of its own.
// A lane's record address is a scalar base plus a 32-bit byte offset that advances by 32 stride per chunk, clamped to the
// call's last record (so that every lane of every load is in bounds without a per-lane branch); the offsets of a call
// stay below 2^32 because a call of more than 2^26 records is walked in pieces of 2^26 (a whole number of strides).
template <int R, int NT, bool GROUTE = false>
__device__ __forceinline__ void far_field_lines(const HotRec* hot, const ColdRec* cold, int m0, int m1, int stride, int reach_lim,
                                                double xc, int wlo, int whi, double x0, double Hf, double* lh, double* lc,
                                                int lane, double (&C)[NT], WaveAcc<R>& S, int& g_lo, int& g_hi) {
    // (the records of a call are all far lines: with the series from FF_MID on, the lines between FF_MID and FF_FAR
    // half-spans are among them - inside the cap, so on the only shape that has them their Gaussian parts go to the near walk)
    static_assert(GROUTE || NT != FF_NT_MID, "the mid class needs the near walk to take its Gaussian parts");
    typedef double v2f64 __attribute__((ext_vector_type(2)));
    typedef const char __attribute__((address_space(1)))* GlobalBytes;
    typedef const v2f64 __attribute__((address_space(1)))* GlobalF64x2;
    constexpr int PIECE = 1 << 26;
    for (int p0 = m0; p0 < m1;) {
        const int p1 = m1 - p0 > PIECE ? p0 + PIECE : m1;
        const GlobalBytes base = (GlobalBytes)(unsigned long long)(hot + p0);
        const unsigned int last = (unsigned int)(p1 - 1 - p0) * 32u;
        unsigned int off = (unsigned int)lane * 32u;
        v2f64 h0, h1;
        auto fetch = [&](v2f64& h0, v2f64& h1) {
            const GlobalF64x2 r = (GlobalF64x2)(base + min(off, last));
            h0 = r[0]; h1 = r[1];
            off += (unsigned int)stride * 32u;
        };
        fetch(h0, h1);
        int c0 = p0;
        // (the chunk loop unrolled by two, with two register sets swapping roles instead of one rotating into the other,
        // was built and measured: 0.07e6 fewer vector and 0.42e6 more scalar instructions per merged C3 launch on the
        // three-waves-per-SIMD build, 20-52 bytes of scratch per lane on the builds held to 128 registers - not kept)
        for (; c0 + 64 <= p1; c0 += stride) {
            const v2f64 w0 = h0, w1 = h1;
            if (c0 + stride < p1) fetch(h0, h1);
            far_chunk<R, NT, GROUTE, false>(w0, w1, cold, c0, p1, reach_lim, xc, wlo, whi, x0, Hf, lh, lc, lane, C, S, g_lo, g_hi);
        }
        if (c0 < p1) far_chunk<R, NT, GROUTE, true>(h0, h1, cold, c0, p1, reach_lim, xc, wlo, whi, x0, Hf, lh, lc, lane, C, S, g_lo, g_hi);
        p0 = p1;
    }
}

// ---- narrow windows: skewed line ranges ---------------------------------------------------------
// The upper layers of a column have windows of 50-640 points (pyradClasses.py:655: 5 P / 1013.25 cm^-1).
// In the span kernel above a wave walks every line that reaches ANY of its 64 R points, and most of
// those end inside the span: masked lanes (8 instead of 5 instructions per point, half of them for
// nothing), and a span may not be wider than a line's support, so the narrowest layers run R = 1.
// Here every LANE walks the lines that reach ITS R points: sorted centre indices make that a
// contiguous range [A', B') of records per lane, shifted by R points from lane to lane, so at
// iteration t lane l is on record A'(l) + t: the lanes run down the line list side by side, each at
// about the same offset from its current line (a skewed, systolic walk).  Every lane has the same
// number of lines up to density fluctuations, none of them masked except the few (0-2 per lane)
// that cover only part of the lane's R points: per lane  [A', A) partial, [A, B) full, [B, B') partial,
//     A' = #{c < p0 - H}   A = #{c < p0 + R-1 - H}   B = #{c <= p0 + H}   B' = #{c <= p0 + R-1 + H}.
// The four counts of all 64 lanes come from one scatter + scan per chunk: record j adds itself to the
// first threshold above its centre (ds_max of j+1: centres are sorted, so the count IS the largest
// such j+1), then a prefix maximum over the thresholds (R per lane, DPP scan across lanes).
// Records are staged per chunk of 112 in the wave's LDS (hot 32 B + cold 32 B) and read back with
// per-lane addresses (neighbouring lanes read the same or the next record: conflict-free).
// The Gaussian part of a line is evaluated by the lanes whose points it can still change (|d| < dgi, K1's
// cut-off), two exp per lane and line, in a walk of its own over per-lane ranges counted the same way, so
// that all lanes are at the cores of their current lines at the same time.  Summation order per point:
// Lorentz terms of the partially covering lines, then of the fully covering ones, ascending; then the
// Gaussian terms, ascending: fixed, so reruns are bit-identical.
// Records per chunk: what fits beside the counters so that four workgroups share a CU's 160 KB of LDS.
template <int R> struct SkewChunk { static constexpr int value = R >= 8 ? 80 : 112; };

__device__ __forceinline__ unsigned int dpp_max_u32(unsigned int v, unsigned int moved) { return v > moved ? v : moved; }

// inclusive prefix maximum over the 64 lanes
__device__ __forceinline__ unsigned int wave_prefix_max_u32(unsigned int v) {
    v = dpp_max_u32(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = dpp_max_u32(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = dpp_max_u32(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = dpp_max_u32(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = dpp_max_u32(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = dpp_max_u32(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return v;
}

// cnt[i] = #{records of the chunk with centre < base + i}, i = 0 .. 64 R; returns this lane's counts at
// i = R lane (lo) and i = R lane + R - 1 (hi).  cnt holds j+1 of the last record whose first counted
// threshold is i (0: none) when called.
template <int R>
__device__ __forceinline__ void skew_counts(const unsigned int* __restrict__ cnt, int lane, int& lo, int& hi) {
    unsigned int m[R];
#pragma unroll
    for (int k = 0; k < R; ++k) m[k] = cnt[lane * R + k];
#pragma unroll
    for (int k = 1; k < R; ++k) m[k] = m[k] > m[k - 1] ? m[k] : m[k - 1];
    const unsigned int inc = wave_prefix_max_u32(m[R - 1]);
    unsigned int ex = (unsigned int)__shfl_up((int)inc, 1, 64);
    if (lane == 0) ex = 0u;
    lo = (int)(ex > m[0] ? ex : m[0]);
    hi = (int)inc;
}

__device__ __forceinline__ int wave_max_i32(int v) {        // v >= 0; the result is wave-uniform
    return __builtin_amdgcn_readlane((int)wave_prefix_max_u32((unsigned int)v), 63);
}

// One lane's Lorentz walk over the records [ja, ja + la) and then (TWO) [jb, jb + lb) of the chunk (per-lane
// bounds), into the running fraction.  The trip count is the longest walk of the wave (one DPP maximum); a
// lane that has finished reads the chunk's sentinel record (K = 0, centre at the span start so that its
// denominators stay small).  The loop is branch-free (a lane-dependent `if` around the loop-carried sums
// costs dozens of register copies per iteration), in blocks of at most `every` iterations between flushes
// of the running fraction; the next record's LDS read is issued before the current record's arithmetic.
// `it` counts the wave's iterations since the last flush, so every lane's product of denominators stays bounded.
template <int R, bool MASKED, bool TWO>
__device__ __forceinline__ void skew_lorentz(const double* __restrict__ lh, int sentinel, int ja, int la, int jb, int lb,
                                             double x0, double Hf, WaveAcc<R>& S, int& it) {
    typedef double v2f64 __attribute__((ext_vector_type(2)));
    const v2f64* rec = reinterpret_cast<const v2f64*>(lh);
    la = max(la, 0);
    const int len = la + (TWO ? max(lb, 0) : 0);
    const int T = wave_max_i32(len);
    const int jb_off = jb - la;
    auto index = [&](int t) {
        if (TWO) return t < la ? ja + t : (t < len ? jb_off + t : sentinel);
        return t < la ? ja + t : sentinel;
    };
    for (int t0 = 0; t0 < T;) {
        const int nb = min(S.every - it, T - t0);
        int jj = index(t0);
        v2f64 n0 = rec[jj * 2], n1 = rec[jj * 2 + 1];
#pragma unroll 2
        for (int t = 0; t < nb; ++t) {
            const v2f64 c0 = n0, c1 = n1;
            jj = index(t0 + t + 1);
            n0 = rec[jj * 2]; n1 = rec[jj * 2 + 1];
            const double d0 = x0 - c0.x;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const double d = d0 + (double)k;
                const double den = fma(d, d, c0.y);
                double K = c1.x;
                if (MASKED) K = (fabs(d) <= Hf) ? K : 0.0;
                const double tt = K * S.D[k];
                S.N[k] = fma(S.N[k], den, tt);
                S.D[k] *= den;
            }
        }
        it += nb;
        t0 += nb;
        if (it >= S.every) { S.flush(); it = 0; }
    }
}

// Edge lines of a span of the far-field kernel (support ends inside the span) through the skewed walk: the
// left-edge lines [iA, iB) and the right-edge lines [iC, iD) are staged side by side (64 + 64 records per
// round), every lane counts the ones that reach its R points - a lane near the left end of the span has
// many left-edge and few right-edge lines, a lane near the right end the opposite, the sum is the same for
// all lanes - and walks them in one unmasked loop (lines covering all its points) and one masked loop (the
// 0-2 lines that cover only some).  14 unmasked iterations for all lanes instead of 28 masked ones.
// Rounds with a record whose Gaussian part reaches the span, or whose denominator needs the plain divide,
// take the masked span path (accumulate_lines); K1's cut-off makes that rare for windows this wide.
// (Rounds that need the masked span path are only MARKED here - bit r of `odd` for round r < 64, everything from round 64
// on wholesale - and run afterwards through one accumulate_lines call site of the kernel (edge_rounds_masked): inlined into
// every edge routine the rare path cost them registers and the kernel a third of its code size.)
template <int R>
__device__ __forceinline__ void skew_edges(const HotRec* hot, const ColdRec* cold, int iA, int iB, int iC, int iD, int wlo,
                                           int whi, int H, double x0, double Hf, double* lh, double* lc,
                                           unsigned int* cntL, unsigned int* cntR, int lane, WaveAcc<R>& S, unsigned long long& odd) {
    typedef double v2f64 __attribute__((ext_vector_type(2)));
    typedef const v2f64 __attribute__((address_space(1)))* GlobalF64x2;
    const GlobalF64x2 gh = (GlobalF64x2)(unsigned long long)hot;
    constexpr int SENT = 128;                             // records 0..63: left-edge, 64..127: right-edge, 128: the sentinel
    auto slot = [&](int c, int base) { const int i = c - base + 1; return i < 0 ? 0 : (i > 64 * R + 1 ? 64 * R + 1 : i); };
    int round = 0;
    for (int cL = iA, cR = iC; (cL < iB || cR < iD) && round < 64; cL += 64, cR += 64, ++round) {
        const int nL = max(min(iB - cL, 64), 0), nR = max(min(iD - cR, 64), 0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < R; ++k) { cntL[lane * R + k] = 0u; cntR[lane * R + k] = 0u; }
        if (lane < 8) { cntL[64 * R + lane] = 0u; cntR[64 * R + lane] = 0u; }
        if (lane == 0) { lh[SENT * 4] = (double)wlo; lh[SENT * 4 + 1] = 1.0; lh[SENT * 4 + 2] = 0.0; lh[SENT * 4 + 3] = 0.0; }
        v2f64 l0 = {0, 1}, l1 = {0, 0}, r0 = {0, 1}, r1 = {0, 0};
        const bool vL = lane < nL, vR = lane < nR;
        if (vL) { const long long g = (long long)(cL + lane) * 2; l0 = gh[g]; l1 = gh[g + 1]; }
        if (vR) { const long long g = (long long)(cR + lane) * 2; r0 = gh[g]; r1 = gh[g + 1]; }
        const int ciL = (int)l0.x, ciR = (int)r0.x;
        // the walk adds Lorentz terms only: a record with a Gaussian part that reaches the span, or outside the
        // running-fraction range, sends this round through the masked span path
        const bool oddL = vL && (max(0, max(ciL - whi, wlo - ciL)) < __double2loint(l1.y) || (__double2hiint(l1.y) & REC_DIRECT_DIV));
        const bool oddR = vR && (max(0, max(ciR - whi, wlo - ciR)) < __double2loint(r1.y) || (__double2hiint(r1.y) & REC_DIRECT_DIV));
        if (__any(oddL || oddR)) { odd |= 1ull << round; continue; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (vL) {
            reinterpret_cast<v2f64*>(lh)[lane * 2] = l0;
            reinterpret_cast<v2f64*>(lh)[lane * 2 + 1] = l1;
            atomicMax(&cntL[slot(ciL, wlo - H)], (unsigned int)(lane + 1));              // A', A
        }
        if (vR) {
            reinterpret_cast<v2f64*>(lh)[(64 + lane) * 2] = r0;
            reinterpret_cast<v2f64*>(lh)[(64 + lane) * 2 + 1] = r1;
            atomicMax(&cntR[slot(ciR, wlo + H + 1)], (unsigned int)(lane + 1));          // B, B'
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int a_part, a_full, b_full, b_part;
        skew_counts<R>(cntL, lane, a_part, a_full);
        skew_counts<R>(cntR, lane, b_full, b_part);
        int it = S.cnt;
        // lines covering all of the lane's points: left-edge [a_full, nL), right-edge [0, b_full); then the partial ones
        skew_lorentz<R, false, true>(lh, SENT, a_full, nL - a_full, 64, b_full, x0, Hf, S, it);
        skew_lorentz<R, true, true>(lh, SENT, a_part, a_full - a_part, 64 + b_full, b_part - b_full, x0, Hf, S, it);
        S.cnt = it;
    }
}

// Round 5: the edge lines through the far-field series.  An edge line is 4-39 half-spans from the span centre, so over the
// points it covers its Lorentz term is the same smooth function the series of far_field_lines expands - but it covers only
// part of the span.  Left-edge lines are sorted by where their support ends, right-edge lines by where it starts: the lines
// that cover ALL R points of a lane are a SUFFIX of the left-edge list and a PREFIX of the right-edge list, at positions the
// threshold counts of the skewed walk already give (a_full, b_full).  So one lane takes one line, computes its series
// coefficients q_n (three instructions per term, as for a far line), a wave prefix sum over the lanes (left-edge lines loaded
// in reverse order, so that the prefix IS the suffix; all terms positive: no cancellation, fixed tree) turns q_n into "sum
// over the first j lines" for every j at once, and every lane picks the one partial sum that belongs to its points
// (ds_bpermute) and adds it to ITS coefficient C_n of the edge lines' polynomial, evaluated by Horner at its R points at
// the end.  ~52 instructions per term and 64 + 64 lines instead of 21 per line and lane: the 84 edge lines of a merged
// 100-2500 cm^-1 span cost ~900 wave-instructions instead of ~1,900 (14 % of the kernel, PMC).  The 0-2 lines per lane
// that cover only some of its points keep the masked walk; rounds with a Gaussian part that reaches the span or a
// denominator outside the running-fraction range keep the masked span path, as before.  Like the skewed walk it runs BEFORE
// the far lines' series phase, so that its NTE coefficients and that phase's NT are never live together.
// NTE terms: by the distance of the job's nearest edge line, H - 32 R points (FarTerms classes from FF_EDGE_MIN = 8 half-spans
// on: 20 terms there, 11 from 37 on, exact to half an ulp); nearer than 8 half-spans 30 terms would cost what the walk costs: the walk stays.
// inclusive prefix sum over the 64 lanes (lanes without a source add 0); fixed summation tree.  The two steps across rows
// fetch with full masks and are switched on per row by a factor (m15: 1.0 in rows 1 and 3, m31: 1.0 in rows 2 and 3, else
// 0.0; x * 1.0 is exact and the values are finite, so the sums are those of masked moves) - a DPP move under a partial row
// mask needs its destination preset, two more instructions per step.
__device__ __forceinline__ double wave_prefix_sum_f64(double v, double m15, double m31) {
    v += dpp_move_f64<0x111>(v);                // row_shr:1
    v += dpp_move_f64<0x112>(v);                // row_shr:2
    v += dpp_move_f64<0x114>(v);                // row_shr:4
    v += dpp_move_f64<0x118>(v);                // row_shr:8
    v = fma(dpp_move_f64<0x142>(v), m15, v);    // row_bcast:15 -> rows 1, 3
    v = fma(dpp_move_f64<0x143>(v), m31, v);    // row_bcast:31 -> rows 2, 3
    return v;
}

template <int R>
__device__ __forceinline__ void series_edges(const HotRec* hot, const ColdRec* cold, int iA, int iB, int iC, int iD, int wlo,
                                             int whi, int H, double x0, double Hf, double xc, int nte, double* lh, double* lc,
                                             unsigned int* cntL, unsigned int* cntR, int lane, WaveAcc<R>& S, unsigned long long& odd) {
    // Round 6: no coefficient array.  The polynomial of the edge lines is summed in ASCENDING powers as the terms come -
    // v_k += p_n tau_k^n with a running power per point - so a lane keeps 3 R doubles (tau, tau^n, v) instead of NTE
    // coefficients, both sides share one pass, and the term loop is a real loop with a run-time count (one body instead of
    // three unrolled instantiations).  |tau| < 1 and the p_n fall by at least 8x per term (edge lines are >= 8 half-spans
    // away), so the ascending sum is as accurate as Horner's.  With the coefficient array the kernel needed 162 VGPRs,
    // spilled 35 at its 128 and wrote the wave's sums to scratch in every round (round-5 verdict: 625 MB of stores on
    // the column where 250 MB are compulsory).
    double tau[R], v[R];
#pragma unroll
    for (int k = 0; k < R; ++k) { tau[k] = ((x0 + (double)k) - xc) * (1.0 / (32.0 * R)); v[k] = 0.0; }
    typedef double v2f64 __attribute__((ext_vector_type(2)));
    typedef const v2f64 __attribute__((address_space(1)))* GlobalF64x2;
    const GlobalF64x2 gh = (GlobalF64x2)(unsigned long long)hot;
    constexpr int SENT = 128;                             // records 0..63: left-edge, 64..127: right-edge, 128: the sentinel
    constexpr double hh = 32.0 * R;
    const double m15 = (lane & 16) ? 1.0 : 0.0, m31 = (lane & 32) ? 1.0 : 0.0;
    auto slot = [&](int c, int base) { const int i = c - base + 1; return i < 0 ? 0 : (i > 64 * R + 1 ? 64 * R + 1 : i); };
    int round = 0;
    for (int cL = iA, cR = iC; (cL < iB || cR < iD) && round < 64; cL += 64, cR += 64, ++round) {
        const int nL = max(min(iB - cL, 64), 0), nR = max(min(iD - cR, 64), 0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < R; ++k) { cntL[lane * R + k] = 0u; cntR[lane * R + k] = 0u; }
        if (lane < 8) { cntL[64 * R + lane] = 0u; cntR[64 * R + lane] = 0u; }
        if (lane == 0) { lh[SENT * 4] = (double)wlo; lh[SENT * 4 + 1] = 1.0; lh[SENT * 4 + 2] = 0.0; lh[SENT * 4 + 3] = 0.0; }
        v2f64 l0 = {0, 1}, l1 = {0, 0}, r0 = {0, 1}, r1 = {0, 0};
        const bool vL = lane < nL, vR = lane < nR;
        const int oL = nL - 1 - lane;                    // left-edge lines in REVERSE order over the lanes: prefix sums = suffix sums
        if (vL) { const long long g = (long long)(cL + oL) * 2; l0 = gh[g]; l1 = gh[g + 1]; }
        if (vR) { const long long g = (long long)(cR + lane) * 2; r0 = gh[g]; r1 = gh[g + 1]; }
        const int ciL = (int)l0.x, ciR = (int)r0.x;
        const bool oddL = vL && (max(0, max(ciL - whi, wlo - ciL)) < __double2loint(l1.y) || (__double2hiint(l1.y) & REC_DIRECT_DIV));
        const bool oddR = vR && (max(0, max(ciR - whi, wlo - ciR)) < __double2loint(r1.y) || (__double2hiint(r1.y) & REC_DIRECT_DIV));
        if (__any(oddL || oddR)) { odd |= 1ull << round; continue; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (vL) {
            reinterpret_cast<v2f64*>(lh)[oL * 2] = l0;
            reinterpret_cast<v2f64*>(lh)[oL * 2 + 1] = l1;
            atomicMax(&cntL[slot(ciL, wlo - H)], (unsigned int)(oL + 1));                // A', A
        }
        if (vR) {
            reinterpret_cast<v2f64*>(lh)[(64 + lane) * 2] = r0;
            reinterpret_cast<v2f64*>(lh)[(64 + lane) * 2 + 1] = r1;
            atomicMax(&cntR[slot(ciR, wlo + H + 1)], (unsigned int)(lane + 1));          // B, B'
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int a_part, a_full, b_full, b_part;
        skew_counts<R>(cntL, lane, a_part, a_full);
        skew_counts<R>(cntR, lane, b_full, b_part);
        // lines covering all of the lane's points: left-edge [a_full, nL) = the lanes 0 .. nL-1-a_full of the reversed
        // order, right-edge [0, b_full) = the lanes 0 .. b_full-1
        const int gL = nL - 1 - a_full, gR = b_full - 1;
        const double hasL = gL >= 0 ? 1.0 : 0.0, hasR = gR >= 0 ? 1.0 : 0.0;
        const int srcL = max(gL, 0), srcR = max(gR, 0);
        double alL, bpL, qaL, qbL, alR, bpR, qaR, qbR;
        auto start = [&](double cf, double a2, double K, double& al, double& bp, double& qa, double& qb) {
            const double dl = cf - xc, sq = fma(dl, dl, a2);
            double be = __builtin_amdgcn_rcp(sq);
            be = fma(fma(-sq, be, 1.0), be, be);
            be = fma(fma(-sq, be, 1.0), be, be);
            al = (dl * (2.0 * hh)) * be; bp = (hh * hh) * be;
            qa = K * be; qb = al * qa;
        };
        start(l0.x, l0.y, vL ? l1.x : 0.0, alL, bpL, qaL, qbL);
        start(r0.x, r0.y, vR ? r1.x : 0.0, alR, bpR, qaR, qbR);
        // sum over the lines that cover this lane's points, of term n of their series: the prefix sums of both sides,
        // each lane picking its own (left first, then right: fixed order)
        auto pick = [&](double qL, double qR) {
            const double pL = __shfl(wave_prefix_sum_f64(qL, m15, m31), srcL, 64);
            const double pR = __shfl(wave_prefix_sum_f64(qR, m15, m31), srcR, 64);
            return fma(pR, hasR, pL * hasL);
        };
        double pw[R];
        {
            const double p0 = pick(qaL, qaR), p1 = pick(qbL, qbR);
#pragma unroll
            for (int k = 0; k < R; ++k) { v[k] += p0; pw[k] = tau[k]; v[k] = fma(p1, pw[k], v[k]); }
        }
        // q_n = al q_(n-1) - bp q_(n-2) written over q_(n-2): two terms per trip, so that the pair (q_(n-2), q_(n-1)) never moves
        auto term = [&](double& oldL, double newestL, double& oldR, double newestR) {
            oldL = fma(alL, newestL, -(bpL * oldL));
            oldR = fma(alR, newestR, -(bpR * oldR));
            const double p = pick(oldL, oldR);
#pragma unroll
            for (int k = 0; k < R; ++k) { pw[k] *= tau[k]; v[k] = fma(p, pw[k], v[k]); }
        };
        int n = 2;
#pragma clang loop unroll(disable)
        for (; n + 1 < nte; n += 2) {
            term(qaL, qbL, qaR, qbR);
            term(qbL, qaL, qbR, qaR);
        }
        if (n < nte) term(qaL, qbL, qaR, qbR);
        // the 0-2 lines per lane that cover only some of its points: the masked walk, folded in at once
        int it = 0;
        skew_lorentz<R, true, true>(lh, SENT, a_part, a_full - a_part, 64 + b_full, b_part - b_full, x0, Hf, S, it);
        S.flush();
    }
#pragma unroll
    for (int k = 0; k < R; ++k) S.acc[k] += v[k];
}

// Fused sweep of a layer with ONE line list (lbl_layer_step_dev): the arithmetic and operation order of
// layer_sweep_kernel applied in the accumulate kernel's output stage, where the cross section of a point
// is in a register:  xs_m = 0 + cross section (pyradClasses.py:566-571), k = 0 + xs_m * conc * P / 1E4 /
// kB / T (pyradClasses.py:583, 707-712).  Layers with several line lists keep the separate sweep launch:
// both ways of folding them into this kernel were built and measured slower (DESIGN.md "what did not help":
// one workgroup walking all line lists of its points, -6 %; the last workgroup of a tile folding it, -3 %).
__device__ __forceinline__ void fused_fold(const FusedSweep& A, const AccumJob& J, double xsec, double& xs_m, double& kk) {
#pragma clang fp contract(off)
    if (J.chain_flags & CHAIN_MOL_FIRST) xs_m = 0.0;
    xs_m += xsec;
    if (J.chain_flags & CHAIN_MOL_LAST) kk += A.budget ? xs_m * A.factor : abs_coef_term(xs_m, J.conc, A.P, A.T, A.rT);
}

// after the last line list: transmittance and outgoing radiance of the point
// (pyradClasses.py:716, 784-787; pyradPlanck.py:38-44)
__device__ __forceinline__ void fused_finish(const FusedSweep& A, long long j, double kk) {
#pragma clang fp contract(off)
    if (A.abs_coef) A.abs_coef[j] = kk;
    const double tr = A.budget ? exp_neg_budget(kk * A.depth) : exp(-kk * A.depth);
    if (A.trans) A.trans[j] = tr;
    if (A.I_out) {
        const double nu = linspace_at(j, A.n, A.start, A.stop, A.step);
        const double B = A.budget ? planck_budget(nu, A.pa, A.pbkT) : planck_wn(nu, A.T, A.rT, A.pa, A.pb);
        const double Iin = A.I_in ? A.I_in[j] : (A.budget ? planck_budget(nu, A.pa, A.pbk_surface)
                                                          : planck_wn(nu, A.surface_T, A.r_surface_T, A.pa, A.pb));
        const double transmitted = tr * Iin;
        const double emitted = (1.0 - tr) * B;
        A.I_out[j] = transmitted + emitted;
    }
}

// What leaves an accumulate job for grid point j: the sum times the job's exact output scale (1.0 for a line list's cross
// section; 2^e for a merged layer job, whose records K1 weighted by conc P / 1E4 / k / T / 2^e: the absorption coefficient),
// stored if the job has an output array, and the sweep of the point when it is fused in.
__device__ __forceinline__ void output_point(const AccumJob& J, double* __restrict__ out, long long j, double sum) {
    const double t = sum * J.out_scale;
    if (out) out[j] = t;
    if (J.fuse.on == 2) {
        // merged layer job (lbl_layer_merged_step_dev): t is the layer's absorption coefficient (pyradClasses.py:707-712)
        fused_finish(J.fuse, j, t);
    } else if (J.fuse.on) {
        // a layer with ONE line list: the sweep of a point right here, its cross section is in a register
        double xs_m = 0.0, kk = 0.0;
        fused_fold(J.fuse, J, t, xs_m, kk);
        fused_finish(J.fuse, j, kk);
    }
}


// The edge rounds the skewed walk / the edge series left out (a record whose Gaussian part reaches the span or whose
// denominator needs the plain divide; everything beyond 64 rounds): the masked span path, one call site.
template <int R>
__device__ __forceinline__ void edge_rounds_masked(const HotRec* hot, const ColdRec* cold, int iA, int iB, int iC, int iD, int wlo,
                                                   int whi, double x0, double Hf, double* lh, double* lc, int lane, WaveAcc<R>& S,
                                                   unsigned long long odd) {
    double unused[16];                                 // (no 16-point Gaussian runs on this path: 4-point passes into the sums)
    while (odd) {
        const int r = __builtin_ctzll(odd);
        odd &= odd - 1;
        // (one call over [lo, hi): left- and right-edge records alike are "masked" records for accumulate_lines)
        for (int side = 0; side < 2; ++side) {
            const int lo = (side ? iC : iA) + 64 * r, end = side ? iD : iB;
            const int hi = min(lo + 64, end);
            if (lo < hi) accumulate_lines<R, 0>(hot, cold, lo, hi, iB, iC, wlo, whi, x0, Hf, lh, lc, lane, S, unused, 64, 1, 0);
        }
    }
    for (int side = 0; side < 2; ++side) {             // beyond 64 rounds of 64 lines per side: wholesale
        const int lo = (side ? iC : iA) + 64 * 64, end = side ? iD : iB;
        if (lo < end) accumulate_lines<R, 0>(hot, cold, lo, end, iB, iC, wlo, whi, x0, Hf, lh, lc, lane, S, unused, 64, 1, 0);
    }
}

// GRUN: points per lane of a Gaussian run (gauss_runs).  16: 128 VGPRs, four waves per SIMD.  32 (round 6; the production
// shape R = 4, LS = 1 with the series only): half the exp per point in the Gaussian parts for 32 more registers of sums -
// 164 VGPRs, three waves per SIMD, 43 KB of LDS per workgroup.  Same box, merged 100-2500 cm^-1 cell: K2 242.9 -> 233.1 us
// (-4 %), half of it (a shard of 2) -4 %, budget mode -3.5 %, the column's wide layers +-0; a launch that fits ONE round of
// the chip's 4,096 wave slots loses (a per-list shard of 8, 3,516 waves: 44.6 -> 46.4 us - it needs a second round at three
// waves per SIMD), so the host picks 32 for launches of more than 4,096 waves (lbl_set_option "accum_gauss_run").
template <int R, int LS, int NT = 0, int GRUN = 16>                                      // NT: far-field series terms (0: every pair direct)
__global__ __launch_bounds__((LS > 4 ? 64 * LS : 256), (R >= 4 ? (GRUN == 32 ? 3 : 4) : 1))   // HIP: min waves per SIMD
void xsec_accumulate_lds_kernel(const AccumJob* __restrict__ jobs, const int2* __restrict__ worklist) {
    constexpr bool FF = NT > 0;
    constexpr int NW = LS > 4 ? LS : 4;              // wavefronts per workgroup (LS = 8: 512 threads)
    constexpr int PG = NW / LS;                      // point groups (64*R points each) per workgroup
    // per wave: hot records [0,256), cold records [256,512); after the line loop the same words
    // hold the wave's 64*R sums in point order (+ padding) for the coalesced store
    static_assert(GRUN == 16 || (GRUN == 32 && FF && R == 4 && LS == 1), "32-point Gaussian runs: production shape of the far-field kernel only");
    constexpr int STAGE_MIN = GRUN == 32 ? 4 * 272 : FF ? 576 : 520;        // FF: 8 x 72 doubles for wave_sum_rows; else 512 + the 64-byte record list of gauss_runs; 32-point runs: four fold regions
    constexpr int STAGE = (68 * R > STAGE_MIN) ? 68 * R : STAGE_MIN;
    __shared__ double s_stage[NW][STAGE];
    // edge lines through the skewed walk (skew_edges): the production shape only (unsplit spans of 256 points)
    constexpr bool EDGE_SKEW = FF && LS == 1 && R == 4;
    __shared__ unsigned int s_ecnt[EDGE_SKEW ? NW : 1][2][EDGE_SKEW ? 64 * R + 8 : 1];

    // worklist: (job, tile) pairs of the whole launch sorted by decreasing line count (longest
    // first), built once per (line lists, grid) on the host; without it blockIdx.y is the job
    int job = blockIdx.y, tile;
    if (worklist) {
        const int2 wk = worklist[blockIdx.x];
        job = wk.x; tile = wk.y;
    } else {
        tile = xcd_tile(blockIdx.x, jobs[job].n_tiles, jobs[job].pad);
    }
    const AccumJob& J = jobs[job];
    const int lane = threadIdx.x & 63;
    const int wave = uniform_i32(threadIdx.x >> 6);
    const int grp = wave / LS, part = wave % LS;
    const int n_end = J.p_end;
    const long long wave_lo_ll = (long long)J.p_begin + (long long)(tile < 0 ? 0 : tile) * (64LL * R * PG) + (long long)grp * (64LL * R);
    const bool active = tile >= 0 && wave_lo_ll < n_end;
    if (LS == 1 && !active) return;                  // no workgroup barrier below when waves do not share points
    const int wlo = active ? (int)wave_lo_ll : 0;
    const int whi = active ? min(wlo + 64 * R - 1, n_end - 1) : 0;
    const int H = J.H;
    const int p0 = wlo + lane * R;
    const double x0 = (double)p0;
    const double Hf = (double)H;
    WaveAcc<R> S;
    S.init(J.flush_every);
    double* lh = s_stage[wave];
    double* lc = s_stage[wave] + 256;

    // line ranges of this span: tabulated by the host with the schedule, else searched here
    const int32_t* tab = nullptr;
    if (active && J.span_tab) tab = J.span_tab + (size_t)((wlo - J.p_begin) / (64 * R)) * 8;
    if (active && !FF) {
        int iA, iB, iC, iD;
        if (tab) { iA = uniform_i32(tab[0]); iB = uniform_i32(tab[1]); iC = uniform_i32(tab[2]); iD = uniform_i32(tab[3]); }
        else wave_line_ranges(J.cidx, J.n_lines, wlo, whi, H, lane, iA, iB, iC, iD);
        // this wave's share of the span's lines: every LS-th chunk of 64, starting at chunk `part`
        double G[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) G[k] = 0.0;
        accumulate_lines<R, 2>(J.hot, J.cold, iA + part * 64, iD, iB, iC, wlo, whi, x0, Hf, lh, lc, lane, S, G, 64 * LS);
        if (R == 4) gauss_runs_fold<R, 16>(G, s_stage[wave], lane, S.acc);
        S.flush();
    }
    if (active && FF) {
        // interior lines at least FF_FAR half-spans from the span centre go through the series; the
        // chunks of every class are dealt round-robin to the LS waves, each class starting at a
        // different wave so that the short classes do not all land on wave 0
        constexpr int FAR = FarThreshold<NT>::value;
        constexpr int NEAR = LorentzNear<NT>::value;          // the series takes the Lorentz terms from here on (< FAR: round 6)
        static_assert(NEAR == FAR || EDGE_SKEW, "the mid class needs the near walk that knows the Lorentz sub-range");
        const long long fl = (long long)wlo + 32 * R - 1 - (long long)FAR * 32 * R;
        const long long fr = (long long)wlo + 32 * R + (long long)FAR * 32 * R;
        const double xc = (double)wlo + (32.0 * R - 0.5);
        int iA, iB, iC, iD, iF1, iF2, iN1, iN2;
        if (tab) {           // wave-uniform values: keep them in scalar registers
            iA = uniform_i32(tab[0]); iB = uniform_i32(tab[1]); iC = uniform_i32(tab[2]); iD = uniform_i32(tab[3]);
            iF1 = uniform_i32(tab[4]); iF2 = uniform_i32(tab[5]);
            iN1 = NEAR < FAR ? uniform_i32(tab[6]) : iF1; iN2 = NEAR < FAR ? uniform_i32(tab[7]) : iF2;
        }
        else {
            wave_line_ranges_far(J.cidx, J.n_lines, wlo, whi, H, fl, fr, lane, iA, iB, iC, iD, iF1, iF2, iN1, iN2,
                                 (long long)wlo + 32 * R - 1 - (long long)FF_MID * 32 * R, (long long)wlo + 32 * R + (long long)FF_MID * 32 * R);
            if (!(NEAR < FAR)) { iN1 = iF1; iN2 = iF2; }
        }
        if (LBL_ABLATE(J, 8)) { iA = iB; iD = iC; }                       // (diagnostic builds, timing only: no edge lines)
        const bool any_far = !LBL_ABLATE(J, 256) && (iN1 - iB) + (iC - iN2) > 0;      // (256: far lines dropped)
        // edge lines first (skewed walk), while neither the series coefficients nor the Gaussian run sums are live
        // (also on spans without any far line - windows just above the kernel's limit, grid ends: their interior lines
        // are all near, [iF1, iF2) = [iB, iC))
        const bool edges_done = EDGE_SKEW;
#ifndef LBL_EDGE_SERIES
#define LBL_EDGE_SERIES 1
#endif
        constexpr bool EDGE_SERIES = EDGE_SKEW && LBL_EDGE_SERIES;       // (0: the skewed walk of round 3 everywhere, for A/B builds)
        if (edges_done) {
            unsigned int* eL = s_ecnt[EDGE_SKEW ? wave : 0][0];
            unsigned int* eR = s_ecnt[EDGE_SKEW ? wave : 0][1];
            // the job's nearest edge line is H - 32 R points from the span centre (wave-uniform: the job's window)
            typedef FarTerms<FF ? NT : FF_NT> FT;
            const int dmin = H - 32 * R;
            unsigned long long odd = 0ull;
            // a round of the series costs ~52 wave-instructions per term + ~250 whatever it holds, the walk ~21 per line: the
            // series from 40 (11 terms, windows of 37 half-spans and more) to 62 (20 terms, 8 half-spans) edge lines per span on (a merged 100-2500 cm^-1 span has 84, one of its line lists 28:
            // measured on the per-list step, series for everything: K2 +4.5 %)
            const int n_edge = (iB - iA) + (iD - iC);
            const int nte = FT::template edge_terms<R>(dmin);
            if (EDGE_SERIES && dmin >= FF_EDGE_MIN * 32 * R && n_edge * 21 >= 52 * nte + 250)
                series_edges<R>(J.hot, J.cold, iA, iB, iC, iD, wlo, whi, H, x0, Hf, xc, nte, lh, lc, eL, eR, lane, S, odd);
            else
                skew_edges<R>(J.hot, J.cold, iA, iB, iC, iD, wlo, whi, H, x0, Hf, lh, lc, eL, eR, lane, S, odd);
            if (odd || iB - iA > 64 * 64 || iD - iC > 64 * 64)
                edge_rounds_masked<R>(J.hot, J.cold, iA, iB, iC, iD, wlo, whi, x0, Hf, lh, lc, lane, S, odd);
        }
        int iG1 = iF1, iG2 = iF2;                  // the near walk's records (wave-uniform; wider than [iF1, iF2) on EDGE_SKEW only)
        if (any_far) {
            // the running fraction of the edge lines is folded in first: N = 0, D = 1 are then constants through the series
            // phase instead of 16 live registers beside its 60 of coefficients (28 instructions per span)
            S.flush();
            constexpr int NTC = FF ? NT : 2;               // (the array of the instantiations without the series is never touched)
            double C[NTC];
#pragma unroll
            for (int n = 0; n < NTC; ++n) C[n] = 0.0;
            // (EDGE_SKEW: the Gaussian parts of the far records inside FF_GAUSS_CAP half-spans belong to the near walk below;
            // the two calls widen [iG1, iG2) to hold them.  Line-split shapes keep them here: their waves are dealt whole far
            // chunks and would have to agree on the range across a workgroup barrier this kernel does not have at this point.)
            // the largest Gaussian cut-off of the record blocks that meet [iB, iC), once per span (one block per lane, a wave
            // maximum), as the distance in dmin2's units from which a far chunk skips its reach test (far_chunk)
            int reach_lim = INT_MAX;
            if (J.block_reach) {
                int r = 0;
                const int b1 = (iC - 1) >> 8;
                for (int b = iB >> 8; b <= b1; b += 64)
                    if (b + lane <= b1) r = max(r, J.block_reach[b + lane]);
                const int reach = wave_max_i32(r);
                if (reach < (1 << 29)) reach_lim = 2 * (reach + 32 * R) + 1;
            }
            far_field_lines<R, NTC, EDGE_SKEW>(J.hot, J.cold, iB + ((part + 1) % LS) * 64, iN1, 64 * LS, reach_lim, xc, wlo, whi, x0, Hf, lh, lc, lane, C, S, iG1, iG2);
            far_field_lines<R, NTC, EDGE_SKEW>(J.hot, J.cold, iN2 + ((part + 2) % LS) * 64, iC, 64 * LS, reach_lim, xc, wlo, whi, x0, Hf, lh, lc, lane, C, S, iG1, iG2);
            wave_sum_rows<NTC>(C, s_stage[wave], lane);
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const double tau = ((x0 + (double)k) - xc) * (1.0 / (32.0 * R));
                double v = C[NTC - 1];
#pragma unroll
                for (int n = NTC - 2; n >= 0; --n) v = fma(v, tau, C[n]);
                S.acc[k] += v;
            }
        }
        // the direct classes: left-edge, near and right-edge lines.  Without far lines (narrow window)
        // they are one contiguous run and go through the first stream alone (one prologue, not three).
        // (the LS waves of a span interleave these classes line by line; series chunks are dealt whole)
        // (Gaussian parts of interior lines: 16-point runs into G, folded into the sums once per span)
        double G[GRUN];
#pragma unroll
        for (int k = 0; k < GRUN; ++k) G[k] = 0.0;
        if (LBL_ABLATE(J, 512)) {                                            // (512: near lines dropped)
        } else if (edges_done) {
            // (Lorentz terms for [iN1, iN2), Gaussian runs for every record of [iG1, iG2) whose part reaches the span)
            accumulate_lines<R, 1, GRUN>(J.hot, J.cold, iG1, iG2, iB, iC, wlo, whi, x0, Hf, lh, lc, lane, S, G, 64, LS, part, iN1, iN2);
        } else {
            accumulate_lines<R, 1, GRUN>(J.hot, J.cold, iA, any_far ? iB : iD, iB, iC, wlo, whi, x0, Hf, lh, lc, lane, S, G, 64, LS, part);
            if (any_far) {
                accumulate_lines<R, 1, GRUN>(J.hot, J.cold, iF1, iF2, iB, iC, wlo, whi, x0, Hf, lh, lc, lane, S, G, 64, LS, part);
                accumulate_lines<R, 1, GRUN>(J.hot, J.cold, iC, iD, iB, iC, wlo, whi, x0, Hf, lh, lc, lane, S, G, 64, LS, part);
            }
        }
        if (R == 4) gauss_runs_fold<R, GRUN>(G, s_stage[wave], lane, S.acc);
        S.flush();
    }

    // Results leave through LDS so that every store instruction writes 512 contiguous bytes
    // (a lane owns R CONSECUTIVE points; storing them directly would touch 64 cache lines per
    // instruction).  With LS > 1 the LS partial sums of a span meet here in a fixed order.
    double* mine = s_stage[wave];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < R; ++k) mine[span_slot(lane * R + k)] = S.acc[k];
    if (LS > 1) __syncthreads();
    else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    if (active) {
        // the LS waves of a span share its output rows (and the fused sweep of their points); every
        // point is summed over the waves in the same order whichever wave stores it
        double* __restrict__ out = J.out;
        const int w0 = wave - part;                      // first wave of this span
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (LS > 1 && (i % LS) != part) continue;        // row i belongs to wave i % LS of the span
            const int o = i * 64 + lane;
            double t = s_stage[w0][span_slot(o)];
            for (int q = 1; q < LS; ++q) t += s_stage[w0 + q][span_slot(o)];
            if (wlo + o < n_end) output_point(J, out, wlo + o, t);
        }
    }
}

// One lane's walk over the records [g0, g1) whose Gaussian part may reach its R points (a per-lane range
// again, from the largest reach of the chunk; K1's own cut-off of every record decides inside): two exp per
// lane and line, all lanes at the cores of their current lines at the same time.  Branches are wave-uniform;
// a lane that does not need the term runs it with amplitude 0.  MASKED: points beyond the line's support are
// switched off (needed only when the largest reach of the chunk comes within R points of the support's end).
template <int R, bool MASKED>
__device__ __forceinline__ void skew_gauss(const double* __restrict__ lh, int cold_off, int sentinel, int g0, int g1,
                                           double x0, double Hf, WaveAcc<R>& S) {
    typedef double v2f64 __attribute__((ext_vector_type(2)));
    const v2f64* rec = reinterpret_cast<const v2f64*>(lh);
    const int len = max(g1 - g0, 0);
    const int T = wave_max_i32(len);
    for (int t = 0; t < T; ++t) {
        const int jc = t < len ? g0 + t : sentinel;
        const v2f64 h0 = rec[jc * 2];
        const double gf = lh[(jc * 2 + 1) * 2 + 1];
        const v2f64 gg = rec[cold_off + jc * 2];                     // KG, b
        const double q2 = lh[(cold_off + jc * 2 + 1) * 2];
        const double d0 = x0 - h0.x;
        const bool need = fabs(d0 + 0.5 * (R - 1)) < gf;           // the sentinel's reach is 0
        const bool recur = q2 >= 0.0 && R >= 4;
        const bool need_r = need && recur, need_n = need && !recur;
        if (__any(need_r))
            gauss_term<R, 1, MASKED>(need_r ? gg.x : 0.0, need_r ? gg.y : 0.0, true, d0, Hf, need_r ? q2 : 1.0, S.acc);
        if (__any(need_n))
            gauss_term<R, 0, MASKED>(need_n ? gg.x : 0.0, need_n ? gg.y : 0.0, false, d0, Hf, 0.0, S.acc);
    }
}

// LS (round 5): the LS waves of a workgroup share ONE span of 64 R points and take every LS-th record of its lines; their
// partial sums meet in LDS in a fixed order.  For the merged layer jobs: three times the lines per point make a chunk of
// records cover a third of the positions, less than the span is wide, so that only part of the lanes has lines in it and
// the walk runs as long as the busiest lane of every chunk (measured on the column's 17 narrow layers: merged 1.58 ms
// against 1.44 with one job per line list); dealt over 4 waves a chunk covers the whole span again.
template <int R, int LS = 1>
__global__ __launch_bounds__(256, 4) void xsec_accumulate_skew_kernel(const AccumJob* __restrict__ jobs,
                                                                   const int2* __restrict__ worklist) {
    static_assert(LS == 1 || LS == 2 || LS == 4, "line split of the skewed-range kernel");
    constexpr int PG = 4 / LS;                       // spans per workgroup
    constexpr int SKEW_CH = SkewChunk<R>::value;
    constexpr int NROUND = (SKEW_CH + 63) / 64;
    constexpr int NCNT = 64 * R + 8;                 // thresholds 0 .. 64 R, one dump slot, padding
    constexpr int COLD = (SKEW_CH + 1) * 2;           // first cold record, in 16-byte units
    __shared__ double s_rec[4][(SKEW_CH + 1) * 8];   // per wave: hot records 0 .. CH (CH: the sentinel), then the cold records 0 .. CH
    __shared__ unsigned int s_cnt[4][2][NCNT];
    int job = blockIdx.y, tile;
    if (worklist) {
        const int2 wk = worklist[blockIdx.x];
        job = wk.x; tile = wk.y;
    } else {
        tile = xcd_tile(blockIdx.x, jobs[job].n_tiles, jobs[job].pad);
    }
    const AccumJob& J = jobs[job];
    const int lane = threadIdx.x & 63;
    const int wave = uniform_i32(threadIdx.x >> 6);
    const int n_end = J.p_end;
    const int grp = wave / LS, part = wave % LS;
    const long long wave_lo_ll = (long long)J.p_begin + (long long)(tile < 0 ? 0 : tile) * (64LL * R * PG) + (long long)grp * (64LL * R);
    const bool active = tile >= 0 && wave_lo_ll < n_end;
    if (LS == 1 && !active) return;                  // waves are independent: no workgroup barrier below
    const int wlo = active ? (int)wave_lo_ll : 0;
    const int whi = active ? min(wlo + 64 * R - 1, n_end - 1) : 0;
    const int H = J.H;
    const int p0 = wlo + lane * R;
    const double x0 = (double)p0;
    const double Hf = (double)H;
    WaveAcc<R> S;
    S.init(J.flush_every);
    double* lh = s_rec[wave];
    double* lc = s_rec[wave] + COLD * 2;
    unsigned int* cntL = s_cnt[wave][0];
    unsigned int* cntR = s_cnt[wave][1];

    int iA = 0, iD = 0;
    if (!active) {
    } else if (J.span_tab) {
        const int32_t* tab = J.span_tab + (size_t)((wlo - J.p_begin) / (64 * R)) * 8;
        iA = uniform_i32(tab[0]); iD = uniform_i32(tab[3]);
    } else {
        int iB, iC;
        wave_line_ranges(J.cidx, J.n_lines, wlo, whi, H, lane, iA, iB, iC, iD);
    }
    // this wave's records: iA + part, iA + part + LS, ...
    const int n_mine = iD - iA > part ? (iD - iA - part + LS - 1) / LS : 0;
    auto record = [&](int s) { return (long long)(iA + part) + (long long)s * LS; };
    typedef double v2f64 __attribute__((ext_vector_type(2)));
    typedef const v2f64 __attribute__((address_space(1)))* GlobalF64x2;
    const GlobalF64x2 gh = (GlobalF64x2)(unsigned long long)J.hot;
    const GlobalF64x2 gc = (GlobalF64x2)(unsigned long long)J.cold;
    auto zero_counters = [&]() {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < R; ++k) { cntL[lane * R + k] = 0u; cntR[lane * R + k] = 0u; }
        if (lane < 8) { cntL[64 * R + lane] = 0u; cntR[64 * R + lane] = 0u; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    // every centre of [iA, iD) lies in [wlo - H, whi + H], so these differences fit an int
    auto slot = [&](int c, int base) { const int i = c - base + 1; return i < 0 ? 0 : (i > 64 * R + 1 ? 64 * R + 1 : i); };
    int it = 0;
    if (lane == 0) {                                      // the sentinel: centre at the span start, a2 = 1, K = 0, no Gaussian reach
        lh[SKEW_CH * 4] = (double)wlo; lh[SKEW_CH * 4 + 1] = 1.0; lh[SKEW_CH * 4 + 2] = 0.0; lh[SKEW_CH * 4 + 3] = 0.0;
        lc[SKEW_CH * 4] = 0.0; lc[SKEW_CH * 4 + 1] = 0.0; lc[SKEW_CH * 4 + 2] = 1.0; lc[SKEW_CH * 4 + 3] = 0.0;
    }
    for (int c0 = 0; c0 < n_mine; c0 += SKEW_CH) {
        const int n = min(SKEW_CH, n_mine - c0);
        zero_counters();
        unsigned long long dmask[NROUND];
        int cen[NROUND];
        bool live[NROUND];
        int reach = 0;
#pragma unroll
        for (int r = 0; r < NROUND; ++r) {
            dmask[r] = 0ull; cen[r] = 0; live[r] = false;
            if (r * 64 >= n) continue;                    // (wave-uniform)
            const int s = r * 64 + lane;
            const bool valid = s < n;
            v2f64 h0 = {0, 1}, h1 = {0, 0}, q0 = {0, 0}, q1 = {0, 0};
            if (valid) {
                const long long g = record(c0 + s) * 2;
                h0 = gh[g]; h1 = gh[g + 1];
                q0 = gc[g]; q1 = gc[g + 1];
            }
            const int dgi = valid ? __double2loint(h1.y) : 0, fl = __double2hiint(h1.y);
            const bool direct = valid && (fl & REC_DIRECT_DIV) != 0;
            dmask[r] = __ballot(direct);
            if (direct) { h0.y = 1.0; h1.x = 0.0; }                           // a2 = 1, KL = 0 in the walk's copy
            // Gaussian reach as a double: the term can matter for a lane whose R points come within dgi of the centre
            h1.y = dgi > 0 ? (double)dgi + 0.5 * (R - 1) : 0.0;
            reach = max(reach, dgi);
            live[r] = valid;
            cen[r] = (int)h0.x;
            if (valid) {
                reinterpret_cast<v2f64*>(lh)[s * 2] = h0;
                reinterpret_cast<v2f64*>(lh)[s * 2 + 1] = h1;
                reinterpret_cast<v2f64*>(lc)[s * 2] = q0;
                reinterpret_cast<v2f64*>(lc)[s * 2 + 1] = q1;
                // left family: base wlo - H (A', A); right family: base wlo + H + 1 (B, B')
                atomicMax(&cntL[slot(cen[r], wlo - H)], (unsigned int)(s + 1));
                atomicMax(&cntR[slot(cen[r], wlo + H + 1)], (unsigned int)(s + 1));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int a_part, a_full, b_full, b_part;
        skew_counts<R>(cntL, lane, a_part, a_full);
        skew_counts<R>(cntR, lane, b_full, b_part);
        if (a_full >= b_full) { a_full = b_part; b_full = b_part; }         // support narrower than the lane's R points: all masked
        // Gaussian ranges from the largest reach of the chunk: records with centre in [p0 - g, p0 + R-1 + g], g = reach - 1
        int g_lo = 0, g_hi = 0;
        const int gmax = wave_max_i32(reach);
        if (gmax > 0 && !LBL_ABLATE(J, 1)) {
            const int g = gmax - 1;
            zero_counters();
#pragma unroll
            for (int r = 0; r < NROUND; ++r) {
                if (live[r]) {
                    atomicMax(&cntL[slot(cen[r], wlo - g)], (unsigned int)(r * 64 + lane + 1));
                    atomicMax(&cntR[slot(cen[r], wlo + g + 1)], (unsigned int)(r * 64 + lane + 1));
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            int unused;
            skew_counts<R>(cntL, lane, g_lo, unused);
            skew_counts<R>(cntR, lane, unused, g_hi);
            g_lo = max(g_lo, a_part); g_hi = min(g_hi, b_part);             // only lines whose support reaches the lane's points
        }
        if (!LBL_ABLATE(J, 2)) skew_lorentz<R, true, true>(lh, SKEW_CH, a_part, a_full - a_part, b_full, b_part - b_full, x0, Hf, S, it);
        if (!LBL_ABLATE(J, 4)) skew_lorentz<R, false, false>(lh, SKEW_CH, a_full, b_full - a_full, 0, 0, x0, Hf, S, it);
        // a record within reach g of a lane's block has |d| <= g + R - 1 at every point of the lane
        if (gmax + R - 2 <= H) skew_gauss<R, false>(lh, COLD, SKEW_CH, g_lo, g_hi, x0, Hf, S);
        else skew_gauss<R, true>(lh, COLD, SKEW_CH, g_lo, g_hi, x0, Hf, S);
        // lines whose denominator is outside the running-fraction range (K1: REC_DIRECT_DIV): plain divide
#pragma unroll
        for (int r = 0; r < NROUND; ++r) {
            unsigned long long dm = dmask[r];
            while (dm) {
                const int s = r * 64 + __builtin_ctzll(dm);
                dm &= dm - 1;
                const double d0 = x0 - lh[s * 4];
                const double* c = lc + s * 4;
                const double a2 = 1.0 / c[1], KL = c[3];
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    const double d = d0 + (double)k;
                    const double t = KL / fma(d, d, a2);
                    S.acc[k] += (fabs(d) <= Hf) ? t : 0.0;
                }
            }
        }
    }
    S.flush();

    // results leave through LDS so that every store instruction writes 512 contiguous bytes; with LS > 1 the LS partial
    // sums of a span meet here, added in wave order whichever wave stores the row
    double* mine = s_rec[wave];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < R; ++k) mine[span_slot(lane * R + k)] = S.acc[k];
    if (LS > 1) __syncthreads();
    else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    if (!active) return;
    double* __restrict__ out = J.out;
    const int w0 = wave - part;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        if (LS > 1 && (i % LS) != part) continue;        // row i belongs to wave i % LS of the span
        const int o = i * 64 + lane;
        double t = s_rec[w0][span_slot(o)];
        for (int q = 1; q < LS; ++q) t += s_rec[w0 + q][span_slot(o)];
        if (wlo + o < n_end) output_point(J, out, wlo + o, t);
    }
}

// exclusive prefix sum of n counts into prefix[0..n] (single workgroup of 1024 threads)
static int scan_blocks(int n) { const int tiles = (n + 1023) / 1024; return tiles < 1 ? 1 : (tiles > 64 ? 64 : tiles); }

// Exclusive prefix sums of n counts, prefix[n] = the total.  Round 6: up to 64 workgroups instead of one (a single block spent
// 48-143 us on the 30,472 / 79,696 tile costs of a re-windowed column: 78 strided loads per thread, twice).  Block b owns a
// segment of whole 1024-element tiles; it first adds up everything BEFORE its segment (the whole block, coalesced - the last
// block reads the array once: 320 KB from L2), then scans its own tiles with a wave prefix + 16 wave totals.  No block waits
// for another.
__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}
__global__ __launch_bounds__(1024) void scan_counts_kernel(const unsigned int* __restrict__ counts, int n,
                                                           unsigned long long* __restrict__ prefix) {
    __shared__ unsigned long long s_wave[16];
    __shared__ unsigned long long s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tiles = (n + 1023) / 1024;
    const int tiles_per_block = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const long long lo = (long long)blockIdx.x * tiles_per_block * 1024;
    const long long hi = min(lo + (long long)tiles_per_block * 1024, (long long)n);
    if (n == 0) { if (blockIdx.x == 0 && t == 0) prefix[0] = 0ull; return; }
    if (lo >= n) return;
    unsigned long long s = 0;
    for (long long i = t; i < lo; i += 1024) s += counts[i];
    s = wave_incl_scan_u64(s, lane);
    if (lane == 63) s_wave[wave] = s;
    __syncthreads();
    if (t == 0) {
        unsigned long long b = 0;
        for (int w = 0; w < 16; ++w) b += s_wave[w];
        s_base = b;
    }
    __syncthreads();
    unsigned long long base = s_base;
    for (long long tile = lo; tile < hi; tile += 1024) {
        const long long i = tile + t;
        const unsigned long long v = i < hi ? (unsigned long long)counts[i] : 0ull;
        const unsigned long long incl = wave_incl_scan_u64(v, lane);
        __syncthreads();                                   // (s_wave of the previous tile has been read by everybody)
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (int w = 0; w < 16; ++w) { const unsigned long long x = s_wave[w]; if (w < wave) before += x; total += x; }
        if (i < hi) prefix[i] = base + before + incl - v;
        base += total;
    }
    if (hi == n && t == 0) prefix[n] = base;
}

// ----------------------------------------------------------------------------------------
// Schedule of a launch group, built on the device (time to first spectrum: a pressure or range change
// re-windows the layer, pyradClasses.py:734-752 -> resetData cls:45-56, and the next getter recomputes)
// ----------------------------------------------------------------------------------------
// What a launch group's accumulate kernels need besides the line records: for every span of 64 R points the six
// lower bounds of its edge / near / far lines in the sorted centre indices (one 32-byte row of the span table), and
// the dispatch order of its (job, tile) workgroups - longest first, XCD-partitioned when the launch has several
// rounds, bin-packed per CU when it has one (group_schedule in lbl_api.hip has the reasoning and the measurements).
// Until round 4 the host built both from its own evaluation of the centre indices: 4 ms for the 100-2500 cm^-1
// cell and 80 ms for the 30-layer column on one host thread, per re-windowing.  Here the bounds are searched in the
// very array K1 wrote (cidx), right after K1 in the same stream, and the order is sorted on the chip; nothing is
// copied back and the host never waits.  Dispatch order never changes a result; the span tables are the lower
// bounds of the same integers either way (tests/test_gpu_parity.py::test_device_schedule_*).
__global__ __launch_bounds__(256) void sched_spans_kernel(const SchedJob* __restrict__ jobs, int n_jobs, int total_spans, int R,
                                                          int spans_per_tile, long long far_reach, double cost_near,
                                                          double cost_edge, double cost_far, double cost_fixed,
                                                          int32_t* __restrict__ tabs, unsigned int* __restrict__ tile_cost,
                                                          int2* __restrict__ items) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;               // span of the group, job-major
    if (g >= total_spans) return;
    int k = 0;
    while (k + 1 < n_jobs && g >= jobs[k + 1].span_first) ++k;
    const SchedJob J = jobs[k];
    const int q = g - J.span_first;                                     // span of the job's shard
    const long long span = 64LL * R;
    const long long lo = (long long)J.p_begin + (long long)q * span;
    const long long hi = min(lo + span - 1, (long long)J.p_end - 1);
    const long long H = J.H;
    int iA = lower_bound_i32(J.cidx, J.n_lines, lo - H);
    int iB = lower_bound_i32(J.cidx, J.n_lines, hi - H);
    int iC = lower_bound_i32(J.cidx, J.n_lines, lo + H + 1);
    int iD = lower_bound_i32(J.cidx, J.n_lines, hi + H + 1);
    if (hi - H >= lo + H + 1) { iB = iD; iC = iD; }                     // span wider than the support: no interior line
    int iF1 = iB, iF2 = iC;
    if (far_reach > 0) {                                                // (same arithmetic as wave_line_ranges_far)
        iF1 = min(max(lower_bound_i32(J.cidx, J.n_lines, lo + 32 * R - far_reach), iB), iC);     // first line with c > fl
        iF2 = min(max(lower_bound_i32(J.cidx, J.n_lines, lo + 32 * R + far_reach), iF1), iC);    // first line with c >= fr
    }
    int iN1 = iF1, iN2 = iF2;                                           // the bounds at FF_MID half-spans, inside [iF1, iF2]
    if (far_reach > 0) {
        const long long mid_reach = (long long)FF_MID * 32 * R;
        iN1 = min(max(lower_bound_i32(J.cidx, J.n_lines, lo + 32 * R - mid_reach), iF1), iF2);
        iN2 = min(max(lower_bound_i32(J.cidx, J.n_lines, lo + 32 * R + mid_reach), iN1), iF2);
    }
    int32_t* e = tabs + ((size_t)J.span_first + (size_t)q) * 8;
    e[0] = iA; e[1] = iB; e[2] = iC; e[3] = iD; e[4] = iF1; e[5] = iF2; e[6] = iN1; e[7] = iN2;
    // wave-instructions of the span, as group_schedule prices them
    const double n_far = (double)((iF1 - iB) + (iC - iF2)), n_edge = (double)((iB - iA) + (iD - iC)), n_near = (double)(iF2 - iF1);
    const double c = n_near * cost_near + n_edge * cost_edge + n_far * cost_far + cost_fixed;
    const int tile = q / spans_per_tile;
    atomicAdd(&tile_cost[J.tile_first + tile], (unsigned int)(c + 0.5));          // integer adds: any order, same sum
    if (q % spans_per_tile == 0) { int2 it; it.x = k; it.y = tile; items[J.tile_first + tile] = it; }
}

// ascending bitonic sort of n (a power of two) 64-bit keys in LDS by the whole workgroup
__device__ __forceinline__ void bitonic_sort_lds(unsigned long long* keys, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            // one compare-exchange per thread and pass: pair p = (i, i | j) with bit j of i clear, so every lane works (walking
            // all i and skipping the upper partners left half of every wave idle: 0.59 ms for the 16,384 keys of an XCD's part
            // of the column's narrow layers)
            for (int p = threadIdx.x; p < (n >> 1); p += blockDim.x) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int l = i | j;
                const unsigned long long a = keys[i], b = keys[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { keys[i] = b; keys[l] = a; }
            }
        }
    }
    __syncthreads();
}

// key that sorts by decreasing cost, ties by increasing position (what std::stable_sort gives the host)
__device__ __forceinline__ unsigned long long sched_key(unsigned int cost, int pos) {
    return ((unsigned long long)(0xFFFFFFFFu - cost) << 32) | (unsigned int)pos;
}

// chunk (of `chunks` equal shares of the total cost, in positional order) that item i falls into
__device__ __forceinline__ int sched_chunk_of(const unsigned long long* __restrict__ prefix, int i, double share, int chunks) {
    const int c = (int)((double)prefix[i] / share);
    return c < chunks ? c : chunks - 1;
}

// Launches of several rounds: XCD-partitioned longest-first.  Workgroup i of the accumulate launch runs on XCD i mod 8
// and every XCD has its own L2: the positional tile sequence is cut into `chunks` (8 x 32) pieces of equal cost,
// piece c goes to part c mod 8, every part is sorted longest-first and the parts are interleaved - XCD x reads the
// records of part x only.
// Parts hold different numbers of items: up to the smallest part the interleave is strict (rank r of part x at slot
// 8 r + x); what the longer parts have left follows round by round over the parts that still have items (their
// cheapest tiles; the XCD alignment of that tail does not matter).
// Round 6: three kernels over the whole chip instead of one workgroup per part.  (1) sched_parts_kernel writes every part's keys,
// in positional order, to global scratch; (2) sched_tile_sort_kernel sorts every tile of 1,024 keys by itself; (3)
// sched_rank_xcd_kernel, one thread per key, adds up how many keys of the part's OTHER tiles sort before its own (a binary search
// per tile) - keys are unique (they end in the position), so own place + those counts IS the key's place in the sorted part -
// and writes its item straight to the dispatch list.  The 79,696 tiles of a re-windowed column's narrow layers took the bitonic
// sort in LDS (one workgroup per part, 16,384 keys, 105 passes) 0.36 ms.  Same order as that sort (and as std::stable_sort on
// the host).
__global__ __launch_bounds__(1024) void sched_parts_kernel(const unsigned long long* __restrict__ prefix,
                                                           const unsigned int* __restrict__ tile_cost, int N, int chunks,
                                                           unsigned long long* __restrict__ g_keys, int g_stride,
                                                           int* __restrict__ part_count) {
    __shared__ int s_start[8 * 64 + 1];               // first item of every chunk (chunks <= 512)
    const int x = blockIdx.x;
    const double share = (double)prefix[N] / (double)chunks + 1e-9;
    for (int c = threadIdx.x; c <= chunks; c += blockDim.x) {
        // first i in [0, N] whose chunk is >= c (chunk numbers do not decrease with i)
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sched_chunk_of(prefix, mid, share, chunks) < c) lo = mid + 1; else hi = mid;
        }
        s_start[c] = (c == chunks) ? N : lo;
    }
    __syncthreads();
    unsigned long long* keys = g_keys + (size_t)x * (size_t)g_stride;
    int off = 0;
    for (int c = x; c < chunks; c += 8) {
        const int a = s_start[c], b = s_start[c + 1];
        for (int i = a + (int)threadIdx.x; i < b; i += blockDim.x) keys[off + (i - a)] = sched_key(tile_cost[i], i);
        off += b - a;
    }
    if (threadIdx.x == 0) part_count[x] = off;
}

// (2) every tile of 1,024 keys of a part sorted by itself (bitonic, in LDS; the last tile padded with keys that sort last)
__global__ __launch_bounds__(256) void sched_tile_sort_kernel(unsigned long long* __restrict__ g_keys, int g_stride,
                                                              const int* __restrict__ part_count, int max_part) {
    __shared__ unsigned long long s_keys[1024];
    const int x = blockIdx.y;
    const int n_x = part_count[x];
    const int t0 = blockIdx.x * 1024;
    if (n_x > max_part || t0 >= n_x) return;                  // (whole workgroup)
    unsigned long long* keys = g_keys + (size_t)x * (size_t)g_stride + t0;
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) s_keys[i] = t0 + i < n_x ? keys[i] : ~0ull;
    bitonic_sort_lds(s_keys, 1024);
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) keys[i] = s_keys[i];
}

// (3) one thread per key: its place in its own sorted tile + the number of smaller keys in every other tile of the part (a
// binary search in the tile staged in LDS) is its place in the sorted part; the item goes straight to the dispatch list.
__global__ __launch_bounds__(1024) void sched_rank_xcd_kernel(const unsigned long long* __restrict__ g_keys, int g_stride,
                                                              const int* __restrict__ part_count, const int2* __restrict__ items,
                                                              int2* __restrict__ worklist, int max_part) {
    __shared__ unsigned long long s_tile[1024];
    const int x = blockIdx.y;
    const int n_x = part_count[x];
    const int t_mine = blockIdx.x;
    if (n_x > max_part || t_mine * 1024 >= n_x) return;         // (whole workgroup: no barrier is left behind; larger parts: the sort below)
    const unsigned long long* keys = g_keys + (size_t)x * (size_t)g_stride;
    const unsigned long long key = keys[t_mine * 1024 + threadIdx.x];           // (padding: ~0, sorted behind the tile's keys)
    int rank = threadIdx.x;
    const int n_tiles = (n_x + 1023) / 1024;
    for (int t = 0; t < n_tiles; ++t) {
        if (t == t_mine) continue;                            // (uniform over the workgroup)
        __syncthreads();
        s_tile[threadIdx.x] = keys[t * 1024 + threadIdx.x];
        __syncthreads();
        int lo = 0, hi = 1024;                                // first index whose key is not below mine (keys are unique): 0 .. 1024
        while (lo < hi) {                                     // (11 steps at most)
            const int mid = (lo + hi) >> 1;
            if (s_tile[mid] < key) lo = mid + 1; else hi = mid;
        }
        rank += lo;
    }
    if (key == ~0ull) return;
    int cnt[8], m = part_count[0];
#pragma unroll
    for (int y = 0; y < 8; ++y) { cnt[y] = part_count[y]; m = min(m, cnt[y]); }
    const int r = rank;
    const int src = (int)(unsigned int)(key & 0xFFFFFFFFull);
    long long pos;
    if (r < m) {
        pos = 8LL * r + x;
    } else {
        pos = 8LL * m;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            pos += max(0, min(cnt[y], r) - m);                     // full rounds m .. r-1
            if (y < x && cnt[y] > r) pos += 1;                      // parts ahead of x in round r
        }
    }
    worklist[pos] = items[src];
}

// Parts of more than kRankPartMax items (one part can hold most of a group's cheap tiles when a few tiles carry most of the
// cost; the build covers up to 2^20 tiles) are not ranked - quadratic - but sorted: one workgroup per such part, bitonic, in the
// dynamic LDS (cap keys, a power of two) or, beyond that, in the part's global scratch.  min_part: parts up to this size are
// left to the rank kernel (the two kernels write disjoint positions of the dispatch list).
constexpr int kRankPartMax = 32768;
__global__ __launch_bounds__(1024) void sched_order_xcd_kernel(const unsigned long long* __restrict__ prefix,
                                                               const unsigned int* __restrict__ tile_cost,
                                                               const int2* __restrict__ items, int N, int chunks, int cap,
                                                               unsigned long long* __restrict__ g_keys, int g_stride,
                                                               int2* __restrict__ worklist, int min_part) {
    extern __shared__ unsigned long long s_keys_lds[];
    __shared__ int s_start[8 * 64 + 1];               // first item of every chunk (chunks <= 512)
    __shared__ int s_count[8];
    const int x = blockIdx.x;
    const double share = (double)prefix[N] / (double)chunks + 1e-9;
    for (int c = threadIdx.x; c <= chunks; c += blockDim.x) {
        // first i in [0, N] whose chunk is >= c (chunk numbers do not decrease with i)
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sched_chunk_of(prefix, mid, share, chunks) < c) lo = mid + 1; else hi = mid;
        }
        s_start[c] = (c == chunks) ? N : lo;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        int n = 0;
        for (int c = threadIdx.x; c < chunks; c += 8) n += s_start[c + 1] - s_start[c];
        s_count[threadIdx.x] = n;
    }
    __syncthreads();
    const int n_x = s_count[x];
    if (n_x <= min_part) return;                      // (whole workgroup; the rank kernel places this part's items)
    int size = 1;
    while (size < n_x) size <<= 1;
    // a part that does not fit the LDS (one part can hold most of a group's cheap tiles when a few tiles carry most of
    // the cost) is sorted in global scratch instead: g_stride >= the next power of two of N keys per part; slow, rare
    unsigned long long* s_keys = size <= cap ? s_keys_lds : g_keys + (size_t)x * (size_t)g_stride;
    for (int i = threadIdx.x; i < size; i += blockDim.x) s_keys[i] = ~0ull;
    __syncthreads();
    int off = 0;
    for (int c = x; c < chunks; c += 8) {
        const int a = s_start[c], b = s_start[c + 1];
        for (int i = a + (int)threadIdx.x; i < b; i += blockDim.x) s_keys[off + (i - a)] = sched_key(tile_cost[i], i);
        off += b - a;
    }
    bitonic_sort_lds(s_keys, size);
    int m = s_count[0];
#pragma unroll
    for (int y = 1; y < 8; ++y) m = min(m, s_count[y]);
    for (int r = threadIdx.x; r < n_x; r += blockDim.x) {
        const int src = (int)(unsigned int)(s_keys[r] & 0xFFFFFFFFull);
        long long pos;
        if (r < m) {
            pos = 8LL * r + x;
        } else {
            pos = 8LL * m;
            for (int y = 0; y < 8; ++y) {
                pos += max(0, min(s_count[y], r) - m);                 // full rounds m .. r-1
                if (y < x && s_count[y] > r) pos += 1;                  // parts ahead of x in round r
            }
        }
        worklist[pos] = items[src];
    }
}

// minimum over the 64 lanes, the same value in every lane: four DPP butterfly steps inside the rows of 16 (always-valid
// sources), then the four row minima through scalar registers.  (The packing loop below runs this once per item: with
// __shfl_xor - six ds_bpermute round trips of ~100 cycles - it took 0.6 ms for 879 items, round 4.)
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_min_u64(unsigned long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned int)v, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned int)(v >> 32), CTRL, 0xf, 0xf, false);
    const unsigned long long o = ((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo;
    return o < v ? o : v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    v = dpp_min_u64<0xB1>(v);        // quad_perm [1,0,3,2]
    v = dpp_min_u64<0x4E>(v);        // quad_perm [2,3,0,1]
    v = dpp_min_u64<0x141>(v);       // row_half_mirror
    v = dpp_min_u64<0x140>(v);       // row_mirror: every lane of a row holds the row's minimum
    auto row = [&](int l) {
        return ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), l) << 32) |
               (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, l);
    };
    const unsigned long long a = row(0), b = row(16), c = row(32), d = row(48);
    const unsigned long long ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

template <int CTRL>
__device__ __forceinline__ unsigned int dpp_min_u32(unsigned int v) {
    const unsigned int o = (unsigned int)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, CTRL, 0xf, 0xf, false);
    return o < v ? o : v;
}
__device__ __forceinline__ unsigned int wave_min_u32(unsigned int v) {
    v = dpp_min_u32<0xB1>(v);
    v = dpp_min_u32<0x4E>(v);
    v = dpp_min_u32<0x141>(v);
    v = dpp_min_u32<0x140>(v);
    const unsigned int a = (unsigned int)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned int)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned int c = (unsigned int)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned int)__builtin_amdgcn_readlane((int)v, 48);
    const unsigned int ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// The packing loop of sched_order_pack_kernel, one wave: item k (longest first) to the least loaded bin with a free
// slot, lowest bin number on a tie.  Lane l owns bins l, 64 + l, ...; the two versions assign identically.
__device__ __forceinline__ void pack_bins_u64(const unsigned long long* s_keys, short* s_bin, short* s_tier, short* s_size,
                                              int N, int n_cu, int slots) {
    const int lane = threadIdx.x;
    unsigned long long load[8];
    int cnt[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) { load[b] = 0ull; cnt[b] = 0; }
    for (int k = 0; k < N; ++k) {
        const unsigned int cost = 0xFFFFFFFFu - (unsigned int)(s_keys[k] >> 32);
        unsigned long long best = ~0ull;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int bin = b * 64 + lane;
            const unsigned long long cand = (bin < n_cu && cnt[b] < slots) ? ((load[b] << 10) | (unsigned long long)bin) : ~0ull;
            best = cand < best ? cand : best;
        }
        best = wave_min_u64(best);
        const int bin = (int)(best & 1023ull);
        if ((bin & 63) == lane) {
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (b == (bin >> 6)) { s_tier[k] = (short)cnt[b]; load[b] += cost; cnt[b] += 1; }
            s_bin[k] = (short)bin;
        }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) if (b * 64 + lane < n_cu) s_size[b * 64 + lane] = (short)cnt[b];
}
// 32-bit keys (load << 12 | bin << 3 | items in the bin; all ones once the bin is full or absent): the wave minimum is
// then a scalar that names the bin, its lane, its tier and its load at once, so the winner's new key is scalar
// arithmetic and one select per register, and the (bin, tier) of item k0 + j is kept by lane j -
// no LDS and no divergent branch inside the loop.  While every load is zero, item k goes to bin k: the first n_cu
// items (of non-zero cost) are placed without the loop.
template <int NB>
__device__ __forceinline__ void pack_bins_u32(const unsigned long long* s_keys, short* s_bin, short* s_tier, short* s_size,
                                              int N, int n_cu, int slots) {
    const int lane = threadIdx.x;
    auto cost_of = [&](int k) { return k < N ? 0xFFFFFFFFu - (unsigned int)(s_keys[k] >> 32) : 0u; };
    const int first = N < n_cu ? N : n_cu;
    const bool seeded = cost_of(first - 1) > 0u;       // sorted longest-first: then all of the first tier are non-zero
    unsigned int key[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int bin = b * 64 + lane;
        key[b] = bin < n_cu ? (unsigned int)(bin << 3) : 0xFFFFFFFFu;
        if (seeded && bin < first) {
            key[b] = slots > 1 ? ((cost_of(bin) << 12) | (unsigned int)(bin << 3) | 1u) : 0xFFFFFFFFu;
            s_bin[bin] = (short)bin;
            s_tier[bin] = 0;
        }
    }
    for (int k0 = seeded ? first : 0; k0 < N; k0 += 64) {
        const int my_cost = (int)cost_of(k0 + lane);   // the costs of 64 items, one per lane
        const int n = N - k0 < 64 ? N - k0 : 64;
        int placed = 0;                                // lane j: (bin << 3 | tier) of item k0 + j
        for (int j = 0; j < n; ++j) {
            const unsigned int cost = (unsigned int)__builtin_amdgcn_readlane(my_cost, j);
            unsigned int best = key[0];
#pragma unroll
            for (int b = 1; b < NB; ++b) best = key[b] < best ? key[b] : best;
            best = wave_min_u32(best);                                 // uniform
            const int bin = (int)((best >> 3) & 511u), tier = (int)(best & 7u);
            const unsigned int next = tier + 1 < slots ? best + (cost << 12) + 1u : 0xFFFFFFFFu;
            const bool mine = (bin & 63) == lane;
#pragma unroll
            for (int b = 0; b < NB; ++b) key[b] = (mine && (bin >> 6) == b) ? next : key[b];
            placed = lane == j ? (int)(best & 4095u) : placed;
        }
        if (lane < n) { s_bin[k0 + lane] = (short)(placed >> 3); s_tier[k0 + lane] = (short)(placed & 7); }
    }
    // a bin's item count: what its key says, or `slots` once it is full
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if (b * 64 + lane < n_cu) s_size[b * 64 + lane] = (short)(key[b] == 0xFFFFFFFFu ? slots : (int)(key[b] & 7u));
}

// Launches of one round (every workgroup resident from the first cycle, nothing dispatched dynamically: the kernel
// lasts as long as the busiest CU): items sorted longest-first, each to the least loaded of the n_cu bins that still
// has a free slot, emitted bin-interleaved so that the dispatcher's round robin over the CUs rebuilds the bins.
// One workgroup of 256; N <= 1024 items, n_cu <= 512 bins (8 per lane of the packing wave).
__global__ __launch_bounds__(256) void sched_order_pack_kernel(const unsigned int* __restrict__ tile_cost,
                                                               const int2* __restrict__ items, int N, int n_cu,
                                                               int2* __restrict__ worklist) {
    __shared__ unsigned long long s_keys[1024];
    __shared__ short s_bin[1024], s_tier[1024];
    __shared__ short s_size[512];
    __shared__ int s_tier_off[8];
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) s_keys[i] = i < N ? sched_key(tile_cost[i], i) : ~0ull;
    bitonic_sort_lds(s_keys, 1024);
    const int slots = (N + n_cu - 1) / n_cu;           // <= 4 (N <= 4 n_cu)
    // A bin's load stays below slots * (largest cost): when that fits 20 bits the packing loop runs on 32-bit keys,
    // ~40 instructions per item instead of ~160 (64-bit compares and selects, LDS stores under a divergent branch).
    const unsigned int max_cost = 0xFFFFFFFFu - (unsigned int)(s_keys[0] >> 32);
    const bool narrow = N > 0 && slots <= 7 && (unsigned long long)max_cost * (unsigned int)slots < (1ull << 20);
    if (threadIdx.x < 64) {
        if (narrow && n_cu <= 256) pack_bins_u32<4>(s_keys, s_bin, s_tier, s_size, N, n_cu, slots);
        else if (narrow) pack_bins_u32<8>(s_keys, s_bin, s_tier, s_size, N, n_cu, slots);
        else pack_bins_u64(s_keys, s_bin, s_tier, s_size, N, n_cu, slots);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < slots && t < 8; ++t) {
            s_tier_off[t] = run;
            for (int b = 0; b < n_cu; ++b) run += s_size[b] > t ? 1 : 0;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        const int bin = s_bin[k], t = s_tier[k];
        int rank = 0;
        for (int b = 0; b < bin; ++b) rank += s_size[b] > t ? 1 : 0;
        worklist[s_tier_off[t] + rank] = items[(int)(unsigned int)(s_keys[k] & 0xFFFFFFFFull)];
    }
}

// Single-round launches, packed per XCD (round 5).  Workgroup p of a launch runs on XCD p % 8: XCD x packs ITS tiles
// longest-first into its own n_cu / 8 CUs (one wave per XCD, one bin per lane: the loop of pack_bins_u32) and emits them
// at the positions k 8 + x; eight waves in parallel, ~35 us where the one-wave packing of 879 items over all CUs took
// 0.14 ms (0.43 before its 32-bit keys, 0.60 in round 4).  Which tiles are an XCD's:
//   local 1: a CONTIGUOUS run of the tile sequence worth an eighth of the cost (midpoint rule on the cost prefix; `chunks`
//     / 8 runs per XCD): its L2 then holds its own records only - 5.3 MB fetched per launch instead of 14.8 on a
//     per-list shard of 8 (879 workgroups), 5.5 instead of 21 on a one-list 500-900 cm^-1 cell (782).  But every wave of a
//     single round starts at the same time and walks its records in step with its neighbours, and with neighbours that
//     are neighbours in the SPECTRUM all CUs of an XCD ask for the same lines of the same L2 channels at once.  Measured
//     against the mixed order, same box: launches whose waves each own a span (4 spans per workgroup) 391 workgroups
//     +-0, 588 +-0, 879 -1 %; launches whose spans are shared by 2 or 4 waves (which read the same records again) 782
//     workgroups +10 %, 586 (merged shard of 16) +17 %, a per-list shard of 16 +9 % (the order inside the XCD - tiers
//     closed up, one position per CU and tier, bins by fill - changed nothing; 2, 4 or 8 runs per XCD neither).  So: the
//     launches with unsplit spans (the caller's rule; "accum_xcd_pack" 2 / 3 force either).
//   local 0: every 8th tile of the longest-first order - each XCD a like sample of the whole spectrum, which is what
//     the one packing over all CUs (sched_order_pack_kernel) gave it.
// A local launch falls back to the mixed order inside this kernel when a run does not fit the `m_cap` positions the
// host reserved per XCD (costs piled up in a few tiles) or when the busiest CU of some XCD carries more than `tol`
// percent above the mean of the eight by the cost model (an XCD whose run holds the spectrum's expensive tiles cannot
// hand any to another XCD's CUs).  Positions without a tile hold (0, -1): workgroups that exit at once.
__global__ __launch_bounds__(512) void sched_order_pack_xcd_kernel(const unsigned int* __restrict__ tile_cost,
                                                                   const int2* __restrict__ items, int N, int n_cu, int m_cap,
                                                                   int local, int chunks, int tol, int2* __restrict__ worklist) {
    __shared__ unsigned long long s_keys[1024];
    __shared__ unsigned long long s_pref[1024];          // inclusive prefix of the costs, in tile order
    __shared__ unsigned long long s_scan[8];
    __shared__ int s_end[9], s_cnt[8], s_retry;
    __shared__ unsigned int s_make[8];
    __shared__ short s_xcd[1024];
    __shared__ short s_place[1024];                      // k-th item of XCD x (slot x * 128 + k ... see at()) -> bin << 3 | tier
    __shared__ short s_inv[8][7 * 64];                   // position of the XCD -> its k-th item, -1 idle
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = wave, B = n_cu >> 3;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const bool mixed = local == 0 || attempt == 1;
        if (!mixed) {
            // cost prefix: two items per thread, a wave scan, the eight wave totals
            const unsigned int c0 = 2 * tid < N ? tile_cost[2 * tid] : 0u, c1 = 2 * tid + 1 < N ? tile_cost[2 * tid + 1] : 0u;
            unsigned long long run = (unsigned long long)c0 + c1;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long o = __shfl_up(run, d);
                if (lane >= d) run += o;
            }
            if (lane == 63) s_scan[wave] = run;
            if (tid < 8) s_cnt[tid] = 0;
            __syncthreads();
            unsigned long long base = 0ull, total = 0ull;
#pragma unroll
            for (int w = 0; w < 8; ++w) { base += w < wave ? s_scan[w] : 0ull; total += s_scan[w]; }
            s_pref[2 * tid + 1] = base + run;
            s_pref[2 * tid] = base + run - c1;
            __syncthreads();
            // XCD of item i: the midpoint of its cost falls into one of `chunks` equal shares of the total; share c is XCD c % 8's
            for (int i = tid; i < N; i += blockDim.x) {
                const unsigned long long cost = (unsigned long long)tile_cost[i];
                const unsigned long long mid = 2ull * (s_pref[i] - cost) + cost;        // 2 x midpoint
                unsigned long long c = total ? mid * (unsigned long long)chunks / (2ull * total) : 0ull;
                c = c >= (unsigned long long)chunks ? (unsigned long long)chunks - 1ull : c;
                s_xcd[i] = (short)(c & 7ull);
                atomicAdd(&s_cnt[(int)(c & 7ull)], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int run_n = 0, worst = 0;
                for (int y = 0; y < 8; ++y) { s_end[y] = run_n; run_n += s_cnt[y]; worst = max(worst, s_cnt[y]); }
                s_end[8] = run_n;
                s_retry = worst > m_cap ? 1 : 0;
            }
            __syncthreads();
            if (s_retry) continue;                       // (uniform: every thread reads the same flag)
        }
        // one sort: (by XCD,) longest first, ties by position
        __syncthreads();
        for (int i = tid; i < 1024; i += blockDim.x) {
            unsigned long long key = ~0ull;
            if (i < N)
                key = ((unsigned long long)(mixed ? 0 : s_xcd[i]) << 42) | ((unsigned long long)(0xFFFFFFFFu - tile_cost[i]) << 10) | (unsigned long long)i;
            s_keys[i] = key;
        }
        bitonic_sort_lds(s_keys, 1024);
        // wave x packs its items - the sorted positions [s_end[x], s_end[x + 1]), or x, x + 8, ... - into its bins = lanes 0 .. B - 1
        const int first = mixed ? x : s_end[x], stride = mixed ? 8 : 1;
        const int n_x = mixed ? (N - x + 7) / 8 : s_end[x + 1] - s_end[x];
        auto at = [&](int k) { return first + k * stride; };
        const int slots = (n_x + B - 1) / B;             // <= 7 (sched_xcd_positions)
        auto cost_at = [&](int k) { return k < n_x ? 0xFFFFFFFFu - (unsigned int)((s_keys[at(k)] >> 10) & 0xFFFFFFFFull) : 0u; };
        // loads as 23-bit numbers: costs scaled down where slots x (largest cost) needs more (the order of nearly equal
        // loads is all that changes)
        int shift = 0;
        while (n_x > 0 && (((unsigned long long)cost_at(0) * (unsigned int)(slots > 0 ? slots : 1)) >> shift) >= (1ull << 23)) ++shift;
        const int seed_n = n_x < B ? n_x : B;
        const bool seeded = n_x > 0 && (cost_at(seed_n - 1) >> shift) > 0u;     // while every load is zero, item k goes to bin k
        unsigned int key = lane < B ? (unsigned int)(lane << 3) : 0xFFFFFFFFu;  // load << 9 | bin << 3 | items in the bin
        if (seeded && lane < seed_n) {
            key = slots > 1 ? (((cost_at(lane) >> shift) << 9) | (unsigned int)(lane << 3) | 1u) : 0xFFFFFFFFu;
            s_place[at(lane)] = (short)(lane << 3);
        }
        int full_cnt = (seeded && lane < seed_n && slots == 1) ? 1 : 0;         // what an all-ones key no longer says
        unsigned int my_load = (seeded && lane < seed_n) ? cost_at(lane) : 0u;  // the bin's load, unscaled
        for (int k0 = seeded ? seed_n : 0; k0 < n_x; k0 += 64) {
            const int my_raw = (int)cost_at(k0 + lane);
            const int my_cost = (int)((unsigned int)my_raw >> shift);
            const int n = n_x - k0 < 64 ? n_x - k0 : 64;
            int placed = 0;
            for (int j = 0; j < n; ++j) {
                const unsigned int cost = (unsigned int)__builtin_amdgcn_readlane(my_cost, j);
                const unsigned int raw = (unsigned int)__builtin_amdgcn_readlane(my_raw, j);
                const unsigned int best = wave_min_u32(key);
                const int bin = (int)((best >> 3) & 63u), tier = (int)(best & 7u);
                const bool last = tier + 1 >= slots;
                const unsigned int next = last ? 0xFFFFFFFFu : best + (cost << 9) + 1u;
                if (lane == bin) { key = next; full_cnt = last ? tier + 1 : 0; my_load += raw; }
                placed = lane == j ? (int)(best & 511u) : placed;
            }
            if (lane < n) s_place[at(k0 + lane)] = (short)placed;
        }
        if (!mixed) {
            unsigned int mk = my_load;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mk = max(mk, (unsigned int)__shfl_xor((int)mk, d));
            if (lane == 0) s_make[x] = mk;
            __syncthreads();
            unsigned long long sum = 0ull;
            unsigned int worst = 0u;
#pragma unroll
            for (int y = 0; y < 8; ++y) { sum += s_make[y]; worst = max(worst, s_make[y]); }
            if (tol >= 0 && (unsigned long long)worst * 800ull > sum * (unsigned long long)(100 + tol)) continue;   // (uniform)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int my_size = lane < B ? (key == 0xFFFFFFFFu ? full_cnt : (int)(key & 7u)) : 0;
        // tier by tier, closed up, the bins in bin order
        for (int k = lane; k < m_cap; k += 64) s_inv[x][k] = (short)-1;
        unsigned long long tier_mask[8];
        int tier_off[8];
        int off = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            tier_mask[t] = __ballot(my_size > t);
            tier_off[t] = off;
            off += __popcll(tier_mask[t]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < n_x; k += 64) {
            const int pl = s_place[at(k)], bin = pl >> 3, t = pl & 7;
            unsigned long long m = 0ull;
            int o = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) { m = u == t ? tier_mask[u] : m; o = u == t ? tier_off[u] : o; }
            s_inv[x][o + __popcll(m & ((1ull << bin) - 1ull))] = (short)k;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < m_cap; k += 64) {
            const int src = s_inv[x][k];
            worklist[(size_t)k * 8 + x] = src >= 0 ? items[(int)(s_keys[at(src)] & 1023ull)] : make_int2(0, -1);
        }
        return;
    }
}

// (sched_xcd_positions, sched_launch_items, sched_device_supported, sched_key_stride, sched_scratch_bytes: lbl_launch_shapes.h -
// pure host arithmetic shared with the sanitizer harness of the host shim)
void launch_schedule_build(const SchedJob* d_jobs, int n_jobs, int total_spans, int total_tiles, int R, int spans_per_tile,
                           long long far_reach, double cost_near, double cost_edge, double cost_far, double cost_fixed,
                           int n_cu, int32_t* tabs, void* scratch, int2* worklist, hipStream_t s, int xcd_chunks, bool xcd_pack,
                           int single_round_chunks, int xcd_tol, int xcd_local) {
    if (total_spans <= 0 || total_tiles <= 0) return;
    const size_t n = (size_t)total_tiles;
    char* base = (char*)scratch;
    unsigned int* tile_cost = (unsigned int*)base;                      base += (n * 4 + 255) & ~(size_t)255;
    int2* items = (int2*)base;                                          base += (n * 8 + 255) & ~(size_t)255;
    unsigned long long* prefix = (unsigned long long*)base;             base += ((n + 1) * 8 + 255) & ~(size_t)255;
    unsigned long long* g_keys = (unsigned long long*)base;
    (void)hipMemsetAsync(tile_cost, 0, (size_t)total_tiles * sizeof(unsigned int), s);
    hipLaunchKernelGGL(sched_spans_kernel, dim3((total_spans + 255) / 256), dim3(256), 0, s, d_jobs, n_jobs, total_spans, R,
                       spans_per_tile, far_reach, cost_near, cost_edge, cost_far, cost_fixed, tabs, tile_cost, items);
    if (total_tiles <= 4 * n_cu) {
        const int m_cap = xcd_pack ? sched_xcd_positions(total_tiles, n_cu) : 0;
        if (m_cap > 0) {
            // (runs per XCD: 1 by default.  A tile's records reach ~20 tiles to either side, so only runs much longer than that
            // keep an L2 to its own records: one run of ~50-110 tiles fetched 5.3-5.5 MB where 2 / 4 / 8 runs fetched 6.0 / 7.1 /
            // 9.2 and the packing over all CUs 14.8-21; the step times of 1, 2, 4 and 8 runs did not differ on the shards.)
            const int local = xcd_local == 1 || (xcd_local < 0 && spans_per_tile >= 4) ? 1 : 0;         // (auto: unsplit spans only)
            hipLaunchKernelGGL(sched_order_pack_xcd_kernel, dim3(1), dim3(512), 0, s, tile_cost, items, total_tiles, n_cu, m_cap,
                               local, 8 * single_round_chunks, xcd_tol, worklist);
        } else {
            hipLaunchKernelGGL(sched_order_pack_kernel, dim3(1), dim3(256), 0, s, tile_cost, items, total_tiles, n_cu, worklist);
        }
        return;
    }
    hipLaunchKernelGGL(scan_counts_kernel, dim3(scan_blocks(total_tiles)), dim3(1024), 0, s, tile_cost, total_tiles, prefix);
    // the parts' keys to global scratch, then one thread per key ranks it inside its part (see sched_rank_xcd_kernel)
    const int chunks = 8 * (xcd_chunks > 0 && xcd_chunks <= 64 ? xcd_chunks : 32);
    const int stride = sched_key_stride(total_tiles);
    int* part_count = reinterpret_cast<int*>(g_keys + (size_t)8 * (size_t)stride);         // (the scratch block's last 256 bytes)
    hipLaunchKernelGGL(sched_parts_kernel, dim3(8), dim3(1024), 0, s, prefix, tile_cost, total_tiles, chunks, g_keys, stride, part_count);
    const int part_tiles = (std::min(total_tiles, kRankPartMax) + 1023) / 1024;
    hipLaunchKernelGGL(sched_tile_sort_kernel, dim3(part_tiles, 8), dim3(256), 0, s, g_keys, stride, part_count, kRankPartMax);
    hipLaunchKernelGGL(sched_rank_xcd_kernel, dim3(part_tiles, 8), dim3(1024), 0, s, g_keys, stride, part_count, items, worklist, kRankPartMax);
    if (total_tiles > kRankPartMax) {
        // (a part of that size sorts in its own slice of the key scratch, which the rank kernel does not read for such a part)
        int cap = 16384;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(sched_order_xcd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                cap * (int)sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            cap = 4096;
        }
        hipLaunchKernelGGL(sched_order_xcd_kernel, dim3(8), dim3(1024), cap * sizeof(unsigned long long), s, prefix, tile_cost, items,
                           total_tiles, chunks, cap, g_keys, stride, worklist, kRankPartMax);
    }
}

// ----------------------------------------------------------------------------------------
// K2v: the true Voigt line shape (lbl_xsec_voigt_dev; beyond the reference)
// ----------------------------------------------------------------------------------------
// The reference's profile is a Gaussian below lhw / ghw = 0.01, a Lorentzian above 100 and a pseudo-Voigt between; K2v
// evaluates  A Re w((x + i lhw) / ghw) / (ghw sqrt(pi))  for every line instead, over the reference's scatter geometry
// (pyradClasses.py:390-400: centre point once, both wings for dx = 1 .. W - 2, points outside the grid dropped), as the
// same owner-computes gather as K2.  None of K2's records or kernels is touched: the prep kernel writes records of its own
// from line_physics(), the accumulate kernel streams them through wave-private LDS like variant 3 and evaluates every pair
// with voigt_k (lbl_voigt_func.h).  One fixed summation order per point (line order), no atomics.
__global__ __launch_bounds__(256) void voigt_prep_kernel(const PrepJob* __restrict__ jobs, const VoigtJob* __restrict__ vjobs) {
    const PrepJob& J = jobs[blockIdx.y];
    const VoigtJob& V = vjobs[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int regime = -1;
    if (i < J.n_lines) {
        const LinePhysics L = line_physics(J, i);
        long long idx = (long long)L.fidx;
        if (idx > 2000000000LL) idx = 2000000000LL;
        if (idx < -2000000000LL) idx = -2000000000LL;
        VoigtRec r;
        r.cf = (double)idx;
        r.xs = J.resolution / L.ghw;
        r.y = L.ratio;                                                // lhw / ghw (pyradClasses.py:378)
        r.amp = L.A * (1.0 / (L.ghw * 1.7724538509055159));           // sqrt(pi)
        V.rec[i] = r;
        V.cidx[i] = (int32_t)idx;
        regime = line_regime(L.ratio);                                // the counters keep the reference's meaning
    }
    __shared__ unsigned int s_cnt[4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < 3; ++k) {
        const unsigned long long m = __ballot(regime == k);
        if (lane == 0) s_cnt[wave][k] = (unsigned int)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < 3)
        J.block_counts[blockIdx.x * 3 + threadIdx.x] =
            s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
}

// A wave owns 64 kVoigtR consecutive points of its job's shard, finds the lines whose window meets them (wave_line_ranges:
// [iA, iD)) and walks them in chunks of kVoigtChunk records: lane l fetches record c0 + l with two 16-byte loads, parks it
// in the wave's 2 KB of LDS, and every record is read back as a broadcast (all lanes, one address).  Waves stay
// independent: no workgroup barrier.  Per pair: d = p - cf (exact), x = |d| xs, masked by |d| <= H.
__global__ __launch_bounds__(256) void voigt_accumulate_kernel(const VoigtJob* __restrict__ jobs) {
    constexpr int R = kVoigtR;
    const VoigtJob& J = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int wave = uniform_i32(threadIdx.x >> 6);
    const int n_end = J.p_end;
    const long long wave_lo_ll = (long long)J.p_begin + ((long long)blockIdx.x * 4 + wave) * (64LL * R);
    if (wave_lo_ll >= n_end) return;
    const int wlo = (int)wave_lo_ll;
    const int whi = min(wlo + 64 * R - 1, n_end - 1);
    const int H = J.H;
    int iA, iB, iC, iD;
    wave_line_ranges(J.cidx, J.n_lines, wlo, whi, H, lane, iA, iB, iC, iD);

    __shared__ double s_rec[4][kVoigtChunk * 4];
    double* lr = s_rec[wave];
    const int p0 = wlo + lane * R;
    const double x0 = (double)p0;
    const double Hf = (double)H;
    double acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = 0.0;
    for (int c0 = iA; c0 < iD; c0 += kVoigtChunk) {
        const int n = min(kVoigtChunk, iD - c0);
        __builtin_amdgcn_wave_barrier();                    // (every lane is done with the chunk before)
        if (lane < n) {
            const double2* src = reinterpret_cast<const double2*>(J.rec + c0 + lane);
            double2* dst = reinterpret_cast<double2*>(lr + lane * 4);
            dst[0] = src[0];
            dst[1] = src[1];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int j = 0; j < n; ++j) {
            const double cf = lr[j * 4], xs = lr[j * 4 + 1], y = lr[j * 4 + 2], amp = lr[j * 4 + 3];
            const double d0 = x0 - cf;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const double ad = fabs(d0 + (double)k);
                if (ad <= Hf) acc[k] += amp * voigt_k(ad * xs, y);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k)
        if (p0 + k < n_end) J.out[p0 + k] = acc[k];
}

// lbl_voigt_function_dev: the device function the accumulate kernel inlines, elementwise (tests)
__global__ __launch_bounds__(256) void voigt_function_kernel(const double* __restrict__ x, const double* __restrict__ y, long long n,
                                                             double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = voigt_k(x[i], y[i]);
}

// ----------------------------------------------------------------------------------------
// K2v-T: the temperature derivative of the true Voigt cross section (lbl_xsec_voigt_dt_dev)
// ----------------------------------------------------------------------------------------
// Under the Voigt shape a line's contribution  amp K(|d| xs, y)  is smooth in T, and the centre index, the window and the
// pressure shift do not depend on T, so the per-point sum is differentiated term by term:
//     d/dT [amp K(x, y)] = amp (a K + bx GX + by GY),   GX = x dK/dx, GY = y dK/dy (voigt_kgrad, lbl_voigt_func.h)
//     a  = d ln amp / dT = dlnw_dT + c2 E / T^2 - (c2 nu' / T^2) / expm1(c2 nu' / T) - 1 / (2 T)
//          (the caller's factor, e.g. -d ln Q / dT; Boltzmann; stimulated emission; the 1 / ghw of amp)
//     bx = d ln x / dT = -1 / (2 T)  (ghw ~ sqrt T),      by = d ln y / dT = -(n_air + 1/2) / T  (lhw ~ T^-n_air)
// The prep kernel writes K2v's four record fields, from the same expressions, and a, by beside them; it counts no regimes
// (lbl_last_regime_counts keeps describing the last value batch).
__global__ __launch_bounds__(256) void voigt_dT_prep_kernel(const PrepJob* __restrict__ jobs, const VoigtDTJob* __restrict__ vjobs) {
    const PrepJob& J = jobs[blockIdx.y];
    const VoigtDTJob& V = vjobs[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= J.n_lines) return;
    const LinePhysics L = line_physics(J, i);
    long long idx = (long long)L.fidx;
    if (idx > 2000000000LL) idx = 2000000000LL;
    if (idx < -2000000000LL) idx = -2000000000LL;
    VoigtDTRec r;
    r.cf = (double)idx;
    r.xs = J.resolution / L.ghw;
    r.y = L.ratio;
    r.amp = L.A * (1.0 / (L.ghw * 1.7724538509055159));           // sqrt(pi)
    const double c2 = cLight * hPlanck * 100.0 / kB;
    const double c2_T2 = c2 * J.inv_T * J.inv_T;
    const double u = c2 * L.broadened * J.inv_T;
    r.a = V.dlnw_dT + c2_T2 * J.elower[i] - c2_T2 * L.broadened / expm1(u) - 0.5 * J.inv_T;
    r.by = -(J.n_air[i] + 0.5) * J.inv_T;
    V.rec[i] = r;
    V.cidx[i] = (int32_t)idx;
}

// One pair added to a point's sum, every operation spelled out: the same inputs give the same bits whichever lane, point
// slot or shard evaluates them.
__device__ __forceinline__ double voigt_dT_add(double acc, double x, double y, double amp, double a, double bx, double by) {
#pragma clang fp contract(off)
    double K, GX, GY;
    voigt_kgrad(x, y, &K, &GX, &GY);
    return acc + amp * fma(a, K, fma(bx, GX, by * GY));
}

// K2v's geometry exactly (owner-computes, wave_line_ranges, wave-private LDS chunks read back as broadcasts, no workgroup
// barrier, no atomics, line order, |d| <= H, the centre point once); a record is 48 bytes: three 16-byte loads per lane,
// 3 KB of LDS per wave.
__global__ __launch_bounds__(256) void voigt_dT_accumulate_kernel(const VoigtDTJob* __restrict__ jobs) {
    constexpr int R = kVoigtR;
    const VoigtDTJob& J = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int wave = uniform_i32(threadIdx.x >> 6);
    const int n_end = J.p_end;
    const long long wave_lo_ll = (long long)J.p_begin + ((long long)blockIdx.x * 4 + wave) * (64LL * R);
    if (wave_lo_ll >= n_end) return;
    const int wlo = (int)wave_lo_ll;
    const int whi = min(wlo + 64 * R - 1, n_end - 1);
    const int H = J.H;
    int iA, iB, iC, iD;
    wave_line_ranges(J.cidx, J.n_lines, wlo, whi, H, lane, iA, iB, iC, iD);

    __shared__ double s_rec[4][kVoigtChunk * 6];
    double* lr = s_rec[wave];
    const int p0 = wlo + lane * R;
    const double x0 = (double)p0;
    const double Hf = (double)H;
    const double bx = J.bx;
    double acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = 0.0;
    for (int c0 = iA; c0 < iD; c0 += kVoigtChunk) {
        const int n = min(kVoigtChunk, iD - c0);
        __builtin_amdgcn_wave_barrier();                    // (every lane is done with the chunk before)
        if (lane < n) {
            const double2* src = reinterpret_cast<const double2*>(J.rec + c0 + lane);
            double2* dst = reinterpret_cast<double2*>(lr + lane * 6);
            dst[0] = src[0];
            dst[1] = src[1];
            dst[2] = src[2];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int j = 0; j < n; ++j) {
            const double cf = lr[j * 6], xs = lr[j * 6 + 1], y = lr[j * 6 + 2], amp = lr[j * 6 + 3];
            const double a = lr[j * 6 + 4], by = lr[j * 6 + 5];
            const double d0 = x0 - cf;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const double ad = fabs(d0 + (double)k);
                if (ad <= Hf) acc[k] = voigt_dT_add(acc[k], ad * xs, y, amp, a, bx, by);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k)
        if (p0 + k < n_end) J.out[p0 + k] = acc[k];
}

// lbl_voigt_gradient_dev: voigt_kgrad elementwise (tests)
__global__ __launch_bounds__(256) void voigt_gradient_kernel(const double* __restrict__ x, const double* __restrict__ y, long long n,
                                                             double* __restrict__ K, double* __restrict__ GX, double* __restrict__ GY) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        double k, gx, gy;
        voigt_kgrad(x[i], y[i], &k, &gx, &gy);
        K[i] = k; GX[i] = gx; GY[i] = gy;
    }
}

// ----------------------------------------------------------------------------------------
// K3: np.interp from linspace(min,max,n_work) onto linspace(min,max,n_base)
//     (pyradClasses.py:401-405, 159-162)
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void regrid_kernel(const double* __restrict__ work, long long n_work,
                                                     double* __restrict__ out, long long n_base,
                                                     double start, double stop, double step_w, double step_b) {
#pragma clang fp contract(off)
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_base) return;
    const double x = linspace_at(j, n_base, start, stop, step_b);
    double res;
    if (n_work == 1) {
        // np.interp with a single sample: x > xp[0] -> right, x < xp[0] -> left, equal -> fp[0]
        res = work[0];
    } else if (x > stop) {
        res = work[n_work - 1];
    } else if (x < start) {
        res = work[0];
    } else {
        long long i = (long long)((x - start) / step_w);
        if (i < 0) i = 0;
        if (i > n_work - 1) i = n_work - 1;
        while (i > 0 && linspace_at(i, n_work, start, stop, step_w) > x) --i;
        while (i < n_work - 1 && linspace_at(i + 1, n_work, start, stop, step_w) <= x) ++i;
        const double xi = linspace_at(i, n_work, start, stop, step_w);
        if (i == n_work - 1 || xi == x) {
            res = work[i];
        } else {
            const double xi1 = linspace_at(i + 1, n_work, start, stop, step_w);
            const double yi = work[i], yi1 = work[i + 1];
            const double slope = (yi1 - yi) / (xi1 - xi);
            res = slope * (x - xi) + yi;
            if (isnan(res)) {
                res = slope * (x - xi1) + yi1;
                if (isnan(res) && yi == yi1) res = yi;
            }
        }
    }
    out[j] = res;
}

// ----------------------------------------------------------------------------------------
// K4: fused layer sweep
// ----------------------------------------------------------------------------------------
// Cross sections are read in batches of NB independent loads (the term list is wave-uniform: pointers and
// flags come from the argument block by scalar loads; explicit global address space, so that a load does not
// wait for the scalar ones).  The first version walked molecules and isotopologues with dependent scalar
// loads and waited for every value before asking for the next: 0.52 of the HBM rate.
typedef const double __attribute__((address_space(1)))* GlobalF64;
__device__ __forceinline__ double load_global_f64(const double* p, long long j) {
    return ((GlobalF64)(unsigned long long)p)[j];
}

template <bool NT, int NP, bool BUDGET = false>
__global__ __launch_bounds__(256) void layer_sweep_kernel(const SweepArgs A) {
#pragma clang fp contract(off)
    // NP grid points per thread (2: 16-byte accesses; the host gives this instantiation an even first point and count)
    constexpr int NB = 4;
    typedef double vec __attribute__((ext_vector_type(NP)));
    auto ld = [&](const double* p, long long j) {
        vec v;
        if (NP == 1) v[0] = NT ? __builtin_nontemporal_load(p + j) : load_global_f64(p, j);
        else v = NT ? __builtin_nontemporal_load(reinterpret_cast<const vec*>(p + j)) : *reinterpret_cast<const vec*>(p + j);
        return v;
    };
    auto st = [&](double* p, long long j, vec v) {
        if (NP == 1) { if (NT) __builtin_nontemporal_store(v[0], p + j); else p[j] = v[0]; }
        else { if (NT) __builtin_nontemporal_store(v, reinterpret_cast<vec*>(p + j)); else *reinterpret_cast<vec*>(p + j) = v; }
    };
    const long long stride = (long long)gridDim.x * blockDim.x * NP;
    const long long jend = A.first + A.count;
    const int n_full = A.n_iso - A.n_iso % NB;
    for (long long j = A.first + ((long long)blockIdx.x * blockDim.x + threadIdx.x) * NP; j < jend; j += stride) {
        // Layer.absCoef (pyradClasses.py:707-712): zeros + sum over molecules of
        // Molecule.absCoef = crossSection * concentration * P / 1E4 / k / T (pyradClasses.py:583),
        // Molecule.crossSection = zeros + sum over isotopologues (pyradClasses.py:566-571)
        vec kk = (vec)(0.0), xs = (vec)(0.0);
        auto term = [&](int t, vec v) {
            xs += v;
            if (A.term_flags[t] & TERM_LAST_MOL) {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    kk[p] += BUDGET ? xs[p] * A.term_factor[t] : abs_coef_term(xs[p], A.term_conc[t], A.P, A.T, A.rT);
                    xs[p] = 0.0;
                }
            }
        };
        for (int t0 = 0; t0 < n_full; t0 += NB) {
            vec v[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) v[u] = ld(A.xsec[t0 + u], j);
#pragma unroll
            for (int u = 0; u < NB; ++u) term(t0 + u, v[u]);
        }
        {
            vec v[NB];
#pragma unroll
            for (int u = 0; u < NB - 1; ++u) v[u] = n_full + u < A.n_iso ? ld(A.xsec[n_full + u], j) : (vec)(0.0);
#pragma unroll
            for (int u = 0; u < NB - 1; ++u) if (n_full + u < A.n_iso) term(n_full + u, v[u]);
        }
        if (A.abs_coef) st(A.abs_coef, j, kk);
        vec tr;
#pragma unroll
        for (int p = 0; p < NP; ++p) tr[p] = BUDGET ? exp_neg_budget(kk[p] * A.depth) : exp(-kk[p] * A.depth);     // pyradClasses.py:716
        if (A.trans) st(A.trans, j, tr);
        if (A.I_out) {
            vec out;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double nu = linspace_at(j + p, A.n, A.start, A.stop, A.step);
                double B, Iin;
                if (BUDGET) {
                    B = planck_budget(nu, A.pa, A.pbkT);
                    Iin = A.I_in ? A.I_in[j + p] : planck_budget(nu, A.pa, A.pbk_surface);
                } else {
                    double pa_n, pb_n;
                    planck_point(nu, A.pa, A.pb, pa_n, pb_n);
                    B = planck_at(pa_n, pb_n, A.T, A.rT);                       // Layer.planck(self.T)
                    Iin = A.I_in ? A.I_in[j + p] : planck_at(pa_n, pb_n, A.surface_T, A.r_surface_T);
                }
                const double transmitted = tr[p] * Iin;                     // pyradClasses.py:785
                const double emitted = (1.0 - tr[p]) * B;                   // pyradClasses.py:786
                out[p] = transmitted + emitted;
            }
            st(A.I_out, j, out);
        }
    }
}

// ----------------------------------------------------------------------------------------
// K5: column fold (pyradClasses.py:784-787 applied layer after layer)
// ----------------------------------------------------------------------------------------
template <bool BUDGET>
__global__ __launch_bounds__(256) void column_sweep_kernel(const ColumnArgs* __restrict__ Ap) {
#pragma clang fp contract(off)
    const ColumnArgs& A = *Ap;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long jend = A.first + A.count;
    for (long long j = A.first + (long long)blockIdx.x * blockDim.x + threadIdx.x; j < jend; j += stride) {
        const double nu = linspace_at(j, A.n, A.start, A.stop, A.step);
        double I = A.I_in ? A.I_in[j] : (BUDGET ? planck_budget(nu, A.pa, A.pbk_surface)
                                                : planck_wn(nu, A.surface_T, A.r_surface_T, A.pa, A.pb));
        for (int l = 0; l < A.n_layers; ++l) {
            const double tr = A.trans[l][j];
            const double B = BUDGET ? planck_budget(nu, A.pa, A.pbkT[l]) : planck_wn(nu, A.layer_T[l], A.r_layer_T[l], A.pa, A.pb);
            const double transmitted = tr * I;
            const double emitted = (1.0 - tr) * B;
            I = transmitted + emitted;
        }
        A.I_out[j] = I;
    }
}

// K5b: column step straight from the cross sections.  For every grid point the layers are visited
// bottom to top: absorption coefficient and transmittance exactly as layer_sweep_kernel computes
// them, then the fold of column_sweep_kernel.  One pass over the cross sections replaces one sweep
// launch per layer plus the fold, and the per-layer arrays are written only if asked for.
// The column is a flat list of terms (one per cross-section array, bottom layer first; flags mark the last
// term of a molecule and of a layer).  NB terms are loaded at once, independent of one another; everything
// that depends on the grid point only (2E8 h c^2 n^3 and 100 h c n / k of pyradPlanck.py:41-42) is computed
// once per point, not once per layer.
// exp(x) for 0 <= x <= 1e-3 (the Planck exponent's growth over the 1-3 grid steps between a thread's points): degree-4
// Taylor polynomial, remainder x^5 / 120 <= 8.4e-18 relative
__device__ __forceinline__ double expm1_tiny(double x) {
    return x * fma(x, fma(x, fma(x, 1.0 / 24.0, 1.0 / 6.0), 0.5), 1.0);
}

// ---- the fold's budget arithmetic, shared by K5c and K5d --------------------------------------------------------------
// column_step_kernel (K5b, below) writes the same operations out itself: moved onto these helpers, its gfx950 code is no
// longer instruction for instruction what it is, and it is the fold that transmission() and the benchmark time.
// Default arithmetic with several points per thread: ONE exp per thread and layer for the Planck function (round 6).
// exp(nu_p c) = exp(nu_0 c) exp((nu_p - nu_0) c): the difference of two neighbouring grid wavenumbers is exact in fp64 and
// (nu_p - nu_0) c <= 1e-3 for every layer (checked here with the column's largest c = 100 h c / k / T_min), so the second
// factor is a degree-4 polynomial (7 instructions instead of the 17 of exp; 1-2 ulp).  Also only where no active lane of the
// wave can meet a special case - exponent above 700, exp(b) - 1 not positive (nu = 0), NaN wavenumbers - which keep the
// general expression with its selects and its IEEE division.  The result is wave-uniform.  (A: any argument block with the
// column's pbkT_min and pbkT_max, read only as far as the test gets)
template <int NP, class Args>
__device__ __forceinline__ bool fold_fast_path(const Args& A, const double (&nu)[NP], bool active) {
#pragma clang fp contract(off)
    const double dnu_last = nu[NP - 1] - nu[0];
    const bool plain = NP > 1 && nu[0] * A.pbkT_min >= 1e-6 && nu[NP - 1] * A.pbkT_max <= 690.0
                       && dnu_last * A.pbkT_max <= 1e-3 && dnu_last >= 0.0;
    return NP > 1 && __builtin_amdgcn_ballot_w64(active && !plain) == 0ull;
}

// B(nu, T) = pa_n / (exp(nu pbkT) - 1) with pa_n = pa nu^3, pbkT = 100 h c / k / T.  FAST: from the thread's single exp
// E0 = exp_clamped(nu0 pbkT) of its first point (`first`: nu is that point); else the general expression, planck_budget's
// value bit for bit.  DT: also dB/dT = B b e^b / ((e^b - 1) T) into *dB from the same exp (rT = 1 / T).
// (a NaN exponent must stay a NaN, as in np.exp(nan): fmin / fmax drop it, so it is put back explicitly)
template <bool FAST, bool DT = false>
__device__ __forceinline__ double fold_planck(bool first, double nu, double nu0, double pa_n, double pbkT, double E0,
                                              double rT = 0.0, double* dB = nullptr) {
#pragma clang fp contract(off)
    if (FAST) {
        const double E = first ? E0 : fma(E0, expm1_tiny((nu - nu0) * pbkT), E0);
        const double rc = rcp_newton(E - 1.0);
        const double B = pa_n * rc;
        if (DT) *dB = B * ((E * rc) * (nu * pbkT)) * rT;
        return B;
    }
    const double b = nu * pbkT;
    const double e = exp_clamped(fmin(b, 700.0)) - 1.0;
    if (!DT) {
        const double B = (b > 700.0) ? 0.0 : (e > 0.0 ? pa_n * rcp_newton(fmax(e, 1e-300)) : pa_n / e);
        return b != b ? b : B;
    }
    const double rc = rcp_newton(fmax(e, 1e-300));
    const double B = (b > 700.0) ? 0.0 : (e > 0.0 ? pa_n * rc : pa_n / e);
    *dB = b != b ? b : ((b > 700.0) ? 0.0 : (e > 0.0 ? B * (((e + 1.0) * rc) * b) * rT : B * (b * (e + 1.0) / e) * rT));
    return b != b ? b : B;
}

// I <- t I + (1 - t) B.  FAST: the last product and sum as one fma (three instructions instead of four).  (B + t (I - B)
// would be two, but loses I against B: with I < 1e-16 B behind a layer of optical depth ~1e-16 the result
// t I + (1 - t) B ~ I + 1e-16 B would come out as 1e-16 B alone.)
template <bool FAST>
__device__ __forceinline__ double fold_update(double tr, double I, double B) {
#pragma clang fp contract(off)
    if (FAST) return fma(tr, I, (1.0 - tr) * B);
    const double transmitted = tr * I;
    const double emitted = (1.0 - tr) * B;
    return transmitted + emitted;
}

// NP values of one array from grid point j on (16- / 32-byte loads for NP = 2 / 4; the caller's j is a multiple of NP)
template <int NP> using f64v = double __attribute__((ext_vector_type(NP)));
template <int NP>
__device__ __forceinline__ f64v<NP> load_points(const double* p, long long j) {
    typedef const f64v<NP> __attribute__((address_space(1)))* GlobalVec;
    f64v<NP> v;
    if (NP == 1) v[0] = load_global_f64(p, j);
    else v = *(GlobalVec)(unsigned long long)(p + j);
    return v;
}

// KFOLD (round 6): the fold over absorption coefficients (lbl_column_fold_dev, the column handle) - every term IS a layer, its
// factor 1: the per-molecule sums are skipped (0 + v = v, v * 1 = v: the same bits) and the flags are never read.
template <int NP, bool BUDGET = false, bool KFOLD = false>
__global__ __launch_bounds__(256, (NP == 4 ? 3 : 1)) void column_step_kernel(const ColumnStepArgs* __restrict__ Ap, long long first, long long count) {
#pragma clang fp contract(off)
    // NP grid points per thread (2: 16-byte loads, 4: 32-byte; the host gives these instantiations a first point and a count
    // that are multiples of NP)
    // terms per batch of loads (two batches in flight).  Four points per thread: 2 - the fold over absorption coefficients 128 VGPRs,
    // four waves per SIMD (135 us for the 30-layer column), the step from cross sections 138 / three
    constexpr int NB = NP == 4 ? 2 : 6;     // (the fold over absorption coefficients with 3: 158 VGPRs, three waves per SIMD, no faster; 4 spills)
    typedef double vec __attribute__((ext_vector_type(NP)));
    typedef const vec __attribute__((address_space(1)))* GlobalVec;
    const ColumnStepArgs& A = *Ap;
    const long long stride = (long long)gridDim.x * blockDim.x * NP;
    const long long jend = first + count;
    const int n_terms = A.n_terms;
    const int n_full = n_terms - n_terms % NB;
    const bool layer_arrays = A.layer_arrays != 0;          // (streaming / non-temporal loads measured 18 % SLOWER here: 536 vs 455 us)
    auto load = [&](const double* p, long long j) {
        vec v;
        if (NP == 1) v[0] = load_global_f64(p, j);
        else v = *(GlobalVec)(unsigned long long)(p + j);
        return v;
    };
    for (long long j = first + ((long long)blockIdx.x * blockDim.x + threadIdx.x) * NP; j < jend; j += stride) {
        double pa_n[NP], pb_n[NP], I[NP], kk[NP], xs[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double nu = linspace_at(j + p, A.n, A.start, A.stop, A.step);
            if (BUDGET) {
                pa_n[p] = A.pa * (nu * nu * nu); pb_n[p] = nu;           // (budget: the exponent is nu * term_pbkT)
                I[p] = A.I_in ? A.I_in[j + p] : planck_budget(nu, A.pa, A.pbk_surface);
            } else {
                planck_point(nu, A.pa, A.pb, pa_n[p], pb_n[p]);
                I[p] = A.I_in ? A.I_in[j + p] : planck_at(pa_n[p], pb_n[p], A.surface_T, A.r_surface_T);
            }
            kk[p] = 0.0; xs[p] = 0.0;
        }
        // Round 6, default arithmetic with several points per thread: ONE exp per thread and layer for the Planck function.
        // exp(nu_p c) = exp(nu_0 c) exp((nu_p - nu_0) c): the difference of two neighbouring grid wavenumbers is exact in
        // fp64 and (nu_p - nu_0) c <= 1e-3 for every layer (checked here with the column's largest c = 100 h c / k / T_min),
        // so the second factor is a degree-4 polynomial (7 instructions instead of the 17 of exp; 1-2 ulp).  Also only
        // where no lane of the wave can meet a special case - exponent above 700, exp(b) - 1 not positive (nu = 0), NaN
        // wavenumbers - which keep the general expression with its selects and its IEEE division (wave-uniform branch).
        const double dnu_last = BUDGET ? pb_n[NP - 1] - pb_n[0] : 0.0;
        const bool plain = BUDGET && NP > 1 && pb_n[0] * A.pbkT_min >= 1e-6 && pb_n[NP - 1] * A.pbkT_max <= 690.0
                           && dnu_last * A.pbkT_max <= 1e-3 && dnu_last >= 0.0;
        const bool fast = BUDGET && NP > 1 && __builtin_amdgcn_ballot_w64(!plain) == 0ull;
        int l = 0;
        // (arr_tag: std::true_type - per-layer arrays may be asked for, looked up per term; false_type - known to be absent: the
        //  wave-uniform test per point otherwise splits the four points' exponentials into separate basic blocks, round 6)
        auto term = [&](auto fast_tag, auto arr_tag, int t, vec v) {
            constexpr bool FAST = decltype(fast_tag)::value;
            constexpr bool ARRAYS = decltype(arr_tag)::value;
            const int f = KFOLD ? (TERM_LAST_MOL | TERM_LAST_LAYER) : A.term_flags[t];
            if (!KFOLD) {
#pragma unroll
                for (int p = 0; p < NP; ++p) xs[p] += v[p];
            }
            if (LBL_ABLATE(A, 16)) { I[0] += v[0]; return; }       // (diagnostic builds: memory traffic only)
            if (!KFOLD && (f & TERM_LAST_MOL)) {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    kk[p] += BUDGET ? xs[p] * A.term_factor[t] : abs_coef_term(xs[p], A.term_conc[t], A.term_P[t], A.term_T[t], A.term_rT[t]);
                    xs[p] = 0.0;
                }
            }
            if (f & TERM_LAST_LAYER) {
                double E0 = 0.0;
                if (FAST) E0 = exp_clamped(pb_n[0] * A.term_pbkT[t]);
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const double kp = KFOLD ? v[p] : kk[p];
                    const double tr = BUDGET ? exp_neg_budget(kp * A.term_depth[t]) : exp(-kp * A.term_depth[t]);
                    if (ARRAYS && layer_arrays) {
                        if (A.abs_coef[l]) A.abs_coef[l][j + p] = kp;
                        if (A.trans[l]) A.trans[l][j + p] = tr;
                    }
                    double B;
                    if (FAST) {
                        const double E = p == 0 ? E0 : fma(E0, expm1_tiny((pb_n[p] - pb_n[0]) * A.term_pbkT[t]), E0);
                        B = pa_n[p] * rcp_newton(E - 1.0);
                    } else if (BUDGET) {
                        const double b = pb_n[p] * A.term_pbkT[t];
                        const double e = exp_clamped(fmin(b, 700.0)) - 1.0;
                        B = (b > 700.0) ? 0.0 : (e > 0.0 ? pa_n[p] * rcp_newton(fmax(e, 1e-300)) : pa_n[p] / e);
                        B = b != b ? b : B;
                    } else {
                        B = planck_at(pa_n[p], pb_n[p], A.term_T[t], A.term_rT[t]);
                    }
                    if (FAST) {
                        // tr I + (1 - tr) B with the last product and sum as one fma (three instructions instead of four).
                        // (B + tr (I - B) would be two, but loses I against B: with I < 1e-16 B behind a layer of optical
                        // depth ~1e-16 the result tr I + (1 - tr) B ~ I + 1e-16 B would come out as 1e-16 B alone.)
                        I[p] = fma(tr, I[p], (1.0 - tr) * B);
                    } else {
                        const double transmitted = tr * I[p];
                        const double emitted = (1.0 - tr) * B;
                        I[p] = transmitted + emitted;
                    }
                    kk[p] = 0.0;
                }
                if (ARRAYS && layer_arrays) ++l;
            }
        };
        // two batches of NB loads in flight: the next batch is requested before the current one is consumed
        vec cur[NB], nxt[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) { cur[u] = (vec)(0.0); nxt[u] = (vec)(0.0); }
        if (n_full > 0) {
#pragma unroll
            for (int u = 0; u < NB; ++u) cur[u] = LBL_ABLATE(A, 32) ? (vec)(1e-22 * (double)(j & 7)) : load(A.xsec[u], j);
        }
        auto walk = [&](auto fast_tag, auto arr_tag) {
            for (int t0 = 0; t0 < n_full; t0 += NB) {
                if (t0 + NB < n_full) {
#pragma unroll
                    for (int u = 0; u < NB; ++u) nxt[u] = LBL_ABLATE(A, 32) ? (vec)(1e-22 * (double)(j & 7)) : load(A.xsec[t0 + NB + u], j);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) term(fast_tag, arr_tag, t0 + u, cur[u]);
#pragma unroll
                for (int u = 0; u < NB; ++u) cur[u] = nxt[u];
            }
            for (int t = n_full; t < n_terms; ++t) term(fast_tag, arr_tag, t, load(A.xsec[t], j));
        };
        if (BUDGET && NP > 1 && fast && !layer_arrays) walk(std::true_type{}, std::false_type{});
        else if (BUDGET && NP > 1 && fast) walk(std::true_type{}, std::true_type{});
        else walk(std::false_type{}, std::true_type{});
#pragma unroll
        for (int p = 0; p < NP; ++p) A.I_out[j + p] = I[p];
    }
}

__global__ __launch_bounds__(256) void planck_kernel(double* __restrict__ out, long long n, double start,
                                                     double stop, double step, double T, double rT, double pa, double pb) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = planck_wn(linspace_at(j, n, start, stop, step), T, rT, pa, pb);
}

// ----------------------------------------------------------------------------------------
// K6: band integral, sum(nan_to_num(y)) (pyradClasses.py:26-29); fixed reduction tree
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ double nan_to_num(double v) {
    if (isnan(v)) return 0.0;
    if (isinf(v)) return v > 0 ? 1.7976931348623157e308 : -1.7976931348623157e308;
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// every block sums a fixed, contiguous slice in a fixed order -> deterministic partials
__global__ __launch_bounds__(256) void band_partial_kernel(const double* __restrict__ y, long long n,
                                                           double* __restrict__ partial, long long per_block) {
    __shared__ double sh[4];
    const long long lo = (long long)blockIdx.x * per_block;
    const long long hi = min(lo + per_block, n);
    double s = 0.0;
    for (long long j = lo + threadIdx.x; j < hi; j += blockDim.x) s += nan_to_num(y[j]);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void band_final_kernel(const double* __restrict__ partial, int n_partial,
                                                         double* __restrict__ result) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int j = threadIdx.x; j < n_partial; j += blockDim.x) s += partial[j];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) result[0] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ----------------------------------------------------------------------------------------
// K5c / K5d: column transport (lbl_column_flux_dev, lbl_column_jacobian_dev; the semantics are in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// Both walk the fold of column_step_kernel<4, true, true> over the layers' absorption coefficients for NA angles at once:
// every thread owns NP grid points (NP on the aligned groups of a band, 1 on its head and tail points, the way
// launch_column_step_b treats its tail).  Per point and layer: one Planck term shared by all angles (fold_planck: one exp per
// thread and layer on the wave-uniform fast path, the general expression otherwise - the fold's guard and arithmetic), and
// one exp_neg_budget(tau_l / mu_k) per angle and direction.
// Sums: per thread (nan_to_num per point), wave_sum, lane 0 adds the result to its wave's slot in LDS; at the end the four
// waves' slots are added in a fixed order into ONE partial per workgroup and value, and column_flux_final_kernel adds the
// partials in a fixed order.  No float atomics: the same inputs and launch give the same bits.

// grid point j + p of the thread and the Planck numerator pa nu^3 there
template <int NP>
__device__ __forceinline__ void column_points(const ColumnRT& A, long long j, double (&nu)[NP], double (&pa_n)[NP]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        nu[p] = linspace_at(j + p, A.n, A.start, A.stop, A.step);
        pa_n[p] = A.pa * (nu[p] * nu[p] * nu[p]);
    }
}

// One step of the fold for the thread's NP points, shared by K5c (a layer) and K5e (a path segment through a layer): the
// Planck term of every point (fold_planck: from ONE exp per thread on the fast path), then update(p, k_p, B_p), which forms
// the optical depths from the absorption coefficient k_p = v[p] and folds them into the caller's radiances.
template <bool FAST, int NP, class Update>
__device__ __forceinline__ void transport_step(const double (&nu)[NP], const double (&pa_n)[NP], double pbkT, f64v<NP> v,
                                               Update update) {
#pragma clang fp contract(off)
    double E0 = 0.0;
    if (FAST) E0 = exp_clamped(nu[0] * pbkT);
#pragma unroll
    for (int p = 0; p < NP; ++p) update(p, v[p], fold_planck<FAST>(p == 0, nu[p], nu[0], pa_n[p], pbkT, E0));
}

// sum_k W_k v(k), angle 0 first
template <int NA, class V>
__device__ __forceinline__ double angle_sum(const ColumnRT& A, V v) {
#pragma clang fp contract(off)
    double f = A.w[0] * v(0);
#pragma unroll
    for (int k = 1; k < NA; ++k) f = fma(A.w[k], v(k), f);
    return f;
}

// One step of K5i's linear source for the thread's NP points: transport_step with two Planck values, Ba where the light
// enters (pbkT_a) and Bb where it leaves (pbkT_b); update(p, k_p, Ba_p, Bb_p - Ba_p).
template <bool FAST, int NP, class Update>
__device__ __forceinline__ void linear_step(const double (&nu)[NP], const double (&pa_n)[NP], double pbkT_a, double pbkT_b,
                                            f64v<NP> v, Update update) {
#pragma clang fp contract(off)
    double Ea0 = 0.0, Eb0 = 0.0;
    if (FAST) {
        Ea0 = exp_clamped(nu[0] * pbkT_a);
        Eb0 = exp_clamped(nu[0] * pbkT_b);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const double Ba = fold_planck<FAST>(p == 0, nu[p], nu[0], pa_n[p], pbkT_a, Ea0);
        const double Bb = fold_planck<FAST>(p == 0, nu[p], nu[0], pa_n[p], pbkT_b, Eb0);
        update(p, v[p], Ba, Bb - Ba);
    }
}

// K5i: I <- t I + (1 - t) Ba + g(tau) dB, t = tr = exp_neg_budget(tau)
template <bool FAST>
__device__ __forceinline__ double linear_update(double tau, double tr, double I, double Ba, double dB) {
#pragma clang fp contract(off)
    const double isothermal = fold_update<FAST>(tr, I, Ba);
    const double slope = linear_source_g(tau, tr) * dB;
    return isothermal + slope;
}

// The band frame: what the kernels that sum a band into Jacobian or level slots share (K5d, K5h, K5j, K5k).  The
// [wave][slot] block `acc` in LDS (declared by the kernel, kSlot doubles per wave) is zeroed; a grid-stride loop hands every
// thread NP points j .. j + NP - 1 of the two runs [lo0, lo0 + n0) and [lo1, lo1 + n1) and calls walk(fast_tag, j, active, nu,
// pa_n, add) for them; at the end the four waves' slots are added in a fixed order into the workgroup's partial of nv values.
// What makes the kernels on it right is stated here, once:
//   - the loop bound is uniform over the workgroup, and an idle lane (active == false) works on a valid point, lo0, so that
//     every lane takes part in the wave reductions; a walk adds 0 for it and stores nothing;
//   - add(slot, s) is wave_sum and then lane 0 adding to its wave's slot: no atomics, one order, the same bits every run;
//   - the one-exp Planck path (fast_tag = std::true_type) is taken by a whole wave or not at all (fold_fast_path) and only
//     with several points per thread: a band's head and tail points go to the <1, ...> instantiation, general expression.
// The flux kernels of K5c, K5g and K5i keep this loop in their own bodies: registers ("Two frames carry ...").
// PLANCK = false (K5k, which has no source term) leaves out the wavenumbers, the Planck numerators and the dispatch: nu and
// pa_n are then not set, and the walk gets std::false_type.
// (threads: blockDim.x, read by the __global__ kernel itself.  Read in a device function it is not folded to the launch's
// uniform workgroup size: it stays a load and a select on the workgroup's index, in a vector register.)
template <int NP, int kSlot, bool PLANCK = true, class Args, class Walk>
__device__ __forceinline__ void band_frame(const Args& A, unsigned threads, long long lo0, long long n0, long long lo1,
                                           long long n1, double* __restrict__ partial, double* acc, int nv, Walk walk) {
#pragma clang fp contract(off)
    for (int t = threadIdx.x; t < 4 * kSlot; t += threads) acc[t] = 0.0;
    __syncthreads();
    double* my = acc + (threadIdx.x >> 6) * kSlot;
    const bool lane0 = (threadIdx.x & 63) == 0;
    auto add = [&](int slot, double s) {
        s = wave_sum(s);
        if (lane0) my[slot] += s;
    };
    const long long total = n0 + n1;
    const long long stride = (long long)gridDim.x * threads * NP;
    for (long long q0 = (long long)blockIdx.x * threads * NP; q0 < total; q0 += stride) {
        const long long q = q0 + (long long)threadIdx.x * NP;
        const bool active = q < total;
        const long long j = !active ? lo0 : (q < n0 ? lo0 + q : lo1 + (q - n0));
        double nu[NP], pa_n[NP];
        if constexpr (PLANCK) {
            column_points<NP>(A, j, nu, pa_n);
            const bool fast = fold_fast_path<NP>(A, nu, active);
            if constexpr (NP > 1) {
                if (fast) walk(std::true_type{}, j, active, nu, pa_n, add);
                else walk(std::false_type{}, j, active, nu, pa_n, add);
            } else {
                walk(std::false_type{}, j, active, nu, pa_n, add);
            }
        } else {
            walk(std::false_type{}, j, active, nu, pa_n, add);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nv; t += threads)
        partial[(long long)blockIdx.x * nv + t] = (acc[t] + acc[kSlot + t]) + (acc[2 * kSlot + t] + acc[3 * kSlot + t]);
}

// The layer walks of the column kernels: step(l, k) for the layers bottom to top (column_up) or top to bottom (column_down),
// k the thread's NP absorption coefficients of layer l, loaded one layer ahead of their use.  For the column Jacobian
// kernels (K5d, K5h, K5j); the flux and solar kernels write the same loop out: on these two their code changes, and
// surface_flux_kernel<4, 7> goes to scratch ("One step body ...").
template <int NP, class Args, class Step>
__device__ __forceinline__ void column_up(const Args& A, long long j, int L, Step step) {
    typedef f64v<NP> vec;
    vec cur = L > 0 ? load_points<NP>(A.abs_coef[0], j) : (vec)(0.0);
    for (int l = 0; l < L; ++l) {
        const vec nxt = l + 1 < L ? load_points<NP>(A.abs_coef[l + 1], j) : cur;
        step(l, cur);
        cur = nxt;
    }
}
template <int NP, class Args, class Step>
__device__ __forceinline__ void column_down(const Args& A, long long j, int L, Step step) {
    typedef f64v<NP> vec;
    vec cur = L > 0 ? load_points<NP>(A.abs_coef[L - 1], j) : (vec)(0.0);
    for (int l = L - 1; l >= 0; --l) {
        const vec nxt = l > 0 ? load_points<NP>(A.abs_coef[l - 1], j) : cur;
        step(l, cur);
        cur = nxt;
    }
}

// K5c: walks the layers bottom to top for the upward radiances I_up[k] and then top to bottom for the downward ones,
// re-reading k_l and recomputing B_l on the way down (the registers cannot hold 128 layers' worth).  With the angle set
// {(1, pi)} the upward radiance at the top is the fold's I_out bit for bit wherever both take the same Planck path (every
// wave fast, or the same general points).  Level sums: after every layer step each thread adds its points' sum_k W_k I_k.
template <int NP, int NA>
__global__ __launch_bounds__(256) void column_flux_kernel(const FluxArgs* __restrict__ Ap, long long lo0, long long n0,
                                                          long long lo1, long long n1, double* __restrict__ partial) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    constexpr int kSlot = 2 * (kMaxLayers + 1);
    __shared__ double acc[4 * kSlot];            // [wave][up levels 0..L, down levels 0..L]
    const FluxArgs& A = *Ap;
    const int L = A.n_layers;
    const int nv = 2 * (L + 1);
    for (int t = threadIdx.x; t < 4 * kSlot; t += blockDim.x) acc[t] = 0.0;
    __syncthreads();
    double* my = acc + (threadIdx.x >> 6) * kSlot;
    const bool lane0 = (threadIdx.x & 63) == 0;
    const long long total = n0 + n1;
    const long long stride = (long long)gridDim.x * blockDim.x * NP;
    // (the loop bound is uniform over the workgroup: every lane takes part in the wave reductions, idle lanes on a valid point)
    for (long long q0 = (long long)blockIdx.x * blockDim.x * NP; q0 < total; q0 += stride) {
        const long long q = q0 + (long long)threadIdx.x * NP;
        const bool active = q < total;
        const long long j = !active ? lo0 : (q < n0 ? lo0 + q : lo1 + (q - n0));
        double nu[NP], pa_n[NP], I[NA][NP];
        column_points<NP>(A, j, nu, pa_n);
        const bool fast = fold_fast_path<NP>(A, nu, active);
        // sum_k W_k I_k per point, nan_to_num, summed over the thread's points, the wave, and into the wave's slot
        auto level = [&](int slot, double* spec) {
            double s = 0.0;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double f = angle_sum<NA>(A, [&](int k) { return I[k][p]; });
                if (spec && active) spec[j + p] = f;
                s += active ? nan_to_num(f) : 0.0;
            }
            s = wave_sum(s);
            if (lane0) my[slot] += s;
        };
        auto layer = [&](auto fast_tag, int l, vec v) {
            constexpr bool FAST = decltype(fast_tag)::value;
            const double depth = A.depth[l];
            transport_step<FAST, NP>(nu, pa_n, A.pbkT[l], v, [&](int p, double kp, double B) {
                const double tau = kp * depth;
#pragma unroll
                for (int k = 0; k < NA; ++k) I[k][p] = fold_update<FAST>(exp_neg_budget(tau * A.rmu[k]), I[k][p], B);
            });
        };
        auto walk = [&](auto fast_tag) {
            // upward: I_0 = I_surface or B(nu, surface_T); level l + 1 after layer l
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double Is = A.I_surface ? A.I_surface[j + p] : planck_budget(nu[p], A.pa, A.pbk_surface);
#pragma unroll
                for (int k = 0; k < NA; ++k) I[k][p] = Is;
            }
            level(0, L == 0 ? A.up_top : nullptr);
            vec cur = L > 0 ? load_points<NP>(A.abs_coef[0], j) : (vec)(0.0);
            for (int l = 0; l < L; ++l) {
                const vec nxt = l + 1 < L ? load_points<NP>(A.abs_coef[l + 1], j) : cur;
                layer(fast_tag, l, cur);
                level(l + 1, l + 1 == L ? A.up_top : nullptr);
                cur = nxt;
            }
            // downward: I_L = I_top or 0; level l after layer l
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double It = A.I_top ? A.I_top[j + p] : 0.0;
#pragma unroll
                for (int k = 0; k < NA; ++k) I[k][p] = It;
            }
            level(L + 1 + L, L == 0 ? A.down_surface : nullptr);
            cur = L > 0 ? load_points<NP>(A.abs_coef[L - 1], j) : (vec)(0.0);
            for (int l = L - 1; l >= 0; --l) {
                const vec nxt = l > 0 ? load_points<NP>(A.abs_coef[l - 1], j) : cur;
                layer(fast_tag, l, cur);
                level(L + 1 + l, l == 0 ? A.down_surface : nullptr);
                cur = nxt;
            }
        };
        if constexpr (NP > 1) {
            if (fast) walk(std::true_type{});
            else walk(std::false_type{});
        } else {
            walk(std::false_type{});
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nv; t += blockDim.x)
        partial[(long long)blockIdx.x * nv + t] = (acc[t] + acc[kSlot + t]) + (acc[2 * kSlot + t] + acc[3 * kSlot + t]);
}

// level_flux[t] = sum over the partials of value t, in the order of band_final_kernel (one workgroup per value)
__global__ __launch_bounds__(256) void column_flux_final_kernel(const double* __restrict__ partial, int n_partial, int nv,
                                                                double* __restrict__ level_flux) {
    __shared__ double sh[4];
    const int t = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < n_partial; b += blockDim.x) s += partial[(long long)b * nv + t];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) level_flux[t] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// The ray frame: what five of the six ray kernels (K5e - K5j) share; K5f's ray_jacobian_kernel keeps the same set-up and loops
// in its own body (it measures slower on the frame: DESIGN.md, "Two frames carry ...").
// A thread owns NP grid points from j on and a workgroup one bundle of RB rays with one layer sequence; the frame finds
// both, forms what every ray kernel needs per point and per ray, and walks the bundle's segments for the kernel, which supplies only its start values, what happens at a surface marker and
// its step through a real segment.  Stated here, once:
//   - the idle lanes of the last workgroup (active == false) work on a valid point, lo0, and store nothing: the Planck path
//     is chosen per wave (fold_fast_path), so every lane has to have a point;
//   - ray, segment and layer indices are uniform over the workgroup, so the tables behind the argument block and the layer
//     scalars come through scalar loads, and the branch on a marker is uniform too (the rays of a bundle share their layer
//     sequence, markers included);
//   - k_l is loaded one REAL segment ahead of its use, past the markers;
//   - head and tail points go to the <1, 1, ...> instantiation and its general Planck expression (dispatch).
// MARKERS = false (K5e: no surface in the path) leaves out the emissivity, the marker branch and the search for the
// next real segment.
template <int NP, int RB, bool MARKERS, class Args>
struct RayFrame {
    typedef f64v<NP> vec;
    const Args& A;
    const char* blk;                    // the argument block: A, and behind it the tables at A.off_*
    long long j;                        // the thread's first grid point
    bool active, fast;
    double nu[NP], pa_n[NP], Is[NP];    // per point: column_points and the surface's source
    double em[NP];                      //   and the surface's emissivity: set only with MARKERS, not to be read without
    int rid[RB], s0[RB];                // per ray of the bundle: its index and its first segment
    bool surface[RB];                   //   and whether it starts at the surface (source kind 1)
    int ns;                             // segments, markers included (the same for every ray of the bundle, as are its
    const int32_t* __restrict__ lay;    //   layers, lay[0 .. ns), and its rows)
    const double* __restrict__ seg_length;

    // (threads: blockDim.x, read by the __global__ kernel itself, as for band_frame)
    __device__ __forceinline__ RayFrame(const Args* Ap, unsigned threads, long long lo0, long long n0, long long lo1,
                                        long long n1, int order_first) : A(*Ap), blk((const char*)Ap) {
#pragma clang fp contract(off)
        const int32_t* __restrict__ ray_first = (const int32_t*)(blk + A.off_ray_first);
        const int32_t* __restrict__ source_kind = (const int32_t*)(blk + A.off_source_kind);
        const int32_t* __restrict__ order = (const int32_t*)(blk + A.off_order);
        seg_length = (const double*)(blk + A.off_seg_length);
        const long long q = ((long long)blockIdx.x * threads + threadIdx.x) * NP;
        active = q < n0 + n1;
        j = !active ? lo0 : (q < n0 ? lo0 + q : lo1 + (q - n0));
        column_points<NP>(A, j, nu, pa_n);
        fast = fold_fast_path<NP>(A, nu, active);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            Is[p] = A.I_surface ? A.I_surface[j + p] : planck_budget(nu[p], A.pa, A.pbk_surface);
            if constexpr (MARKERS) em[p] = A.emissivity ? A.emissivity[j + p] : A.emissivity_all;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            rid[i] = order[order_first + (int)blockIdx.y * RB + i];
            s0[i] = ray_first[rid[i]];
            surface[i] = source_kind[rid[i]] == 1;
        }
        ns = ray_first[rid[0] + 1] - s0[0];
        lay = (const int32_t*)(blk + A.off_seg_layer) + s0[0];
    }

    // walk(fast_tag): the one-exp Planck path for a wave that may take it, the general expression otherwise
    template <class Walk>
    __device__ __forceinline__ void dispatch(Walk walk) const {
        if constexpr (NP > 1) {
            if (fast) walk(std::true_type{});
            else walk(std::false_type{});
        } else {
            walk(std::false_type{});
        }
    }

    // the nearest real segment at or after s / at or before s (ns / -1: none)
    __device__ __forceinline__ int real_from(int s) const {
        if constexpr (MARKERS) while (s < ns && lay[s] == kRaySurfaceMarker) ++s;
        return s;
    }
    __device__ __forceinline__ int real_back(int s) const {
        if constexpr (MARKERS) while (s >= 0 && lay[s] == kRaySurfaceMarker) --s;
        return s;
    }

    // The segments in order of travel: marker() at a surface marker, step(s, k, len) for a real segment s with the points'
    // absorption coefficients k of its layer and every ray's path length len[i] through it.
    template <class Marker, class Step>
    __device__ __forceinline__ void forward(Marker marker, Step step) const {
        int ahead = real_from(0);
        vec cur = ahead < ns ? load_points<NP>(A.abs_coef[lay[ahead]], j) : (vec)(0.0);
        for (int s = 0; s < ns; ++s) {
            if (MARKERS && lay[s] == kRaySurfaceMarker) {
                marker();
                continue;
            }
            ahead = real_from(s + 1);
            const vec nxt = ahead < ns ? load_points<NP>(A.abs_coef[lay[ahead]], j) : cur;
            double len[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) len[i] = seg_length[s0[i] + s];
            step(s, cur, len);
            cur = nxt;
        }
    }

    // The same last to first (the Jacobian kernels' second pass)
    template <class Marker, class Step>
    __device__ __forceinline__ void backward(Marker marker, Step step) const {
        int behind = real_back(ns - 1);
        vec cur = behind >= 0 ? load_points<NP>(A.abs_coef[lay[behind]], j) : (vec)(0.0);
        for (int s = ns - 1; s >= 0; --s) {
            if (MARKERS && lay[s] == kRaySurfaceMarker) {
                marker();
                continue;
            }
            behind = real_back(s - 1);
            const vec nxt = behind >= 0 ? load_points<NP>(A.abs_coef[lay[behind]], j) : cur;
            double len[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) len[i] = seg_length[s0[i] + s];
            step(s, cur, len);
            cur = nxt;
        }
    }

    // every ray's radiance and, where asked for, total transmittance at the thread's points
    __device__ __forceinline__ void store(const double (&I)[RB][NP], const double (&Tt)[RB][NP]) const {
        if (!active) return;
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const long long o = (long long)rid[i] * A.n + j;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                A.radiance[o + p] = I[i][p];
                if (A.transmittance) A.transmittance[o + p] = Tt[i][p];
            }
        }
    }
};

// K5e: ray paths (lbl_ray_radiance_dev; the semantics are in include/pyrad_hip.h).  K5c's step along an ordered list of
// (layer, path length) segments instead of the column bottom to top: no level sums, so no reductions and nothing shared
// between threads.  One workgroup = 256 NP points x one BUNDLE of RB rays that cross the same layers in the same order
// (the host finds them, lbl_column_transport.hip): k_l is loaded and B_l formed once per segment for the bundle, and every
// ray of it pays only its own exp(-k_l length) and update - the way K5c's angles share a layer.  The operations of one ray
// are the same in every bundle size, so its bits do not depend on the rays it travels with.  Ray, segment and layer
// indices are uniform over the workgroup: the tables and the layer scalars come through scalar loads.
template <int NP, int RB>
__global__ __launch_bounds__(256) void ray_radiance_kernel(const RayArgs* __restrict__ Ap, long long lo0, long long n0,
                                                           long long lo1, long long n1, int order_first) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    const RayArgs& A = *Ap;
    const RayFrame<NP, RB, false, RayArgs> F(Ap, blockDim.x, lo0, n0, lo1, n1, order_first);
    double I[RB][NP], Tt[RB][NP];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
#pragma unroll
        for (int p = 0; p < NP; ++p) { I[i][p] = F.surface[i] ? F.Is[p] : 0.0; Tt[i][p] = 1.0; }
    }
    F.dispatch([&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        F.forward([] {}, [&](int s, vec cur, const double (&len)[RB]) {
            transport_step<FAST, NP>(F.nu, F.pa_n, A.pbkT[F.lay[s]], cur, [&](int p, double kp, double B) {
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    const double tr = exp_neg_budget(kp * len[i]);
                    I[i][p] = fold_update<FAST>(tr, I[i][p], B);
                    Tt[i][p] = Tt[i][p] * tr;
                }
            });
        });
    });
    F.store(I, Tt);
}

// ----------------------------------------------------------------------------------------
// K5g: reflecting surface (lbl_column_flux_surface_dev, lbl_ray_radiance_surface_dev; the semantics are in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// What leaves a surface of emissivity e that emits Is and reflects R: e Is + (1 - e) R, every operation rounded.  With
// e == 1 it is Is bit for bit for every finite R (1 Is + 0 R), which is what makes both kernels below return K5c's and K5e's
// bits over a black surface without a special case.
__device__ __forceinline__ double surface_leaving(double e, double Is, double R) {
#pragma clang fp contract(off)
    const double emitted = e * Is;
    const double reflected = (1.0 - e) * R;
    return emitted + reflected;
}

// K5c's kernel with the walks in the other order: DOWNWARD first, so that the downward radiances at level 0 are in the
// registers when the surface is met; they are turned in place into the upward ones - Lambertian: every angle gets
// F_down(0) / w_sum, so that sum_k W_k (1 - e) R_k = (1 - e) F_down(0) under the quadrature whatever the angle set;
// specular: each angle its own - and the upward walk starts from them.  The step, the level sums, the slots and the
// partials are K5c's (each level slot receives the same terms in the same order), column_flux_final_kernel finishes.
// The surface source Is is formed BEFORE the downward walk, where K5c forms it - with nothing else in the registers - and
// waits in LDS, one slot per thread and point that only its thread touches: formed at the surface, between the walks with
// every angle's radiance alive, the general Planck expression costs the seven-angle body 11 spilled registers at K5c's
// three waves per SIMD.  So the surface adds no register that lives through a walk; e is read where it is used.
// (the second launch bound: the waves per SIMD of K5c's instantiation for the same NP and NA - 4 with one angle, 3 up to
// seven, 2 with eight; left to itself the seven-angle body takes 171 registers, 3 more than three waves allow)
template <int NP, int NA> constexpr int surface_flux_waves() { return NP == 1 ? 1 : NA == 1 ? 4 : NA <= 7 ? 3 : 2; }
template <int NP, int NA>
__global__ __launch_bounds__(256, (surface_flux_waves<NP, NA>())) void surface_flux_kernel(const SurfaceFluxArgs* __restrict__ Ap, long long lo0, long long n0,
                                                           long long lo1, long long n1, double* __restrict__ partial) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    constexpr int kSlot = 2 * (kMaxLayers + 1);
    __shared__ double acc[4 * kSlot];            // [wave][up levels 0..L, down levels 0..L]
    __shared__ double source[NP * 256];          // [point][thread]: Is, from before the downward walk to the surface
    const SurfaceFluxArgs& A = *Ap;
    const int L = A.n_layers;
    const int nv = 2 * (L + 1);
    for (int t = threadIdx.x; t < 4 * kSlot; t += blockDim.x) acc[t] = 0.0;
    __syncthreads();
    double* my = acc + (threadIdx.x >> 6) * kSlot;
    const bool lane0 = (threadIdx.x & 63) == 0;
    const long long total = n0 + n1;
    const long long stride = (long long)gridDim.x * blockDim.x * NP;
    // (the loop bound is uniform over the workgroup: every lane takes part in the wave reductions, idle lanes on a valid point)
    for (long long q0 = (long long)blockIdx.x * blockDim.x * NP; q0 < total; q0 += stride) {
        const long long q = q0 + (long long)threadIdx.x * NP;
        const bool active = q < total;
        const long long j = !active ? lo0 : (q < n0 ? lo0 + q : lo1 + (q - n0));
        double nu[NP], pa_n[NP], I[NA][NP];
        column_points<NP>(A, j, nu, pa_n);
        const bool fast = fold_fast_path<NP>(A, nu, active);
        // sum_k W_k I_k per point, nan_to_num, summed over the thread's points, the wave, and into the wave's slot
        auto level = [&](int slot, double* spec, double* spec2 = nullptr) {
            double s = 0.0;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double f = angle_sum<NA>(A, [&](int k) { return I[k][p]; });
                if (spec && active) spec[j + p] = f;
                if (spec2 && active) spec2[j + p] = f;
                s += active ? nan_to_num(f) : 0.0;
            }
            s = wave_sum(s);
            if (lane0) my[slot] += s;
        };
        auto layer = [&](auto fast_tag, int l, vec v) {
            constexpr bool FAST = decltype(fast_tag)::value;
            const double depth = A.depth[l];
            transport_step<FAST, NP>(nu, pa_n, A.pbkT[l], v, [&](int p, double kp, double B) {
                const double tau = kp * depth;
#pragma unroll
                for (int k = 0; k < NA; ++k) I[k][p] = fold_update<FAST>(exp_neg_budget(tau * A.rmu[k]), I[k][p], B);
            });
        };
        auto walk = [&](auto fast_tag) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
                source[p * 256 + threadIdx.x] = A.I_surface ? A.I_surface[j + p] : planck_budget(nu[p], A.pa, A.pbk_surface);
            // downward: I_L = I_top or 0; level l after layer l
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double It = A.I_top ? A.I_top[j + p] : 0.0;
#pragma unroll
                for (int k = 0; k < NA; ++k) I[k][p] = It;
            }
            level(L + 1 + L, L == 0 ? A.down_surface : nullptr);
            vec cur = L > 0 ? load_points<NP>(A.abs_coef[L - 1], j) : (vec)(0.0);
            for (int l = L - 1; l >= 0; --l) {
                const vec nxt = l > 0 ? load_points<NP>(A.abs_coef[l - 1], j) : cur;
                layer(fast_tag, l, cur);
                level(L + 1 + l, l == 0 ? A.down_surface : nullptr);
                cur = nxt;
            }
            // the surface: I_up[0] = e Is + (1 - e) R, in place
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double e = A.emissivity ? A.emissivity[j + p] : A.emissivity_all;
                const double Is = source[p * 256 + threadIdx.x];
                const double diffuse = angle_sum<NA>(A, [&](int k) { return I[k][p]; }) / A.w_sum;
#pragma unroll
                for (int k = 0; k < NA; ++k) I[k][p] = surface_leaving(e, Is, A.reflection == 0 ? diffuse : I[k][p]);
            }
            // upward: level l + 1 after layer l
            level(0, A.up_surface, L == 0 ? A.up_top : nullptr);
            cur = L > 0 ? load_points<NP>(A.abs_coef[0], j) : (vec)(0.0);
            for (int l = 0; l < L; ++l) {
                const vec nxt = l + 1 < L ? load_points<NP>(A.abs_coef[l + 1], j) : cur;
                layer(fast_tag, l, cur);
                level(l + 1, l + 1 == L ? A.up_top : nullptr);
                cur = nxt;
            }
        };
        if constexpr (NP > 1) {
            if (fast) walk(std::true_type{});
            else walk(std::false_type{});
        } else {
            walk(std::false_type{});
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nv; t += blockDim.x)
        partial[(long long)blockIdx.x * nv + t] = (acc[t] + acc[kSlot + t]) + (acc[2 * kSlot + t] + acc[3 * kSlot + t]);
}

// K5e's kernel with a surface in the path: a segment whose layer is kRaySurfaceMarker is no segment but the place where the
// ray meets the surface and is reflected specularly (I <- e Is + (1 - e) I, Ttot <- Ttot (1 - e)), and a ray that starts at
// the surface starts with e Is + (1 - e) Rd, Rd the diffuse reflection of surface_down (0 without it).  The rays of a bundle
// share their layer sequence, markers included, so the branch on a marker is uniform over the workgroup; the prefetch of
// k_l runs one real segment ahead, past the markers.  The operations of a real segment are K5e's.
// One body for this kernel and K5i's (LINEAR: linear_step and linear_update with the segment's own pair of Planck exponents,
// entry and exit in the light's direction of travel, from the table beside seg_length - the rays of a bundle share the
// pairs as they share the layers, the host bundles by both, so the pair is read from the bundle's first ray).
template <int NP, int RB, bool LINEAR, class Args>
__device__ __forceinline__ void ray_surface_walks(const Args* Ap, unsigned threads, long long lo0, long long n0, long long lo1,
                                                  long long n1, int order_first) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    const Args& A = *Ap;
    const RayFrame<NP, RB, true, Args> F(Ap, threads, lo0, n0, lo1, n1, order_first);
    double I[RB][NP], Tt[RB][NP];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double Rd = A.surface_down ? A.surface_down[F.j + p] / A.surface_down_norm : 0.0;
            I[i][p] = F.surface[i] ? surface_leaving(F.em[p], F.Is[p], Rd) : 0.0;
            Tt[i][p] = 1.0;
        }
    }
    const double* pbk = nullptr;        // (LINEAR) the bundle's exponent pairs, formed once, outside the segment loop
    if constexpr (LINEAR) pbk = (const double*)(F.blk + A.off_seg_pbkT) + 2 * (long long)F.s0[0];
    F.dispatch([&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        F.forward([&] {
#pragma unroll
            for (int i = 0; i < RB; ++i) {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    I[i][p] = surface_leaving(F.em[p], F.Is[p], I[i][p]);
                    Tt[i][p] = Tt[i][p] * (1.0 - F.em[p]);
                }
            }
        }, [&](int s, vec cur, const double (&len)[RB]) {
            if constexpr (LINEAR) {
                linear_step<FAST, NP>(F.nu, F.pa_n, pbk[2 * s], pbk[2 * s + 1], cur, [&](int p, double kp, double Ba, double dB) {
#pragma unroll
                    for (int i = 0; i < RB; ++i) {
                        const double tau = kp * len[i];
                        const double tr = exp_neg_budget(tau);
                        I[i][p] = linear_update<FAST>(tau, tr, I[i][p], Ba, dB);
                        Tt[i][p] = Tt[i][p] * tr;
                    }
                });
            } else {
                transport_step<FAST, NP>(F.nu, F.pa_n, A.pbkT[F.lay[s]], cur, [&](int p, double kp, double B) {
#pragma unroll
                    for (int i = 0; i < RB; ++i) {
                        const double tr = exp_neg_budget(kp * len[i]);
                        I[i][p] = fold_update<FAST>(tr, I[i][p], B);
                        Tt[i][p] = Tt[i][p] * tr;
                    }
                });
            }
        });
    });
    F.store(I, Tt);
}

template <int NP, int RB>
__global__ __launch_bounds__(256) void ray_surface_kernel(const RaySurfaceArgs* __restrict__ Ap, long long lo0, long long n0,
                                                          long long lo1, long long n1, int order_first) {
    ray_surface_walks<NP, RB, false>(Ap, blockDim.x, lo0, n0, lo1, n1, order_first);
}

// ----------------------------------------------------------------------------------------
// K5k: direct solar beam (lbl_column_solar_dev; the semantics are in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// K5c's walks without a source term: a value is only ever attenuated, S <- exp_neg_budget(k_l depth_l rate) S, so there is no
// Planck term, no wavenumber and no fast / general split.  Two kernels over one body, each carrying NB values per point in
// registers the way K5c carries its angles:
//   solar_beam_kernel<NP, NB>     NB beams, rate = slant[s][l], weight = beam_w[s].  Down from S0 at the top; the spectral
//                                 F_down(0) goes to f0 (Lambertian).  Specular: the surface turns every beam in place,
//                                 U_s = (1 - e) S_s, and the upward walk follows in the same kernel (K5g's order of walks),
//                                 so that no beam's S_s[0] has to be kept or formed twice.
//   solar_diffuse_kernel<NP, NA>  Lambertian: NA angles, rate = 1 / mu_k, weight = W_k.  Up from (1 - e) f0 / w_sum.
// A beam's operations are the same whatever the other beams of the call are (one exp and one product per layer, its own
// table row), so its bits do not depend on them; a level's flux is the fma chain of angle_sum over the beams, beam 0 first.
// Rates, weights and depths are workgroup-uniform and come through scalar loads.  Level sums, slots, partials and the final
// reduction are K5c's; the beam kernel's partial holds [down 0..L] (Lambertian) or [up 0..L, down 0..L] (specular), the
// diffuse kernel's [up 0..L].
template <int NP, int NB, bool DIFFUSE>
__device__ __forceinline__ void solar_walks(const SolarArgs& A, unsigned threads, long long lo0, long long n0, long long lo1,
                                            long long n1, double* __restrict__ partial, double* acc) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    constexpr int kSlot = 2 * (kMaxLayers + 1);
    const int L = A.n_layers;
    const bool specular = !DIFFUSE && A.reflection == 1;
    const int nv = specular ? 2 * (L + 1) : L + 1;
    const int down0 = specular ? L + 1 : 0;
    auto rate = [&](int s, int l) { return DIFFUSE ? A.rmu[s] : A.slant[s][l]; };
    auto wt = [&](int s) { return DIFFUSE ? A.w[s] : A.beam_w[s]; };
    band_frame<NP, kSlot, false>(A, threads, lo0, n0, lo1, n1, partial, acc, nv, [&](auto, long long j, bool active,
                                 const double (&)[NP], const double (&)[NP], auto add) {
        double S[NB][NP];
        // sum_s w_s S_s per point (beam 0 first), nan_to_num, summed over the thread's points, the wave, into the wave's slot
        auto level = [&](int slot, double* spec, double* spec2 = nullptr) {
            double sum = 0.0;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                double f = wt(0) * S[0][p];
#pragma unroll
                for (int s = 1; s < NB; ++s) f = fma(wt(s), S[s][p], f);
                if (spec && active) spec[j + p] = f;
                if (spec2 && active) spec2[j + p] = f;
                sum += active ? nan_to_num(f) : 0.0;
            }
            add(slot, sum);
        };
        auto layer = [&](int l, vec v) {
            const double depth = A.depth[l];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double tau = v[p] * depth;
#pragma unroll
                for (int s = 0; s < NB; ++s) S[s][p] = exp_neg_budget(tau * rate(s, l)) * S[s][p];
            }
        };
        vec cur;
        if constexpr (!DIFFUSE) {
            // downward: S_s[L] = S0; level l after layer l
            const vec top = load_points<NP>(A.S0, j);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
#pragma unroll
                for (int s = 0; s < NB; ++s) S[s][p] = top[p];
            }
            double* const surface2 = A.down_surface != A.f0 ? A.down_surface : nullptr;
            level(down0 + L, L == 0 ? A.f0 : nullptr, L == 0 ? surface2 : nullptr);
            cur = L > 0 ? load_points<NP>(A.abs_coef[L - 1], j) : (vec)(0.0);
            for (int l = L - 1; l >= 0; --l) {
                const vec nxt = l > 0 ? load_points<NP>(A.abs_coef[l - 1], j) : cur;
                layer(l, cur);
                level(down0 + l, l == 0 ? A.f0 : nullptr, l == 0 ? surface2 : nullptr);
                cur = nxt;
            }
        }
        if (DIFFUSE || specular) {
            // the surface: nothing is emitted, (1 - e) of what came down leaves again
            vec f0;
            if constexpr (DIFFUSE) f0 = load_points<NP>(A.f0, j);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double e = A.emissivity ? A.emissivity[j + p] : A.emissivity_all;
                if constexpr (DIFFUSE) {
                    const double leaving = ((1.0 - e) * f0[p]) / A.w_sum;
#pragma unroll
                    for (int s = 0; s < NB; ++s) S[s][p] = leaving;
                } else {
#pragma unroll
                    for (int s = 0; s < NB; ++s) S[s][p] = (1.0 - e) * S[s][p];
                }
            }
            // upward: level l + 1 after layer l
            level(0, A.up_surface, L == 0 ? A.up_top : nullptr);
            cur = L > 0 ? load_points<NP>(A.abs_coef[0], j) : (vec)(0.0);
            for (int l = 0; l < L; ++l) {
                const vec nxt = l + 1 < L ? load_points<NP>(A.abs_coef[l + 1], j) : cur;
                layer(l, cur);
                level(l + 1, l + 1 == L ? A.up_top : nullptr);
                cur = nxt;
            }
        }
    });
}

template <int NP, int NB>
__global__ __launch_bounds__(256) void solar_beam_kernel(const SolarArgs* __restrict__ Ap, long long lo0, long long n0,
                                                         long long lo1, long long n1, double* __restrict__ partial) {
    __shared__ double acc[4 * 2 * (kMaxLayers + 1)];     // [wave][up levels 0..L, down levels 0..L]
    solar_walks<NP, NB, false>(*Ap, blockDim.x, lo0, n0, lo1, n1, partial, acc);
}

template <int NP, int NA>
__global__ __launch_bounds__(256) void solar_diffuse_kernel(const SolarArgs* __restrict__ Ap, long long lo0, long long n0,
                                                            long long lo1, long long n1, double* __restrict__ partial) {
    __shared__ double acc[4 * 2 * (kMaxLayers + 1)];
    solar_walks<NP, NA, true>(*Ap, blockDim.x, lo0, n0, lo1, n1, partial, acc);
}

// ----------------------------------------------------------------------------------------
// K5l: two-stream multiple scattering of the beams (lbl_column_twostream_dev; the semantics are in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// A scattering layer couples the levels both ways, so one walk does not do: the column is solved by adding, in two kernels.
//   twostream_down_kernel<NB>  top to bottom, where the direct beams are at hand: per layer the two-stream solution (R, T and
//                              per beam Td, Rb, Tb), the beams' sources P and Q, and the composition of the stack above the
//                              level: dn_i = Rs_i up_i + Ds_i.  It writes Rs, Ds, the two numbers U1, U0 of the upward step
//                              up_(l+1) = U1 up_l + U0, and the direct flux, per level, into the workspace.
//   twostream_up_kernel        bottom to top through those five numbers alone (no coefficient, no beam and no scatterer is
//                              read again, so it has one instantiation): the surface, then up and dn per level, the spectra
//                              and every level sum.
// Up to 129 levels of five numbers cannot live in registers, hence the workspace, [number][level][point of the pass]: a
// wave's accesses are 512 contiguous bytes.  One point per thread: a point carries 12 scatterer numbers and NB beam values
// besides the layer's temporaries, and four points would spill.  The scatterers are always kMaxScatterers: those beyond n_scat
// have amount, extinction and albedo 0 from the host and add exact zeros.  Slants, 1 / slant, amounts, depths and beam weights
// are workgroup-uniform and come through scalar loads.
// Sums (second kernel): nan_to_num per point, wave_sum, the four waves added in a fixed order, and the tile's value added to
// slot (tile of the band) % slots of the partials by the one workgroup that owns the slot, tiles ascending; the passes of a
// band follow each other in stream order, so a slot's additions are the same whatever the pass size; column_flux_final_kernel
// finishes.  No float atomics.
// What the family's kernels (K5l here; K5m, K5n, K5o and K5p below) share.
// a point's scatterers, per unit amount: what each adds to a layer's absorption, scattering and asymmetry-weighted depths
__device__ __forceinline__ void scatterer_numbers(const ScatterPart& A, long long j, double (&al)[kMaxScatterers],
                                                  double (&si)[kMaxScatterers], double (&et)[kMaxScatterers]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < kMaxScatterers; ++c) {
        const double ext = A.ext[c] ? load_global_f64(A.ext[c], j) : A.ext_all[c];
        const double ssa = A.ssa[c] ? load_global_f64(A.ssa[c], j) : A.ssa_all[c];
        const double gc = A.asym[c] ? load_global_f64(A.asym[c], j) : A.asym_all[c];
        const double f = A.delta_scaling ? gc * gc : 0.0;
        al[c] = ext * (1.0 - ssa);
        si[c] = (ext * ssa) * (1.0 - f);
        et[c] = (ext * ssa) * (gc - f);
    }
}

// layer l (of depth `depth`) at a point with absorption coefficient k: its depths and the two-stream solution for diffuse light.  At t == 0
// (`empty`) R = 0 and T = 1, and nothing else is to be used; `conservative` is den == 0, where Ab = 0.
struct TwoStreamLayer {
    double ta, ts, tsg, t, w, g, Da, g1, g2, lam, R, T, Ab;
    bool empty, conservative;
};
__device__ __forceinline__ TwoStreamLayer twostream_layer(const ScatterPart& A, int l, double depth, double k,
                                                          const double (&al)[kMaxScatterers],
                                                          const double (&si)[kMaxScatterers],
                                                          const double (&et)[kMaxScatterers]) {
#pragma clang fp contract(off)
    constexpr double D = 1.7320508075688772;        // sqrt(3), rounded
    TwoStreamLayer Y;
    double ta = k * depth, ts = 0.0, tsg = 0.0;
#pragma unroll
    for (int c = 0; c < kMaxScatterers; ++c) {
        const double am = A.amount[c][l];
        ta = ta + am * al[c];
        ts = ts + am * si[c];
        tsg = tsg + am * et[c];
    }
    const double t = ta + ts;
    const double a = ta / t, b = (t - tsg) / t;
    const double Da = D * a, Db = D * b;
    const double g1 = 0.5 * (Db + Da), g2 = 0.5 * (Db - Da);
    const double lam = sqrt(Da * Db);
    const double lt = lam * t;
    const double E = exp_neg_budget(lt);
    const double g1l = g1 + lam;
    const double Gam = g2 / g1l;
    const double oG = ((Da + lam) * (Db + lam)) / (g1l * g1l);
    const double oE = -expm1(-2.0 * lt);
    const double den = oG + (Gam * Gam) * oE;
    const double g1t = g1 * t;
    Y.ta = ta; Y.ts = ts; Y.tsg = tsg; Y.t = t;
    Y.w = ts / t; Y.g = ts == 0.0 ? 0.0 : tsg / ts;
    Y.Da = Da; Y.g1 = g1; Y.g2 = g2; Y.lam = lam;
    Y.empty = t == 0.0;
    Y.conservative = den == 0.0;
    Y.R = den == 0.0 ? g1t / (1.0 + g1t) : (Gam * oE) / den;
    Y.T = den == 0.0 ? 1.0 / (1.0 + g1t) : (E * oG) / den;
    if (Y.empty) { Y.R = 0.0; Y.T = 1.0; }
    Y.Ab = den == 0.0 ? 0.0 : ((-expm1(-lt) * ((Da + lam) / g1l)) * (1.0 - Gam * E)) / den;
    return Y;
}

// the layer (R, T, its sources P up and Q down) joined to the stack above it, dn = Rs up + Ds: the stack from the layer's
// bottom in Rs, Ds (NaN once some layer's t was not finite) and the upward step up_(l+1) = U1 up_l + U0
__device__ __forceinline__ void twostream_add(double R, double T, double P, double Q, bool bad, double& Rs, double& Ds,
                                              double& U1, double& U0) {
#pragma clang fp contract(off)
    const double c = 1.0 - R * Rs;
    U1 = T / c;
    U0 = (R * Ds + P) / c;
    const double Dn = Q + T * ((Ds + Rs * P) / c);
    Rs = R + (T * U1) * Rs;
    Ds = Dn;
    if (bad) Rs = Ds = __builtin_nan("");
}

// The downward walk of K5l and K5m: the point of this thread, its scatterers, then top to bottom the layer solution, the
// stack above each level and the workspace's four numbers per level.  What a kernel adds: top(j) sets up its own state and
// gives Ds at the top of the column; sources(l, lay, P, Q) gives the layer's sources; level(i, ws) stores what else the
// kernel keeps per level.  (threads: blockDim.x, read by the __global__ kernel itself - see band_frame)
template <class Args, class Top, class Sources, class Level>
__device__ __forceinline__ void twostream_down_frame(const Args& A, unsigned threads, long long first, long long count, Top top,
                                                     Sources sources, Level level) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * threads + threadIdx.x;
    if (q >= count) return;
    const long long j = first + q;
    const int L = A.n_layers;
    const long long row = A.ws_points;
    double* const W = A.workspace + q;
    auto ws = [&](int v, int i) -> double& { return W[((long long)v * (L + 1) + i) * row]; };
    double al[kMaxScatterers], si[kMaxScatterers], et[kMaxScatterers];
    scatterer_numbers(A, j, al, si, et);
    double Rs = 0.0, Ds = top(j);
    bool bad = false;
    ws(0, L) = Rs; ws(1, L) = Ds; level(L, ws);
    double k = L > 0 ? load_global_f64(A.abs_coef[L - 1], j) : 0.0;
    for (int l = L - 1; l >= 0; --l) {
        const double k_next = l > 0 ? load_global_f64(A.abs_coef[l - 1], j) : k;
        const TwoStreamLayer lay = twostream_layer(A, l, A.depth[l], k, al, si, et);
        bad = bad || !isfinite(lay.t);
        double P, Q;
        sources(l, lay, P, Q);
        double U1, U0;
        twostream_add(lay.R, lay.T, P, Q, bad, Rs, Ds, U1, U0);
        ws(2, l + 1) = U1; ws(3, l + 1) = U0;
        ws(0, l) = Rs; ws(1, l) = Ds; level(l, ws);
        k = k_next;
    }
}

// the end of a tile in the upward kernels (K5l, K5m, K5p): the four waves' rows acc[wave][0 .. nv), kSlot doubles apart, added
// in a fixed order into the tile's slot of the partials
template <int kSlot>
__device__ __forceinline__ void tile_slot_add(double* slot, const double* acc, int nv, unsigned threads) {
#pragma clang fp contract(off)
    __syncthreads();
    for (int t = threadIdx.x; t < nv; t += threads)
        slot[t] = slot[t] + ((acc[t] + acc[kSlot + t]) + (acc[2 * kSlot + t] + acc[3 * kSlot + t]));
    __syncthreads();
}

// The upward walk of K5l and K5m over ROWS rows of level sums (up, diffuse down and, with 3, the direct flux of workspace
// quantity 4): the tiles of this workgroup's slot in ascending order; per tile the surface - surface(active, j, Rs, Ds, F)
// gives `up` there - then up and dn per level from the workspace alone, the spectra, the wave sums, and the tile's value
// added to its slot.  acc: 4 x ROWS x (kMaxLayers + 1) doubles of LDS, [wave][row][level].
template <int ROWS, class Args, class Surface>
__device__ __forceinline__ void twostream_up_frame(const Args& A, unsigned threads, long long tile0, long long first,
                                                   long long count, int slots, double* __restrict__ partial, double* acc,
                                                   Surface surface) {
#pragma clang fp contract(off)
    constexpr int kSlot = ROWS * (kMaxLayers + 1);
    const int L = A.n_layers;
    const int levels = L + 1, nv = ROWS * levels;
    const long long row = A.ws_points;
    double* const my = acc + (threadIdx.x >> 6) * kSlot;
    const bool lane0 = (threadIdx.x & 63) == 0;
    const long long tiles = (count + kTwoStreamTile - 1) / kTwoStreamTile;
    // (the loop bound is uniform over the workgroup: every lane takes part in the wave reductions)
    for (long long tile = blockIdx.x; tile < tiles; tile += slots) {
        const long long q = tile * kTwoStreamTile + threadIdx.x;
        const bool active = q < count;
        const long long j = first + q;
        const double* const W = A.workspace + q;
        auto ws = [&](int v, int i) { return active ? W[((long long)v * levels + i) * row] : 0.0; };
        double Rs = ws(0, 0), Ds = ws(1, 0), F = 0.0;
        if constexpr (ROWS == 3) F = ws(4, 0);
        const bool bad = isnan(Rs) || isnan(Ds);
        const double nan = __builtin_nan("");
        double up = surface(active, j, Rs, Ds, F);
        for (int i = 0; i <= L; ++i) {
            if (i > 0) {
                up = ws(2, i) * up + ws(3, i);
                Rs = ws(0, i); Ds = ws(1, i);
                if constexpr (ROWS == 3) F = ws(4, i);
            }
            double dn = Rs * up + Ds;
            if (bad) up = dn = F = nan;
            if (active) {
                if (i == 0) {
                    if (A.up_surface) A.up_surface[j] = up;
                    if (A.down_surface) A.down_surface[j] = dn;
                    if constexpr (ROWS == 3)
                        if (A.direct_surface) A.direct_surface[j] = F;
                }
                if (i == L && A.up_top) A.up_top[j] = up;
            }
            const double s_up = wave_sum(active ? nan_to_num(up) : 0.0);
            const double s_dn = wave_sum(active ? nan_to_num(dn) : 0.0);
            if (lane0) { my[i] = s_up; my[levels + i] = s_dn; }
            if constexpr (ROWS == 3) {
                const double s_F = wave_sum(active ? nan_to_num(F) : 0.0);
                if (lane0) my[2 * levels + i] = s_F;
            }
        }
        tile_slot_add<kSlot>(partial + ((tile0 + tile) % slots) * nv, acc, nv, threads);
    }
}

// The upward walk that recomputes the layers (K5n, K5o, K5p): the point's scatterer numbers and the stack above the surface
// from the downward kernel's workspace, then per layer twostream_layer, up <- U1 up + U0, Rs and Ds of the level above and
// dn = Rs up + Ds, with up and dn of the level below kept.  Two calls, the kernel's level-0 work between them: surface(w)
// gives `up` at the surface from w.Rs and w.Ds; layer(l, lay, k) sees the walk at the top of layer l; the NaN rule on w.up
// ends it.  q: the point's place in the pass (K5p: the tile's first point in a lane beyond the pass).
struct UpWalk {
    const double* W; long long row; int levels;     // the point's workspace: quantity v at level i is W[(v levels + i) row]
    double al[kMaxScatterers], si[kMaxScatterers], et[kMaxScatterers];
    double Rs, Ds, up, dn;              // at the level the walk has reached
    double upB, dnB;                    // up and dn at the level below it
    bool bad;                           // some layer's t was not finite: every result of the point is NaN
    __device__ __forceinline__ double ws(int v, int i) const { return W[((long long)v * levels + i) * row]; }
};
template <class Args, class Surface>
__device__ __forceinline__ void twostream_up_start(const Args& A, long long q, long long j, UpWalk& w, Surface surface) {
#pragma clang fp contract(off)
    w.W = A.workspace + q; w.row = A.ws_points; w.levels = A.n_layers + 1;
    scatterer_numbers(A, j, w.al, w.si, w.et);
    w.Rs = w.ws(0, 0); w.Ds = w.ws(1, 0);
    w.bad = isnan(w.Rs) || isnan(w.Ds);
    w.up = surface(w);
    w.dn = w.Rs * w.up + w.Ds;
}
template <class Args, class Layer>
__device__ __forceinline__ void twostream_up_layers(const Args& A, long long j, UpWalk& w, Layer layer) {
#pragma clang fp contract(off)
    const int L = A.n_layers;
    double k = L > 0 ? load_global_f64(A.abs_coef[0], j) : 0.0;
    for (int l = 0; l < L; ++l) {
        const double k_next = l + 1 < L ? load_global_f64(A.abs_coef[l + 1], j) : k;
        const TwoStreamLayer lay = twostream_layer(A, l, A.depth[l], k, w.al, w.si, w.et);
        w.upB = w.up; w.dnB = w.dn;
        w.up = w.ws(2, l + 1) * w.up + w.ws(3, l + 1);
        w.Rs = w.ws(0, l + 1); w.Ds = w.ws(1, l + 1);
        w.dn = w.Rs * w.up + w.Ds;
        layer(l, lay, k);
        k = k_next;
    }
    if (w.bad) w.up = __builtin_nan("");
}

template <int NB>
__global__ __launch_bounds__(256) void twostream_down_kernel(const TwoStreamArgs* __restrict__ Ap, long long first,
                                                             long long count) {
#pragma clang fp contract(off)
    const TwoStreamArgs& A = *Ap;
    constexpr double D = 1.7320508075688772;        // sqrt(3), rounded
    double S[NB];
    auto direct = [&]() {
        double f = A.beam_w[0] * S[0];
#pragma unroll
        for (int s = 1; s < NB; ++s) f = fma(A.beam_w[s], S[s], f);
        return f;
    };
    twostream_down_frame(A, blockDim.x, first, count,
        [&](long long j) {
            const double top = load_global_f64(A.S0, j);
#pragma unroll
            for (int s = 0; s < NB; ++s) S[s] = top;
            return 0.0;
        },
        [&](int l, const TwoStreamLayer& lay, double& P, double& Q) {
            const double t = lay.t, w = lay.w, g = lay.g, Da = lay.Da, g1 = lay.g1, g2 = lay.g2, lam = lay.lam;
            const double R = lay.R, T = lay.T, Ab = lay.Ab;
            const bool empty = lay.empty;
            P = 0.0; Q = 0.0;
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                const double Td = exp_neg_budget(t * A.slant[s][l]);       // (exactly 1 at t = 0)
                double m = A.m[s][l];
                const double g3 = 0.5 * (1.0 - (D * g) * m), g4 = 1.0 - g3;
                const double a2 = g1 * g3 + g2 * g4;
                double Tdm = Td;
                if (fabs(1.0 - lam * m) < 1e-6) {
                    m = (1.0 - 1e-6) / lam;
                    Tdm = exp_neg_budget(t / m);
                }
                const double pole = (1.0 - lam * m) * (1.0 + lam * m);
                const double Cp = (w * (g3 - a2 * m)) / pole;
                const double u = (w * (1.0 + (Da * (g4 - g3)) * m)) / pole;
                const double Y = (Cp * T) * (1.0 - Tdm);
                const double Rb = empty ? 0.0 : Y + (R * u + Cp * Ab);
                const double Tb = empty ? 0.0 : (u * (T - Tdm) + (Cp * Tdm) * Ab) - Y;
                const double Fd = A.beam_w[s] * S[s];
                P = s == 0 ? Rb * Fd : fma(Rb, Fd, P);
                Q = s == 0 ? Tb * Fd : fma(Tb, Fd, Q);
                S[s] = Td * S[s];
            }
        },
        [&](int i, auto& ws) { ws(4, i) = direct(); });
}

__global__ __launch_bounds__(256) void twostream_up_kernel(const TwoStreamArgs* __restrict__ Ap, long long tile0, long long first,
                                                           long long count, int slots, double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double acc[4 * 3 * (kMaxLayers + 1)];     // [wave][up levels 0..L, diffuse down levels 0..L, direct levels 0..L]
    const TwoStreamArgs& A = *Ap;
    // the reflecting surface under the diffuse and the direct light
    twostream_up_frame<3>(A, blockDim.x, tile0, first, count, slots, partial, acc,
        [&](bool active, long long j, double Rs, double Ds, double F) {
            const double e = !active ? 1.0 : A.emissivity ? A.emissivity[j] : A.emissivity_all;
            const double albedo = 1.0 - e;
            return (albedo * (Ds + F)) / (1.0 - albedo * Rs);
        });
}

// ----------------------------------------------------------------------------------------
// K5m: thermal fluxes through scattering layers (lbl_column_flux_scatter_dev; the semantics are in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// K5l's two kernels with the layers' own emission in place of the beams: the layer solution (twostream_layer) and the adding
// step (twostream_add) are K5l's, the sources are P = Bt Ab + d h up at the layer's top and Q = Bb Ab - d h down at its
// bottom, with Bt, Bb = pi B at the top and bottom edge, d = Bb - Bt and h = (Ab + 2 R) / (D (t - tsg)) - T: the particular
// solution pi B(tau) +- d / ((g1 + g2) t) of a Planck function linear in optical depth, with the homogeneous response
// subtracted and 1 + R - T = Ab + 2 R.  Ab comes without cancellation, so a thin layer emits Ab pi B and not a rounding error.
//   scatter_flux_down_kernel<LINEAR>  top to bottom from Ds_L = pi I_top; LINEAR = false: one Planck value per layer (d = 0,
//                                     no h); LINEAR = true: two, the top edge's carried over from the layer above where the
//                                     two temperatures are equal (a workgroup-uniform test).  Four numbers per level.
//   scatter_flux_up_kernel            the emitting Lambertian surface, then K5l's upward walk and sums over two rows.
// A thread holds one point, so the fold's one-exp-per-thread Planck path (successive points of a thread) has nothing to run
// along: every Planck value is the fold's general expression (planck_budget; the calls exist in the default arithmetic only).
// Workspace layout, tiles, scalar loads, the partial slots by tile of the band and the absence of atomics are K5l's.
// pi B at the bottom and the top edge of layer l (K5m's downward walk, K5n's upward one).  LINEAR: the edge that the walk
// reaches first is the far edge of the layer before it where the two temperatures are equal (a workgroup-uniform test), and
// then comes from `carried`, which receives this layer's far edge; otherwise one Planck value per layer.
template <bool LINEAR>
__device__ __forceinline__ void planck_edge_pair(const ScatterFluxArgs& A, double nu, int l, bool down, bool first_layer,
                                                 double& carried, double& Bb, double& Bt) {
#pragma clang fp contract(off)
    if (!LINEAR) {
        Bb = Bt = kPi * planck_budget(nu, A.pa, A.pbkT[l]);
        return;
    }
    const double near = down ? A.pbkT_top[l] : A.pbkT[l], far = down ? A.pbkT[l] : A.pbkT_top[l];
    const bool shared_edge = !first_layer && near == (down ? A.pbkT[l + 1] : A.pbkT_top[l - 1]);
    const double Bn = shared_edge ? carried : kPi * planck_budget(nu, A.pa, near);
    const double Bf = kPi * planck_budget(nu, A.pa, far);
    carried = Bf;
    Bb = down ? Bf : Bn;
    Bt = down ? Bn : Bf;
}

// the emitting Lambertian surface of K5m and K5n at point j: `up` there, under the stack dn = Rs up + Ds
__device__ __forceinline__ double emitting_surface_up(const ScatterFluxArgs& A, long long j, double nu, double Rs, double Ds) {
#pragma clang fp contract(off)
    const double e = A.emissivity ? A.emissivity[j] : A.emissivity_all;
    const double Is = A.I_surface ? A.I_surface[j] : planck_budget(nu, A.pa, A.pbk_surface);
    const double albedo = 1.0 - e;
    return (e * (kPi * Is) + albedo * Ds) / (1.0 - albedo * Rs);
}

// K5m's downward walk; `level` is twostream_down_frame's hook (K5m: nothing; K5p: Tu per level)
template <bool LINEAR, class Level>
__device__ __forceinline__ void scatter_flux_down_walk(const ScatterFluxArgs& A, unsigned threads, long long first, long long count,
                                                       Level level) {
#pragma clang fp contract(off)
    constexpr double D = 1.7320508075688772;        // sqrt(3), rounded
    const int L = A.n_layers;
    double nu = 0.0;
    double B_above = 0.0;                           // LINEAR: pi B at the bottom edge of the layer above
    twostream_down_frame(A, threads, first, count,
        [&](long long j) {
            nu = linspace_at(j, A.n, A.start, A.stop, A.step);
            return A.I_top ? kPi * load_global_f64(A.I_top, j) : 0.0;
        },
        [&](int l, const TwoStreamLayer& lay, double& P, double& Q) {
            double Bb, Bt;
            planck_edge_pair<LINEAR>(A, nu, l, true, l == L - 1, B_above, Bb, Bt);
            P = Bb * lay.Ab; Q = P;
            if (LINEAR) {
                const double d = Bb - Bt;
                const double h = (lay.Ab + 2.0 * lay.R) / (D * (lay.t - lay.tsg)) - lay.T;
                P = Bt * lay.Ab + d * h;
                Q = Bb * lay.Ab - d * h;
            }
            if (lay.empty || lay.conservative || lay.ta == 0.0) P = Q = 0.0;       // (nothing absorbs: nothing emits)
        },
        level);
}

template <bool LINEAR>
__global__ __launch_bounds__(256) void scatter_flux_down_kernel(const ScatterFluxArgs* __restrict__ Ap, long long first,
                                                                long long count) {
    scatter_flux_down_walk<LINEAR>(*Ap, blockDim.x, first, count, [](int, auto&) {});
}

__global__ __launch_bounds__(256) void scatter_flux_up_kernel(const ScatterFluxArgs* __restrict__ Ap, long long tile0,
                                                              long long first, long long count, int slots,
                                                              double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double acc[4 * 2 * (kMaxLayers + 1)];     // [wave][up levels 0..L, down levels 0..L]
    const ScatterFluxArgs& A = *Ap;
    twostream_up_frame<2>(A, blockDim.x, tile0, first, count, slots, partial, acc,
        [&](bool active, long long j, double Rs, double Ds, double) {
            return !active ? 0.0 : emitting_surface_up(A, j, linspace_at(j, A.n, A.start, A.stop, A.step), Rs, Ds);
        });
}

// ----------------------------------------------------------------------------------------
// K5n: radiances through scattering layers (lbl_column_radiance_scatter_dev; the semantics are in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// The two-stream source function technique on K5m's column.  The first pass is scatter_flux_down_kernel<LINEAR> as it
// stands (ScatterRadianceArgs begins with ScatterFluxArgs); scatter_radiance_up_kernel<LINEAR, NV> is K5m's upward walk
// without the sums, and per layer and view one closed-form integral of the source function
//     pi S+-(s) = Bs(s) + (w / 2) sigma(s) +- kap Delta(s),   sigma = F+ + F- - 2 Bs,  Delta = F+ - F-,  kap = w D g mu / 2
// (a + w = 1).  sigma and Delta - 2 c, c = d / (D (t - tsg)), solve y'' = lam^2 y, so each is fixed by its values at the two
// edges of the layer, which the walk has at hand (up and dn at the level below and above):
//     y(s) = y(0) sinh(lam (t - s)) / sinh(lam t) + y(t) sinh(lam s) / sinh(lam t).
// This basis is the linear interpolation at lam = 0 (K5m's den == 0 branch: no switch-over here) and has weights in [0, 1]
// however thick the layer: nothing grows, and no edge value is extrapolated from the other edge.  With u = lam t,
// tau = t / mu, E = exp(-u), Tv = exp(-tau), x = (1 - lam mu) tau the weights against exp(-s / mu) ds / mu are
//     W  = -expm1(-tau)                                                        of 1
//     Wp = (A1 + A2) / (1 + E)                                                 of both sinh ratios together
//          A1 = tau (E - Tv) / x = (x >= 0 ? E : Tv) (-expm1(-|x|)) / |1 - lam mu|   (tau E at x == 0)
//          A2 = -expm1(-(tau + u)) / (1 + lam mu)
//     W1 = ((2 u / -expm1(-2 u)) (A1 / tau) - Tv) / (1 + lam mu)                of sinh(lam s) / sinh(lam t)
// Wp is a sum of positive terms (relative accuracy, also of a thin layer); A1 is smooth through lam mu = 1, no argument of an
// exponential is positive, and W1 - the second divided difference of exp over the nodes 0, -(tau - u), -(tau + u), divided by
// the largest node distance - is good to an absolute rounding error everywhere: it multiplies the difference of the edge
// values, so y(0) Wp + (y(t) - y(0)) W1 tends to (t / mu) y for a thin layer.  The Planck part is the ray kernels'
// (1 - Tv) B_in + g(tau) (B_out - B_in) (linear_source_g), so a column without scatterers (w = 0) gives their expression.
// Both directions run in the one walk: an up view carries I <- Tv I + J, a down view I <- I + C J, C <- Tv C from the surface.
// The layer quantities are recomputed (twostream_layer: the coefficient and the scatterers' numbers read again, 8 bytes and
// about 80 fp64 operations, one sqrt, one exp and two expm1 per point and layer) and not stored: t, lam, w, g, tsg and the two
// Planck values would add 7 numbers per level, 56 bytes written and 56 read per point and layer, about 14 ps of HBM time at
// 8 TB/s against 2 ps of fp64 at the vector rate - and a workspace 2.75 times K5m's.  So the workspace is K5m's.
// One point per thread as K5l/K5m; NV in {1, 2, 4, 8, 16} is the view count rounded up (the views beyond n_views are
// computed with mu = 1 and not stored), so a view's arithmetic does not depend on its neighbours.
// The weights of one view in one layer (K5n, K5o), as above: tau = t / mu, Tv = exp(-tau), Wp and W1, from the layer's
// t, lam, u = lam t, E = exp(-u) and m2 = 2 u / -expm1(-2 u) (1 at u == 0), which do not depend on the view.
struct ViewWeights {
    double tau, Tv, Wp, W1;
};
__device__ __forceinline__ ViewWeights view_weights(double t, double lam, double u, double E, double m2, double mu, double rmu) {
#pragma clang fp contract(off)
    ViewWeights Y;
    const double tau = t * rmu;
    const double Tv = exp_neg_budget(tau);
    const double lm = lam * mu;
    const double q1 = 1.0 - lm, p1 = 1.0 + lm;
    const double x = q1 * tau, ax = fabs(x);
    const double sel = x >= 0.0 ? E : Tv;
    const double em = -expm1(-ax);
    const double A1 = sel * (ax == 0.0 ? tau : em / fabs(q1));
    const double A1t = sel * (ax == 0.0 ? 1.0 : em / ax);
    const double A2 = -expm1(-(tau + u)) / p1;
    Y.tau = tau; Y.Tv = Tv;
    Y.Wp = (A1 + A2) / (1.0 + E);
    Y.W1 = (m2 * A1t - Tv) / p1;
    return Y;
}

// The views of K5n and K5o over the upward walk: I and C per view, per layer what the weights take that does not depend on
// the view, per view its weights and kap = w D g mu / 2, the source integral J from the kernel - source(down, mu, vw, hw, kap),
// grouped as the kernel groups it - and the carry: an up view I <- Tv I + J, a down view I <- I + C J, C <- Tv C.
template <int NV>
struct ViewWalk {
    double I[NV], C[NV];
    template <class Args>
    __device__ __forceinline__ void start(const Args& A, const ViewPart& V, long long j, const UpWalk& w) {
#pragma clang fp contract(off)
        if (A.down_surface) A.down_surface[j] = w.bad ? __builtin_nan("") : w.dn;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            I[v] = V.view_down[v] ? 0.0 : w.up / kPi;
            C[v] = 1.0;
        }
    }
    template <class Source>
    __device__ __forceinline__ void layer(const ViewPart& V, const TwoStreamLayer& lay, Source source) {
#pragma clang fp contract(off)
        constexpr double D = 1.7320508075688772;        // sqrt(3), rounded
        const double t = lay.t, lam = lay.lam, u = lam * t;
        const double E = exp_neg_budget(u);
        const double m2 = u == 0.0 ? 1.0 : fmin(2.0 * u, 2000.0) / -expm1(-2.0 * u);     // (E == 0 beyond 800)
        const double hw = 0.5 * lay.w, Dg = D * lay.g;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const double mu = V.view_mu[v];
            const ViewWeights vw = view_weights(t, lam, u, E, m2, mu, V.view_rmu[v]);
            const double kap = hw * (Dg * mu);
            const double J = source(V.view_down[v] != 0, mu, vw, hw, kap);
            if (V.view_down[v]) {
                I[v] = I[v] + C[v] * (J / kPi);
                C[v] = C[v] * vw.Tv;
            } else
                I[v] = I[v] * vw.Tv + J / kPi;
        }
    }
    // after the walk: the flux up at the top and the views' rows; arrive(I, C) gives a down view's radiance at the surface
    template <class Args, class Arrive>
    __device__ __forceinline__ void finish(const Args& A, const ViewPart& V, long long n, long long j, const UpWalk& w,
                                           Arrive arrive) {
#pragma clang fp contract(off)
        if (A.up_top) A.up_top[j] = w.up;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (v < V.n_views) {
                const double r = V.view_down[v] ? arrive(I[v], C[v]) : I[v];
                V.radiance[(long long)v * n + j] = w.bad ? __builtin_nan("") : r;
            }
        }
    }
};

template <bool LINEAR, int NV>
__global__ __launch_bounds__(256) void scatter_radiance_up_kernel(const ScatterRadianceArgs* __restrict__ Ap, long long first,
                                                                  long long count) {
#pragma clang fp contract(off)
    const ScatterRadianceArgs& A = *Ap;
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    const long long j = first + q;
    constexpr double D = 1.7320508075688772;        // sqrt(3), rounded
    const double nu = linspace_at(j, A.n, A.start, A.stop, A.step);
    UpWalk w;
    twostream_up_start(A, q, j, w, [&](const UpWalk& s) { return emitting_surface_up(A, j, nu, s.Rs, s.Ds); });
    ViewWalk<NV> views;
    views.start(A, A.views, j, w);
    double B_below = 0.0;                           // LINEAR: pi B at the top edge of the layer below
    twostream_up_layers(A, j, w, [&](int l, const TwoStreamLayer& lay, double) {
        double Bb, Bt;
        planck_edge_pair<LINEAR>(A, nu, l, false, l == 0, B_below, Bb, Bt);
        if (lay.empty) return;
        const double c2 = LINEAR && lay.ta != 0.0 ? (2.0 * (Bb - Bt)) / (D * (lay.t - lay.tsg)) : 0.0;
        const double sig0 = (w.up + w.dn) - 2.0 * Bt, sigt = (w.upB + w.dnB) - 2.0 * Bb;      // top edge, bottom edge
        const double del0 = w.up - w.dn, delt = w.upB - w.dnB;
        views.layer(A.views, lay, [&](bool down, double, const ViewWeights& vw, double hw, double kap) {
            const double Wp = vw.Wp, W1 = vw.W1;
            const double Wt = -expm1(-vw.tau);
            const double gl = lbl::linear_source_g(vw.tau, vw.Tv);
            const double part = c2 * (Wt - Wp);
            if (down)
                return (Bt * Wt + gl * (Bb - Bt)) + hw * (sigt * Wp + (sig0 - sigt) * W1)
                       - kap * (part + (delt * Wp + (del0 - delt) * W1));
            return (Bb * Wt + gl * (Bt - Bb)) + hw * (sig0 * Wp + (sigt - sig0) * W1)
                   + kap * (part + (del0 * Wp + (delt - del0) * W1));
        });
    });
    const double Itop = A.I_top ? load_global_f64(A.I_top, j) : 0.0;
    views.finish(A, A.views, A.n, j, w, [&](double I, double C) { return I + C * Itop; });
}

// ----------------------------------------------------------------------------------------
// K5o: scattered sunlight along a view (lbl_column_beam_radiance_dev; the semantics are in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// K5n's technique on K5l's column with one beam.  The first pass is twostream_down_kernel<1> as it stands (BeamViewArgs
// begins with TwoStreamArgs; the workspace is K5l's, quantity 4 the beam's flux Fd_i through the horizontal);
// beam_view_kernel<NV> is K5l's upward walk without the sums - its surface, up and dn per level, the three spectra - and per
// layer and view the closed-form integral of
//     pi S+-(s) = (w / 2) sigma(s) +- kap Delta(s) + (w / (2 D m)) (1 -+ 3 g mu m) Fd exp(-s / m),   kap = w D g mu / 2,
// Fd = Fd_(l+1) at the layer's top.  sigma = F+ + F- and Delta = F+ - F- less their particular parts (2 Cp - u) Fd exp(-s / m)
// and u Fd exp(-s / m) (K5l's Cp and u = Cp - Cm, restated here: with the moved m and Tdm at the pole lam m = 1, so that the
// edge values are those the adding used) solve y'' = lam^2 y: K5n's sinh-ratio basis between the edge values and its weights
// Wp and W1 (view_weights).  What multiplies Fd exp(-s / m) is gathered in one bracket per view and integrates to
//     Xu = -expm1(-(tau + t / m)) / (1 + mu / m)                                       (up view,   against exp(-s / mu))
//     Xd = (x >= 0 ? Tdm : Tv) (-expm1(-|x|)) / |1 - mu / m|,  x = (1 - mu / m) tau    (down view, against exp(-(t - s) / mu);
//                                                                                       tau Tv at x == 0: smooth through mu == m)
// No exponential has a positive argument and no branch fires at lam == 0 or den == 0.  The layer is recomputed for K5n's
// reason (the workspace would grow from 5 to 11 numbers per level).  One point per thread; NV as K5n.
template <int NV>
__global__ __launch_bounds__(256) void beam_view_kernel(const BeamViewArgs* __restrict__ Ap, long long first, long long count) {
#pragma clang fp contract(off)
    const BeamViewArgs& A = *Ap;
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    const long long j = first + q;
    constexpr double D = 1.7320508075688772;        // sqrt(3), rounded
    UpWalk w;
    double F0 = 0.0;
    // K5l's surface (twostream_up_kernel)
    twostream_up_start(A, q, j, w, [&](const UpWalk& s) {
        F0 = s.ws(4, 0);
        const double e = A.emissivity ? A.emissivity[j] : A.emissivity_all;
        const double albedo = 1.0 - e;
        return (albedo * (s.Ds + F0)) / (1.0 - albedo * s.Rs);
    });
    if (A.direct_surface) A.direct_surface[j] = w.bad ? __builtin_nan("") : F0;
    ViewWalk<NV> views;
    views.start(A, A.views, j, w);
    twostream_up_layers(A, j, w, [&](int l, const TwoStreamLayer& lay, double) {
        const double Fd = w.ws(4, l + 1);
        if (lay.empty) return;
        const double t = lay.t, lam = lay.lam;
        // the beam's terms, K5l's (twostream_down_kernel)
        double tm = t * A.slant[0][l];
        double m = A.m[0][l], rm = A.slant[0][l];
        const double g3 = 0.5 * (1.0 - (D * lay.g) * m), g4 = 1.0 - g3;
        const double a2 = lay.g1 * g3 + lay.g2 * g4;
        if (fabs(1.0 - lam * m) < 1e-6) {
            m = (1.0 - 1e-6) / lam;
            tm = t / m;
            rm = 1.0 / m;
        }
        const double Tdm = exp_neg_budget(tm);
        const double pole = (1.0 - lam * m) * (1.0 + lam * m);
        const double Cp = (lay.w * (g3 - a2 * m)) / pole;
        const double cu = (lay.w * (1.0 + (lay.Da * (g4 - g3)) * m)) / pole;
        const double cs = Cp + (Cp - cu);               // Cp + Cm
        const double Fb = Fd * Tdm;                     // the in-layer beam term at the bottom edge
        const double sig0 = (w.up + w.dn) - cs * Fd, sigt = (w.upB + w.dnB) - cs * Fb;      // top edge, bottom edge
        const double del0 = (w.up - w.dn) - cu * Fd, delt = (w.upB - w.dnB) - cu * Fb;
        const double g3x = 3.0 * lay.g;
        const double hs = (0.5 * lay.w) / D;
        views.layer(A.views, lay, [&](bool down, double mu, const ViewWeights& vw, double hw, double kap) {
            const double tau = vw.tau, Tv = vw.Tv, Wp = vw.Wp, W1 = vw.W1;
            const double mr = mu * rm;
            if (down) {
                const double qb = 1.0 - mr;
                const double xb = qb * tau, axb = fabs(xb);
                const double Xd = (xb >= 0.0 ? Tdm : Tv) * (axb == 0.0 ? tau : -expm1(-axb) / fabs(qb));
                const double beam = (hw * cs - kap * cu) + hs * (rm + g3x * mu);
                return (hw * (sigt * Wp + (sig0 - sigt) * W1) - kap * (delt * Wp + (del0 - delt) * W1)) + (Fd * Xd) * beam;
            }
            const double Xu = -expm1(-(tau + tm)) / (1.0 + mr);
            const double beam = (hw * cs + kap * cu) + hs * (rm - g3x * mu);
            return (hw * (sig0 * Wp + (sigt - sig0) * W1) + kap * (del0 * Wp + (delt - del0) * W1)) + (Fd * Xu) * beam;
        });
    });
    views.finish(A, A.views, A.n, j, w, [](double I, double) { return I; });
}

// ----------------------------------------------------------------------------------------
// K5p: Jacobians of the outgoing flux through scattering layers (lbl_column_jacobian_scatter_dev; the semantics and the
// derivation are in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// The layer relations are linear in the fluxes, so F = up_L answers a change of one layer through two weights: with the stack
// above level l + 1 (Rs', Tu' from the downward walk) and the stack below level l (A_l, built here going up)
//     w1 = Tu' / ((1 - R Rs') - T^2 A_l Rs' / (1 - R A_l)),   w2 = w1 T A_l / (1 - R A_l)
//     dF = w1 (dT up_l + dR dn_(l+1) + dP) + w2 (dT dn_(l+1) + dR up_l + dQ).
//   scatter_jacobian_down_kernel<LINEAR>  K5m's downward walk (scatter_flux_down_walk: the same code, the same bits) with
//                                         Tu_L = 1, Tu_i = Tu_(i+1) U1_(i+1) as a fifth number per level.
//   scatter_jacobian_up_kernel<LINEAR>    the surface and its two rows, then bottom to top per layer: the layer recomputed as
//                                         K5n does (twostream_layer), p dX/dp and q dX/dq of X = R, T, Ab and h in closed form
//                                         (p = D ta, q = D (t - tsg); nothing is divided by sqrt(ta) or sqrt(q)), the two
//                                         weights, the layer's rows and its terms (jacobian_terms).
// One point per thread.  A workgroup takes the tiles of its partial slot in ascending order, as K5l's upward kernel does; per
// tile every row is one wave_sum whose result lane 0 of each wave stores at acc[wave][row], the row order being jac's: F,
// dF/dT_s, dF/de, L d ln tau, NT L temperatures (NT per layer), n_scat x L amounts, the terms.  Every row is stored once per
// tile; then the four waves are added in a fixed order into the tile's slot.  4 x kScatterJacMaxSlots doubles of LDS
// (45,152 bytes).  A lane beyond the pass's points computes the tile's first point again and adds zeros.
// pi B and pi dB/dT at the bottom and top edge of layer l on the way up; LINEAR: the bottom edge is the top edge of the layer
// below where the two temperatures are equal (a workgroup-uniform test), and then comes from cB, cdB
template <bool LINEAR>
__device__ __forceinline__ void planck_edge_pair_dT(const ScatterJacArgs& A, double nu, double pa_n, int l, double& cB,
                                                    double& cdB, double& Bb, double& Bt, double& dBb, double& dBt) {
#pragma clang fp contract(off)
    double d;
    if (!LINEAR) {
        Bb = Bt = kPi * fold_planck<false, true>(false, nu, nu, pa_n, A.pbkT[l], 0.0, A.rT[l], &d);
        dBb = dBt = kPi * d;
        return;
    }
    if (l > 0 && A.pbkT[l] == A.pbkT_top[l - 1]) {
        Bb = cB; dBb = cdB;
    } else {
        Bb = kPi * fold_planck<false, true>(false, nu, nu, pa_n, A.pbkT[l], 0.0, A.rT[l], &d);
        dBb = kPi * d;
    }
    Bt = kPi * fold_planck<false, true>(false, nu, nu, pa_n, A.pbkT_top[l], 0.0, A.rT_top[l], &d);
    dBt = kPi * d;
    cB = Bt; cdB = dBt;
}

// p dX/dp and q dX/dq of a layer's R, T and Ab, p = D ta = r^2, q = D (t - tsg) = s^2: with x = r s, E = exp(-x),
// Gam = (s - r) / (s + r), G = r s / (s + r)^2 = (1 - Gam^2) / 4, oE = 1 - E^2 and N = 1 - Gam^2 E^2 = 4 G + Gam^2 oE
//     p R_p = G (-oE (1 + Gam^2 E^2) + 4 x Gam E^2) / N^2      q R_q = G (oE (1 + Gam^2 E^2) + 4 x Gam E^2) / N^2
//     p T_p = 2 G E (Gam oE - x (1 + Gam^2 E^2)) / N^2         q T_q = -2 G E (Gam oE + x (1 + Gam^2 E^2)) / N^2
//     p Ab_p = G (oE + 2 x E) / (1 + Gam E)^2                  q Ab_q = -G (oE - 2 x E) / (1 + Gam E)^2
// (G / N <= 1 / 4: no quotient grows in a thin layer).  den == 0 (and N == 0): the branch's R = y / (1 + y), T = 1 / (1 + y),
// y = (p + q) / 2, Ab = 0.
struct TwoStreamLayerD {
    double pR, qR, pT, qT, pAb, qAb;
};
__device__ __forceinline__ TwoStreamLayerD twostream_layer_partials(const TwoStreamLayer& lay, double p, double q) {
#pragma clang fp contract(off)
    TwoStreamLayerD Y;
    const double r = sqrt(p), s = sqrt(q);
    const double sr = s + r;
    const double Gam = (s - r) / sr;
    const double G = (r / sr) * (s / sr);
    const double x = r * s;
    const double E = exp_neg_budget(x);
    const double oE = -expm1(-2.0 * x);
    const double GE = Gam * E;
    const double N = 4.0 * G + (Gam * Gam) * oE;
    if (lay.conservative || !(N > 0.0)) {
        const double i1 = 1.0 / (1.0 + 0.5 * (p + q));
        Y.pR = (0.5 * p) * (i1 * i1); Y.qR = (0.5 * q) * (i1 * i1);
        Y.pT = -Y.pR; Y.qT = -Y.qR;
        Y.pAb = 0.0; Y.qAb = 0.0;
        return Y;
    }
    const double gN = (G / N) / N;
    const double m = 1.0 + GE * GE;
    const double xE = x * E;
    Y.pR = gN * (4.0 * (xE * GE) - oE * m);
    Y.qR = gN * (4.0 * (xE * GE) + oE * m);
    Y.pT = (2.0 * gN) * (GE * oE - xE * m);
    Y.qT = -(2.0 * gN) * (GE * oE + xE * m);
    const double S = G / ((1.0 + GE) * (1.0 + GE));
    Y.pAb = S * (oE + 2.0 * xE);
    Y.qAb = -(S * (oE - 2.0 * xE));
    return Y;
}

// (K5d's, defined with the Jacobian kernels below)
template <int NP, class Args, class Add>
__device__ __forceinline__ void jacobian_terms(const Args& A, int l, long long j, bool active, const double (&Gd)[NP],
                                               int slot0, Add add);

template <bool LINEAR>
__global__ __launch_bounds__(256) void scatter_jacobian_down_kernel(const ScatterJacArgs* __restrict__ Ap, long long first,
                                                                    long long count) {
#pragma clang fp contract(off)
    const int L = Ap->n_layers;
    double Tu = 1.0;
    scatter_flux_down_walk<LINEAR>(*Ap, blockDim.x, first, count, [&](int i, auto& ws) {
        if (i < L) Tu = Tu * ws(2, i + 1);
        ws(4, i) = Tu;
    });
}

template <bool LINEAR>
__global__ __launch_bounds__(256) void scatter_jacobian_up_kernel(const ScatterJacArgs* __restrict__ Ap, long long tile0,
                                                                  long long first, long long count, int slots,
                                                                  double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int NT = LINEAR ? 2 : 1;
    constexpr int kSlot = kScatterJacMaxSlots;
    constexpr double D = 1.7320508075688772;        // sqrt(3), rounded
    __shared__ double acc[4 * kSlot];               // [wave][row of jac]
    const ScatterJacArgs& A = *Ap;
    const int L = A.n_layers, C = A.n_scat;
    const int nv = scatter_jacobian_slots(NT, L, C, A.n_terms);
    const int row_T = 3 + L, row_scat = row_T + NT * L, row_term = row_scat + C * L;
    double* const my = acc + (threadIdx.x >> 6) * kSlot;
    const bool lane0 = (threadIdx.x & 63) == 0;
    const double nan = __builtin_nan("");
    const long long tiles = (count + kTwoStreamTile - 1) / kTwoStreamTile;
    // (the loop bound is uniform over the workgroup: every lane takes part in the wave reductions)
    for (long long tile = blockIdx.x; tile < tiles; tile += slots) {
        const long long q0 = tile * kTwoStreamTile;
        const bool active = q0 + threadIdx.x < count;
        const long long qq = active ? q0 + threadIdx.x : q0;
        const long long j = first + qq;
        auto add = [&](int slot, double v) {
            const double s = wave_sum(active ? nan_to_num(v) : 0.0);
            if (lane0) my[slot] = s;
        };
        // (jacobian_terms hands over a value that is masked and nan_to_num'ed already)
        auto add_term = [&](int slot, double v) {
            const double s = wave_sum(v);
            if (lane0) my[slot] = s;
        };
        const double nu = linspace_at(j, A.n, A.start, A.stop, A.step);
        const double pa_n = A.pa * (nu * nu * nu);
        // the surface: up_0 = (e Es + (1 - e) Ds_0) / c0, c0 = 1 - (1 - e) Rs_0
        UpWalk w;
        twostream_up_start(A, qq, j, w, [&](const UpWalk& s) { return emitting_surface_up(A, j, nu, s.Rs, s.Ds); });
        const bool bad = w.bad;
        const double e = A.emissivity ? A.emissivity[j] : A.emissivity_all;
        {
            double dBs = 0.0;
            const double Is = A.I_surface ? A.I_surface[j]
                                          : fold_planck<false, true>(false, nu, nu, pa_n, A.pbk_surface, 0.0, A.r_surface_T, &dBs);
            const double gs = w.ws(4, 0) / (1.0 - (1.0 - e) * w.Rs);
            add(1, bad ? nan : (gs * e) * (kPi * dBs));
            add(2, bad ? nan : gs * (kPi * Is - w.dn));
        }
        double Al = 1.0 - e;                            // what the stack below level l reflects
        double cB = 0.0, cdB = 0.0;                     // LINEAR: pi B and pi dB/dT at the top edge of the layer below
        twostream_up_layers(A, j, w, [&](int l, const TwoStreamLayer& lay, double k) {
            const double depth = A.depth[l];
            const double upB = w.upB, dn = w.dn, Rs = w.Rs;
            const double R = lay.R, T = lay.T, Ab = lay.Ab;
            const double TA = (T * Al) / (1.0 - R * Al);
            const double w1 = w.ws(4, l + 1) / ((1.0 - R * Rs) - (T * TA) * Rs);
            const double w2 = w1 * TA;
            Al = R + T * TA;
            double Bb, Bt, dBb, dBt;
            planck_edge_pair_dT<LINEAR>(A, nu, pa_n, l, cB, cdB, Bb, Bt, dBb, dBt);
            const double tq = lay.t - lay.tsg;
            double pF = 0.0, qF = 0.0, gT[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) gT[i] = 0.0;
            if (!lay.empty) {
                const TwoStreamLayerD d = twostream_layer_partials(lay, D * lay.ta, D * tq);
                double pP = 0.0, qP = 0.0, pQ = 0.0, qQ = 0.0;
                if (!(lay.conservative || lay.ta == 0.0)) {        // (else nothing absorbs: P = Q = 0)
                    if (LINEAR) {
                        const double dq = D * tq;
                        const double h = (Ab + 2.0 * R) / dq - T;
                        const double ph = (d.pAb + 2.0 * d.pR) / dq - d.pT;
                        const double qh = ((d.qAb + 2.0 * d.qR) - (Ab + 2.0 * R)) / dq - d.qT;
                        const double dB = Bb - Bt;
                        pP = Bt * d.pAb + dB * ph; pQ = Bb * d.pAb - dB * ph;
                        qP = Bt * d.qAb + dB * qh; qQ = Bb * d.qAb - dB * qh;
                        gT[0] = (w1 * h + w2 * (Ab - h)) * dBb;
                        gT[NT - 1] = (w1 * (Ab - h) + w2 * h) * dBt;
                    } else {
                        pP = pQ = Bb * d.pAb;
                        qP = qQ = Bb * d.qAb;
                        gT[0] = ((w1 + w2) * Ab) * dBb;
                    }
                }
                pF = w1 * ((d.pT * upB + d.pR * dn) + pP) + w2 * ((d.pT * dn + d.pR * upB) + pQ);
                qF = w1 * ((d.qT * upB + d.qR * dn) + qP) + w2 * ((d.qT * dn + d.qR * upB) + qQ);
            }
            // per unit of ta and of t - tsg: dF/dta = fa + fq, dF/dts = fq, dF/dtsg = -fq
            const double fa = lay.ta > 0.0 ? pF / lay.ta : 0.0;
            const double fq = tq > 0.0 ? qF / tq : 0.0;
            double Gd[1] = {depth * (fa + fq)};
            double dtau = k * Gd[0];
            if (bad) {
                Gd[0] = dtau = nan;
#pragma unroll
                for (int i = 0; i < NT; ++i) gT[i] = nan;
            }
            if (active && A.ln_tau_spec) A.ln_tau_spec[(long long)l * A.n + j] = dtau;
            add(3 + l, dtau);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                if (active && A.T_spec) A.T_spec[(long long)(NT * l + i) * A.n + j] = gT[i];
                add(row_T + NT * l + i, gT[i]);
            }
#pragma unroll
            for (int c = 0; c < kMaxScatterers; ++c) {          // (n_scat is uniform over the workgroup)
                if (c < C) {
                    const double v = A.amount[c][l] * (w.al[c] * (fa + fq) + (w.si[c] - w.et[c]) * fq);
                    add(row_scat + c * L + l, bad ? nan : v);
                }
            }
            jacobian_terms<1>(A, l, j, active, Gd, row_term, add_term);
        });
        if (active && A.up_top) A.up_top[j] = w.up;
        add(0, w.up);
        tile_slot_add<kSlot>(partial + ((tile0 + tile) % slots) * nv, acc, nv, blockDim.x);
    }
}

// ----------------------------------------------------------------------------------------
// K5i: linear-in-optical-depth Planck source (lbl_column_flux_linear_dev, lbl_ray_radiance_linear_dev; the semantics are in
// include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// K5g's two kernels with a Planck function that runs linearly in optical depth through a layer or segment, from Ba = B(Ta)
// where the light enters to Bb = B(Tb) where it leaves:
//     I <- t I + (1 - t) Ba + g(tau) (Bb - Ba),   g(tau) = 1 - (1 - t) / tau   (linear_source_g, lbl_linear_source.h).
// The first two terms are fold_update's value and the third is added to it, so with Ta == Tb (Bb - Ba == 0, g finite) a step
// returns fold_update's bits, and both kernels K5g's.  Per point and step: a second Planck value, from a second exp per
// thread on the fast path (whose test covers every edge temperature of the call), and per angle or ray one g.

// surface_flux_kernel with linear_step: going down the light enters a layer at its top edge and leaves at its bottom edge,
// going up the other way round.  Everything else - Is in LDS, the surface, the level slots, the partials - is K5g's.
// (the second launch bound: 4 points per thread take 135-163 registers with one to four angles, three waves per SIMD, and
// 171-195 with five to eight, two waves; K5g's bounds - 4 waves with one angle, 3 up to seven - leave 5, 4 and 12 spilled
// registers at one, five and six angles.  g without a branch: linear_source_g)
template <int NP, int NA> constexpr int linear_flux_waves() { return NP == 1 ? 1 : NA <= 4 ? 3 : 2; }
template <int NP, int NA>
__global__ __launch_bounds__(256, (linear_flux_waves<NP, NA>())) void linear_flux_kernel(const LinearFluxArgs* __restrict__ Ap, long long lo0, long long n0,
                                                          long long lo1, long long n1, double* __restrict__ partial) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    constexpr int kSlot = 2 * (kMaxLayers + 1);
    __shared__ double acc[4 * kSlot];            // [wave][up levels 0..L, down levels 0..L]
    __shared__ double source[NP * 256];          // [point][thread]: Is, from before the downward walk to the surface
    const LinearFluxArgs& A = *Ap;
    const int L = A.n_layers;
    const int nv = 2 * (L + 1);
    for (int t = threadIdx.x; t < 4 * kSlot; t += blockDim.x) acc[t] = 0.0;
    __syncthreads();
    double* my = acc + (threadIdx.x >> 6) * kSlot;
    const bool lane0 = (threadIdx.x & 63) == 0;
    const long long total = n0 + n1;
    const long long stride = (long long)gridDim.x * blockDim.x * NP;
    // (the loop bound is uniform over the workgroup: every lane takes part in the wave reductions, idle lanes on a valid point)
    for (long long q0 = (long long)blockIdx.x * blockDim.x * NP; q0 < total; q0 += stride) {
        const long long q = q0 + (long long)threadIdx.x * NP;
        const bool active = q < total;
        const long long j = !active ? lo0 : (q < n0 ? lo0 + q : lo1 + (q - n0));
        double nu[NP], pa_n[NP], I[NA][NP];
        column_points<NP>(A, j, nu, pa_n);
        const bool fast = fold_fast_path<NP>(A, nu, active);
        auto level = [&](int slot, double* spec, double* spec2 = nullptr) __attribute__((always_inline)) {
            double s = 0.0;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double f = angle_sum<NA>(A, [&](int k) { return I[k][p]; });
                if (spec && active) spec[j + p] = f;
                if (spec2 && active) spec2[j + p] = f;
                s += active ? nan_to_num(f) : 0.0;
            }
            s = wave_sum(s);
            if (lane0) my[slot] += s;
        };
        // (entered at pbkT_a, left at pbkT_b)
        auto layer = [&](auto fast_tag, int l, vec v, double pbkT_a, double pbkT_b) __attribute__((always_inline)) {
            constexpr bool FAST = decltype(fast_tag)::value;
            const double depth = A.depth[l];
            linear_step<FAST, NP>(nu, pa_n, pbkT_a, pbkT_b, v, [&](int p, double kp, double Ba, double dB) __attribute__((always_inline)) {
                const double tau = kp * depth;
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    const double tk = tau * A.rmu[k];
                    I[k][p] = linear_update<FAST>(tk, exp_neg_budget(tk), I[k][p], Ba, dB);
                }
            });
        };
        auto walk = [&](auto fast_tag) __attribute__((always_inline)) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
                source[p * 256 + threadIdx.x] = A.I_surface ? A.I_surface[j + p] : planck_budget(nu[p], A.pa, A.pbk_surface);
            // downward: I_L = I_top or 0; level l after layer l
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double It = A.I_top ? A.I_top[j + p] : 0.0;
#pragma unroll
                for (int k = 0; k < NA; ++k) I[k][p] = It;
            }
            level(L + 1 + L, L == 0 ? A.down_surface : nullptr);
            vec cur = L > 0 ? load_points<NP>(A.abs_coef[L - 1], j) : (vec)(0.0);
            for (int l = L - 1; l >= 0; --l) {
                const vec nxt = l > 0 ? load_points<NP>(A.abs_coef[l - 1], j) : cur;
                layer(fast_tag, l, cur, A.pbkT_top[l], A.pbkT[l]);
                level(L + 1 + l, l == 0 ? A.down_surface : nullptr);
                cur = nxt;
            }
            // the surface: I_up[0] = e Is + (1 - e) R, in place
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double e = A.emissivity ? A.emissivity[j + p] : A.emissivity_all;
                const double Is = source[p * 256 + threadIdx.x];
                const double diffuse = angle_sum<NA>(A, [&](int k) { return I[k][p]; }) / A.w_sum;
#pragma unroll
                for (int k = 0; k < NA; ++k) I[k][p] = surface_leaving(e, Is, A.reflection == 0 ? diffuse : I[k][p]);
            }
            // upward: level l + 1 after layer l
            level(0, A.up_surface, L == 0 ? A.up_top : nullptr);
            cur = L > 0 ? load_points<NP>(A.abs_coef[0], j) : (vec)(0.0);
            for (int l = 0; l < L; ++l) {
                const vec nxt = l + 1 < L ? load_points<NP>(A.abs_coef[l + 1], j) : cur;
                layer(fast_tag, l, cur, A.pbkT[l], A.pbkT_top[l]);
                level(l + 1, l + 1 == L ? A.up_top : nullptr);
                cur = nxt;
            }
        };
        if constexpr (NP > 1) {
            if (fast) walk(std::true_type{});
            else walk(std::false_type{});
        } else {
            walk(std::false_type{});
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nv; t += blockDim.x)
        partial[(long long)blockIdx.x * nv + t] = (acc[t] + acc[kSlot + t]) + (acc[2 * kSlot + t] + acc[3 * kSlot + t]);
}

// ray_surface_walks with LINEAR: markers, the diffuse start term and the prefetch are K5g's; a ray's operations are the
// same in every bundle size.
template <int NP, int RB>
__global__ __launch_bounds__(256) void linear_ray_kernel(const LinearRayArgs* __restrict__ Ap, long long lo0, long long n0,
                                                         long long lo1, long long n1, int order_first) {
    ray_surface_walks<NP, RB, true>(Ap, blockDim.x, lo0, n0, lo1, n1, order_first);
}

// ----------------------------------------------------------------------------------------
// What the column Jacobian kernels (K5d, K5h, K5j) share.  K5h with a black surface returns K5d's bits and K5j with equal
// edge temperatures K5h's because the operations in question are the same code, not copies of it.  Every body sets
// fp contract(off) itself: the pragma ends with a function's body.
// ----------------------------------------------------------------------------------------
// A layer's terms: term_k Gd per point, Gd = depth G, summed into the terms' slots, which begin at slot0 (in K5h and K5j
// walks 2 and 3 each add their leg)
template <int NP, class Args, class Add>
__device__ __forceinline__ void jacobian_terms(const Args& A, int l, long long j, bool active, const double (&Gd)[NP],
                                               int slot0, Add add) {
#pragma clang fp contract(off)
    for (int t = A.layer_term[l]; t < A.layer_term[l + 1]; ++t) {
        const f64v<NP> km = load_points<NP>(A.term_k[t], j);
        double s = 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p) s += active ? nan_to_num(km[p] * Gd[p]) : 0.0;
        add(slot0 + A.term_slot[t], s);
    }
}

// One point's values of layer l into the spectra and into the thread's sums: d ln tau and NT temperature values (the
// layer's: 1; K5j, its bottom and top edge: 2; T_spec holds NT rows per layer).  `store`: this walk stores (K5d's only walk,
// walk 2 of K5h and K5j); otherwise it adds to what the same thread stored (their walk 3).  T_spec names the temperature
// spectra's member of the argument block: the pointers are read here, behind `active`, as a kernel's own body would read
// them - handed over as values they are loaded ahead of every step and cost up to 33 registers (K5j) and a wave (K5d, K5j).
template <int NT, class Args, class Owner>
__device__ __forceinline__ void jacobian_emit(bool store, bool active, const Args& A, double* Owner::*T_spec, int l, long long j,
                                              int p, double dtau, const double (&gT)[NT], double& s_tau, double (&s_T)[NT]) {
#pragma clang fp contract(off)
    if (active && A.ln_tau_spec) {
        double* o = A.ln_tau_spec + (long long)l * A.n + j + p;
        *o = store ? dtau : *o + dtau;
    }
    if (active && A.*T_spec) {
        double* o = A.*T_spec + (long long)(NT * l) * A.n + j + p;
#pragma unroll
        for (int r = 0; r < NT; ++r) {
            *o = store ? gT[r] : *o + gT[r];
            o += A.n;
        }
    }
    s_tau += active ? nan_to_num(dtau) : 0.0;
#pragma unroll
    for (int r = 0; r < NT; ++r) s_T[r] += active ? nan_to_num(gT[r]) : 0.0;
}

// K5d's downward step through layer l (the derivation is at column_jacobian_kernel): I holds D, Ak the transmittance A to
// the top.  HEAD: the band values ahead of the layers' (K5d: 2, K5h: 3); STORE: jacobian_emit's `store`.
template <bool FAST, int HEAD, bool STORE, int NP, int NA, class Add>
__device__ __forceinline__ void jacobian_down_step(const JacArgs& A, int L, int l, f64v<NP> v, long long j, bool active,
                                                   const double (&nu)[NP], const double (&pa_n)[NP], double (&I)[NA][NP],
                                                   const double (&Imax)[NA][NP], double (&Ak)[NA][NP], Add add) {
#pragma clang fp contract(off)
    const double pbkT = A.pbkT[l], depth = A.depth[l], rT = A.rT[l];
    double E0 = 0.0;
    if (FAST) E0 = exp_clamped(nu[0] * pbkT);
    double s_tau = 0.0, s_T[1] = {0.0}, Gd[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const double tau = v[p] * depth;
        double dB;
        const double B = fold_planck<FAST, true>(p == 0, nu[p], nu[0], pa_n[p], pbkT, E0, rT, &dB);
        double G = 0.0, gT[1] = {0.0};
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const double tr = exp_neg_budget(tau * A.rmu[k]);
            const double At = Ak[k][p] * tr;
            const double g = fmin(fmax(Ak[k][p] * B + I[k][p], -(At * Imax[k][p])), At * B);
            G = fma(A.wrmu[k], g, G);
            const double a1 = Ak[k][p] * (1.0 - tr);
            gT[0] = fma(A.w[k], a1 * dB, gT[0]);
            I[k][p] = I[k][p] + a1 * B;              // D_(l-1) = D_l + A_l (1 - t_l) B_l
            Ak[k][p] = At;                           // A_(l-1) = A_l t_l
        }
        Gd[p] = depth * G;
        jacobian_emit<1>(STORE, active, A, &JacArgs::T_spec, l, j, p, tau * G, gT, s_tau, s_T);
    }
    add(HEAD + l, s_tau);
    add(HEAD + L + l, s_T[0]);
    jacobian_terms<NP>(A, l, j, active, Gd, HEAD + 2 * L, add);
}

// F_top into slot 0; then I becomes D = -I_top and A = 1: the state the downward derivative walk starts from
template <int NP, int NA, class Add>
__device__ __forceinline__ void flux_top_turn(const ColumnRT& A, bool active, double (&I)[NA][NP], double (&Ak)[NA][NP],
                                              Add add) {
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        s += active ? nan_to_num(angle_sum<NA>(A, [&](int k) { return I[k][p]; })) : 0.0;
#pragma unroll
        for (int k = 0; k < NA; ++k) { I[k][p] = -I[k][p]; Ak[k][p] = 1.0; }
    }
    add(0, s);
}

// The reflecting surface of K5h and K5j between walk 1 (downward from the top, which `start` sets up: I_L = I_top or 0,
// Dmax the same, Ttot = 1) and walk 2.  `turn`: dF/dT_s = e sum_k W_k Ttot_k dBs/dT and dF/de = sum_k W_k Ttot_k (Is - R_k)
// are complete here (slots 1 and 2, e_spec); then the state becomes walk 2's: I_up[0] = e Is + (1 - e) R, Imax, the weight
// Qf of what is seen through the surface in Ak, C = 1 and D' = -D.
template <int NP, int NA>
struct ReflectingSurfaceTurn {
    static __device__ __forceinline__ void start(const SurfaceJacArgs& A, long long j, double (&I)[NA][NP], double (&Dm)[NA][NP],
                                                 double (&Ak)[NA][NP]) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double It = A.I_top ? A.I_top[j + p] : 0.0;
#pragma unroll
            for (int k = 0; k < NA; ++k) { I[k][p] = It; Dm[k][p] = It; Ak[k][p] = 1.0; }
        }
    }
    template <class Add>
    static __device__ __forceinline__ void turn(const SurfaceJacArgs& A, long long j, bool active, const double (&nu)[NP],
                                                const double (&pa_n)[NP], double (&I)[NA][NP], double (&Imax)[NA][NP],
                                                double (&Ak)[NA][NP], double (&Ck)[NA][NP], double (&Dp)[NA][NP], Add add) {
#pragma clang fp contract(off)
        double s_Ts = 0.0, s_e = 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double e = A.emissivity ? A.emissivity[j + p] : A.emissivity_all;
            double dBs = 0.0;
            const double Is = A.I_surface ? A.I_surface[j + p]
                                          : fold_planck<false, true>(false, nu[p], nu[p], pa_n[p], A.pbk_surface, 0.0,
                                                                     A.r_surface_T, &dBs);
            const double edBs = e * dBs;
            const double diffuse = angle_sum<NA>(A, [&](int k) { return I[k][p]; }) / A.w_sum;
            const double Tdiffuse = angle_sum<NA>(A, [&](int k) { return Ak[k][p]; }) / A.w_sum;
            const double dTs = angle_sum<NA>(A, [&](int k) { return Ak[k][p] * edBs; });
            const double de = angle_sum<NA>(A, [&](int k) { return Ak[k][p] * (Is - (A.reflection == 0 ? diffuse : I[k][p])); });
            if (active && A.e_spec) A.e_spec[j + p] = de;
            s_Ts += active ? nan_to_num(dTs) : 0.0;
            s_e += active ? nan_to_num(de) : 0.0;
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const double D = I[k][p];
                I[k][p] = surface_leaving(e, Is, A.reflection == 0 ? diffuse : D);
                Imax[k][p] = I[k][p];
                Ak[k][p] = (1.0 - e) * (A.reflection == 0 ? Tdiffuse : Ak[k][p]);
                Ck[k][p] = 1.0;
                Dp[k][p] = -D;
            }
        }
        add(1, s_Ts);
        add(2, s_e);
    }
};

// K5d: K5c's upward fold, keeping per angle only the radiance I and its running maximum Imax over the levels; then a
// downward pass that re-reads k_l and recomputes B_l as K5c's does, and keeps per angle the transmittance A to the top and
// D = E - I_top, E the emission of the layers above that reaches the top.  Then
//     A_l t_l (B_l - I_l) = A_l B_l + E_l - I_top = A_l B_l + D_l,
// clamped to [-A_l t_l Imax, A_l t_l B_l] (both bounds exact for non-negative sources): where the path above is opaque the
// true value underflows to ~0 while E - I_top is rounding noise that tau / mu would amplify.  Per point and layer:
// G = sum_k (W_k / mu_k) g_k; d ln tau_l = tau_l G, molecule term m of the layer = k_(m,l) depth_l G, dT_l = sum_k W_k A (1 - t) dB_l/dT.
// The downward pass is jacobian_down_step, storing; the turn at the top flux_top_turn; the layer loops column_up / column_down.
template <int NP, int NA>
__global__ __launch_bounds__(256) void column_jacobian_kernel(const JacArgs* __restrict__ Ap, long long lo0, long long n0,
                                                              long long lo1, long long n1, double* __restrict__ partial) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    constexpr int kSlot = jacobian_slots(2, 1, kMaxLayers, kMaxJacobianTerms);
    __shared__ double acc[4 * kSlot];            // [wave][F_top, dT_s, L x ln tau, L x T, terms]
    const JacArgs& A = *Ap;
    const int L = A.n_layers;
    const int nv = jacobian_slots(2, 1, L, A.n_terms);
    band_frame<NP, kSlot>(A, blockDim.x, lo0, n0, lo1, n1, partial, acc, nv, [&](auto fast_tag, long long j, bool active,
                          const double (&nu)[NP], const double (&pa_n)[NP], auto add) {
        constexpr bool FAST = decltype(fast_tag)::value;
        double dBs[NP], I[NA][NP], Imax[NA][NP], Ak[NA][NP];
        // upward: I_0 = I_surface or B(nu, surface_T), as K5c
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            dBs[p] = 0.0;
            const double Is = A.I_surface ? A.I_surface[j + p]
                                          : fold_planck<false, true>(false, nu[p], nu[p], pa_n[p], A.pbk_surface, 0.0,
                                                                     A.r_surface_T, &dBs[p]);
#pragma unroll
            for (int k = 0; k < NA; ++k) { I[k][p] = Is; Imax[k][p] = Is; }
        }
        column_up<NP>(A, j, L, [&](int l, vec v) {
            const double pbkT = A.pbkT[l], depth = A.depth[l];
            double E0 = 0.0;
            if (FAST) E0 = exp_clamped(nu[0] * pbkT);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double tau = v[p] * depth;
                double dB;          // (not used on the way up; the DT form keeps the down pass's instruction sequence for B)
                const double B = fold_planck<FAST, true>(p == 0, nu[p], nu[0], pa_n[p], pbkT, E0, 0.0, &dB);
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    I[k][p] = fold_update<FAST>(exp_neg_budget(tau * A.rmu[k]), I[k][p], B);
                    Imax[k][p] = fmax(Imax[k][p], I[k][p]);
                }
            }
        });
        flux_top_turn<NP, NA>(A, active, I, Ak, add);
        column_down<NP>(A, j, L, [&](int l, vec v) {
            jacobian_down_step<FAST, 2, true, NP, NA>(A, L, l, v, j, active, nu, pa_n, I, Imax, Ak, add);
        });
        // dF/dT_s = sum_k W_k A_(-1)k dB(nu, T_s)/dT (0 when the surface is a given spectrum)
        double s = 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p)
            s += active ? nan_to_num(angle_sum<NA>(A, [&](int k) { return Ak[k][p] * dBs[p]; })) : 0.0;
        add(1, s);
    });
}

// ----------------------------------------------------------------------------------------
// What the ray Jacobian kernels (K5f, K5h, K5j) share
// ----------------------------------------------------------------------------------------
// The rows of a bundle's rays in `jac`.  One row per ray, kind and crossed layer: the layer's first segment in backward
// order stores, every later one adds to what the same thread stored (the host marks the first, kRayRowStore, in seg_slot).
// The segments' slots, the term rows and the count of crossed layers are the same for every ray of the bundle.
template <int NP, int RB>
struct RayRows {
    const RayJacArgs& A;
    long long j;                        // the thread's first grid point
    long long row0[RB];                 // each ray's first row
    const int32_t* slot;                // per segment of the bundle: the rank of its layer among the crossed ones | kRayRowStore
    const int32_t* term_row;            // per sorted term: its row
    int crossed;                        // distinct layers crossed

    __device__ __forceinline__ RayRows(const RayJacArgs& A_, const char* blk, const int (&rid)[RB], int s0, long long j_)
        : A(A_), j(j_) {
        const long long* row_first = (const long long*)(blk + A.off_row_first);
#pragma unroll
        for (int i = 0; i < RB; ++i) row0[i] = row_first[rid[i]];
        slot = (const int32_t*)(blk + A.off_seg_slot) + s0;
        term_row = (const int32_t*)(blk + A.off_term_row) + ((const int32_t*)(blk + A.off_ray_terms))[rid[0]];
        crossed = ((const int32_t*)(blk + A.off_ray_crossed))[rid[0]];
    }
    // whether segment s stores its layer's rows, and the layer's rank (both uniform over the workgroup)
    __device__ __forceinline__ bool stores(int s) const { return (slot[s] & kRayRowStore) != 0; }
    __device__ __forceinline__ long long rank(int s) const { return slot[s] & (kRayRowStore - 1); }
    // row `row` of ray i at point p
    __device__ __forceinline__ void put(int i, long long row, int p, double v, bool store) const {
#pragma clang fp contract(off)
        double* o = A.jac + (row0[i] + row) * A.n + (j + p);
        *o = store ? v : *o + v;
    }
};

// K5d's downward step along real segment s (layer l), last to first (the derivation is at ray_jacobian_kernel): I holds D,
// Ak the transmittance A from the segment's end to the observer; g is kept for the segment's terms.  HEAD: the ray's rows
// ahead of the layers' (K5f: 1, K5h: 2).
template <bool FAST, int HEAD, int NP, int RB>
__device__ __forceinline__ void ray_backward_step(const RayJacArgs& A, const RayRows<NP, RB>& R, int s, int l, f64v<NP> cur,
                                                  const double (&len)[RB], bool active, const double (&nu)[NP],
                                                  const double (&pa_n)[NP], double (&I)[RB][NP], const double (&Imax)[RB][NP],
                                                  double (&Ak)[RB][NP], double (&g)[RB][NP]) {
#pragma clang fp contract(off)
    const bool store = R.stores(s);
    const long long row_tau = HEAD + R.rank(s);
    const long long row_T = row_tau + R.crossed;
    const double pbkT = A.pbkT[l], rT = A.rT[l];
    double E0 = 0.0;
    if (FAST) E0 = exp_clamped(nu[0] * pbkT);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        double dB;
        const double B = fold_planck<FAST, true>(p == 0, nu[p], nu[0], pa_n[p], pbkT, E0, rT, &dB);
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const double tau = cur[p] * len[i];
            const double tr = exp_neg_budget(tau);
            const double At = Ak[i][p] * tr;
            g[i][p] = fmin(fmax(Ak[i][p] * B + I[i][p], -(At * Imax[i][p])), At * B);
            const double a1 = Ak[i][p] * (1.0 - tr);
            if (active) {
                R.put(i, row_tau, p, tau * g[i][p], store);
                R.put(i, row_T, p, a1 * dB, store);
            }
            I[i][p] = I[i][p] + a1 * B;              // D_(s-1) = D_s + A_s (1 - t_s) B_s
            Ak[i][p] = At;                           // A_(s-1) = A_s t_s
        }
    }
}

// The terms of segment s (layer l): k_m len g per ray and point into the term's row, stored or added to as the layer's rows
template <int NP, int RB>
__device__ __forceinline__ void ray_terms(const RayJacArgs& A, const RayRows<NP, RB>& R, int s, int l, const double (&len)[RB],
                                          bool active, const double (&g)[RB][NP]) {
#pragma clang fp contract(off)
    const bool store = R.stores(s);
    for (int t = A.layer_term[l]; t < A.layer_term[l + 1]; ++t) {
        const f64v<NP> km = load_points<NP>(A.term_k[t], R.j);
        const long long row = R.term_row[t];
        if (active) {
#pragma unroll
            for (int i = 0; i < RB; ++i) {
#pragma unroll
                for (int p = 0; p < NP; ++p) R.put(i, row, p, (km[p] * len[i]) * g[i][p], store);
            }
        }
    }
}

// The state of the ray Jacobian kernels that know surface markers (K5h, K5j) and everything they do outside a real segment.
// Forward: I <- e Is + (1 - e) I at a marker, as ray_surface_kernel, Imax takes the result, and dI/de is carried along in Ak:
// S <- t S per segment (the kernel's step), S <- (Is - I) + (1 - e) S at a marker (the backward identity would divide by
// 1 - e); a ray from the surface starts with I = e Is and S = Is.  Backward: a marker emits, D += A e Is, adds A e dBs/dT to
// the ray's row 0 (the first marker met stores, as a layer's rows are stored, the source at the very end adds or stores)
// and then dims what lies before it, A <- A (1 - e).  Rows: [dT_source, de, ...].
template <int NP, int RB, class Args>
struct RaySurfaceWalk {
    const RayFrame<NP, RB, true, Args>& F;
    const RayRows<NP, RB> R;
    double I[RB][NP], Imax[RB][NP], Ak[RB][NP];          // (Ak: S = dI/de on the forward walk)
    bool row0_stored;                                     // backward: a marker has stored row 0

    __device__ __forceinline__ RaySurfaceWalk(const RayFrame<NP, RB, true, Args>& F_)
        : F(F_), R(F_.A, F_.blk, F_.rid, F_.s0[0], F_.j), row0_stored(false) {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < RB; ++i) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                I[i][p] = F.surface[i] ? surface_leaving(F.em[p], F.Is[p], 0.0) : 0.0;
                Imax[i][p] = I[i][p];
                Ak[i][p] = F.surface[i] ? F.Is[p] : 0.0;
            }
        }
    }
    // e dB(nu, source_T)/dT at point p (0 when the source is a given spectrum)
    __device__ __forceinline__ double source_dT(int p) const {
#pragma clang fp contract(off)
        double dBs = 0.0;
        if (!F.A.I_surface)
            fold_planck<false, true>(false, F.nu[p], F.nu[p], F.pa_n[p], F.A.pbk_surface, 0.0, F.A.r_source_T, &dBs);
        return F.em[p] * dBs;
    }
    __device__ __forceinline__ void forward_marker() {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < RB; ++i) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                Ak[i][p] = (F.Is[p] - I[i][p]) + (1.0 - F.em[p]) * Ak[i][p];
                I[i][p] = surface_leaving(F.em[p], F.Is[p], I[i][p]);
                Imax[i][p] = fmax(Imax[i][p], I[i][p]);
            }
        }
    }
    // after the forward walk: the radiance and dI/de; then I becomes D = -I_final and A = 1
    __device__ __forceinline__ void turn() {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < RB; ++i) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (F.active && F.A.radiance) F.A.radiance[(long long)F.rid[i] * F.A.n + F.j + p] = I[i][p];
                if (F.active) R.put(i, 1, p, Ak[i][p], true);
                I[i][p] = -I[i][p];
                Ak[i][p] = 1.0;
            }
        }
    }
    __device__ __forceinline__ void backward_marker() {
#pragma clang fp contract(off)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double edBs = F.A.I_surface ? 0.0 : source_dT(p);
            const double eIs = F.em[p] * F.Is[p];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                if (F.active && !F.A.I_surface) R.put(i, 0, p, Ak[i][p] * edBs, !row0_stored);
                I[i][p] = I[i][p] + Ak[i][p] * eIs;
                Ak[i][p] = Ak[i][p] * (1.0 - F.em[p]);
            }
        }
        if (!F.A.I_surface) row0_stored = true;
    }
    // after the backward walk, the source's part of dI/dT_source: A_0 e dBs/dT for a ray from the surface at source_T
    __device__ __forceinline__ void source_row() const {
#pragma clang fp contract(off)
        if (F.active) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double edBs = source_dT(p);
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    const double v = F.surface[i] && !F.A.I_surface ? Ak[i][p] * edBs : 0.0;
                    if (!row0_stored || F.surface[i]) R.put(i, 0, p, v, !row0_stored);
                }
            }
        }
    }
};

// K5f: ray-path Jacobians (lbl_ray_jacobian_dev; the semantics are in include/pyrad_hip.h).  K5e's walk over the bundle's
// segments (the same transport_step, exp and update, so the radiance is K5e's bit for bit), keeping per ray and point the
// running maximum Imax of I; then K5d's downward pass along the segments last to first: k_l re-read a segment ahead, B_l
// and dB_l/dT recomputed, and per ray the transmittance A from the segment's end to the observer and D = E - I_final.
//     A t (B - I_s) = A B + D, clamped to [-A t Imax, A t B]            (I_s: the radiance entering the segment)
// Rows as RayRows keeps them.  No atomics, no memset, no LDS, nothing shared between threads: the same inputs give the
// same bits, and a ray's rows do not depend on the rays it travels with.
// TERMS = false leaves the term loop out (a call without terms): the bundle then need not keep g for it and fits two waves
// per SIMD; the arithmetic of every other row is the same.
// The frame (set-up and segment loops) is the kernel's own, not RayFrame (it measures slower on it: DESIGN.md, "Two frames
// carry ..."); the backward step, the term loop and the rows are the shared ray_backward_step, ray_terms and RayRows.
template <int NP, int RB, bool TERMS>
__global__ __launch_bounds__(256) void ray_jacobian_kernel(const RayJacArgs* __restrict__ Ap, long long lo0, long long n0,
                                                           long long lo1, long long n1, int order_first) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    const RayJacArgs& A = *Ap;
    const char* blk = (const char*)Ap;
    const int32_t* __restrict__ ray_first = (const int32_t*)(blk + A.off_ray_first);
    const int32_t* __restrict__ seg_layer = (const int32_t*)(blk + A.off_seg_layer);
    const double* __restrict__ seg_length = (const double*)(blk + A.off_seg_length);
    const int32_t* __restrict__ source_kind = (const int32_t*)(blk + A.off_source_kind);
    const int32_t* __restrict__ order = (const int32_t*)(blk + A.off_order);
    // (idle lanes of the last workgroup work on a valid point and store nothing)
    const long long q = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * NP;
    const bool active = q < n0 + n1;
    const long long j = !active ? lo0 : (q < n0 ? lo0 + q : lo1 + (q - n0));
    double nu[NP], pa_n[NP], Is[NP], I[RB][NP], Imax[RB][NP], Ak[RB][NP];
    column_points<NP>(A, j, nu, pa_n);
    const bool fast = fold_fast_path<NP>(A, nu, active);
#pragma unroll
    for (int p = 0; p < NP; ++p) Is[p] = A.I_surface ? A.I_surface[j + p] : planck_budget(nu[p], A.pa, A.pbk_surface);
    int rid[RB], s0[RB];
    bool surface[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        rid[i] = order[order_first + (int)blockIdx.y * RB + i];
        s0[i] = ray_first[rid[i]];
        surface[i] = source_kind[rid[i]] == 1;
#pragma unroll
        for (int p = 0; p < NP; ++p) { I[i][p] = surface[i] ? Is[p] : 0.0; Imax[i][p] = I[i][p]; }
    }
    const int ns = ray_first[rid[0] + 1] - s0[0];        // (the same for every ray of the bundle, as are its layers and rows)
    const int32_t* lay = seg_layer + s0[0];
    const RayRows<NP, RB> R(A, blk, rid, s0[0], j);
    auto walk = [&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        // forward: K5e's walk, and the running maximum
        vec cur = ns > 0 ? load_points<NP>(A.abs_coef[lay[0]], j) : (vec)(0.0);
        for (int s = 0; s < ns; ++s) {
            const vec nxt = s + 1 < ns ? load_points<NP>(A.abs_coef[lay[s + 1]], j) : cur;
            double len[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) len[i] = seg_length[s0[i] + s];
            transport_step<FAST, NP>(nu, pa_n, A.pbkT[lay[s]], cur, [&](int p, double kp, double B) {
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    I[i][p] = fold_update<FAST>(exp_neg_budget(kp * len[i]), I[i][p], B);
                    Imax[i][p] = fmax(Imax[i][p], I[i][p]);
                }
            });
            cur = nxt;
        }
        // the radiance; then I becomes D = -I_final and A = 1
#pragma unroll
        for (int i = 0; i < RB; ++i) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (active && A.radiance) A.radiance[(long long)rid[i] * A.n + j + p] = I[i][p];
                I[i][p] = -I[i][p];
                Ak[i][p] = 1.0;
            }
        }
        // backward
        cur = ns > 0 ? load_points<NP>(A.abs_coef[lay[ns - 1]], j) : (vec)(0.0);
        for (int s = ns - 1; s >= 0; --s) {
            const vec nxt = s > 0 ? load_points<NP>(A.abs_coef[lay[s - 1]], j) : cur;
            double len[RB], g[RB][NP];
#pragma unroll
            for (int i = 0; i < RB; ++i) len[i] = seg_length[s0[i] + s];
            ray_backward_step<FAST, 1, NP, RB>(A, R, s, lay[s], cur, len, active, nu, pa_n, I, Imax, Ak, g);
            if constexpr (TERMS) ray_terms<NP, RB>(A, R, s, lay[s], len, active, g);
            cur = nxt;
        }
        // dI/dT_source = A dB(nu, source_T)/dT for a ray from the surface at source_T, else 0
        if (active) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                double dBs = 0.0;
                if (!A.I_surface) fold_planck<false, true>(false, nu[p], nu[p], pa_n[p], A.pbk_surface, 0.0, A.r_source_T, &dBs);
#pragma unroll
                for (int i = 0; i < RB; ++i) R.put(i, 0, p, surface[i] && !A.I_surface ? Ak[i][p] * dBs : 0.0, true);
            }
        }
    };
    if constexpr (NP > 1) {
        if (fast) walk(std::true_type{});
        else walk(std::false_type{});
    } else {
        walk(std::false_type{});
    }
}

// ----------------------------------------------------------------------------------------
// K5h: Jacobians over a reflecting surface (lbl_column_jacobian_surface_dev, lbl_ray_jacobian_surface_dev; the semantics are
// in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// Column: three walks.  (1) K5g's downward walk from I_top, keeping per angle the radiance, its running maximum Dmax over
// the levels and the transmittance Ttot; at the surface dF/de and dF/dT_s are complete (both need only Ttot, Is and what
// came down), and the state turns in place into that of walk (2): I_up[0] = e Is + (1 - e) R, Imax, and for the light that
// went DOWN through a layer and is seen through the surface the weight Qf (Q_k = W_k Qf), C = 1 and D' = -D.  (2) K5d's
// upward walk, and beside it the downward leg mirrored: with C the transmittance from the layer's lower edge to the
// surface and D' = E' - D, E' the emission of the layers below that reaches the surface,
//     C_l t_l (B_l - Id_(l+1)) = C_l B_l + D'_l,   clamped to [-C_l t_l Dmax, C_l t_l B_l]
// - K5d's identity upside down, so no level radiance is stored.  This walk STORES the reflected leg's part of the spectra
// and adds its sums to the band slots.  (3) K5d's downward pass, which ADDS its part to what the same thread stored.
// With e == 1: Qf = 0, walk (2) contributes +-0 everywhere, I_up[0] = Is, and walks (2) and (3) are K5d's operations in
// K5d's order - K5d's bits on its own groups of points (the one-exp Planck path starts from a thread's first point).
// Walk 1's start and the surface are ReflectingSurfaceTurn, the turn at the top flux_top_turn, walk 3 K5d's own
// jacobian_down_step, adding; walks 1 and 2 are this kernel's.
template <int NP, int NA>
__global__ __launch_bounds__(256) void surface_jacobian_kernel(const SurfaceJacArgs* __restrict__ Ap, long long lo0, long long n0,
                                                               long long lo1, long long n1, double* __restrict__ partial) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    constexpr int kSlot = jacobian_slots(3, 1, kMaxLayers, kMaxJacobianTerms);
    __shared__ double acc[4 * kSlot];            // [wave][F_top, dT_s, de, L x ln tau, L x T, terms]
    const SurfaceJacArgs& A = *Ap;
    const int L = A.n_layers;
    const int nv = jacobian_slots(3, 1, L, A.n_terms);
    band_frame<NP, kSlot>(A, blockDim.x, lo0, n0, lo1, n1, partial, acc, nv, [&](auto fast_tag, long long j, bool active,
                          const double (&nu)[NP], const double (&pa_n)[NP], auto add) {
        constexpr bool FAST = decltype(fast_tag)::value;
        // walk 1: I = Id, Dm = Dmax, Ak = Ttot;  walk 2: I = Iu, Imax, Ck = C, Dp = D', Dm, Ak = Qf;  walk 3: I = D, Imax, Ak = A
        double I[NA][NP], Imax[NA][NP], Ak[NA][NP], Ck[NA][NP], Dp[NA][NP], Dm[NA][NP];
        // walk 1, downward
        ReflectingSurfaceTurn<NP, NA>::start(A, j, I, Dm, Ak);
        column_down<NP>(A, j, L, [&](int l, vec v) {
            const double pbkT = A.pbkT[l], depth = A.depth[l];
            double E0 = 0.0;
            if (FAST) E0 = exp_clamped(nu[0] * pbkT);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double tau = v[p] * depth;
                double dB;
                const double B = fold_planck<FAST, true>(p == 0, nu[p], nu[0], pa_n[p], pbkT, E0, 0.0, &dB);
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    const double tr = exp_neg_budget(tau * A.rmu[k]);
                    I[k][p] = fold_update<FAST>(tr, I[k][p], B);
                    Dm[k][p] = fmax(Dm[k][p], I[k][p]);
                    Ak[k][p] = Ak[k][p] * tr;
                }
            }
        });
        ReflectingSurfaceTurn<NP, NA>::turn(A, j, active, nu, pa_n, I, Imax, Ak, Ck, Dp, add);
        // walk 2, upward
        column_up<NP>(A, j, L, [&](int l, vec v) {
            const double pbkT = A.pbkT[l], depth = A.depth[l], rT = A.rT[l];
            double E0 = 0.0;
            if (FAST) E0 = exp_clamped(nu[0] * pbkT);
            double s_tau = 0.0, s_T[1] = {0.0}, Gd[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double tau = v[p] * depth;
                double dB;
                const double B = fold_planck<FAST, true>(p == 0, nu[p], nu[0], pa_n[p], pbkT, E0, rT, &dB);
                double G = 0.0, gT[1] = {0.0};
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    const double tr = exp_neg_budget(tau * A.rmu[k]);
                    // the downward leg through this layer, seen through the surface
                    const double Ct = Ck[k][p] * tr;
                    const double g = fmin(fmax(Ck[k][p] * B + Dp[k][p], -(Ct * Dm[k][p])), Ct * B);
                    G = fma(A.wrmu[k], Ak[k][p] * g, G);
                    const double c1 = Ck[k][p] * (1.0 - tr);
                    gT[0] = fma(A.w[k], Ak[k][p] * (c1 * dB), gT[0]);
                    Dp[k][p] = Dp[k][p] + c1 * B;            // D'_(l+1) = D'_l + C_l (1 - t_l) B_l
                    Ck[k][p] = Ct;                           // C_(l+1) = C_l t_l
                    // the upward leg: K5d's walk
                    I[k][p] = fold_update<FAST>(tr, I[k][p], B);
                    Imax[k][p] = fmax(Imax[k][p], I[k][p]);
                }
                Gd[p] = depth * G;
                jacobian_emit<1>(true, active, A, &JacArgs::T_spec, l, j, p, tau * G, gT, s_tau, s_T);
            }
            add(3 + l, s_tau);
            add(3 + L + l, s_T[0]);
            jacobian_terms<NP>(A, l, j, active, Gd, 3 + 2 * L, add);
        });
        flux_top_turn<NP, NA>(A, active, I, Ak, add);
        // walk 3, downward: K5d's
        column_down<NP>(A, j, L, [&](int l, vec v) {
            jacobian_down_step<FAST, 3, false, NP, NA>(A, L, l, v, j, active, nu, pa_n, I, Imax, Ak, add);
        });
    });
}

// Rays: K5f's kernel with K5g's surface in the path.  A marker (layer kRaySurfaceMarker) is part of the bundle's common
// sequence, so the branch on it is uniform over the workgroup.  What happens at a marker, at the start and between and
// after the walks is RaySurfaceWalk's; the backward step through a real segment is K5f's own ray_backward_step and
// ray_terms.  Rows: [dT_source, de, K5f's].  With e == 1 and no marker every operation on I, Imax, D and A is K5f's.
template <int NP, int RB, bool TERMS>
__global__ __launch_bounds__(256) void ray_surface_jacobian_kernel(const RaySurfaceJacArgs* __restrict__ Ap, long long lo0,
                                                                   long long n0, long long lo1, long long n1, int order_first) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    const RaySurfaceJacArgs& A = *Ap;
    const RayFrame<NP, RB, true, RaySurfaceJacArgs> F(Ap, blockDim.x, lo0, n0, lo1, n1, order_first);
    RaySurfaceWalk<NP, RB, RaySurfaceJacArgs> W(F);
    F.dispatch([&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        // forward: ray_surface_kernel's walk, the running maximum and dI/de
        F.forward([&] { W.forward_marker(); }, [&](int s, vec cur, const double (&len)[RB]) {
            transport_step<FAST, NP>(F.nu, F.pa_n, A.pbkT[F.lay[s]], cur, [&](int p, double kp, double B) {
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    const double tr = exp_neg_budget(kp * len[i]);
                    W.I[i][p] = fold_update<FAST>(tr, W.I[i][p], B);
                    W.Imax[i][p] = fmax(W.Imax[i][p], W.I[i][p]);
                    W.Ak[i][p] = tr * W.Ak[i][p];
                }
            });
        });
        W.turn();
        F.backward([&] { W.backward_marker(); }, [&](int s, vec cur, const double (&len)[RB]) {
            double g[RB][NP];
            ray_backward_step<FAST, 2, NP, RB>(A, W.R, s, F.lay[s], cur, len, F.active, F.nu, F.pa_n, W.I, W.Imax, W.Ak, g);
            if constexpr (TERMS) ray_terms<NP, RB>(A, W.R, s, F.lay[s], len, F.active, g);
        });
        W.source_row();
    });
}

// ----------------------------------------------------------------------------------------
// K5j: Jacobians of the linear-in-optical-depth Planck source (lbl_column_jacobian_linear_dev, lbl_ray_jacobian_linear_dev;
// the semantics are in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// K5h's walks with K5i's step I <- t I + (1 - t) Ba + g (Bb - Ba) = t I + h Ba + g Bb, h = (1 - t) - g = tau g'(tau)
// (linear_source_g, linear_source_dg of lbl_linear_source.h).  With A the transmittance behind the step and D = E - I_final,
// E the emission behind the step that reaches the end (K5d's identity with the step's whole emission in it),
//     A t (Ba - I_in) = A (Ba + g (Bb - Ba)) + D,   clamped to [-A t Imax, A t Ba],        D <- D + A ((1 - t) Ba + g (Bb - Ba)),
// so no level radiance is stored here either.  Per step G = that + A g' (Bb - Ba): d ln tau = tau G and a term = k_m x G (no
// division by tau: a point without absorption stays finite), dTa = A h dB(Ta)/dT, dTb = A g dB(Tb)/dT.
// Per point and step: two Planck values with their temperature derivatives (two exps per thread on the fast path), and per
// angle or ray one exp, one g and one g'.

// Ba, Bb and their temperature derivatives for the thread's point p (E0: the thread's two exps on the fast path)
template <bool FAST>
__device__ __forceinline__ void linear_planck_pair(bool first, double nu, double nu0, double pa_n, double pbkT_a, double pbkT_b,
                                                   double Ea0, double Eb0, double rT_a, double rT_b, double& Ba, double& Bb,
                                                   double& dBa, double& dBb) {
    Ba = fold_planck<FAST, true>(first, nu, nu0, pa_n, pbkT_a, Ea0, rT_a, &dBa);
    Bb = fold_planck<FAST, true>(first, nu, nu0, pa_n, pbkT_b, Eb0, rT_b, &dBb);
}

// What walks 2 and 3 of linear_jacobian_kernel need of layer l before its points: the layer's scalars, bottom and top edge,
// and on the fast path the thread's two exps; then per point the two Planck values with their temperature derivatives
template <bool FAST>
struct LinearLayer {
    double pbkT, pbkT_top, depth, rT, rT_top, E0, E0_top;
    __device__ __forceinline__ LinearLayer(const LinearJacArgs& A, int l, double nu0)
        : pbkT(A.pbkT[l]), pbkT_top(A.pbkT_top[l]), depth(A.depth[l]), rT(A.rT[l]), rT_top(A.rT_top[l]), E0(0.0), E0_top(0.0) {
#pragma clang fp contract(off)
        if (FAST) {
            E0 = exp_clamped(nu0 * pbkT);
            E0_top = exp_clamped(nu0 * pbkT_top);
        }
    }
    __device__ __forceinline__ void planck(bool first, double nu, double nu0, double pa_n, double& Bbot, double& Btop,
                                           double& dBbot, double& dBtop) const {
        linear_planck_pair<FAST>(first, nu, nu0, pa_n, pbkT, pbkT_top, E0, E0_top, rT, rT_top, Bbot, Btop, dBbot, dBtop);
    }
};

// Column: surface_jacobian_kernel's three walks.  Walk 1 is linear_flux_kernel's downward walk (entered at the top edge,
// left at the bottom edge) with Dmax and Ttot; the surface is K5h's (ReflectingSurfaceTurn, as is walk 1's start); walk 2
// carries the upward leg (entered at the bottom edge) and the mirrored downward leg, walk 3 the upward leg's derivatives.
// Both later walks add to the band slots; of the spectra walk 2 stores and walk 3 adds to what the same thread stored
// (jacobian_emit with two temperature rows).  Band slots: [F, dT_s, de, L x ln tau, 2 L x T_edge (bottom, top), terms].
// Points per thread: K5h's - 4 with one and two angles, 2 beyond.  The state is its six values per angle and point, and a
// step keeps four Planck values, g, g' and h beside them: 256 VGPRs and up to 202 AGPRs at one wave per SIMD, no scratch
// (DESIGN.md "K5j").
template <int NP, int NA>
__global__ __launch_bounds__(256) void linear_jacobian_kernel(const LinearJacArgs* __restrict__ Ap, long long lo0, long long n0,
                                                              long long lo1, long long n1, double* __restrict__ partial) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    constexpr int kSlot = jacobian_slots(3, 2, kMaxLayers, kMaxJacobianTerms);
    __shared__ double acc[4 * kSlot];            // [wave][F_top, dT_s, de, L x ln tau, 2 L x T_edge, terms]
    const LinearJacArgs& A = *Ap;
    const int L = A.n_layers;
    const int nv = jacobian_slots(3, 2, L, A.n_terms);
    band_frame<NP, kSlot>(A, blockDim.x, lo0, n0, lo1, n1, partial, acc, nv, [&](auto fast_tag, long long j, bool active,
                          const double (&nu)[NP], const double (&pa_n)[NP], auto add) __attribute__((always_inline)) {
        constexpr bool FAST = decltype(fast_tag)::value;
        // walk 1: I = Id, Dm = Dmax, Ak = Ttot;  walk 2: I = Iu, Imax, Ck = C, Dp = D', Dm, Ak = Qf;  walk 3: I = D, Imax, Ak = A
        double I[NA][NP], Imax[NA][NP], Ak[NA][NP], Ck[NA][NP], Dp[NA][NP], Dm[NA][NP];
        // a layer's sums into its band slots, and its terms
        auto sums = [&](int l, double s_tau, const double (&s_T)[2], const double (&Gd)[NP]) __attribute__((always_inline)) {
            add(3 + l, s_tau);
            add(3 + L + 2 * l, s_T[0]);
            add(3 + L + 2 * l + 1, s_T[1]);
            jacobian_terms<NP>(A, l, j, active, Gd, 3 + 3 * L, add);
        };
        // walk 1, downward
        ReflectingSurfaceTurn<NP, NA>::start(A, j, I, Dm, Ak);
        column_down<NP>(A, j, L, [&](int l, vec v) __attribute__((always_inline)) {
            const double depth = A.depth[l];
            linear_step<FAST, NP>(nu, pa_n, A.pbkT_top[l], A.pbkT[l], v, [&](int p, double kp, double Ba, double dB) __attribute__((always_inline)) {
                const double tau = kp * depth;
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    const double x = tau * A.rmu[k];
                    const double tr = exp_neg_budget(x);
                    I[k][p] = linear_update<FAST>(x, tr, I[k][p], Ba, dB);
                    Dm[k][p] = fmax(Dm[k][p], I[k][p]);
                    Ak[k][p] = Ak[k][p] * tr;
                }
            });
        });
        ReflectingSurfaceTurn<NP, NA>::turn(A, j, active, nu, pa_n, I, Imax, Ak, Ck, Dp, add);
        // walk 2, upward; (gT, s_T: bottom edge, top edge)
        column_up<NP>(A, j, L, [&](int l, vec v) __attribute__((always_inline)) {
            const LinearLayer<FAST> Y(A, l, nu[0]);
            double s_tau = 0.0, s_T[2] = {0.0, 0.0}, Gd[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double tau = v[p] * Y.depth;
                double Bbot, Btop, dBbot, dBtop;
                Y.planck(p == 0, nu[p], nu[0], pa_n[p], Bbot, Btop, dBbot, dBtop);
                const double dBu = Btop - Bbot, dBd = Bbot - Btop;
                double G = 0.0, gT[2] = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    const double x = tau * A.rmu[k];
                    const double tr = exp_neg_budget(x);
                    const double g = linear_source_g(x, tr);
                    const double dg = linear_source_dg(x, tr);
                    const double h = x * dg;
                    // the downward leg through this layer (top edge to bottom edge), seen through the surface
                    const double Ct = Ck[k][p] * tr;
                    const double gd = fmin(fmax(Ck[k][p] * (Btop + g * dBd) + Dp[k][p], -(Ct * Dm[k][p])), Ct * Btop);
                    G = fma(A.wrmu[k], Ak[k][p] * (gd + Ck[k][p] * (dg * dBd)), G);
                    gT[1] = fma(A.w[k], Ak[k][p] * ((Ck[k][p] * h) * dBtop), gT[1]);
                    gT[0] = fma(A.w[k], Ak[k][p] * ((Ck[k][p] * g) * dBbot), gT[0]);
                    Dp[k][p] = Dp[k][p] + Ck[k][p] * ((1.0 - tr) * Btop + g * dBd);      // D' <- D' + C (the step's emission)
                    Ck[k][p] = Ct;
                    // the upward leg: linear_flux_kernel's step
                    I[k][p] = linear_update<FAST>(x, tr, I[k][p], Bbot, dBu);
                    Imax[k][p] = fmax(Imax[k][p], I[k][p]);
                }
                Gd[p] = Y.depth * G;
                jacobian_emit<2>(true, active, A, &LinearJacArgs::T_edge_spec, l, j, p, tau * G, gT, s_tau, s_T);
            }
            sums(l, s_tau, s_T, Gd);
        });
        flux_top_turn<NP, NA>(A, active, I, Ak, add);
        // walk 3, downward
        column_down<NP>(A, j, L, [&](int l, vec v) __attribute__((always_inline)) {
            const LinearLayer<FAST> Y(A, l, nu[0]);
            double s_tau = 0.0, s_T[2] = {0.0, 0.0}, Gd[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double tau = v[p] * Y.depth;
                double Bbot, Btop, dBbot, dBtop;
                Y.planck(p == 0, nu[p], nu[0], pa_n[p], Bbot, Btop, dBbot, dBtop);
                const double dBu = Btop - Bbot;
                double G = 0.0, gT[2] = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    const double x = tau * A.rmu[k];
                    const double tr = exp_neg_budget(x);
                    const double g = linear_source_g(x, tr);
                    const double dg = linear_source_dg(x, tr);
                    const double h = x * dg;
                    const double At = Ak[k][p] * tr;
                    const double gu = fmin(fmax(Ak[k][p] * (Bbot + g * dBu) + I[k][p], -(At * Imax[k][p])), At * Bbot);
                    G = fma(A.wrmu[k], gu + Ak[k][p] * (dg * dBu), G);
                    gT[0] = fma(A.w[k], (Ak[k][p] * h) * dBbot, gT[0]);
                    gT[1] = fma(A.w[k], (Ak[k][p] * g) * dBtop, gT[1]);
                    I[k][p] = I[k][p] + Ak[k][p] * ((1.0 - tr) * Bbot + g * dBu);        // D <- D + A (the step's emission)
                    Ak[k][p] = At;
                }
                Gd[p] = Y.depth * G;
                jacobian_emit<2>(false, active, A, &LinearJacArgs::T_edge_spec, l, j, p, tau * G, gT, s_tau, s_T);
            }
            sums(l, s_tau, s_T, Gd);
        });
    });
}

// Rays: ray_surface_jacobian_kernel's walks (RaySurfaceWalk) with linear_ray_kernel's step.  Forward every operation on I is
// linear_ray_kernel's, on the same groups of points, so `radiance` is lbl_ray_radiance_linear_dev's bit for bit; Imax and
// dI/de are carried as K5h carries them.  Backward a real segment stores its own two temperature rows (once, never added
// to: seg_Trow names them) and stores or adds to its layer's ln tau row and term rows (ray_terms) as K5f's do.
// Rows: [dT_source, de, c x d ln tau, (dTa, dTb) per real segment in order of travel, terms].
template <int NP, int RB>
__global__ __launch_bounds__(256) void ray_linear_jacobian_kernel(const LinearRayJacArgs* __restrict__ Ap, long long lo0,
                                                                  long long n0, long long lo1, long long n1, int order_first) {
#pragma clang fp contract(off)
    typedef f64v<NP> vec;
    const LinearRayJacArgs& A = *Ap;
    const RayFrame<NP, RB, true, LinearRayJacArgs> F(Ap, blockDim.x, lo0, n0, lo1, n1, order_first);
    RaySurfaceWalk<NP, RB, LinearRayJacArgs> W(F);
    const double* pbk = (const double*)(F.blk + A.off_seg_pbkT) + 2 * (long long)F.s0[0];
    const double* srT = (const double*)(F.blk + A.off_seg_rT) + 2 * (long long)F.s0[0];
    const int32_t* Trow = (const int32_t*)(F.blk + A.off_seg_Trow) + F.s0[0];
    F.dispatch([&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        // forward: linear_ray_kernel's walk, the running maximum and dI/de
        F.forward([&] { W.forward_marker(); }, [&](int s, vec cur, const double (&len)[RB]) {
            linear_step<FAST, NP>(F.nu, F.pa_n, pbk[2 * s], pbk[2 * s + 1], cur, [&](int p, double kp, double Ba, double dB) {
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    const double tau = kp * len[i];
                    const double tr = exp_neg_budget(tau);
                    W.I[i][p] = linear_update<FAST>(tau, tr, W.I[i][p], Ba, dB);
                    W.Imax[i][p] = fmax(W.Imax[i][p], W.I[i][p]);
                    W.Ak[i][p] = tr * W.Ak[i][p];
                }
            });
        });
        W.turn();
        F.backward([&] { W.backward_marker(); }, [&](int s, vec cur, const double (&len)[RB]) {
            const bool store = W.R.stores(s);
            const long long row_tau = 2 + W.R.rank(s);
            const long long row_Ta = Trow[s];
            const double pbkT_a = pbk[2 * s], pbkT_b = pbk[2 * s + 1], rT_a = srT[2 * s], rT_b = srT[2 * s + 1];
            double G[RB][NP];
            double Ea0 = 0.0, Eb0 = 0.0;
            if (FAST) {
                Ea0 = exp_clamped(F.nu[0] * pbkT_a);
                Eb0 = exp_clamped(F.nu[0] * pbkT_b);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                double Ba, Bb, dBa, dBb;
                linear_planck_pair<FAST>(p == 0, F.nu[p], F.nu[0], F.pa_n[p], pbkT_a, pbkT_b, Ea0, Eb0, rT_a, rT_b, Ba, Bb, dBa, dBb);
                const double dB = Bb - Ba;
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    const double tau = cur[p] * len[i];
                    const double tr = exp_neg_budget(tau);
                    const double g = linear_source_g(tau, tr);
                    const double dg = linear_source_dg(tau, tr);
                    const double At = W.Ak[i][p] * tr;
                    const double gc = fmin(fmax(W.Ak[i][p] * (Ba + g * dB) + W.I[i][p], -(At * W.Imax[i][p])), At * Ba);
                    G[i][p] = gc + W.Ak[i][p] * (dg * dB);
                    if (F.active) {
                        W.R.put(i, row_tau, p, tau * G[i][p], store);
                        W.R.put(i, row_Ta, p, (W.Ak[i][p] * (tau * dg)) * dBa, true);
                        W.R.put(i, row_Ta + 1, p, (W.Ak[i][p] * g) * dBb, true);
                    }
                    W.I[i][p] = W.I[i][p] + W.Ak[i][p] * ((1.0 - tr) * Ba + g * dB);     // D <- D + A (the step's emission)
                    W.Ak[i][p] = At;
                }
            }
            ray_terms<NP, RB>(A, W.R, s, F.lay[s], len, F.active, G);
        });
        W.source_row();
    });
}

// ----------------------------------------------------------------------------------------
// K7: line survey (pyradClasses.py:409-428): S added into the bin of each line, in line order
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void line_survey_kernel(const double* __restrict__ nu, const double* __restrict__ sw,
                                                          int n_lines, double range_min, double resolution,
                                                          double* __restrict__ out, long long n_base) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    const long long c = (long long)((nu[i] - range_min) / resolution);
    if (c < 0 || c > n_base - 1) return;
    if (i > 0 && (long long)((nu[i - 1] - range_min) / resolution) == c) return;   // not the first line of its bin
    double s = 0.0;                           // lineSurvey starts from zeros (pyradClasses.py:416)
    for (int k = i; k < n_lines; ++k) {
        if ((long long)((nu[k] - range_min) / resolution) != c) break;
        s = s + sw[k];
    }
    out[c] = s;
}

// ----------------------------------------------------------------------------------------
// launchers (called from lbl_api.hip)
// ----------------------------------------------------------------------------------------
void launch_line_prep(const PrepJob* d_jobs, int n_jobs, int max_lines, hipStream_t s) {
    if (n_jobs <= 0 || max_lines <= 0) return;
    dim3 grid((max_lines + 255) / 256, n_jobs);
    hipLaunchKernelGGL(line_prep_kernel, grid, dim3(256), 0, s, d_jobs);
}

void launch_line_prep_merged(const PrepJob* d_lists, const MergedPrep* d_jobs, int n_jobs, int max_total, hipStream_t s) {
    if (n_jobs <= 0 || max_total <= 0) return;
    dim3 grid((max_total + 255) / 256, n_jobs);
    hipLaunchKernelGGL(line_prep_merged_kernel, grid, dim3(256), 0, s, d_lists, d_jobs);
}

void launch_line_quantities(const PrepJob* d_job, int n_lines, long long* index, double* lhw, double* ghw, double* intensity,
                            int32_t* regime, hipStream_t s) {
    if (n_lines <= 0) return;
    hipLaunchKernelGGL(line_quantities_kernel, dim3((n_lines + 255) / 256), dim3(256), 0, s, d_job, index, lhw, ghw, intensity, regime);
}

template <int R>
static void launch_accum_scalar(const AccumJob* d_jobs, int n_jobs, int max_tiles, hipStream_t s) {
    dim3 grid(((max_tiles + 7) / 8) * 8, n_jobs);
    hipLaunchKernelGGL((xsec_accumulate_kernel<R>), grid, dim3(256), 0, s, d_jobs);   // 0: IEEE divide + exp per pair
}

template <int R, int NT>
static void launch_accum_lds(const AccumJob* d_jobs, int n_jobs, int max_tiles, int LS, const int2* worklist,
                             int total_tiles, hipStream_t s, int gauss_run = 16) {
    dim3 grid(((max_tiles + 7) / 8) * 8, n_jobs);
    if (worklist) {
        if (total_tiles <= 0) return;
        grid = dim3(total_tiles, 1);
    }
#ifdef LBL_DIAG        // (scripts/cost_fit.py): unused dynamic LDS to limit the workgroups resident per CU
    static const int pad = getenv("LBL_DIAG_LDS_PAD") ? atoi(getenv("LBL_DIAG_LDS_PAD")) : 0;
#else
    constexpr int pad = 0;
#endif
    switch (LS) {
        case 8: hipLaunchKernelGGL((xsec_accumulate_lds_kernel<R, 8, NT>), grid, dim3(512), pad, s, d_jobs, worklist); break;
        case 4: hipLaunchKernelGGL((xsec_accumulate_lds_kernel<R, 4, NT>), grid, dim3(256), pad, s, d_jobs, worklist); break;
        case 2: hipLaunchKernelGGL((xsec_accumulate_lds_kernel<R, 2, NT>), grid, dim3(256), pad, s, d_jobs, worklist); break;
        default:
            if constexpr (R == 4 && NT > 0) {
                if (gauss_run == 32) {        // the three-waves-per-SIMD build; exact mode: its series starts at FF_MID half-spans (38 terms)
                    hipLaunchKernelGGL((xsec_accumulate_lds_kernel<4, 1, (NT == FF_NT ? FF_NT_MID : NT), 32>), grid, dim3(256), pad, s, d_jobs, worklist);
                    break;
                }
            }
            hipLaunchKernelGGL((xsec_accumulate_lds_kernel<R, 1, NT>), grid, dim3(256), pad, s, d_jobs, worklist); break;
    }
}

void launch_accumulate_skew(const AccumJob* d_jobs, int n_jobs, int max_tiles, int R, const int2* worklist, int total_tiles,
                            hipStream_t s, int LS) {
    if (n_jobs <= 0 || max_tiles <= 0) return;
    dim3 grid(((max_tiles + 7) / 8) * 8, n_jobs);
    if (worklist) {
        if (total_tiles <= 0) return;
        grid = dim3(total_tiles, 1);
    }
    if (R == 8 && LS == 4) { hipLaunchKernelGGL((xsec_accumulate_skew_kernel<8, 4>), grid, dim3(256), 0, s, d_jobs, worklist); return; }
    if (R == 8 && LS == 2) { hipLaunchKernelGGL((xsec_accumulate_skew_kernel<8, 2>), grid, dim3(256), 0, s, d_jobs, worklist); return; }
    switch (R) {
        case 8: hipLaunchKernelGGL((xsec_accumulate_skew_kernel<8>), grid, dim3(256), 0, s, d_jobs, worklist); break;
        case 2: hipLaunchKernelGGL((xsec_accumulate_skew_kernel<2>), grid, dim3(256), 0, s, d_jobs, worklist); break;
        case 1: hipLaunchKernelGGL((xsec_accumulate_skew_kernel<1>), grid, dim3(256), 0, s, d_jobs, worklist); break;
        default: hipLaunchKernelGGL((xsec_accumulate_skew_kernel<4>), grid, dim3(256), 0, s, d_jobs, worklist); break;
    }
}

// far-field threshold (in half-spans of 32 R points) and the cost of a far line relative to a near
// one (3 instructions per series term and 64 lines against 5 R per line), for the host's schedule
void accumulate_far_field_params(int R, int* far_half_spans, double* far_cost, int budget) {
    *far_half_spans = budget ? FF_FAR_BUDGET : FF_FAR;
    *far_cost = (3.0 * 17.0 + 12.0) / 64.0 / (5.0 * R);           // (17 terms: the average over a +-39 half-span window, either mode)
}


// f(std::integral_constant<int, R>) for the points per lane of a launch: 1, 2, 4, and 8 for everything else
template <class F>
static void with_points_per_lane(int R, F&& f) {
    switch (R) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        default: f(std::integral_constant<int, 8>()); break;
    }
}

void launch_accumulate(const AccumJob* d_jobs, int n_jobs, int max_tiles, int R, int LS, int variant,
                       const int2* worklist, int total_tiles, hipStream_t s, int budget, int gauss_run) {
    if (n_jobs <= 0 || max_tiles <= 0) return;
    // (gauss_run: launch_accum_lds reads it for R == 4 with the far-field series only)
    if (variant >= 5 && budget)
        with_points_per_lane(R, [&](auto r) { launch_accum_lds<decltype(r)::value, FF_NT_BUDGET>(d_jobs, n_jobs, max_tiles, LS, worklist, total_tiles, s, gauss_run); });
    else if (variant >= 5)
        with_points_per_lane(R, [&](auto r) { launch_accum_lds<decltype(r)::value, FF_NT>(d_jobs, n_jobs, max_tiles, LS, worklist, total_tiles, s, gauss_run); });
    else if (variant >= 3)
        with_points_per_lane(R, [&](auto r) { launch_accum_lds<decltype(r)::value, 0>(d_jobs, n_jobs, max_tiles, LS, worklist, total_tiles, s); });
    else
        with_points_per_lane(R, [&](auto r) { launch_accum_scalar<decltype(r)::value>(d_jobs, n_jobs, max_tiles, s); });
}

void launch_voigt_prep(const PrepJob* d_prep, const VoigtJob* d_jobs, int n_jobs, int max_lines, hipStream_t s) {
    if (n_jobs <= 0 || max_lines <= 0) return;
    for (int j0 = 0; j0 < n_jobs; j0 += 65535) {            // (a launch's second dimension holds 65,535 workgroups)
        dim3 grid((max_lines + 255) / 256, std::min(n_jobs - j0, 65535));
        hipLaunchKernelGGL(voigt_prep_kernel, grid, dim3(256), 0, s, d_prep + j0, d_jobs + j0);
    }
}

void launch_voigt_accumulate(const VoigtJob* d_jobs, int n_jobs, long long max_points, hipStream_t s) {
    if (n_jobs <= 0 || max_points <= 0) return;
    for (int j0 = 0; j0 < n_jobs; j0 += 65535) {
        dim3 grid((unsigned)((max_points + kVoigtTile - 1) / kVoigtTile), std::min(n_jobs - j0, 65535));
        hipLaunchKernelGGL(voigt_accumulate_kernel, grid, dim3(256), 0, s, d_jobs + j0);
    }
}

void launch_voigt_dT_prep(const PrepJob* d_prep, const VoigtDTJob* d_jobs, int n_jobs, int max_lines, hipStream_t s) {
    if (n_jobs <= 0 || max_lines <= 0) return;
    for (int j0 = 0; j0 < n_jobs; j0 += 65535) {
        dim3 grid((unsigned)((max_lines + 255) / 256), std::min(n_jobs - j0, 65535));
        hipLaunchKernelGGL(voigt_dT_prep_kernel, grid, dim3(256), 0, s, d_prep + j0, d_jobs + j0);
    }
}

void launch_voigt_dT_accumulate(const VoigtDTJob* d_jobs, int n_jobs, long long max_points, hipStream_t s) {
    if (n_jobs <= 0 || max_points <= 0) return;
    for (int j0 = 0; j0 < n_jobs; j0 += 65535) {
        dim3 grid((unsigned)((max_points + kVoigtTile - 1) / kVoigtTile), std::min(n_jobs - j0, 65535));
        hipLaunchKernelGGL(voigt_dT_accumulate_kernel, grid, dim3(256), 0, s, d_jobs + j0);
    }
}

void launch_voigt_gradient(const double* x, const double* y, long long n, double* K, double* GX, double* GY, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(voigt_gradient_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n, K, GX, GY);
}

void launch_voigt_function(const double* x, const double* y, long long n, double* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(voigt_function_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n, out);
}

void launch_regrid(const double* work, long long n_work, double* out, long long n_base, double start,
                   double stop, hipStream_t s) {
    if (n_base <= 0) return;
    const double step_w = n_work > 1 ? (stop - start) / (double)(n_work - 1) : 0.0;
    const double step_b = n_base > 1 ? (stop - start) / (double)(n_base - 1) : 0.0;
    hipLaunchKernelGGL(regrid_kernel, dim3((unsigned)((n_base + 255) / 256)), dim3(256), 0, s, work, n_work, out,
                       n_base, start, stop, step_w, step_b);
}

static int sweep_blocks(long long n) {       // (one point per thread on a larger grid measured no faster: 442 vs 433 us for the column)
#ifdef LBL_DIAG
    static const long long cap = getenv("LBL_DIAG_SWEEP_BLOCKS") ? atoll(getenv("LBL_DIAG_SWEEP_BLOCKS")) : 4096;
#else
    constexpr long long cap = 4096;
#endif
    long long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <bool NT, bool BUDGET>
static void launch_layer_sweep_nt(const SweepArgs& a, hipStream_t s) {
#ifdef LBL_DIAG
    static const bool pairs = !getenv("LBL_DIAG_SWEEP_NP1");
#else
    constexpr bool pairs = true;
#endif
    if (pairs && (a.first & 1) == 0 && a.count >= 2) {      // two points per thread with 16-byte accesses; an odd last point by itself
        SweepArgs m = a;
        m.count = a.count & ~1LL;
        hipLaunchKernelGGL((layer_sweep_kernel<NT, 2, BUDGET>), dim3(sweep_blocks(m.count / 2)), dim3(256), 0, s, m);
        if (a.count & 1) {
            SweepArgs t = a;
            t.first = a.first + m.count; t.count = 1;
            hipLaunchKernelGGL((layer_sweep_kernel<NT, 1, BUDGET>), dim3(1), dim3(64), 0, s, t);
        }
        return;
    }
    hipLaunchKernelGGL((layer_sweep_kernel<NT, 1, BUDGET>), dim3(sweep_blocks(a.count)), dim3(256), 0, s, a);
}

void launch_layer_sweep(const SweepArgs& a, hipStream_t s) {
    if (a.count <= 0) return;
    if (a.budget) { if (a.variant) launch_layer_sweep_nt<true, true>(a, s); else launch_layer_sweep_nt<false, true>(a, s); return; }
    if (a.variant) launch_layer_sweep_nt<true, false>(a, s);
    else launch_layer_sweep_nt<false, false>(a, s);
}

template <bool BUDGET>
static void launch_column_step_b(const ColumnStepArgs* d_args, long long first, long long count, hipStream_t s, bool kfold);

void launch_column_step(const ColumnStepArgs* d_args, long long first, long long count, hipStream_t s, int budget, int kfold) {
    if (count <= 0) return;
    if (budget) launch_column_step_b<true>(d_args, first, count, s, kfold != 0);
    else launch_column_step_b<false>(d_args, first, count, s, false);
}

template <bool BUDGET>
static void launch_column_step_b(const ColumnStepArgs* d_args, long long first, long long count, hipStream_t s, bool kfold) {
#ifdef LBL_DIAG
    static const bool pairs = !getenv("LBL_DIAG_COLUMN_NP1");
#else
    constexpr bool pairs = true;
#endif
    // default arithmetic: four points per thread (32-byte loads, three terms per batch; one Planck exp per thread and layer);
    // the reference's rounding chain: two (four measured slower there in round 3: 174 VGPRs with six terms per batch)
    if constexpr (BUDGET) {
        if (pairs && (first & 3) == 0 && count >= 4) {
            const long long quad = count & ~3LL;
            if (kfold) hipLaunchKernelGGL((column_step_kernel<4, true, true>), dim3(sweep_blocks(quad / 4)), dim3(256), 0, s, d_args, first, quad);
            else hipLaunchKernelGGL((column_step_kernel<4, true>), dim3(sweep_blocks(quad / 4)), dim3(256), 0, s, d_args, first, quad);
            if (count & 3) hipLaunchKernelGGL((column_step_kernel<1, true>), dim3(1), dim3(64), 0, s, d_args, first + quad, count & 3);
            return;
        }
    }
    if (pairs && (first & 1) == 0 && count >= 2) {     // two points per thread with 16-byte loads; an odd last point by itself
        const long long even = count & ~1LL;
        hipLaunchKernelGGL((column_step_kernel<2, BUDGET>), dim3(sweep_blocks(even / 2)), dim3(256), 0, s, d_args, first, even);
        if (count & 1) hipLaunchKernelGGL((column_step_kernel<1, BUDGET>), dim3(1), dim3(64), 0, s, d_args, first + even, 1LL);
        return;
    }
    hipLaunchKernelGGL((column_step_kernel<1, BUDGET>), dim3(sweep_blocks(count)), dim3(256), 0, s, d_args, first, count);
}

void launch_column_sweep(const ColumnArgs* d_args, long long count, hipStream_t s, int budget) {
    if (count <= 0) return;
    if (budget) hipLaunchKernelGGL(column_sweep_kernel<true>, dim3(sweep_blocks(count)), dim3(256), 0, s, d_args);
    else hipLaunchKernelGGL(column_sweep_kernel<false>, dim3(sweep_blocks(count)), dim3(256), 0, s, d_args);
}

// emissivity / absorbance / optical depth from a transmittance array
// (pyradClasses.py:73-76, 330-340, 596-606, 718-732)
__global__ __launch_bounds__(256) void optical_kernel(const double* __restrict__ tr, long long n, int kind,
                                                      double* __restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        const double t = tr[j];
        double v;
        if (kind == 0) v = 1.0 - t;                  // emissivity = 1 - transmittance
        else if (kind == 1) v = log10(1.0 / t);      // absorbance = log10(1 / transmittance)
        else v = -log(t);                            // optical depth = -ln transmittance
        out[j] = v;
    }
}

// zeros + in[0] + in[1] + ... (pyradClasses.py:566-571, 684-689)
__global__ __launch_bounds__(256) void sum_kernel(const SumArgs A) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < A.n; j += stride) {
        double s = 0.0;
        for (int i = 0; i < A.n_in; ++i) s += A.in[i][j];
        A.out[j] = s;
    }
}

// padded all-gather result (slot r = rank r's shard) -> grid order
__global__ __launch_bounds__(256) void gather_compact_kernel(const CompactArgs A) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (int r = 0; r < A.world; ++r) {
        const double* __restrict__ src = A.gathered + (long long)r * A.slot;
        double* __restrict__ dst = A.out + A.first[r];
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < A.count[r]; i += stride) dst[i] = src[i];
    }
}

void launch_gather_compact(const CompactArgs& a, long long max_count, hipStream_t s) {
    if (max_count <= 0) return;
    hipLaunchKernelGGL(gather_compact_kernel, dim3(sweep_blocks(max_count)), dim3(256), 0, s, a);
}

void launch_sum(const SumArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(sum_kernel, dim3(sweep_blocks(a.n)), dim3(256), 0, s, a);
}

void launch_optical(const double* trans, long long n, int kind, double* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(optical_kernel, dim3(sweep_blocks(n)), dim3(256), 0, s, trans, n, kind, out);
}

void launch_planck(double* out, long long n, double start, double stop, double T, double rT, double pa, double pb, hipStream_t s) {
    if (n <= 0) return;
    const double step = n > 1 ? (stop - start) / (double)(n - 1) : 0.0;
    hipLaunchKernelGGL(planck_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, start, stop, step,
                       T, rT, pa, pb);
}


void launch_band_integral(const double* y, long long n, double* partial, double* result, hipStream_t s) {
    const int nb = band_partial_count(n);
    hipLaunchKernelGGL(band_partial_kernel, dim3(nb), dim3(256), 0, s, y, n, partial, (long long)16384);
    hipLaunchKernelGGL(band_final_kernel, dim3(1), dim3(256), 0, s, partial, nb, result);
}

// ---- K5c / K5d launch: one band [first, first + count) ---------------------------------------------------------------
// Groups of NP points aligned to NP on the global grid (the fold's quads for NP = 4) go to kernel<NP>, at most kFluxMaxBlocks
// workgroups (grid-stride beyond, so the partial scratch is bounded); the band's head and tail points (at most 2 (NP - 1))
// to ONE 64-lane workgroup of kernel<1>, whose partial follows the others'; then the fixed-order reduction into out[0 .. nv).
int column_transport_partials(long long count, int np) {
    const long long groups = count / np + 1;
    return (int)std::min<long long>((groups + 255) / 256, kFluxMaxBlocks) + 1;
}

template <int NP, class Args>
static void launch_column_band(void (*kernel_np)(const Args*, long long, long long, long long, long long, double*),
                               void (*kernel_1)(const Args*, long long, long long, long long, long long, double*),
                               const Args* d_args, int nv, long long first, long long count, double* partial, double* out,
                               hipStream_t s) {
    if (count <= 0) return;
    const long long end = first + count;
    const long long q0 = (first + NP - 1) & ~(long long)(NP - 1);
    long long q1 = end & ~(long long)(NP - 1);
    if (q1 < q0) q1 = q0;
    const long long nq = q1 - q0;
    const long long nh = std::min(q0, end) - first;
    const long long nt = end > q1 ? end - q1 : 0;
    int blocks = 0;
    if (nq > 0) {
        blocks = (int)std::min<long long>((nq / NP + 255) / 256, kFluxMaxBlocks);
        hipLaunchKernelGGL(kernel_np, dim3(blocks), dim3(256), 0, s, d_args, q0, nq, q0, 0LL, partial);
    }
    if (nh + nt > 0) {
        hipLaunchKernelGGL(kernel_1, dim3(1), dim3(64), 0, s, d_args, nh > 0 ? first : q1, nh, q1, nt,
                           partial + (long long)blocks * nv);
        ++blocks;
    }
    hipLaunchKernelGGL(column_flux_final_kernel, dim3(nv), dim3(256), 0, s, partial, blocks, nv, out);
}

// f(std::integral_constant<int, NA>) for n_angles = NA in 1..kMaxFluxAngles
template <class F>
static void with_angles(int n_angles, F f) {
    switch (n_angles) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: break;
    }
}

void launch_column_flux(const FluxArgs* d_args, int n_layers, int n_angles, long long first, long long count, double* partial,
                        double* level_flux, hipStream_t s) {
    with_angles(n_angles, [&](auto na) {
        constexpr int NA = decltype(na)::value;
        launch_column_band<4>(column_flux_kernel<4, NA>, column_flux_kernel<1, NA>, d_args, 2 * (n_layers + 1), first, count,
                              partial, level_flux, s);
    });
}

// K5g: K5c's launch for the kernel that meets a reflecting surface between its two walks
void launch_surface_flux(const SurfaceFluxArgs* d_args, int n_layers, int n_angles, long long first, long long count,
                         double* partial, double* level_flux, hipStream_t s) {
    with_angles(n_angles, [&](auto na) {
        constexpr int NA = decltype(na)::value;
        launch_column_band<4>(surface_flux_kernel<4, NA>, surface_flux_kernel<1, NA>, d_args, 2 * (n_layers + 1), first, count,
                              partial, level_flux, s);
    });
}

// K5k: K5c's launch twice over one partial block (stream order keeps the first reduction ahead of the second kernel): the
// beams' downward walk into the down half of level_flux, then the Lambertian upward walk into the up half; with a specular
// surface the beam kernel does both walks and fills both halves.
void launch_solar(const SolarArgs* d_args, int n_layers, int n_beams, int n_angles, int reflection, long long first,
                  long long count, double* partial, double* level_flux, hipStream_t s) {
    const int levels = n_layers + 1;
    with_angles(n_beams, [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        if (reflection == 1)
            launch_column_band<4>(solar_beam_kernel<4, NB>, solar_beam_kernel<1, NB>, d_args, 2 * levels, first, count, partial,
                                  level_flux, s);
        else
            launch_column_band<4>(solar_beam_kernel<4, NB>, solar_beam_kernel<1, NB>, d_args, levels, first, count, partial,
                                  level_flux + levels, s);
    });
    if (reflection == 1) return;
    with_angles(n_angles, [&](auto na) {
        constexpr int NA = decltype(na)::value;
        launch_column_band<4>(solar_diffuse_kernel<4, NA>, solar_diffuse_kernel<1, NA>, d_args, levels, first, count, partial,
                              level_flux, s);
    });
}

// K5l, K5m: the partial-sum slots of a band of `count` points
int twostream_partials(long long count) {
    return (int)std::min<long long>(std::max<long long>((count + kTwoStreamTile - 1) / kTwoStreamTile, 1), kFluxMaxBlocks);
}

// One pass of a band for K5l and K5m - the downward kernel over the pass's points, one per thread (launch_down(tiles) launches
// the family's), then its upward kernel with one workgroup per partial slot that the pass's tiles reach (a workgroup takes the
// tiles of its slot in ascending order).
template <class Args, class LaunchDown, class UpKernel>
static void scatter_pass(const Args* d_args, LaunchDown launch_down, UpKernel up_kernel, long long band_first, long long first,
                         long long count, int slots, double* partial, hipStream_t s) {
    if (count <= 0) return;
    const long long tiles = (count + kTwoStreamTile - 1) / kTwoStreamTile;
    launch_down((unsigned)tiles);
    hipLaunchKernelGGL(up_kernel, dim3((unsigned)std::min<long long>(tiles, slots)), dim3(kTwoStreamTile), 0, s, d_args,
                       (first - band_first) / kTwoStreamTile, first, count, slots, partial);
}

// scatter_flux_down_kernel<linear> over the pass's points (K5m's and K5n's first kernel)
static void launch_scatter_flux_down(const ScatterFluxArgs* d_args, bool linear, unsigned tiles, long long first, long long count,
                                     hipStream_t s) {
    const auto kernel = linear ? scatter_flux_down_kernel<true> : scatter_flux_down_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kTwoStreamTile), 0, s, d_args, first, count);
}

void launch_scatter_pass(const TwoStreamArgs* d_args, int n_beams, long long band_first, long long first, long long count,
                         int slots, double* partial, hipStream_t s) {
    scatter_pass(d_args, [&](unsigned tiles) {
        with_angles(n_beams, [&](auto nb) {
            hipLaunchKernelGGL(twostream_down_kernel<decltype(nb)::value>, dim3(tiles), dim3(kTwoStreamTile), 0, s, d_args, first,
                               count);
        });
    }, twostream_up_kernel, band_first, first, count, slots, partial, s);
}

void launch_scatter_pass(const ScatterFluxArgs* d_args, bool linear, long long band_first, long long first, long long count,
                         int slots, double* partial, hipStream_t s) {
    scatter_pass(d_args, [&](unsigned tiles) { launch_scatter_flux_down(d_args, linear, tiles, first, count, s); },
                 scatter_flux_up_kernel, band_first, first, count, slots, partial, s);
}

void launch_scatter_final_values(int nv, int slots, const double* partial, double* values, hipStream_t s) {
    hipLaunchKernelGGL(column_flux_final_kernel, dim3(nv), dim3(256), 0, s, partial, slots, nv, values);
}

void launch_scatter_final(int rows, int n_layers, int slots, const double* partial, double* level_flux, hipStream_t s) {
    launch_scatter_final_values(rows * (n_layers + 1), slots, partial, level_flux, s);
}

// K5p's pass: its downward kernel, then its upward kernel over the partial slots that the pass's tiles reach
void launch_scatter_pass(const ScatterJacArgs* d_args, bool linear, long long band_first, long long first, long long count,
                         int slots, double* partial, hipStream_t s) {
    const auto down = linear ? scatter_jacobian_down_kernel<true> : scatter_jacobian_down_kernel<false>;
    const auto up = linear ? scatter_jacobian_up_kernel<true> : scatter_jacobian_up_kernel<false>;
    scatter_pass(d_args, [&](unsigned tiles) {
        hipLaunchKernelGGL(down, dim3(tiles), dim3(kTwoStreamTile), 0, s, d_args, first, count);
    }, up, band_first, first, count, slots, partial, s);
}

// f(std::integral_constant<int, NV>) for the view count rounded up to NV in {1, 2, 4, 8, 16}
template <class F>
static void with_views(int n_views, F f) {
    if (n_views <= 1) f(std::integral_constant<int, 1>{});
    else if (n_views <= 2) f(std::integral_constant<int, 2>{});
    else if (n_views <= 4) f(std::integral_constant<int, 4>{});
    else if (n_views <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

void launch_scatter_radiance_pass(const ScatterRadianceArgs* d_args, bool linear, int n_views, long long first, long long count,
                                  hipStream_t s) {
    if (count <= 0) return;
    const unsigned tiles = (unsigned)((count + kTwoStreamTile - 1) / kTwoStreamTile);
    launch_scatter_flux_down(d_args, linear, tiles, first, count, s);       // (the block begins with K5m's)
    with_views(n_views, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        const auto kernel = linear ? scatter_radiance_up_kernel<true, NV> : scatter_radiance_up_kernel<false, NV>;
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kTwoStreamTile), 0, s, d_args, first, count);
    });
}

void launch_beam_view_pass(const BeamViewArgs* d_args, int n_views, long long first, long long count, hipStream_t s) {
    if (count <= 0) return;
    const unsigned tiles = (unsigned)((count + kTwoStreamTile - 1) / kTwoStreamTile);
    hipLaunchKernelGGL(twostream_down_kernel<1>, dim3(tiles), dim3(kTwoStreamTile), 0, s, d_args, first,
                       count);                                              // (the block begins with K5l's)
    with_views(n_views, [&](auto nv) {
        hipLaunchKernelGGL(beam_view_kernel<decltype(nv)::value>, dim3(tiles), dim3(kTwoStreamTile), 0, s, d_args, first, count);
    });
}

// The points per thread of the three column Jacobian kernels: 4 with one and two angles, 2 beyond.  One rule, three reasons:
// K5d keeps three values per angle and point and no instantiation may spill (DESIGN.md "K5d"); K5h takes K5d's groups of
// points, so that a black surface gives K5d's bits, and its walk 2 keeps six values per angle and point alive (DESIGN.md
// "K5h"); K5j takes K5h's groups, so that equal edge temperatures give K5h's bits, and a step of it keeps four Planck values,
// g, g' and h beside the six (DESIGN.md "K5j").
template <int NA> constexpr int jacobian_np() { return NA <= 2 ? 4 : 2; }

int jacobian_points(int n_angles) {
    int np = 1;
    with_angles(n_angles, [&](auto na) { np = jacobian_np<decltype(na)::value>(); });
    return np;
}

void launch_column_jacobian(const JacArgs* d_args, int n_layers, int n_angles, int n_terms, long long first, long long count,
                            double* partial, double* jac, hipStream_t s) {
    with_angles(n_angles, [&](auto na) {
        constexpr int NA = decltype(na)::value;
        constexpr int NP = jacobian_np<NA>();
        launch_column_band<NP>(column_jacobian_kernel<NP, NA>, column_jacobian_kernel<1, NA>, d_args,
                               jacobian_slots(2, 1, n_layers, n_terms), first, count, partial, jac, s);
    });
}

// K5e: the aligned groups of 4 points for the bundles of kRayBundle rays (order[0 .. kRayBundle n_bundles)) and then for the
// single rays behind them, the head and tail points (at most 6) for every ray on its own in one 64-lane workgroup each; the
// split of the points is launch_column_band's.  No grid-stride bound: nothing here is sized by the grid.  One split for
// every ray kernel (K5e - K5j): `bundle` is its <4, kRayBundle>, `single` its <4, 1> and `tail` its <1, 1> instantiation.
template <class Args>
using RayKernel = void (*)(const Args*, long long, long long, long long, long long, int);

template <class Args>
static void launch_ray_split(RayKernel<Args> bundle, RayKernel<Args> single, RayKernel<Args> tail, const Args* d_args,
                             long long n, int n_rays, int n_bundles, hipStream_t s) {
    constexpr int NP = 4;
    if (n <= 0 || n_rays <= 0) return;
    const long long q1 = n & ~(long long)(NP - 1);
    const long long nt = n - q1;
    const int n_single = n_rays - kRayBundle * n_bundles;
    if (q1 > 0) {
        const unsigned blocks = (unsigned)((q1 / NP + 255) / 256);
        if (n_bundles > 0)
            hipLaunchKernelGGL(bundle, dim3(blocks, n_bundles), dim3(256), 0, s, d_args, 0LL, q1, 0LL, 0LL, 0);
        if (n_single > 0)
            hipLaunchKernelGGL(single, dim3(blocks, n_single), dim3(256), 0, s, d_args, 0LL, q1, 0LL, 0LL, kRayBundle * n_bundles);
    }
    if (nt > 0) hipLaunchKernelGGL(tail, dim3(1, n_rays), dim3(64), 0, s, d_args, q1, 0LL, q1, nt, 0);
}

void launch_ray_radiance(const RayArgs* d_args, long long n, int n_rays, int n_bundles, hipStream_t s) {
    launch_ray_split<RayArgs>(ray_radiance_kernel<4, kRayBundle>, ray_radiance_kernel<4, 1>, ray_radiance_kernel<1, 1>, d_args, n,
                              n_rays, n_bundles, s);
}

// K5g: launch_ray_radiance's split of the points and of the rays for the kernel that knows surface markers
void launch_ray_surface(const RaySurfaceArgs* d_args, long long n, int n_rays, int n_bundles, hipStream_t s) {
    launch_ray_split<RaySurfaceArgs>(ray_surface_kernel<4, kRayBundle>, ray_surface_kernel<4, 1>, ray_surface_kernel<1, 1>, d_args,
                                     n, n_rays, n_bundles, s);
}

// K5i: K5g's launches - 4 points per thread for every angle count and bundle size, so that with equal edge temperatures the
// one-exp Planck path starts from the same points and returns K5g's bits
void launch_linear_flux(const LinearFluxArgs* d_args, int n_layers, int n_angles, long long first, long long count,
                        double* partial, double* level_flux, hipStream_t s) {
    with_angles(n_angles, [&](auto na) {
        constexpr int NA = decltype(na)::value;
        launch_column_band<4>(linear_flux_kernel<4, NA>, linear_flux_kernel<1, NA>, d_args, 2 * (n_layers + 1), first, count,
                              partial, level_flux, s);
    });
}

void launch_linear_ray(const LinearRayArgs* d_args, long long n, int n_rays, int n_bundles, hipStream_t s) {
    launch_ray_split<LinearRayArgs>(linear_ray_kernel<4, kRayBundle>, linear_ray_kernel<4, 1>, linear_ray_kernel<1, 1>, d_args, n,
                                    n_rays, n_bundles, s);
}

// K5f: launch_ray_radiance's split of the points and of the rays (the radiance is K5e's bit for bit only on K5e's own groups
// of 4 points: the one-exp Planck path starts from the thread's first point).  4 points per thread hold 3 doubles per ray
// and point, 48 for a bundle, without scratch (DESIGN.md "K5f"); a call without terms takes the bundle kernel without the
// term loop.
void launch_ray_jacobian(const RayJacArgs* d_args, long long n, int n_rays, int n_bundles, int n_terms, hipStream_t s) {
    launch_ray_split<RayJacArgs>(n_terms > 0 ? ray_jacobian_kernel<4, kRayBundle, true> : ray_jacobian_kernel<4, kRayBundle, false>,
                                 ray_jacobian_kernel<4, 1, true>, ray_jacobian_kernel<1, 1, true>, d_args, n, n_rays, n_bundles, s);
}

// K5h: K5d's launch at K5d's points per thread (jacobian_np)
void launch_surface_jacobian(const SurfaceJacArgs* d_args, int n_layers, int n_angles, int n_terms, long long first,
                             long long count, double* partial, double* jac, hipStream_t s) {
    with_angles(n_angles, [&](auto na) {
        constexpr int NA = decltype(na)::value;
        constexpr int NP = jacobian_np<NA>();
        launch_column_band<NP>(surface_jacobian_kernel<NP, NA>, surface_jacobian_kernel<1, NA>, d_args,
                               jacobian_slots(3, 1, n_layers, n_terms), first, count, partial, jac, s);
    });
}

// K5h: launch_ray_jacobian's split of the points and of the rays for the kernel that knows surface markers
void launch_ray_surface_jacobian(const RaySurfaceJacArgs* d_args, long long n, int n_rays, int n_bundles, int n_terms,
                                 hipStream_t s) {
    launch_ray_split<RaySurfaceJacArgs>(n_terms > 0 ? ray_surface_jacobian_kernel<4, kRayBundle, true>
                                                    : ray_surface_jacobian_kernel<4, kRayBundle, false>,
                                        ray_surface_jacobian_kernel<4, 1, true>, ray_surface_jacobian_kernel<1, 1, true>, d_args, n,
                                        n_rays, n_bundles, s);
}

// K5j: K5h's launches.  The column's points per thread are jacobian_np's; the rays keep K5i's groups of 4 points,
// which is what makes `radiance` lbl_ray_radiance_linear_dev's bit for bit.  (One bundle kernel: without the term loop it
// spills two registers, and it runs at one wave per SIMD either way.)
void launch_linear_jacobian(const LinearJacArgs* d_args, int n_layers, int n_angles, int n_terms, long long first,
                            long long count, double* partial, double* jac, hipStream_t s) {
    with_angles(n_angles, [&](auto na) {
        constexpr int NA = decltype(na)::value;
        constexpr int NP = jacobian_np<NA>();
        launch_column_band<NP>(linear_jacobian_kernel<NP, NA>, linear_jacobian_kernel<1, NA>, d_args,
                               jacobian_slots(3, 2, n_layers, n_terms), first, count, partial, jac, s);
    });
}

void launch_linear_ray_jacobian(const LinearRayJacArgs* d_args, long long n, int n_rays, int n_bundles, hipStream_t s) {
    launch_ray_split<LinearRayJacArgs>(ray_linear_jacobian_kernel<4, kRayBundle>, ray_linear_jacobian_kernel<4, 1>,
                                       ray_linear_jacobian_kernel<1, 1>, d_args, n, n_rays, n_bundles, s);
}

void launch_line_survey(const double* nu, const double* sw, int n_lines, double range_min, double resolution,
                        double* out, long long n_base, hipStream_t s) {
    if (n_lines <= 0) return;
    hipLaunchKernelGGL(line_survey_kernel, dim3((n_lines + 255) / 256), dim3(256), 0, s, nu, sw, n_lines, range_min,
                       resolution, out, n_base);
}

// ----------------------------------------------------------------------------------------
// K8: instrument channels (lbl_ils_convolve_dev; the definition is in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// out[r][c] = sum_j w_cj S_r[j] / sum_j w_cj over the channel's support, w_cj = shape(((double)j - p_c) * step / width_c).
// One workgroup per (channel, block of NR rows): a thread evaluates the weight of its point once and uses it for the NR rows
// and the normaliser, all held in registers.  Every sum is carried as an unevaluated pair (hi, lo): the product w S exactly
// (fma), the addition by two-sum with the rounding errors collected in lo.  The normaliser goes through the very same steps
// in the same order, so numerator and normaliser of a constant row S = s are s sum_j w_cj and sum_j w_cj to ~2^-100 of each,
// and the final division returns s itself; plain fp64 sums do not (fl(s x) is not s fl(x) unless s is a power of two).
// Order of every sum: thread t takes the points t, t + 256, ...; the wave's 64 pairs are added by a fixed shuffle tree; thread
// r adds the four waves' pairs of row r in wave order.  No atomics: the same inputs give the same bits, and a row's bits do
// not depend on the rows beside it.
// Workgroup ids are dealt round-robin over the eight XCDs; gridDim.x is a multiple of 8, so XCD x gets the ids x, x + 8, ...
// of every grid row, and slot (id & 7) * chunk + (id >> 3) of the channel list sorted by support start gives each XCD one
// contiguous run of overlapping supports for its own L2.
struct dd { double hi, lo; };

__device__ __forceinline__ void dd_add(dd& a, double p, double e) {
#pragma clang fp contract(off)
    const double s = a.hi + p;
    const double bb = s - a.hi;
    const double err = (a.hi - (s - bb)) + (p - bb);
    a.hi = s;
    a.lo += err + e;
}

__device__ __forceinline__ dd dd_wave_sum(dd a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double h2 = __shfl_down(a.hi, off, 64), l2 = __shfl_down(a.lo, off, 64);
        dd_add(a, h2, l2);
    }
    return a;
}

template <int SHAPE>
__device__ __forceinline__ double ils_weight(double x, double width, const IlsArgs& A, const double* __restrict__ table) {
#pragma clang fp contract(off)
    if (SHAPE == ILS_TABLE) {
        if (!(x >= -A.table_half && x <= A.table_half)) return 0.0;
        const double u = (x + A.table_half) * A.table_rdx;
        int i = (int)u;
        i = i < 0 ? 0 : (i > A.n_table - 2 ? A.n_table - 2 : i);
        const double f = u - (double)i;
        const double v0 = table[i], v1 = table[i + 1];
        return v0 + f * (v1 - v0);
    }
    const double t = x / width;
    if (SHAPE == ILS_GAUSSIAN) return exp(-2.772588722239781 * (t * t));          // -4 ln 2
    if (SHAPE == ILS_TRIANGLE) return fmax(0.0, 1.0 - fabs(t));
    if (SHAPE == ILS_BOXCAR) return fabs(t) <= 0.5 ? 1.0 : 0.0;
    const double pt = kPi * t;                                                     // ILS_SINC
    return pt == 0.0 ? 1.0 : sin(pt) / pt;
}

template <int SHAPE, int NR>
__global__ __launch_bounds__(256) void ils_convolve_kernel(const IlsArgs* __restrict__ Ap) {
#pragma clang fp contract(off)
    const IlsArgs& A = *Ap;
    const char* base = (const char*)Ap;
    const long long slot = (long long)(blockIdx.x & 7) * A.chunk + (blockIdx.x >> 3);
    if (slot >= A.n_channels) return;                                               // (workgroup-uniform; gridDim.x = 8 chunk)
    const int c = ((const int32_t*)(base + A.off_order))[slot];
    const double p = ((const double*)(base + A.off_position))[c];
    const double width = ((const double*)(base + A.off_width))[c];
    const long long first = ((const long long*)(base + A.off_first))[c];
    const long long count = ((const long long*)(base + A.off_count))[c];
    const double* table = (const double*)(base + A.off_table);
    const double* const* rows = (const double* const*)(base + A.off_rows);
    const int r0 = blockIdx.y * NR;
    // (the rows past the last one repeat it; their sums are not stored)
    const double* row[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) row[i] = rows[min(r0 + i, A.n_rows - 1)] + first;

    dd den = {0.0, 0.0}, num[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) num[i] = {0.0, 0.0};
    for (long long j = threadIdx.x; j < count; j += 256) {
        double v[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) v[i] = row[i][j];
        const double x = ((double)(first + j) - p) * A.step;
        const double w = ils_weight<SHAPE>(x, width, A, table);
        dd_add(den, w, 0.0);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const double pr = w * v[i];
            dd_add(num[i], pr, fma(w, v[i], -pr));
        }
    }

    __shared__ dd sh[4][NR + 1];
    const int wave = threadIdx.x >> 6;
    den = dd_wave_sum(den);
#pragma unroll
    for (int i = 0; i < NR; ++i) num[i] = dd_wave_sum(num[i]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) sh[wave][i] = num[i];
        sh[wave][NR] = den;
    }
    __syncthreads();
    if (threadIdx.x < NR && r0 + (int)threadIdx.x < A.n_rows) {
        dd nu = sh[0][threadIdx.x], de = sh[0][NR];
        for (int k = 1; k < 4; ++k) {
            dd_add(nu, sh[k][threadIdx.x].hi, sh[k][threadIdx.x].lo);
            dd_add(de, sh[k][NR].hi, sh[k][NR].lo);
        }
        // (nu.hi + nu.lo) / (de.hi + de.lo): the quotient of the leading parts, then its exact remainder and the trailing parts
        const double q = nu.hi / de.hi;
        const double rem = fma(-q, de.hi, nu.hi);
        A.out[(size_t)(r0 + threadIdx.x) * (size_t)A.n_channels + (size_t)c] = q + ((rem + nu.lo) - q * de.lo) / de.hi;
    }
}

template <int NR>
static void launch_ils_shape(const IlsArgs* d_args, int shape, dim3 grid, hipStream_t s) {
    switch (shape) {
        case ILS_GAUSSIAN: hipLaunchKernelGGL((ils_convolve_kernel<ILS_GAUSSIAN, NR>), grid, dim3(256), 0, s, d_args); break;
        case ILS_TRIANGLE: hipLaunchKernelGGL((ils_convolve_kernel<ILS_TRIANGLE, NR>), grid, dim3(256), 0, s, d_args); break;
        case ILS_BOXCAR: hipLaunchKernelGGL((ils_convolve_kernel<ILS_BOXCAR, NR>), grid, dim3(256), 0, s, d_args); break;
        case ILS_SINC: hipLaunchKernelGGL((ils_convolve_kernel<ILS_SINC, NR>), grid, dim3(256), 0, s, d_args); break;
        case ILS_TABLE: hipLaunchKernelGGL((ils_convolve_kernel<ILS_TABLE, NR>), grid, dim3(256), 0, s, d_args); break;
        default: break;
    }
}

// a single row travels alone (NR = 1); more rows in blocks of kIlsRowBlock.  grid.x = 8 * chunk (see above)
void launch_ils_convolve(const IlsArgs* d_args, int shape, int n_rows, long long n_channels, hipStream_t s) {
    if (n_rows < 1 || n_channels < 1) return;
    const unsigned gx = 8u * (unsigned)((n_channels + 7) / 8);
    if (n_rows == 1) launch_ils_shape<1>(d_args, shape, dim3(gx, 1), s);
    else launch_ils_shape<kIlsRowBlock>(d_args, shape, dim3(gx, (n_rows + kIlsRowBlock - 1) / kIlsRowBlock), s);
}

// ----------------------------------------------------------------------------------------
// K9: k-distributions (lbl_rank_order_dev, lbl_ranked_means_dev; the definition is in include/pyrad_hip.h)
// ----------------------------------------------------------------------------------------
// Ranking.  A segment is one band of one row.  Point i of it (band-local index) is the pair (key, i): key = the bits of the
// value in sign-magnitude order after -0 -> +0 and every NaN -> all ones, so that unsigned order of the keys is numpy's
// ascending order with NaN last, and the index settles every tie in grid order - the stable order.  All pairs of a segment
// are distinct, so any correct sort gives the same permutation.
//   kdist_tile_sort_kernel   one workgroup per tile of kKdistTile points: keys built, bitonic network over the next power of
//                            two of the tile's points in LDS (padded with pairs that sort last);
//   kdist_merge_kernel       pass p merges runs of kKdistTile << p pairs two by two: one workgroup per kKdistTile outputs finds
//                            its two input ranges by a merge-path search on the output diagonals, brings them to LDS, every
//                            thread finds the start of its 8 outputs the same way in LDS and merges them serially.
// Whichever launch completes a segment (the tile sort for a band of one tile, else the band's last merge pass) writes the
// results instead of pairs: order = first + index as a double, sorted = the row's value there (gathered, so bit for bit).
// grid = (work items of one row, rows); the item -> band map is a prefix table of at most 65 entries in the argument block.
__device__ __forceinline__ unsigned long long kdist_key(double x) {
    unsigned long long b = (unsigned long long)__double_as_longlong(x);
    if (x != x) return ~0ull;
    if (x == 0.0) b = 0ull;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ bool kdist_less(unsigned long long ka, unsigned int ia, unsigned long long kb, unsigned int ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// number of pairs taken from A among the first d outputs of merge(A[0, na), B[0, nb)) (0 <= d <= na + nb)
template <typename KP, typename IP>
__device__ __forceinline__ long long kdist_merge_path(KP ak, IP ai, long long na, KP bk, IP bi, long long nb, long long d) {
    long long lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (kdist_less(ak[mid], ai[mid], bk[d - 1 - mid], bi[d - 1 - mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int kdist_band_of(const int32_t* __restrict__ start, int n_bands, int item) {
    int b = 0;
    while (b + 1 < n_bands && item >= start[b + 1]) ++b;
    return b;
}

// `total` pairs of LDS (sk, si) leave for the segment's outputs at [at, at + total): pairs, or the results when the segment is complete
__device__ __forceinline__ void kdist_emit(const RankArgs& A, const unsigned long long* sk, const unsigned int* si, int total,
                                           bool last, int buf, long long row_at, long long first, const double* __restrict__ x) {
    if (last) {
        for (int i = threadIdx.x; i < total; i += 256) {
            const unsigned int j = si[i];
            A.order[row_at + i] = (double)(first + (long long)j);
            if (A.sorted) A.sorted[row_at + i] = x[j];
        }
    } else {
        for (int i = threadIdx.x; i < total; i += 256) {
            A.keys[buf][row_at + i] = sk[i];
            A.idx[buf][row_at + i] = si[i];
        }
    }
}

__global__ __launch_bounds__(256) void kdist_tile_sort_kernel(const RankArgs* __restrict__ Ap) {
    __shared__ unsigned long long sk[kKdistTile];
    __shared__ unsigned int si[kKdistTile];
    const RankArgs& A = *Ap;
    const int b = kdist_band_of(A.item_start[0], A.n_bands, blockIdx.x);
    const long long t0 = (long long)((int)blockIdx.x - A.item_start[0][b]) * kKdistTile;
    const long long count = A.count[b], first = A.first[b];
    if (t0 >= count) return;                                                        // (workgroup-uniform; never with the host's grid)
    const int valid = (int)(count - t0 < kKdistTile ? count - t0 : kKdistTile);
    const double* __restrict__ x = ((const double* const*)((const char*)Ap + A.off_rows))[blockIdx.y] + first;
    int m = 2;
    while (m < valid) m <<= 1;
    for (int i = threadIdx.x; i < m; i += 256) {
        const bool in = i < valid;
        sk[i] = in ? kdist_key(x[t0 + i]) : ~0ull;
        si[i] = in ? (unsigned int)(t0 + i) : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (m >> 1); t += 256) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long ka = sk[lo], kb = sk[hi];
                const unsigned int ia = si[lo], ib = si[hi];
                const bool up = (lo & k) == 0;
                if (up ? kdist_less(kb, ib, ka, ia) : kdist_less(ka, ia, kb, ib)) {
                    sk[lo] = kb; sk[hi] = ka;
                    si[lo] = ib; si[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    kdist_emit(A, sk, si, valid, A.passes[b] == 0, 0, (long long)blockIdx.y * A.s_total + A.s_start[b] + t0, first, x);
}

__global__ __launch_bounds__(256) void kdist_merge_kernel(const RankArgs* __restrict__ Ap, int p) {
    __shared__ unsigned long long sk[kKdistTile];
    __shared__ unsigned int si[kKdistTile];
    __shared__ long long split[2];
    const RankArgs& A = *Ap;
    const int b = kdist_band_of(A.item_start[p + 1], A.n_bands, blockIdx.x);
    const long long c0 = (long long)((int)blockIdx.x - A.item_start[p + 1][b]) * kKdistTile;
    const long long count = A.count[b], first = A.first[b];
    if (c0 >= count) return;                                                        // (workgroup-uniform; never with the host's grid)
    const long long W = (long long)kKdistTile << p;
    const long long base = c0 & ~(2 * W - 1);                                       // the pair of runs this tile of outputs lies in
    const long long lenA = count - base < W ? count - base : W;
    const long long lenB = count - base - lenA < W ? count - base - lenA : W;
    const long long d0 = c0 - base, d1 = d0 + kKdistTile < lenA + lenB ? d0 + kKdistTile : lenA + lenB;
    const long long seg = (long long)blockIdx.y * A.s_total + A.s_start[b];
    const unsigned long long* __restrict__ ak = A.keys[p & 1] + seg + base;
    const unsigned int* __restrict__ ai = A.idx[p & 1] + seg + base;
    if (threadIdx.x == 0 || threadIdx.x == 64)
        split[threadIdx.x >> 6] = kdist_merge_path(ak, ai, lenA, ak + lenA, ai + lenA, lenB, threadIdx.x ? d1 : d0);
    __syncthreads();
    const long long a0 = split[0], b0 = d0 - a0;
    const int nA = (int)(split[1] - a0), total = (int)(d1 - d0), nB = total - nA;
    for (int i = threadIdx.x; i < total; i += 256) {
        const long long src = i < nA ? a0 + i : lenA + b0 + (i - nA);
        sk[i] = ak[src];
        si[i] = ai[src];
    }
    __syncthreads();
    // the 8 outputs [8 t, 8 t + 8) of this thread
    const int d = min((int)threadIdx.x * 8, total);
    int pa = (int)kdist_merge_path(sk, si, (long long)nA, sk + nA, si + nA, (long long)nB, (long long)d);
    int pb = nA + (d - pa);
    const int endB = nA + nB;
    unsigned long long rk[8];
    unsigned int ri[8];
    unsigned long long ka = pa < nA ? sk[pa] : 0ull, kb = pb < endB ? sk[pb] : 0ull;
    unsigned int ia = pa < nA ? si[pa] : 0u, ib = pb < endB ? si[pb] : 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool takeA = pb >= endB || (pa < nA && kdist_less(ka, ia, kb, ib));
        rk[i] = takeA ? ka : kb;
        ri[i] = takeA ? ia : ib;
        if (takeA) {
            ++pa;
            if (pa < nA) { ka = sk[pa]; ia = si[pa]; }
        } else {
            ++pb;
            if (pb < endB) { kb = sk[pb]; ib = si[pb]; }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (d + i < total) { sk[d + i] = rk[i]; si[d + i] = ri[i]; }
    }
    __syncthreads();
    const double* __restrict__ x = ((const double* const*)((const char*)Ap + A.off_rows))[blockIdx.y] + first;
    kdist_emit(A, sk, si, total, A.passes[b] == p + 1, (p + 1) & 1, seg + c0, first, x);
}

void launch_kdist_rank(const RankArgs* d_args, const RankArgs& host, hipStream_t s) {
    const int nb = host.n_bands;
    if (host.n_rows < 1 || nb < 1) return;
    hipLaunchKernelGGL(kdist_tile_sort_kernel, dim3(host.item_start[0][nb], host.n_rows), dim3(256), 0, s, d_args);
    for (int p = 0; p < kKdistMaxPasses; ++p)
        if (host.item_start[p + 1][nb] > 0)
            hipLaunchKernelGGL(kdist_merge_kernel, dim3(host.item_start[p + 1][nb], host.n_rows), dim3(256), 0, s, d_args, p);
}

// Means over intervals of the rank.  kdist_partial_kernel: one workgroup per kKdistTile ranks of one interval of one row reads
// the order (coalesced), gathers the row there and adds: thread t the ranks t, t + 256, ... in turn, the wave's 64 sums by a
// fixed shuffle tree, the four waves' sums in wave order.  kdist_means_kernel: one wave per (row, interval) adds the
// interval's partial sums - lane l the partials l, l + 64, ... in turn, then the same tree - divides by the number of ranks
// and fetches the order statistics at the edges.  No atomics, one order of additions whatever else is in the call.  Every sum
// starts from -0.0, the identity of IEEE addition for every value (0.0 would turn -0.0 into +0.0); an interval of one rank is
// copied.  An order value outside its band is clamped into it: no read leaves the row.
__device__ __forceinline__ double kdist_wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ long long kdist_point(double o, long long first, long long count) {
    const double lo = (double)first, hi = (double)(first + count - 1);      // (exact: grid indices are far below 2^53)
    o = o >= lo ? o : lo;                                                   // (NaN: first)
    return (long long)(o <= hi ? o : hi);
}

__global__ __launch_bounds__(256) void kdist_partial_kernel(const MeansArgs* __restrict__ Ap) {
#pragma clang fp contract(off)
    __shared__ double sh[4];
    const MeansArgs& A = *Ap;
    const MeansInterval* __restrict__ I = (const MeansInterval*)((const char*)Ap + A.off_intervals);
    int lo = 0, hi = A.g_total - 1;                       // the interval of this chunk: the last one that starts at or before it
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (I[mid].chunk_start <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const MeansInterval iv = I[lo];
    const long long r0 = (long long)((int)blockIdx.x - iv.chunk_start) * kKdistTile;
    const int m = (int)(iv.len - r0 < kKdistTile ? iv.len - r0 : kKdistTile);
    const long long first = A.first[iv.band], count = A.count[iv.band];
    const double* __restrict__ x = ((const double* const*)((const char*)Ap + A.off_rows))[blockIdx.y];
    const double* __restrict__ order = ((const double* const*)((const char*)Ap + A.off_orders))[blockIdx.y] + iv.lo + r0;
    double acc = -0.0;
    for (int i = threadIdx.x; i < m; i += 256) acc += x[kdist_point(order[i], first, count)];
    acc = kdist_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) A.partial[(size_t)blockIdx.y * (size_t)A.n_chunks + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void kdist_means_kernel(const MeansArgs* __restrict__ Ap) {
#pragma clang fp contract(off)
    const MeansArgs& A = *Ap;
    const int g = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= A.g_total) return;                           // (wave-uniform; no barrier below)
    const MeansInterval* __restrict__ I = (const MeansInterval*)((const char*)Ap + A.off_intervals);
    const MeansInterval iv = I[g];
    const int c1 = I[g + 1].chunk_start;
    const double* __restrict__ part = A.partial + (size_t)blockIdx.y * (size_t)A.n_chunks;
    double acc = -0.0;
    for (int c = iv.chunk_start + lane; c < c1; c += 64) acc += part[c];
    acc = kdist_wave_sum(acc);
    if (lane != 0) return;
    const long long first = A.first[iv.band], count = A.count[iv.band];
    const double* __restrict__ x = ((const double* const*)((const char*)Ap + A.off_rows))[blockIdx.y];
    const double* __restrict__ order = ((const double* const*)((const char*)Ap + A.off_orders))[blockIdx.y];
    const double at_edge = x[kdist_point(order[iv.lo], first, count)];
    A.mean[(size_t)blockIdx.y * (size_t)A.g_total + g] = iv.len == 1 ? at_edge : acc / (double)iv.len;
    if (A.lower) {
        double* lower = A.lower + (size_t)blockIdx.y * (size_t)(A.g_total + A.n_bands) + g + iv.band;
        lower[0] = at_edge;
        if (g + 1 == A.g_start[iv.band + 1]) lower[1] = x[kdist_point(order[A.s_start[iv.band] + count - 1], first, count)];
    }
}

void launch_kdist_means(const MeansArgs* d_args, const MeansArgs& host, hipStream_t s) {
    if (host.n_rows < 1 || host.g_total < 1) return;
    hipLaunchKernelGGL(kdist_partial_kernel, dim3(host.n_chunks, host.n_rows), dim3(256), 0, s, d_args);
    hipLaunchKernelGGL(kdist_means_kernel, dim3((host.g_total + 3) / 4, host.n_rows), dim3(256), 0, s, d_args);
}

}  // namespace lbl
