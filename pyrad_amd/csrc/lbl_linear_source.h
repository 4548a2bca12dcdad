// The weight of the linear-in-optical-depth Planck source (K5i of lbl_kernels.hip; the semantics are in include/pyrad_hip.h):
// one text for the device and for the host (tests/test_linear_source_cpu.py compiles this header with g++).
//
//     g(tau) = 1 - (1 - t) / tau,   t = exp(-tau)          -> tau / 2 as tau -> 0,  -> 1 as tau -> inf
//
// A piece of a layer of optical depth tau whose Planck function runs linearly in optical depth from Ba, where the light
// enters, to Bb, where it leaves, emits (1 - t) Ba + g(tau) (Bb - Ba).  The caller passes the t it has already formed.
//
//   tau >= LBL_LINEAR_G_TAU0   the expression itself: 1 - t is exact for t >= 1/2 and rounded once below, the quotient and
//                              the difference are rounded once each - together at most 2^-53 absolute, which against g >=
//                              tau / 2 (1 - tau / 3) is 2^-52 / (tau (1 - tau / 3)) <= 9.7e-16 relative at tau0.  An error of one
//                              ulp(t) <= 2^-53 in the caller's t comes out as 2^-53 / tau absolute: 2 / tau^2 = 32 times as
//                              large relative to tau / 2 at tau0, 3.6e-15 (3.9e-15 against g itself), so a t good to 2 ulp
//                              keeps g inside 1e-14, a tenth of the spectral tolerance 1e-13.  (Measured on the host with
//                              libm's exp against 50 digits: 2.1e-15.)
//   tau <  LBL_LINEAR_G_TAU0   the Taylor series tau (1/2 - tau (1/6 - tau (1/24 - ...))) with LBL_LINEAR_G_TERMS terms,
//                              1/2! .. 1/12!: alternating with falling terms, so the truncation is below the first term left
//                              out, tau^12 / 13!.  Against the leading tau / 2 that is 2 tau0^11 / 13! = 7.7e-17 < 2^-53 =
//                              1.1e-16 at tau0 = 1/4 (8.4e-17 against g itself); ten terms would leave 2 tau0^10 / 12! =
//                              4.0e-15.  t is not used, so its error does not enter.
// g(0) = 0 exactly (the series' leading factor), g(+inf) = 1 (1 - 1 / inf), NaN stays NaN, and g rises with tau.
//
// Its derivative (K5j: the Jacobians of the linear source, d/d ln tau through g' and the weight h = tau g' of Ba):
//
//     g'(tau) = (1 - t (1 + tau)) / tau^2 = ((1 - t) / tau - t) / tau      -> 1/2 as tau -> 0,  -> 0 as tau -> inf
//     h(tau)  = (1 - t) - g(tau) = (1 - t) / tau - t = tau g'(tau)         (formed as tau * linear_source_dg in the kernels)
//
//   tau >= LBL_LINEAR_DG_TAU0  the second expression, q = (1 - t) / tau, hh = q - t, hh / tau: no product 0 * inf at tau = +inf.
//                              It is the first one divided through - the numerator 1 - t (1 + tau) = tau hh carries the same
//                              cancellation, ~2^-53 / (1 - t (1 + tau)) relative.  Below tau = ln 2, 1 - t is exact (t >= 1/2)
//                              and so is q - t (q / 2 <= t <= 2 q); q is rounded once, at most 2^-54 absolute (q < 1), and an
//                              error of one ulp(t) = 2^-53 in the caller's t comes out of hh as 2^-53 (1 + 1 / tau).  With a
//                              t good to 2 ulp, the assumption g's bound makes, hh is off by at most 2^-53 (1/2 + 2 (1 + 1 /
//                              tau)) = 8.7e-16 at tau0 = 3/8, against hh(tau0) = 0.14661 that is 5.9e-15, and 6.0e-15 with
//                              the last division's 2^-53: inside 1e-14, a tenth of the spectral tolerance 1e-13, the rule g
//                              was held to.  It falls as tau grows (hh rises, 1 + 1 / tau falls).  g's own switch-over 1/4
//                              would not do: 2^-53 (1/2 + 2 * 5) / hh(1/4) = 1.17e-15 / 0.10600 = 1.1e-14.  (Measured on the
//                              host with libm's exp against 50 digits: 1.5e-15, tests/test_linear_jacobian_cpu.py.)
//   tau <  LBL_LINEAR_DG_TAU0  the Taylor series 1/2 - tau (1/3 - tau (1/8 - ...)), coefficients (-1)^(n+1) n / (n + 1)! for
//                              n = 1 .. LBL_LINEAR_DG_TERMS: alternating with falling terms, so the truncation is below the
//                              first term left out, 14 tau0^13 / 15! = 3.1e-17, against g'(tau0) = 0.39095 that is 7.9e-17 <
//                              2^-53; twelve terms would leave 13 tau0^12 / 14! = 1.15e-15, 2.9e-15 relative.  Horner's
//                              roundings and the coefficients' add up to below 4e-16.  t is not used.
// g'(0) = 1/2 exactly (the series' last fma adds -0 * s to 0.5), g'(+inf) = 0 ((1 / inf - 0) / inf), NaN stays NaN, and g'
// falls with tau.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LBL_LINEAR_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define LBL_LINEAR_FN inline __attribute__((always_inline))
#endif

// the switch-over and the series' length, exported for the tests
#define LBL_LINEAR_G_TAU0 0.25
#define LBL_LINEAR_G_TERMS 11
#define LBL_LINEAR_DG_TAU0 0.375
#define LBL_LINEAR_DG_TERMS 13

namespace lbl {

LBL_LINEAR_FN double linear_source_g(double tau, double t) {
    // every fused multiply-add is spelled out and the compiler adds none: the same inputs give the same bits in every kernel
    // that inlines this function, whatever surrounds the call
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    // both forms and a select, no branch: tau differs from lane to lane, and with a branch per angle and point in their
    // unrolled loops the flux kernel's four-point bodies spill (DESIGN.md "K5i")
    const double direct = 1.0 - (1.0 - t) / tau;
    // 1 / (n + 2)!, n = 10 .. 0; NaN runs through
    double s = 1.0 / 479001600.0;
    s = fma(-tau, s, 1.0 / 39916800.0);
    s = fma(-tau, s, 1.0 / 3628800.0);
    s = fma(-tau, s, 1.0 / 362880.0);
    s = fma(-tau, s, 1.0 / 40320.0);
    s = fma(-tau, s, 1.0 / 5040.0);
    s = fma(-tau, s, 1.0 / 720.0);
    s = fma(-tau, s, 1.0 / 120.0);
    s = fma(-tau, s, 1.0 / 24.0);
    s = fma(-tau, s, 1.0 / 6.0);
    s = fma(-tau, s, 0.5);
    return tau >= LBL_LINEAR_G_TAU0 ? direct : tau * s;
}

LBL_LINEAR_FN double linear_source_dg(double tau, double t) {
    // (fused multiply-adds spelled out, both forms and a select: as linear_source_g, and for the same reasons)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double direct = ((1.0 - t) / tau - t) / tau;
    // n / (n + 1)! = 1 / ((n + 1)! / n), n = 13 .. 1; NaN runs through
    double s = 1.0 / 6706022400.0;
    s = fma(-tau, s, 1.0 / 518918400.0);
    s = fma(-tau, s, 1.0 / 43545600.0);
    s = fma(-tau, s, 1.0 / 3991680.0);
    s = fma(-tau, s, 1.0 / 403200.0);
    s = fma(-tau, s, 1.0 / 45360.0);
    s = fma(-tau, s, 1.0 / 5760.0);
    s = fma(-tau, s, 1.0 / 840.0);
    s = fma(-tau, s, 1.0 / 144.0);
    s = fma(-tau, s, 1.0 / 30.0);
    s = fma(-tau, s, 1.0 / 8.0);
    s = fma(-tau, s, 1.0 / 3.0);
    s = fma(-tau, s, 0.5);
    return tau >= LBL_LINEAR_DG_TAU0 ? direct : s;
}

}  // namespace lbl
