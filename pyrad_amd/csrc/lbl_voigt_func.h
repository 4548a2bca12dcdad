// The Voigt function K(x, y) = Re w(x + i y), w the Faddeeva function: one text for the device (K2v of lbl_kernels.hip,
// lbl_voigt_function_dev) and for the host (tests/test_voigt_cpu.py compiles this header with g++).
// voigt_kgrad below it adds the gradients the temperature derivative needs (K2v-T, tests/test_voigt_dT_cpu.py).
//
// Domain: x >= 0 and (y == 0 or 1e-5 <= y <= 1e4).  Relative error <= 1e-6 there (measured per branch: DESIGN.md "K2v");
// never negative; NaN in, NaN out; where the true value is below 1e-290 the result lies in [0, 1e-290].  y < 0 is the
// caller's error.  For 0 < y < 1e-5 the same branches run: the far and middle branches keep their relative accuracy (their
// real part is proportional to y term by term), the near branch has an ABSOLUTE error of about 2e-16, so where
// exp(-x^2) has died (x > 4) and only y / (sqrt(pi) x^2) is left the relative error grows like 1 / y: measured
// 2.5e-9 at y = 1e-6, 2.8e-8 at y = 1e-7, 2.5e-7 at y = 1e-8, each at x = 9 to 10.
//
// Branches, by s = x^2 + y^2 (a wave of the accumulate kernel usually takes one: s grows with the distance from the
// line centre, and with the pressure):
//   y == 0               exp(-x^2): the rational forms below have no real part on the real axis
//   s >= kVoigtFar       w ~ i / (sqrt(pi) z) (1 + v + 3 v^2 + 15 v^3 + 105 v^4), v = 1 / (2 z^2): one division, no exp
//   s >= kVoigtMid       the same asymptotic series up to (2 k - 1)!! v^k, k = kVoigtMidTerms
//   else                 Weideman's rational approximation with 48 terms (SIAM J. Numer. Anal. 31 (1994) 1497):
//                        w = 2 p(Z) / (L - i z)^2 + (1 / sqrt(pi)) / (L - i z), Z = (L + i z) / (L - i z), L = sqrt(48 / sqrt 2);
//                        the coefficients are the FFT of exp(-t^2) (L^2 + t^2) on t = L tan(theta / 2) (scripts/voigt_coeffs.py)
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LBL_VOIGT_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define LBL_VOIGT_FN inline __attribute__((always_inline))
#endif

// the switch-overs, exported for the tests (a dense band across every one of them)
#define LBL_VOIGT_S_FAR 400.0        /* s = x^2 + y^2 >= this: five-term asymptotic series */
#define LBL_VOIGT_S_MID 100.0        /* s >= this: long asymptotic series; below: Weideman */
#define LBL_VOIGT_MID_TERMS 16

namespace lbl {

constexpr double kVoigtFar = LBL_VOIGT_S_FAR;
constexpr double kVoigtMid = LBL_VOIGT_S_MID;
constexpr int kVoigtMidTerms = LBL_VOIGT_MID_TERMS;
constexpr int kVoigtWeidemanN = 48;
constexpr double kVoigtWeidemanL = 5.825901260487881;      // sqrt(48 / sqrt(2))
constexpr double kVoigtInvSqrtPi = 0.5641895835477563;

LBL_VOIGT_FN double voigt_k(double x, double y) {
    // every fused multiply-add is spelled out and the compiler adds none: the same inputs give the same bits in every kernel
    // that inlines this function (the accumulate kernel, the elementwise test kernel), whatever surrounds the call
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (y == 0.0) return exp(-x * x);
    const double s = x * x + y * y;
    if (s >= kVoigtMid) {
        if (s > 1.7e308) return 0.0;                  // (x^2 overflowed: the true value is below 1e-300)
        // 1 / z = (x - i y) / s;  v = 1 / (2 z^2)
        const double r = 1.0 / s;
        const double qr = x * r, qi = -(y * r);
        const double vr = 0.5 * (qr * qr - qi * qi), vi = qr * qi;
        double pr, pi_;
        if (s >= kVoigtFar) {
            // P = 1 + v (1 + v (3 + v (15 + 105 v)))
            pr = fma(105.0, vr, 15.0); pi_ = 105.0 * vi;
            double t;
            t = fma(pr, vr, fma(-pi_, vi, 3.0)); pi_ = fma(pr, vi, pi_ * vr); pr = t;
            t = fma(pr, vr, fma(-pi_, vi, 1.0)); pi_ = fma(pr, vi, pi_ * vr); pr = t;
            t = fma(pr, vr, fma(-pi_, vi, 1.0)); pi_ = fma(pr, vi, pi_ * vr); pr = t;
        } else {
            // (2 k - 1)!! for k = 0 .. 16
            const double c[17] = {1.0, 1.0, 3.0, 15.0, 105.0, 945.0, 10395.0, 135135.0, 2027025.0, 34459425.0, 654729075.0,
                                  13749310575.0, 316234143225.0, 7905853580625.0, 213458046676875.0, 6190283353629375.0,
                                  191898783962510625.0};
            pr = c[kVoigtMidTerms]; pi_ = 0.0;
            for (int k = kVoigtMidTerms - 1; k >= 0; --k) {
                const double t = fma(pr, vr, fma(-pi_, vi, c[k]));
                pi_ = fma(pr, vi, pi_ * vr);
                pr = t;
            }
        }
        // Re( i / sqrt(pi) q P ) = -(qr Pi + qi Pr) / sqrt(pi)
        const double k = -kVoigtInvSqrtPi * fma(qr, pi_, qi * pr);
        return k < 0.0 ? 0.0 : k;
    }
    // Weideman, N = 48 (highest power first)
    const double a[kVoigtWeidemanN] = {
        -3.70074341541718826e-17, 3.90809708090504099e-17, 8.91304535964125145e-17, 4.33646987676311602e-17,
        2.10357809007447985e-17, 7.06831347963979208e-20, 3.85910504816624698e-16, 7.25379754852292609e-16,
        -1.87923282206915558e-15, -5.23915859509534328e-15, 9.52753636075451554e-15, 4.23425555842355866e-14,
        -3.19334159628465632e-14, -3.22775731097254591e-13, -9.65501738984251051e-14, 2.21541877720001645e-12,
        3.42533409044184144e-12, -1.19354512668394108e-11, -4.38658676752703712e-11, 2.16220023479657394e-11,
        3.87942207730320342e-10, 5.77528985547910890e-10, -2.01565992731615496e-09, -9.59625471307884432e-09,
        -6.38680992890150548e-09, 6.92700063602607607e-08, 2.65494920068709391e-07, 1.94943374672414598e-07,
        -1.94456577900989678e-06, -9.47563824045082754e-06, -1.90544616191120193e-05, 1.75063163711175849e-05,
        3.07869136408890425e-04, 1.48649912519561826e-03, 5.12581354822568610e-03, 1.45468377922374024e-02,
        3.58613699833766827e-02, 7.89558955347000463e-02, 1.57863304433804696e-01, 2.89799890796048121e-01,
        4.92257023913990566e-01, 7.78062419148422779e-01, 1.14922046453977811e+00, 1.59130846911780033e+00,
        2.07075997167429149e+00, 2.53704848744469036e+00, 2.93044989562375635e+00, 3.19406458939507099e+00};
    const double L = kVoigtWeidemanL;
    // L - i z = (L + y) - i x;  L + i z = (L - y) + i x
    const double dr = L + y, di = -x;
    const double rd = 1.0 / (dr * dr + di * di);
    const double ir = dr * rd, ii = -di * rd;                 // 1 / (L - i z)
    const double nr = L - y, ni = x;
    const double Zr = nr * ir - ni * ii, Zi = nr * ii + ni * ir;
    double pr = a[0], pi_ = 0.0;
    for (int k = 1; k < kVoigtWeidemanN; ++k) {
        const double t = fma(pr, Zr, fma(-pi_, Zi, a[k]));
        pi_ = fma(pr, Zi, pi_ * Zr);
        pr = t;
    }
    // w = inv (2 p inv + 1 / sqrt(pi)): the real part
    const double tr = fma(2.0, pr * ir - pi_ * ii, kVoigtInvSqrtPi), ti = 2.0 * (pr * ii + pi_ * ir);
    const double k = tr * ir - ti * ii;
    return k < 0.0 ? 0.0 : k;
}

// K and its logarithmic-argument gradients GX = x dK/dx, GY = y dK/dy (K2v-T of lbl_kernels.hip, lbl_voigt_gradient_dev):
// what d/dT of amp K(x(T), y(T)) needs, since d ln x / dT and d ln y / dT are per-line constants.  Same domain and branches as
// voigt_k, and *K is voigt_k(x, y) bit for bit: the same operations in the same order (the tests compare the bits).
//   near      w' = -2 z w + 2 i / sqrt(pi) with w = K + i L:  dK/dx = -2 (x K - y L),  dK/dy = 2 (x L + y K) - 2 / sqrt(pi)
//   mid, far  the asymptotic series itself, differentiated term by term: with q = 1 / z, v = q^2 / 2, c_k = (2 k - 1)!!,
//             w' = -(i / sqrt(pi)) q^2 sum_k c_(k+1) v^k = -(2 i / sqrt(pi)) v D(v);  dK/dx = Re w',  dK/dy = -Im w'.
//             (The closed form loses about 1e-16 s to cancellation there: K ~ y / (sqrt(pi) s) against 2 z w ~ 1.)
//   y == 0    K = exp(-x^2), GX = -2 x^2 K, GY = 0;   x^2 overflowing: all three 0;   NaN in, NaN out;   GX <= 0 always.
// |dGX| / K and |dGY| / K <= 1e-6 wherever K >= 1e-290 (measured per branch: DESIGN.md "K2v-T").
LBL_VOIGT_FN void voigt_kgrad(double x, double y, double* K, double* GX, double* GY) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double two_isp = 2.0 * kVoigtInvSqrtPi;
    if (y == 0.0) {
        const double x2 = x * x;
        if (x2 > 1.7e308) { *K = 0.0; *GX = 0.0; *GY = 0.0; return; }
        const double k = exp(-x * x);
        *K = k;
        *GX = -2.0 * x2 * k;
        *GY = (x != x) ? x : 0.0;
        return;
    }
    const double s = x * x + y * y;
    if (s >= kVoigtMid) {
        if (s > 1.7e308) { *K = 0.0; *GX = 0.0; *GY = 0.0; return; }
        const double r = 1.0 / s;
        const double qr = x * r, qi = -(y * r);
        const double vr = 0.5 * (qr * qr - qi * qi), vi = qr * qi;
        double pr, pi_, dr, di;
        if (s >= kVoigtFar) {
            pr = fma(105.0, vr, 15.0); pi_ = 105.0 * vi;
            double t;
            t = fma(pr, vr, fma(-pi_, vi, 3.0)); pi_ = fma(pr, vi, pi_ * vr); pr = t;
            t = fma(pr, vr, fma(-pi_, vi, 1.0)); pi_ = fma(pr, vi, pi_ * vr); pr = t;
            t = fma(pr, vr, fma(-pi_, vi, 1.0)); pi_ = fma(pr, vi, pi_ * vr); pr = t;
            // D = 1 + v (3 + v (15 + v (105 + 945 v)))
            dr = fma(945.0, vr, 105.0); di = 945.0 * vi;
            t = fma(dr, vr, fma(-di, vi, 15.0)); di = fma(dr, vi, di * vr); dr = t;
            t = fma(dr, vr, fma(-di, vi, 3.0)); di = fma(dr, vi, di * vr); dr = t;
            t = fma(dr, vr, fma(-di, vi, 1.0)); di = fma(dr, vi, di * vr); dr = t;
        } else {
            // (2 k - 1)!! for k = 0 .. 17
            const double c[18] = {1.0, 1.0, 3.0, 15.0, 105.0, 945.0, 10395.0, 135135.0, 2027025.0, 34459425.0, 654729075.0,
                                  13749310575.0, 316234143225.0, 7905853580625.0, 213458046676875.0, 6190283353629375.0,
                                  191898783962510625.0, 6332659870762850625.0};
            pr = c[kVoigtMidTerms]; pi_ = 0.0;
            for (int k = kVoigtMidTerms - 1; k >= 0; --k) {
                const double t = fma(pr, vr, fma(-pi_, vi, c[k]));
                pi_ = fma(pr, vi, pi_ * vr);
                pr = t;
            }
            dr = c[kVoigtMidTerms + 1]; di = 0.0;
            for (int k = kVoigtMidTerms - 1; k >= 0; --k) {
                const double t = fma(dr, vr, fma(-di, vi, c[k + 1]));
                di = fma(dr, vi, di * vr);
                dr = t;
            }
        }
        const double k = -kVoigtInvSqrtPi * fma(qr, pi_, qi * pr);
        *K = k < 0.0 ? 0.0 : k;
        // E = v D;  w' = (2 / sqrt(pi)) (Ei - i Er)
        const double er = fma(vr, dr, -(vi * di)), ei = fma(vr, di, vi * dr);
        const double gx = x * (two_isp * ei);
        *GX = gx > 0.0 ? 0.0 : gx;
        *GY = y * (two_isp * er);
        return;
    }
    const double a[kVoigtWeidemanN] = {
        -3.70074341541718826e-17, 3.90809708090504099e-17, 8.91304535964125145e-17, 4.33646987676311602e-17,
        2.10357809007447985e-17, 7.06831347963979208e-20, 3.85910504816624698e-16, 7.25379754852292609e-16,
        -1.87923282206915558e-15, -5.23915859509534328e-15, 9.52753636075451554e-15, 4.23425555842355866e-14,
        -3.19334159628465632e-14, -3.22775731097254591e-13, -9.65501738984251051e-14, 2.21541877720001645e-12,
        3.42533409044184144e-12, -1.19354512668394108e-11, -4.38658676752703712e-11, 2.16220023479657394e-11,
        3.87942207730320342e-10, 5.77528985547910890e-10, -2.01565992731615496e-09, -9.59625471307884432e-09,
        -6.38680992890150548e-09, 6.92700063602607607e-08, 2.65494920068709391e-07, 1.94943374672414598e-07,
        -1.94456577900989678e-06, -9.47563824045082754e-06, -1.90544616191120193e-05, 1.75063163711175849e-05,
        3.07869136408890425e-04, 1.48649912519561826e-03, 5.12581354822568610e-03, 1.45468377922374024e-02,
        3.58613699833766827e-02, 7.89558955347000463e-02, 1.57863304433804696e-01, 2.89799890796048121e-01,
        4.92257023913990566e-01, 7.78062419148422779e-01, 1.14922046453977811e+00, 1.59130846911780033e+00,
        2.07075997167429149e+00, 2.53704848744469036e+00, 2.93044989562375635e+00, 3.19406458939507099e+00};
    const double L = kVoigtWeidemanL;
    const double dr = L + y, di = -x;
    const double rd = 1.0 / (dr * dr + di * di);
    const double ir = dr * rd, ii = -di * rd;
    const double nr = L - y, ni = x;
    const double Zr = nr * ir - ni * ii, Zi = nr * ii + ni * ir;
    double pr = a[0], pi_ = 0.0;
    for (int k = 1; k < kVoigtWeidemanN; ++k) {
        const double t = fma(pr, Zr, fma(-pi_, Zi, a[k]));
        pi_ = fma(pr, Zi, pi_ * Zr);
        pr = t;
    }
    const double tr = fma(2.0, pr * ir - pi_ * ii, kVoigtInvSqrtPi), ti = 2.0 * (pr * ii + pi_ * ir);
    const double k = tr * ir - ti * ii;
    const double l = tr * ii + ti * ir;                       // Im w
    *K = k < 0.0 ? 0.0 : k;
    const double gx = x * (-2.0 * (x * k - y * l));
    *GX = gx > 0.0 ? 0.0 : gx;
    *GY = y * (2.0 * (x * l + y * k) - two_isp);
}

}  // namespace lbl
