#!/usr/bin/env python3
"""Prints the constants of the near branch of voigt_k (pyrad_amd/csrc/lbl_voigt_func.h): Weideman's rational approximation of
the Faddeeva function, w(z) = 2 p(Z) / (L - i z)^2 + (1 / sqrt(pi)) / (L - i z), Z = (L + i z) / (L - i z), with N = 48 terms
(J. A. C. Weideman, Computation of the complex error function, SIAM J. Numer. Anal. 31 (1994) 1497-1518).  The polynomial's
coefficients are Fourier coefficients of exp(-t^2) (L^2 + t^2) on t = L tan(theta / 2), highest power first."""
import numpy as np

N = 48
M = 2 * N
L = np.sqrt(N / np.sqrt(2.0))
k = np.arange(-M + 1, M)
t = L * np.tan(k * np.pi / M / 2)
f = np.concatenate([[0.0], np.exp(-t * t) * (L * L + t * t)])
a = np.real(np.fft.fft(np.fft.fftshift(f))) / (2 * M)
a = a[1:N + 1][::-1]
print("L = %r" % float(L))
for i in range(0, N, 4):
    print("        " + " ".join("%.17e," % v for v in a[i:i + 4]))
