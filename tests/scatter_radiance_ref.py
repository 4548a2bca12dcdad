"""The radiances of lbl_column_radiance_scatter_dev (include/pyrad_hip.h) restated in NumPy and float64, for the tests, on
scatter_flux_ref.column's level fluxes (which solves the column in the other order than the kernels).  Inside a layer the
fluxes' sum and difference come from the four fluxes at its two edges (the sinh-ratio basis, the linear interpolation at
lam == 0); the grouping is this file's own: the two weights W0 and W1 of the edge values are each evaluated on their own
(the kernel forms their sum and W1), the source is a Bs + (w / 2) [(1 +- D g mu) F+ + (1 -+ D g mu) F-] with F+ and F-
themselves interpolated (the kernel works with their departures from the Planck function), and a down view is integrated
layer by layer from the top (the kernel accumulates from the surface).  layer_scalar and source_scalar state the
definition - the ODE's solution by its two exponential modes from the two fluxes that enter the layer, and S+- on it - with
any scalar arithmetic (mpmath in the tests, which integrate S+- by quadrature)."""
import numpy as np

import scatter_flux_ref as flux
import twostream_ref as two

PI = np.pi
D = np.sqrt(3.0)


def weights(u, tau, lm):
    """The integrals over s in [0, t] against exp(-s / mu) ds / mu of 1, sinh(lam (t - s)) / sinh(lam t) and
    sinh(lam s) / sinh(lam t), and of what the two leave of 1: W, W0, W1, Wh, from u = lam t, tau = t / mu and lm = lam mu
    (arrays).  Each of W0 and W1 is a second divided difference of exp divided by the largest node distance, tau + u: good
    to an absolute rounding error."""
    u, tau, lm = (np.asarray(v, dtype=np.float64) for v in (u, tau, lm))
    with np.errstate(all="ignore"):
        Tv, E = np.exp(-tau), np.exp(-u)
        x = (1 - lm) * tau
        ax = np.abs(x)
        # (E - Tv) / (tau - u), smooth through x == 0, no positive argument
        small = ax == 0
        A1t = np.where(x >= 0, E, Tv) * np.where(small, 1.0, -np.expm1(-ax) / np.where(small, 1.0, ax))
        big = u > 350
        us = np.where(big, 1.0, u)
        ush = np.where(u == 0, 1.0, us / np.where(u == 0, 1.0, np.sinh(us)))      # u / sinh u
        r0 = np.where(big, 0.0, ush)                                              # (u / sinh u) (A1t <= E: the product is 0)
        r1 = np.where(big, 2 * u, ush * np.exp(us))                               # (u / sinh u) exp(u)
        prod1 = np.where(A1t == 0, 0.0, r1 * A1t)
        W0 = (1 - r0 * A1t) / (1 + lm)
        W1 = (prod1 - Tv) / (1 + lm)
        # the weight of 1 - r0 - r1 >= 0, which multiplies c = d / (D (t - tsg)), as large as 1 / t: W less the weight of
        # r0 + r1 = cosh(lam (s - t / 2)) / cosh(lam t / 2), a sum of positive terms, so that a thin layer's is good to a
        # rounding error of tau and not of 1
        both = (tau * A1t + -np.expm1(-(tau + u)) / (1 + lm)) / (1 + E)
        Wh = -np.expm1(-tau) - both
    return -np.expm1(-tau), W0, W1, Wh


def g_linear(tau):
    """g(tau) = 1 - (1 - exp(-tau)) / tau of the linear source, by its series below 0.25"""
    tau = np.asarray(tau, dtype=np.float64)
    with np.errstate(all="ignore"):
        direct = 1 - -np.expm1(-tau) / tau
        s = np.zeros_like(tau)
        for n in range(14, 1, -1):
            s = 1.0 / float(np.prod(np.arange(1, n + 1, dtype=np.float64))) - tau * s
    return np.where(tau >= 0.25, direct, tau * s)


def radiance(k, depth, nu, T_edge, views, amount=(), numbers=(), delta=1, emissivity=1.0, I_surface=None, surface_T=None,
             I_top=None):
    """The radiances at the n wavenumbers nu for ``views``, pairs (mu, down): (V, n); and the level fluxes up, dn they rest
    on.  The column's arguments are scatter_flux_ref.column's."""
    L, n = len(depth), len(nu)
    k = np.asarray(k, dtype=np.float64).reshape(L, n)
    T_edge = np.asarray(T_edge, dtype=np.float64).reshape(L, 2)
    if L == 0:              # the sky comes down unchanged; the surface emits and sends the rest of it back
        Es = PI * (np.asarray(I_surface, dtype=np.float64) if I_surface is not None else flux.planck(nu, surface_T))
        dn = (PI * np.asarray(I_top, dtype=np.float64) if I_top is not None else np.zeros(n))[None, :]
        up = (emissivity * Es + (1 - np.asarray(emissivity, dtype=np.float64)) * dn[0])[None, :]
    else:
        up, dn = flux.column(k, depth, nu, T_edge, amount, numbers, delta, emissivity, I_surface, surface_T, I_top)
    ta, ts, tsg = two.optical(k, depth, amount, numbers, delta)
    out = np.empty((len(views), n))
    top = np.zeros(n) if I_top is None else np.asarray(I_top, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = ta + ts
        safe = np.where(t == 0, 1.0, t)
        a, b, w = ta / safe, (t - tsg) / safe, ts / safe
        g = np.where(ts == 0, 0.0, tsg / np.where(ts == 0, 1.0, ts))
        lam = np.sqrt((D * a) * (D * b))
        for v, (mu, down) in enumerate(views):
            I = top.copy() if down else up[0] / PI
            for l in (range(L - 1, -1, -1) if down else range(L)):
                Bt, Bb = PI * flux.planck(nu, T_edge[l, 1]), PI * flux.planck(nu, T_edge[l, 0])
                tau = t[l] / mu
                W, W0, W1, Wh = weights(lam[l] * t[l], tau, lam[l] * mu)
                c = np.where(ta[l] == 0, 0.0, (Bb - Bt) / (D * np.where(ta[l] == 0, 1.0, t[l] - tsg[l])))
                G = W - g_linear(tau)                   # the weight of s / t
                # F+ and F- through the layer: top-edge and bottom-edge values, and the particular part +- c
                Fp0, Fpt, Fm0, Fmt = up[l + 1], up[l], dn[l + 1], dn[l]
                if down:                                # s -> t - s: the edges exchange their weights
                    iFp = Fp0 * W1 + Fpt * W0 + c * Wh
                    iFm = Fm0 * W1 + Fmt * W0 - c * Wh
                    iB = Bb * (W - G) + Bt * G
                    iBh = iB - (Bt * W1 + Bb * W0)
                    sg = -1.0
                else:
                    iFp = Fp0 * W0 + Fpt * W1 + c * Wh
                    iFm = Fm0 * W0 + Fmt * W1 - c * Wh
                    iB = Bt * (W - G) + Bb * G
                    iBh = iB - (Bt * W0 + Bb * W1)
                    sg = 1.0
                # F = (interpolated F - interpolated Bs) + Bs: Bs's own integral is exact, its interpolation is not Bs
                iFp, iFm = iFp + iBh, iFm + iBh
                J = a[l] * iB + (w[l] / 2) * ((1 + sg * D * g[l] * mu) * iFp + (1 - sg * D * g[l] * mu) * iFm)
                I = np.where(t[l] == 0, I, I * np.exp(-tau) + J / PI)
            out[v] = I
    bad = ~np.all(np.isfinite(t), axis=0)
    out[:, bad] = np.nan
    return out, up, dn


def layer_scalar(ta, ts, tsg, Bt, Bb, up_b, dn_t, num, sqrt, exp, expm1):
    """One layer in the arithmetic of ``num``: the ODE's solution from the two fluxes that enter it (F+(t) = up_b at the
    bottom, F-(0) = dn_t at the top) as a function (s, t - s) -> (F+, F-), with t, a, w, g, lam.  The two exponential modes
    (Gam, 1) exp(-lam s) and (1, Gam) exp(-lam (t - s)) on the particular solution Bs +- c; the conservative layer
    (lam == 0) by its linear solution."""
    ta, ts, tsg, Bt, Bb, up_b, dn_t = (num(v) for v in (ta, ts, tsg, Bt, Bb, up_b, dn_t))
    t = ta + ts
    Dn = sqrt(num(3))
    a, b, w = ta / t, (t - tsg) / t, ts / t
    g = tsg / ts if ts != 0 else num(0)
    Da, Db = Dn * a, Dn * b
    g1, g2 = (Db + Da) / 2, (Db - Da) / 2
    lam = sqrt(Da * Db)
    if Da == 0:
        # dDelta/ds = 0, dSigma/ds = Db Delta: F- (0) = dn_t, F+(t) = up_b
        # F+ = F- + Delta, F-(s) = dn_t + (Db / 2) Delta s  (from Sigma' = Db Delta), F+(t) = dn_t + (Db t / 2 + 1) Delta
        Delta = (up_b - dn_t) / (1 + Db * t / 2)
        return (lambda s, r: (dn_t + Db * Delta * s / 2 + Delta, dn_t + Db * Delta * s / 2)), t, a, w, g, lam
    c = (Bb - Bt) / (Db * t)
    Gam = g2 / (g1 + lam)
    E = exp(-lam * t)
    x, y = dn_t - (Bt - c), up_b - (Bb + c)
    det = 1 - Gam * Gam * E * E
    al, be = (x - Gam * E * y) / det, (y - Gam * E * x) / det

    def F(s, r):
        Bs = Bt + (Bb - Bt) * s / t if s <= r else Bb - (Bb - Bt) * r / t
        e0, e1 = exp(-lam * s), exp(-lam * r)
        return Bs + c + al * Gam * e0 + be * e1, Bs - c + al * e0 + be * Gam * e1
    return F, t, a, w, g, lam


def source_scalar(F, t, a, w, g, Bt, Bb, mu, down, num, sqrt):
    """(s, t - s) -> pi S+-(s, mu) of the definition (both distances: of t = 1e300 no digits are left for t - s)"""
    Dn = sqrt(num(3))
    Bt, Bb, mu = num(Bt), num(Bb), num(mu)
    sg = -1 if down else 1

    def S(s, r):
        Fp, Fm = F(s, r)
        Bs = Bt + (Bb - Bt) * s / t if s <= r else Bb - (Bb - Bt) * r / t
        return a * Bs + (w / 2) * ((1 + sg * Dn * g * mu) * Fp + (1 - sg * Dn * g * mu) * Fm)
    return S
