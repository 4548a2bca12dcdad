"""The radiances of lbl_column_beam_radiance_dev (include/pyrad_hip.h) restated in NumPy and float64, for the tests, on
twostream_ref.column's level fluxes (which solves the column in the other order than the kernels).  The grouping is this
file's own: inside a layer F+ and F- THEMSELVES are interpolated between their edge values by the sinh-ratio basis
(scatter_radiance_ref.weights: W0 and W1 each on their own), and what the beam's particular part Cp, Cm Fd exp(-s / m)
departs from its own interpolation is added - the kernel interpolates the homogeneous parts and gathers the beam's terms in
one bracket; the beam exponential's integrals are written from the integrals' own form (tau (e1 - e2) / (x2 - x1)); and a
down view is integrated layer by layer from the top (the kernel accumulates from the surface).  layer_scalar and
source_scalar state the definition - the ODE's solution by its two exponential modes on the beam's particular solution from
the two fluxes that enter the layer, and S+- on it - with any scalar arithmetic (mpmath in the tests, which integrate S+- by
quadrature)."""
import numpy as np

import scatter_radiance_ref as thermal
import twostream_ref as two

PI = np.pi
D = np.sqrt(3.0)
MOVED = 1.0 - two.NUDGE         # lam m where the particular solution's pole moves m to


def layer_numbers(ta, ts, tsg):
    """t, w, g, D a, g1, g2, lam of the header from the three depths (arrays); t == 0 gives w = lam = 0"""
    with np.errstate(all="ignore"):
        t = ta + ts
        safe = np.where(t == 0, 1.0, t)
        a, b, w = ta / safe, (t - tsg) / safe, ts / safe
        g = np.where(ts == 0, 0.0, tsg / np.where(ts == 0, 1.0, ts))
        Da, Db = D * a, D * b
        return t, w, g, Da, (Db + Da) / 2, (Db - Da) / 2, np.sqrt(Da * Db)


def moved(k, depth, slant, amount=(), numbers=(), delta=1):
    """(L, n): where the float64 arithmetic moves m off the pole, and |1 - lam m| there"""
    k = np.asarray(k, dtype=np.float64).reshape(len(depth), -1)
    t, w, g, Da, g1, g2, lam = layer_numbers(*two.optical(k, depth, amount, numbers, delta))
    slant = np.asarray(slant, dtype=np.float64)[:, None]
    return beam_terms(t, w, g, Da, g1, g2, lam, slant)[5], np.abs(1 - lam * (1.0 / slant))


def beam_terms(t, w, g, Da, g1, g2, lam, slant):
    """K5l's terms of one beam in one layer at n points, as the header writes them: m (moved at the pole), t / m, Tdm, Cp,
    Cm, and where m was moved"""
    with np.errstate(all="ignore"):
        m = np.broadcast_to(1.0 / slant, t.shape)
        g3 = (1 - (D * g) * m) / 2
        g4 = 1 - g3
        a2 = g1 * g3 + g2 * g4
        moved = np.abs(1 - lam * m) < two.NUDGE
        m = np.where(moved, MOVED / np.where(moved, lam, 1.0), m)
        tm = np.where(moved, t / m, t * slant)
        d = (1 - lam * m) * (1 + lam * m)
        Cp = (w * (g3 - a2 * m)) / d
        u = (w * (1 + (Da * (g4 - g3)) * m)) / d
    return m, tm, np.exp(-tm), Cp, Cp - u, moved


def beam_integrals(tau, tm, t, mu, m):
    """exp(-s / m) against exp(-s / mu) ds / mu and against exp(-(t - s) / mu) ds / mu over [0, t]: Xu, Xd"""
    with np.errstate(all="ignore"):
        Xu = -np.expm1(-(tau + tm)) * (m / (m + mu))
        dx = np.abs(t * ((mu - m) / (mu * m)))              # |t / m - t / mu|
        dx = np.where(np.isfinite(dx), dx, np.inf)
        phi = np.where(dx == 0, 1.0, -np.expm1(-dx) / np.where(dx == 0, 1.0, dx))
        Xd = np.exp(-np.minimum(tm, tau)) * np.where(phi == 0, 0.0, tau * phi)
    return Xu, Xd


def radiance(k, depth, S0, beam_weight, slant, views, amount=(), numbers=(), delta=1, emissivity=1.0):
    """The radiances at n points for ``views``, pairs (mu, down): (V, n); the level fluxes up, dn (diffuse), direct they
    rest on; and the smallest |1 - lam m| of every point.  One beam: ``beam_weight`` a number, ``slant`` (L,); the column's
    other arguments are twostream_ref.column's."""
    L = len(depth)
    S0 = np.asarray(S0, dtype=np.float64)
    n = len(S0)
    k = np.asarray(k, dtype=np.float64).reshape(L, n)
    slant = np.asarray(slant, dtype=np.float64).reshape(L)
    if L == 0:                  # the beam reaches the surface unchanged; nothing comes down diffusely
        direct = (beam_weight * S0)[None, :]
        dn = np.zeros((1, n))
        up = ((1 - np.asarray(emissivity, dtype=np.float64)) * direct[0])[None, :]
        pole = np.full(n, np.inf)
    else:
        up, dn, direct, pole = two.column(k, depth, S0, [beam_weight], slant[None, :], amount, numbers, delta, emissivity)
    ta, ts, tsg = two.optical(k, depth, amount, numbers, delta)
    out = np.empty((len(views), n))
    t, w, g, Da, g1, g2, lam = layer_numbers(ta, ts, tsg)
    with np.errstate(all="ignore"):
        for v, (mu, down) in enumerate(views):
            I = np.zeros(n) if down else up[0] / PI
            for l in (range(L - 1, -1, -1) if down else range(L)):
                m, tm, Tdm, Cp, Cm, _ = beam_terms(t[l], w[l], g[l], Da[l], g1[l], g2[l], lam[l], slant[l])
                tau = t[l] / mu
                W, W0, W1, Wh = thermal.weights(lam[l] * t[l], tau, lam[l] * mu)
                Xu, Xd = beam_integrals(tau, tm, t[l], mu, m)
                Fd = direct[l + 1]
                Fp0, Fpt, Fm0, Fmt = up[l + 1], up[l], dn[l + 1], dn[l]
                if down:                                # s -> t - s: the edges exchange their weights
                    X, sg = Xd, -1.0
                    own = W1 + Tdm * W0                 # the beam exponential's own interpolation, integrated
                    iFp, iFm = Fp0 * W1 + Fpt * W0, Fm0 * W1 + Fmt * W0
                else:
                    X, sg = Xu, 1.0
                    own = W0 + Tdm * W1
                    iFp, iFm = Fp0 * W0 + Fpt * W1, Fm0 * W0 + Fmt * W1
                iFp, iFm = iFp + (Cp * Fd) * (X - own), iFm + (Cm * Fd) * (X - own)
                J = ((w[l] / 2) * ((1 + sg * D * g[l] * mu) * iFp + (1 - sg * D * g[l] * mu) * iFm)
                     + (w[l] / (2 * D * m)) * (1 - sg * 3 * g[l] * mu * m) * (Fd * X))
                I = np.where(t[l] == 0, I, I * np.exp(-tau) + J / PI)
            out[v] = I
    bad = ~np.all(np.isfinite(t), axis=0)
    out[:, bad] = np.nan
    return out, up, dn, direct, pole


def layer_scalar(ta, ts, tsg, slant, moved, Fd, up_b, dn_t, num, sqrt, exp):
    """One layer in the arithmetic of ``num``: the beam's terms (m moved to (1 - 1e-6) / lam where ``moved`` says so - the
    float64 decision, taken as data; g3, g4 and a2 keep the unmoved m) and the ODE's solution from the two fluxes that enter
    it (F+(t) = up_b at the bottom, F-(0) = dn_t at the top) as a function (s, t - s) -> (F+, F-, beam) with
    beam = Fd exp(-s / m); with t, w, g, m, Cp, Cm, Tdm.  The two exponential modes (Gam, 1) exp(-lam s) and
    (1, Gam) exp(-lam (t - s)) on the particular solution (Cp, Cm) beam; the conservative layer (lam == 0) by its linear
    solution."""
    ta, ts, tsg, slant, Fd, up_b, dn_t = (num(v) for v in (ta, ts, tsg, slant, Fd, up_b, dn_t))
    t = ta + ts
    Dn = sqrt(num(3))
    a, b, w = ta / t, (t - tsg) / t, ts / t
    g = tsg / ts if ts != 0 else num(0)
    Da, Db = Dn * a, Dn * b
    g1, g2 = (Db + Da) / 2, (Db - Da) / 2
    lam = sqrt(Da * Db)
    m = 1 / slant
    g3 = (1 - Dn * g * m) / 2
    g4 = 1 - g3
    a1, a2 = g1 * g4 + g2 * g3, g1 * g3 + g2 * g4
    if moved:
        m = num(MOVED) / lam
    d = (1 - lam * m) * (1 + lam * m)
    Cp = w * (g3 - a2 * m) / d
    Cm = -w * (g4 + a1 * m) / d
    Tdm = exp(-t / m)
    x, y = dn_t - Cm * Fd, up_b - Cp * Fd * Tdm         # what the homogeneous part has to bring in
    if Da == 0:
        # Delta' = 0, F-' = (Db / 2) Delta: F-_h(0) = x, F+_h(t) = x + (Db t / 2 + 1) Delta
        Delta = (y - x) / (1 + Db * t / 2)

        def F(s, r):
            beam = Fd * exp(-s / m)
            return x + Db * Delta * s / 2 + Delta + Cp * beam, x + Db * Delta * s / 2 + Cm * beam, beam
        return F, t, w, g, m, Cp, Cm, Tdm
    Gam = g2 / (g1 + lam)
    E = exp(-lam * t)
    det = 1 - Gam * Gam * E * E
    al, be = (x - Gam * E * y) / det, (y - Gam * E * x) / det

    def F(s, r):
        e0, e1 = exp(-lam * s), exp(-lam * r)
        beam = Fd * exp(-s / m)
        return Cp * beam + al * Gam * e0 + be * e1, Cm * beam + al * e0 + be * Gam * e1, beam
    return F, t, w, g, m, Cp, Cm, Tdm


def source_scalar(F, w, g, m, mu, down, num, sqrt):
    """(s, t - s) -> pi S+-(s, mu) of the definition"""
    Dn = sqrt(num(3))
    mu = num(mu)
    sg = -1 if down else 1

    def S(s, r):
        Fp, Fm, beam = F(s, r)
        return ((w / 2) * ((1 + sg * Dn * g * mu) * Fp + (1 - sg * Dn * g * mu) * Fm)
                + (w / (2 * Dn * m)) * (1 - sg * 3 * g * mu * m) * beam)
    return S
