"""The thermal two-stream column of lbl_column_flux_scatter_dev (include/pyrad_hip.h) restated in NumPy and float64, for the
tests: the layer's R and T from twostream_ref.layer, its diffuse absorptance Ab from the header's formula, the layer sources
P and Q of a Planck function linear in optical depth, and the column solved in the OTHER order than the kernels use - adding
from the surface upwards (A, G), then downwards from the top - so that agreement checks the solution and not a transcript.
dense() solves the same level relations as one linear system; sources_scalar evaluates P and Q in the ungrouped form with any
scalar arithmetic (mpmath in the tests)."""
import numpy as np

import twostream_ref as two

H, C, KB = 6.62607004e-34, 299792458.0, 1.38064852E-23
PI = np.pi
D = np.sqrt(3.0)


def planck(nu, T):
    """B(nu, T), W m^-2 sr^-1 per cm^-1 at the wavenumbers nu (cm^-1)"""
    nu = np.asarray(nu, dtype=np.float64)
    with np.errstate(all="ignore"):
        return 2E8 * H * C ** 2 * nu ** 3 / np.expm1(100 * H * C * nu / KB / T)


def absorptance(ta, ts, tsg):
    """The layer's diffuse absorptance 1 - R - T in the header's form, without cancellation (0 where den == 0), and den == 0"""
    ta, ts, tsg = (np.asarray(v, dtype=np.float64) for v in (ta, ts, tsg))
    with np.errstate(all="ignore"):
        t = ta + ts
        Da, Db = D * (ta / t), D * ((t - tsg) / t)
        g1, g2 = (Db + Da) / 2, (Db - Da) / 2
        lam = np.sqrt(Da * Db)
        E = np.exp(-(lam * t))
        Gam = g2 / (g1 + lam)
        oG = ((Da + lam) * (Db + lam)) / ((g1 + lam) * (g1 + lam))
        den = oG + (Gam * Gam) * -np.expm1(-2 * (lam * t))
        cons = den == 0
        Ab = np.where(cons, 0, ((-np.expm1(-(lam * t)) * ((Da + lam) / (g1 + lam))) * (1 - Gam * E)) / np.where(cons, 1.0, den))
    return Ab, cons


def sources(ta, ts, tsg, Bt, Bb):
    """One layer at n points with pi B = Bt at its top edge and Bb at its bottom edge: R, T, Ab, and what it emits upward at
    its top, P, and downward at its bottom, Q"""
    ta, ts, tsg, Bt, Bb = (np.asarray(v, dtype=np.float64) for v in (ta, ts, tsg, Bt, Bb))
    R, T = two.layer(ta, ts, tsg, [1.0])[:2]
    Ab, cons = absorptance(ta, ts, tsg)
    with np.errstate(all="ignore"):
        t = ta + ts
        d = Bb - Bt
        h = (Ab + 2 * R) / (D * (t - tsg)) - T
        P, Q = Bt * Ab + d * h, Bb * Ab - d * h
    dark = (t == 0) | cons | (ta == 0)
    return R, T, Ab, np.where(dark, 0.0, P), np.where(dark, 0.0, Q)


def sources_scalar(ta, ts, tsg, Bt, Bb, num, sqrt, exp, expm1):
    """P and Q of one layer in the arithmetic of ``num``, in the ungrouped form: the particular solution pi B(tau) +- c with
    the homogeneous response subtracted.  The caller keeps away from t == 0 and ta == 0."""
    R, T = two.layer_scalar(ta, ts, tsg, 1.0, num, sqrt, exp, expm1)[:2]
    ta, ts, tsg, Bt, Bb = num(ta), num(ts), num(tsg), num(Bt), num(Bb)
    t = ta + ts
    c = (Bb - Bt) / (sqrt(num(3)) * (t - tsg))
    return (Bt + c) - R * (Bt - c) - T * (Bb + c), (Bb - c) - R * (Bb + c) - T * (Bt - c)


def solve(R, T, P, Q, e, Es, dn_top):
    """The column from its layers' R, T, P, Q (L, n): the stack below level l answers up_l = A_l dn_l + G_l, built from the
    surface (A_0 = 1 - e, G_0 = e Es) upwards; then dn from dn_L = dn_top downwards.  Returns up, dn (L + 1, n)."""
    R, T, P, Q = (np.asarray(v, dtype=np.float64) for v in (R, T, P, Q))
    L, n = R.shape
    e = np.broadcast_to(np.asarray(e, dtype=np.float64), (n,))
    A, G = np.empty((L + 1, n)), np.empty((L + 1, n))
    with np.errstate(all="ignore"):
        A[0], G[0] = 1 - e, e * np.broadcast_to(Es, (n,))
        for l in range(L):
            c = 1 - A[l] * R[l]
            A[l + 1] = R[l] + T[l] * T[l] * A[l] / c
            G[l + 1] = P[l] + T[l] * (G[l] + A[l] * Q[l]) / c
        up, dn = np.empty((L + 1, n)), np.empty((L + 1, n))
        dn[L] = np.broadcast_to(dn_top, (n,))
        up[L] = A[L] * dn[L] + G[L]
        for l in range(L - 1, -1, -1):
            dn[l] = (T[l] * dn[l + 1] + Q[l] + R[l] * G[l]) / (1 - A[l] * R[l])
            up[l] = A[l] * dn[l] + G[l]
    return up, dn


def column(k, depth, nu, T_edge, amount=(), numbers=(), delta=1, emissivity=1.0, I_surface=None, surface_T=None, I_top=None):
    """The column at the n wavenumbers nu: k (L, n), depth (L,), T_edge (L, 2) the bottom and top edge temperature of every
    layer (equal: the isothermal layer), amount (C, L), numbers C triples (ext, ssa, g), emissivity a number or (n,), the
    surface's radiance I_surface (n,) or B(nu, surface_T), the radiance I_top (n,) coming down at the top or None.
    Returns up, dn, each (L + 1, n).  A point with a t that is not finite is NaN at every level."""
    k = np.asarray(k, dtype=np.float64).reshape(len(depth), -1)
    L, n = k.shape
    T_edge = np.asarray(T_edge, dtype=np.float64).reshape(L, 2)
    ta, ts, tsg = two.optical(k, depth, amount, numbers, delta)
    R, T, P, Q = (np.empty((L, n)) for _ in range(4))
    for l in range(L):
        R[l], T[l], _, P[l], Q[l] = sources(ta[l], ts[l], tsg[l], PI * planck(nu, T_edge[l, 1]), PI * planck(nu, T_edge[l, 0]))
    Es = PI * (np.asarray(I_surface, dtype=np.float64) if I_surface is not None else planck(nu, surface_T))
    up, dn = solve(R, T, P, Q, emissivity, Es, 0.0 if I_top is None else PI * np.asarray(I_top, dtype=np.float64))
    bad = ~np.all(np.isfinite(ta + ts), axis=0)
    up[:, bad], dn[:, bad] = np.nan, np.nan
    return up, dn


def scale(nu, T_edge, I_surface=None, surface_T=None, I_top=None):
    """pi times the largest of the Planck values and boundary radiances that enter a point: the unit of the tolerances (n,)"""
    s = np.zeros(len(nu))
    for T in np.unique(np.asarray(T_edge, dtype=np.float64)):
        s = np.maximum(s, planck(nu, T))
    s = np.maximum(s, np.abs(I_surface) if I_surface is not None else planck(nu, surface_T))
    if I_top is not None:
        s = np.maximum(s, np.abs(I_top))
    return PI * s


def dense(R, T, P, Q, e, Es, dn_top):
    """The layer relations of ONE point as a dense linear system (numpy.linalg.solve), the emitting surface and dn_L in the
    system: R, T, P, Q (L,) -> up, dn (L + 1,)"""
    L = len(R)
    N = 2 * (L + 1)                 # unknowns up_0 .. up_L, dn_0 .. dn_L
    M, rhs = np.zeros((N, N)), np.zeros(N)
    M[0, 0], M[0, L + 1], rhs[0] = 1.0, -(1 - e), e * Es         # up_0 - (1 - e) dn_0 = e Es
    for l in range(L):
        r = 1 + l                   # up_(l+1) - T up_l - R dn_(l+1) = P
        M[r, l + 1], M[r, l], M[r, L + 1 + l + 1], rhs[r] = 1.0, -T[l], -R[l], P[l]
        r = 1 + L + l               # dn_l - T dn_(l+1) - R up_l = Q
        M[r, L + 1 + l] = 1.0
        M[r, L + 1 + l + 1] -= T[l]
        M[r, l] -= R[l]
        rhs[r] = Q[l]
    M[N - 1, N - 1], rhs[N - 1] = 1.0, dn_top
    sol = np.linalg.solve(M, rhs)
    return sol[:L + 1], sol[L + 1:]


band_sums = two.band_sums
