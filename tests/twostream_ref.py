"""The two-stream column of lbl_column_twostream_dev (include/pyrad_hip.h) restated in NumPy, for the tests: the layer
solution as the header writes it, and the column solved in the OTHER order than the kernels use - the direct beams first,
then adding from the surface upwards (A, G), then downwards - so that agreement checks the solution and not a transcript.
Every function takes a ``dtype`` (np.float64, or np.longdouble for the points near the particular solution's pole);
layer_scalar evaluates the same layer formulas with any scalar arithmetic (mpmath in the tests)."""
import numpy as np

NUDGE = 1e-6


def scatterer_numbers(ext, ssa, g, delta, dtype=np.float64):
    """alpha, sigma, eta of one scatterer from its extinction, albedo and asymmetry (numbers or arrays)"""
    ext, ssa, g = (np.asarray(v, dtype=dtype) for v in (ext, ssa, g))
    f = g * g if delta else np.zeros_like(g)
    return ext * (1 - ssa), (ext * ssa) * (1 - f), (ext * ssa) * (g - f)


def layer(ta, ts, tsg, slant, dtype=np.float64):
    """One layer at n points: ta, ts, tsg (n,), slant (S,) -> R, T (n,), Td, Rb, Tb (S, n) and pole = |1 - lam m| (S, n)"""
    ta, ts, tsg = (np.asarray(v, dtype=dtype) for v in (ta, ts, tsg))
    slant = np.asarray(slant, dtype=dtype)
    D = np.sqrt(dtype(3))
    one = dtype(1)
    with np.errstate(all="ignore"):
        t = ta + ts
        empty = t == 0
        a, b, w = ta / t, (t - tsg) / t, ts / t
        g = np.where(ts == 0, 0, tsg / np.where(ts == 0, one, ts))
        Da, Db = D * a, D * b
        g1, g2 = (Db + Da) / 2, (Db - Da) / 2
        lam = np.sqrt(Da * Db)
        E = np.exp(-(lam * t))
        Gam = g2 / (g1 + lam)
        oG = ((Da + lam) * (Db + lam)) / ((g1 + lam) * (g1 + lam))
        oE = -np.expm1(-2 * (lam * t))
        den = oG + (Gam * Gam) * oE
        cons = den == 0
        safe = np.where(cons, one, den)
        R = np.where(cons, g1 * t / (1 + g1 * t), (Gam * oE) / safe)
        T = np.where(cons, 1 / (1 + g1 * t), (E * oG) / safe)
        R, T = np.where(empty, 0, R), np.where(empty, 1, T)
        Ab = np.where(cons, 0, ((-np.expm1(-(lam * t)) * ((Da + lam) / (g1 + lam))) * (1 - Gam * E)) / safe)
        S = len(slant)
        Td, Rb, Tb, pole = (np.empty((S,) + t.shape, dtype=dtype) for _ in range(4))
        for s in range(S):
            m = np.broadcast_to(one / slant[s], t.shape)
            Td[s] = np.exp(-(t * slant[s]))
            g3 = (1 - (D * g) * m) / 2
            g4 = 1 - g3
            a2 = g1 * g3 + g2 * g4
            pole[s] = np.abs(1 - lam * m)
            near = pole[s] < NUDGE
            m = np.where(near, (1 - dtype(NUDGE)) / np.where(near, lam, one), m)
            Tdm = np.where(near, np.exp(-(t / m)), Td[s])
            d = (1 - lam * m) * (1 + lam * m)
            Cp = (w * (g3 - a2 * m)) / d
            u = (w * (1 + (Da * (g4 - g3)) * m)) / d
            Y = (Cp * T) * (1 - Tdm)
            Rb[s] = np.where(empty, 0, Y + (R * u + Cp * Ab))
            Tb[s] = np.where(empty, 0, (u * (T - Tdm) + (Cp * Tdm) * Ab) - Y)
    return R, T, Td, Rb, Tb, pole


def layer_scalar(ta, ts, tsg, slant, num, sqrt, exp, expm1):
    """The layer formulas for one point and one beam in the arithmetic of ``num`` (a constructor) and the three functions:
    (R, T, Td, Rb, Tb), with Rb and Tb in the ungrouped form Cp - R Cm - T Cp Td, Cm Td - T Cm - R Cp Td that the header
    derives its own from.  No nudge: the caller keeps away from the pole."""
    ta, ts, tsg, slant = num(ta), num(ts), num(tsg), num(slant)
    t = ta + ts
    if t == 0:
        return num(0), num(1), num(1), num(0), num(0)
    D = sqrt(num(3))
    a, b, w = ta / t, (t - tsg) / t, ts / t
    g = tsg / ts if ts != 0 else num(0)
    Da, Db = D * a, D * b
    g1, g2 = (Db + Da) / 2, (Db - Da) / 2
    lam = sqrt(Da * Db)
    E = exp(-lam * t)
    Gam = g2 / (g1 + lam)
    oG = (Da + lam) * (Db + lam) / (g1 + lam) ** 2
    oE = -expm1(-2 * lam * t)
    den = oG + Gam * Gam * oE
    if den == 0:
        R, T = g1 * t / (1 + g1 * t), 1 / (1 + g1 * t)
    else:
        R, T = Gam * oE / den, E * oG / den
    m = 1 / slant
    Td = exp(-t * slant)
    g3 = (1 - D * g * m) / 2
    g4 = 1 - g3
    a1, a2 = g1 * g4 + g2 * g3, g1 * g3 + g2 * g4
    d = (1 - lam * m) * (1 + lam * m)
    Cp = w * (g3 - a2 * m) / d
    Cm = -w * (g4 + a1 * m) / d
    return R, T, Td, Cp - R * Cm - T * Cp * Td, Cm * Td - T * Cm - R * Cp * Td


def optical(k, depth, amount, numbers, delta, dtype=np.float64):
    """ta, ts, tsg (L, n) from k (L, n), depth (L,), amount (C, L) and per scatterer (ext, ssa, g)"""
    k = np.asarray(k, dtype=dtype)
    L, n = k.shape
    ta = k * np.asarray(depth, dtype=dtype)[:, None]
    ts, tsg = np.zeros((L, n), dtype=dtype), np.zeros((L, n), dtype=dtype)
    for c, (ext, ssa, g) in enumerate(numbers):
        al, si, et = scatterer_numbers(ext, ssa, g, delta, dtype)
        am = np.asarray(amount[c], dtype=dtype)[:, None]
        with np.errstate(all="ignore"):
            ta, ts, tsg = ta + am * al, ts + am * si, tsg + am * et
    return ta, ts, tsg


def column(k, depth, S0, beam_weight, slant, amount=(), numbers=(), delta=1, emissivity=1.0, dtype=np.float64):
    """The column at n points: k (L, n), depth (L,), S0 (n,), beam_weight (S,), slant (S, L), amount (C, L), numbers C
    triples (ext, ssa, g), emissivity a number or (n,).  Returns up, dn (diffuse), direct, each (L + 1, n), and the smallest
    |1 - lam m| of every point over its layers and beams (n,; inf without layers)."""
    k = np.asarray(k, dtype=dtype).reshape(len(depth), -1)
    L, n = k.shape
    S0 = np.asarray(S0, dtype=dtype)
    bw = np.asarray(beam_weight, dtype=dtype)
    slant = np.asarray(slant, dtype=dtype).reshape(len(bw), L)
    e = np.asarray(emissivity, dtype=dtype)
    ta, ts, tsg = optical(k, depth, amount, numbers, delta, dtype)
    R, T = np.empty((L, n), dtype=dtype), np.empty((L, n), dtype=dtype)
    P, Q = np.zeros((L, n), dtype=dtype), np.zeros((L, n), dtype=dtype)
    Sb = np.empty((len(bw), L + 1, n), dtype=dtype)
    Sb[:, L] = S0
    pole = np.full(n, np.inf)
    with np.errstate(all="ignore"):
        for l in range(L - 1, -1, -1):
            R[l], T[l], Td, Rb, Tb, pl = layer(ta[l], ts[l], tsg[l], slant[:, l], dtype)
            pole = np.minimum(pole, pl.min(axis=0).astype(np.float64))
            for s in range(len(bw)):
                Fd = bw[s] * Sb[s, l + 1]
                P[l] += Rb[s] * Fd
                Q[l] += Tb[s] * Fd
                Sb[s, l] = Td[s] * Sb[s, l + 1]
        direct = np.einsum("s,sin->in", bw, Sb) if len(bw) > 1 else bw[0] * Sb[0]
        A, G = np.empty((L + 1, n), dtype=dtype), np.empty((L + 1, n), dtype=dtype)
        A[0] = (1 - e) * np.ones(n, dtype=dtype)
        G[0] = (1 - e) * direct[0]
        for l in range(L):
            c = 1 - A[l] * R[l]
            A[l + 1] = R[l] + T[l] * T[l] * A[l] / c
            G[l + 1] = P[l] + T[l] * (G[l] + A[l] * Q[l]) / c
        dn, up = np.zeros((L + 1, n), dtype=dtype), np.empty((L + 1, n), dtype=dtype)
        up[L] = G[L]
        for l in range(L - 1, -1, -1):
            dn[l] = (T[l] * dn[l + 1] + Q[l] + R[l] * G[l]) / (1 - A[l] * R[l])
            up[l] = A[l] * dn[l] + G[l]
    return up, dn, direct, pole


def dense(R, T, P, Q, e, direct0):
    """The layer relations of ONE point as a dense linear system (numpy.linalg.solve): R, T, P, Q (L,) -> up, dn (L + 1,)"""
    L = len(R)
    N = 2 * (L + 1)                 # unknowns up_0 .. up_L, dn_0 .. dn_L
    M, rhs = np.zeros((N, N)), np.zeros(N)
    M[0, 0], M[0, L + 1], rhs[0] = 1.0, -(1 - e), (1 - e) * direct0
    for l in range(L):
        r = 1 + l                   # up_(l+1) - T up_l - R dn_(l+1) = P
        M[r, l + 1], M[r, l], M[r, L + 1 + l + 1], rhs[r] = 1.0, -T[l], -R[l], P[l]
        r = 1 + L + l               # dn_l - T dn_(l+1) - R up_l = Q
        M[r, L + 1 + l] = 1.0
        M[r, L + 1 + l + 1] -= T[l]
        M[r, l] -= R[l]
        rhs[r] = Q[l]
    M[N - 1, N - 1] = 1.0           # dn_L = 0
    sol = np.linalg.solve(M, rhs)
    return sol[:L + 1], sol[L + 1:]


def band_sums(values, first, count):
    """sum over the band's points of nan_to_num, per level: values (L + 1, n) -> (L + 1,)"""
    return np.nan_to_num(np.asarray(values, dtype=np.float64)[:, first:first + count]).sum(axis=1)
