"""The Jacobian of lbl_column_jacobian_scatter_dev (include/pyrad_hip.h) restated in NumPy and float64, for the tests.
Not the kernels' route: the layer's logarithmic derivatives p dX/dp and q dX/dq come from the quotient rule applied to
R = Gam oE / N and the product rule applied to Ab = (1 - Gam) (1 - E) / (1 + Gam E), not from the header's closed forms (a depth that is 0 has the logarithmic
derivative 0 by definition), and the column's derivative from the adjoint of the DENSE system
of scatter_flux_ref.dense - M^T lam = e_(up_L), dF/dtheta = lam . (d rhs/dtheta - dM/dtheta x) - solved for all points in
one batched numpy.linalg.solve.  column_scalar is the same column in any scalar arithmetic (mpmath in the tests), to be
differentiated numerically there."""
import numpy as np

import scatter_flux_ref as sf
import twostream_ref as two

PI, D = sf.PI, sf.D


def planck_dT(nu, T):
    """dB/dT of scatter_flux_ref.planck"""
    nu = np.asarray(nu, dtype=np.float64)
    with np.errstate(all="ignore"):
        b = 100 * sf.H * sf.C * nu / sf.KB / T
        return sf.planck(nu, T) * b / -np.expm1(-b) / T


def layer_partials(ta, ts, tsg):
    """R, T, Ab, h of one layer at n points and their logarithmic derivatives to p = D ta and q = D (t - tsg), as a dict of
    (n,) arrays: X, and X_p = p dX/dp, X_q = q dX/dq for X in R, T, Ab, h; `dark` where the layer emits nothing, `empty`
    where t == 0.  The quotient rule on R = Gam oE / N, N = c2 + Gam^2 oE, c2 = 1 - Gam^2, the product rule on Ab, and
    T = 1 - R - Ab, with p dGam/dp = -r s / (s + r)^2 = -q dGam/dq and p dx/dp = q dx/dq = x / 2: nothing of order 1 is
    subtracted in a thin layer (the quotient rule on T would, and h divides the result by q)."""
    ta, ts, tsg = (np.asarray(v, dtype=np.float64) for v in (ta, ts, tsg))
    R, T = two.layer(ta, ts, tsg, [1.0])[:2]
    Ab, cons = sf.absorptance(ta, ts, tsg)
    with np.errstate(all="ignore"):
        t = ta + ts
        empty = t == 0
        p, q = D * ta, D * (t - tsg)
        r, s = np.sqrt(p), np.sqrt(q)
        x = r * s
        Gam = (s - r) / (s + r)
        E = np.exp(-x)
        oE = -np.expm1(-2 * x)
        G = (r / (s + r)) * (s / (s + r))
        c2 = 4 * G
        N = c2 + Gam * Gam * oE
        out = {"R": R, "T": T, "Ab": Ab}
        y = (p + q) / 2             # den == 0: R = y / (1 + y), T = 1 / (1 + y)
        # Ab = (1 - Gam) (1 - E) / (1 + Gam E), a product: its logarithmic derivative term by term
        oG1, oE1 = 2 * (r / (s + r)), -np.expm1(-x)
        for name, dGam, part in (("p", -G, p), ("q", G, q)):
            dx = x / 2
            dc2 = -2 * Gam * dGam
            doE = 2 * E * E * dx
            dN = dc2 + 2 * Gam * oE * dGam + Gam * Gam * doE
            dR = (dGam * oE + Gam * doE) / N - R * dN / N
            dAb = Ab * (-dGam / oG1 + E * dx / oE1 - (E * dGam - Gam * E * dx) / (1 + Gam * E))
            dR = np.where(cons, (part / 2) / (1 + y) ** 2, dR)
            dAb = np.where(cons, 0.0, dAb)
            out["R_" + name] = np.where(empty, 0.0, dR)
            out["Ab_" + name] = np.where(empty, 0.0, dAb)
            out["T_" + name] = -(out["R_" + name] + out["Ab_" + name])
        out["h"] = (Ab + 2 * R) / q - T
        out["h_p"] = (out["Ab_p"] + 2 * out["R_p"]) / q - out["T_p"]
        out["h_q"] = ((out["Ab_q"] + 2 * out["R_q"]) - (Ab + 2 * R)) / q - out["T_q"]
    out["dark"] = empty | cons | (ta == 0)
    out["empty"] = empty
    return out


def adjoint(R, T, e):
    """lam of M^T lam = e_(up_L) for the dense system of scatter_flux_ref.dense at n points: R, T (L, n), e (n,) ->
    (2 (L + 1), n): lam[0] answers the surface's row, lam[1 + l] layer l's upward row, lam[1 + L + l] its downward row"""
    L, n = R.shape
    N = 2 * (L + 1)
    M = np.zeros((n, N, N))
    M[:, 0, 0], M[:, 0, L + 1] = 1.0, -(1 - e)
    for l in range(L):
        a, b = 1 + l, 1 + L + l
        M[:, a, l + 1] += 1.0
        M[:, a, l] -= T[l]
        M[:, a, L + 1 + l + 1] -= R[l]
        M[:, b, L + 1 + l] += 1.0
        M[:, b, L + 1 + l + 1] -= T[l]
        M[:, b, l] -= R[l]
    M[:, N - 1, N - 1] = 1.0
    rhs = np.zeros((n, N, 1))
    rhs[:, L, 0] = 1.0
    return np.linalg.solve(M.transpose(0, 2, 1), rhs)[:, :, 0].T


def jacobian(k, depth, nu, T_edge, linear, amount=(), numbers=(), delta=1, emissivity=1.0, I_surface=None, surface_T=None,
             I_top=None, terms=(), term_layer=()):
    """Every spectral row of lbl_column_jacobian_scatter_dev at the n wavenumbers nu; the arguments are
    scatter_flux_ref.column's, `linear` the Planck source, `terms` (M, n) partial absorption coefficients of the layers
    term_layer.  Returns a dict: F, dTs, de (n,), dtau (L, n), dT (NT L, n), dscat (C, L, n), dterm (M, n); a point with
    a t that is not finite is NaN in every row."""
    k = np.asarray(k, dtype=np.float64).reshape(len(depth), -1)
    L, n = k.shape
    nu = np.asarray(nu, dtype=np.float64)
    T_edge = np.asarray(T_edge, dtype=np.float64).reshape(L, 2)
    NT = 2 if linear else 1
    C = len(numbers)
    ta, ts, tsg = two.optical(k, depth, amount, numbers, delta)
    e = np.broadcast_to(np.asarray(emissivity, dtype=np.float64), (n,))
    lay = [layer_partials(ta[l], ts[l], tsg[l]) for l in range(L)]
    Bb = [PI * sf.planck(nu, T_edge[l, 0]) for l in range(L)]
    Bt = [PI * sf.planck(nu, T_edge[l, 1]) for l in range(L)]
    R = np.array([y["R"] for y in lay]).reshape(L, n)
    T = np.array([y["T"] for y in lay]).reshape(L, n)
    up, dn = sf.column(k, depth, nu, T_edge, amount, numbers, delta, emissivity, I_surface, surface_T, I_top)
    bad = ~np.all(np.isfinite(ta + ts), axis=0)
    good = ~bad
    lam = np.full((2 * (L + 1), n), np.nan)
    if good.any():
        lam[:, good] = adjoint(np.where(good, R, 0.0)[:, good], np.where(good, T, 1.0)[:, good], e[good])
    Es = PI * (np.asarray(I_surface, dtype=np.float64) if I_surface is not None else sf.planck(nu, surface_T))
    out = {"F": up[L].copy(), "de": lam[0] * (Es - dn[0])}
    out["dTs"] = lam[0] * e * PI * planck_dT(nu, surface_T) if I_surface is None else np.zeros(n)
    dtau, dT, dta_all = np.zeros((L, n)), np.zeros((NT * L, n)), np.zeros((L, n))
    dscat = np.zeros((C, L, n))
    with np.errstate(all="ignore"):
        for l in range(L):
            y = lay[l]
            w1, w2 = lam[1 + l], lam[1 + L + l]
            d = Bb[l] - Bt[l]
            F = {}
            for v in ("p", "q"):
                if linear:
                    dP = Bt[l] * y["Ab_" + v] + d * y["h_" + v]
                    dQ = Bb[l] * y["Ab_" + v] - d * y["h_" + v]
                else:
                    dP = dQ = Bb[l] * y["Ab_" + v]
                dP, dQ = np.where(y["dark"], 0.0, dP), np.where(y["dark"], 0.0, dQ)
                F[v] = (w1 * (y["T_" + v] * up[l] + y["R_" + v] * dn[l + 1] + dP)
                        + w2 * (y["T_" + v] * dn[l + 1] + y["R_" + v] * up[l] + dQ))
            # p F_p = ta dF/dta's part through p, q F_q = (t - tsg) dF/d(t - tsg): 0 where the depth is 0
            tq = (ta[l] + ts[l]) - tsg[l]
            fa = np.where(ta[l] > 0, F["p"] / np.where(ta[l] > 0, ta[l], 1.0), 0.0)
            fq = np.where(tq > 0, F["q"] / np.where(tq > 0, tq, 1.0), 0.0)
            F_ta, F_ts, F_tsg = fa + fq, fq, -fq
            dta_all[l] = F_ta
            dtau[l] = k[l] * depth[l] * F_ta
            for c, (ext, ssa, g) in enumerate(numbers):
                al, si, et = two.scatterer_numbers(ext, ssa, g, delta)
                dscat[c, l] = amount[c][l] * (al * F_ta + si * F_ts + et * F_tsg)
            dBb = PI * planck_dT(nu, T_edge[l, 0])
            dBt = PI * planck_dT(nu, T_edge[l, 1])
            if linear:
                h, Ab = y["h"], y["Ab"]
                dT[2 * l] = np.where(y["dark"], 0.0, (w1 * h + w2 * (Ab - h)) * dBb)
                dT[2 * l + 1] = np.where(y["dark"], 0.0, (w1 * (Ab - h) + w2 * h) * dBt)
            else:
                dT[l] = np.where(y["dark"], 0.0, (w1 + w2) * y["Ab"] * dBb)
        dterm = np.zeros((len(terms), n))
        for m, l in enumerate(term_layer):
            dterm[m] = np.asarray(terms[m], dtype=np.float64) * depth[l] * dta_all[l]
    out.update(dtau=dtau, dT=dT, dscat=dscat, dterm=dterm)
    for v in out.values():
        v[..., bad] = np.nan
    return out


def band_rows(J, first, count):
    """jac's rows of one band from jacobian()'s dict: [F, dTs, de, L d ln tau, NT L dT, C x L amounts, terms], each the sum
    over the band's points of nan_to_num"""
    rows = np.concatenate([J["F"][None], J["dTs"][None], J["de"][None], J["dtau"], J["dT"],
                           J["dscat"].reshape(-1, J["F"].shape[0]), J["dterm"]])
    return np.nan_to_num(rows[:, first:first + count]).sum(axis=1)


def column_scalar(ta, ts, tsg, Bb, Bt, e, Es, dn_top, linear, num, sqrt, exp, expm1):
    """up_L of one point in the arithmetic of ``num``: the layers from twostream_ref.layer_scalar and
    scatter_flux_ref.sources_scalar (planck_linear 0: Bt = Bb, whose P = Q = (1 - R - T) Bb), joined by adding from the
    surface upwards.  ta, ts, tsg, Bb, Bt: one number per layer."""
    A, G = 1 - num(e), num(e) * num(Es)
    for l in range(len(ta)):
        R, T = two.layer_scalar(ta[l], ts[l], tsg[l], 1.0, num, sqrt, exp, expm1)[:2]
        if ta[l] + ts[l] == 0 or ta[l] == 0:
            P = Q = num(0)
        else:
            P, Q = sf.sources_scalar(ta[l], ts[l], tsg[l], Bt[l] if linear else Bb[l], Bb[l], num, sqrt, exp, expm1)
        c = 1 - A * R
        A, G = R + T * T * A / c, P + T * (G + A * Q) / c
    return A * num(dn_top) + G
