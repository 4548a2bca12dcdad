"""CPU: Jacobians of the linear-in-optical-depth Planck source (Atmosphere.jacobiansLinear, pathJacobiansLinear and
observeLinear; lbl_column_jacobian_linear_dev, lbl_ray_jacobian_linear_dev, lbl_ray_jacobian_linear_rows; kernels K5j) without
a device - g' of pyrad_amd/csrc/lbl_linear_source.h compiled with g++ from the text the device compiles, the NumPy
restatements of both semantics that the GPU tests compare against, checked here against central finite differences of the
NumPy forward model of tests/test_gpu_linear_source.py; the C ABI surface, the kernels' resource report, the row layout, the
level-temperature chain and the host-side validation, which runs before anything touches a context."""
import ctypes
import decimal
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyrad_oracle as orc
from pyrad_amd import _native, model, settings
from test_gpu_linear_source import flux_walk, g_of, leaving, step, walk
from test_jacobian_cpu import planck_dT
from test_surface_jacobian_cpu import weight_sum

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
G_HEADER = os.path.join(_native.CSRC, "lbl_linear_source.h")
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
SYMBOLS = ("lbl_column_jacobian_linear_dev", "lbl_ray_jacobian_linear_dev", "lbl_ray_jacobian_linear_rows")
MARKER = -1           # the segment layer of a surface marker
BAD_ARG = -1
DG_TAU0 = 0.375
DG_BOUND = 1e-14      # what the header derives for the closed form at its switch-over: a tenth of the spectral tolerance


# ---- g' -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dg_c(tmp_path_factory):
    """linear_source_dg(tau, t) over arrays, from a small shared library built from the header with g++"""
    d = tmp_path_factory.mktemp("linear_dg")
    src = d / "linear_dg.cpp"
    src.write_text('#include "%s"\n'
                   'extern "C" void dg_array(const double* tau, const double* t, long n, double* out) {\n'
                   '    for (long i = 0; i < n; ++i) out[i] = lbl::linear_source_dg(tau[i], t[i]);\n'
                   '}\n'
                   'extern "C" double dg_tau0() { return LBL_LINEAR_DG_TAU0; }\n'
                   'extern "C" int dg_terms() { return LBL_LINEAR_DG_TERMS; }\n' % G_HEADER)
    lib = d / "liblinear_dg.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(lib), str(src)])
    dll = ctypes.CDLL(str(lib))
    P = ctypes.POINTER(ctypes.c_double)
    dll.dg_array.argtypes = [P, P, ctypes.c_long, P]
    dll.dg_array.restype = None
    dll.dg_tau0.restype = ctypes.c_double
    dll.dg_terms.restype = ctypes.c_int

    def call(tau, t):
        tau, t = np.ascontiguousarray(tau, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64)
        out = np.empty(tau.shape)
        dll.dg_array(tau.ctypes.data_as(P), t.ctypes.data_as(P), tau.size, out.ctypes.data_as(P))
        return out
    call.tau0, call.terms = dll.dg_tau0(), dll.dg_terms()
    return call


def _dg_exact(tau):
    """(1 - t (1 + tau)) / tau^2 at 50 digits (the series below 1e-3, where the expression loses its digits)"""
    ctx = decimal.Context(prec=50)
    x = decimal.Decimal(float(tau))
    if x < decimal.Decimal("1e-3"):
        s, power = decimal.Decimal(0), decimal.Decimal(1)      # sum_n (-1)^(n+1) n x^(n-1) / (n+1)!: 30 terms, the last below 1e-120
        for n in range(1, 31):
            c = ctx.divide(decimal.Decimal(n), decimal.Decimal(math.factorial(n + 1)))
            s = ctx.add(s, ctx.multiply(c if n % 2 else -c, power))
            power = ctx.multiply(power, x)
        return s
    t = ctx.exp(-x)
    return ctx.divide(ctx.subtract(1, ctx.multiply(t, ctx.add(1, x))), ctx.multiply(x, x))


def test_dg_against_fifty_digits(dg_c):
    tau0, terms = dg_c.tau0, dg_c.terms
    with open(G_HEADER) as fh:
        text = fh.read()
    assert re.search(r"#define\s+LBL_LINEAR_DG_TAU0\s+0\.375\b", text) and tau0 == DG_TAU0
    assert re.search(r"#define\s+LBL_LINEAR_DG_TERMS\s+13\b", text) and terms == 13
    # the series' truncation at tau_0 - its first term left out, (n + 1) tau0^n / (n + 2)! - is below 2^-53 relative to g'(tau_0);
    # one term fewer is not
    dg0 = float(_dg_exact(tau0))
    assert (terms + 1) * tau0 ** terms / math.factorial(terms + 2) < 2.0 ** -53 * dg0
    assert terms * tau0 ** (terms - 1) / math.factorial(terms + 1) > 2.0 ** -53 * dg0
    # the closed form's bound as the header derives it: 2^-53 (1/2 + 2 (1 + 1 / tau)) / hh + 2^-53 with a t good to 2 ulp
    hh = lambda x: (1 - math.exp(-x)) / x - math.exp(-x)
    derived = 2.0 ** -53 * (0.5 + 2 * (1 + 1 / tau0)) / hh(tau0) + 2.0 ** -53
    assert derived <= DG_BOUND < 2.0 ** -53 * (0.5 + 2 * (1 + 1 / 0.25)) / hh(0.25) + 2.0 ** -53      # and g's 1/4 would miss it
    tau = np.concatenate([[0.0, 1e-300, 1e-12], np.logspace(-9, math.log10(800.0), 2000), np.linspace(0.3, 0.45, 301),
                          [np.nextafter(tau0, 0.0), tau0, np.nextafter(tau0, 1.0)]])
    tau.sort()
    t = np.array([math.exp(-x) for x in tau])
    dg = dg_c(tau, t)
    worst, where = 0.0, 0.0
    for x, v in zip(tau, dg):
        ref = _dg_exact(x)
        err = float(abs((decimal.Decimal(float(v)) - ref) / ref))
        if err > worst:
            worst, where = err, x
    print("worst relative error of g': %.3e at tau = %.6g (derived bound at tau_0 %.2e)" % (worst, where, derived))
    assert worst <= DG_BOUND, (worst, where)
    # Falling, across the switch-over too.  Two neighbouring doubles differ in g' by ~4e-17 while the closed form carries the
    # error derived above (an ulp of t alone moves it by 2^-53 (1 + 1 / tau) / tau), so falling is asked of samples whose true
    # decrease, |g''| dtau >= 0.18 dtau on [0.3, 0.45], exceeds twice that bound, 2 * 1e-14 * 0.5: dtau >= 1e-12 does by a
    # factor of 18.  Both grids below straddle tau_0: 5e-4 apart, and 1e-12 apart over the 200 steps around it.
    coarse = np.concatenate([[0.0], np.logspace(-9, math.log10(800.0), 2000), np.linspace(0.3, 0.45, 301)])
    coarse.sort()
    fine = tau0 + 1e-12 * np.arange(-100, 101)
    for grid in (coarse, fine):
        v = dg_c(grid, [math.exp(-x) for x in grid])
        assert np.any(grid < tau0) and np.any(grid >= tau0)
        assert np.all(np.diff(v) <= 0.0), "g' must not rise"
    assert np.all((dg >= 0.0) & (dg <= 0.5))
    # ... and the two forms meet at tau_0 within the bound
    lo, hi = dg_c([np.nextafter(tau0, 0.0), tau0], [math.exp(-np.nextafter(tau0, 0.0)), math.exp(-tau0)])
    assert abs(lo - hi) <= DG_BOUND * hi
    # h = tau g' agrees with (1 - t) - g, the step's weight of Ba, on the NumPy side
    x = np.logspace(-6, 2, 400)
    tt = np.exp(-x)
    assert np.allclose(x * dg_c(x, tt), (1 - tt) - g_of(x, tt), rtol=1e-9, atol=1e-16)


def test_dg_limits(dg_c):
    dg = dg_c([0.0, np.inf, np.nan, 800.0, 1e-300], [1.0, 0.0, np.nan, 0.0, 1.0])
    assert dg[0] == 0.5
    assert dg[1] == 0.0 and not np.isnan(dg[1])
    assert np.isnan(dg[2])
    assert dg[3] == (1.0 / 800.0) / 800.0
    assert dg[4] == 0.5
    assert np.isnan(dg_c([np.nan], [0.5])[0]) and np.isnan(dg_c([1.0], [np.nan])[0])


# ---- the semantics, restated in NumPy (include/pyrad_hip.h; every level radiance stored) -------------------------------------
def dg_of(tau, t):
    """g'(tau) = ((1 - t) / tau - t) / tau, by its Taylor series below its switch-over"""
    tau = np.asarray(tau, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        direct = ((1.0 - t) / tau - t) / tau
        s = np.zeros_like(tau)
        for n in range(22, 0, -1):                      # n / (n + 1)!
            s = n / float(math.factorial(n + 1)) - tau * s
        return np.where(tau >= DG_TAU0, direct, s)


def linear_jacobian_reference(x, k, edges, depth, mu, w, e, reflection, surface_T=None, surface=None, top=None, terms=(),
                              idx=None, res=1.0):
    """lbl_column_jacobian_linear_dev: dict of band values (leading band axis) and spectra.  edges[l] = (bottom, top)
    temperature of layer l; e: a number or x.size values; terms: (layer, k_m) pairs.  The forward model is flux_walk's."""
    L, n = len(k), x.size
    idx = [(0, n)] if idx is None else idx
    e = e * np.ones(n)
    Bb = [orc.planckWavenumber(x, edges[l][0]) for l in range(L)]
    Bt = [orc.planckWavenumber(x, edges[l][1]) for l in range(L)]
    dBb = [planck_dT(x, edges[l][0]) for l in range(L)]
    dBt = [planck_dT(x, edges[l][1]) for l in range(L)]
    Is = np.array(surface, dtype=np.float64) if surface is not None else orc.planckWavenumber(x, surface_T)
    dBs = np.zeros(n) if surface is not None else planck_dT(x, surface_T)
    Wsum = weight_sum(w)
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        tau = [[(k[l] * depth[l]) * (1.0 / m) for l in range(L)] for m in mu]
        t = [[np.exp(-tau[a][l]) for l in range(L)] for a in range(len(mu))]
        Id, Ttot = [], []
        for a in range(len(mu)):                       # Id[l + 1] enters layer l from above, at its top edge
            lev = [None] * (L + 1)
            lev[L] = np.zeros(n) if top is None else np.array(top, dtype=np.float64)
            for l in range(L - 1, -1, -1):
                lev[l] = step(lev[l + 1], tau[a][l], Bt[l], Bb[l])[0]
            Id.append(lev)
            Ttot.append(np.prod(t[a], axis=0) if L else np.ones(n))
        F0 = sum(wk * lev[0] for wk, lev in zip(w, Id))
        S = sum(wk * tt for wk, tt in zip(w, Ttot))
        F, dTs, de = np.zeros(n), np.zeros(n), np.zeros(n)
        dtau, core, dT = np.zeros((L, n)), np.zeros((L, n)), np.zeros((2 * L, n))
        for a, (m, wk) in enumerate(zip(mu, w)):
            R = F0 / Wsum if reflection == "lambertian" else Id[a][0]
            Q = (1 - e) * wk * (S / Wsum if reflection == "lambertian" else Ttot[a])
            Iu = [leaving(e, Is, R)]
            for l in range(L):                         # Iu[l] enters layer l from below, at its bottom edge
                Iu.append(step(Iu[l], tau[a][l], Bb[l], Bt[l])[0])
            A, C = [None] * L, [None] * L
            acc = np.ones(n)
            for l in range(L - 1, -1, -1):
                A[l] = acc
                acc = acc * t[a][l]
            acc = np.ones(n)
            for l in range(L):
                C[l] = acc
                acc = acc * t[a][l]
            F += wk * Iu[L]
            for l in range(L):
                xl, tl = tau[a][l], t[a][l]
                g, dg = g_of(xl, tl), dg_of(xl, tl)
                h = xl * dg
                cu = tl * (Bb[l] - Iu[l]) + dg * (Bt[l] - Bb[l])
                cd = tl * (Bt[l] - Id[a][l + 1]) + dg * (Bb[l] - Bt[l])
                dtau[l] += wk * A[l] * (xl * tl * (Bb[l] - Iu[l]) + h * (Bt[l] - Bb[l])) \
                    + Q * C[l] * (xl * tl * (Bt[l] - Id[a][l + 1]) + h * (Bb[l] - Bt[l]))
                core[l] += (wk * A[l] * cu + Q * C[l] * cd) / m
                dT[2 * l] += dBb[l] * (wk * A[l] * h + Q * C[l] * g)
                dT[2 * l + 1] += dBt[l] * (wk * A[l] * g + Q * C[l] * h)
            dTs += e * wk * Ttot[a] * dBs
            de += wk * Ttot[a] * (Is - R)
    band = lambda y: np.array([res * np.sum(np.nan_to_num(y[..., i:j]), axis=-1) for i, j in idx])
    out = dict(olr=band(F), surfaceTemperature=band(dTs), emissivity=band(de), opticalDepth=band(dtau), edgeTemperature=band(dT),
               opticalDepthSpectrum=dtau, edgeTemperatureSpectrum=dT, emissivitySpectrum=de, olrSpectrum=F)
    out["terms"] = np.stack([band(km * depth[l] * core[l]) for l, km in terms], axis=-1) if terms else None
    return out


def linear_path_jacobian_reference(x, k, layers, lengths, temps, kind, e, surface_T=None, surface=None, terms=()):
    """lbl_ray_jacobian_linear_dev for one ray: dict(radiance, sourceTemperature, emissivity, opticalDepth {layer: row},
    segmentTemperature [(dTa, dTb) per real segment in order of travel], terms {term index: row}), by the direct forms with
    the radiance arriving at every element stored.  The forward model is walk's (without a diffuse start term)."""
    n = x.size
    e = e * np.ones(n)
    Is = dBs = np.zeros(n)
    if surface is not None:
        Is = np.array(surface, dtype=np.float64)
    elif surface_T is not None:
        Is, dBs = orc.planckWavenumber(x, surface_T), planck_dT(x, surface_T)
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        I = [leaving(e, Is, 0.0) * np.ones(n) if kind == 1 else np.zeros(n)]      # I[s] arrives at element s
        f = []                                                                     # what element s passes on of it
        for l, s, (Ta, Tb) in zip(layers, lengths, temps):
            if l == MARKER:
                f.append(1 - e)
                I.append(leaving(e, Is, I[-1]))
            else:
                nxt, t = step(I[-1], k[l] * s, orc.planckWavenumber(x, Ta), orc.planckWavenumber(x, Tb))
                f.append(t)
                I.append(nxt)
        crossed = sorted(set(l for l in layers if l != MARKER))
        dtau = {l: np.zeros(n) for l in crossed}
        rows = {m: np.zeros(n) for m, (l, km) in enumerate(terms) if l in crossed}
        seg = [None] * len(layers)
        dTs, de = np.zeros(n), np.zeros(n)
        A = np.ones(n)
        for s in range(len(layers) - 1, -1, -1):
            l, length = layers[s], lengths[s]
            if l == MARKER:
                dTs += A * e * dBs
                de += A * (Is - I[s])
            else:
                Ta, Tb = temps[s]
                Ba, Bb = orc.planckWavenumber(x, Ta), orc.planckWavenumber(x, Tb)
                tau, t = k[l] * length, f[s]
                g, dg = g_of(tau, t), dg_of(tau, t)
                dtau[l] += A * (tau * t * (Ba - I[s]) + (tau * dg) * (Bb - Ba))
                seg[s] = (A * (tau * dg) * planck_dT(x, Ta), A * g * planck_dT(x, Tb))
                for m, (lm, km) in enumerate(terms):
                    if lm == l:
                        rows[m] += km * length * A * (t * (Ba - I[s]) + dg * (Bb - Ba))
            A = A * f[s]
        if kind == 1:
            dTs += A * e * dBs
            de += A * Is
    return dict(radiance=I[-1], sourceTemperature=dTs, emissivity=de, opticalDepth=dtau,
                segmentTemperature=[p for p in seg if p is not None], terms=rows)


# ---- both restatements against central differences of the forward model ----------------------------------------------------
def _tiny_column(seed=5):
    """4 layers, 7 points, two molecules per layer, optical depths from thin to a few (both forms of g and g' are met)"""
    rng = np.random.default_rng(seed)
    x = np.linspace(640.0, 700.0, 7)
    k_m = [[rng.uniform(1e-6, 4e-5, x.size) for m in range(2)] for l in range(4)]
    k = [sum(km) for km in k_m]
    edges = [(296.0, 279.0), (277.0, 246.0), (249.0, 222.0), (220.0, 209.0)]       # (not continuous: the edges are independent)
    return x, k_m, k, edges, [1.5e4, 4e4, 9e4, 7e4]


def _near(a, fd, scale, what):
    assert np.all(np.abs(a - fd) <= 1e-6 * np.abs(fd) + 1e-9 * scale), (what, a, fd)


@pytest.mark.parametrize("reflection", ["lambertian", "specular"])
def test_column_restatement_against_finite_differences(reflection):
    x, k_m, k, edges, depth = _tiny_column()
    mu, w = model.fluxAngles(3)
    Ts = 295.0
    e = np.linspace(0.35, 0.95, x.size)
    top = 0.4 * orc.planckWavenumber(x, 250.0)
    terms = [(l, km) for l in range(len(k)) for km in k_m[l]]
    ref = linear_jacobian_reference(x, k, edges, depth, mu, w, e, reflection, surface_T=Ts, top=top, terms=terms)
    scale = np.max(ref["olrSpectrum"])
    taus = np.concatenate([k[l] * depth[l] / m for l in range(len(k)) for m in mu])
    assert np.any(taus < 0.25) and np.any(taus > DG_TAU0)

    def F(k=k, edges=edges, depth=depth, e=e, Ts=Ts):
        return flux_walk(x, k, edges, depth, mu, w, orc.planckWavenumber(x, Ts), e, reflection, top=top)[2]

    assert np.allclose(ref["olrSpectrum"], F(), rtol=1e-14, atol=0)
    eps, h = 1e-4, 1e-2
    for l in range(len(k)):
        dp, dm = list(depth), list(depth)
        dp[l] *= np.exp(eps)
        dm[l] *= np.exp(-eps)
        _near(ref["opticalDepthSpectrum"][l], (F(depth=dp) - F(depth=dm)) / (2 * eps), scale, "ln tau %d" % l)
        for side in range(2):
            Tp, Tm = [list(p) for p in edges], [list(p) for p in edges]
            Tp[l][side] += h
            Tm[l][side] -= h
            _near(ref["edgeTemperatureSpectrum"][2 * l + side], (F(edges=Tp) - F(edges=Tm)) / (2 * h), scale,
                  "T edge %d %d" % (l, side))
    for t, (l, km) in enumerate(terms):
        kp, kn = list(k), list(k)
        kp[l] = k[l] + eps * km
        kn[l] = k[l] - eps * km
        _near(ref["terms"][0, t], np.sum((F(k=kp) - F(k=kn)) / (2 * eps)), scale, "term %d" % t)
    _near(ref["surfaceTemperature"][0], np.sum((F(Ts=Ts + h) - F(Ts=Ts - h)) / (2 * h)), scale, "T_s")
    fd = (F(e=e + 0.04) - F(e=e - 0.04)) / 0.08                  # F is affine in e
    assert np.all(np.abs(ref["emissivitySpectrum"] - fd) <= 1e-12 * scale), (ref["emissivitySpectrum"], fd)
    for l in range(len(k)):
        assert np.allclose(ref["terms"][:, 2 * l] + ref["terms"][:, 2 * l + 1], ref["opticalDepth"][:, l], rtol=1e-12, atol=0)
    # equal edges: the surface variant's restatement, and bottom + top is its dF/dT_l
    from test_surface_jacobian_cpu import surface_jacobian_reference
    T = [t0 for t0, _ in edges]
    same = linear_jacobian_reference(x, k, [(t0, t0) for t0 in T], depth, mu, w, e, reflection, surface_T=Ts, top=top, terms=terms)
    iso = surface_jacobian_reference(x, k, T, depth, mu, w, e, reflection, surface_T=Ts, top=top, terms=terms)
    for name in ("olr", "surfaceTemperature", "emissivity", "opticalDepth", "terms"):
        assert np.allclose(same[name], iso[name], rtol=1e-12, atol=1e-15 * scale), name
    assert np.allclose(same["edgeTemperature"][:, 0::2] + same["edgeTemperature"][:, 1::2], iso["temperature"], rtol=1e-12, atol=0)


RAYS = (([3, 2, 1, 0, MARKER, 0, 1, 2, 3], 0), ([3, 2, 1, 0, MARKER, 0, 1], 0), ([1, 0, MARKER, 0, 2], 1), ([MARKER, 0, 1, 2, 3], 0),
        ([2, 1, MARKER], 1), ([1, 0, MARKER, 0, MARKER, 0, 1], 0), ([MARKER], 0), ([MARKER], 1), ([0, 1, 2, 3], 1), ([], 1),
        ([2, 1, 1, 0, 1], 0))


@pytest.mark.parametrize("ray", range(len(RAYS)))
def test_ray_restatement_against_finite_differences(ray):
    x, k_m, k, _, depth = _tiny_column()
    layers, kind = RAYS[ray]
    rs = np.random.RandomState(ray)
    lengths = [0.0 if l == MARKER else float(rs.uniform(1e4, 6e4)) for l in layers]
    temps = [(0.0, 0.0) if l == MARKER else tuple(rs.uniform(205.0, 300.0, 2)) for l in layers]
    Ts = 295.0
    e = np.linspace(0.35, 0.95, x.size)
    terms = [(l, km) for l in range(len(k)) for km in k_m[l]]
    ref = linear_path_jacobian_reference(x, k, layers, lengths, temps, kind, e, surface_T=Ts, terms=terms)

    def I(k=k, lengths=lengths, temps=temps, e=e, Ts=Ts):
        return walk(x, k, layers, lengths, temps, kind, e=e, Is=orc.planckWavenumber(x, Ts))[0]

    scale = max(np.max(ref["radiance"]), 1e-300)
    assert np.allclose(ref["radiance"], I(), rtol=1e-14, atol=0)
    eps, h = 1e-4, 1e-2
    for l in range(len(k)):
        if l not in ref["opticalDepth"]:
            assert l not in layers
            continue
        lp = [s * np.exp(eps) if ll == l else s for ll, s in zip(layers, lengths)]
        lm = [s * np.exp(-eps) if ll == l else s for ll, s in zip(layers, lengths)]
        _near(ref["opticalDepth"][l], (I(lengths=lp) - I(lengths=lm)) / (2 * eps), scale, "ln tau %d" % l)
    real = [s for s, l in enumerate(layers) if l != MARKER]
    assert len(ref["segmentTemperature"]) == len(real)
    for i, s in enumerate(real):
        for side in range(2):
            Tp, Tm = [list(p) for p in temps], [list(p) for p in temps]
            Tp[s][side] += h
            Tm[s][side] -= h
            _near(ref["segmentTemperature"][i][side], (I(temps=Tp) - I(temps=Tm)) / (2 * h), scale, "T seg %d %d" % (s, side))
    for t, (l, km) in enumerate(terms):
        assert (t in ref["terms"]) == (l in layers)
        if t in ref["terms"]:
            kp, kn = list(k), list(k)
            kp[l] = k[l] + eps * km
            kn[l] = k[l] - eps * km
            _near(ref["terms"][t], (I(k=kp) - I(k=kn)) / (2 * eps), scale, "term %d" % t)
    _near(ref["sourceTemperature"], (I(Ts=Ts + h) - I(Ts=Ts - h)) / (2 * h), scale, "T_s")
    fd = (I(e=e + 0.04) - I(e=e - 0.04)) / 0.08
    assert np.all(np.abs(ref["emissivity"] - fd) <= 1e-12 * scale), (ref["emissivity"], fd)
    given = linear_path_jacobian_reference(x, k, layers, lengths, temps, kind, e, surface=orc.planckWavenumber(x, Ts))
    assert np.all(given["sourceTemperature"] == 0.0) and np.allclose(given["emissivity"], ref["emissivity"], rtol=1e-14)


# ---- the C ABI surface -------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"int\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    sig = _native.SIGNATURES
    assert sig["lbl_column_jacobian_linear_dev"] == sig["lbl_column_jacobian_surface_dev"]
    assert sig["lbl_ray_jacobian_linear_dev"] == sig["lbl_ray_jacobian_surface_dev"]
    assert sig["lbl_ray_jacobian_linear_rows"] == sig["lbl_ray_jacobian_surface_rows"]
    assert re.search(r"lbl_column_jacobian_linear_dev\([^;]*const double\* T_edge", text)
    assert re.search(r"lbl_column_jacobian_linear_dev\([^;]*jac_T_edge_spectra", text)
    assert re.search(r"lbl_ray_jacobian_linear_dev\([^;]*const double\* seg_T", text)
    assert hasattr(_native.Context, "column_jacobian_linear_dev") and hasattr(_native.Context, "ray_jacobian_linear_dev")
    assert lib.lbl_abi_version() == 5 and "#define LBL_ABI_VERSION 5" in text
    with open(os.path.join(os.path.dirname(HEADER), "..", "INTEGRATION.md")) as fh:
        doc = fh.read()
    for name in SYMBOLS:
        assert name in doc, name
    for method in ("jacobiansLinear", "pathJacobiansLinear", "observeLinear"):
        assert callable(getattr(model.Atmosphere, method)), method


def _template_args(name, kernel):
    m = re.search(kernel + r"I((?:Li\d+E)+)E", name)
    assert m, name
    return tuple(int(v) for v in re.findall(r"Li(\d+)E", m.group(1)))


def test_linear_jacobian_kernels_in_the_resource_report():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    column = {_template_args(n, "linear_jacobian_kernel"): f for n, f in k.items()
              if "linear_jacobian_kernel" in n and "ray_linear_jacobian_kernel" not in n}
    rays = {_template_args(n, "ray_linear_jacobian_kernel"): f for n, f in k.items() if "ray_linear_jacobian_kernel" in n}
    # the head-and-tail kernel of one point per thread for 1..8 angles; 4 points per thread for 1 and 2 angles, 2 beyond
    assert sorted(column) == sorted([(1, na) for na in range(1, 9)] + [(4, 1), (4, 2)] + [(2, na) for na in range(3, 9)])
    # bundles of 4 rays, single rays, the tail: always 4 points per thread on the body (lbl_ray_radiance_linear_dev's groups)
    assert sorted(rays) == [(1, 1), (4, 1), (4, 4)]
    for args, f in list(column.items()) + list(rays.items()):
        print(args, f["VGPRs"], f.get("AGPRs"), f["Occupancy [waves/SIMD]"], f.get("LDS Size [bytes/block]"))
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (args, f)
    for args, f in rays.items():
        assert f.get("LDS Size [bytes/block]") == 0, (args, f)


# ---- the row layout ----------------------------------------------------------------------------------------------------------
def layout(rays, terms=()):
    """per ray 2 + c + 2 s + m rows: c distinct layers, s segments that are no markers, m terms in a crossed layer"""
    first = [0]
    for lay in rays:
        crossed = set(lay) - {MARKER}
        first.append(first[-1] + 2 + len(crossed) + 2 * sum(1 for l in lay if l != MARKER) + sum(1 for l in terms if l in crossed))
    return first


def rows_of(rays, terms=(), n_layers=4, **kw):
    ray_first = np.cumsum([0] + [len(r) for r in rays])
    return _native.ray_jacobian_rows(n_layers, ray_first, [l for r in rays for l in r], terms, **kw)


def test_rows_of_linear_rays():
    mirror = [3, 2, 1, 0, MARKER, 0, 1, 2, 3]                # four distinct layers, eight segments: 2 + 4 + 16
    first, rows = rows_of([mirror], linear=True)
    assert list(first) == [0, 22] and rows == 22
    first, rows = rows_of([[MARKER]], linear=True)           # a marker alone: dI/dT_source and dI/de
    assert list(first) == [0, 2] and rows == 2
    first, rows = rows_of([[]], linear=True)
    assert list(first) == [0, 2] and rows == 2
    first, rows = rows_of([[1, 1, 0, 1]], linear=True)       # a layer crossed three times: one ln tau row, six temperature rows
    assert list(first) == [0, 2 + 2 + 8] and rows == 12
    rays = [mirror, [MARKER], [], [0, 1, 2, 3], [MARKER, MARKER], [2, 1, MARKER, 1], [1, 0, MARKER, 0, MARKER, 0, 1]]
    first, rows = rows_of(rays, linear=True)
    assert list(first) == layout(rays) == [0, 22, 24, 26, 40, 42, 52, 66] and rows == 66
    terms = [0, 0, 1, 3, 3, 2, 0]
    first, rows = rows_of(rays, terms, linear=True)
    assert list(first) == layout(rays, terms) and rows == layout(rays, terms)[-1]
    # against the surface layout: c temperature rows give way to 2 s
    a, b = rows_of(rays, terms, surface=True), rows_of(rays, terms, linear=True)
    extra = [2 * sum(1 for l in r if l != MARKER) - len(set(r) - {MARKER}) for r in rays]
    assert list(np.diff(b[0]) - np.diff(a[0])) == extra
    for bad in ([0, -2, 1], [0, 4, 1]):
        with pytest.raises(_native.LblError) as err:
            rows_of([bad], linear=True)
        assert err.value.code == BAD_ARG
    with pytest.raises(_native.LblError) as err:
        rows_of([[0, 1]], [4], linear=True)
    assert err.value.code == BAD_ARG


# ---- the model: validation before any device work ----------------------------------------------------------------------------
def _atmosphere(layers=LAYERS):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("linear jacobians")
    for depth, T, P in layers:
        atm.addLayer(depth, T, P, 600, 610)
    return atm


@pytest.fixture()
def no_context(monkeypatch):
    """every check below must fail before the engine (and with it a device context) is asked for"""
    def refuse():
        raise AssertionError("the context was touched before the arguments were validated")
    monkeypatch.setattr(model, "_ctx", refuse)
    settings.set_resolution_multiplier(1)
    yield


def test_validation_before_any_device_work(no_context):
    atm = _atmosphere()
    n = len(atm[0].xAxis)
    lev = [295.0, 280.0, 255.0, 230.0, 212.0]
    plain, warm = atm.nadirPath(), atm.nadirPath(levelTemperatures=lev)
    mirror = atm.reflectedPath(levelTemperatures=lev)
    ins = model.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    for bad in (lev[:4], lev + [200.0], [295.0, 280.0, 255.0, 230.0, 0.0], [295.0, 280.0, 255.0, -230.0, 212.0],
                [295.0, 280.0, float("inf"), 230.0, 212.0], [295.0, 280.0, 255.0, 230.0, float("nan")], "warm", 250.0, False):
        with pytest.raises(ValueError, match="levelTemperatures"):
            atm.jacobiansLinear(surfaceTemperature=288, levelTemperatures=bad)
        with pytest.raises(ValueError, match="levelTemperatures"):
            atm.jacobiansLinear(surfaceTemperature=288, emissivity=0.9, levelTemperatures=bad)
        with pytest.raises(ValueError, match="levelTemperatures"):
            atm.observeLinear(ins, surfaceTemperature=288, levelTemperatures=bad)
    cold = _atmosphere([(1e4, 100.0, 500.0), (1e4, 400.0, 300.0)])      # default levels that come out <= 0
    with pytest.raises(ValueError, match="levelTemperatures"):
        cold.jacobiansLinear(surfaceTemperature=288)
    with pytest.raises(ValueError, match="levelTemperatures"):
        cold.observeLinear(ins, surfaceTemperature=288)
    # every path must carry temperatures; the first that does not is named
    with pytest.raises(ValueError, match="path 0"):
        atm.pathJacobiansLinear(plain, surfaceTemperature=288)
    with pytest.raises(ValueError, match="path 2"):
        atm.pathJacobiansLinear([warm, warm, plain, plain], surfaceTemperature=288)
    with pytest.raises(ValueError, match="temperatures"):
        atm.pathJacobiansLinear([warm, atm.limbPath(1.5e4)], surfaceTemperature=288)
    # a bounce without an emissivity
    with pytest.raises(ValueError, match="bounce"):
        atm.pathJacobiansLinear(mirror, surfaceTemperature=288)
    with pytest.raises(ValueError, match="bounce"):
        atm.pathJacobiansLinear([warm, mirror], surfaceTemperature=288, reflection="specular")
    # a path from the surface under the diffuse reflection
    for paths in (warm, [mirror, warm]):
        with pytest.raises(ValueError, match="lambertian"):
            atm.pathJacobiansLinear(paths, surfaceTemperature=288, emissivity=0.9)
        with pytest.raises(ValueError, match="lambertian"):
            atm.pathJacobiansLinear(paths, surfaceTemperature=288, emissivity=0.9, reflection="lambertian")
    # what the layer-source methods refuse, these refuse too
    for e in (-0.01, 1.5, float("nan"), "water", np.full(n - 1, 0.9)):
        with pytest.raises(ValueError, match="emissivity"):
            atm.jacobiansLinear(surfaceTemperature=288, emissivity=e)
        with pytest.raises(ValueError, match="emissivity"):
            atm.pathJacobiansLinear(mirror, surfaceTemperature=288, emissivity=e, reflection="specular")
        with pytest.raises(ValueError, match="emissivity"):
            atm.observeLinear(ins, surfaceTemperature=288, emissivity=e)
    for r in ("mirror", 0, None):
        with pytest.raises(ValueError, match="reflection"):
            atm.jacobiansLinear(surfaceTemperature=288, emissivity=0.9, reflection=r)
        with pytest.raises(ValueError, match="reflection"):
            atm.pathJacobiansLinear(mirror, surfaceTemperature=288, emissivity=0.9, reflection=r)
    with pytest.raises(ValueError, match="topSpectrum"):
        atm.jacobiansLinear(surfaceTemperature=288, topSpectrum=np.zeros(n))
    with pytest.raises(ValueError, match="topSpectrum"):
        atm.jacobiansLinear(surfaceTemperature=288, emissivity=0.9, topSpectrum=np.zeros(n - 1))
    with pytest.raises(ValueError, match="angles"):
        atm.jacobiansLinear(surfaceTemperature=288, angles=[(0.5, 0.0)])
    with pytest.raises(ValueError, match="surface"):
        atm.jacobiansLinear()
    with pytest.raises(ValueError, match="surface"):
        atm.pathJacobiansLinear(mirror, emissivity=0.9)
    with pytest.raises(ValueError, match="temperature"):
        atm.jacobiansLinear(surfaceTemperature=288, temperature="all")
    with pytest.raises(ValueError, match="temperature"):
        atm.pathJacobiansLinear(warm, surfaceTemperature=288, temperature="all")
    with pytest.raises(ValueError, match="mu"):
        atm.observeLinear(ins, surfaceTemperature=288, mu=0.0)
    with pytest.raises(ValueError, match="instrument"):
        atm.observeLinear("iasi", surfaceTemperature=288)
    with pytest.raises(ValueError, match="instrument"):
        atm.pathJacobiansLinear(warm, surfaceTemperature=288, instrument="iasi")
    with pytest.raises(ValueError, match="paths"):
        atm.pathJacobiansLinear([], surfaceTemperature=288)
    # valid calls get as far as the context
    with pytest.raises(AssertionError, match="context"):
        atm.jacobiansLinear(surfaceTemperature=288, levelTemperatures=lev)
    with pytest.raises(AssertionError, match="context"):
        atm.jacobiansLinear(surfaceTemperature=288, emissivity=0.9, reflection="specular", topSpectrum=np.zeros(n))
    with pytest.raises(AssertionError, match="context"):
        atm.pathJacobiansLinear([warm, mirror], surfaceTemperature=288, emissivity=0.9, reflection="specular")
    with pytest.raises(AssertionError, match="context"):
        atm.pathJacobiansLinear([mirror, atm.zenithPath(levelTemperatures=lev)], surfaceTemperature=288, emissivity=0.9)
    with pytest.raises(AssertionError, match="context"):
        atm.pathJacobiansLinear(warm, surfaceTemperature=288)
    with pytest.raises(AssertionError, match="context"):
        atm.observeLinear(ins, surfaceTemperature=288, jacobians=True, levelTemperatures=lev)


def test_level_chain_matrix(no_context):
    for layers in (LAYERS, [(1e4, 250.0, 500.0)], [(1e4, 290.0, 500.0), (3e4, 240.0, 200.0)],
                   [(1e4, T, 500.0) for T in (290.0, 270.0, 240.0)]):
        atm = _atmosphere(layers)
        L = len(layers)
        M = atm._level_chain()
        assert M.shape == (L + 1, L)
        T = np.array([l[1] for l in layers], dtype=np.float64)
        np.testing.assert_allclose(M @ T, atm.levelTemperatures(), rtol=1e-15)
        assert np.allclose(M.sum(axis=1), 1.0, rtol=0, atol=1e-15)       # a uniform shift of the layers shifts every level
        for l in range(L):                                                # the map is linear: a difference is its column
            up = [(d, t + (1.0 if i == l else 0.0), p) for i, (d, t, p) in enumerate(layers)]
            dn = [(d, t - (1.0 if i == l else 0.0), p) for i, (d, t, p) in enumerate(layers)]
            fd = (_atmosphere(up).levelTemperatures() - _atmosphere(dn).levelTemperatures()) / 2.0
            np.testing.assert_allclose(M[:, l], fd, rtol=0, atol=1e-12)


def test_levels_of_edges():
    edge = np.arange(24.0).reshape(3, 4, 2)                              # (bands, L, 2)
    lev = model.Atmosphere._levels_of_edges(edge)
    assert lev.shape == (3, 5)
    assert np.array_equal(lev[:, 0], edge[:, 0, 0]) and np.array_equal(lev[:, 4], edge[:, 3, 1])
    assert np.array_equal(lev[:, 1:4], edge[:, :3, 1] + edge[:, 1:, 0])


def test_result_objects_without_the_new_fields_behave_as_before():
    j = model.Jacobians(1.0, 2.0, np.zeros(2), np.zeros(2), None, [], [1.0], [1.0], temperatureAbsorption=np.ones(2))
    assert j.edgeTemperature is None and j.levelTemperature is None and j.levelTemperatureSpectrum is None
    assert np.array_equal(j.temperatureFull, np.ones(2))
    j = model.Jacobians(1.0, 2.0, None, np.zeros(2), None, [], [1.0], [1.0], temperatureAbsorption=np.ones(2),
                        edgeTemperature=np.ones((2, 2)), levelTemperature=np.ones(3), levelTemperatureSpectrum=np.ones((3, 5)))
    assert j.temperatureFull is None and j.edgeTemperature.shape == (2, 2) and j.levelTemperature.shape == (3,)
    assert "layers=2" in repr(j)
    p = model.PathJacobians(np.ones(3), np.ones((1, 3)), np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), None, None, [], [],
                            temperatureAbsorption=np.ones((1, 2, 3)))
    assert p.segmentTemperature is None and np.array_equal(p.temperatureFull, np.ones((1, 2, 3)))
    assert "layers=2" in repr(p)
    x = np.array([650.0, 660.0, 670.0])
    p = model.PathJacobians(x, np.full((1, 3), 0.1), np.full((1, 2, 3), 1e-3), np.zeros((1, 2, 3)), None, None, [], [], channels=True)
    assert p.brightnessTemperatureJacobian.shape == (1, 2, 3)
    p = model.PathJacobians(x, np.full((1, 3), 0.1), None, np.zeros((1, 2, 3)), None, None, [], [], channels=True,
                            segmentTemperature=[np.zeros((4, 2, 3))])
    assert p.temperature is None and p.temperatureFull is None and p.brightnessTemperatureJacobian is None
    assert p.brightnessTemperature.shape == (1, 3) and "layers=2" in repr(p)
    o = model.Observation(np.array([650.0]), np.array([0.1]), 1.0, temperatureJacobian=np.array([[0.2]]),
                          opticalDepthJacobian=np.array([[0.1]]))
    assert o.levelTemperatureJacobian is None and o.brightnessTemperatureJacobian is not None and "jacobians=True" in repr(o)
    assert "jacobians=False" in repr(model.Observation(np.array([650.0]), np.array([0.1]), 1.0))
    o = model.Observation(np.array([650.0]), np.array([0.1]), 1.0, opticalDepthJacobian=np.array([[0.1]]),
                          levelTemperatureJacobian=np.array([[0.2], [0.3]]))
    assert o.temperatureJacobian is None and o.brightnessTemperatureJacobian is None and o.levelTemperatureJacobian.shape == (2, 1)


def test_the_layer_source_methods_point_to_the_new_ones():
    import inspect
    for old, new in (("jacobians", "jacobiansLinear"), ("pathJacobians", "pathJacobiansLinear"), ("observe", "observeLinear")):
        a, b = getattr(model.Atmosphere, old), getattr(model.Atmosphere, new)
        assert "planck" not in inspect.signature(a).parameters and "layer source" in a.__doc__ and new in a.__doc__
        pa, pb = list(inspect.signature(a).parameters), list(inspect.signature(b).parameters)
        assert pb[:len(pa)] == pa and set(pb[len(pa):]) <= {"levelTemperatures"}, (old, pb)
