"""GPU: Jacobians of the linear-in-optical-depth Planck source - Atmosphere.jacobiansLinear, pathJacobiansLinear and
observeLinear (lbl_column_jacobian_linear_dev, lbl_ray_jacobian_linear_dev, kernels K5j) - against the NumPy restatements of
tests/test_linear_jacobian_cpu.py, for their identity with the layer source's Jacobians at equal temperatures, against
finite differences through the public forward calls, in their physical limits, for the identities between the three
products, and for independence of the rays, determinism, the chunks, laziness and the C ABI's refusals.

Tolerances are K5d's and K5h's, imported: bands rel 1e-9 + FLOOR x olr (check), spectra 1e-9 + 1e-11 x scale
(spectra_close), finite differences 1e-6 + 1e-10 x olr.  The clamped identity is K5h's with the step's whole emission in it,
so its floor is derived as there.  Column, lines, rays and synthetic coefficients are the earlier tests'."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyrad_oracle as orc
from test_gpu_jacobian import FLOOR, check
from test_gpu_linear_source import (LEVELS, linear_rays, model_columns, run_raw_flux, run_raw_rays, spectral_emissivity,
                                    with_temperatures)
from test_gpu_paths import LAYERS, column, ctx, lines, pyrad, synthetic_k  # noqa: F401
from test_gpu_surface import marked_rays
from test_gpu_surface_jacobian import run_raw_jac, run_raw_ray_jac, spectra_close
from test_jacobian_cpu import planck_dT
from test_linear_jacobian_cpu import MARKER, linear_jacobian_reference, linear_path_jacobian_reference

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
REFLECTIONS = ("lambertian", "specular")
RNG = (600, 610.07)   # about 1,000 points at multiplier 1, with a tail that is no multiple of 4


# ---- the raw ABI on uploaded synthetic coefficients ---------------------------------------------------------------------
def run_raw_lin_jac(ctx, k, edges, depth, mu, w, e, reflection, lo=600.0, hi=700.0, source_T=0.0, I_source=None, top=None,
                    bands=None, terms=(), spectra=True):
    """lbl_column_jacobian_linear_dev: (band values [band, 3 + 3 L + terms], ln tau spectra, T_edge spectra, e spectrum);
    edges: (bottom, top) per layer; terms: (layer, k_m) pairs.  jac is NaN beforehand."""
    L, n = k.shape
    first, count = ([0], [n]) if bands is None else ([a for a, _ in bands], [b - a for a, b in bands])
    nb, nv = len(first), 3 + 3 * L + len(terms)
    bufs = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    tb = [ctx.buffer(n).upload(km) for _, km in terms]
    jac, st, sT, se = ctx.buffer(nb * nv), ctx.buffer(max(L * n, 1)), ctx.buffer(max(2 * L * n, 1)), ctx.buffer(n)
    extra = []
    try:
        src = eb = pb = None
        if I_source is not None:
            src = ctx.buffer(n).upload(I_source); extra.append(src)
        if np.ndim(e):
            eb = ctx.buffer(n).upload(e); extra.append(eb)
        if top is not None:
            pb = ctx.buffer(n).upload(top); extra.append(pb)
        jac.upload(np.full(nb * nv, np.nan))
        ctx.column_jacobian_linear_dev(bufs, edges, depth, lo, hi, n, mu, w, first, count, jac, eb if eb is not None else e,
                                       reflection=REFLECTIONS.index(reflection), I_surface=src, surface_T=source_T, I_top=pb,
                                       term_abs_coef=tb, term_layer=[l for l, _ in terms],
                                       ln_tau_spectra=st if spectra else None, T_edge_spectra=sT if spectra else None,
                                       e_spectrum=se if spectra else None)
        v = jac.download(nb * nv).reshape(nb, nv)
        if not spectra:
            return v, None, None, None
        return v, st.download(L * n).reshape(L, n), sT.download(2 * L * n).reshape(2 * L, n), se.download(n)
    finally:
        for b in bufs + tb + [jac, st, sT, se] + extra:
            b.free()


def check_raw_lin_jac(ctx, k, edges, depth, mu, w, e, reflection, lo=600.0, hi=700.0, source_T=0.0, I_source=None, top=None,
                      bands=None, terms=()):
    L, n = k.shape
    x = np.linspace(lo, hi, n)
    v, st, sT, se = run_raw_lin_jac(ctx, k, edges, depth, mu, w, e, reflection, lo, hi, source_T, I_source, top, bands, terms)
    assert not np.isnan(v).any()
    ref = linear_jacobian_reference(x, list(k), edges, depth, mu, w, e, reflection, surface_T=source_T or None,
                                    surface=I_source, top=top, terms=terms, idx=bands)
    olr = ref["olr"]
    check(v[:, 0], olr, olr, rel=1e-12, what="olr")
    # F is lbl_column_flux_linear_dev's upward flux at the top (to rounding: the calls group a thread's points differently)
    sums = run_raw_flux(ctx, list(k), edges, depth, mu, w, e, reflection, lo, hi, source_T, I_source, top, bands)[0]
    check(v[:, 0], sums[:, 0, L], olr, rel=1e-12, what="F against the forward call")
    check(v[:, 1], ref["surfaceTemperature"], olr, what="T_s")
    check(v[:, 2], ref["emissivity"], olr, what="e")
    check(v[:, 3:3 + L], ref["opticalDepth"], olr, what="ln tau")
    check(v[:, 3 + L:3 + 3 * L], ref["edgeTemperature"], olr, what="T edge")
    if terms:
        check(v[:, 3 + 3 * L:], ref["terms"], olr, what="terms")
    inside = np.ones(n, dtype=bool)
    if bands is not None:                        # (points outside every band keep 0 in the spectra)
        inside[:] = False
        for a, b in bands:
            inside[a:b] = True
    scale = max(np.max(np.abs(np.where(inside, ref["olrSpectrum"], 0.0))), 1e-300)
    tag = "%s L=%d n=%d angles=%d" % (reflection, L, n, len(mu))
    spectra_close(st, np.where(inside, ref["opticalDepthSpectrum"], 0.0), scale, tag + " ln tau")
    spectra_close(sT, np.where(inside, ref["edgeTemperatureSpectrum"], 0.0), scale, tag + " T edge")
    spectra_close(se, np.where(inside, ref["emissivitySpectrum"], 0.0), scale, tag + " e")
    # without the spectra: the same band values
    assert np.array_equal(v, run_raw_lin_jac(ctx, k, edges, depth, mu, w, e, reflection, lo, hi, source_T, I_source, top, bands,
                                             terms, spectra=False)[0])
    return v


def random_edges(rs, L):
    return [tuple(p) for p in rs.uniform(205.0, 300.0, (L, 2))]


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 5003])
def test_raw_column_sizes(ctx, pyrad, n):
    rs = np.random.RandomState(700 + n)
    for L, angles in ((1, 3), (4, 1), (4, 8)):
        k = synthetic_k(rs, L, n)
        edges = random_edges(rs, L)
        depth = list(rs.uniform(0.5e4, 2e4, L))
        mu, w = pyrad.fluxAngles(angles)
        e = rs.uniform(0.3, 1.0, n)
        e[::7] = 1.0
        e[3::11] = 0.0
        terms = [(l, rs.uniform(0.0, 1.0, n) * k[l]) for l in range(L)] + [(0, k[0])]
        bands = None if n < 1027 else [(1, 515), (515, 516), (518, n)]     # off the groups of four, and a single point
        for reflection in REFLECTIONS:
            check_raw_lin_jac(ctx, k, edges, depth, mu, w, e, reflection, source_T=295.0, top=rs.uniform(0.0, 0.2, n),
                              bands=bands, terms=terms)
        check_raw_lin_jac(ctx, k, edges, depth, mu, w, 0.7, "lambertian", I_source=rs.uniform(0.0, 0.2, n))
        check_raw_lin_jac(ctx, k, edges, depth, mu, w, 1.0, "specular", source_T=295.0, terms=terms[:1])    # the black surface


def test_raw_column_128_layers_eight_angles(ctx, pyrad):
    rs = np.random.RandomState(737)
    L, n = 128, 1027
    k = synthetic_k(rs, L, n, tau_lo=-6.0, tau_hi=-5.0, huge=0.002)
    lev = np.linspace(292.0, 178.0, L + 1) + rs.uniform(-0.4, 0.4, L + 1)
    edges = list(zip(lev[:-1], lev[1:]))
    depth = list(rs.uniform(0.5e4, 1e4, L))
    mu, w = pyrad.fluxAngles(8)
    e = rs.uniform(0.3, 1.0, n)
    for reflection in REFLECTIONS:
        check_raw_lin_jac(ctx, k, edges, depth, mu, w, e, reflection, source_T=300.0, top=rs.uniform(0.0, 0.1, n),
                          terms=[(0, k[0]), (127, k[127]), (64, 0.5 * k[64])])


def test_column_calls_repeat_bit_for_bit(ctx, pyrad):
    rs = np.random.RandomState(741)
    L, n = 4, 5003
    k = synthetic_k(rs, L, n)
    edges, depth = random_edges(rs, L), list(rs.uniform(0.5e4, 2e4, L))
    mu, w = pyrad.fluxAngles(3)
    kw = dict(source_T=290.0, top=rs.uniform(0.0, 0.1, n), terms=[(1, 0.5 * k[1])], bands=[(3, 2001), (2001, n)])
    e = rs.uniform(0.3, 1.0, n)
    a = run_raw_lin_jac(ctx, k, edges, depth, mu, w, e, "lambertian", **kw)
    b = run_raw_lin_jac(ctx, k, edges, depth, mu, w, e, "lambertian", **kw)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


# ---- rays through the raw ABI ------------------------------------------------------------------------------------------------
def run_raw_lin_ray_jac(ctx, k, rays, e=1.0, lo=600.0, hi=700.0, I_source=None, source_T=0.0, terms=()):
    """rays: [(layers, lengths, kind, temps)] -> (radiance R x n, rows x n, row_first); terms: (layer, k_m) pairs"""
    from pyrad_amd import _native
    L, n = k.shape
    ray_first = np.cumsum([0] + [len(r[0]) for r in rays])
    seg_layer = [l for r in rays for l in r[0]]
    row_first, rows = _native.ray_jacobian_rows(L, ray_first, seg_layer, [l for l, _ in terms], linear=True)
    bufs = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    tb = [ctx.buffer(n).upload(km) for _, km in terms]
    rad, jac = ctx.buffer(len(rays) * n), ctx.buffer(rows * n)
    extra = []
    try:
        src = eb = None
        if I_source is not None:
            src = ctx.buffer(n).upload(I_source); extra.append(src)
        if np.ndim(e):
            eb = ctx.buffer(n).upload(e); extra.append(eb)
        jac.upload(np.full(rows * n, np.nan))               # nothing is zeroed beforehand: every value must be written
        ctx.ray_jacobian_linear_dev(bufs, [t for r in rays for pair in r[3] for t in pair], lo, hi, n, ray_first, seg_layer,
                                    [s for r in rays for s in r[1]], [r[2] for r in rays], jac, eb if eb is not None else e,
                                    I_source=src, source_T=source_T, term_abs_coef=tb, term_layer=[l for l, _ in terms],
                                    radiance=rad)
        return rad.download().reshape(len(rays), n), jac.download().reshape(rows, n), row_first
    finally:
        for b in bufs + tb + [rad, jac] + extra:
            b.free()


def wanted_rows(ref):
    crossed = sorted(ref["opticalDepth"])
    return [ref["sourceTemperature"], ref["emissivity"]] + [ref["opticalDepth"][l] for l in crossed] \
        + [row for pair in ref["segmentTemperature"] for row in pair] + [ref["terms"][m] for m in sorted(ref["terms"])]


def check_raw_lin_ray_jac(ctx, k, rays, e=1.0, lo=600.0, hi=700.0, I_source=None, source_T=0.0, terms=()):
    L, n = k.shape
    x = np.linspace(lo, hi, n)
    I, J, first = run_raw_lin_ray_jac(ctx, k, rays, e, lo, hi, I_source, source_T, terms)
    # the radiance is lbl_ray_radiance_linear_dev's, bit for bit: the same step on the same groups of points
    assert np.array_equal(I, run_raw_rays(ctx, list(k), rays, e, lo, hi, I_source, source_T)[0])
    assert not np.isnan(J).any()
    Ts = None if I_source is not None or not source_T > 0 else source_T
    worst = 0.0
    for r, (layers, lengths, kind, temps) in enumerate(rays):
        ref = linear_path_jacobian_reference(x, list(k), layers, lengths, temps, kind, e, surface_T=Ts, surface=I_source,
                                             terms=terms)
        want = wanted_rows(ref)
        assert first[r + 1] - first[r] == len(want), r
        got = J[first[r]:first[r + 1]]
        scale = max(np.max(np.abs(ref["radiance"])), np.max(np.abs(I_source)) if I_source is not None else 0.0, 1e-300)
        # (a segment's temperature rows scale with dB/dT of its own temperatures, whatever reaches the observer)
        err = np.abs(got - np.array(want))
        bound = 1e-9 * np.abs(np.array(want)) + 1e-11 * scale
        worst = max(worst, np.max(err / bound))
        assert np.all(err <= bound), (r, layers, np.max(err / bound))
        if kind == 0 and MARKER not in layers:
            assert np.all(got[0] == 0.0) and np.all(got[1] == 0.0), r
    print("n = %d, %d rays: worst error / bound %.2e" % (n, len(rays), worst))
    return I, J


def marked_linear_rays(rs, L):
    """tests/test_gpu_surface.py's marked rays, each segment with random temperatures (a marker's pair is ignored)"""
    return [(lay, lens, kind, [(0.0, 0.0) if l == MARKER else tuple(rs.uniform(200.0, 310.0, 2)) for l in lay])
            for lay, lens, kind in marked_rays(rs, L)]


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 5003])
def test_raw_rays_sizes(ctx, n):
    rs = np.random.RandomState(800 + n)
    L = 3
    k = synthetic_k(rs, L, n)
    e = rs.uniform(0.5, 1.0, n)
    e[::7] = 1.0
    e[3::11] = 0.0
    terms = [(l, rs.uniform(0.0, 1.0, n) * k[l]) for l in range(L)] + [(1, k[1])]
    rays = linear_rays(rs, L)                  # bundles by layers AND temperatures, markers, marker-only rays
    check_raw_lin_ray_jac(ctx, k, rays, 0.8, source_T=295.0)
    check_raw_lin_ray_jac(ctx, k, rays, e, source_T=295.0, terms=terms)
    check_raw_lin_ray_jac(ctx, k, rays, e, I_source=rs.uniform(0.0, 0.2, n), terms=terms[:1])
    if n in (4, 1027):
        check_raw_lin_ray_jac(ctx, k, marked_linear_rays(rs, L), e, source_T=295.0, terms=terms)
        # the black surface: no marker, the default emissivity
        black = [r for r in rays if MARKER not in r[0]]
        check_raw_lin_ray_jac(ctx, k, black, source_T=295.0, terms=terms)


def test_raw_rays_128_layers_down_and_up(ctx):
    rs = np.random.RandomState(817)
    L, n = 128, 1027
    k = synthetic_k(rs, L, n, tau_lo=-6.0, tau_hi=-5.0, huge=0.002)
    lev = np.linspace(292.0, 178.0, L + 1) + rs.uniform(-0.4, 0.4, L + 1)
    d = list(rs.uniform(0.5e4, 1e4, L))
    seq = list(range(L - 1, -1, -1)) + [MARKER] + list(range(L))
    lens = [d[l] for l in range(L - 1, -1, -1)] + [0.0] + d
    temps = [(lev[l + 1], lev[l]) for l in range(L - 1, -1, -1)] + [(0.0, 0.0)] + [(lev[l], lev[l + 1]) for l in range(L)]
    assert len(seq) == 257
    check_raw_lin_ray_jac(ctx, k, [(seq, lens, 0, temps), (seq, lens, 1, temps)], rs.uniform(0.3, 1.0, n), source_T=300.0)


def test_rays_are_independent_and_calls_deterministic(ctx):
    rs = np.random.RandomState(871)
    L, n = 3, 1027
    k = synthetic_k(rs, L, n)
    e = rs.uniform(0.3, 1.0, n)
    seq = [2, 1, 0, MARKER, 0, 1]
    temps = [tuple(p) for p in rs.uniform(200.0, 310.0, (3, 2))] + [(0.0, 0.0)] + [tuple(p) for p in rs.uniform(200.0, 310.0, (2, 2))]
    band = [(seq, list(rs.uniform(0.5e4, 2e4, 3)) + [0.0] + list(rs.uniform(0.5e4, 2e4, 2)), i % 2, temps) for i in range(6)]
    terms = [(0, 0.5 * k[0]), (2, k[2])]
    kw = dict(source_T=295.0, terms=terms)
    I, J, first = run_raw_lin_ray_jac(ctx, k, band, e, **kw)
    I2, J2, _ = run_raw_lin_ray_jac(ctx, k, band, e, **kw)
    assert np.array_equal(I, I2) and np.array_equal(J, J2)
    Ir, Jr, fr = run_raw_lin_ray_jac(ctx, k, band[::-1], e, **kw)
    per = first[1] - first[0]
    assert per == 2 + 3 + 2 * 5 + 2 and np.all(np.diff(first) == per)
    for r in range(6):
        alone = run_raw_lin_ray_jac(ctx, k, [band[r]], e, **kw)
        assert np.array_equal(alone[0][0], I[r]) and np.array_equal(alone[1], J[first[r]:first[r + 1]]), r
        assert np.array_equal(Ir[5 - r], I[r]) and np.array_equal(Jr[fr[5 - r]:fr[6 - r]], J[first[r]:first[r + 1]]), r


# ---- equal temperatures: the layer source's Jacobians ------------------------------------------------------------------------
@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_equal_edges_are_the_surface_jacobians(ctx, pyrad, reflection):
    rs = np.random.RandomState(905)
    L, n = 4, 1027
    k = synthetic_k(rs, L, n)
    T = [288.0, 262.0, 231.0, 214.0]
    depth = list(rs.uniform(0.5e4, 2e4, L))
    e, top = rs.uniform(0.3, 1.0, n), rs.uniform(0.0, 0.1, n)
    terms = [(l, rs.uniform(0.0, 1.0, n) * k[l]) for l in range(L)]
    for angles in (1, 3, 8):
        mu, w = pyrad.fluxAngles(angles)
        kw = dict(source_T=295.0, top=top, terms=terms, bands=[(2, 515), (515, n)])
        v, st, sT, se = run_raw_lin_jac(ctx, k, [(t, t) for t in T], depth, mu, w, e, reflection, **kw)
        s, sst, ssT, sse = run_raw_jac(ctx, k, T, depth, mu, w, e, reflection, **kw)
        olr = s[:, 0]
        check(v[:, 0], olr, olr, rel=1e-12, what="olr")
        check(v[:, 1:3 + L], s[:, 1:3 + L], olr, what="T_s, e, ln tau")
        check(v[:, 3 + 3 * L:], s[:, 3 + 2 * L:], olr, what="terms")
        # bottom plus top edge is dF/dT_l
        check(v[:, 3 + L:3 + 3 * L:2] + v[:, 4 + L:3 + 3 * L:2], s[:, 3 + L:3 + 2 * L], olr, what="T")
        scale = np.max(run_raw_flux(ctx, list(k), [(t, t) for t in T], depth, mu, w, e, reflection, source_T=295.0, top=top)[1])
        spectra_close(st, sst, scale, "ln tau")
        spectra_close(sT[0::2] + sT[1::2], ssT, scale, "T")
        spectra_close(se, sse, scale, "e")


def test_equal_segment_temperatures_are_the_surface_ray_jacobians(ctx):
    rs = np.random.RandomState(911)
    L, n = 3, 1027
    k = synthetic_k(rs, L, n)
    T = [288.0, 250.0, 215.0]
    e = rs.uniform(0.5, 1.0, n)
    terms = [(l, rs.uniform(0.0, 1.0, n) * k[l]) for l in range(L)]
    plain = marked_rays(rs, L)
    rays = [(lay, lens, kind, [(0.0, 0.0) if l == MARKER else (T[l], T[l]) for l in lay]) for lay, lens, kind in plain]
    I, J, first = run_raw_lin_ray_jac(ctx, k, rays, e, source_T=295.0, terms=terms)
    Is, Js, fs = run_raw_ray_jac(ctx, k, T, plain, e, source_T=295.0, terms=terms)
    assert np.array_equal(I, Is)                      # (g (Bb - Ba) adds +0 to the layer source's step)
    for r, (lay, _, _) in enumerate(plain):
        crossed = sorted(set(lay) - {MARKER})
        c, real = len(crossed), [l for l in lay if l != MARKER]
        a, b = J[first[r]:first[r + 1]], Js[fs[r]:fs[r + 1]]
        scale = max(np.max(np.abs(I[r])), 1e-300)
        spectra_close(a[:2 + c], b[:2 + c], scale, "%d T_s, e, ln tau" % r)
        spectra_close(a[2 + c + 2 * len(real):], b[2 + 2 * c:], scale, "%d terms" % r)
        seg = a[2 + c:2 + c + 2 * len(real)].reshape(len(real), 2, n)
        for i, l in enumerate(crossed):                # dTa + dTb summed over a layer's segments is dI/dT_l
            total = sum(seg[j, 0] + seg[j, 1] for j, ll in enumerate(real) if ll == l)
            spectra_close(total, b[2 + c + i], scale, "%d T %d" % (r, l))


# ---- finite differences through the public forward calls ----------------------------------------------------------------------
def default_levels(T, d):
    """Atmosphere.levelTemperatures(), restated"""
    L = len(T)
    lev = np.empty(L + 1)
    if L == 1:
        lev[:] = T[0]
        return lev
    for i in range(1, L):
        lev[i] = T[i - 1] + (T[i] - T[i - 1]) * d[i - 1] / (d[i - 1] + d[i])
    lev[0] = 2.0 * T[0] - lev[1]
    lev[L] = 2.0 * T[L - 1] - lev[L - 1]
    return lev


@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_finite_differences(pyrad, lines, reflection):
    from pyrad_amd import engine, settings
    atm = column(pyrad, rng=(600, 700))
    Ts, e0 = 288.0, 0.7
    mu, w = pyrad.fluxAngles(3)
    top = 0.3 * np.array(atm[0].planck(250))
    kw = dict(angles=3, topSpectrum=top, reflection=reflection, emissivity=e0, surfaceTemperature=Ts)
    j = atm.jacobiansLinear(levelTemperatures=LEVELS, **kw)
    olr = j.olr
    f0 = atm.fluxes(planck="linear", levelTemperatures=LEVELS, **kw)
    assert abs(olr - f0.up[-1]) <= 1e-13 * f0.up[-1]
    assert j.temperature is None and j.edgeTemperature.shape == (4, 2) and j.levelTemperature.shape == (5,)
    assert np.array_equal(j.levelTemperature, pyrad.Atmosphere._levels_of_edges(j.edgeTemperature))

    def near(a, fd, what):
        print("%s: analytic %.6e differences %.6e" % (what, a, fd))
        assert abs(a - fd) <= 1e-6 * abs(a) + 1e-10 * olr, (what, a, fd)

    def up(lev=LEVELS, **over):
        return atm.fluxes(planck="linear", levelTemperatures=lev, **dict(kw, **over)).up[-1]

    eps, h = 1e-4, 1e-2
    for i in range(5):
        lp, lm = LEVELS.copy(), LEVELS.copy()
        lp[i] += h
        lm[i] -= h
        near(j.levelTemperature[i], (up(lp) - up(lm)) / (2 * h), "level %d" % i)
    for l, L in enumerate(atm):
        d0 = L.depth
        L.changeDepth(d0 * np.exp(eps))
        fp = up()
        L.changeDepth(d0 * np.exp(-eps))
        fm = up()
        L.changeDepth(d0)
        near(j.opticalDepth[l], (fp - fm) / (2 * eps), "ln tau %d" % l)
    near(j.surfaceTemperature, (up(surfaceTemperature=Ts + h) - up(surfaceTemperature=Ts - h)) / (2 * h), "T_s")
    fd = (up(emissivity=e0 + 0.05) - up(emissivity=e0 - 0.05)) / 0.1
    assert abs(j.emissivity - fd) <= 1e-10 * olr
    # the default levels: .temperature is the chain through levelTemperatures() (the Planck part: the coefficients held,
    # the differences through the forward entry point)
    jd = atm.jacobiansLinear(**kw)
    assert jd.temperature.shape == (4,)
    assert np.allclose(jd.temperature, jd.levelTemperature @ atm._level_chain(), rtol=1e-14, atol=0)
    assert np.array_equal(atm.jacobiansLinear(levelTemperatures=True, **kw).temperature, jd.temperature)      # True: the default levels
    res = settings.BASE_RESOLUTION
    n = atm[0].xAxis.size
    ctx = engine.get_engine().ctx
    kb = [L.__dict__["_sweep_state"].bufs["abs_coef"] for L in atm]
    T, d = [float(L.T) for L in atm], [float(L.depth) for L in atm]
    assert np.array_equal(default_levels(T, d), atm.levelTemperatures())
    level, tb = ctx.buffer(2 * (len(atm) + 1)), ctx.buffer(n).upload(top)
    try:
        def flux_top(TT):
            lev = default_levels(TT, d)
            ctx.column_flux_linear_dev(kb, np.column_stack([lev[:-1], lev[1:]]), d, 600, 700, n, mu, w, [0], [n], level, e0,
                                       reflection=REFLECTIONS.index(reflection), surface_T=Ts, I_top=tb)
            return level.download(2 * (len(atm) + 1))[len(atm)] * res
        for l in range(len(atm)):
            Tp, Tm = list(T), list(T)
            Tp[l] += h
            Tm[l] -= h
            near(jd.temperature[l], (flux_top(Tp) - flux_top(Tm)) / (2 * h), "T %d" % l)
    finally:
        level.free()
        tb.free()


def test_black_surface_bands_and_molecules(pyrad, lines):
    """emissivity=None is the black surface: emissivity 1 without the dF/de fields; bands give a leading axis; the molecule
    terms add up to the layer's; at equal level temperatures the layer source's values come back"""
    atm = column(pyrad, rng=RNG)
    x = atm[0].xAxis
    n = x.size
    bands = [(x[0], x[301]), (x[301], np.inf)]
    a = atm.jacobiansLinear(surfaceTemperature=288, levelTemperatures=LEVELS, spectra=True, bands=bands)
    b = atm.jacobiansLinear(surfaceTemperature=288, levelTemperatures=LEVELS, spectra=True, bands=bands, emissivity=1.0)
    assert a.emissivity is None and a.emissivitySpectrum is None and b.emissivity.shape == (2,)
    for name in ("olr", "surfaceTemperature", "opticalDepth", "edgeTemperature", "levelTemperature", "opticalDepthSpectrum",
                 "levelTemperatureSpectrum"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.edgeTemperature.shape == (2, 4, 2) and a.levelTemperature.shape == (2, 5) and a.levelTemperatureSpectrum.shape == (5, n)
    assert a.temperatureSpectrum is None and len(a.molecules) == 4 and a.molecules[0].shape == (2, 2)
    from pyrad_amd import settings
    res = settings.BASE_RESOLUTION                    # the band values' factor, as fluxes() documents it
    whole = atm.jacobiansLinear(surfaceTemperature=288, levelTemperatures=LEVELS)
    check(a.levelTemperature.sum(axis=0), whole.levelTemperature, whole.olr, what="bands add up")
    check(res * np.sum(a.levelTemperatureSpectrum, axis=1), whole.levelTemperature, whole.olr, what="spectrum adds up")
    for l in range(4):
        check(a.molecules[l].sum(axis=-1), a.opticalDepth[:, l], a.olr, what="molecules add up to the layer")
    # with level temperatures equal to the layers' on both sides: the layer source's values
    iso = column(pyrad, rng=RNG, layers=tuple((d, 255, P) for d, _, P in LAYERS))
    f = iso.jacobiansLinear(surfaceTemperature=288)
    g = iso.jacobians(surfaceTemperature=288)
    check(f.opticalDepth, g.opticalDepth, g.olr, what="ln tau")
    check(f.edgeTemperature.sum(axis=-1), g.temperature, g.olr, what="edges add up to the layer")
    check(np.stack(f.molecules), np.stack(g.molecules), g.olr, what="molecules")
    assert f.temperatureAbsorption is None and f.temperatureFull is None
    # dk/dT needs the Voigt line shape here as in jacobians(): refused before the device is asked
    for call in (lambda: iso.jacobiansLinear(surfaceTemperature=288, temperature="full"),
                 lambda: iso.pathJacobiansLinear(iso.nadirPath(levelTemperatures=True), surfaceTemperature=288, temperature="full")):
        with pytest.raises(ValueError, match="voigt"):
            call()


def test_finite_differences_paths(pyrad, lines):
    atm = column(pyrad, rng=RNG)
    Ts, e0 = 295.0, 0.7
    paths = [atm.nadirPath(levelTemperatures=LEVELS), atm.reflectedPath(mu=0.6, levelTemperatures=LEVELS),
             atm.limbPath(2.5e4, levelTemperatures=LEVELS)]
    kw = dict(surfaceTemperature=Ts, emissivity=e0, reflection="specular")
    j = atm.pathJacobiansLinear(paths, **kw)
    want = atm.radiance(paths, planck="linear", **kw)
    assert np.array_equal(j.radiance, want.radiance)
    assert j.temperature is None and [s.shape[0] for s in j.segmentTemperature] == [len(p) for p in paths]
    h = 1e-2
    for r, p in enumerate(paths):
        rad = lambda q: atm.radiance(q, planck="linear", **kw).radiance[0]
        scale = np.max(j.radiance[r])
        for s in range(len(p)):
            for side in range(2):
                tp, tm = [list(t) for t in p.temperatures], [list(t) for t in p.temperatures]
                tp[s][side] += h
                tm[s][side] -= h
                fd = (rad(with_temperatures(p, tp, pyrad)) - rad(with_temperatures(p, tm, pyrad))) / (2 * h)
                assert np.all(np.abs(j.segmentTemperature[r][s, side] - fd) <= 1e-6 * np.abs(fd) + 1e-10 * scale), (r, s, side)
        # (Richardson, as tests/test_gpu_surface_jacobian.py: at a single grid point the third derivative is not small)
        eps = 2e-3
        for l in sorted(set(p.layers)):
            def central(step):
                qs = [pyrad.Path(p.layers, [x * np.exp(sg * step) if ll == l else x for ll, x in zip(p.layers, p.lengths)],
                                 source=p.source, bounce=p.bounce, temperatures=p.temperatures) for sg in (1, -1)]
                return (rad(qs[0]) - rad(qs[1])) / (2 * step)
            fd = (4 * central(eps / 2) - central(eps)) / 3
            assert np.all(np.abs(j.opticalDepth[r, l] - fd) <= 1e-6 * np.abs(fd) + 1e-10 * scale), (r, l)


# ---- physics that does not lean on the restatement -------------------------------------------------------------------------
def one_segment(ctx, k_value, length, Ta, Tb, n=1027):
    x = np.linspace(600.0, 700.0, n)
    I, J, first = run_raw_lin_ray_jac(ctx, np.full((1, n), k_value), [([0], [length], 0, [(Ta, Tb)])])
    assert list(first) == [0, 5]
    return x, J[3] / planck_dT(x, Ta), J[4] / planck_dT(x, Tb)


def test_opaque_layer(ctx):
    tau = 1e4
    x, a, b = one_segment(ctx, 1.0, tau, 280.0, 240.0)
    # g dB(Tb): t underflows, so g = 1 - 1 / tau, exactly 1e-4 away from dB(Tb) - that bound is met with equality, so the
    # comparison grants it the 1e-13 that the row is granted against NumPy's dB(Tb) in the first place
    assert np.all(np.abs(b - (1.0 - 1.0 / tau)) <= 1e-13) and np.all(b < 1.0) and np.all(np.abs(b - 1.0) <= 1e-4 + 1e-13)
    assert np.all((a >= 0.5 / tau) & (a <= 2.0 / tau)) and np.all(np.abs(a * tau - 1.0) <= 1e-12)  # h dB(Ta), of order 1 / tau


def test_thin_layer_reaches_the_series_and_tells_the_edges_apart(ctx):
    tau = 2.0 ** -10
    x, a, b = one_segment(ctx, 2.0 ** -20, 1024.0, 280.0, 240.0)
    # h = tau / 2 - tau^2 / 3 + tau^3 / 8 - ..., g = tau / 2 - tau^2 / 6 + tau^3 / 24 - ...: alternating, falling terms
    assert np.all(np.abs(a - (tau / 2 - tau ** 2 / 3)) <= tau ** 3 / 8 * (1 + 1e-9))
    assert np.all(np.abs(b - (tau / 2 - tau ** 2 / 6)) <= tau ** 3 / 24 * (1 + 1e-9))
    assert np.all(np.abs(a - tau / 2) <= tau ** 2) and np.all(np.abs(b - tau / 2) <= tau ** 2)
    assert tau ** 2 / 6 > 100 * tau ** 3 / 8               # swapped edges miss the first two bounds by far


@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_isothermal_cavity(pyrad, lines, reflection):
    atm = column(pyrad, rng=RNG)
    x = atm[0].xAxis
    B = orc.planckWavenumber(x, 260)
    for e in (0.0, 0.37, None, spectral_emissivity(x)):
        kw = dict(emissivity=e, topSpectrum=B) if e is not None else {}
        j = atm.jacobiansLinear(surfaceTemperature=260, levelTemperatures=[260.0] * 5, reflection=reflection, **kw)
        if e is None:                                  # the black surface sees no top spectrum: only the layers are isothermal
            continue
        print(reflection, np.ndim(e), np.max(np.abs(j.opticalDepth)) / j.olr, abs(j.emissivity) / j.olr)
        assert np.all(np.abs(j.opticalDepth) <= FLOOR * j.olr), j.opticalDepth
        assert np.all(np.abs(np.concatenate([np.ravel(m) for m in j.molecules])) <= FLOOR * j.olr)
        assert abs(j.emissivity) <= FLOOR * j.olr
    # over the black surface the layers above an isothermal column at the surface's temperature change nothing either
    j = atm.jacobiansLinear(surfaceTemperature=260, levelTemperatures=[260.0] * 5, reflection=reflection)
    assert np.all(np.abs(j.opticalDepth) <= FLOOR * j.olr), j.opticalDepth


# ---- identities between the three products ------------------------------------------------------------------------------------
def test_reflected_path_is_the_specular_column_and_observe(pyrad, lines):
    atm = column(pyrad, rng=RNG)
    x = atm[0].xAxis
    n, L = x.size, len(atm)
    step = x[1] - x[0]
    ins = pyrad.Instrument(x[5:-5:7], shape="boxcar", width=0.6 * step)          # a boxcar of one grid step: the point itself
    assert np.all(ins.support(RNG[0], RNG[1], n)[2] == 1)
    at = slice(5, n - 5, 7)
    for e in (0.6, spectral_emissivity(x)):
        for kw in (dict(surfaceTemperature=295), dict(surfaceSpectrum=atm[0].planck(300))):
            ray = atm.pathJacobiansLinear(atm.reflectedPath(levelTemperatures=True), emissivity=e, **kw)
            col = atm.jacobiansLinear(emissivity=e, reflection="specular", angles=[(1.0, 1.0)], spectra=True, molecules=False, **kw)
            scale = np.max(ray.radiance[0])
            spectra_close(ray.opticalDepth[0], col.opticalDepthSpectrum, scale, "ln tau")
            spectra_close(ray.emissivity[0], col.emissivitySpectrum, scale, "e")
            # the path goes down through layers L-1 .. 0 (entry: the upper level) and up through 0 .. L-1 (entry: the lower)
            seg = ray.segmentTemperature[0]
            assert seg.shape == (2 * L, 2, n)
            lev = np.zeros((L + 1, n))
            for s in range(L):
                l = L - 1 - s
                lev[l + 1] += seg[s, 0]
                lev[l] += seg[s, 1]
                lev[s] += seg[L + s, 0]
                lev[s + 1] += seg[L + s, 1]
            spectra_close(lev, col.levelTemperatureSpectrum, scale, "levels")
            ob = atm.observeLinear(ins, emissivity=e, jacobians=True, **kw)
            flux = atm.fluxes(emissivity=e, reflection="specular", angles=[(1.0, 1.0)], spectra=True, planck="linear", **kw)
            spectra_close(ob.radiance, flux.upSpectrum[at], scale, "observe radiance")
            assert np.array_equal(ob.radiance, atm.observeLinear(ins, emissivity=e, **kw).radiance)
            assert ob.temperatureJacobian is None and ob.levelTemperatureJacobian.shape == (L + 1, len(ins))
            spectra_close(ob.opticalDepthJacobian, col.opticalDepthSpectrum[:, at], scale, "observe ln tau")
            spectra_close(ob.levelTemperatureJacobian, col.levelTemperatureSpectrum[:, at], scale, "observe levels")
            spectra_close(ob.emissivityJacobian, col.emissivitySpectrum[at], scale, "observe e")
    # a wider instrument, given levels, the black surface: the radiance is the convolved linear-source spectrum
    wide = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    for mu in (1.0, 0.55):
        for kw in (dict(), dict(emissivity=0.8)):
            ob = atm.observeLinear(wide, surfaceTemperature=295, mu=mu, levelTemperatures=LEVELS, jacobians=True, **kw)
            flux = atm.fluxes(surfaceTemperature=295, angles=[(mu, 1.0)], spectra=True, planck="linear", levelTemperatures=LEVELS,
                              reflection="specular", **kw)
            assert np.array_equal(ob.radiance, pyrad.convolve(wide, flux.upSpectrum, *RNG))
            assert (ob.emissivityJacobian is None) == (not kw)
            col = atm.jacobiansLinear(surfaceTemperature=295, angles=[(mu, 1.0)], spectra=True, molecules=False,
                                      levelTemperatures=LEVELS, reflection="specular", **kw)
            scale = np.max(ob.radiance)
            spectra_close(ob.levelTemperatureJacobian, pyrad.convolve(wide, col.levelTemperatureSpectrum, *RNG), scale, "levels")
            spectra_close(ob.opticalDepthJacobian, pyrad.convolve(wide, col.opticalDepthSpectrum, *RNG), scale, "ln tau")


def test_paths_against_numpy_and_chunks(pyrad, lines):
    """the model's rows -> arrays mapping, with molecules, over chunks of 512 rows, and through an instrument"""
    atm = column(pyrad, rng=RNG)
    x, k, T, depth = model_columns(pyrad, atm)
    terms = [(l, np.array(m.absCoef)) for l, L in enumerate(atm) for m in L]
    rs = np.random.RandomState(3)
    bent = pyrad.Path([1, 0, 0, 2], [3e4, 2e4, 1e4, 7e3], source="surface", bounce=2,
                      temperatures=[tuple(p) for p in rs.uniform(210.0, 300.0, (4, 2))])
    paths = [atm.reflectedPath(levelTemperatures=LEVELS), atm.reflectedPath(mu=0.4, observerLevel=2, levelTemperatures=True),
             atm.zenithPath(levelTemperatures=LEVELS), atm.nadirPath(levelTemperatures=LEVELS),
             pyrad.Path([], [], source="space", bounce=0, temperatures=[]), atm.limbPath(2.5e4, levelTemperatures=LEVELS), bent]
    e = spectral_emissivity(x)
    got = atm.pathJacobiansLinear(paths, surfaceTemperature=295, molecules=True, emissivity=e, reflection="specular")
    want = atm.radiance(paths, surfaceTemperature=295, emissivity=e, reflection="specular", planck="linear")
    assert np.array_equal(got.radiance, want.radiance)
    assert got.temperature is None and got.temperatureFull is None
    for r, p in enumerate(paths):
        lay, lens = p._segments()
        ref = linear_path_jacobian_reference(x, k, lay, lens, p._segment_temperatures(), 1 if p.source == "surface" else 0, e,
                                             surface_T=295, terms=terms)
        scale = max(np.max(np.abs(ref["radiance"])), 1e-300)
        spectra_close(got.surfaceTemperature[r], ref["sourceTemperature"], scale, "%d T_s" % r)
        spectra_close(got.emissivity[r], ref["emissivity"], scale, "%d e" % r)
        assert got.segmentTemperature[r].shape == (len(p), 2, x.size)
        if len(p):
            spectra_close(got.segmentTemperature[r], np.array(ref["segmentTemperature"]), scale, "%d segments" % r)
        for l in range(len(atm)):
            if l not in ref["opticalDepth"]:
                assert np.all(got.opticalDepth[r, l] == 0.0) and np.all(got.molecules[l][r] == 0.0)
                continue
            spectra_close(got.opticalDepth[r, l], ref["opticalDepth"][l], scale, "%d ln tau %d" % (r, l))
            for m in range(2):
                spectra_close(got.molecules[l][r, m], ref["terms"][2 * l + m], scale, "%d molecule %d of %d" % (r, m, l))
    # the black surface: emissivity 1 without dI/de
    black = [p for p in paths if p.bounce is None]
    a = atm.pathJacobiansLinear(black, surfaceTemperature=295)
    b = atm.pathJacobiansLinear(black, surfaceTemperature=295, emissivity=1.0, reflection="specular")
    assert a.emissivity is None and b.emissivity is not None
    for name in ("radiance", "opticalDepth", "surfaceTemperature"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert all(np.array_equal(p, q) for p, q in zip(a.segmentTemperature, b.segmentTemperature))
    # 40 mirror paths with molecules are 40 x (2 + 4 + 16 + 8) rows: three chunks, the same bits as each path alone
    many = [atm.reflectedPath(mu=m, levelTemperatures=LEVELS) for m in np.linspace(1.0, 0.3, 40)]
    a = atm.pathJacobiansLinear(many, surfaceTemperature=295, molecules=True, emissivity=e)
    for r in (0, 16, 17, 34, 39):
        b = atm.pathJacobiansLinear(many[r], surfaceTemperature=295, molecules=True, emissivity=e)
        for name in ("radiance", "opticalDepth", "surfaceTemperature", "emissivity"):
            assert np.array_equal(getattr(a, name)[r], getattr(b, name)[0]), (r, name)
        assert np.array_equal(a.segmentTemperature[r], b.segmentTemperature[0]), r
        assert all(np.array_equal(p[r], q[0]) for p, q in zip(a.molecules, b.molecules))
    # channels: every row convolved, the segment rows among them
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    ch = atm.pathJacobiansLinear(paths[:3], surfaceTemperature=295, emissivity=e, instrument=ins)
    full = atm.pathJacobiansLinear(paths[:3], surfaceTemperature=295, emissivity=e)
    assert ch.brightnessTemperature.shape == (3, len(ins)) and ch.brightnessTemperatureJacobian is None
    assert np.array_equal(ch.emissivity, pyrad.convolve(ins, full.emissivity, *RNG))
    assert np.array_equal(ch.opticalDepth[1], pyrad.convolve(ins, full.opticalDepth[1], *RNG))
    assert np.array_equal(ch.segmentTemperature[2][:, 1], pyrad.convolve(ins, full.segmentTemperature[2][:, 1], *RNG))


# ---- laziness ------------------------------------------------------------------------------------------------------------------
def test_no_accumulate_after_transmission(pyrad, lines, ctx):
    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    ctx.profile_enable(["xsec_accumulate"])
    try:
        ctx.profile_reset()
        atm.jacobiansLinear(surfaceTemperature=288, molecules=False)
        atm.pathJacobiansLinear([atm.nadirPath(levelTemperatures=True), atm.limbPath(2.5e4, levelTemperatures=True)],
                                surfaceTemperature=288)
        atm.observeLinear(ins, surfaceTemperature=288, jacobians=True)
        assert ctx.profile_read()["xsec_accumulate"][0] == 0
        atm[2].changeTemperature(250)                      # one layer due: the counter does count
        atm.jacobiansLinear(surfaceTemperature=288, molecules=False)
        assert ctx.profile_read()["xsec_accumulate"][0] >= 1
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


# ---- refusals of the C entry points ------------------------------------------------------------------------------------------
def test_column_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    rs = np.random.RandomState(5)
    L, n = 3, 1027
    k = synthetic_k(rs, L, n)
    nv = 3 + 3 * L + 1
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    jac, st, sT, se = ctx.buffer(nv), ctx.buffer(L * n), ctx.buffer(2 * L * n), ctx.buffer(n)
    src, top, em = (ctx.buffer(n).upload(np.full(n, v)) for v in (0.1, 0.02, 0.8))
    jac_short, n_short, spec_short, edge_short = ctx.buffer(nv - 1), ctx.buffer(n - 1), ctx.buffer(L * n - 1), ctx.buffer(2 * L * n - 1)
    i64, f64 = lambda v: (C.c_int64 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    nmax, tmax = _native.limit("flux_angles"), _native.limit("jacobian_terms")
    edges = [288.0, 270.0, 268.0, 240.0, 238.0, 215.0]
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), T=f64(edges),
                depth=f64([1e4, 2e4, 1e4]), lo=600.0, hi=700.0, n=n, I_surface=src.h, surface_T=0.0, I_top=top.h, n_angles=2,
                mu=f64([1.0, 0.5]), weight=f64([1.0, 2.0]), n_bands=1, band_first=i64([0]), band_count=i64([n]),
                emissivity=em.h, emissivity_all=0.5, reflection=0, n_terms=1, term_abs_coef=(C.c_void_p * 1)(kb[1].h),
                term_layer=i32([1]), jac=jac.h, ln_tau=st.h, T_spec=sT.h, e_spec=se.h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_jacobian_linear_dev(*[a[key] for key in good])

    def edge(i, v):
        out = list(edges)
        out[i] = v
        return f64(out)

    bad = [dict(abs_coef=None), dict(T=None), dict(depth=None), dict(mu=None), dict(weight=None), dict(band_first=None),
           dict(band_count=None), dict(jac=None), dict(n_layers=-1), dict(n_layers=_native.limit("layers_per_column") + 1),
           dict(n=-5), dict(n_angles=0), dict(n_angles=nmax + 1, mu=f64([0.5] * (nmax + 1)), weight=f64([1.0] * (nmax + 1))),
           dict(n_bands=0), dict(n_bands=_native.limit("flux_bands") + 1), dict(I_surface=None, surface_T=0.0),
           dict(band_count=i64([n + 1])), dict(band_first=i64([-1])), dict(band_count=i64([0])),
           dict(depth=f64([1e4, -1.0, 1e4])), dict(mu=f64([1.0, 0.0])), dict(mu=f64([1.0, 1.5])),
           dict(weight=f64([1.0, float("inf")])), dict(I_surface=n_short.h),
           dict(abs_coef=(C.c_void_p * L)(kb[0].h, n_short.h, kb[2].h)),
           # the edge temperatures: finite and > 0, bottom and top
           dict(T=edge(2, 0.0)), dict(T=edge(3, 0.0)), dict(T=edge(0, -1.0)), dict(T=edge(5, float("nan"))),
           dict(T=edge(4, float("inf"))), dict(T=edge(1, float("inf"))),
           # the Jacobian's own, with the new layouts
           dict(jac=jac_short.h), dict(ln_tau=spec_short.h), dict(T_spec=edge_short.h), dict(T_spec=st.h), dict(n_terms=-1),
           dict(n_terms=tmax + 1), dict(term_abs_coef=None), dict(term_layer=None), dict(term_layer=i32([L])),
           dict(term_layer=i32([-1])), dict(term_abs_coef=(C.c_void_p * 1)(n_short.h)),
           # the surface's own
           dict(I_top=n_short.h), dict(e_spec=n_short.h), dict(reflection=2), dict(reflection=-1),
           dict(emissivity=None, emissivity_all=-0.01), dict(emissivity=None, emissivity_all=1.01),
           dict(emissivity=None, emissivity_all=float("nan")), dict(emissivity=n_short.h),
           dict(weight=f64([1.0, -1.0])), dict(weight=f64([1.0, -2.0])), dict(weight=f64([1e308, 1e308])),
           dict(weight=f64([1.0, float("nan")]))]
    outs = (jac, st, sT, se)
    try:
        assert call() == 0
        want = [b.download() for b in outs]
        for b in outs:
            b.upload(np.full(b.n, -7.0))
        assert call(ctx=None) == BAD_ARG
        for kw in bad:
            assert call(**kw) == BAD_ARG, sorted(kw)
            assert lib.lbl_last_error(ctx.h), sorted(kw)
        ctx.set_option("sweep_ieee_divisions", 1)
        try:
            assert call() == BAD_ARG
            assert b"sweep_ieee_divisions" in lib.lbl_last_error(ctx.h)
        finally:
            ctx.set_option("sweep_ieee_divisions", 0)
        for b in outs:                                          # nothing was enqueued by a refused call
            assert np.all(b.download() == -7.0)
        assert call(emissivity_all=7.0) == 0                    # not looked at beside a buffer
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        # the black surface: emissivity NULL with emissivity_all 1
        assert call(ln_tau=None, T_spec=None, e_spec=None, I_top=None, emissivity=None, emissivity_all=1.0, reflection=1,
                    n_terms=0, term_abs_coef=None, term_layer=None) == 0
    finally:
        for b in kb + [jac, st, sT, se, src, top, em, jac_short, n_short, spec_short, edge_short]:
            b.free()


def test_ray_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    rs = np.random.RandomState(3)
    L, n, R = 3, 1027, 2
    k = synthetic_k(rs, L, n)
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    rows = (2 + 3 + 2 * 3 + 1) + (2 + 2 + 2 * 2 + 1)            # ray 0: 0 M 1 2, ray 1: 2 1; the term lies in layer 1
    rad, jac, src = ctx.buffer(R * n), ctx.buffer(rows * n), ctx.buffer(n).upload(np.full(n, 0.1))
    em = ctx.buffer(n).upload(np.full(n, 0.8))
    short, jac_short, n_short = ctx.buffer(R * n - 1), ctx.buffer(rows * n - 1), ctx.buffer(n - 1)
    i32, f64 = lambda v: (C.c_int32 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    tmax = _native.limit("jacobian_terms")
    temps = [288.0, 270.0, float("nan"), -1.0, 268.0, 240.0, 238.0, 215.0, 215.0, 238.0, 240.0, 268.0]   # (a marker's pair is ignored)
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), T=f64(temps), lo=600.0,
                hi=700.0, n=n, n_rays=R, ray_first=i32([0, 4, 6]), seg_layer=i32([0, MARKER, 1, 2, 2, 1]),
                seg_length=f64([1e4, 0.0, 2e4, 1e4, 3e4, 1e4]), source_kind=i32([1, 0]), I_source=src.h, source_T=0.0,
                emissivity=em.h, emissivity_all=0.5, n_terms=1, term_abs_coef=(C.c_void_p * 1)(kb[1].h), term_layer=i32([1]),
                radiance=rad.h, jac=jac.h)
    assert _native.ray_jacobian_rows(L, [0, 4, 6], [0, MARKER, 1, 2, 2, 1], [1], linear=True)[1] == rows

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_ray_jacobian_linear_dev(*[a[key] for key in good])

    def temp(i, v):
        out = list(temps)
        out[i] = v
        return f64(out)

    bad = [dict(abs_coef=None), dict(T=None), dict(ray_first=None), dict(seg_layer=None), dict(seg_length=None),
           dict(source_kind=None), dict(jac=None), dict(n_layers=0), dict(n=0), dict(n_rays=0),
           dict(ray_first=i32([1, 4, 6])), dict(ray_first=i32([0, 4, 3])),
           dict(seg_layer=i32([0, MARKER, 3, 2, 2, 1])), dict(seg_layer=i32([0, -2, 1, 2, 2, 1])),
           dict(seg_length=f64([1e4, 0.0, -1.0, 1e4, 3e4, 1e4])), dict(seg_length=f64([1e4, 0.0, float("nan"), 1e4, 3e4, 1e4])),
           dict(source_kind=i32([2, 0])),
           # the segment temperatures: finite and > 0, entry and exit (a marker's pair excepted)
           dict(T=temp(0, 0.0)), dict(T=temp(1, -5.0)), dict(T=temp(4, float("nan"))), dict(T=temp(11, float("inf"))),
           dict(seg_length=f64([1e4, 1.0, 2e4, 1e4, 3e4, 1e4])),
           dict(source_kind=i32([0, 0]), I_source=None, source_T=0.0),
           dict(emissivity=None, emissivity_all=-0.01), dict(emissivity=None, emissivity_all=1.01),
           dict(emissivity=None, emissivity_all=float("nan")), dict(emissivity=n_short.h),
           dict(radiance=short.h), dict(jac=jac_short.h), dict(I_source=n_short.h),
           dict(abs_coef=(C.c_void_p * L)(kb[0].h, n_short.h, kb[2].h)),
           dict(n_terms=-1), dict(n_terms=tmax + 1), dict(term_abs_coef=None), dict(term_layer=None),
           dict(term_layer=i32([L])), dict(term_layer=i32([-1])), dict(term_abs_coef=(C.c_void_p * 1)(n_short.h))]
    try:
        assert call() == 0
        want_I, want_J = rad.download(), jac.download()
        assert not np.isnan(want_J).any()
        rad.upload(np.full(R * n, -7.0))
        jac.upload(np.full(rows * n, -7.0))
        assert call(ctx=None) == BAD_ARG
        for kw in bad:
            assert call(**kw) == BAD_ARG, sorted(kw)
            assert lib.lbl_last_error(ctx.h), sorted(kw)
        ctx.set_option("sweep_ieee_divisions", 1)
        try:
            assert call() == BAD_ARG
            assert b"sweep_ieee_divisions" in lib.lbl_last_error(ctx.h)
        finally:
            ctx.set_option("sweep_ieee_divisions", 0)
        assert np.all(rad.download() == -7.0) and np.all(jac.download() == -7.0)
        assert call(radiance=None, emissivity_all=7.0) == 0
        assert np.array_equal(jac.download(), want_J) and np.all(rad.download() == -7.0)
        assert call() == 0
        assert np.array_equal(rad.download(), want_I) and np.array_equal(jac.download(), want_J)
    finally:
        for b in kb + [rad, jac, src, em, short, jac_short, n_short]:
            b.free()


# ---- temperature="full": dk/dT as terms, under the Voigt line shape ------------------------------------------------------------
@pytest.fixture()
def voigt_model():
    """tests/test_gpu_voigt_dT.py's model: the Voigt line shape, under which k is smooth in T"""
    from pyrad_amd import data, model, settings, synthetic
    model.Layer.hasAtmosphere = False
    settings.set_layer_step("merged")
    settings.set_line_shape("voigt")
    data.set_source(data.synthetic_source(dict(co2=synthetic.make_lines(41, 150, 590, 615),
                                               h2o=synthetic.make_lines(42, 150, 590, 615))))
    yield model
    settings.set_line_shape("reference")
    data.set_source(None)
    model.Layer.hasAtmosphere = False


def test_full_temperature_jacobian_against_finite_differences(voigt_model):
    """dF/dT_l of jacobiansLinear(temperature="full") with the default levels - the chain through levelTemperatures() plus the
    absorption part through dk_l/dT - against R = (4 D1 - D2) / 3 of the model's own olr, D1 and D2 the central differences
    at +-1 K and +-2 K; tolerance |D1 - D2| + 1e-6 |R|, the differences' own truncation estimate
    (tests/test_gpu_voigt_dT.py's procedure and column)."""
    from test_gpu_voigt_dT import LAYERS as VOIGT_LAYERS, _layer
    atm = voigt_model.Atmosphere("fd")
    for depth, T, P in VOIGT_LAYERS:
        _layer(voigt_model, atm, depth, T, P)
    kw = dict(surfaceTemperature=288, angles=3, emissivity=0.8)
    plain = atm.jacobiansLinear(**kw)
    full = atm.jacobiansLinear(temperature="full", **kw)
    for name in ("olr", "surfaceTemperature", "temperature", "opticalDepth", "edgeTemperature", "levelTemperature"):
        assert np.array_equal(getattr(full, name), getattr(plain, name)), name
    assert plain.temperatureAbsorption is None and plain.temperatureFull is None
    assert full.temperatureAbsorption.shape == full.temperature.shape == (3,)
    assert np.array_equal(full.temperatureFull, full.temperature + full.temperatureAbsorption)
    lean = atm.jacobiansLinear(temperature="full", molecules=False, **kw)
    assert np.array_equal(lean.temperatureAbsorption, full.temperatureAbsorption) and lean.molecules is None
    # with given levels the per-layer chain is None, and with it temperatureFull; the absorption part does not depend on that
    given = atm.jacobiansLinear(temperature="full", levelTemperatures=atm.levelTemperatures(), **kw)
    assert given.temperature is None and given.temperatureFull is None
    assert np.array_equal(given.temperatureAbsorption, full.temperatureAbsorption)
    for l, (L, (_, T, _)) in enumerate(zip(atm, VOIGT_LAYERS)):
        F = {}
        for d in (-2, -1, 1, 2):
            L.changeTemperature(T + d)
            F[d] = float(atm.jacobiansLinear(molecules=False, **kw).olr)
        L.changeTemperature(T)
        D1, D2 = (F[1] - F[-1]) / 2, (F[2] - F[-2]) / 4
        R = (4 * D1 - D2) / 3
        err = abs(full.temperatureFull[l] - R)
        print("layer %d: full %.9e, Planck chain %.9e, differences %.9e, |err| %.2e, |D1 - D2| %.2e"
              % (l, full.temperatureFull[l], full.temperature[l], R, err, abs(D1 - D2)))
        assert err <= abs(D1 - D2) + 1e-6 * abs(R), (l, err, abs(D1 - D2))
