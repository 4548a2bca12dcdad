"""GPU: Jacobians over a reflecting surface - Atmosphere.jacobians, pathJacobians and observe with an emissivity
(lbl_column_jacobian_surface_dev, lbl_ray_jacobian_surface_dev, kernels K5h) - against the NumPy restatements of
tests/test_surface_jacobian_cpu.py, for their identities with the black surface and between the two kernels, against finite
differences through the public surface, in their physical limits, and for independence of the rays, determinism and the C
ABI's refusals.  Column and tolerances are tests/test_gpu_jacobian.py's, rays and synthetic coefficients
tests/test_gpu_surface.py's.

Tolerances.  Bands: rel 1e-9 + 1e-12 x olr; spectra: 1e-9 + 1e-11 x scale; finite differences: 1e-6 + 1e-10 x olr
(tests/test_gpu_jacobian.py derives the floor for the upward leg: the unclamped A B + D carries about L 1e-16 of the outgoing
radiance, tau / mu multiplies it, and the clamp to [-A t Imax, A t B] holds the product below 40 L 1e-16 Imax).  The reflected
leg obeys the same bound with Dmax in place of Imax: its unclamped form C_l B_l + D'_l carries the rounding of D (the
downward radiance at the surface) and of E', about L 1e-16 D <= L 1e-16 Dmax; d ln tau multiplies it by tau / mu, and where
that factor is large the clamp to [-C_l t_l Dmax, C_l t_l B_l] bounds the value by C t max(B_l, Dmax) (tau / mu) with x e^-x <=
0.37, so the error per point is at most about 40 L 1e-16 max(Dmax, B_l).  It enters F through Q_k <= (1 - e) W_k Ttot <= W_k:
never more than the upward leg's own weight, and Dmax <= max(I_top, max_l B_l), the scale of the outgoing radiance itself."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyrad_oracle as orc
from test_gpu_jacobian import FLOOR, band_idx, check, column, lines, molecules_array, pyrad  # noqa: F401
from test_gpu_paths import ctx, nine_paths, synthetic_k  # noqa: F401
from test_gpu_surface import marked_rays, run_raw_rays, spectral_emissivity
from test_jacobian_cpu import planck_dT
from test_surface_jacobian_cpu import MARKER, surface_jacobian_reference, surface_path_jacobian_reference, weight_sum

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
REFLECTIONS = ("lambertian", "specular")
RNG = (600, 700.07)   # 10,007 points: a tail of three


def spectra_close(got, want, scale, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bound = 1e-9 * np.abs(want) + 1e-11 * scale
    print("%s: worst |error| / scale %.2e, worst error / bound %.2e" % (what, np.max(err) / scale if err.size else 0.0,
                                                                      np.max(err / bound) if err.size else 0.0))
    assert np.all(err <= bound), what


def reference(pyrad, atm, mu, w, e, reflection, surface_T=None, surface=None, top=None, bands=None):
    from pyrad_amd import settings
    x = atm[0].xAxis
    k = [np.array(pyrad.getAbsCoef(L)) for L in atm]
    terms = [(l, np.array(pyrad.getAbsCoef(m))) for l, L in enumerate(atm) for m in L]
    return surface_jacobian_reference(x, k, [L.T for L in atm], [L.depth for L in atm], mu, w, e, reflection,
                                      surface_T=surface_T, surface=surface, top=top, terms=terms, idx=band_idx(x, bands),
                                      res=settings.BASE_RESOLUTION)


# ---- 1. against NumPy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflection", REFLECTIONS)
@pytest.mark.parametrize("angles", [1, 3, 8, [(1.0, 1.0), (0.3, 2.0)]])
def test_against_numpy(pyrad, lines, angles, reflection):
    atm = column(pyrad, rng=RNG)
    x = atm[0].xAxis
    n = x.size
    edges = [0, 1001, 2502, 2503, 6007, n]              # edges at indices not = 0 (mod 4), a single-point band
    banded = [(x[a], x[b] if b < n else np.inf) for a, b in zip(edges[:-1], edges[1:])]
    mu, w = pyrad.fluxAngles(angles)
    top = 0.3 * np.array(atm[0].planck(250))
    table = ([598.0, 620.0, 655.5, 712.0], [0.95, 0.6, 0.8, 0.99])
    for e, e_grid, kw, bands in (
            (0.8, 0.8, dict(surfaceTemperature=288), None),
            (spectral_emissivity(x), spectral_emissivity(x), dict(surfaceSpectrum=0.9 * atm[0].planck(295), topSpectrum=top), banded),
            (table, np.interp(x, *table), dict(surfaceTemperature=288, topSpectrum=top), banded)):
        j = atm.jacobians(angles=angles, bands=bands, spectra=True, molecules=True, emissivity=e, reflection=reflection, **kw)
        ref = reference(pyrad, atm, mu, w, e_grid, reflection, surface_T=kw.get("surfaceTemperature"),
                        surface=kw.get("surfaceSpectrum"), top=kw.get("topSpectrum"), bands=bands)
        sq = (lambda a: a[0]) if bands is None else (lambda a: a)
        olr = sq(ref["olr"])
        assert np.array_equal(j.mu, mu) and np.array_equal(j.weight, w)
        check(j.olr, olr, olr, rel=1e-12, what="olr")
        # the forward model is fluxes()'s
        f = atm.fluxes(angles=angles, bands=bands, emissivity=e, reflection=reflection, **kw)
        assert np.all(np.abs(j.olr - f.up[..., -1]) <= 1e-13 * f.up[..., -1])
        if "surfaceTemperature" in kw:
            check(j.surfaceTemperature, sq(ref["surfaceTemperature"]), olr, what="T_s")
        else:
            assert j.surfaceTemperature is None
        check(j.emissivity, sq(ref["emissivity"]), olr, what="e")
        check(j.opticalDepth, sq(ref["opticalDepth"]), olr, what="ln tau")
        check(j.temperature, sq(ref["temperature"]), olr, what="T")
        check(molecules_array(j), sq(ref["terms"]).reshape(np.shape(olr) + (len(atm), 2)), olr, what="molecules")
        res = x[1] - x[0]
        scale = np.max(np.abs(ref["olr"])) / (res * n)
        for name in ("opticalDepthSpectrum", "temperatureSpectrum", "emissivitySpectrum"):
            spectra_close(getattr(j, name), ref[name], scale, "%s %s %s" % (reflection, np.ndim(e_grid), name))
        # without spectra: the same band values, no spectrum
        b = atm.jacobians(angles=angles, bands=bands, molecules=False, emissivity=e, reflection=reflection, **kw)
        assert b.emissivitySpectrum is None and b.opticalDepthSpectrum is None and b.molecules is None
        for name in ("olr", "emissivity", "opticalDepth", "temperature"):
            assert np.array_equal(getattr(b, name), getattr(j, name)), name


# ---- the raw ABI on uploaded synthetic coefficients --------------------------------------------------------------------
def run_raw_jac(ctx, k, T, depth, mu, w, e, reflection, lo=600.0, hi=700.0, source_T=0.0, I_source=None, top=None,
                bands=None, terms=()):
    """lbl_column_jacobian_surface_dev: (band values [band, 3 + 2 L + terms], ln tau spectra, T spectra, e spectrum);
    terms: (layer, k_m) pairs"""
    L, n = k.shape
    first, count = ([0], [n]) if bands is None else ([a for a, _ in bands], [b - a for a, b in bands])
    nb, nv = len(first), 3 + 2 * L + len(terms)
    bufs = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    tb = [ctx.buffer(n).upload(km) for _, km in terms]
    jac, st, sT, se = ctx.buffer(nb * nv), ctx.buffer(max(L * n, 1)), ctx.buffer(max(L * n, 1)), ctx.buffer(n)
    extra = []
    try:
        src = eb = pb = None
        if I_source is not None:
            src = ctx.buffer(n).upload(I_source); extra.append(src)
        if np.ndim(e):
            eb = ctx.buffer(n).upload(e); extra.append(eb)
        if top is not None:
            pb = ctx.buffer(n).upload(top); extra.append(pb)
        ctx.column_jacobian_surface_dev(bufs, T, depth, lo, hi, n, mu, w, first, count, jac, eb if eb is not None else e,
                                        reflection=REFLECTIONS.index(reflection), I_surface=src, surface_T=source_T, I_top=pb,
                                        term_abs_coef=tb, term_layer=[l for l, _ in terms], ln_tau_spectra=st, T_spectra=sT,
                                        e_spectrum=se)
        return (jac.download(nb * nv).reshape(nb, nv), st.download(L * n).reshape(L, n) if L else np.zeros((0, n)),
                sT.download(L * n).reshape(L, n) if L else np.zeros((0, n)), se.download(n))
    finally:
        for b in bufs + tb + [jac, st, sT, se] + extra:
            b.free()


def check_raw_jac(ctx, k, T, depth, mu, w, e, reflection, lo=600.0, hi=700.0, source_T=0.0, I_source=None, top=None,
                  bands=None, terms=()):
    L, n = k.shape
    x = np.linspace(lo, hi, n)
    v, st, sT, se = run_raw_jac(ctx, k, T, depth, mu, w, e, reflection, lo, hi, source_T, I_source, top, bands, terms)
    ref = surface_jacobian_reference(x, list(k), T, depth, mu, w, e, reflection, surface_T=source_T or None, surface=I_source,
                                     top=top, terms=terms, idx=bands)
    olr = ref["olr"]
    check(v[:, 0], olr, olr, rel=1e-12, what="olr")
    check(v[:, 1], ref["surfaceTemperature"], olr, what="T_s")
    check(v[:, 2], ref["emissivity"], olr, what="e")
    check(v[:, 3:3 + L], ref["opticalDepth"], olr, what="ln tau")
    check(v[:, 3 + L:3 + 2 * L], ref["temperature"], olr, what="T")
    if terms:
        check(v[:, 3 + 2 * L:], ref["terms"], olr, what="terms")
    inside = np.ones(n, dtype=bool)
    if bands is not None:                        # (points outside every band keep 0 in the spectra)
        inside[:] = False
        for a, b in bands:
            inside[a:b] = True
    scale = max(np.max(np.abs(np.where(inside, ref["olrSpectrum"], 0.0))), 1e-300)
    tag = "%s L=%d n=%d angles=%d" % (reflection, L, n, len(mu))
    spectra_close(st, np.where(inside, ref["opticalDepthSpectrum"], 0.0), scale, tag + " ln tau")
    spectra_close(sT, np.where(inside, ref["temperatureSpectrum"], 0.0), scale, tag + " T")
    spectra_close(se, np.where(inside, ref["emissivitySpectrum"], 0.0), scale, tag + " e")
    return v


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 5003])
def test_raw_column_sizes(ctx, pyrad, n):
    rs = np.random.RandomState(300 + n)
    for L, angles in ((1, 3), (4, 2), (4, 5)):
        k = synthetic_k(rs, L, n)
        T = list(np.linspace(288.0, 215.0, L))
        depth = list(rs.uniform(0.5e4, 2e4, L))
        mu, w = pyrad.fluxAngles(angles)
        e = rs.uniform(0.3, 1.0, n)
        e[::7] = 1.0
        e[3::11] = 0.0
        terms = [(l, rs.uniform(0.0, 1.0, n) * k[l]) for l in range(L)] + [(0, k[0])]
        bands = None if n < 1027 else [(1, 515), (515, 516), (518, n)]
        for reflection in REFLECTIONS:
            check_raw_jac(ctx, k, T, depth, mu, w, e, reflection, source_T=295.0, top=rs.uniform(0.0, 0.2, n), bands=bands,
                          terms=terms)
        check_raw_jac(ctx, k, T, depth, mu, w, 0.7, "lambertian", I_source=rs.uniform(0.0, 0.2, n))


def test_raw_column_128_layers_eight_angles(ctx, pyrad):
    rs = np.random.RandomState(37)
    L, n = 128, 1027
    k = synthetic_k(rs, L, n, tau_lo=-6.0, tau_hi=-5.0, huge=0.002)
    T = list(np.linspace(290.0, 180.0, L))
    depth = list(rs.uniform(0.5e4, 1e4, L))
    mu, w = pyrad.fluxAngles(8)
    e = rs.uniform(0.3, 1.0, n)
    for reflection in REFLECTIONS:
        check_raw_jac(ctx, k, T, depth, mu, w, e, reflection, source_T=300.0, top=rs.uniform(0.0, 0.1, n),
                      terms=[(0, k[0]), (127, k[127]), (64, 0.5 * k[64])])


def test_raw_column_beyond_the_grid_stride_bound(ctx, pyrad):
    """1,024 workgroups of 1,024 points, then the grid-stride loop's second round, and a tail of 1 point (n = 4 q + 1)"""
    rs = np.random.RandomState(41)
    n = 1048576 + 1029
    k = synthetic_k(rs, 2, n)
    mu, w = pyrad.fluxAngles(2)
    check_raw_jac(ctx, k, [255.0, 230.0], [1e4, 2e4], mu, w, rs.uniform(0.3, 1.0, n), "lambertian", source_T=290.0,
                  top=rs.uniform(0.0, 0.1, n))


# ---- 2. emissivity 1 is the black surface ------------------------------------------------------------------------------
BAND_FIELDS = ("olr", "surfaceTemperature", "temperature", "opticalDepth")
SPECTRA = ("temperatureSpectrum", "opticalDepthSpectrum")


@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_emissivity_one_is_the_black_surface(pyrad, lines, reflection):
    atm = column(pyrad, rng=RNG)
    x = atm[0].xAxis
    edges = [0, 1001, 2502, 2503, 6007, x.size]
    bands = [(x[a], x[b] if b < x.size else np.inf) for a, b in zip(edges[:-1], edges[1:])]
    for angles in (1, 2, [(1.0, 1.0), (0.3, 2.0)], 3, 8):
        mu, _ = pyrad.fluxAngles(angles)
        for kw in (dict(surfaceTemperature=288), dict(surfaceTemperature=288, bands=bands)):
            black = atm.jacobians(angles=angles, spectra=True, **kw)
            for e in (1.0, np.ones(x.size)):
                got = atm.jacobians(angles=angles, spectra=True, emissivity=e, reflection=reflection, **kw)
                assert black.emissivity is None and got.emissivity is not None
                if len(mu) <= 2:
                    for name in BAND_FIELDS + SPECTRA:
                        assert np.array_equal(getattr(got, name), getattr(black, name)), (angles, sorted(kw), name)
                    assert all(np.array_equal(p, q) for p, q in zip(got.molecules, black.molecules))
                else:
                    for name in BAND_FIELDS:
                        check(getattr(got, name), getattr(black, name), black.olr, what=name)
                    check(molecules_array(got), molecules_array(black), black.olr, what="molecules")
                    scale = np.max(np.abs(black.olr)) / ((x[1] - x[0]) * x.size)
                    for name in SPECTRA:
                        spectra_close(getattr(got, name), getattr(black, name), scale, name)


def test_emissivity_one_is_the_black_surface_paths(pyrad, lines):
    atm = column(pyrad, rng=(600, 610.07))
    paths = nine_paths(pyrad, atm)
    assert len(paths) == 10
    for kw in (dict(surfaceTemperature=295), dict(surfaceSpectrum=atm[0].planck(300))):
        black = atm.pathJacobians(paths, molecules=True, **kw)
        for e in (1.0, np.ones(atm[0].xAxis.size)):
            got = atm.pathJacobians(paths, molecules=True, emissivity=e, reflection="specular", **kw)
            for name in ("radiance", "temperature", "opticalDepth", "surfaceTemperature"):
                assert np.array_equal(getattr(got, name), getattr(black, name)), name
            assert all(np.array_equal(p, q) for p, q in zip(got.molecules, black.molecules))
            assert black.emissivity is None and got.emissivity.shape == got.radiance.shape


# ---- 3. finite differences through the public surface -----------------------------------------------------------------------
@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_finite_differences(pyrad, lines, reflection):
    from pyrad_amd import engine, settings
    atm = column(pyrad, rng=(600, 700))
    Ts, e0 = 288.0, 0.7
    mu, w = pyrad.fluxAngles(3)
    top = 0.3 * np.array(atm[0].planck(250))
    kw = dict(angles=3, topSpectrum=top, reflection=reflection)
    j = atm.jacobians(surfaceTemperature=Ts, emissivity=e0, **kw)
    olr = j.olr
    res = settings.BASE_RESOLUTION
    n = atm[0].xAxis.size

    def near(a, fd, what):
        print("%s: analytic %.6e differences %.6e" % (what, a, fd))
        assert abs(a - fd) <= 1e-6 * abs(a) + 1e-10 * olr, (what, a, fd)

    def up(e=e0, T_s=Ts):
        return atm.fluxes(surfaceTemperature=T_s, emissivity=e, **kw).up[-1]

    eps, h = 1e-4, 1e-2
    for l, L in enumerate(atm):
        d0 = L.depth
        L.changeDepth(d0 * np.exp(eps))
        fp = up()
        L.changeDepth(d0 * np.exp(-eps))
        fm = up()
        L.changeDepth(d0)
        near(j.opticalDepth[l], (fp - fm) / (2 * eps), "ln tau %d" % l)
    near(j.surfaceTemperature, (up(T_s=Ts + h) - up(T_s=Ts - h)) / (2 * h), "T_s")
    # F is affine in e: the central difference is the derivative up to the rounding of the two fluxes
    fd = (up(e=e0 + 0.05) - up(e=e0 - 0.05)) / 0.1
    print("dF/de: analytic %.12e differences %.12e" % (j.emissivity, fd))
    assert abs(j.emissivity - fd) <= 1e-10 * olr
    # the layer temperatures (Planck part) through the forward entry point, the coefficients held
    ctx = engine.get_engine().ctx
    kb = [L.__dict__["_sweep_state"].bufs["abs_coef"] for L in atm]
    T, d = [L.T for L in atm], [L.depth for L in atm]
    level, tb = ctx.buffer(2 * (len(atm) + 1)), ctx.buffer(n).upload(top)
    try:
        def flux_top(TT):
            ctx.column_flux_surface_dev(kb, TT, d, 600, 700, n, mu, w, [0], [n], level, e0,
                                        reflection=REFLECTIONS.index(reflection), surface_T=Ts, I_top=tb)
            return level.download(2 * (len(atm) + 1))[len(atm)] * res
        for l in range(len(atm)):
            Tp, Tm = list(T), list(T)
            Tp[l] += h
            Tm[l] -= h
            near(j.temperature[l], (flux_top(Tp) - flux_top(Tm)) / (2 * h), "T %d" % l)
    finally:
        level.free()
        tb.free()


def test_finite_differences_paths(pyrad, lines):
    atm = column(pyrad, rng=(600, 610.07))
    Ts, e0 = 295.0, 0.7
    mirror = atm.reflectedPath(mu=0.6)
    bent = pyrad.Path([1, 0, 0, 2], [3e4, 2e4, 1e4, 7e3], source="surface", bounce=2)
    for p in (mirror, bent):
        kw = dict(reflection="specular")
        j = atm.pathJacobians(p, surfaceTemperature=Ts, emissivity=e0, **kw)
        rad = lambda q=p, e=e0, T_s=Ts: atm.radiance(q, surfaceTemperature=T_s, emissivity=e, **kw).radiance[0]
        scale = np.max(j.radiance[0])
        assert np.array_equal(j.radiance[0], rad())
        # one bounce: I is affine in e
        fd = (rad(e=e0 + 0.05) - rad(e=e0 - 0.05)) / 0.1
        print("dI/de: worst |difference| / max I %.2e" % (np.max(np.abs(j.emissivity[0] - fd)) / scale))
        assert np.all(np.abs(j.emissivity[0] - fd) <= 1e-10 * scale)
        # (Richardson: a plain central difference is off by eps^2 / 6 times the third derivative, which at a single grid
        # point is not small against the first)
        eps, h = 2e-3, 1e-2
        for l in sorted(set(p.layers)):
            def central(step):
                qs = [pyrad.Path(p.layers, [s * np.exp(sg * step) if ll == l else s for ll, s in zip(p.layers, p.lengths)],
                                 source=p.source, bounce=p.bounce) for sg in (1, -1)]
                return (rad(q=qs[0]) - rad(q=qs[1])) / (2 * step)
            fd = (4 * central(eps / 2) - central(eps)) / 3
            print("ln tau %d: worst |difference| / max I %.2e" % (l, np.max(np.abs(j.opticalDepth[0, l] - fd)) / scale))
            assert np.all(np.abs(j.opticalDepth[0, l] - fd) <= 1e-6 * np.abs(fd) + 1e-10 * scale), l
        fd = (rad(T_s=Ts + h) - rad(T_s=Ts - h)) / (2 * h)
        assert np.all(np.abs(j.surfaceTemperature[0] - fd) <= 1e-6 * np.abs(fd) + 1e-10 * scale)


# ---- 4. the ray is the column's one vertical angle, and observe() the column's -------------------------------------------
def test_reflected_path_is_the_specular_column_and_observe(pyrad, lines):
    atm = column(pyrad, rng=(600, 610.07))
    x = atm[0].xAxis
    step = x[1] - x[0]
    ins = pyrad.Instrument(x[5:-5:7], shape="boxcar", width=0.6 * step)          # a boxcar of one grid step: the point itself
    assert np.all(ins.support(600, 610.07, x.size)[2] == 1)
    for e in (0.6, spectral_emissivity(x)):
        for kw in (dict(surfaceTemperature=295), dict(surfaceSpectrum=atm[0].planck(300))):
            ray = atm.pathJacobians(atm.reflectedPath(), emissivity=e, **kw)
            col = atm.jacobians(emissivity=e, reflection="specular", angles=[(1.0, 1.0)], spectra=True, molecules=False, **kw)
            scale = np.max(ray.radiance[0])
            spectra_close(ray.opticalDepth[0], col.opticalDepthSpectrum, scale, "ln tau")
            spectra_close(ray.temperature[0], col.temperatureSpectrum, scale, "T")
            spectra_close(ray.emissivity[0], col.emissivitySpectrum, scale, "e")
            ob = atm.observe(ins, emissivity=e, jacobians=True, **kw)
            flux = atm.fluxes(emissivity=e, reflection="specular", angles=[(1.0, 1.0)], spectra=True, **kw)
            at = slice(5, x.size - 5, 7)
            spectra_close(ob.radiance, flux.upSpectrum[at], scale, "observe radiance")
            assert np.array_equal(ob.radiance, atm.observe(ins, emissivity=e, **kw).radiance)
            spectra_close(ob.opticalDepthJacobian, col.opticalDepthSpectrum[:, at], scale, "observe ln tau")
            spectra_close(ob.temperatureJacobian, col.temperatureSpectrum[:, at], scale, "observe T")
            spectra_close(ob.emissivityJacobian, col.emissivitySpectrum[at], scale, "observe e")
    # without an emissivity observe() is what it was
    ob = atm.observe(ins, surfaceTemperature=295, jacobians=True)
    one = atm.observe(ins, surfaceTemperature=295, jacobians=True, emissivity=1.0)
    assert ob.emissivityJacobian is None and one.emissivityJacobian.shape == (len(ins),)
    for name in ("radiance", "temperatureJacobian", "opticalDepthJacobian"):
        assert np.array_equal(getattr(ob, name), getattr(one, name)), name


# ---- 5. physics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_isothermal_cavity(pyrad, lines, reflection):
    from test_gpu_jacobian import LAYERS
    atm = column(pyrad, layers=tuple((d, 260, P) for d, _, P in LAYERS))
    x = atm[0].xAxis
    B = orc.planckWavenumber(x, 260)
    for e in (0.0, 0.37, 1.0, spectral_emissivity(x)):
        j = atm.jacobians(surfaceTemperature=260, topSpectrum=B, emissivity=e, reflection=reflection)
        print(reflection, np.ndim(e), np.max(np.abs(j.opticalDepth)) / j.olr, abs(j.emissivity) / j.olr)
        assert np.all(np.abs(j.opticalDepth) <= FLOOR * j.olr), j.opticalDepth
        assert np.all(np.abs(molecules_array(j)) <= FLOOR * j.olr)
        assert abs(j.emissivity) <= FLOOR * j.olr


def test_perfect_mirror_has_no_surface_temperature(pyrad, lines):
    atm = column(pyrad)
    for reflection in REFLECTIONS:
        j = atm.jacobians(surfaceTemperature=288, emissivity=0.0, reflection=reflection, spectra=True)
        assert j.surfaceTemperature == 0.0
    p = atm.pathJacobians(atm.reflectedPath(), surfaceTemperature=288, emissivity=0.0)
    assert np.all(p.surfaceTemperature == 0.0)


@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_transparent_column(ctx, pyrad, reflection):
    rs = np.random.RandomState(53)
    L, n = 3, 1027
    x = np.linspace(600.0, 700.0, n)
    mu, w = pyrad.fluxAngles(3)
    e, top, Ts = rs.uniform(0.2, 1.0, n), rs.uniform(0.0, 0.1, n), 290.0
    v, st, sT, se = run_raw_jac(ctx, np.zeros((L, n)), [280.0, 250.0, 220.0], [1e4] * L, mu, w, e, reflection, source_T=Ts,
                                top=top)
    Is, Wsum = orc.planckWavenumber(x, Ts), weight_sum(w)
    assert np.all(st == 0.0) and np.all(sT == 0.0) and np.all(v[:, 3:] == 0.0)
    assert np.all(np.abs(se - Wsum * (Is - top)) <= 1e-14 * Wsum * Is)
    assert abs(v[0, 2] - np.sum(Wsum * (Is - top))) <= 1e-12 * v[0, 0]
    assert abs(v[0, 1] - np.sum(e * Wsum * planck_dT(x, Ts))) <= 1e-9 * v[0, 1]


# ---- 6. rays through the raw ABI -------------------------------------------------------------------------------------------
def run_raw_ray_jac(ctx, k, T, rays, e, lo=600.0, hi=700.0, I_source=None, source_T=0.0, terms=()):
    """rays: [(layers, lengths, kind)] -> (radiance R x n, rows x n, row_first); terms: (layer, k_m) pairs"""
    from pyrad_amd import _native
    L, n = k.shape
    ray_first = np.cumsum([0] + [len(r[0]) for r in rays])
    seg_layer = [l for r in rays for l in r[0]]
    row_first, rows = _native.ray_jacobian_rows(L, ray_first, seg_layer, [l for l, _ in terms], surface=True)
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
        ctx.ray_jacobian_surface_dev(bufs, T, lo, hi, n, ray_first, seg_layer, [s for r in rays for s in r[1]],
                                     [r[2] for r in rays], jac, eb if eb is not None else e, I_source=src, source_T=source_T,
                                     term_abs_coef=tb, term_layer=[l for l, _ in terms], radiance=rad)
        return rad.download().reshape(len(rays), n), jac.download().reshape(rows, n), row_first
    finally:
        for b in bufs + tb + [rad, jac] + extra:
            b.free()


def check_raw_ray_jac(ctx, k, T, rays, e, lo=600.0, hi=700.0, I_source=None, source_T=0.0, terms=()):
    L, n = k.shape
    x = np.linspace(lo, hi, n)
    I, J, first = run_raw_ray_jac(ctx, k, T, rays, e, lo, hi, I_source, source_T, terms)
    # the radiance is lbl_ray_radiance_surface_dev's, bit for bit
    assert np.array_equal(I, run_raw_rays(ctx, k, T, rays, e, lo, hi, I_source, source_T)[0])
    assert not np.isnan(J).any()
    Ts = None if I_source is not None or not source_T > 0 else source_T
    worst = 0.0
    for r, (layers, lengths, kind) in enumerate(rays):
        ref = surface_path_jacobian_reference(x, list(k), T, layers, lengths, kind, e, surface_T=Ts, surface=I_source,
                                              terms=terms)
        crossed = sorted(ref["opticalDepth"])
        want = [ref["sourceTemperature"], ref["emissivity"]] + [ref["opticalDepth"][l] for l in crossed] \
            + [ref["temperature"][l] for l in crossed] + [ref["terms"][m] for m in sorted(ref["terms"])]
        assert first[r + 1] - first[r] == len(want), r
        got = J[first[r]:first[r + 1]]
        scale = max(np.max(np.abs(ref["radiance"])), np.max(np.abs(I_source)) if I_source is not None else 0.0, 1e-300)
        err = np.abs(got - np.array(want))
        bound = 1e-9 * np.abs(np.array(want)) + 1e-11 * scale
        worst = max(worst, np.max(err / bound))
        assert np.all(err <= bound), (r, layers, np.max(err / bound))
        if kind == 0 and MARKER not in layers:
            assert np.all(got[0] == 0.0) and np.all(got[1] == 0.0), r
    print("n = %d, %d rays: worst error / bound %.2e" % (n, len(rays), worst))
    return I, J


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 5003])
def test_raw_rays_sizes(ctx, n):
    rs = np.random.RandomState(200 + n)
    L = 3
    k = synthetic_k(rs, L, n)
    T = [288.0, 250.0, 215.0]
    rays = marked_rays(rs, L)
    assert len(rays) == 53
    e = rs.uniform(0.5, 1.0, n)
    e[::7] = 1.0
    e[3::11] = 0.0
    terms = [(l, rs.uniform(0.0, 1.0, n) * k[l]) for l in range(L)] + [(1, k[1])]
    check_raw_ray_jac(ctx, k, T, rays, 0.8, source_T=295.0)
    check_raw_ray_jac(ctx, k, T, rays, e, source_T=295.0, terms=terms)
    check_raw_ray_jac(ctx, k, T, rays, e, I_source=rs.uniform(0.0, 0.2, n), terms=terms[:1])


def test_raw_rays_128_layers_down_and_up(ctx):
    rs = np.random.RandomState(17)
    L, n = 128, 1027
    k = synthetic_k(rs, L, n, tau_lo=-6.0, tau_hi=-5.0, huge=0.002)
    T = list(np.linspace(290.0, 180.0, L))
    d = list(rs.uniform(0.5e4, 1e4, L))
    seq = list(range(L - 1, -1, -1)) + [MARKER] + list(range(L))
    lens = [d[l] for l in range(L - 1, -1, -1)] + [0.0] + d
    assert len(seq) == 257
    check_raw_ray_jac(ctx, k, T, [(seq, lens, 0), (seq, lens, 1)], rs.uniform(0.3, 1.0, n), source_T=300.0)


def test_rays_are_independent_and_calls_deterministic(ctx):
    rs = np.random.RandomState(71)
    L, n = 3, 1027
    k = synthetic_k(rs, L, n)
    T = [288.0, 250.0, 215.0]
    e = rs.uniform(0.3, 1.0, n)
    seq = [2, 1, 0, MARKER, 0, 1]
    band = [(seq, list(rs.uniform(0.5e4, 2e4, 3)) + [0.0] + list(rs.uniform(0.5e4, 2e4, 2)), i % 2) for i in range(6)]
    terms = [(0, 0.5 * k[0]), (2, k[2])]
    kw = dict(source_T=295.0, terms=terms)
    I, J, first = run_raw_ray_jac(ctx, k, T, band, e, **kw)
    I2, J2, _ = run_raw_ray_jac(ctx, k, T, band, e, **kw)
    assert np.array_equal(I, I2) and np.array_equal(J, J2)
    Ir, Jr, fr = run_raw_ray_jac(ctx, k, T, band[::-1], e, **kw)
    per = first[1] - first[0]
    assert np.all(np.diff(first) == per)
    for r in range(6):
        alone = run_raw_ray_jac(ctx, k, T, [band[r]], e, **kw)
        assert np.array_equal(alone[0][0], I[r]) and np.array_equal(alone[1], J[first[r]:first[r + 1]]), r
        assert np.array_equal(Ir[5 - r], I[r]) and np.array_equal(Jr[fr[5 - r]:fr[6 - r]], J[first[r]:first[r + 1]]), r


def test_paths_against_numpy_and_chunks(pyrad, lines):
    """the model's rows -> arrays mapping with the extra row, over chunks of 512 rows"""
    atm = column(pyrad, rng=(600, 610.07))
    x = atm[0].xAxis
    k = [np.array(pyrad.getAbsCoef(L)) for L in atm]
    T = [L.T for L in atm]
    terms = [(l, np.array(m.absCoef)) for l, L in enumerate(atm) for m in L]
    paths = [atm.reflectedPath(), atm.reflectedPath(mu=0.4), atm.reflectedPath(observerLevel=2), atm.zenithPath(),
             atm.nadirPath(), pyrad.Path([], [], source="space", bounce=0), atm.limbPath(2.5e4),
             pyrad.Path([1, 0, 0, 2], [3e4, 2e4, 1e4, 7e3], source="surface", bounce=2)]
    e = spectral_emissivity(x)
    got = atm.pathJacobians(paths, surfaceTemperature=295, molecules=True, emissivity=e, reflection="specular")
    want = atm.radiance(paths, surfaceTemperature=295, emissivity=e, reflection="specular")
    assert np.array_equal(got.radiance, want.radiance)
    for r, p in enumerate(paths):
        lay, lens = p._segments()
        ref = surface_path_jacobian_reference(x, k, T, lay, lens, 1 if p.source == "surface" else 0, e, surface_T=295,
                                              terms=terms)
        scale = max(np.max(np.abs(ref["radiance"])), 1e-300)
        spectra_close(got.surfaceTemperature[r], ref["sourceTemperature"], scale, "%d T_s" % r)
        spectra_close(got.emissivity[r], ref["emissivity"], scale, "%d e" % r)
        for l in range(len(atm)):
            if l not in ref["opticalDepth"]:
                assert np.all(got.opticalDepth[r, l] == 0.0) and np.all(got.temperature[r, l] == 0.0)
                assert np.all(got.molecules[l][r] == 0.0)
                continue
            spectra_close(got.opticalDepth[r, l], ref["opticalDepth"][l], scale, "%d ln tau %d" % (r, l))
            spectra_close(got.temperature[r, l], ref["temperature"][l], scale, "%d T %d" % (r, l))
            for m in range(2):
                spectra_close(got.molecules[l][r, m], ref["terms"][2 * l + m], scale, "%d molecule %d of %d" % (r, m, l))
    # 40 mirror paths with molecules are 40 x 18 rows: two chunks, the same bits as each path alone
    many = [atm.reflectedPath(mu=m) for m in np.linspace(1.0, 0.3, 40)]
    a = atm.pathJacobians(many, surfaceTemperature=295, molecules=True, emissivity=e)
    for r in (0, 27, 28, 39):
        b = atm.pathJacobians(many[r], surfaceTemperature=295, molecules=True, emissivity=e)
        for name in ("radiance", "temperature", "opticalDepth", "surfaceTemperature", "emissivity"):
            assert np.array_equal(getattr(a, name)[r], getattr(b, name)[0]), (r, name)
    # channels: every row convolved, the emissivity row among them
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    ch = atm.pathJacobians(paths[:3], surfaceTemperature=295, emissivity=e, instrument=ins)
    full = atm.pathJacobians(paths[:3], surfaceTemperature=295, emissivity=e)
    assert np.array_equal(ch.emissivity, pyrad.convolve(ins, full.emissivity, 600, 610.07))
    assert np.array_equal(ch.opticalDepth[1], pyrad.convolve(ins, full.opticalDepth[1], 600, 610.07))


# ---- 7. refusals of the C entry points -----------------------------------------------------------------------------------
def test_column_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    rs = np.random.RandomState(5)
    L, n = 3, 1027
    k = synthetic_k(rs, L, n)
    nv = 3 + 2 * L + 1
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    jac, st, sT, se = ctx.buffer(nv), ctx.buffer(L * n), ctx.buffer(L * n), ctx.buffer(n)
    src, top, em = (ctx.buffer(n).upload(np.full(n, v)) for v in (0.1, 0.02, 0.8))
    jac_short, n_short, spec_short = ctx.buffer(nv - 1), ctx.buffer(n - 1), ctx.buffer(L * n - 1)
    i64, f64 = lambda v: (C.c_int64 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    nmax, tmax = _native.limit("flux_angles"), _native.limit("jacobian_terms")
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), T=f64([288.0, 250.0, 215.0]),
                depth=f64([1e4, 2e4, 1e4]), lo=600.0, hi=700.0, n=n, I_surface=src.h, surface_T=0.0, I_top=top.h, n_angles=2,
                mu=f64([1.0, 0.5]), weight=f64([1.0, 2.0]), n_bands=1, band_first=i64([0]), band_count=i64([n]),
                emissivity=em.h, emissivity_all=0.5, reflection=0, n_terms=1, term_abs_coef=(C.c_void_p * 1)(kb[1].h),
                term_layer=i32([1]), jac=jac.h, ln_tau=st.h, T_spec=sT.h, e_spec=se.h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_jacobian_surface_dev(*[a[key] for key in good])

    bad = [dict(abs_coef=None), dict(T=None), dict(depth=None), dict(mu=None), dict(weight=None), dict(band_first=None),
           dict(band_count=None), dict(jac=None), dict(n_layers=-1), dict(n_layers=_native.limit("layers_per_column") + 1),
           dict(n=-5), dict(n_angles=0), dict(n_angles=nmax + 1, mu=f64([0.5] * (nmax + 1)), weight=f64([1.0] * (nmax + 1))),
           dict(n_bands=0), dict(n_bands=_native.limit("flux_bands") + 1), dict(I_surface=None, surface_T=0.0),
           dict(band_count=i64([n + 1])), dict(band_first=i64([-1])), dict(band_count=i64([0])),
           dict(T=f64([288.0, 0.0, 215.0])), dict(depth=f64([1e4, -1.0, 1e4])), dict(mu=f64([1.0, 0.0])),
           dict(mu=f64([1.0, 1.5])), dict(weight=f64([1.0, float("inf")])),
           dict(I_surface=n_short.h), dict(abs_coef=(C.c_void_p * L)(kb[0].h, n_short.h, kb[2].h)),
           # the Jacobian's own
           dict(jac=jac_short.h), dict(ln_tau=spec_short.h), dict(T_spec=spec_short.h), dict(n_terms=-1),
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
        assert call(ln_tau=None, T_spec=None, e_spec=None, I_top=None, emissivity=None, reflection=1, n_terms=0,
                    term_abs_coef=None, term_layer=None) == 0
    finally:
        for b in kb + [jac, st, sT, se, src, top, em, jac_short, n_short, spec_short]:
            b.free()


def test_ray_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    rs = np.random.RandomState(3)
    L, n, R = 3, 1027, 2
    k = synthetic_k(rs, L, n)
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    rows = 2 + 2 * 3 + 1 + 2 + 2 * 2 + 1                      # ray 0 crosses 0 1 2, ray 1 crosses 1 2; the term lies in layer 1
    rad, jac, src = ctx.buffer(R * n), ctx.buffer(rows * n), ctx.buffer(n).upload(np.full(n, 0.1))
    em = ctx.buffer(n).upload(np.full(n, 0.8))
    short, jac_short, n_short = ctx.buffer(R * n - 1), ctx.buffer(rows * n - 1), ctx.buffer(n - 1)
    i32, f64 = lambda v: (C.c_int32 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    tmax = _native.limit("jacobian_terms")
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), T=f64([288.0, 250.0, 215.0]), lo=600.0,
                hi=700.0, n=n, n_rays=R, ray_first=i32([0, 4, 6]), seg_layer=i32([0, MARKER, 1, 2, 2, 1]),
                seg_length=f64([1e4, 0.0, 2e4, 1e4, 3e4, 1e4]), source_kind=i32([1, 0]), I_source=src.h, source_T=0.0,
                emissivity=em.h, emissivity_all=0.5, n_terms=1, term_abs_coef=(C.c_void_p * 1)(kb[1].h), term_layer=i32([1]),
                radiance=rad.h, jac=jac.h)
    assert _native.ray_jacobian_rows(L, [0, 4, 6], [0, MARKER, 1, 2, 2, 1], [1], surface=True)[1] == rows

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_ray_jacobian_surface_dev(*[a[key] for key in good])

    bad = [dict(abs_coef=None), dict(T=None), dict(ray_first=None), dict(seg_layer=None), dict(seg_length=None),
           dict(source_kind=None), dict(jac=None), dict(n_layers=0), dict(n=0), dict(n_rays=0),
           dict(ray_first=i32([1, 4, 6])), dict(ray_first=i32([0, 4, 3])),
           dict(seg_layer=i32([0, MARKER, 3, 2, 2, 1])), dict(seg_layer=i32([0, -2, 1, 2, 2, 1])),
           dict(seg_length=f64([1e4, 0.0, -1.0, 1e4, 3e4, 1e4])), dict(seg_length=f64([1e4, 0.0, float("nan"), 1e4, 3e4, 1e4])),
           dict(T=f64([288.0, 0.0, 215.0])), dict(source_kind=i32([2, 0])),
           # a marker with a length; a ray with a marker and no surface source
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
        # the radiance is optional, emissivity_all is not looked at beside a buffer; the context goes on computing
        assert call(radiance=None, emissivity_all=7.0) == 0
        assert np.array_equal(jac.download(), want_J) and np.all(rad.download() == -7.0)
        assert call() == 0
        assert np.array_equal(rad.download(), want_I) and np.array_equal(jac.download(), want_J)
    finally:
        for b in kb + [rad, jac, src, em, short, jac_short, n_short]:
            b.free()
