"""GPU: Atmosphere.pathJacobians (lbl_ray_jacobian_dev, kernel K5f) - the radiance against radiance() bit for bit, every row
against a NumPy restatement with the level radiances stored (written out below), against K5d and observe() for the nadir
view, against finite differences of radiance(), the full temperature Jacobian under the Voigt shape, independence of the
rays, determinism, chunking, the C ABI's refusals and the absence of side effects."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyrad_oracle as orc
from pyrad_amd import synthetic
from test_gpu_paths import LAYERS, nine_paths

pytestmark = pytest.mark.gpu

BAD_ARG = -1
RNG = (600, 610.07)          # 1,007 points (asserted below): three of them go to the tail kernel
T_SURFACE = 295              # (at 288 K the bottom layer's B - I is 0 and its row says nothing)
# Bound of the spectral comparison with NumPy, per point: |got - want| <= RTOL |want| + FLOOR max_j |I_r|.  The floor is
# derived, not measured: the clamped form A B + D carries about 40 S 1e-16 Imax per point for S segments (docstring of
# tests/test_gpu_jacobian.py), 2.8e-14 Imax at the 7 segments of the longest path here; a NumPy run of both forms on a column
# of this shape gave at most 8e-15 max I.  1e-12 is about 35x the derived bound.
RTOL, FLOOR = 1e-9, 1e-12


@pytest.fixture()
def pyrad():
    from pyrad_amd import model, data, settings
    model.Layer.hasAtmosphere = False
    settings.set_resolution_multiplier(1)
    settings.set_layer_step("merged")
    settings.set_line_shape("reference")
    yield model
    settings.set_line_shape("reference")
    settings.set_layer_step("merged")
    settings.set_resolution_multiplier(1)
    data.set_source(None)


@pytest.fixture()
def lines():
    from pyrad_amd import data
    data.set_source(data.synthetic_source(dict(co2=synthetic.make_lines(51, 800, 580, 720),
                                               h2o=synthetic.make_lines(52, 500, 580, 720))))


@pytest.fixture()
def ctx(pyrad):
    from pyrad_amd import engine
    return engine.get_engine().ctx


def column(pyrad, rng=RNG, layers=LAYERS):
    atm = pyrad.Atmosphere("col")
    for depth, T, P in layers:
        L = atm.addLayer(depth, T, P, *rng)
        L.addMolecule('co2', ppm=400)
        L.addMolecule('h2o', percentage=0.5)
    assert len(atm[0].xAxis) % 4 != 0
    return atm


def all_paths(pyrad, atm):
    """the ten paths of tests/test_gpu_paths.py (the last one has no segment), a path from the surface that repeats a layer
    non-adjacently and skips two, and four more nadir cosines: with the two nadir views of the ten, one bundle of four rays
    over the sequence 0 1 2 3 and two left-over single ones"""
    return (nine_paths(pyrad, atm) + [pyrad.Path([1, 1, 0, 1], [3e4, 1e4, 2e4, 5e3], source="surface")]
            + [atm.nadirPath(mu=m) for m in (0.9, 0.7, 0.55, 0.3)])


def planck_dT(x, T):
    """dB/dT = B b e^b / ((e^b - 1) T), b = 100 h c nu / k / T"""
    b = 100 * orc.h * orc.c * x / orc.k / T
    return orc.planckWavenumber(x, T) * b * np.exp(b) / ((np.exp(b) - 1) * T)


# ---- the semantics, restated in NumPy with every level radiance stored --------------------------------------------------------
def path_reference(x, k, T, path, surface, surface_T, terms=()):
    """(radiance, dTs, {layer: d ln tau}, {layer: dT}, {term index: row}) of one path by the direct form A t (B - I_s);
    terms: (layer, k_m) pairs; surface: the source spectrum of a path from the surface"""
    I = [np.array(surface, dtype=np.float64) if path.source == "surface" else np.zeros(x.size)]
    t = []
    with np.errstate(under="ignore"):
        for l, s in zip(path.layers, path.lengths):
            t.append(np.exp(-k[l] * s))
            I.append(t[-1] * I[-1] + (1 - t[-1]) * orc.planckWavenumber(x, T[l]))
        A = np.ones(x.size)
        dtau, dT, rows = {}, {}, {}
        for l in set(path.layers):
            dtau[l], dT[l] = np.zeros(x.size), np.zeros(x.size)
        for m, (l, km) in enumerate(terms):
            if l in dtau:
                rows[m] = np.zeros(x.size)
        for s in range(len(path) - 1, -1, -1):
            l, length = path.layers[s], path.lengths[s]
            core = A * t[s] * (orc.planckWavenumber(x, T[l]) - I[s])
            dtau[l] += k[l] * length * core
            dT[l] += A * (1 - t[s]) * planck_dT(x, T[l])
            for m, (lm, km) in enumerate(terms):
                if lm == l:
                    rows[m] += km * length * core
            A = A * t[s]
    dTs = A * planck_dT(x, surface_T) if path.source == "surface" and surface_T is not None else np.zeros(x.size)
    return I[-1], dTs, dtau, dT, rows


def close(got, want, scale, rtol=RTOL, floor=FLOOR):
    """(worst |got - want| / bound, all inside)"""
    bound = rtol * np.abs(want) + floor * scale
    ratio = np.max(np.abs(got - want) / np.where(bound > 0, bound, 1.0)) if got.size else 0.0
    return ratio, bool(np.all(np.abs(got - want) <= bound))


# ---- 1. the radiance is radiance()'s ---------------------------------------------------------------------------------------------
def test_radiance_bits(pyrad, lines):
    atm = column(pyrad)
    paths = all_paths(pyrad, atm)
    for kw in (dict(surfaceTemperature=T_SURFACE), dict(surfaceSpectrum=atm[0].planck(300))):
        want = atm.radiance(paths, **kw)
        got = atm.pathJacobians(paths, **kw)
        assert got.radiance.shape == (len(paths), len(atm[0].xAxis)) and got.paths == paths
        assert np.array_equal(got.wavenumber, want.wavenumber)
        assert np.array_equal(got.radiance, want.radiance)
        assert (got.surfaceTemperature is None) == ("surfaceSpectrum" in kw)
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    got = atm.pathJacobians(paths, surfaceTemperature=T_SURFACE, instrument=ins)
    want = atm.radiance(paths, surfaceTemperature=T_SURFACE, instrument=ins)
    assert np.array_equal(got.radiance, want.radiance) and np.array_equal(got.wavenumber, ins.centres)
    assert np.array_equal(got.brightnessTemperature, pyrad.brightnessTemperature(ins.centres, want.radiance))


# ---- 2. against NumPy, spectral ----------------------------------------------------------------------------------------------------
def test_against_numpy(pyrad, lines):
    atm = column(pyrad)
    paths = all_paths(pyrad, atm)
    x = atm[0].xAxis
    k = [np.array(pyrad.getAbsCoef(L)) for L in atm]
    T = [L.T for L in atm]
    km = [[np.array(m.absCoef) for m in L] for L in atm]
    terms = [(l, km[l][m]) for l in range(len(atm)) for m in range(len(atm[l]))]
    for kw, surface, Ts in ((dict(surfaceTemperature=T_SURFACE), orc.planckWavenumber(x, T_SURFACE), T_SURFACE),
                            (dict(surfaceSpectrum=atm[0].planck(300)), np.array(atm[0].planck(300)), None)):
        got = atm.pathJacobians(paths, molecules=True, **kw)
        assert got.opticalDepth.shape == got.temperature.shape == (len(paths), len(atm), x.size)
        assert [a.shape for a in got.molecules] == [(len(paths), 2, x.size)] * len(atm)
        assert got.moleculeNames == [["co2", "h2o"]] * len(atm)
        assert got.temperatureAbsorption is None and got.temperatureFull is None and got.brightnessTemperature is None
        bad = []
        for r, p in enumerate(paths):
            I, dTs, dtau, dT, rows = path_reference(x, k, T, p, surface, Ts, terms)
            scale = np.max(np.abs(I))
            worst = 0.0
            ok = True
            if Ts is not None:
                e, inside = close(got.surfaceTemperature[r], dTs, scale)
                worst, ok = max(worst, e), ok and inside
                if p.source == "space":
                    assert np.all(got.surfaceTemperature[r] == 0.0), r
            for l in range(len(atm)):
                mol = got.molecules[l][r]
                if l not in dtau:
                    assert np.all(got.opticalDepth[r, l] == 0.0) and np.all(got.temperature[r, l] == 0.0), (r, l)
                    assert np.all(mol == 0.0), (r, l)
                    continue
                for g, w in ((got.opticalDepth[r, l], dtau[l]), (got.temperature[r, l], dT[l]),
                             (mol[0], rows[2 * l]), (mol[1], rows[2 * l + 1])):
                    e, inside = close(g, w, scale)
                    worst, ok = max(worst, e), ok and inside
            print("ray %d (%s): worst error / bound %.3g, max I %.3e" % (r, p.name, worst, scale))
            if not ok:
                bad.append((r, worst))
        assert not bad, bad


# ---- 3. against K5d and observe() ----------------------------------------------------------------------------------------------------
def test_nadir_against_the_flux_jacobian_and_observe(pyrad, lines):
    atm = column(pyrad)
    got = atm.pathJacobians(atm.nadirPath(), surfaceTemperature=T_SURFACE)
    want = atm.jacobians(surfaceTemperature=T_SURFACE, angles=[(1.0, 1.0)], molecules=False, spectra=True)
    scale = np.max(np.abs(got.radiance[0]))
    for name, g, w in (("opticalDepth", got.opticalDepth[0], want.opticalDepthSpectrum),
                       ("temperature", got.temperature[0], want.temperatureSpectrum)):
        print("%s: bit-equal to K5d: %s, worst |difference| / max I %.2e" % (name, np.array_equal(g, w), np.max(np.abs(g - w)) / scale))
        assert np.all(np.abs(g - w) <= 1e-12 * np.abs(w) + 1e-12 * scale), name
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    got = atm.pathJacobians(atm.nadirPath(), surfaceTemperature=T_SURFACE, instrument=ins)
    ob = atm.observe(ins, surfaceTemperature=T_SURFACE, mu=1, jacobians=True)
    scale = np.max(np.abs(ob.radiance))
    assert np.array_equal(got.radiance[0], ob.radiance)
    for name, g, w in (("temperature", got.temperature[0], ob.temperatureJacobian),
                       ("opticalDepth", got.opticalDepth[0], ob.opticalDepthJacobian),
                       ("brightnessTemperature", got.brightnessTemperatureJacobian[0], ob.brightnessTemperatureJacobian)):
        assert g.shape == w.shape == (len(atm), len(ins))
        print("channels, %s: bit-equal to observe(): %s" % (name, np.array_equal(g, w)))
        assert np.all(np.abs(g - w) <= 1e-12 * np.abs(w) + 1e-12 * scale), name


# ---- 4. finite differences -------------------------------------------------------------------------------------------------------------
def richardson(F, h):
    """(R, |D1 - D2|) from F[-2], F[-1], F[1], F[2] at steps -2h .. 2h"""
    D1, D2 = (F[1] - F[-1]) / (2 * h), (F[2] - F[-2]) / (4 * h)
    return (4 * D1 - D2) / 3, np.abs(D1 - D2)


def test_optical_depth_rows_against_finite_differences(pyrad, lines):
    """d ln tau_l of every ray and crossed layer against R = (4 D1 - D2) / 3, D1 and D2 the central differences of
    radiance() with that layer's segment lengths scaled by exp(+-1e-3) and exp(+-2e-3).  Per point |got - R| <= |D1 - D2| +
    1e-6 |R| + 1e-11 max |I|.  On the CPU restatement every ray and layer stayed below 0.04 of that bound while the
    Jacobian is about 1e5 times it; that the bound is small against the Jacobian is asserted per ray for its most
    sensitive layer (at least 1e3 times the bound: an error of a thousandth of a row would show)."""
    atm = column(pyrad)
    paths = all_paths(pyrad, atm)
    got = atm.pathJacobians(paths, surfaceTemperature=T_SURFACE, molecules=True)
    h = 1e-3
    jobs, moved = [], []
    for r, p in enumerate(paths):
        for l in sorted(set(p.layers)):
            for d in (-2, -1, 1, 2):
                f = np.exp(d * h)
                moved.append(pyrad.Path(p.layers, [x * f if pl == l else x for pl, x in zip(p.layers, p.lengths)], source=p.source))
                jobs.append((r, l, d))
    assert len(moved) <= 512
    I = atm.radiance(moved, surfaceTemperature=T_SURFACE).radiance
    F = {job: I[i] for i, job in enumerate(jobs)}
    for r, p in enumerate(paths):
        scale = np.max(np.abs(got.radiance[r]))
        sharpest = 0.0
        for l in sorted(set(p.layers)):
            R, dD = richardson({d: F[(r, l, d)] for d in (-2, -1, 1, 2)}, h)
            bound = dD + 1e-6 * np.abs(R) + 1e-11 * scale
            err = np.abs(got.opticalDepth[r, l] - R)
            sharpest = max(sharpest, np.max(np.abs(got.opticalDepth[r, l])) / np.max(bound))
            print("ray %d layer %d: worst error / bound %.3g, max |row| / max bound %.3g" % (
                r, l, np.max(err / bound), np.max(np.abs(got.opticalDepth[r, l])) / np.max(bound)))
            assert np.all(err <= bound), (r, l, float(np.max(err / bound)))
            # the molecules of the layer add up to the layer (K5d's precedent)
            total = got.molecules[l][r].sum(axis=0)
            assert np.all(np.abs(total - got.opticalDepth[r, l]) <= 1e-10 * np.abs(got.opticalDepth[r, l]) + 1e-12 * scale), (r, l)
        if len(p):
            assert sharpest >= 1e3, (r, sharpest)


def test_temperature_rows_against_finite_differences(pyrad, lines, ctx):
    """dI/dT_l (Planck part) the same way: lbl_ray_radiance_dev with T[l] +- 0.01 K and +- 0.02 K over the same coefficient
    buffers; per point |got - R| <= |D1 - D2| + 1e-6 |R| + 1e-11 max |I|"""
    atm = column(pyrad)
    paths = all_paths(pyrad, atm)
    got = atm.pathJacobians(paths, surfaceTemperature=T_SURFACE)
    n = len(atm[0].xAxis)
    bufs = [ctx.buffer(n).upload(np.array(pyrad.getAbsCoef(L))) for L in atm]
    rad = ctx.buffer(len(paths) * n)
    ray_first = np.cumsum([0] + [len(p) for p in paths])
    T0 = [float(L.T) for L in atm]
    h = 0.01
    try:
        for l in range(len(atm)):
            F = {}
            for d in (-2, -1, 1, 2):
                T = list(T0)
                T[l] += d * h
                ctx.ray_radiance_dev(bufs, T, RNG[0], RNG[1], n, ray_first, [x for p in paths for x in p.layers],
                                     [x for p in paths for x in p.lengths], [pyrad.Path.SOURCES.index(p.source) for p in paths],
                                     rad, source_T=float(T_SURFACE))
                F[d] = rad.download().reshape(len(paths), n)
            R, dD = richardson(F, h)
            for r, p in enumerate(paths):
                scale = np.max(np.abs(got.radiance[r]))
                bound = dD[r] + 1e-6 * np.abs(R[r]) + 1e-11 * scale
                err = np.abs(got.temperature[r, l] - R[r])
                print("ray %d layer %d: worst error / bound %.3g, max |row| / max bound %.3g" % (
                    r, l, np.max(err / bound), np.max(np.abs(got.temperature[r, l])) / np.max(bound)))
                assert np.all(err <= bound), (r, l, float(np.max(err / bound)))
                if l not in p.layers:
                    assert np.all(R[r] == 0.0) and np.all(got.temperature[r, l] == 0.0)
    finally:
        for b in bufs + [rad]:
            b.free()


# ---- 5. the full temperature Jacobian under the Voigt shape ------------------------------------------------------------------------------
def test_full_temperature_against_finite_differences(pyrad):
    """temperatureFull of a limb and a nadir path in one boxcar channel over the range against Richardson differences of
    radiance(..., instrument=...) under changeTemperature(T +- 1, +- 2): |got - R| <= |D1 - D2| + 1e-6 |R|, as test 7 of
    tests/test_gpu_voigt_dT.py has it for the flux, on its 3-layer column."""
    from pyrad_amd import data, settings
    from test_gpu_voigt_dT import LAYERS as LAYERS_V, LO, HI
    settings.set_line_shape("voigt")
    data.set_source(data.synthetic_source(dict(co2=synthetic.make_lines(41, 150, 590, 615),
                                               h2o=synthetic.make_lines(42, 150, 590, 615))))
    atm = column(pyrad, rng=(LO, HI + 0.03), layers=LAYERS_V)
    paths = [atm.limbPath(1.5e4), atm.nadirPath()]
    ins = pyrad.Instrument([0.5 * (LO + HI)], shape="boxcar", width=HI - LO - 0.5)
    kw = dict(surfaceTemperature=288, instrument=ins)
    planck = atm.pathJacobians(paths, **kw)
    full = atm.pathJacobians(paths, temperature="full", **kw)
    assert planck.temperatureAbsorption is None and planck.temperatureFull is None
    for name in ("radiance", "temperature", "opticalDepth", "surfaceTemperature", "brightnessTemperatureJacobian"):
        assert np.array_equal(getattr(full, name), getattr(planck, name)), name
    assert full.temperatureAbsorption.shape == full.temperature.shape == (2, 3, 1)
    assert np.array_equal(full.temperatureFull, full.temperature + full.temperatureAbsorption)
    spectral = atm.pathJacobians(paths, temperature="full", molecules=True, surfaceTemperature=288)
    assert spectral.temperatureFull.shape == (2, 3, len(atm[0].xAxis)) and len(spectral.molecules) == 3
    assert np.all(spectral.temperatureAbsorption[0, 0] == 0.0)           # the limb path stays above layer 0
    told_apart = False
    for l, (L, (_, T, _)) in enumerate(zip(atm, LAYERS_V)):
        F = {}
        for d in (-2, -1, 1, 2):
            L.changeTemperature(T + d)
            F[d] = atm.radiance(paths, **kw).radiance
        L.changeTemperature(T)
        R, dD = richardson(F, 1.0)
        for r in range(len(paths)):
            err = abs(full.temperatureFull[r, l, 0] - R[r, 0])
            print("path %d layer %d: full %.9e, Planck part %.9e, differences %.9e, |err| %.2e, |D1 - D2| %.2e"
                  % (r, l, full.temperatureFull[r, l, 0], full.temperature[r, l, 0], R[r, 0], err, dD[r, 0]))
            assert err <= dD[r, 0] + 1e-6 * abs(R[r, 0]), (r, l, err, dD[r, 0])
            told_apart = told_apart or abs(full.temperatureAbsorption[r, l, 0]) > 10 * dD[r, 0]
    assert told_apart, "the column cannot tell the full Jacobian from its Planck part"


# ---- 6. independence, determinism and chunking ------------------------------------------------------------------------------------------
FIELDS = ("radiance", "temperature", "opticalDepth", "surfaceTemperature")


def same(a, r, b, s):
    return (all(np.array_equal(getattr(a, f)[r], getattr(b, f)[s]) for f in FIELDS)
            and all(np.array_equal(x[r], y[s]) for x, y in zip(a.molecules, b.molecules)))


def test_rays_are_independent_and_calls_deterministic(pyrad, lines):
    atm = column(pyrad)
    paths = all_paths(pyrad, atm)
    kw = dict(surfaceTemperature=T_SURFACE, molecules=True)
    a = atm.pathJacobians(paths, **kw)
    b = atm.pathJacobians(paths, **kw)
    rev = atm.pathJacobians(paths[::-1], **kw)
    R = len(paths)
    for r in range(R):
        assert same(a, r, b, r), r
        assert same(a, r, rev, R - 1 - r), r
        assert same(a, r, atm.pathJacobians(paths[r], **kw), 0), r
    # rays 0, 1, 11, 12 travel as a bundle in the call above; here ray 12 leads a bundle of other companions
    band = atm.pathJacobians([paths[12], atm.nadirPath(mu=0.8), atm.nadirPath(mu=0.2), paths[0], paths[13]], **kw)
    assert same(a, 12, band, 0) and same(a, 0, band, 3) and same(a, 13, band, 4)


def test_chunks_give_the_same_bits(pyrad, lines):
    from pyrad_amd import _native as nat
    atm = column(pyrad)
    paths = all_paths(pyrad, atm)
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    kw = dict(surfaceTemperature=T_SURFACE, molecules=True, instrument=ins)
    whole = atm.pathJacobians(paths, **kw)
    spectral = atm.pathJacobians(paths, surfaceTemperature=T_SURFACE, molecules=True)
    keep = nat.limit
    for rows in (40, 8):               # 17 rows for a nadir ray with its 8 molecule terms: several chunks; one ray beyond a block
        nat.limit = lambda name: rows if name == "ils_rows" else keep(name)
        try:
            chunked = atm.pathJacobians(paths, **kw)
            chunked_spectral = atm.pathJacobians(paths, surfaceTemperature=T_SURFACE, molecules=True)
        finally:
            nat.limit = keep
        for r in range(len(paths)):
            assert same(whole, r, chunked, r), (rows, r)
            assert same(spectral, r, chunked_spectral, r), (rows, r)
        assert np.array_equal(whole.brightnessTemperatureJacobian, chunked.brightnessTemperatureJacobian, equal_nan=True)
    assert sum(1 + 2 * len(set(p.layers)) + 2 * len(set(p.layers)) for p in paths) >= 3 * 40


# ---- 7. refusals of the C entry point -------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from pyrad_amd import _native
    from test_gpu_paths import synthetic_k
    lib = ctx.lib
    rs = np.random.RandomState(5)
    L, n, R = 3, 1027, 2
    k = synthetic_k(rs, L, n)
    T = [288.0, 250.0, 215.0]
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    tb = [ctx.buffer(n).upload(0.5 * k[1]), ctx.buffer(n).upload(0.25 * k[0])]
    rows = 7 + 5 + 2 + 1                               # ray 0 crosses 0 1 2 and both terms, ray 1 crosses 2 1 and one term
    rad, jac, src = ctx.buffer(R * n), ctx.buffer(rows * n), ctx.buffer(n).upload(np.full(n, 0.1))
    short, rad_short, t_short = ctx.buffer(rows * n - 1), ctx.buffer(R * n - 1), ctx.buffer(n - 1)
    i32, f64 = lambda v: (C.c_int32 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    ptrs = lambda bs: (C.c_void_p * max(len(bs), 1))(*[b.h if b is not None else None for b in bs])
    many = _native.limit("jacobian_terms") + 1
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=ptrs(kb), T=f64(T), lo=600.0, hi=700.0, n=n, n_rays=R,
                ray_first=i32([0, 3, 5]), seg_layer=i32([0, 1, 2, 2, 1]), seg_length=f64([1e4, 2e4, 1e4, 3e4, 1e4]),
                source_kind=i32([1, 0]), I_source=src.h, source_T=0.0, n_terms=2, term_abs_coef=ptrs(tb),
                term_layer=i32([1, 0]), radiance=rad.h, jac=jac.h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_ray_jacobian_dev(*[a[key] for key in good])

    bad = [dict(n_terms=-1), dict(n_terms=many, term_abs_coef=ptrs(tb * many), term_layer=i32([0] * many)),
           dict(term_abs_coef=None), dict(term_layer=None), dict(term_abs_coef=ptrs([tb[0], None])),
           dict(term_layer=i32([1, 3])), dict(term_layer=i32([-1, 0])), dict(term_abs_coef=ptrs([tb[0], t_short])),
           dict(jac=None), dict(jac=short.h), dict(radiance=rad_short.h),
           # what lbl_ray_radiance_dev refuses
           dict(abs_coef=None), dict(T=None), dict(ray_first=None), dict(seg_layer=None), dict(seg_length=None),
           dict(source_kind=None), dict(n_layers=0), dict(n=0), dict(n_rays=0), dict(ray_first=i32([1, 3, 5])),
           dict(ray_first=i32([0, 3, 2])), dict(seg_layer=i32([0, 1, 3, 2, 1])), dict(seg_length=f64([1e4, -1.0, 1e4, 3e4, 1e4])),
           dict(T=f64([288.0, 0.0, 215.0])), dict(source_kind=i32([2, 0])), dict(I_source=None, source_T=0.0)]
    try:
        assert call() == 0
        want_I, want_J = rad.download(), jac.download()
        rad.upload(np.full(R * n, -7.0))
        jac.upload(np.full(rows * n, -7.0))
        assert lib.lbl_ray_jacobian_dev(None, *[good[key] for key in list(good)[1:]]) == BAD_ARG
        for kw in bad:
            assert call(**kw) == BAD_ARG, sorted(kw)
            assert lib.lbl_last_error(ctx.h), sorted(kw)
        ctx.set_option("sweep_ieee_divisions", 1)
        try:
            assert call() == BAD_ARG
            assert b"sweep_ieee_divisions" in lib.lbl_last_error(ctx.h)
        finally:
            ctx.set_option("sweep_ieee_divisions", 0)
        # rows x n beyond int64 cannot be reached with buffers that exist: jac == short covers the size check
        assert np.all(rad.download() == -7.0) and np.all(jac.download() == -7.0)
        # the context goes on computing: the same bits; without a radiance output; without terms
        assert call() == 0
        assert np.array_equal(rad.download(), want_I) and np.array_equal(jac.download(), want_J)
        jac.upload(np.full(rows * n, -7.0))
        assert call(radiance=None) == 0 and np.array_equal(jac.download(), want_J)
        jac.upload(np.full(rows * n, -7.0))
        assert call(n_terms=0, term_abs_coef=None, term_layer=None) == 0
        lean = jac.download()
        assert np.array_equal(lean[:7 * n], want_J[:7 * n])                       # ray 0 without its two term rows
        assert np.array_equal(lean[7 * n:12 * n], want_J[9 * n:14 * n])           # ray 1 without its one
        assert np.all(lean[12 * n:] == -7.0)
        # and the values are the semantics': ray 0 against NumPy
        x = np.linspace(600.0, 700.0, n)
        path = type("P", (), dict(layers=(0, 1, 2), lengths=(1e4, 2e4, 1e4), source="surface", __len__=lambda self: 3))()
        I, dTs, dtau, dT, trow = path_reference(x, k, T, path, np.full(n, 0.1), None, [(1, 0.5 * k[1]), (0, 0.25 * k[0])])
        J = want_J.reshape(rows, n)
        scale = np.max(np.abs(I))
        assert np.all(J[0] == 0.0)
        for l in range(3):
            assert close(J[1 + l], dtau[l], scale)[1] and close(J[4 + l], dT[l], scale)[1], l
        assert close(J[7], trow[0], scale)[1] and close(J[8], trow[1], scale)[1]
    finally:
        for b in kb + tb + [rad, jac, src, short, rad_short, t_short]:
            b.free()


def test_model_refuses_the_ieee_sweeps(pyrad, lines, ctx):
    atm = column(pyrad)
    ctx.set_option("sweep_ieee_divisions", 1)
    try:
        with pytest.raises(ValueError, match="sweep_ieee_divisions"):
            atm.pathJacobians(atm.nadirPath(), surfaceTemperature=T_SURFACE)
    finally:
        ctx.set_option("sweep_ieee_divisions", 0)


# ---- 8. no side effects -------------------------------------------------------------------------------------------------------------------
def test_no_side_effects(pyrad, lines):
    atm = column(pyrad)
    paths = all_paths(pyrad, atm)

    def results():
        j = atm.jacobians(surfaceTemperature=T_SURFACE, spectra=True)
        r = atm.radiance(paths, surfaceTemperature=T_SURFACE, transmittance=True)
        return ([np.array(atm.transmission(surfaceTemperature=T_SURFACE)), r.radiance, r.transmittance, j.olr, j.temperature,
                 j.opticalDepth, j.surfaceTemperature, j.temperatureSpectrum, j.opticalDepthSpectrum] + list(j.molecules))

    before = results()
    atm.pathJacobians(paths, surfaceTemperature=T_SURFACE, molecules=True)
    atm.pathJacobians(paths, surfaceSpectrum=atm[0].planck(300),
                      instrument=pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5))
    after = results()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
