"""GPU: Atmosphere.fluxes (lbl_column_flux_dev) against a NumPy restatement of its semantics (written out below), against
the existing fold, against analytic limits, and for determinism, laziness and the C ABI's refusals."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import pyrad_oracle as orc
from pyrad_amd import synthetic

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))


@pytest.fixture()
def pyrad():
    from pyrad_amd import model, data, settings
    model.Layer.hasAtmosphere = False
    settings.set_resolution_multiplier(1)
    settings.set_layer_step("merged")
    yield model
    settings.set_layer_step("merged")
    settings.set_resolution_multiplier(1)
    data.set_source(None)


def source(**species_lines):
    from pyrad_amd import data
    return data.set_source(data.synthetic_source(species_lines))


def column(pyrad, rng=(600, 700), layers=LAYERS, co2=400, h2o=0.5):
    atm = pyrad.Atmosphere("col")
    for depth, T, P in layers:
        L = atm.addLayer(depth, T, P, *rng)
        L.addMolecule('co2', ppm=co2)
        L.addMolecule('h2o', percentage=h2o)
    return atm


@pytest.fixture()
def lines():
    source(co2=synthetic.make_lines(51, 800, 580, 720), h2o=synthetic.make_lines(52, 500, 580, 720))


# ---- the semantics, restated in NumPy ----------------------------------------------------------------------------------
def reference(pyrad, atm, mu, weight, surface_T=None, surface=None, top=None, bands=None):
    """(up, down) band fluxes [band, level] and the spectral up flux at the top / down flux at the surface, level by level
    (one grid-sized array per angle in memory, so that the 30-layer column fits)"""
    from pyrad_amd import settings
    x = atm[0].xAxis
    n = x.size
    nl = len(atm)
    k = [np.array(pyrad.getAbsCoef(L)) for L in atm]
    idx = [(0, n)] if bands is None else [(int(np.searchsorted(x, lo)), int(np.searchsorted(x, hi))) for lo, hi in bands]
    res = settings.BASE_RESOLUTION

    def level(I):
        F = sum(w * Ik for w, Ik in zip(weight, I))                   # spectral flux sum_k W_k I_k
        return F, [res * np.sum(np.nan_to_num(F[a:b])) for a, b in idx]

    def step(l, I):
        B = orc.planckWavenumber(x, atm[l].T)
        for i, m in enumerate(mu):
            t = np.exp(-k[l] * atm[l].depth / m)
            I[i] = t * I[i] + (1 - t) * B

    up = np.zeros((len(idx), nl + 1))
    down = np.zeros((len(idx), nl + 1))
    I0 = np.array(surface) if surface is not None else orc.planckWavenumber(x, surface_T)
    I = [I0.copy() for _ in mu]
    F, up[:, 0] = level(I)
    for l in range(nl):
        step(l, I)
        F, up[:, l + 1] = level(I)
    su = F
    IL = np.array(top) if top is not None else np.zeros(n)
    I = [IL.copy() for _ in mu]
    F, down[:, nl] = level(I)
    for l in range(nl - 1, -1, -1):
        step(l, I)
        F, down[:, l] = level(I)
    return up, down, su, F


def heating(pyrad, atm, net):
    return pyrad.heatingRates(net, [L.P for L in atm], [L.T for L in atm], [L.depth for L in atm])


# ---- 1. identity with the existing fold --------------------------------------------------------------------------------
def test_one_vertical_angle_is_the_fold(pyrad, lines):
    atm = column(pyrad)
    f = atm.fluxes(surfaceTemperature=288, angles=[(1.0, np.pi)], spectra=True)
    toa = np.array(atm.transmission(surfaceTemperature=288))
    assert np.array_equal(f.upSpectrum, np.pi * toa)
    assert f.up[-1] == pytest.approx(pyrad.integrateSpectrum(toa), rel=1e-13)
    surf = atm[0].planck(300)
    f = atm.fluxes(surfaceSpectrum=surf, angles=[(1.0, np.pi)], spectra=True)
    toa = np.array(atm.transmission(surfaceSpectrum=surf))
    assert np.array_equal(f.upSpectrum, np.pi * toa)
    assert f.up[-1] == pytest.approx(pyrad.integrateSpectrum(toa), rel=1e-13)


# ---- 2. against NumPy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angles", [1, 3, 8, "diffusivity", [(1.0, 1.0), (0.3, 2.0), (0.75, 0.5)]])
def test_against_numpy(pyrad, lines, angles):
    atm = column(pyrad)
    top = 0.3 * atm[0].planck(250)
    for kw in (dict(), dict(topSpectrum=top)):
        f = atm.fluxes(surfaceTemperature=288, angles=angles, spectra=True, **kw)
        mu, w = pyrad.fluxAngles(angles)
        assert np.array_equal(f.mu, mu) and np.array_equal(f.weight, w)
        fu, fd, su, sd = reference(pyrad, atm, mu, w, surface_T=288, top=kw.get("topSpectrum"))
        assert f.up.shape == f.down.shape == f.net.shape == (len(atm) + 1,) and f.heatingRate.shape == (len(atm),)
        assert rel_err(f.up, fu[0]) <= 1e-12
        assert rel_err(f.down, fd[0], floor=1e-300) <= 1e-12
        assert rel_err(f.net, fu[0] - fd[0]) <= 1e-12
        assert rel_err(f.heatingRate, heating(pyrad, atm, fu[0] - fd[0])) <= 1e-10
        assert rel_err(f.upSpectrum, su) <= 1e-13
        assert rel_err(f.downSpectrum, sd, floor=1e-300) <= 1e-13


# ---- 3. analytic limits ---------------------------------------------------------------------------------------------------
def test_transparent_column(pyrad, lines):
    atm = column(pyrad, co2=0, h2o=0)
    f = atm.fluxes(surfaceTemperature=288)
    want = pyrad.integrateSpectrum(orc.planckWavenumber(atm[0].xAxis, 288), np.pi)
    assert rel_err(f.up, np.full(len(atm) + 1, want)) <= 1e-13
    assert np.all(f.down == 0.0)


def test_isothermal_column(pyrad, lines):
    atm = column(pyrad, layers=tuple((d, 260, P) for d, _, P in LAYERS))
    f = atm.fluxes(surfaceTemperature=260)
    want = pyrad.integrateSpectrum(orc.planckWavenumber(atm[0].xAxis, 260), np.pi)
    assert rel_err(f.up, np.full(len(atm) + 1, want)) <= 1e-13


def test_optically_thick_bottom_layer(pyrad, lines):
    atm = column(pyrad, layers=((1e4, 290, 1013.25),) + LAYERS[1:])
    k0 = np.array(pyrad.getAbsCoef(atm[0]))
    assert np.min(k0) > 0
    atm[0].changeDepth(80.0 / np.min(k0))             # optical depth >= 80 at every point: t < 1e-34 at every angle
    f = atm.fluxes(surfaceTemperature=250)
    want = pyrad.integrateSpectrum(orc.planckWavenumber(atm[0].xAxis, 290), np.pi)
    assert f.down[0] == pytest.approx(want, rel=1e-12)


# ---- 4. bands ---------------------------------------------------------------------------------------------------------------
def test_bands(pyrad, lines):
    atm = column(pyrad, rng=(600, 700.07))           # an odd number of grid points
    x = atm[0].xAxis
    assert x.size % 2 == 1
    edges = [0, 1001, 2502, 2503, 6007, x.size]        # edges at indices not = 0 (mod 4), a single-point band
    bands = [(x[a], x[b] if b < x.size else np.inf) for a, b in zip(edges[:-1], edges[1:])]
    f = atm.fluxes(surfaceTemperature=288, bands=bands, spectra=True)
    whole = atm.fluxes(surfaceTemperature=288, spectra=True)
    mu, w = pyrad.fluxAngles(3)
    fu, fd, su, _ = reference(pyrad, atm, mu, w, surface_T=288, bands=bands)
    assert f.up.shape == (len(bands), len(atm) + 1) and f.heatingRate.shape == (len(bands), len(atm))
    assert rel_err(f.up, fu) <= 1e-12 and rel_err(f.down, fd) <= 1e-12
    assert rel_err(f.up.sum(axis=0), whole.up) <= 1e-13 and rel_err(f.down.sum(axis=0), whole.down) <= 1e-13
    assert rel_err(f.upSpectrum, su) <= 1e-13
    sub = atm.fluxes(surfaceTemperature=288, bands=[bands[1], bands[3]])
    assert rel_err(sub.up, fu[[1, 3]]) <= 1e-12


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------
def test_deterministic(pyrad, lines):
    cold = column(pyrad).fluxes(surfaceTemperature=288, spectra=True)
    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    a = atm.fluxes(surfaceTemperature=288, spectra=True)
    b = atm.fluxes(surfaceTemperature=288, spectra=True)
    for f in (a, b):
        for name in ("up", "down", "net", "heatingRate", "upSpectrum", "downSpectrum"):
            assert np.array_equal(getattr(f, name), getattr(cold, name)), name


# ---- 6. laziness and interleaving ---------------------------------------------------------------------------------------------
def test_interleaving_with_transmission_and_mutators(pyrad, lines):
    from pyrad_amd import settings

    def fresh(T2=270, P3=80.0, d3=1e5):
        layers = list(LAYERS)
        layers[1] = (layers[1][0], T2, layers[1][2])
        layers[3] = (d3, layers[3][1], P3)
        return column(pyrad, layers=tuple(layers))

    def same(f, g, tol=1e-13):
        assert rel_err(f.up, g.up) <= tol and rel_err(f.down, g.down) <= tol
        assert rel_err(f.heatingRate, g.heatingRate) <= 1e-10

    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    atm[1].changeTemperature(250)
    same(atm.fluxes(surfaceTemperature=288), fresh(T2=250).fluxes(surfaceTemperature=288))
    assert rel_err(atm.transmission(surfaceTemperature=288), fresh(T2=250).transmission(surfaceTemperature=288)) <= 1e-13
    atm[3].changePressure(60.0)
    atm[3].changeDepth(2e5)
    same(atm.fluxes(surfaceTemperature=288), fresh(T2=250, P3=60.0, d3=2e5).fluxes(surfaceTemperature=288))
    merged = fresh().fluxes(surfaceTemperature=288, angles=3)
    settings.set_layer_step("per-list")
    try:
        per_list = fresh().fluxes(surfaceTemperature=288, angles=3)
    finally:
        settings.set_layer_step("merged")
    same(per_list, merged, tol=1e-12)


def test_no_accumulate_after_transmission(pyrad, lines, monkeypatch):
    from pyrad_amd import engine
    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    ctx = engine.get_engine().ctx
    jobs = []
    for name in ("layers_merged_accumulate_dev", "layer_merged_step_dev", "xsec_accumulate_dev", "layer_step_dev",
                 "layer_sweep_dev"):
        orig = getattr(ctx, name)
        monkeypatch.setattr(ctx, name, lambda first, *a, _o=orig, _n=name, **kw: (jobs.append((_n, len(first))), _o(first, *a, **kw))[1])
    atm.fluxes(surfaceTemperature=288)
    assert all(count == 0 for _, count in jobs), jobs
    atm[2].changeTemperature(250)                      # one layer due: one job for it alone
    jobs.clear()
    atm.fluxes(surfaceTemperature=288)
    assert jobs == [("layers_merged_accumulate_dev", 1)], jobs


# ---- 7. full size ---------------------------------------------------------------------------------------------------------
def test_config_c5_column(pyrad):
    from pyrad_amd import settings
    cfg = synthetic.config_c5()
    c0 = cfg["layers"][0]
    settings.set_resolution_multiplier(c0["base_resolution"] / .01)
    source(**{m["species"]: m["lines"] for m in c0["molecules"]})
    atm = pyrad.Atmosphere("c5")
    for c in cfg["layers"]:
        L = atm.addLayer(c["depth"], c["T"], c["P"], c["range_min"], c["range_max"], name=c["name"],
                         dynamicResolution=c.get("dynamic_resolution", True))
        for m in c["molecules"]:
            L.addMolecule(m["species"], **m["conc"])
    bands = [(100, 600), (600, 750), (750, 1200), (1200, 2500 + 1)]
    f = atm.fluxes(surfaceTemperature=cfg["surface_T"], angles=3, bands=bands)
    mu, w = pyrad.fluxAngles(3)
    fu, fd, _, _ = reference(pyrad, atm, mu, w, surface_T=cfg["surface_T"], bands=bands)
    assert rel_err(f.up, fu) <= 1e-12 and rel_err(f.down, fd) <= 1e-12
    assert rel_err(f.heatingRate, heating(pyrad, atm, fu - fd)) <= 1e-10


# ---- 8. refusals of the C entry point -----------------------------------------------------------------------------------------
def test_refusals(pyrad, lines):
    from pyrad_amd import _native, engine
    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    ctx = engine.get_engine().ctx
    n = atm[0].xAxis.size
    kb = [L.__dict__["_sweep_state"].bufs["abs_coef"] for L in atm]
    T = [L.T for L in atm]
    d = [L.depth for L in atm]
    level = ctx.buffer(2 * (len(atm) + 1))
    short = ctx.buffer(2 * len(atm))
    spec_short = ctx.buffer(n - 1)
    try:
        args = (kb, T, d, 600, 700, n)
        ctx.column_flux_dev(*args, [1.0], [np.pi], [0], [n], level, surface_T=288.0)       # accepted
        nmax = _native.limit("flux_angles")
        with pytest.raises(_native.LblError) as e:
            ctx.column_flux_dev(*args, [0.5] * (nmax + 1), [1.0] * (nmax + 1), [0], [n], level, surface_T=288.0)
        assert e.value.code == BAD_ARG
        for bad in (dict(level_flux=short), dict(up_top=spec_short)):
            kw = dict(level_flux=level, surface_T=288.0)
            kw.update(bad)
            with pytest.raises(_native.LblError) as e:
                ctx.column_flux_dev(*args, [1.0], [np.pi], [0], [n], **kw)
            assert e.value.code == BAD_ARG
        with pytest.raises(_native.LblError) as e:
            ctx.column_flux_dev(*args, [1.0], [np.pi], [0], [n + 1], level, surface_T=288.0)
        assert e.value.code == BAD_ARG
        ctx.set_option("sweep_ieee_divisions", 1)
        try:
            with pytest.raises(_native.LblError) as e:
                ctx.column_flux_dev(*args, [1.0], [np.pi], [0], [n], level, surface_T=288.0)
            assert e.value.code == BAD_ARG
        finally:
            ctx.set_option("sweep_ieee_divisions", 0)
    finally:
        for b in (level, short, spec_short):
            b.free()
