"""GPU: Atmosphere.jacobians (lbl_column_jacobian_dev) against the NumPy restatement of its semantics (test_jacobian_cpu.py),
against finite differences through the public and ctypes surfaces, against identities, and for determinism, laziness, the
absence of side effects and the C ABI's refusals.

Tolerances.  The kernel evaluates A_lk t_lk (B_l - I_lk) as A_lk B_l + E_lk - I_Lk, clamped to [-A_lk t_lk Imax_k,
A_lk t_lk B_l].  The unclamped difference carries the rounding of E and I_L, a few ulp of I_L per layer (about L 1e-16 I_L),
which d ln tau multiplies by tau / mu.  Where tau / mu is large the clamp bounds the value by A t max(B, Imax) (tau / mu),
and x e^-x stays below 0.37: the error per point is at most about 40 L 1e-16 Imax, i.e. about 1e-13 of the point's own
outgoing radiance for a handful of layers.  Summed over a band that stays below 1e-12 x olr: the absolute floor below."""
import numpy as np
import pytest

from oracle import pyrad_oracle as orc
from pyrad_amd import synthetic
from test_jacobian_cpu import jacobian_reference

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
FLOOR = 1e-12         # x olr of the band (see the module docstring)


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


def band_idx(x, bands):
    return None if bands is None else [(int(np.searchsorted(x, lo)), int(np.searchsorted(x, hi))) for lo, hi in bands]


def reference(pyrad, atm, mu, w, surface_T=None, surface=None, bands=None):
    from pyrad_amd import settings
    x = atm[0].xAxis
    k = [np.array(pyrad.getAbsCoef(L)) for L in atm]
    terms = [(l, np.array(pyrad.getAbsCoef(m))) for l, L in enumerate(atm) for m in L]
    return jacobian_reference(x, k, [L.T for L in atm], [L.depth for L in atm], mu, w, surface_T=surface_T,
                              surface=surface, terms=terms, idx=band_idx(x, bands), res=settings.BASE_RESOLUTION)


def check(got, want, olr, rel=1e-9, what=""):
    """|got - want| <= rel |want| + FLOOR olr, olr broadcast over the band axis"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    olr = np.asarray(olr, dtype=np.float64).reshape(np.shape(olr) + (1,) * (want.ndim - np.ndim(olr)))
    bad = np.abs(got - want) > rel * np.abs(want) + FLOOR * np.abs(olr)
    assert not bad.any(), (what, got[bad], want[bad])


def molecules_array(j):
    return np.stack([np.asarray(m) for m in j.molecules], axis=-2)          # [..., layer, molecule]


# ---- 1. against NumPy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angles", [1, 3, "diffusivity", [(1.0, 1.0), (0.3, 2.0)]])
@pytest.mark.parametrize("banded", [False, True])
def test_against_numpy(pyrad, lines, angles, banded):
    atm = column(pyrad, rng=(600, 700.07))
    x = atm[0].xAxis
    bands = None
    if banded:
        edges = [0, 1001, 2502, 2503, 6007, x.size]    # edges at indices not = 0 (mod 4), a single-point band
        bands = [(x[a], x[b] if b < x.size else np.inf) for a, b in zip(edges[:-1], edges[1:])]
    mu, w = pyrad.fluxAngles(angles)
    for kw in (dict(surfaceTemperature=288), dict(surfaceSpectrum=0.9 * atm[0].planck(295))):
        j = atm.jacobians(angles=angles, bands=bands, spectra=True, **kw)
        ref = reference(pyrad, atm, mu, w, surface_T=kw.get("surfaceTemperature"), surface=kw.get("surfaceSpectrum"),
                        bands=bands)
        sq = (lambda a: a[0]) if bands is None else (lambda a: a)
        olr = sq(ref["olr"])
        assert np.array_equal(j.mu, mu) and np.array_equal(j.weight, w)
        check(j.olr, olr, olr, rel=1e-12, what="olr")
        if "surfaceTemperature" in kw:
            check(j.surfaceTemperature, sq(ref["surfaceTemperature"]), olr, what="T_s")
        else:
            assert j.surfaceTemperature is None
        check(j.opticalDepth, sq(ref["opticalDepth"]), olr, what="ln tau")
        check(j.temperature, sq(ref["temperature"]), olr, what="T")
        check(molecules_array(j), sq(ref["terms"]).reshape(np.shape(olr) + (len(atm), 2)), olr, what="molecules")
        assert j.moleculeNames == [["co2", "h2o"]] * len(atm)
        # spectra: per point, floor against the point's own spectral olr scale
        res = x[1] - x[0]
        scale = np.max(np.abs(ref["olr"])) / (res * x.size)
        for name in ("opticalDepthSpectrum", "temperatureSpectrum"):
            got, want = getattr(j, name), ref[name]
            assert got.shape == (len(atm), x.size)
            assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want) + 1e-11 * scale), name


# ---- 2. finite differences through the public and ctypes surfaces -------------------------------------------------------
def test_finite_differences(pyrad, lines):
    from pyrad_amd import engine, settings
    atm = column(pyrad)
    Ts = 288.0
    mu, w = pyrad.fluxAngles(3)
    j = atm.jacobians(surfaceTemperature=Ts, angles=3)
    olr = j.olr
    ctx = engine.get_engine().ctx
    n = atm[0].xAxis.size
    res = settings.BASE_RESOLUTION

    def near(a, fd, what):
        assert abs(a - fd) <= 1e-6 * abs(a) + 1e-10 * olr, (what, a, fd)

    eps, h = 1e-4, 1e-2
    for l, L in enumerate(atm):
        d0 = L.depth
        L.changeDepth(d0 * np.exp(eps))
        fp = atm.fluxes(surfaceTemperature=Ts).up[-1]
        L.changeDepth(d0 * np.exp(-eps))
        fm = atm.fluxes(surfaceTemperature=Ts).up[-1]
        L.changeDepth(d0)
        near(j.opticalDepth[l], (fp - fm) / (2 * eps), "ln tau %d" % l)
    kb = [L.__dict__["_sweep_state"].bufs["abs_coef"] for L in atm]
    T = [L.T for L in atm]
    d = [L.depth for L in atm]
    level = ctx.buffer(2 * (len(atm) + 1))
    kbuf = ctx.buffer(n)
    try:
        def top(kbufs, TT):
            ctx.column_flux_dev(kbufs, TT, d, 600, 700, n, mu, w, [0], [n], level, surface_T=Ts)
            return level.download(2 * (len(atm) + 1))[len(atm)] * res
        for l in range(len(atm)):
            Tp, Tm = list(T), list(T)
            Tp[l] += h
            Tm[l] -= h
            near(j.temperature[l], (top(kb, Tp) - top(kb, Tm)) / (2 * h), "T %d" % l)
        for l, L in enumerate(atm):
            kl = np.array(pyrad.getAbsCoef(L))
            for m, mol in enumerate(L):
                km = np.array(pyrad.getAbsCoef(mol))
                fs = []
                for sgn in (1, -1):
                    kbuf.upload(kl + sgn * eps * km)
                    fs.append(top([kbuf if i == l else kb[i] for i in range(len(atm))], T))
                near(j.molecules[l][m], (fs[0] - fs[1]) / (2 * eps), "molecule %d of layer %d" % (m, l))
    finally:
        level.free()
        kbuf.free()
    fp = atm.fluxes(surfaceTemperature=Ts + h).up[-1]
    fm = atm.fluxes(surfaceTemperature=Ts - h).up[-1]
    near(j.surfaceTemperature, (fp - fm) / (2 * h), "T_s")


# ---- 3. identities -----------------------------------------------------------------------------------------------------------
def test_molecules_add_up_to_the_layer(pyrad, lines):
    atm = column(pyrad)
    j = atm.jacobians(surfaceTemperature=288, bands=[(600, 650), (650, 701)])
    for l in range(len(atm)):
        s = np.asarray(j.molecules[l]).sum(axis=-1)
        assert np.all(np.abs(s - j.opticalDepth[:, l]) <= 1e-10 * np.abs(j.opticalDepth[:, l]) + FLOOR * j.olr), l


def test_isothermal_column(pyrad, lines):
    atm = column(pyrad, layers=tuple((d, 260, P) for d, _, P in LAYERS))
    j = atm.jacobians(surfaceTemperature=260)
    assert np.all(np.abs(j.opticalDepth) <= FLOOR * j.olr), j.opticalDepth
    assert np.all(np.abs(molecules_array(j)) <= FLOOR * j.olr)


def test_opaque_top_layer_hides_the_layers_below(pyrad, lines):
    atm = column(pyrad, layers=LAYERS[1:] + ((1e4, 290, 1013.25),))      # (broad lines on top: k > 0 at every point)
    kt = np.array(pyrad.getAbsCoef(atm[-1]))
    assert np.min(kt) > 0
    atm[-1].changeDepth(80.0 / np.min(kt))             # optical depth >= 80 at every point: t < 1e-34 at every angle
    j = atm.jacobians(surfaceTemperature=300)
    below = slice(0, len(atm) - 1)
    for v in (j.opticalDepth[below], j.temperature[below], molecules_array(j)[below], j.surfaceTemperature):
        assert np.all(np.abs(v) <= FLOOR * j.olr), v
    assert abs(j.temperature[-1]) > 1e-3 * j.olr / 288      # the top layer itself emits


def test_single_layer_closed_form(pyrad, lines):
    from pyrad_amd import settings
    atm = column(pyrad, layers=LAYERS[1:2])
    x = atm[0].xAxis
    k = np.array(pyrad.getAbsCoef(atm[0]))
    Ts, T, d = 295.0, atm[0].T, atm[0].depth
    mu, w = pyrad.fluxAngles(3)
    j = atm.jacobians(surfaceTemperature=Ts, angles=3)
    B, Bs = orc.planckWavenumber(x, T), orc.planckWavenumber(x, Ts)
    from test_jacobian_cpu import planck_dT
    res = settings.BASE_RESOLUTION
    olr = dtau = dT = dTs = 0.0
    for m, wk in zip(mu, w):
        t = np.exp(-k * d / m)
        olr += res * np.sum(wk * (t * Bs + (1 - t) * B))
        dtau += res * np.sum(wk * (k * d / m) * t * (B - Bs))
        dT += res * np.sum(wk * (1 - t) * planck_dT(x, T))
        dTs += res * np.sum(wk * t * planck_dT(x, Ts))
    check(j.olr, olr, olr, rel=1e-12)
    check(j.opticalDepth[0], dtau, olr)
    check(j.temperature[0], dT, olr)
    check(j.surfaceTemperature, dTs, olr)


# ---- 4. olr and determinism ---------------------------------------------------------------------------------------------------
def test_olr_is_the_flux_and_calls_repeat_bit_for_bit(pyrad, lines):
    atm = column(pyrad)
    for angles in (1, 3, 8):
        f = atm.fluxes(surfaceTemperature=288, angles=angles, bands=[(600, 640), (640, 701)])
        a = atm.jacobians(surfaceTemperature=288, angles=angles, bands=[(600, 640), (640, 701)], spectra=True)
        b = atm.jacobians(surfaceTemperature=288, angles=angles, bands=[(600, 640), (640, 701)], spectra=True)
        assert np.all(np.abs(a.olr - f.up[:, -1]) <= 1e-13 * f.up[:, -1])
        for name in ("olr", "surfaceTemperature", "temperature", "opticalDepth", "temperatureSpectrum",
                     "opticalDepthSpectrum"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert all(np.array_equal(p, q) for p, q in zip(a.molecules, b.molecules))


# ---- 5. laziness ------------------------------------------------------------------------------------------------------------------
def _count_jobs(ctx, monkeypatch):
    jobs = []
    for name in ("layers_merged_accumulate_dev", "layer_merged_step_dev", "xsec_accumulate_dev", "layer_step_dev",
                 "layer_sweep_dev"):
        orig = getattr(ctx, name)
        monkeypatch.setattr(ctx, name, lambda first, *a, _o=orig, _n=name, **kw: (jobs.append((_n, len(first))), _o(first, *a, **kw))[1])
    return jobs


def test_no_accumulate_when_resident(pyrad, lines, monkeypatch):
    from pyrad_amd import engine
    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    jobs = _count_jobs(engine.get_engine().ctx, monkeypatch)
    atm.jacobians(surfaceTemperature=288, molecules=False)
    assert all(count == 0 for _, count in jobs), jobs
    atm.jacobians(surfaceTemperature=288)                # the molecule terms: one job per (layer, molecule)
    assert sum(c for _, c in jobs) == 2 * len(atm), jobs
    jobs.clear()
    atm.jacobians(surfaceTemperature=288, angles=1)
    assert all(count == 0 for _, count in jobs), jobs
    atm[2].changeTemperature(250)                      # one layer due: its layer job, then its two molecule jobs
    jobs.clear()
    atm.fluxes(surfaceTemperature=288)
    atm.jacobians(surfaceTemperature=288)
    assert jobs == [("layers_merged_accumulate_dev", 1), ("layers_merged_accumulate_dev", 0),
                    ("layers_merged_accumulate_dev", 2)], jobs


# ---- 6. no side effects --------------------------------------------------------------------------------------------------------
def test_no_side_effects(pyrad, lines):
    def results(atm):
        f = atm.fluxes(surfaceTemperature=288, spectra=True)
        return [np.array(atm.transmission(surfaceTemperature=288)), f.up, f.down, f.upSpectrum, f.downSpectrum,
                np.array(pyrad.getAbsCoef(atm[1])), np.array(pyrad.getTransmittance(atm[2]))]

    def same(a, b):
        assert all(np.array_equal(p, q) for p, q in zip(a, b))

    atm, twin = column(pyrad), column(pyrad)
    before = results(atm)
    same(before, results(twin))
    atm.jacobians(surfaceTemperature=288, spectra=True)
    same(results(atm), before)
    for a in (atm, twin):
        a[1].changeTemperature(250)
    after = results(atm)
    same(after, results(twin))
    layers = list(LAYERS)
    layers[1] = (layers[1][0], 250, layers[1][2])
    fresh = results(column(pyrad, layers=tuple(layers)))
    for p, q in zip(after, fresh):
        assert np.all(np.abs(p - q) <= 1e-13 * np.max(np.abs(q)))


# ---- 7. full size ------------------------------------------------------------------------------------------------------------------
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
    Ts = cfg["surface_T"]
    f = atm.fluxes(surfaceTemperature=Ts, angles=3, bands=bands)
    j = atm.jacobians(surfaceTemperature=Ts, angles=3, bands=bands, spectra=True)
    assert len(atm) == 30 and all(len(L) == 3 for L in atm)
    assert np.all(np.abs(j.olr - f.up[:, -1]) <= 1e-13 * f.up[:, -1])
    for l in range(len(atm)):
        s = np.asarray(j.molecules[l]).sum(axis=-1)
        assert np.all(np.abs(s - j.opticalDepth[:, l]) <= 1e-10 * np.abs(j.opticalDepth[:, l]) + FLOOR * j.olr), l
    x = atm[0].xAxis
    res = settings.BASE_RESOLUTION
    for b, (i0, i1) in enumerate(band_idx(x, bands)):
        for name, field in (("opticalDepthSpectrum", "opticalDepth"), ("temperatureSpectrum", "temperature")):
            s = res * np.sum(np.nan_to_num(getattr(j, name)[:, i0:i1]), axis=-1)
            got = getattr(j, field)[b]
            assert np.all(np.abs(s - got) <= 1e-12 * np.abs(got) + FLOOR * j.olr[b]), (name, b)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(pyrad, lines):
    from pyrad_amd import _native, engine
    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    for bad in dict(angles=9), dict(angles=[(0.0, 1.0)]), dict(bands=[(500, 650)]), dict(bands=[]):
        with pytest.raises(ValueError):
            atm.jacobians(surfaceTemperature=288, **bad)
    ctx = engine.get_engine().ctx
    n = atm[0].xAxis.size
    nl = len(atm)
    kb = [L.__dict__["_sweep_state"].bufs["abs_coef"] for L in atm]
    T = [L.T for L in atm]
    d = [L.depth for L in atm]
    nv = 2 + 2 * nl + 1
    jac = ctx.buffer(nv)
    short = ctx.buffer(nv - 1)
    spec_short = ctx.buffer(nl * n - 1)
    try:
        args = (kb, T, d, 600, 700, n)
        ok = dict(surface_T=288.0, term_abs_coef=[kb[0]], term_layer=[0])
        ctx.column_jacobian_dev(*args, [1.0], [np.pi], [0], [n], jac, **ok)            # accepted
        jac.fill(7.0)

        def refused(*a, **kw):
            with pytest.raises(_native.LblError) as e:
                ctx.column_jacobian_dev(*a, **kw)
            assert e.value.code == BAD_ARG
            assert np.all(jac.download(nv) == 7.0)                                        # nothing enqueued

        nmax = _native.limit("flux_angles")
        refused(*args, [0.5] * (nmax + 1), [1.0] * (nmax + 1), [0], [n], jac, **ok)
        refused(*args, [1.5], [1.0], [0], [n], jac, **ok)
        refused(*args, [1.0], [np.pi], [0], [n + 1], jac, **ok)
        refused(*args, [1.0], [np.pi], [0] * 65, [1] * 65, jac, **ok)
        refused(*args, [1.0], [np.pi], [0], [n], short, **ok)
        refused(*args, [1.0], [np.pi], [0], [n], None, **ok)
        refused(*args, [1.0], [np.pi], [0], [n], jac, surface_T=288.0, term_abs_coef=[kb[0]], term_layer=[nl])
        refused(*args, [1.0], [np.pi], [0], [n], jac, surface_T=288.0, term_abs_coef=[kb[0]], term_layer=[-1])
        refused(*args, [1.0], [np.pi], [0], [n], jac, term_abs_coef=[kb[0]], term_layer=[0])     # no surface
        refused(*args, [1.0], [np.pi], [0], [n], jac, ln_tau_spectra=spec_short, **ok)
        refused(*args, [1.0], [np.pi], [0], [n], jac, T_spectra=spec_short, **ok)
        tmax = _native.limit("jacobian_terms")
        big = ctx.buffer(2 + 2 * nl + tmax + 1)
        try:
            refused(*args, [1.0], [np.pi], [0], [n], big, surface_T=288.0, term_abs_coef=[kb[0]] * (tmax + 1),
                    term_layer=[0] * (tmax + 1))
        finally:
            big.free()
        # NULL and mismatched arguments through the raw entry point
        lib = ctx.lib
        import ctypes as C
        P = (C.c_void_p * nl)(*[b.h for b in kb])
        Td = (C.c_double * nl)(*T)
        Dd = (C.c_double * nl)(*d)
        mu1 = (C.c_double * 1)(1.0)
        w1 = (C.c_double * 1)(np.pi)
        bf = (C.c_int64 * 1)(0)
        bc = (C.c_int64 * 1)(n)
        tk = (C.c_void_p * 1)(kb[0].h)
        tl = (C.c_int32 * 1)(0)
        raw = lambda **o: lib.lbl_column_jacobian_dev(
            ctx.h, o.get("nl", nl), o.get("P", P), o.get("T", Td), o.get("D", Dd), 600.0, 700.0, n, None, 288.0, 1,
            o.get("mu", mu1), o.get("w", w1), 1, o.get("bf", bf), o.get("bc", bc), o.get("nt", 1), o.get("tk", tk),
            o.get("tl", tl), o.get("jac", jac.h), None, None)
        for o in (dict(P=None), dict(T=None), dict(D=None), dict(mu=None), dict(w=None), dict(bf=None), dict(bc=None),
                  dict(tk=None), dict(tl=None), dict(nt=-1), dict(nl=-1), dict(nl=129)):
            assert raw(**o) == BAD_ARG, o
            assert np.all(jac.download(nv) == 7.0)
        ctx.set_option("sweep_ieee_divisions", 1)
        try:
            refused(*args, [1.0], [np.pi], [0], [n], jac, **ok)
            with pytest.raises(ValueError, match="sweep_ieee_divisions"):
                atm.jacobians(surfaceTemperature=288)
        finally:
            ctx.set_option("sweep_ieee_divisions", 0)
    finally:
        for b in (jac, short, spec_short):
            b.free()
