"""GPU: Atmosphere.radiance (lbl_ray_radiance_dev, kernel K5e) against a NumPy restatement of its semantics (written out
below), against the existing fold and observe(), on synthetic absorption coefficients through the raw C ABI, in its
physical limits, and for independence of the rays, determinism, laziness and the C ABI's refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from oracle import pyrad_oracle as orc
from pyrad_amd import synthetic

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
RNG = (600, 610)
# Tolerances (the issue's; precedent: the 1e-13 tests/test_gpu_flux.py holds the same arithmetic to for spectra).  Radiance:
# rel_err <= 1e-13, floor 1e-300 for rays from space.  Transmittance: rel_err(floor=1e-30) <= 1e-13 - below 1e-30 the
# rounding of tau itself, tau * 2^-53, dominates and is not the kernel's.
TOL = 1e-13
# One ray of test_against_numpy cannot meet 1e-13 against NumPy, and NumPy's own `1 - t` is why: the limb ray at 1.7e5 cm
# stays in the thin top layer (80 hPa), one segment, where between the lines tau goes down to 7.5e-6 over the whole chord
# (the CPU oracle's coefficients).  From cold space its radiance is (1 - t) B and nothing else, t = exp(-tau) lies that
# close to 1, and two exps that are each good to an ulp but round t to neighbouring doubles (2^-53 apart just below 1)
# give 1 - t values 2^-53 / tau apart: up to 1.5e-11 on this ray, wherever the two happen to disagree.  Measured on an
# MI355X: worst radiance error of that ray 5.86e-12, what one ulp of t is at tau = 1.9e-5 (every other ray <= 3.3e-14, every
# transmittance, t itself, <= 7.4e-16).  The issue's rule for a bound that a measured worst value forces: at most 4x the
# measured worst, 2.3e-11; 2e-11 also covers one ulp of t at every point of the ray.  It holds for that ray's radiance
# alone; all else stays at TOL.
TOL_THIN_LIMB = 2e-11


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


@pytest.fixture()
def lines():
    from pyrad_amd import data
    data.set_source(data.synthetic_source(dict(co2=synthetic.make_lines(51, 800, 580, 720),
                                               h2o=synthetic.make_lines(52, 500, 580, 720))))


def column(pyrad, rng=RNG, layers=LAYERS, co2=400, h2o=0.5):
    atm = pyrad.Atmosphere("col")
    for depth, T, P in layers:
        L = atm.addLayer(depth, T, P, *rng)
        L.addMolecule('co2', ppm=co2)
        L.addMolecule('h2o', percentage=h2o)
    return atm


def nine_paths(pyrad, atm):
    return [atm.nadirPath(), atm.nadirPath(mu=0.4), atm.nadirPath(observerLevel=2),
            atm.zenithPath(), atm.zenithPath(mu=0.3), atm.zenithPath(observerLevel=2),
            atm.limbPath(5e3), atm.limbPath(2.5e4), atm.limbPath(1.7e5), pyrad.Path([], [], source="surface")]


# ---- the semantics, restated in NumPy ----------------------------------------------------------------------------------
def walk(x, k, T, layers, lengths, source):
    """(radiance, transmittance) of one ray: k[l] the absorption coefficient of layer l on the grid x, T[l] its
    temperature, source the radiance entering the first segment (None: cold space)"""
    I = np.zeros(x.size) if source is None else np.array(source, dtype=np.float64)
    Tt = np.ones(x.size)
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        for l, s in zip(layers, lengths):
            tau = k[l] * s
            t = np.exp(-tau)
            B = orc.planckWavenumber(x, T[l])
            I = t * I + (1 - t) * B
            Tt = Tt * t
    return I, Tt


def reference(pyrad, atm, paths, surface):
    x = atm[0].xAxis
    k = [np.array(pyrad.getAbsCoef(L)) for L in atm]
    T = [L.T for L in atm]
    out = [walk(x, k, T, p.layers, p.lengths, surface if p.source == "surface" else None) for p in paths]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def check(paths_or_kinds, got_I, got_T, want_I, want_T, tol_I=None):
    """tol_I: {ray: bound of its radiance} where it is not TOL"""
    worst = []
    for r, p in enumerate(paths_or_kinds):
        space = (p.source == "space") if hasattr(p, "source") else (p == 0)
        eI = rel_err(got_I[r], want_I[r], floor=1e-300 if space else 0.0)
        eT = rel_err(got_T[r], want_T[r], floor=1e-30)
        print("ray %d: radiance %.2e transmittance %.2e" % (r, eI, eT))
        worst.append((r, eI, eT, (tol_I or {}).get(r, TOL)))
    for r, eI, eT, bound in worst:
        assert eI <= bound and eT <= TOL, (r, eI, eT)


# ---- 1. identity with the fold and with observe() ------------------------------------------------------------------------
def test_nadir_path_is_the_fold_and_observe(pyrad, lines):
    atm = column(pyrad)
    toa = np.array(atm.transmission(surfaceTemperature=288))
    got = atm.radiance(atm.nadirPath(), surfaceTemperature=288)
    assert got.radiance.shape == (1, toa.size) and got.transmittance is None
    assert np.array_equal(got.wavenumber, atm[0].xAxis)
    assert np.array_equal(got.radiance[0], toa)
    surf = atm[0].planck(300)
    toa = np.array(atm.transmission(surfaceSpectrum=surf))
    assert np.array_equal(atm.radiance(atm.nadirPath(), surfaceSpectrum=surf).radiance[0], toa)
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    ob = atm.observe(ins, surfaceTemperature=288, mu=1)
    got = atm.radiance(atm.nadirPath(), surfaceTemperature=288, instrument=ins)
    assert got.radiance.shape == (1, len(ins)) and np.array_equal(got.wavenumber, ins.centres)
    assert np.array_equal(got.radiance[0], ob.radiance)
    ob = atm.observe(ins, surfaceSpectrum=surf, mu=1)
    assert np.array_equal(atm.radiance(atm.nadirPath(), surfaceSpectrum=surf, instrument=ins).radiance[0], ob.radiance)


# ---- 2. against NumPy ----------------------------------------------------------------------------------------------------
def test_against_numpy(pyrad, lines):
    atm = column(pyrad)
    paths = nine_paths(pyrad, atm)
    x = atm[0].xAxis
    for kw, surface in ((dict(surfaceTemperature=288), orc.planckWavenumber(x, 288)),
                        (dict(surfaceSpectrum=atm[0].planck(300)), np.array(atm[0].planck(300)))):
        got = atm.radiance(paths, transmittance=True, **kw)
        assert got.radiance.shape == got.transmittance.shape == (len(paths), x.size)
        assert got.paths == paths
        want_I, want_T = reference(pyrad, atm, paths, surface)
        check(paths, got.radiance, got.transmittance, want_I, want_T, tol_I={8: TOL_THIN_LIMB})
    # the channel values are the convolution of the same rows (K8's own accuracy is tests/test_gpu_instrument.py's)
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    ch = atm.radiance(paths, surfaceTemperature=288, instrument=ins, transmittance=True)
    full = atm.radiance(paths, surfaceTemperature=288, transmittance=True)
    rows = pyrad.convolve(ins, np.concatenate([full.radiance, full.transmittance]), *RNG)
    assert ch.radiance.shape == ch.transmittance.shape == (len(paths), len(ins))
    assert np.array_equal(np.concatenate([ch.radiance, ch.transmittance]), rows)


# ---- 3. the raw C ABI on uploaded synthetic absorption coefficients ---------------------------------------------------------
def synthetic_k(rs, L, n, tau_lo=-5.5, tau_hi=-3.0, huge=0.03):
    """L x n: 10^U(tau_lo, tau_hi) (optical depths of 0.01 .. 20 over 1e4 cm: thinner segments would test NumPy's 1 - t, not
    the kernel), 5% exact zeros, a share ``huge`` so large that t underflows"""
    k = 10.0 ** rs.uniform(tau_lo, tau_hi, size=(L, n))
    u = rs.uniform(size=(L, n))
    k[u < 0.05] = 0.0
    k[u > 1 - huge] = 10.0 ** rs.uniform(-1, 3, size=int(np.sum(u > 1 - huge)))
    return k


def run_raw(ctx, k, T, rays, lo=600.0, hi=700.0, I_source=None, source_T=0.0):
    """rays: [(layers, lengths, kind)] -> (radiance, transmittance), R x n each"""
    L, n = k.shape
    bufs = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    rad, trn = ctx.buffer(len(rays) * n), ctx.buffer(len(rays) * n)
    src = ctx.buffer(n).upload(I_source) if I_source is not None else None
    try:
        ctx.ray_radiance_dev(bufs, T, lo, hi, n, np.cumsum([0] + [len(r[0]) for r in rays]),
                             [l for r in rays for l in r[0]], [s for r in rays for s in r[1]], [r[2] for r in rays], rad,
                             I_source=src, source_T=source_T, transmittance=trn)
        return rad.download().reshape(len(rays), n), trn.download().reshape(len(rays), n)
    finally:
        for b in bufs + [rad, trn] + ([src] if src is not None else []):
            b.free()


def check_raw(ctx, k, T, rays, lo=600.0, hi=700.0, I_source=None, source_T=0.0):
    n = k.shape[1]
    x = np.linspace(lo, hi, n)
    got_I, got_T = run_raw(ctx, k, T, rays, lo, hi, I_source, source_T)
    surface = I_source if I_source is not None else orc.planckWavenumber(x, source_T) if source_T > 0 else None
    want = [walk(x, k, T, r[0], r[1], surface if r[2] == 1 else None) for r in rays]
    check([r[2] for r in rays], got_I, got_T, [w[0] for w in want], [w[1] for w in want])
    return got_I, got_T


@pytest.fixture()
def ctx(pyrad):
    from pyrad_amd import engine
    return engine.get_engine().ctx


def band_of_rays(rs, L):
    """five rays over one layer sequence (a bundle of four and one left over), a reversed one, one that repeats a layer five
    times, a zero-segment ray from each source"""
    up = list(range(L))
    rays = [(up, list(rs.uniform(0.5e4, 2e4, L)), i % 2) for i in range(5)]
    rays.append((up[::-1], list(rs.uniform(0.5e4, 2e4, L)), 0))
    rays.append(([1, 1, 0, 1, 1, 1], list(rs.uniform(0.5e4, 2e4, 6)), 1))
    rays += [([], [], 1), ([], [], 0)]
    return rays


# (the launch has no grid-stride bound - one workgroup per 1,024 points and bundle - so there is no size beyond one to test;
# 5,003 points are five workgroups and a tail)
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 5003])
def test_raw_abi_sizes(ctx, n):
    rs = np.random.RandomState(100 + n)
    L = 3
    k = synthetic_k(rs, L, n)
    T = [288.0, 250.0, 215.0]
    check_raw(ctx, k, T, band_of_rays(rs, L), source_T=295.0)
    check_raw(ctx, k, T, band_of_rays(rs, L), I_source=rs.uniform(0.0, 0.2, n))


def test_raw_abi_128_layers_limb_shaped(ctx):
    rs = np.random.RandomState(7)
    L, n = 128, 1027
    # 255 segments of optical depth 0.005 .. 0.1 each; an opaque layer at 1 point in 4
    k = synthetic_k(rs, L, n, tau_lo=-6.0, tau_hi=-5.0, huge=0.002)
    T = list(np.linspace(290.0, 180.0, L))
    half = list(rs.uniform(0.5e4, 1e4, L))
    seq = list(range(L - 1, 0, -1)) + [0] + list(range(1, L))
    lens = [half[l] for l in seq[:L - 1]] + [2 * half[0]] + [half[l] for l in seq[L:]]
    assert len(seq) == 255
    check_raw(ctx, k, T, [(seq, lens, 0), (seq, lens, 1)], source_T=300.0)


def test_raw_abi_zero_length_segments(ctx):
    rs = np.random.RandomState(11)
    L, n = 3, 1027
    k = synthetic_k(rs, L, n)
    T = [288.0, 250.0, 215.0]
    src = rs.uniform(0.0, 0.2, n)
    rays = [([0, 1, 2, 1], [0.0] * 4, 1), ([2, 0], [0.0] * 2, 0)]
    got_I, got_T = check_raw(ctx, k, T, rays, I_source=src)
    assert np.all(got_T == 1.0)
    assert np.array_equal(got_I[0], src) and np.all(got_I[1] == 0.0)      # (B is finite on 600-700 cm^-1)


# ---- 4. independence and determinism -------------------------------------------------------------------------------------
def test_rays_are_independent_and_calls_deterministic(pyrad, lines):
    atm = column(pyrad)
    paths = nine_paths(pyrad, atm)[:9]
    a = atm.radiance(paths, surfaceTemperature=288, transmittance=True)
    I, Tt = a.radiance.copy(), a.transmittance.copy()
    b = atm.radiance(paths, surfaceTemperature=288, transmittance=True)
    assert np.array_equal(b.radiance, I) and np.array_equal(b.transmittance, Tt)
    rev = atm.radiance(paths[::-1], surfaceTemperature=288, transmittance=True)
    assert np.array_equal(rev.radiance[::-1], I) and np.array_equal(rev.transmittance[::-1], Tt)
    for r, p in enumerate(paths):
        alone = atm.radiance(p, surfaceTemperature=288, transmittance=True)
        assert np.array_equal(alone.radiance[0], I[r]) and np.array_equal(alone.transmittance[0], Tt[r]), r
    # four and five rays over one layer sequence travel as a bundle: the same bits as each one alone
    mus = [1.0, 0.8, 0.6, 0.4, 0.25]
    band = atm.radiance([atm.nadirPath(mu=m) for m in mus], surfaceTemperature=288, transmittance=True)
    for r, m in enumerate(mus):
        alone = atm.radiance(atm.nadirPath(mu=m), surfaceTemperature=288, transmittance=True)
        assert np.array_equal(alone.radiance[0], band.radiance[r]), m
        assert np.array_equal(alone.transmittance[0], band.transmittance[r]), m


# ---- 5. physics limits -----------------------------------------------------------------------------------------------------
def test_isothermal_column(pyrad, lines):
    atm = column(pyrad, layers=tuple((d, 260, P) for d, _, P in LAYERS))
    paths = [atm.nadirPath(), atm.nadirPath(mu=0.4), atm.nadirPath(observerLevel=2), pyrad.Path([2, 1, 2], [3e4, 1e5, 7e3])]
    got = atm.radiance(paths, surfaceTemperature=260)
    want = orc.planckWavenumber(atm[0].xAxis, 260)
    for r in range(len(paths)):
        assert rel_err(got.radiance[r], want) <= TOL, r


def test_transparent_column(pyrad, lines):
    atm = column(pyrad, co2=0, h2o=0)
    got = atm.radiance([atm.limbPath(5e3), atm.limbPath(1.7e5), atm.zenithPath(), atm.zenithPath(mu=0.3)], transmittance=True)
    assert np.all(got.radiance == 0.0) and np.all(got.transmittance == 1.0)


def test_opaque_tangent_layer(pyrad, lines):
    atm = column(pyrad)
    k1 = np.array(pyrad.getAbsCoef(atm[1]))
    assert np.min(k1) > 0
    p = atm.limbPath(2.5e4)                              # tangent layer 1
    assert p.layers == (3, 2, 1, 2, 3)
    scale = 80.0 / (np.min(k1) * p.lengths[2])          # optical depth >= 80 along the tangent segment: t < 1e-34
    opaque = pyrad.Path(p.layers, p.lengths[:2] + (p.lengths[2] * scale,) + p.lengths[3:], source="space")
    got = atm.radiance(opaque, transmittance=True)
    x = atm[0].xAxis
    k = [np.array(pyrad.getAbsCoef(L)) for L in atm]
    T = [L.T for L in atm]
    # what the far side sends is lost: the tangent layer's Planck function, then the near side's layers 2 and 3
    near, _ = walk(x, k, T, p.layers[3:], p.lengths[3:], orc.planckWavenumber(x, T[1]))
    assert rel_err(got.radiance[0], near) <= TOL
    assert np.all(got.transmittance[0] <= 1e-34)


# ---- 6. refusals of the C entry point ----------------------------------------------------------------------------------------
def test_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    rs = np.random.RandomState(3)
    L, n, R = 3, 1027, 2
    k = synthetic_k(rs, L, n)
    T = [288.0, 250.0, 215.0]
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    rad, trn, src = ctx.buffer(R * n), ctx.buffer(R * n), ctx.buffer(n).upload(np.full(n, 0.1))
    short, src_short = ctx.buffer(R * n - 1), ctx.buffer(n - 1)
    k_short = ctx.buffer(n - 1)
    i32, f64 = lambda v: (C.c_int32 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    many = _native.limit("ray_paths") + 1
    too_long = _native.limit("ray_segments") + 1
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), T=f64(T), lo=600.0, hi=700.0, n=n,
                n_rays=R, ray_first=i32([0, 3, 5]), seg_layer=i32([0, 1, 2, 2, 1]), seg_length=f64([1e4, 2e4, 1e4, 3e4, 1e4]),
                source_kind=i32([1, 0]), I_source=src.h, source_T=0.0, radiance=rad.h, transmittance=trn.h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_ray_radiance_dev(a["ctx"], a["n_layers"], a["abs_coef"], a["T"], a["lo"], a["hi"], a["n"], a["n_rays"],
                                        a["ray_first"], a["seg_layer"], a["seg_length"], a["source_kind"], a["I_source"],
                                        a["source_T"], a["radiance"], a["transmittance"])

    bad = [dict(abs_coef=None), dict(T=None), dict(ray_first=None), dict(seg_layer=None), dict(seg_length=None),
           dict(source_kind=None), dict(radiance=None),
           dict(n_layers=0), dict(n_layers=_native.limit("layers_per_column") + 1), dict(n=0), dict(n=-5),
           dict(n_rays=0), dict(n_rays=many, ray_first=i32([0] * (many + 1)), source_kind=i32([0] * many)),
           dict(ray_first=i32([1, 3, 5])), dict(ray_first=i32([0, 3, 2])),
           dict(n_rays=1, ray_first=i32([0, too_long]), seg_layer=i32([0] * too_long), seg_length=f64([1.0] * too_long)),
           dict(seg_layer=i32([0, 1, 3, 2, 1])), dict(seg_layer=i32([0, -1, 2, 2, 1])),
           dict(seg_length=f64([1e4, -1.0, 1e4, 3e4, 1e4])), dict(seg_length=f64([1e4, float("nan"), 1e4, 3e4, 1e4])),
           dict(seg_length=f64([1e4, float("inf"), 1e4, 3e4, 1e4])),
           dict(T=f64([288.0, 0.0, 215.0])), dict(T=f64([288.0, float("nan"), 215.0])),
           dict(source_kind=i32([2, 0])), dict(source_kind=i32([1, -1])),
           dict(I_source=None, source_T=0.0),
           dict(radiance=short.h), dict(transmittance=short.h), dict(I_source=src_short.h),
           dict(abs_coef=(C.c_void_p * L)(kb[0].h, k_short.h, kb[2].h))]
    try:
        assert call() == 0
        want_I, want_T = rad.download(), trn.download()
        rad.upload(np.full(R * n, -7.0))
        trn.upload(np.full(R * n, -7.0))
        assert lib.lbl_ray_radiance_dev(None, *[good[key] for key in list(good)[1:]]) == BAD_ARG      # a NULL ctx
        for kw in bad:
            assert call(**kw) == BAD_ARG, sorted(kw)
            assert lib.lbl_last_error(ctx.h), sorted(kw)
        ctx.set_option("sweep_ieee_divisions", 1)
        try:
            assert call() == BAD_ARG
            assert b"sweep_ieee_divisions" in lib.lbl_last_error(ctx.h)
        finally:
            ctx.set_option("sweep_ieee_divisions", 0)
        # nothing was enqueued by a refused call: the outputs still hold the marker, and the context goes on computing
        assert np.all(rad.download() == -7.0) and np.all(trn.download() == -7.0)
        assert call(source_kind=i32([0, 0]), I_source=None) == 0            # rays from space need no surface source
        assert call() == 0
        assert np.array_equal(rad.download(), want_I) and np.array_equal(trn.download(), want_T)
        x = np.linspace(600.0, 700.0, n)
        want = walk(x, k, T, [0, 1, 2], [1e4, 2e4, 1e4], np.full(n, 0.1))
        assert rel_err(want_I[:n], want[0]) <= TOL and rel_err(want_T[:n], want[1], floor=1e-30) <= TOL
    finally:
        for b in kb + [rad, trn, src, short, src_short, k_short]:
            b.free()


# ---- 7. laziness -------------------------------------------------------------------------------------------------------------
def test_no_accumulate_after_transmission(pyrad, lines, ctx):
    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    ctx.profile_enable(["xsec_accumulate"])
    try:
        ctx.profile_reset()
        atm.radiance([atm.nadirPath(), atm.limbPath(2.5e4)], surfaceTemperature=288)
        assert ctx.profile_read()["xsec_accumulate"][0] == 0
        atm[2].changeTemperature(250)                      # one layer due: the counter does count
        atm.radiance([atm.nadirPath(), atm.limbPath(2.5e4)], surfaceTemperature=288)
        assert ctx.profile_read()["xsec_accumulate"][0] >= 1
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
