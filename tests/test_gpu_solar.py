"""GPU: Atmosphere.solarFluxes (lbl_column_solar_dev, kernels K5k) against a NumPy float64 restatement of its semantics
(written out below), in its analytic limits, against the ray machinery, on hand-made coefficients through the raw C ABI,
and for superposition, independence of the beams, determinism, laziness and the C ABI's refusals.

Tolerances: band values 1e-12 and spectra 1e-13 relative, what tests/test_gpu_flux.py holds the same exp and the same kind
of recurrence to; floor 1e-300 where a value underflows.  Heating rates are differences of nearly equal net fluxes: their
allowance is absolute, 1e-12 of the heating rate the band's largest level flux would cause if one layer absorbed it whole."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from pyrad_amd import synthetic
from test_gpu_flux import LAYERS, column, pyrad, source  # noqa: F401

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
TOL_BAND, TOL_SPEC, FLOOR = 1e-12, 1e-13, 1e-300
WINDOWS = {"thermal": (600, 700), "near-ir": (3500, 3600)}
BEAMS = {"one": 0.6, "three": [(0.9, 0.2), (0.5, 0.5), (0.15, 0.3)],
         "eight": [(1.0 - 0.11 * i, 0.05 + 0.02 * i) for i in range(8)]}
REFLECTIONS = ("lambertian", "specular")


@pytest.fixture(params=sorted(WINDOWS))
def window(request):
    lo, hi = WINDOWS[request.param]
    source(co2=synthetic.make_lines(51, 800, lo - 20, hi + 20), h2o=synthetic.make_lines(52, 500, lo - 20, hi + 20))
    return lo, hi


@pytest.fixture()
def lines():
    source(co2=synthetic.make_lines(51, 800, 580, 720), h2o=synthetic.make_lines(52, 500, 580, 720))


@pytest.fixture()
def ctx(pyrad):
    from pyrad_amd import engine
    return engine.get_engine().ctx


def spectral_emissivity(x):
    return 0.55 + 0.4 * np.sin(0.37 * (x - x[0])) ** 2


def solar_source(x):
    """a smooth, positive irradiance of order 1 with structure on the grid"""
    return 0.8 + 0.5 * np.cos(0.21 * (x - x[0])) ** 2


# ---- the semantics, restated in NumPy ----------------------------------------------------------------------------------
def restate(k, depth, S0, beam_w, slant, mu, w, e, reflection, idx=None, dtype=np.float64):
    """include/pyrad_hip.h, "direct solar beam": (up, down) raw band sums [band, level] and the spectral F_up at the top,
    F_down at the surface and F_up at the surface.  k: L x n; slant: beams x L; e: a number or n values."""
    k = np.asarray(k, dtype=dtype)
    L, n = k.shape
    f = lambda v: np.asarray(v, dtype=dtype)
    depth, S0, beam_w, slant, mu, w, e = f(depth), f(S0), f(beam_w), f(slant).reshape(len(beam_w), L), f(mu), f(w), f(e)
    idx = [(0, n)] if idx is None else idx
    up = np.zeros((len(idx), L + 1), dtype=dtype)
    down = np.zeros((len(idx), L + 1), dtype=dtype)

    def level(weights, values):
        F = weights[0] * values[0]
        for wt, v in zip(weights[1:], values[1:]):
            F = F + wt * v
        return F, [np.sum(np.nan_to_num(F[a:b].astype(np.float64)).astype(dtype)) for a, b in idx]

    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        tau = k * depth[:, None]
        S = [S0.copy() for _ in beam_w]
        sd, down[:, L] = level(beam_w, S)
        for l in range(L - 1, -1, -1):
            S = [np.exp(-tau[l] * slant[s, l]) * S[s] for s in range(len(beam_w))]
            sd, down[:, l] = level(beam_w, S)
        if reflection == "lambertian":
            wsum = dtype(0.0)
            for wt in w:
                wsum = wsum + wt
            I = [((1 - e) * sd) / wsum for _ in mu]
            weights, rates = w, [np.full(L, 1 / m, dtype=dtype) for m in mu]
        else:
            I = [(1 - e) * Ss for Ss in S]
            weights, rates = beam_w, slant
        s0, up[:, 0] = level(weights, I)
        su = s0
        for l in range(L):
            I = [np.exp(-tau[l] * rates[i][l]) * I[i] for i in range(len(I))]
            su, up[:, l + 1] = level(weights, I)
    return up, down, su, sd, s0


def inside(n, idx):
    m = np.zeros(n, dtype=bool)
    for a, b in idx:
        m[a:b] = True
    return m


def heating_allowance(pyrad, atm, up, down):
    """1e-12 of the heating rate the band's largest level flux would cause if absorbed whole in the layer, K/day"""
    P, T, depth = (np.array(v, dtype=np.float64) for v in zip(*[(L.P, L.T, L.depth) for L in atm]))
    mass = (100.0 * P / (pyrad.R_DRY_AIR * T)) * (depth / 100.0)
    largest = np.max(np.maximum(np.abs(up), np.abs(down)), axis=-1)
    return 1e-12 * np.asarray(largest)[..., None] / (pyrad.CP_AIR * mass) * 86400.0


def check_model(pyrad, atm, got, S0, e, reflection, angles, bands_idx=None, banded=False):
    from pyrad_amd import settings
    x = atm[0].xAxis
    k = np.array([np.array(pyrad.getAbsCoef(L)) for L in atm])
    depth = [L.depth for L in atm]
    mu, w = pyrad.fluxAngles(angles)
    ev = e if np.ndim(e) == 0 else np.asarray(e)
    up, down, su, sd, s0 = restate(k, depth, S0, got.beamWeight, got.slant, mu, w, ev, reflection, bands_idx)
    res = settings.BASE_RESOLUTION
    up, down = up * res, down * res
    if not banded:
        up, down = up[0], down[0]
    if bands_idx is not None:
        m = inside(x.size, bands_idx)
        su, sd, s0 = (np.where(m, v, 0.0) for v in (su, sd, s0))
    errs = dict(up=rel_err(got.up, up, floor=FLOOR), down=rel_err(got.down, down, floor=FLOOR),
                upSpectrum=rel_err(got.upSpectrum, su, floor=FLOOR), downSpectrum=rel_err(got.downSpectrum, sd, floor=FLOOR),
                upSurfaceSpectrum=rel_err(got.upSurfaceSpectrum, s0, floor=FLOOR))
    heat = pyrad.heatingRates(up - down, [L.P for L in atm], [L.T for L in atm], depth)
    heat_err = np.max(np.abs(got.heatingRate - heat) / heating_allowance(pyrad, atm, up, down))
    print(reflection, angles, "e=%s" % (e if np.ndim(e) == 0 else "spectrum"),
          " ".join("%s %.2e" % kv for kv in errs.items()), "heating (allowances of 1e-12) %.2e" % heat_err)
    assert np.array_equal(got.net, got.up - got.down)
    assert np.array_equal(got.absorbedSurface, got.down[..., 0] - got.up[..., 0])
    assert errs["up"] <= TOL_BAND and errs["down"] <= TOL_BAND, errs
    assert max(errs["upSpectrum"], errs["downSpectrum"], errs["upSurfaceSpectrum"]) <= TOL_SPEC, errs
    assert heat_err <= 1.0, heat_err


# ---- 1. against NumPy --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflection", REFLECTIONS)
@pytest.mark.parametrize("geometry", ["plane", "spherical"])
@pytest.mark.parametrize("beams", sorted(BEAMS))
def test_against_numpy(pyrad, window, beams, geometry, reflection):
    atm = column(pyrad, rng=window)
    x = atm[0].xAxis
    S0 = solar_source(x)
    L = len(atm)
    for e in (1.0, 0.0, 0.3, spectral_emissivity(x)):
        for angles in ((1, 3, 8, "diffusivity") if reflection == "lambertian" else (3,)):
            got = atm.solarFluxes(solarSpectrum=S0, mu0=BEAMS[beams], geometry=geometry, emissivity=e, reflection=reflection,
                                  angles=angles, spectra=True)
            mu_s, w_s = pyrad._solar_beams(BEAMS[beams])
            assert np.array_equal(got.mu0, mu_s) and np.array_equal(got.beamWeight, w_s * mu_s)
            assert got.slant.shape == (len(mu_s), L)
            assert np.array_equal(got.slant, pyrad.solarSlants([Ly.depth for Ly in atm], list(zip(mu_s, w_s)), geometry))
            assert got.up.shape == got.down.shape == got.net.shape == (L + 1,) and got.heatingRate.shape == (L,)
            assert np.all(np.diff(got.down) >= 0) and np.all(np.diff(got.up) <= 0)        # nothing emits: only attenuation
            check_model(pyrad, atm, got, S0, e, reflection, angles)


def test_black_body_sun(pyrad, window):
    """solarTemperature is solarIrradiance on the grid; without a surface albedo the column only absorbs"""
    atm = column(pyrad, rng=window)
    x = atm[0].xAxis
    got = atm.solarFluxes(solarTemperature=5772.0, distanceAU=1.2, mu0=0.5, spectra=True)
    check_model(pyrad, atm, got, pyrad.solarIrradiance(x, 5772.0, 1.2), 1.0, "lambertian", 3)
    assert np.all(got.up == 0.0) and np.all(got.heatingRate >= 0.0)
    assert 0.0 < got.down[0] < got.down[-1]                           # the beam is neither untouched nor extinguished
    print("down at the surface / at the top: %.4f" % (got.down[0] / got.down[-1]))
    # a source made from numbers stays on the device: the same numbers find it, other numbers replace it
    kw = dict(distanceAU=1.2, mu0=0.5, spectra=True)
    again = atm.solarFluxes(solarTemperature=5772.0, **kw)
    cooler = atm.solarFluxes(solarTemperature=5000.0, **kw)
    flat = atm.solarFluxes(solarSpectrum=2.0, mu0=0.5, spectra=True)
    back = atm.solarFluxes(solarTemperature=5772.0, **kw)
    for f in (again, back):
        assert np.array_equal(f.downSpectrum, got.downSpectrum) and np.array_equal(f.down, got.down)
    check_model(pyrad, atm, cooler, pyrad.solarIrradiance(x, 5000.0, 1.2), 1.0, "lambertian", 3)
    check_model(pyrad, atm, flat, np.full(x.size, 2.0), 1.0, "lambertian", 3)
    other = column(pyrad, rng=(window[0], window[1] + 10))          # another grid: nothing is found
    check_model(pyrad, other, other.solarFluxes(solarTemperature=5772.0, **kw), pyrad.solarIrradiance(other[0].xAxis, 5772.0, 1.2),
                1.0, "lambertian", 3)


# ---- 2. the transparent column -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_transparent_column(pyrad, lines, reflection):
    from pyrad_amd import settings
    atm = column(pyrad, co2=0, h2o=0)
    x = atm[0].xAxis
    S0 = solar_source(x)
    mu_s, w_s = pyrad._solar_beams(BEAMS["three"])
    beam_sum = (w_s[0] * mu_s[0]) * S0
    for m, wt in list(zip(mu_s, w_s))[1:]:
        beam_sum = beam_sum + (wt * m) * S0
    want = np.full(len(atm) + 1, settings.BASE_RESOLUTION * np.sum(beam_sum))
    mirror = atm.solarFluxes(solarSpectrum=S0, mu0=BEAMS["three"], geometry="spherical", emissivity=0.0, reflection=reflection)
    assert rel_err(mirror.down, want) <= 1e-13
    assert rel_err(mirror.up, mirror.down) <= 1e-13
    assert np.all(np.abs(mirror.heatingRate) <= heating_allowance(pyrad, atm, mirror.up, mirror.down) * 10)
    black = atm.solarFluxes(solarSpectrum=S0, mu0=BEAMS["three"], emissivity=1.0, reflection=reflection, spectra=True)
    assert rel_err(black.down, want) <= 1e-13
    assert np.all(black.up == 0.0) and np.all(black.upSpectrum == 0.0) and np.all(black.upSurfaceSpectrum == 0.0)
    assert rel_err(black.absorbedSurface, want[0]) <= 1e-13


# ---- 3. superposition and independence of the beams ---------------------------------------------------------------------
@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_beams_superpose_and_do_not_see_each_other(pyrad, lines, reflection):
    atm = column(pyrad)
    x = atm[0].xAxis
    kw = dict(solarSpectrum=solar_source(x), geometry="spherical", emissivity=0.4, reflection=reflection, spectra=True)
    a, b = (0.7, 0.25), (0.3, 1.5)
    both = atm.solarFluxes(mu0=[a, b], **kw)
    fa, fb = atm.solarFluxes(mu0=[a], **kw), atm.solarFluxes(mu0=[b], **kw)
    for name in ("up", "down", "net", "upSpectrum", "downSpectrum", "upSurfaceSpectrum"):
        assert rel_err(getattr(both, name), getattr(fa, name) + getattr(fb, name), floor=FLOOR) <= 1e-13, name
    # a beam's operations do not depend on the beams it travels with (DESIGN.md "K5k"): alone, or first among three whose
    # others have no weight (fma(0, S, f) == f), the same bits
    alone = atm.solarFluxes(mu0=[a], **kw)
    first = atm.solarFluxes(mu0=[a, (0.3, 0.0), (0.9, 0.0)], **kw)
    assert np.array_equal(alone.downSpectrum, first.downSpectrum)
    assert np.array_equal(alone.down, first.down)
    assert np.array_equal(alone.upSpectrum, first.upSpectrum) and np.array_equal(alone.up, first.up)
    # ... and the position among them changes only the order of the sum
    last = atm.solarFluxes(mu0=[b, a], **kw)
    assert rel_err(last.downSpectrum, both.downSpectrum, floor=FLOOR) <= 1e-13


# ---- 4. against the ray machinery ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu0", [1.0, 0.35])
def test_one_beam_is_the_zenith_path_transmittance(pyrad, window, mu0):
    atm = column(pyrad, rng=window)
    x = atm[0].xAxis
    S0 = solar_source(x)
    T = atm.radiance([atm.zenithPath(mu=mu0)], transmittance=True).transmittance[0]
    got = atm.solarFluxes(solarSpectrum=S0, mu0=mu0, spectra=True)
    err = rel_err(got.downSpectrum, mu0 * S0 * T, floor=1e-30)       # (test_gpu_paths: below 1e-30 tau's own rounding)
    print("down spectrum against mu0 S0 T: %.2e" % err)
    assert err <= 1e-12


# ---- 5. bands ----------------------------------------------------------------------------------------------------------
def band_pairs(x, edges):
    return [(x[a], x[b] if b < x.size else np.inf) for a, b in edges]


@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_bands(pyrad, lines, reflection):
    atm = column(pyrad, rng=(600, 700.07))            # an odd number of grid points
    x = atm[0].xAxis
    n = x.size
    S0 = solar_source(x)
    e = spectral_emissivity(x)
    kw = dict(solarSpectrum=S0, mu0=BEAMS["three"], emissivity=e, reflection=reflection, spectra=True)
    # a head, an aligned body and a tail; one point; a gap before the last band
    idx = [(3, 3 + 1027), (1030, 1031), (2001, 4002), (5003, n)]
    got = atm.solarFluxes(bands=band_pairs(x, idx), **kw)
    assert got.up.shape == (len(idx), len(atm) + 1) and got.heatingRate.shape == (len(idx), len(atm))
    assert got.absorbedSurface.shape == (len(idx),)
    check_model(pyrad, atm, got, S0, e, reflection, 3, bands_idx=idx, banded=True)
    out = ~inside(n, idx)
    for spec in (got.upSpectrum, got.downSpectrum, got.upSurfaceSpectrum):
        assert np.all(spec[out] == 0.0) and np.any(spec[~out] > 0.0)
    # 64 bands of uneven lengths that tile the grid: their sum is the whole range
    cuts = np.unique(np.concatenate([[0, n], 1 + np.random.RandomState(3).choice(n - 2, 63, replace=False)]))
    idx = list(zip(cuts[:-1], cuts[1:]))
    assert len(idx) == 64
    many = atm.solarFluxes(bands=band_pairs(x, idx), **kw)
    check_model(pyrad, atm, many, S0, e, reflection, 3, bands_idx=idx, banded=True)
    whole = atm.solarFluxes(**kw)
    assert rel_err(many.up.sum(axis=0), whole.up) <= 1e-13 and rel_err(many.down.sum(axis=0), whole.down) <= 1e-13
    assert np.array_equal(many.downSpectrum, whole.downSpectrum) and np.array_equal(many.upSpectrum, whole.upSpectrum)


# ---- 6. the raw C ABI on hand-made absorption coefficients ----------------------------------------------------------------
def run_raw(ctx, k, depth, S0, beam_w, slant, mu, w, e, reflection, bands=None, spectra=True):
    """lbl_column_solar_dev on uploaded coefficients: (level sums [band, 2, level], up_top, down_surface, up_surface)"""
    L, n = k.shape
    first, count = ([0], [n]) if bands is None else ([a for a, _ in bands], [b - a for a, b in bands])
    nb = len(first)
    bufs = [ctx.buffer(max(n, 1)).upload(k[l]) for l in range(L)]
    level, src = ctx.buffer(nb * 2 * (L + 1)), ctx.buffer(n).upload(np.asarray(S0, dtype=np.float64))
    spec = [ctx.buffer(n) for _ in range(3)] if spectra else [None] * 3
    bufs += [level, src] + [b for b in spec if b is not None]
    try:
        eb = None
        if np.ndim(e):
            eb = ctx.buffer(n).upload(e); bufs.append(eb)
        ctx.column_solar_dev(bufs[:L], depth, 600.0, 700.0, n, src, beam_w, slant, mu, w, first, count, level,
                             emissivity=eb if eb is not None else e, reflection=REFLECTIONS.index(reflection),
                             up_top=spec[0], down_surface=spec[1], up_surface=spec[2])
        return (level.download(nb * 2 * (L + 1)).reshape(nb, 2, L + 1),) + tuple(b.download(n) if b is not None else None for b in spec)
    finally:
        for b in bufs:
            b.free()


def check_raw(ctx, k, depth, S0, beam_w, slant, mu, w, e, reflection, bands=None, spectra=True):
    n = k.shape[1]
    sums, ut, ds, us = run_raw(ctx, k, depth, S0, beam_w, slant, mu, w, e, reflection, bands, spectra)
    fu, fd, su, sd, s0 = restate(k, depth, S0, beam_w, slant, mu, w, e, reflection, bands)
    errs = [rel_err(sums[:, 0], fu, floor=FLOOR), rel_err(sums[:, 1], fd, floor=FLOOR)]
    if spectra:
        if bands is not None:                        # (points outside every band keep 0 in the spectra)
            m = inside(n, bands)
            su, sd, s0 = (np.where(m, v, 0.0) for v in (su, sd, s0))
        errs += [rel_err(ut, su, floor=FLOOR), rel_err(ds, sd, floor=FLOOR), rel_err(us, s0, floor=FLOOR)]
    print(reflection, k.shape, len(beam_w), len(mu), " ".join("%.2e" % v for v in errs))
    assert errs[0] <= TOL_BAND and errs[1] <= TOL_BAND, errs
    assert all(v <= TOL_SPEC for v in errs[2:]), errs
    return sums, ut, ds, us


def hand_made_k(rs, L, n, tau_lo=-5.5, tau_hi=-3.5):
    """L x n: 10^U(tau_lo, tau_hi) (optical depths of 0.03 .. 3 over 1e4 cm) with 5% exact zeros"""
    k = 10.0 ** rs.uniform(tau_lo, tau_hi, size=(L, n))
    k[rs.uniform(size=(L, n)) < 0.05] = 0.0
    return k


@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_raw_one_point_and_no_layer(ctx, pyrad, reflection):
    rs = np.random.RandomState(11)
    mu, w = pyrad.fluxAngles(3)
    beam_w = [0.3, 0.2]
    # n = 1: the head-and-tail kernel alone
    k = hand_made_k(rs, 3, 1)
    check_raw(ctx, k, [1e4, 2e4, 1e4], [1.25], beam_w, rs.uniform(1.0, 3.0, (2, 3)), mu, w, 0.6, reflection)
    # L = 0: every level is the source, and the surface sends (1 - e) of it back
    n = 1027
    S0, e = rs.uniform(0.5, 1.5, n), rs.uniform(0.2, 0.9, n)
    sums, ut, ds, us = check_raw(ctx, np.zeros((0, n)), [], S0, beam_w, np.zeros((2, 0)), mu, w, e, reflection,
                                 bands=[(1, 515), (515, 516), (518, n)])
    m = inside(n, [(1, 515), (515, 516), (518, n)])
    assert rel_err(ds[m], (0.3 * S0 + 0.2 * S0)[m]) <= 1e-15
    # (1 - e, the product, the division by Wsum - itself two roundings - and three weighted terms: nine roundings at most)
    assert rel_err(us[m], ((1 - e) * ds)[m]) <= 9 * 2.0 ** -53 and np.array_equal(ut, us)
    sums, _, _, _ = run_raw(ctx, np.zeros((0, n)), [], S0, beam_w, np.zeros((2, 0)), mu, w, 0.25, reflection)
    assert rel_err(sums[0, 0, 0], 0.75 * sums[0, 1, 0]) <= 1e-13
    if reflection == "specular":                       # no angle is needed by a mirror
        check_raw(ctx, hand_made_k(rs, 2, n), [1e4, 1e4], S0, beam_w, rs.uniform(1.0, 3.0, (2, 2)), [], [], e, reflection)


@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_raw_layer_limit_eight_beams(ctx, pyrad, reflection):
    from pyrad_amd import _native
    rs = np.random.RandomState(13)
    L, n = _native.limit("layers_per_column"), 1029
    assert L == 128
    k = hand_made_k(rs, L, n, tau_lo=-6.5, tau_hi=-5.5)
    depth = list(rs.uniform(0.5e4, 1e4, L))
    mu, w = pyrad.fluxAngles(8)
    check_raw(ctx, k, depth, rs.uniform(0.5, 1.5, n), rs.uniform(0.05, 0.3, 8), rs.uniform(1.0, 4.0, (8, L)), mu, w,
              rs.uniform(0.1, 0.9, n), reflection)


@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_raw_zero_huge_inf_and_nan_coefficients(ctx, pyrad, reflection):
    """single points of 0, 1e300, inf and NaN: NaN goes through nan_to_num in the sums and stays a NaN in the spectra, as in
    NumPy; every other point keeps its value"""
    rs = np.random.RandomState(17)
    L, n = 3, 1029
    k = hand_made_k(rs, L, n)
    k[0, 5], k[1, 6], k[2, 7], k[1, 400] = 0.0, 1e300, np.inf, np.nan
    k[0, 1027], k[2, 1028], k[2, 514] = np.nan, np.inf, 1e300
    with np.errstate(invalid="ignore"):
        clean = np.where(np.isfinite(k) & (k < 1e299), k, 1e-5)
    mu, w = pyrad.fluxAngles(3)
    S0, e = rs.uniform(0.5, 1.5, n), rs.uniform(0.2, 0.9, n)
    slant = rs.uniform(1.0, 3.0, (2, L))
    args = ([1e4, 2e4, 1e4], S0, [0.3, 0.2], slant, mu, w, e, reflection)
    _, ut, ds, us = check_raw(ctx, k, *args)
    assert np.isnan(ds[400]) and np.isnan(ds[1027]) and np.isnan(ut[400]) and np.isnan(us[1027])
    assert ds[6] == 0.0 and ds[7] == 0.0 and ds[1028] == 0.0 and ds[514] == 0.0 and ds[5] > 0.0
    _, ut2, ds2, us2 = run_raw(ctx, clean, *args)
    same = np.all(k == clean, axis=0)
    assert same.sum() == n - 6
    for a, b in ((ut, ut2), (ds, ds2), (us, us2)):
        assert np.array_equal(a[same], b[same])


def test_raw_beyond_the_grid_stride_bound(ctx, pyrad):
    """1,024 workgroups of 1,024 points four times over, then the grid-stride loop's next round, and a tail of 1 point"""
    n = 1024 * 256 * 4 + 1029
    j = np.arange(n)
    k = np.stack([1e-6 * (1 + (j % 7)), 1e-6 * (1 + ((j + 3) % 7))])
    mu, w = pyrad.fluxAngles(3)
    S0 = 1.0 + 0.25 * ((j % 11) / 11.0)
    check_raw(ctx, k, [2e5, 1e5], S0, [0.5, 0.1], [[2.0, 1.9], [1.2, 1.1]], mu, w, 0.7, "lambertian", spectra=False)
    check_raw(ctx, k, [2e5, 1e5], S0, [0.5, 0.1], [[2.0, 1.9], [1.2, 1.1]], mu, w, 0.7, "specular")


# ---- 7. determinism ----------------------------------------------------------------------------------------------------
def test_deterministic_and_unmoved_by_other_calls(pyrad, lines):
    atm = column(pyrad)
    x = atm[0].xAxis
    kw = dict(solarSpectrum=solar_source(x), mu0=BEAMS["three"], geometry="spherical", emissivity=spectral_emissivity(x),
              bands=[(600, 640), (640, 701)], spectra=True)
    names = ("up", "down", "net", "heatingRate", "absorbedSurface", "upSpectrum", "downSpectrum", "upSurfaceSpectrum")
    for reflection in REFLECTIONS:
        a = atm.solarFluxes(reflection=reflection, **kw)
        b = atm.solarFluxes(reflection=reflection, **kw)
        atm.fluxes(surfaceTemperature=288, emissivity=0.9, spectra=True)
        atm.transmission(surfaceTemperature=288)
        c = atm.solarFluxes(reflection=reflection, **kw)
        cold = column(pyrad).solarFluxes(reflection=reflection, **kw)
        for name in names:
            for other in (b, c, cold):
                assert np.array_equal(getattr(a, name), getattr(other, name)), (reflection, name)


# ---- 8. laziness -------------------------------------------------------------------------------------------------------
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
    atm.solarFluxes(solarTemperature=5772.0, mu0=0.5)
    assert all(count == 0 for _, count in jobs), jobs
    atm.fluxes(surfaceTemperature=288)
    atm.solarFluxes(solarTemperature=5772.0, mu0=0.5, emissivity=0.8, reflection="specular")
    assert all(count == 0 for _, count in jobs), jobs
    atm[2].changeTemperature(250)                      # one layer due: one job for it alone
    jobs.clear()
    atm.solarFluxes(solarTemperature=5772.0, mu0=0.5)
    assert jobs == [("layers_merged_accumulate_dev", 1)], jobs


# ---- 9. refusals of the C entry point ----------------------------------------------------------------------------------
def test_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    rs = np.random.RandomState(5)
    L, n = 3, 1027
    k = hand_made_k(rs, L, n)
    nv = 2 * (L + 1)
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    level, ut, ds, us = ctx.buffer(nv), ctx.buffer(n), ctx.buffer(n), ctx.buffer(n)
    src, em = (ctx.buffer(n).upload(np.full(n, v)) for v in (1.1, 0.8))
    level_short, n_short = ctx.buffer(nv - 1), ctx.buffer(n - 1)
    i64, f64 = lambda v: (C.c_int64 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    nmax = _native.limit("flux_angles")
    inf, nan = float("inf"), float("nan")
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), depth=f64([1e4, 2e4, 1e4]), lo=600.0,
                hi=700.0, n=n, S0=src.h, n_beams=2, beam_weight=f64([0.5, 0.1]), slant=f64([2.0, 1.9, 1.8, 1.0, 1.0, 1.0]),
                n_angles=2, mu=f64([1.0, 0.5]), weight=f64([1.0, 2.0]), n_bands=1, band_first=i64([0]), band_count=i64([n]),
                emissivity=em.h, emissivity_all=0.5, reflection=0, level_flux=level.h, up_top=ut.h, down_surface=ds.h,
                up_surface=us.h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_solar_dev(*[a[key] for key in good])

    bad = [  # NULL arrays, negative counts
           dict(abs_coef=None), dict(depth=None), dict(S0=None), dict(beam_weight=None), dict(slant=None), dict(mu=None),
           dict(weight=None), dict(band_first=None), dict(band_count=None), dict(level_flux=None), dict(n_layers=-1),
           dict(n=-5), dict(n_beams=-1), dict(n_angles=-1), dict(n_angles=-1, reflection=1), dict(n_bands=-1),
           # counts beyond their limits (and too few)
           dict(n_layers=_native.limit("layers_per_column") + 1), dict(n_beams=0),
           dict(n_beams=nmax + 1, beam_weight=f64([0.1] * (nmax + 1)), slant=f64([1.0] * (L * (nmax + 1)))),
           dict(n_angles=nmax + 1, mu=f64([0.5] * (nmax + 1)), weight=f64([1.0] * (nmax + 1))), dict(n_angles=0),
           dict(n_bands=0), dict(n_bands=_native.limit("flux_bands") + 1),
           # buffers shorter than n
           dict(level_flux=level_short.h), dict(S0=n_short.h), dict(up_top=n_short.h), dict(down_surface=n_short.h),
           dict(up_surface=n_short.h), dict(emissivity=n_short.h), dict(abs_coef=(C.c_void_p * L)(kb[0].h, n_short.h, kb[2].h)),
           # bands
           dict(band_count=i64([n + 1])), dict(band_first=i64([-1])), dict(band_count=i64([0])), dict(band_first=i64([n])),
           # depths, slants, beam weights
           dict(depth=f64([1e4, -1.0, 1e4])), dict(depth=f64([1e4, nan, 1e4])),
           dict(slant=f64([2.0, 1.9, 1.8, 1.0, -1e-9, 1.0])), dict(slant=f64([2.0, inf, 1.8, 1.0, 1.0, 1.0])),
           dict(slant=f64([2.0, 1.9, 1.8, 1.0, 1.0, nan])),
           dict(beam_weight=f64([0.5, inf])), dict(beam_weight=f64([nan, 0.1])),
           # angles
           dict(mu=f64([1.0, 0.0])), dict(mu=f64([1.0, 1.5])), dict(mu=f64([nan, 0.5])), dict(weight=f64([1.0, inf])),
           # the surface
           dict(reflection=2), dict(reflection=-1),
           dict(emissivity=None, emissivity_all=-0.01), dict(emissivity=None, emissivity_all=1.01),
           dict(emissivity=None, emissivity_all=nan),
           dict(weight=f64([1.0, -1.0])), dict(weight=f64([1.0, -2.0])), dict(weight=f64([1e308, 1e308])),
           dict(weight=f64([1.0, nan]))]
    outs = (level, ut, ds, us)
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
        for b in outs:
            assert np.all(b.download() == -7.0)
        assert call(emissivity_all=7.0) == 0                # not looked at beside a buffer
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        # what is allowed: no spectra, one emissivity, a mirror without angles, weights that a mirror does not add up
        assert call(up_top=None, down_surface=None, up_surface=None, emissivity=None, reflection=1) == 0
        assert call(reflection=1, n_angles=0, mu=None, weight=None) == 0
        assert call(reflection=1, weight=f64([1.0, -1.0])) == 0
        assert call(slant=f64([0.0] * 6), beam_weight=f64([0.0, -1.0])) == 0
        level.download()                                    # (the queue drains without an error)
    finally:
        for b in kb + [level, ut, ds, us, src, em, level_short, n_short]:
            b.free()


# ---- 10. the thermal fluxes are untouched ---------------------------------------------------------------------------------
def test_thermal_fluxes_keep_their_bits(pyrad, lines):
    atm = column(pyrad)
    x = atm[0].xAxis
    names = ("up", "down", "net", "heatingRate", "upSpectrum", "downSpectrum", "upSurfaceSpectrum")
    kw = dict(surfaceTemperature=288, emissivity=0.9, spectra=True)
    before = atm.fluxes(**kw)
    black = atm.fluxes(surfaceTemperature=288, spectra=True)
    for reflection in REFLECTIONS:
        atm.solarFluxes(solarSpectrum=solar_source(x), mu0=BEAMS["eight"], emissivity=0.2, reflection=reflection, angles=8,
                        bands=[(600, 650), (650, 701)], spectra=True)
        after = atm.fluxes(**kw)
        for name in names:
            assert np.array_equal(getattr(before, name), getattr(after, name)), (reflection, name)
    again = atm.fluxes(surfaceTemperature=288, spectra=True)
    for name in names[:-1]:
        assert np.array_equal(getattr(black, name), getattr(again, name)), name
