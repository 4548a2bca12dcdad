"""GPU: the linear-in-optical-depth Planck source - Atmosphere.fluxes and radiance with planck="linear"
(lbl_column_flux_linear_dev, lbl_ray_radiance_linear_dev, kernels K5i) - for its identity with the layer source, against a
NumPy restatement of its semantics (written out below), for the direction of its two temperatures against 128 isothermal
layers, in its physical limits, for the Lambertian start term, and for independence of the rays, determinism, the
instrument, laziness and the C ABI's refusals.  Column, lines, rays and synthetic coefficients are tests/test_gpu_paths.py's."""
import ctypes as C
import decimal

import numpy as np
import pytest

from conftest import rel_err
from oracle import pyrad_oracle as orc
from test_gpu_paths import LAYERS, TOL, band_of_rays, column, ctx, lines, nine_paths, pyrad, synthetic_k  # noqa: F401

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
MARKER = -1           # the segment layer of a surface marker
RNG = (600, 610.07)   # about 1,000 points at multiplier 1, with a tail that is no multiple of 4
# Tolerances: tests/test_gpu_flux.py's for fluxes (spectra 1e-13 with a floor of 1e-300 on downward ones, band fluxes 1e-12,
# heating rates 1e-10) and tests/test_gpu_paths.py's for rays (TOL = 1e-13; radiance floor 1e-300 for rays from space,
# transmittance floor 1e-30).
TOL_BAND, TOL_HEAT = 1e-12, 1e-10
# A ray whose thinnest segment has tau_min < THIN = 2^-52 / 1e-13 is held to max(1e-13, 2^-52 / tau_min): 1 - t of a t that
# lies within an ulp (2^-53 below 1, on either side) of the true one is 2^-52 / tau apart at worst, in NumPy's 1 - t as in the
# kernel's (the reason tests/test_gpu_paths.py has TOL_THIN_LIMB).  It applies to no transmittance and to no other ray.
EPS = 2.0 ** -52
THIN = EPS / TOL
LEVELS = np.array([295.0, 280.0, 255.0, 230.0, 212.0])       # a lapse over the four layers of the model column
G_TAU0 = 0.25


# ---- the semantics, restated in NumPy (include/pyrad_hip.h, "linear-in-optical-depth Planck source") ------------------------
def g_of(tau, t):
    """g(tau) = 1 - (1 - t) / tau, by its Taylor series tau (1/2 - tau (1/6 - tau (1/24 - ...))) below tau_0"""
    tau = np.asarray(tau, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        direct = 1.0 - (1.0 - t) / tau
        s = np.zeros_like(tau)
        for n in range(20, -1, -1):                     # 1 / (n + 2)!
            s = 1.0 / float(np.prod(np.arange(1.0, n + 3.0))) - tau * s
        return np.where(tau >= G_TAU0, direct, tau * s)


def step(I, tau, Ba, Bb):
    """I <- t I + (1 - t) Ba + g(tau) (Bb - Ba); also t"""
    t = np.exp(-tau)
    return t * I + (1 - t) * Ba + g_of(tau, t) * (Bb - Ba), t


def leaving(e, Is, R):
    return e * Is + (1 - e) * R


def walk(x, k, layers, lengths, temps, kind, e=1.0, Is=None, Rd=None):
    """(radiance, transmittance, smallest optical depth > 0) of one ray: k[l] the absorption coefficient of layer l on the
    grid x, temps[s] = (Ta, Tb) of segment s in the direction of travel; kind 1: the ray starts at the surface with e Is +
    (1 - e) Rd (Rd None: 0), kind 0: in cold space; a layer of MARKER is where the ray meets the surface"""
    I = np.zeros(x.size) if kind == 0 else leaving(e, Is, 0.0 if Rd is None else Rd) * np.ones(x.size)
    Tt = np.ones(x.size)
    tau_min = np.inf
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        for l, s, (Ta, Tb) in zip(layers, lengths, temps):
            if l == MARKER:
                I = leaving(e, Is, I)
                Tt = Tt * (1 - e)
                continue
            tau = k[l] * s
            if np.any(tau > 0):
                tau_min = min(tau_min, float(np.min(tau[tau > 0])))
            I, t = step(I, tau, orc.planckWavenumber(x, Ta), orc.planckWavenumber(x, Tb))
            Tt = Tt * t
    return I, Tt, tau_min


def weight_sum(weight):
    total = 0.0
    for w in weight:
        total += float(w)
    return total


def flux_walk(x, k, edges, depth, mu, weight, Is, e, reflection, top=None, idx=None):
    """lbl_column_flux_linear_dev: (up, down) sums [band, level] over the bands idx = [(first, end)], and the spectral F_up
    at the top, F_down at the surface and F_up at the surface; edges[l] = (bottom, top) temperature of layer l"""
    n, nl = x.size, len(k)
    idx = idx or [(0, n)]

    def level(I):
        F = sum(w * Ik for w, Ik in zip(weight, I))                   # spectral flux sum_k W_k I_k, angle 0 first
        return F, [np.sum(np.nan_to_num(F[a:b])) for a, b in idx]

    def layer(l, I, up):
        Ta, Tb = (edges[l][0], edges[l][1]) if up else (edges[l][1], edges[l][0])
        Ba, Bb = orc.planckWavenumber(x, Ta), orc.planckWavenumber(x, Tb)
        for i, m in enumerate(mu):
            I[i] = step(I[i], (k[l] * depth[l]) * (1.0 / m), Ba, Bb)[0]

    up, down = np.zeros((len(idx), nl + 1)), np.zeros((len(idx), nl + 1))
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        I = [(np.zeros(n) if top is None else np.array(top, dtype=np.float64)) for _ in mu]
        F, down[:, nl] = level(I)
        for l in range(nl - 1, -1, -1):
            layer(l, I, False)
            F, down[:, l] = level(I)
        sd = F
        R = [F / weight_sum(weight) for _ in mu] if reflection == "lambertian" else I
        I = [leaving(e, Is, Rk) * np.ones(n) for Rk in R]
        s0, up[:, 0] = level(I)
        F = s0
        for l in range(nl):
            layer(l, I, True)
            F, up[:, l + 1] = level(I)
    return up, down, F, sd, s0


def model_columns(pyrad, atm):
    return (np.asarray(atm[0].xAxis), [np.array(pyrad.getAbsCoef(L)) for L in atm], [L.T for L in atm],
            [L.depth for L in atm])


def spectral_emissivity(x):
    return 0.775 + 0.225 * np.cos(np.linspace(0.0, 9.0 * np.pi, x.size))


def check_rays(kinds, got_I, got_T, want):
    worst = []
    for r, kind in enumerate(kinds):
        eI = rel_err(got_I[r], want[r][0], floor=1e-300 if kind == 0 else 0.0)
        eT = rel_err(got_T[r], want[r][1], floor=1e-30)
        tau_min = want[r][2]
        bound = max(TOL, EPS / tau_min) if tau_min < THIN else TOL
        print("ray %d: radiance %.2e (bound %.2e, tau_min %.2e) transmittance %.2e" % (r, eI, bound, tau_min, eT))
        worst.append((r, eI, eT, bound))
    for r, eI, eT, bound in worst:
        assert eI <= bound and eT <= TOL, (r, eI, eT, bound)


# ---- raw calls on uploaded coefficients ---------------------------------------------------------------------------------
REFLECTIONS = ("lambertian", "specular")


def run_raw_flux(ctx, k, edges, depth, mu, w, e, reflection, lo=600.0, hi=700.0, source_T=0.0, I_source=None, top=None,
                 bands=None, entry="linear"):
    """lbl_column_flux_linear_dev (or, entry "black", lbl_column_flux_dev with edges the layers' temperatures) on uploaded
    coefficients: (level sums [band, 2, level], up_top, down_surface, up_surface)"""
    L, n = len(k), len(k[0]) if len(k) else len(top)
    first, count = ([0], [n]) if bands is None else ([a for a, _ in bands], [b - a for a, b in bands])
    nb = len(first)
    bufs = [ctx.buffer(n).upload(np.ascontiguousarray(k[l])) for l in range(L)]
    level, ut, ds, us = ctx.buffer(nb * 2 * (L + 1)), ctx.buffer(n), ctx.buffer(n), ctx.buffer(n)
    bufs += [level, ut, ds, us]
    src = eb = tb = None
    try:
        if I_source is not None:
            src = ctx.buffer(n).upload(I_source); bufs.append(src)
        if np.ndim(e):
            eb = ctx.buffer(n).upload(e); bufs.append(eb)
        if top is not None:
            tb = ctx.buffer(n).upload(top); bufs.append(tb)
        if entry == "black":
            ctx.column_flux_dev(bufs[:L], edges, depth, lo, hi, n, mu, w, first, count, level, I_surface=src,
                                surface_T=source_T, I_top=tb, up_top=ut, down_surface=ds)
        else:
            ctx.column_flux_linear_dev(bufs[:L], edges, depth, lo, hi, n, mu, w, first, count, level,
                                       eb if eb is not None else e, reflection=REFLECTIONS.index(reflection), I_surface=src,
                                       surface_T=source_T, I_top=tb, up_top=ut, down_surface=ds, up_surface=us)
        return level.download(nb * 2 * (L + 1)).reshape(nb, 2, L + 1), ut.download(n), ds.download(n), us.download(n)
    finally:
        for b in bufs:
            b.free()


def run_raw_rays(ctx, k, rays, e=1.0, lo=600.0, hi=700.0, I_source=None, source_T=0.0, down=None, norm=0.0):
    """rays: [(layers, lengths, kind, temps)] -> (radiance, transmittance), R x n each"""
    L, n = len(k), len(k[0])
    bufs = [ctx.buffer(n).upload(np.ascontiguousarray(k[l])) for l in range(L)]
    bufs += [ctx.buffer(len(rays) * n), ctx.buffer(len(rays) * n)]
    rad, trn = bufs[-2:]
    src = eb = db = None
    try:
        if I_source is not None:
            src = ctx.buffer(n).upload(I_source); bufs.append(src)
        if np.ndim(e):
            eb = ctx.buffer(n).upload(e); bufs.append(eb)
        if down is not None:
            db = ctx.buffer(n).upload(down); bufs.append(db)
        ctx.ray_radiance_linear_dev(bufs[:L], [t for r in rays for pair in r[3] for t in pair], lo, hi, n,
                                    np.cumsum([0] + [len(r[0]) for r in rays]), [l for r in rays for l in r[0]],
                                    [s for r in rays for s in r[1]], [r[2] for r in rays], rad, eb if eb is not None else e,
                                    I_source=src, source_T=source_T, surface_down=db, surface_down_norm=norm, transmittance=trn)
        return rad.download().reshape(len(rays), n), trn.download().reshape(len(rays), n)
    finally:
        for b in bufs:
            b.free()


def with_temperatures(path, temps, pyrad):
    return pyrad.Path(path.layers, path.lengths, path.source, path.name, bounce=path.bounce, temperatures=temps)


# ---- 1. identity with the layer source -----------------------------------------------------------------------------------
@pytest.mark.parametrize("reflection", REFLECTIONS)
def test_equal_edges_are_the_layer_source_fluxes(pyrad, lines, ctx, reflection):
    from pyrad_amd import settings
    atm = column(pyrad, rng=RNG)
    x, k, T, depth = model_columns(pyrad, atm)
    n = x.size
    assert n % 4 != 0
    cut = [0, 101, 502, 503, 807, n]
    idx = list(zip(cut[:-1], cut[1:]))
    bands = [(x[a], x[b] if b < n else np.inf) for a, b in idx]
    top = 0.3 * np.array(atm[0].planck(250))
    edges = [(t, t) for t in T]
    res = settings.BASE_RESOLUTION
    for angles in (1, 3, 8):
        mu, w = pyrad.fluxAngles(angles)
        for e in (None, 0.7, spectral_emissivity(x)):
            for kw, raw in ((dict(surfaceTemperature=288), dict(source_T=288.0)),
                            (dict(surfaceSpectrum=atm[0].planck(300), topSpectrum=top, bands=bands),
                             dict(I_source=np.array(atm[0].planck(300)), top=top, bands=idx))):
                want = atm.fluxes(angles=angles, spectra=True, emissivity=e, reflection=reflection, **kw)
                sums, ut, ds, us = run_raw_flux(ctx, k, edges, depth, mu, w, 1.0 if e is None else e, reflection,
                                                lo=atm[0].rangeMin, hi=atm[0].rangeMax, **raw)
                sums = sums * res
                up, down = (sums[:, 0], sums[:, 1]) if "bands" in kw else (sums[0, 0], sums[0, 1])
                assert np.array_equal(up, want.up) and np.array_equal(down, want.down), (angles, np.ndim(e), sorted(kw))
                assert np.array_equal(ut, want.upSpectrum) and np.array_equal(ds, want.downSpectrum)
                if e is not None:
                    assert np.array_equal(us, want.upSurfaceSpectrum)


def test_equal_segment_temperatures_are_the_layer_source_radiance(pyrad, lines, ctx):
    atm = column(pyrad, rng=RNG)
    x, k, T, depth = model_columns(pyrad, atm)
    same = lambda p: with_temperatures(p, [(T[l], T[l]) for l in p.layers], pyrad)
    nine = nine_paths(pyrad, atm)
    mirror = atm.reflectedPath(mu=0.6)
    for kw in (dict(surfaceTemperature=288), dict(surfaceSpectrum=atm[0].planck(300))):
        # the black-surface call
        want = atm.radiance(nine, transmittance=True, **kw)
        got = atm.radiance([same(p) for p in nine], transmittance=True, planck="linear", **kw)
        assert np.array_equal(got.radiance, want.radiance) and np.array_equal(got.transmittance, want.transmittance)
        # the emissivity call; the path with a bounce goes through it alone
        for e in (0.7, spectral_emissivity(x)):
            want = atm.radiance(nine + [mirror], transmittance=True, emissivity=e, reflection="specular", **kw)
            got = atm.radiance([same(p) for p in nine + [mirror]], transmittance=True, emissivity=e, reflection="specular",
                               planck="linear", **kw)
            assert np.array_equal(got.radiance, want.radiance) and np.array_equal(got.transmittance, want.transmittance)
    # ... and with the Lambertian start term, through the raw entry: the layer source's downward flux handed in
    mu, w = pyrad.fluxAngles(3)
    e = 0.7
    want = atm.radiance(nine + [mirror], surfaceTemperature=288, transmittance=True, emissivity=e)
    down = atm.fluxes(surfaceTemperature=288, spectra=True).downSpectrum
    rays = [(*p._segments(), 1 if p.source == "surface" else 0, same(p)._segment_temperatures()) for p in nine + [mirror]]
    got_I, got_T = run_raw_rays(ctx, k, rays, e, lo=atm[0].rangeMin, hi=atm[0].rangeMax, source_T=288.0, down=down,
                                norm=weight_sum(w))
    assert np.array_equal(got_I, want.radiance) and np.array_equal(got_T, want.transmittance)


def test_an_isothermal_column_is_the_layer_source_through_the_model(pyrad, lines):
    atm = column(pyrad, rng=RNG, layers=tuple((d, 255, P) for d, _, P in LAYERS))
    assert np.array_equal(atm.levelTemperatures(), np.full(5, 255.0))
    x = atm[0].xAxis
    top = 0.3 * np.array(atm[0].planck(250))
    for kw in (dict(), dict(emissivity=0.7), dict(emissivity=spectral_emissivity(x), reflection="specular")):
        a = atm.fluxes(surfaceTemperature=288, topSpectrum=top, spectra=True, **kw)
        b = atm.fluxes(surfaceTemperature=288, topSpectrum=top, spectra=True, planck="linear", **kw)
        for name in ("up", "down", "net", "heatingRate", "upSpectrum", "downSpectrum"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        if kw:
            assert np.array_equal(a.upSurfaceSpectrum, b.upSurfaceSpectrum)
    old = [atm.nadirPath(), atm.nadirPath(mu=0.4), atm.zenithPath(mu=0.3), atm.zenithPath(observerLevel=2)]
    new = [atm.nadirPath(levelTemperatures=True), atm.nadirPath(mu=0.4, levelTemperatures=True),
           atm.zenithPath(mu=0.3, levelTemperatures=True), atm.zenithPath(observerLevel=2, levelTemperatures=True)]
    for kw in (dict(), dict(emissivity=0.7), dict(emissivity=0.7, reflection="specular")):
        bounce = ([atm.reflectedPath()], [atm.reflectedPath(levelTemperatures=True)]) if kw else ([], [])
        a = atm.radiance(old + bounce[0], surfaceTemperature=288, transmittance=True, **kw)
        b = atm.radiance(new + bounce[1], surfaceTemperature=288, transmittance=True, planck="linear", **kw)
        assert np.array_equal(a.radiance, b.radiance) and np.array_equal(a.transmittance, b.transmittance), sorted(kw)


def test_ray_down_and_up_is_the_specular_flux_of_one_vertical_angle(pyrad, lines):
    atm = column(pyrad, rng=RNG)
    x = atm[0].xAxis
    for e in (0.6, spectral_emissivity(x)):
        flux = atm.fluxes(surfaceTemperature=288, emissivity=e, reflection="specular", angles=[(1.0, 1.0)], spectra=True,
                          planck="linear", levelTemperatures=LEVELS)
        ray = atm.radiance(atm.reflectedPath(levelTemperatures=LEVELS), surfaceTemperature=288, emissivity=e,
                           reflection="specular", planck="linear")
        assert np.array_equal(ray.radiance[0], flux.upSpectrum)
        ray = atm.radiance(atm.reflectedPath(observerLevel=0, levelTemperatures=LEVELS), surfaceTemperature=288, emissivity=e,
                           reflection="specular", planck="linear")
        assert np.array_equal(ray.radiance[0], flux.upSurfaceSpectrum)


# ---- 2. against NumPy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angles", [1, 3, 8])
def test_fluxes_against_numpy(pyrad, lines, angles):
    from pyrad_amd import settings
    atm = column(pyrad, rng=RNG)
    x, k, T, depth = model_columns(pyrad, atm)
    edges = list(zip(LEVELS[:-1], LEVELS[1:]))
    mu, w = pyrad.fluxAngles(angles)
    res = settings.BASE_RESOLUTION
    top = 0.3 * np.array(atm[0].planck(250))
    Is = orc.planckWavenumber(x, 288)
    heat = lambda net: pyrad.heatingRates(net, [L.P for L in atm], T, depth)
    for reflection in REFLECTIONS:
        for e in (None, 0.9, spectral_emissivity(x)):
            for t in (None, top):
                f = atm.fluxes(surfaceTemperature=288, topSpectrum=t, angles=angles, spectra=True, emissivity=e,
                               reflection=reflection, planck="linear", levelTemperatures=LEVELS)
                fu, fd, su, sd, s0 = flux_walk(x, k, edges, depth, mu, w, Is, 1.0 if e is None else e, reflection, top=t)
                fu, fd = fu[0] * res, fd[0] * res
                errs = [rel_err(f.up, fu), rel_err(f.down, fd, floor=1e-300), rel_err(f.net, fu - fd),
                        rel_err(f.heatingRate, heat(fu - fd)), rel_err(f.upSpectrum, su),
                        rel_err(f.downSpectrum, sd, floor=1e-300)]
                if e is not None:
                    errs.append(rel_err(f.upSurfaceSpectrum, s0))
                else:
                    assert f.upSurfaceSpectrum is None
                print(reflection, "black" if e is None else np.ndim(e), t is not None, " ".join("%.2e" % v for v in errs))
                assert f.up.shape == f.down.shape == (len(atm) + 1,)
                assert errs[0] <= TOL_BAND and errs[1] <= TOL_BAND and errs[2] <= TOL_BAND
                assert errs[3] <= TOL_HEAT
                assert all(v <= 1e-13 for v in errs[4:])
    # None: the default level temperatures
    a = atm.fluxes(surfaceTemperature=288, angles=angles, spectra=True, planck="linear")
    b = atm.fluxes(surfaceTemperature=288, angles=angles, spectra=True, planck="linear", levelTemperatures=atm.levelTemperatures())
    assert np.array_equal(a.up, b.up) and np.array_equal(a.upSpectrum, b.upSpectrum)
    assert not np.array_equal(a.up, atm.fluxes(surfaceTemperature=288, angles=angles).up)


def linear_rays(rs, L):
    """band_of_rays' rays with random segment temperatures - the five over one layer sequence share theirs, so four of them
    travel as a bundle - then with markers at the front, in the middle and at the back; marker-only rays; five rays over one
    marked sequence of which the last has temperatures of its own (it must not join the others' bundle)"""
    temps = lambda ns: [tuple(v) for v in rs.uniform(200.0, 310.0, (ns, 2))]
    rays, shared = [], temps(L)
    for i, (lay, lens, kind) in enumerate(band_of_rays(rs, L)):
        rays.append((lay, lens, kind, shared if i < 5 else temps(len(lay))))
    for lay, lens, kind, tt in list(rays[4:7]):
        ns = len(lay)
        for where in ([0], [ns // 2], [0, ns]):
            lay2, lens2, tt2 = list(lay), list(lens), list(tt)
            for i in sorted(where, reverse=True):
                lay2.insert(i, MARKER); lens2.insert(i, 0.0); tt2.insert(i, (float("nan"), -1.0))    # a marker's pair is ignored
            rays.append((lay2, lens2, kind, tt2))
    rays += [([MARKER], [0.0], 0, [(0.0, 0.0)]), ([MARKER], [0.0], 1, [(0.0, 0.0)])]
    seq = [L - 1, 1, 0, MARKER, 0, 1]
    tt = temps(3) + [(0.0, 0.0)] + temps(2)
    for i in range(5):
        lens = list(rs.uniform(0.5e4, 2e4, 3)) + [0.0] + list(rs.uniform(0.5e4, 2e4, 2))
        rays.append((seq, lens, i % 2, tt if i < 4 else temps(3) + [(0.0, 0.0)] + temps(2)))
    return rays


def thin_emission(tau, Ba, Bb):
    """(1 - t) Ba + g(tau) (Bb - Ba) from cold space at 50 digits, g by its series (tau is small): the small-tau form
    tau (Ba + Bb) / 2 - tau^2 (Ba / 3 + Bb / 6) + ..."""
    c = decimal.Context(prec=50)
    out = np.empty(len(Ba))
    x = decimal.Decimal(float(tau))
    one_minus_t = c.subtract(1, c.exp(-x))
    g, term = decimal.Decimal(0), x / 2
    for n in range(30):
        g = c.add(g, term)
        term = c.divide(c.multiply(-term, x), decimal.Decimal(n + 3))
    for j in range(len(Ba)):
        a, b = decimal.Decimal(float(Ba[j])), decimal.Decimal(float(Bb[j]))
        out[j] = float(c.add(c.multiply(one_minus_t, a), c.multiply(g, c.subtract(b, a))))
    return out


@pytest.mark.parametrize("n", [3, 1027, 5003])
def test_raw_rays_and_fluxes_against_numpy(ctx, pyrad, n):
    rs = np.random.RandomState(300 + n)
    L = 4
    # rows 4 and 5: k = 1e-7 and 1e-9, tau = 1e-3 and 1e-5 over 1e4 cm - the series of g, which synthetic_k's depths never reach
    k = np.vstack([synthetic_k(rs, L, n), np.full((1, n), 1e-7), np.full((1, n), 1e-9)])
    x = np.linspace(600.0, 700.0, n)
    rays = linear_rays(rs, L)
    e = rs.uniform(0.5, 1.0, n)
    e[::7] = 1.0
    e[3::11] = 0.0
    for ee, kw in ((0.8, dict(source_T=295.0)),
                   (e, dict(I_source=rs.uniform(0.0, 0.2, n), down=rs.uniform(0.0, 0.5, n), norm=2.75))):
        got_I, got_T = run_raw_rays(ctx, k, rays, ee, **kw)
        Is = kw["I_source"] if "I_source" in kw else orc.planckWavenumber(x, 295.0)
        Rd = kw["down"] / kw["norm"] if "down" in kw else None
        want = [walk(x, k, r[0], r[1], r[3], r[2], ee, Is, Rd) for r in rays]
        check_rays([r[2] for r in rays], got_I, got_T, want)
    # the two thin rays, from cold space, against the small-tau form in decimal - not against NumPy's 1 - t
    thin = [([4], [1e4], 0, [(250.0, 300.0)]), ([5], [1e4], 0, [(300.0, 250.0)])]
    got_I, got_T = run_raw_rays(ctx, k, thin, 1.0)
    for r, (lay, lens, _, tt) in enumerate(thin):
        tau = k[lay[0]][0] * lens[0]
        want = thin_emission(tau, orc.planckWavenumber(x, tt[0][0]), orc.planckWavenumber(x, tt[0][1]))
        bound = max(TOL, EPS / tau)
        err = rel_err(got_I[r], want)
        print("thin ray tau %.1e: %.2e (bound %.2e)" % (tau, err, bound))
        assert tau < G_TAU0 and tau < THIN and err <= bound
        assert rel_err(got_T[r], np.full(n, np.exp(-tau))) <= TOL
    # the flux entry on the same coefficients
    edges = [tuple(v) for v in rs.uniform(200.0, 310.0, (L, 2))]
    depth = list(rs.uniform(0.5e4, 2e4, L))
    bands = [(1, n // 2), (n // 2, n // 2 + 1), (n // 2 + 2, n)] if n > 8 else None
    top = rs.uniform(0.0, 0.2, n)
    for angles in (3, 8):
        mu, w = pyrad.fluxAngles(angles)
        for reflection in REFLECTIONS:
            sums, ut, ds, us = run_raw_flux(ctx, k[:L], edges, depth, mu, w, e, reflection, source_T=295.0, top=top, bands=bands)
            fu, fd, su, sd, s0 = flux_walk(x, k[:L], edges, depth, mu, w, orc.planckWavenumber(x, 295.0), e, reflection,
                                           top=top, idx=bands)
            if bands is not None:                        # (points outside every band keep 0 in the spectra)
                inside = np.zeros(n, dtype=bool)
                for a, b in bands:
                    inside[a:b] = True
                su, sd, s0 = (np.where(inside, v, 0.0) for v in (su, sd, s0))
            errs = (rel_err(sums[:, 0], fu), rel_err(sums[:, 1], fd, floor=1e-300), rel_err(ut, su),
                    rel_err(ds, sd, floor=1e-300), rel_err(us, s0))
            print(reflection, n, angles, " ".join("%.2e" % v for v in errs))
            assert errs[0] <= TOL_BAND and errs[1] <= TOL_BAND
            assert errs[2] <= 1e-13 and errs[3] <= 1e-13 and errs[4] <= 1e-13


def ten_paths(pyrad, atm, lev):
    return [atm.nadirPath(levelTemperatures=lev), atm.nadirPath(mu=0.4, levelTemperatures=lev),
            atm.nadirPath(observerLevel=2, levelTemperatures=lev), atm.zenithPath(levelTemperatures=lev),
            atm.zenithPath(mu=0.3, levelTemperatures=lev), atm.zenithPath(observerLevel=2, levelTemperatures=lev),
            atm.limbPath(5e3, levelTemperatures=lev), atm.limbPath(2.5e4, levelTemperatures=lev),
            atm.limbPath(1.7e5, levelTemperatures=lev), pyrad.Path([], [], source="surface", temperatures=[])]


def test_ten_paths_against_numpy(pyrad, lines):
    atm = column(pyrad, rng=RNG)
    x, k, T, depth = model_columns(pyrad, atm)
    paths = ten_paths(pyrad, atm, LEVELS)
    for kw, Is in ((dict(surfaceTemperature=288), orc.planckWavenumber(x, 288)),
                   (dict(surfaceSpectrum=atm[0].planck(300)), np.array(atm[0].planck(300)))):
        got = atm.radiance(paths, transmittance=True, planck="linear", **kw)
        assert got.radiance.shape == got.transmittance.shape == (len(paths), x.size) and got.paths == paths
        kinds = [1 if p.source == "surface" else 0 for p in paths]
        want = [walk(x, k, p.layers, p.lengths, p.temperatures, kind, 1.0, Is) for p, kind in zip(paths, kinds)]
        check_rays(kinds, got.radiance, got.transmittance, want)
    # the source matters: the layer source along the same geometry is something else
    layer = atm.radiance(nine_paths(pyrad, atm)[:1], surfaceTemperature=288)
    linear = atm.radiance(paths[:1], surfaceTemperature=288, planck="linear")
    assert rel_err(linear.radiance[0], layer.radiance[0]) > 1e-6


# ---- 3. direction and physics, independent of the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("mu", [1.0, 0.3])
def test_four_linear_layers_against_128_isothermal_ones(ctx, mu):
    """A column of depth 1.6e5 cm with one k row for every layer (total optical depth 0.05 .. 50 at mu = 1), T falling
    linearly with height from 290 K to 210 K over a surface at 290 K.  Reference: the EXISTING lbl_column_flux_dev on 128 equal
    isothermal layers.  On 4 layers the linear source must be at least 10 times closer to it than the isothermal one, at the
    top and at the surface (NumPy on this arithmetic: 31 and 28 times at mu = 1, 36 and 32 times at mu = 0.3): a swapped
    entry and exit in either walk costs that."""
    rs = np.random.RandomState(77)
    n, Z = 1027, 1.6e5
    krow = 10.0 ** rs.uniform(np.log10(0.05), np.log10(50.0), n) / Z
    T_at = lambda z: 290.0 - 80.0 * z / Z
    angles = ([mu], [1.0])

    def run(L, linear):
        z = np.linspace(0.0, Z, L + 1)
        temps = [(T_at(a), T_at(b)) for a, b in zip(z[:-1], z[1:])] if linear else [T_at((a + b) / 2) for a, b in zip(z[:-1], z[1:])]
        _, ut, ds, _ = run_raw_flux(ctx, [krow] * L, temps, [Z / L] * L, *angles, 1.0, "lambertian", source_T=290.0,
                                    entry="linear" if linear else "black")
        return ut, ds

    ref = run(128, False)
    iso, lin = run(4, False), run(4, True)
    for name, r, a, b in zip(("up at the top", "down at the surface"), ref, iso, lin):
        e_iso, e_lin = rel_err(a, r), rel_err(b, r)
        print("mu %.1f %s: isothermal %.3e linear %.3e ratio %.1f" % (mu, name, e_iso, e_lin, e_iso / e_lin))
        assert e_lin <= e_iso / 10.0, (name, e_iso, e_lin)


# ---- 4. limits -----------------------------------------------------------------------------------------------------------
def test_one_opaque_layer_shows_the_edge_it_is_seen_from(ctx):
    n, tau = 1027, 1e4
    x = np.linspace(600.0, 700.0, n)
    _, ut, ds, _ = run_raw_flux(ctx, [np.full(n, 1.0)], [(250.0, 300.0)], [tau], [1.0], [1.0], 1.0, "lambertian", source_T=280.0)
    up, down = rel_err(ut, orc.planckWavenumber(x, 300.0)), rel_err(ds, orc.planckWavenumber(x, 250.0))
    print("opaque: up %.2e down %.2e (2 / tau = %.1e)" % (up, down, 2 / tau))
    assert up <= 2 / tau and down <= 2 / tau
    assert up > 1e-6 and down > 1e-6                     # ... and not the edge itself: g = 1 - 1 / tau


def test_one_thin_layer_emits_the_mean_of_its_edges(ctx):
    """tau = 2^-10 exactly (k = 2^-20 over 1,024 cm).  From cold space the layer emits (1 - t) Ba + g (Bb - Ba) = tau (Ba +
    Bb) / 2 - tau^2 (Ba / 3 + Bb / 6) + O(tau^3): its distance from tau (Ba + Bb) / 2 is tau^2 on the scale of the mean Planck
    value (Ba + Bb) / 2 - the issue's "within tau^2 relative", read on that scale, since against tau (Ba + Bb) / 2 itself the
    second-order term is tau (2 Ba + Bb) / (3 (Ba + Bb)), about tau / 2, for every correct implementation.  A source that took
    one edge for both is tau |Bb - Ba| / 2 away, 200 times as far here.  The second-order term is checked as well."""
    n = 1027
    tau = 2.0 ** -10
    x = np.linspace(600.0, 700.0, n)
    Bbot, Btop = orc.planckWavenumber(x, 250.0), orc.planckWavenumber(x, 300.0)
    _, ut, ds, _ = run_raw_flux(ctx, [np.full(n, 2.0 ** -20)], [(250.0, 300.0)], [1024.0], [1.0], [1.0], 1.0, "lambertian",
                                I_source=np.zeros(n))
    mean = (Bbot + Btop) / 2
    for name, got, Ba, Bb in (("up", ut, Bbot, Btop), ("down", ds, Btop, Bbot)):
        first = np.max(np.abs(got - tau * mean) / mean)
        second = rel_err(got, tau * mean - tau ** 2 * (Ba / 3 + Bb / 6))
        print("thin %s: %.3e of the mean Planck value (tau^2 = %.3e); with the second-order term %.3e" % (name, first, tau ** 2, second))
        assert first <= tau ** 2
        assert second <= tau ** 2
    assert not np.array_equal(ut, ds)


def test_isothermal_cavity_has_no_net_flux(pyrad, lines):
    from pyrad_amd import settings
    atm = column(pyrad, rng=RNG, layers=tuple((d, 260, P) for d, _, P in LAYERS))
    x = atm[0].xAxis
    B = orc.planckWavenumber(x, 260)
    for reflection in REFLECTIONS:
        f = atm.fluxes(surfaceTemperature=260, topSpectrum=B, emissivity=0.6, reflection=reflection, planck="linear",
                       levelTemperatures=[260.0] * 5)
        worst = np.max(np.abs(f.net) / f.up)
        print(reflection, "net / up at the levels: %.2e" % worst)
        assert np.all(np.abs(f.net) <= 1e-14 * f.up), (reflection, worst)
        assert rel_err(f.up, np.full(5, np.pi * np.sum(B) * settings.BASE_RESOLUTION)) <= TOL


# ---- 5. the Lambertian start term ----------------------------------------------------------------------------------------
def test_lambertian_start_term_is_the_linear_flux_pass(pyrad, lines):
    atm = column(pyrad, rng=RNG)
    x, k, T, depth = model_columns(pyrad, atm)
    Is = orc.planckWavenumber(x, 288)
    _, w = pyrad.fluxAngles(3)
    for lev in (None, LEVELS):
        path = atm.nadirPath(levelTemperatures=True if lev is None else lev)
        got = atm.radiance(path, surfaceTemperature=288, emissivity=0.8, planck="linear", levelTemperatures=lev,
                           transmittance=True)
        down = atm.fluxes(surfaceTemperature=288, planck="linear", levelTemperatures=lev, spectra=True).downSpectrum
        want = walk(x, k, path.layers, path.lengths, path.temperatures, 1, 0.8, Is, down / weight_sum(w))
        check_rays([1], got.radiance, got.transmittance, [want])
        # the diffuse term is there, and it is the linear pass's, not the layer source's
        none = walk(x, k, path.layers, path.lengths, path.temperatures, 1, 0.8, Is, None)
        assert rel_err(got.radiance[0], none[0]) > 1e-9
        other = atm.fluxes(surfaceTemperature=288, spectra=True).downSpectrum
        assert rel_err(down, other) > 1e-6


# ---- 6. other properties -------------------------------------------------------------------------------------------------
def test_rays_are_independent_and_calls_deterministic(pyrad, lines):
    atm = column(pyrad, rng=RNG)
    e = spectral_emissivity(atm[0].xAxis)
    kw = dict(surfaceTemperature=288, transmittance=True, emissivity=e, planck="linear", levelTemperatures=LEVELS)
    other = LEVELS + 3.0
    # ten rays: four nadir views over one sequence and one set of temperatures (a bundle at different cosines), a fifth with
    # other temperatures, mirror paths, a zenith view, two limb rays
    paths = [atm.nadirPath(mu=m, levelTemperatures=LEVELS) for m in (1.0, 0.8, 0.6, 0.4)]
    paths += [atm.nadirPath(mu=0.5, levelTemperatures=other), atm.reflectedPath(levelTemperatures=LEVELS),
              atm.reflectedPath(observerLevel=2, levelTemperatures=LEVELS), atm.zenithPath(levelTemperatures=LEVELS),
              atm.limbPath(2.5e4, levelTemperatures=LEVELS), atm.limbPath(1.7e5, levelTemperatures=LEVELS)]
    assert len(paths) == 10
    a = atm.radiance(paths, **kw)
    I, Tt = a.radiance.copy(), a.transmittance.copy()
    b = atm.radiance(paths, **kw)
    assert np.array_equal(b.radiance, I) and np.array_equal(b.transmittance, Tt)
    rev = atm.radiance(paths[::-1], **kw)
    assert np.array_equal(rev.radiance[::-1], I) and np.array_equal(rev.transmittance[::-1], Tt)
    for r, p in enumerate(paths):
        alone = atm.radiance(p, **kw)
        assert np.array_equal(alone.radiance[0], I[r]) and np.array_equal(alone.transmittance[0], Tt[r]), r
    # same layers, other temperatures: another ray
    assert not np.array_equal(atm.radiance(atm.nadirPath(mu=0.5, levelTemperatures=LEVELS), **kw).radiance[0], I[4])
    f = [atm.fluxes(surfaceTemperature=288, emissivity=e, spectra=True, planck="linear", levelTemperatures=LEVELS)
         for _ in range(2)]
    for name in ("up", "down", "heatingRate", "upSpectrum", "downSpectrum", "upSurfaceSpectrum"):
        assert np.array_equal(getattr(f[0], name), getattr(f[1], name)), name


def test_instrument_rows_are_the_convolved_spectra(pyrad, lines):
    atm = column(pyrad, rng=RNG)
    paths = ten_paths(pyrad, atm, LEVELS) + [atm.reflectedPath(levelTemperatures=LEVELS)]
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    kw = dict(surfaceTemperature=288, transmittance=True, emissivity=0.85, planck="linear", levelTemperatures=LEVELS)
    ch = atm.radiance(paths, instrument=ins, **kw)
    full = atm.radiance(paths, **kw)
    rows = pyrad.convolve(ins, np.concatenate([full.radiance, full.transmittance]), *RNG)
    assert ch.radiance.shape == ch.transmittance.shape == (len(paths), len(ins))
    assert np.array_equal(np.concatenate([ch.radiance, ch.transmittance]), rows)


def test_no_accumulate_after_transmission(pyrad, lines, ctx):
    atm = column(pyrad, rng=RNG)
    atm.transmission(surfaceTemperature=288)
    paths = [atm.nadirPath(levelTemperatures=True), atm.reflectedPath(levelTemperatures=True)]
    ctx.profile_enable(["xsec_accumulate"])
    try:
        ctx.profile_reset()
        atm.radiance(paths, surfaceTemperature=288, emissivity=0.9, planck="linear")
        atm.fluxes(surfaceTemperature=288, planck="linear")
        atm.fluxes(surfaceTemperature=288, emissivity=0.9, planck="linear")
        assert ctx.profile_read()["xsec_accumulate"][0] == 0
        atm[2].changeTemperature(250)                      # one layer due: the counter does count
        atm.fluxes(surfaceTemperature=288, planck="linear")
        assert ctx.profile_read()["xsec_accumulate"][0] >= 1
        ctx.profile_reset()
        atm[1].changeTemperature(255)
        atm.radiance(paths, surfaceTemperature=288, emissivity=0.9, planck="linear")
        assert ctx.profile_read()["xsec_accumulate"][0] >= 1
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


def test_flux_refusals(ctx):
    lib = ctx.lib
    rs = np.random.RandomState(5)
    L, n = 3, 1027
    k = synthetic_k(rs, L, n)
    nv = 2 * (L + 1)
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    level, ut, ds, us = ctx.buffer(nv), ctx.buffer(n), ctx.buffer(n), ctx.buffer(n)
    src, top, em = (ctx.buffer(n).upload(np.full(n, v)) for v in (0.1, 0.02, 0.8))
    level_short, n_short = ctx.buffer(nv - 1), ctx.buffer(n - 1)
    i64, f64 = lambda v: (C.c_int64 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    edges = [290.0, 270.0, 270.0, 240.0, 240.0, 215.0]
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), T_edge=f64(edges),
                depth=f64([1e4, 2e4, 1e4]), lo=600.0, hi=700.0, n=n, I_surface=src.h, surface_T=0.0, I_top=top.h, n_angles=2,
                mu=f64([1.0, 0.5]), weight=f64([1.0, 2.0]), n_bands=1, band_first=i64([0]), band_count=i64([n]),
                emissivity=em.h, emissivity_all=0.5, reflection=0, level_flux=level.h, up_top=ut.h, down_surface=ds.h,
                up_surface=us.h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_flux_linear_dev(*[a[key] for key in good])

    def edge(i, v):
        return dict(T_edge=f64(edges[:i] + [v] + edges[i + 1:]))

    bad = [dict(T_edge=None)]
    # every edge temperature, bottom or top, finite and > 0
    bad += [edge(i, v) for i in (0, 1, 2, 5) for v in (0.0, -250.0, float("nan"), float("inf"), float("-inf"))]
    # what the surface variant refuses
    bad += [dict(abs_coef=None), dict(depth=None), dict(mu=None), dict(weight=None), dict(band_first=None), dict(band_count=None),
            dict(level_flux=None), dict(n_layers=-1), dict(n=-5), dict(n_angles=0), dict(n_bands=0),
            dict(I_surface=None, surface_T=0.0), dict(band_count=i64([n + 1])), dict(band_first=i64([-1])),
            dict(depth=f64([1e4, -1.0, 1e4])), dict(mu=f64([1.0, 0.0])), dict(weight=f64([1.0, float("inf")])),
            dict(level_flux=level_short.h), dict(I_surface=n_short.h), dict(I_top=n_short.h), dict(up_top=n_short.h),
            dict(down_surface=n_short.h), dict(abs_coef=(C.c_void_p * L)(kb[0].h, n_short.h, kb[2].h)),
            dict(reflection=2), dict(reflection=-1), dict(emissivity=None, emissivity_all=-0.01),
            dict(emissivity=None, emissivity_all=1.01), dict(emissivity=None, emissivity_all=float("nan")),
            dict(emissivity=n_short.h), dict(up_surface=n_short.h), dict(weight=f64([1.0, -1.0])),
            dict(weight=f64([1e308, 1e308]))]
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
            assert np.all(b.download() == -7.0)             # nothing was enqueued by a refused call
        assert call() == 0
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        assert call(up_top=None, down_surface=None, up_surface=None, I_top=None, emissivity=None, emissivity_all=1.0,
                    reflection=1) == 0
    finally:
        for b in kb + [level, ut, ds, us, src, top, em, level_short, n_short]:
            b.free()


def test_ray_refusals(ctx):
    lib = ctx.lib
    rs = np.random.RandomState(3)
    L, n, R = 3, 1027, 2
    k = synthetic_k(rs, L, n)
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    rad, trn, src = ctx.buffer(R * n), ctx.buffer(R * n), ctx.buffer(n).upload(np.full(n, 0.1))
    em, down = ctx.buffer(n).upload(np.full(n, 0.8)), ctx.buffer(n).upload(np.full(n, 0.3))
    short, n_short = ctx.buffer(R * n - 1), ctx.buffer(n - 1)
    i32, f64 = lambda v: (C.c_int32 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    nan = float("nan")
    temps = [290.0, 280.0, nan, -5.0, 280.0, 260.0, 260.0, 230.0, 215.0, 240.0, 240.0, 265.0]      # (the marker's pair is ignored)
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), seg_T=f64(temps), lo=600.0, hi=700.0,
                n=n, n_rays=R, ray_first=i32([0, 4, 6]), seg_layer=i32([0, MARKER, 1, 2, 2, 1]),
                seg_length=f64([1e4, 0.0, 2e4, 1e4, 3e4, 1e4]), source_kind=i32([1, 0]), I_source=src.h, source_T=0.0,
                emissivity=em.h, emissivity_all=0.5, surface_down=down.h, surface_down_norm=np.pi, radiance=rad.h,
                transmittance=trn.h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_ray_radiance_linear_dev(*[a[key] for key in good])

    def temp(i, v):
        return dict(seg_T=f64(temps[:i] + [v] + temps[i + 1:]))

    bad = [dict(seg_T=None)]
    # every segment temperature, entry or exit, finite and > 0 - except a marker's
    bad += [temp(i, v) for i in (0, 1, 4, 11) for v in (0.0, -250.0, nan, float("inf"), float("-inf"))]
    # what the surface variant refuses
    bad += [dict(abs_coef=None), dict(ray_first=None), dict(seg_layer=None), dict(seg_length=None), dict(source_kind=None),
            dict(radiance=None), dict(n_layers=0), dict(n=0), dict(n_rays=0), dict(ray_first=i32([1, 4, 6])),
            dict(ray_first=i32([0, 4, 3])), dict(seg_layer=i32([0, MARKER, 3, 2, 2, 1])), dict(seg_layer=i32([0, -2, 1, 2, 2, 1])),
            dict(seg_length=f64([1e4, 0.0, -1.0, 1e4, 3e4, 1e4])), dict(seg_length=f64([1e4, 0.0, nan, 1e4, 3e4, 1e4])),
            dict(source_kind=i32([2, 0])), dict(seg_length=f64([1e4, 1.0, 2e4, 1e4, 3e4, 1e4])),
            dict(source_kind=i32([0, 0]), I_source=None, source_T=0.0),
            dict(emissivity=None, emissivity_all=-0.01), dict(emissivity=None, emissivity_all=1.01),
            dict(emissivity=None, emissivity_all=nan), dict(emissivity=n_short.h), dict(surface_down=n_short.h),
            dict(surface_down_norm=0.0), dict(surface_down_norm=float("inf")), dict(radiance=short.h),
            dict(transmittance=short.h), dict(I_source=n_short.h), dict(abs_coef=(C.c_void_p * L)(kb[0].h, n_short.h, kb[2].h))]
    try:
        assert call() == 0
        want_I, want_T = rad.download(), trn.download()
        rad.upload(np.full(R * n, -7.0))
        trn.upload(np.full(R * n, -7.0))
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
        assert np.all(rad.download() == -7.0) and np.all(trn.download() == -7.0)
        for v in (0.0, nan, float("inf")):                  # a marker's pair may hold anything
            assert call(**temp(2, v)) == 0 and call(**temp(3, v)) == 0
        assert call() == 0
        assert np.array_equal(rad.download(), want_I) and np.array_equal(trn.download(), want_T)
        x = np.linspace(600.0, 700.0, n)
        pairs = list(zip(temps[0::2], temps[1::2]))
        want = walk(x, k, [0, MARKER, 1, 2], [1e4, 0.0, 2e4, 1e4], pairs[:4], 1, 0.8, np.full(n, 0.1), np.full(n, 0.3) / np.pi)
        assert rel_err(want_I[:n], want[0]) <= TOL and rel_err(want_T[:n], want[1], floor=1e-30) <= TOL
    finally:
        for b in kb + [rad, trn, src, em, down, short, n_short]:
            b.free()
