"""GPU: the reflecting surface - Atmosphere.fluxes and radiance with an emissivity (lbl_column_flux_surface_dev,
lbl_ray_radiance_surface_dev, kernels K5g) - for its identities with the black surface and between its two kernels, against
a NumPy restatement of its semantics (written out below), in its physical limits, and for independence of the rays,
determinism, laziness and the C ABI's refusals.  Column, rays and synthetic coefficients are tests/test_gpu_paths.py's."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from oracle import pyrad_oracle as orc
from test_gpu_paths import LAYERS, RNG, TOL, band_of_rays, column, ctx, lines, nine_paths, pyrad, synthetic_k  # noqa: F401

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
MARKER = -1           # the segment layer of a surface marker
# Tolerances: the issue's, which are tests/test_gpu_flux.py's for fluxes (spectra 1e-13 with a floor of 1e-300 on downward
# ones, band fluxes 1e-12, heating rates 1e-10) and tests/test_gpu_paths.py's for rays (TOL = 1e-13; radiance floor 1e-300 for
# rays from space, transmittance floor 1e-30).
TOL_BAND, TOL_HEAT = 1e-12, 1e-10
# The physics identities that hold to a few roundings (Lambertian conservation: three roundings and the angle sum of equal
# radiances; a transparent column: one product): the issue's 1e-14.
TOL_EXACT = 1e-14


# ---- the semantics, restated in NumPy ----------------------------------------------------------------------------------
def leaving(e, Is, R):
    """what leaves a surface of emissivity e that emits Is and reflects R"""
    return e * Is + (1 - e) * R


def walk(x, k, T, layers, lengths, kind, e=1.0, Is=None, Rd=None):
    """(radiance, transmittance) of one ray, tests/test_gpu_paths.py's walk with a surface: k[l] the absorption coefficient
    of layer l on the grid x, T[l] its temperature; kind 1: the ray starts at the surface with e Is + (1 - e) Rd (Rd None: 0),
    kind 0: in cold space; a layer of MARKER is where the ray meets the surface"""
    I = np.zeros(x.size) if kind == 0 else leaving(e, Is, 0.0 if Rd is None else Rd) * np.ones(x.size)
    Tt = np.ones(x.size)
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        for l, s in zip(layers, lengths):
            if l == MARKER:
                I = leaving(e, Is, I)
                Tt = Tt * (1 - e)
                continue
            t = np.exp(-(k[l] * s))
            B = orc.planckWavenumber(x, T[l])
            I = t * I + (1 - t) * B
            Tt = Tt * t
    return I, Tt


def weight_sum(weight):
    total = 0.0
    for w in weight:
        total += float(w)
    return total


def flux_walk(x, k, T, depth, mu, weight, Is, e, reflection, top=None, idx=None):
    """lbl_column_flux_surface_dev: (up, down) sums [band, level] over the bands idx = [(first, end)], and the spectral
    F_up at the top, F_down at the surface and F_up at the surface"""
    n, nl = x.size, len(k)
    idx = idx or [(0, n)]

    def level(I):
        F = sum(w * Ik for w, Ik in zip(weight, I))                   # spectral flux sum_k W_k I_k, angle 0 first
        return F, [np.sum(np.nan_to_num(F[a:b])) for a, b in idx]

    def step(l, I):
        B = orc.planckWavenumber(x, T[l])
        for i, m in enumerate(mu):
            t = np.exp(-(k[l] * depth[l]) * (1.0 / m))
            I[i] = t * I[i] + (1 - t) * B

    up, down = np.zeros((len(idx), nl + 1)), np.zeros((len(idx), nl + 1))
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        I = [(np.zeros(n) if top is None else np.array(top, dtype=np.float64)) for _ in mu]
        F, down[:, nl] = level(I)
        for l in range(nl - 1, -1, -1):
            step(l, I)
            F, down[:, l] = level(I)
        sd = F
        R = [F / weight_sum(weight) for _ in mu] if reflection == "lambertian" else I
        I = [leaving(e, Is, Rk) for Rk in R]
        s0, up[:, 0] = level(I)
        F = s0
        for l in range(nl):
            step(l, I)
            F, up[:, l + 1] = level(I)
    return up, down, F, sd, s0


def model_columns(pyrad, atm):
    return (np.asarray(atm[0].xAxis), [np.array(pyrad.getAbsCoef(L)) for L in atm], [L.T for L in atm],
            [L.depth for L in atm])


def spectral_emissivity(x):
    """between 0.55 and 1 over the range, both ends reached"""
    return 0.775 + 0.225 * np.cos(np.linspace(0.0, 9.0 * np.pi, x.size))


def check_rays(kinds, got_I, got_T, want, tol_I=TOL):
    worst = []
    for r, kind in enumerate(kinds):
        eI = rel_err(got_I[r], want[r][0], floor=1e-300 if kind == 0 else 0.0)
        eT = rel_err(got_T[r], want[r][1], floor=1e-30)
        print("ray %d: radiance %.2e transmittance %.2e" % (r, eI, eT))
        worst.append((r, eI, eT))
    for r, eI, eT in worst:
        assert eI <= tol_I and eT <= TOL, (r, eI, eT)


# ---- 1. identity with the black surface ----------------------------------------------------------------------------------
@pytest.mark.parametrize("reflection", ["lambertian", "specular"])
def test_emissivity_one_is_the_black_surface_fluxes(pyrad, lines, reflection):
    atm = column(pyrad, rng=(600, 610.07))              # an odd number of points: a tail
    x = atm[0].xAxis
    assert x.size % 4 != 0
    edges = [0, 101, 502, 503, 807, x.size]             # bands that start and end off the groups of 4, one of a single point
    bands = [(x[a], x[b] if b < x.size else np.inf) for a, b in zip(edges[:-1], edges[1:])]
    top = 0.3 * atm[0].planck(250)
    for angles in (1, 3, 8, [(1.0, 1.0), (0.3, 2.0)]):
        for kw in (dict(surfaceTemperature=288), dict(surfaceSpectrum=atm[0].planck(300), topSpectrum=top),
                   dict(surfaceTemperature=288, bands=bands)):
            black = atm.fluxes(angles=angles, spectra=True, **kw)
            for e in (1.0, 1, np.ones(x.size)):
                got = atm.fluxes(angles=angles, spectra=True, emissivity=e, reflection=reflection, **kw)
                for name in ("up", "down", "net", "heatingRate", "upSpectrum", "downSpectrum"):
                    assert np.array_equal(getattr(got, name), getattr(black, name)), (angles, sorted(kw), name)
                assert black.upSurfaceSpectrum is None and got.upSurfaceSpectrum.shape == x.shape


def test_emissivity_one_is_the_black_surface_radiance(pyrad, lines):
    atm = column(pyrad)
    paths = nine_paths(pyrad, atm)
    assert len(paths) == 10
    for kw in (dict(surfaceTemperature=288), dict(surfaceSpectrum=atm[0].planck(300))):
        black = atm.radiance(paths, transmittance=True, **kw)
        for extra in (dict(), dict(reflection="specular"), dict(angles=1)):
            got = atm.radiance(paths, transmittance=True, emissivity=1.0, **extra, **kw)
            assert np.array_equal(got.radiance, black.radiance) and np.array_equal(got.transmittance, black.transmittance)
        got = atm.radiance(paths, emissivity=np.ones(atm[0].xAxis.size), **kw)
        assert np.array_equal(got.radiance, black.radiance)


# ---- 2. identity between the two kernels ---------------------------------------------------------------------------------
def test_reflected_path_is_the_specular_flux_of_one_vertical_angle(pyrad, lines):
    atm = column(pyrad, rng=(600, 610.07))
    x = atm[0].xAxis
    for e in (0.6, spectral_emissivity(x)):
        for kw in (dict(surfaceTemperature=288), dict(surfaceSpectrum=atm[0].planck(300))):
            ray = atm.radiance(atm.reflectedPath(), emissivity=e, reflection="specular", **kw)
            flux = atm.fluxes(emissivity=e, reflection="specular", angles=[(1.0, 1.0)], spectra=True, **kw)
            assert np.array_equal(ray.radiance[0], flux.upSpectrum)
            # ... and where the observer stands on the surface: F_up at level 0
            ray = atm.radiance(atm.reflectedPath(observerLevel=0), emissivity=e, reflection="specular", **kw)
            assert np.array_equal(ray.radiance[0], flux.upSurfaceSpectrum)


# ---- 3. against NumPy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angles", [1, 3, 8])
def test_fluxes_against_numpy(pyrad, lines, angles):
    from pyrad_amd import settings
    atm = column(pyrad)
    x, k, T, depth = model_columns(pyrad, atm)
    mu, w = pyrad.fluxAngles(angles)
    res = settings.BASE_RESOLUTION
    top = 0.3 * np.array(atm[0].planck(250))
    Is = orc.planckWavenumber(x, 288)
    heat = lambda net: pyrad.heatingRates(net, [L.P for L in atm], T, depth)
    for reflection in ("lambertian", "specular"):
        for e in (0.9, spectral_emissivity(x)):
            for t in (None, top):
                f = atm.fluxes(surfaceTemperature=288, topSpectrum=t, angles=angles, spectra=True, emissivity=e,
                               reflection=reflection)
                fu, fd, su, sd, s0 = flux_walk(x, k, T, depth, mu, w, Is, e, reflection, top=t)
                fu, fd = fu[0] * res, fd[0] * res
                errs = (rel_err(f.up, fu), rel_err(f.down, fd, floor=1e-300), rel_err(f.net, fu - fd),
                        rel_err(f.heatingRate, heat(fu - fd)), rel_err(f.upSpectrum, su),
                        rel_err(f.downSpectrum, sd, floor=1e-300), rel_err(f.upSurfaceSpectrum, s0))
                print(reflection, np.ndim(e), t is not None, " ".join("%.2e" % v for v in errs))
                assert f.up.shape == f.down.shape == (len(atm) + 1,)
                assert errs[0] <= TOL_BAND and errs[1] <= TOL_BAND and errs[2] <= TOL_BAND
                assert errs[3] <= TOL_HEAT
                assert errs[4] <= 1e-13 and errs[5] <= 1e-13 and errs[6] <= 1e-13
    # an emissivity table is the interpolated array
    nu, val = [598.0, 603.0, 604.5, 612.0], [0.95, 0.6, 0.8, 0.99]
    a = atm.fluxes(surfaceTemperature=288, angles=angles, emissivity=(nu, val), spectra=True)
    b = atm.fluxes(surfaceTemperature=288, angles=angles, emissivity=np.interp(x, nu, val), spectra=True)
    assert np.array_equal(a.up, b.up) and np.array_equal(a.upSpectrum, b.upSpectrum)


def test_radiance_against_numpy(pyrad, lines):
    atm = column(pyrad)
    x, k, T, depth = model_columns(pyrad, atm)
    paths = [atm.nadirPath(), atm.nadirPath(mu=0.4), atm.nadirPath(observerLevel=2), atm.reflectedPath(),
             atm.reflectedPath(mu=0.4), atm.reflectedPath(observerLevel=2), atm.reflectedPath(observerLevel=0),
             atm.zenithPath(), pyrad.Path([], [], source="surface"), pyrad.Path([], [], source="space", bounce=0),
             pyrad.Path([1, 0, 0, 2], [3e4, 2e4, 1e4, 7e3], source="surface", bounce=2)]
    Is = orc.planckWavenumber(x, 288)
    mu, w = pyrad.fluxAngles(3)
    for e in (0.85, spectral_emissivity(x)):
        down = flux_walk(x, k, T, depth, mu, w, Is, 1.0, "specular")[3]          # F_down at the surface under cold space
        for reflection, Rd in (("lambertian", down / weight_sum(w)), ("specular", None)):
            got = atm.radiance(paths, surfaceTemperature=288, transmittance=True, emissivity=e, reflection=reflection)
            want = [walk(x, k, T, *p._segments(), 1 if p.source == "surface" else 0, e, Is, Rd) for p in paths]
            check_rays([1 if p.source == "surface" else 0 for p in paths], got.radiance, got.transmittance, want)
    # the rows go to the instrument unchanged
    ins = pyrad.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    ch = atm.radiance(paths, surfaceTemperature=288, instrument=ins, transmittance=True, emissivity=0.85)
    full = atm.radiance(paths, surfaceTemperature=288, transmittance=True, emissivity=0.85)
    rows = pyrad.convolve(ins, np.concatenate([full.radiance, full.transmittance]), *RNG)
    assert np.array_equal(np.concatenate([ch.radiance, ch.transmittance]), rows)


def with_marker(ray, where):
    """the ray (layers, lengths, kind) with surface markers before the segments `where` (len: behind the last)"""
    lay, lens = list(ray[0]), list(ray[1])
    for i in sorted(where, reverse=True):
        lay.insert(i, MARKER)
        lens.insert(i, 0.0)
    return lay, lens, ray[2]


def marked_rays(rs, L):
    """band_of_rays' rays, each with a marker at the front, at the back, in the middle and twice; a marker-only ray from
    each source, two markers alone; a bundle of four rays over one marked sequence and one left over"""
    rays = []
    for ray in band_of_rays(rs, L):
        ns = len(ray[0])
        rays += [with_marker(ray, w) for w in ([0], [ns], [ns // 2], [ns // 2, ns // 2], [0, ns])]
    rays += [([MARKER], [0.0], 0), ([MARKER], [0.0], 1), ([MARKER, MARKER], [0.0, 0.0], 0)]
    seq = [2, 1, 0, MARKER, 0, 1]
    rays += [(seq, list(rs.uniform(0.5e4, 2e4, 3)) + [0.0] + list(rs.uniform(0.5e4, 2e4, 2)), i % 2) for i in range(5)]
    return rays


def run_raw_rays(ctx, k, T, rays, e, lo=600.0, hi=700.0, I_source=None, source_T=0.0, down=None, norm=0.0):
    """rays: [(layers, lengths, kind)] -> (radiance, transmittance), R x n each"""
    L, n = k.shape
    bufs = [ctx.buffer(n).upload(k[l]) for l in range(L)]
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
        ctx.ray_radiance_surface_dev(bufs[:L], T, lo, hi, n, np.cumsum([0] + [len(r[0]) for r in rays]),
                                     [l for r in rays for l in r[0]], [s for r in rays for s in r[1]], [r[2] for r in rays],
                                     rad, eb if eb is not None else e, I_source=src, source_T=source_T, surface_down=db,
                                     surface_down_norm=norm, transmittance=trn)
        return rad.download().reshape(len(rays), n), trn.download().reshape(len(rays), n)
    finally:
        for b in bufs:
            b.free()


def check_raw_rays(ctx, k, T, rays, e, lo=600.0, hi=700.0, I_source=None, source_T=0.0, down=None, norm=0.0):
    n = k.shape[1]
    x = np.linspace(lo, hi, n)
    got_I, got_T = run_raw_rays(ctx, k, T, rays, e, lo, hi, I_source, source_T, down, norm)
    Is = I_source if I_source is not None else orc.planckWavenumber(x, source_T)
    Rd = down / norm if down is not None else None
    want = [walk(x, k, T, r[0], r[1], r[2], e, Is, Rd) for r in rays]
    check_rays([r[2] for r in rays], got_I, got_T, want)
    return got_I, got_T


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 5003])
def test_raw_rays_sizes(ctx, n):
    rs = np.random.RandomState(200 + n)
    L = 3
    k = synthetic_k(rs, L, n)
    T = [288.0, 250.0, 215.0]
    rays = marked_rays(rs, L)
    e = rs.uniform(0.5, 1.0, n)
    e[::7] = 1.0
    e[3::11] = 0.0
    check_raw_rays(ctx, k, T, rays, 0.8, source_T=295.0)
    check_raw_rays(ctx, k, T, rays, e, I_source=rs.uniform(0.0, 0.2, n), down=rs.uniform(0.0, 0.5, n), norm=2.75)
    check_raw_rays(ctx, k, T, rays, e, source_T=295.0, down=rs.uniform(0.0, 0.5, n), norm=np.pi)


def test_raw_rays_128_layers_down_and_up(ctx):
    rs = np.random.RandomState(17)
    L, n = 128, 1027
    k = synthetic_k(rs, L, n, tau_lo=-6.0, tau_hi=-5.0, huge=0.002)
    T = list(np.linspace(290.0, 180.0, L))
    d = list(rs.uniform(0.5e4, 1e4, L))
    seq = list(range(L - 1, -1, -1)) + [MARKER] + list(range(L))
    lens = [d[l] for l in range(L - 1, -1, -1)] + [0.0] + d
    assert len(seq) == 257
    check_raw_rays(ctx, k, T, [(seq, lens, 0), (seq, lens, 1)], rs.uniform(0.3, 1.0, n), source_T=300.0)


def run_raw_flux(ctx, k, T, depth, mu, w, e, reflection, lo=600.0, hi=700.0, source_T=0.0, I_source=None, top=None, bands=None):
    """lbl_column_flux_surface_dev on uploaded coefficients: (level sums [band, 2, level], up_top, down_surface, up_surface)"""
    L, n = k.shape
    first, count = ([0], [n]) if bands is None else ([a for a, _ in bands], [b - a for a, b in bands])
    nb = len(first)
    bufs = [ctx.buffer(n).upload(k[l]) for l in range(L)]
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
        ctx.column_flux_surface_dev(bufs[:L], T, depth, lo, hi, n, mu, w, first, count, level, eb if eb is not None else e,
                                    reflection=("lambertian", "specular").index(reflection), I_surface=src,
                                    surface_T=source_T, I_top=tb, up_top=ut, down_surface=ds, up_surface=us)
        return level.download(nb * 2 * (L + 1)).reshape(nb, 2, L + 1), ut.download(n), ds.download(n), us.download(n)
    finally:
        for b in bufs:
            b.free()


def check_raw_flux(ctx, k, T, depth, mu, w, e, reflection, lo=600.0, hi=700.0, source_T=0.0, I_source=None, top=None,
                   bands=None):
    n = k.shape[1]
    x = np.linspace(lo, hi, n)
    sums, ut, ds, us = run_raw_flux(ctx, k, T, depth, mu, w, e, reflection, lo, hi, source_T, I_source, top, bands)
    Is = I_source if I_source is not None else orc.planckWavenumber(x, source_T)
    fu, fd, su, sd, s0 = flux_walk(x, k, T, depth, mu, w, Is, e, reflection, top=top, idx=bands)
    if bands is not None:                        # (points outside every band keep 0 in the spectra)
        inside = np.zeros(n, dtype=bool)
        for a, b in bands:
            inside[a:b] = True
        su, sd, s0 = (np.where(inside, v, 0.0) for v in (su, sd, s0))
    errs = (rel_err(sums[:, 0], fu), rel_err(sums[:, 1], fd, floor=1e-300), rel_err(ut, su),
            rel_err(ds, sd, floor=1e-300), rel_err(us, s0))
    print(reflection, k.shape, len(mu), " ".join("%.2e" % v for v in errs))
    assert errs[0] <= TOL_BAND and errs[1] <= TOL_BAND
    assert errs[2] <= 1e-13 and errs[3] <= 1e-13 and errs[4] <= 1e-13


def test_raw_flux_one_layer_and_none(ctx, pyrad):
    rs = np.random.RandomState(31)
    n = 1027
    mu, w = pyrad.fluxAngles(3)
    e = rs.uniform(0.4, 1.0, n)
    for L in (1, 0):
        k = synthetic_k(rs, L, n)
        for reflection in ("lambertian", "specular"):
            check_raw_flux(ctx, k, [270.0] * L, [1e4] * L, mu, w, e, reflection, source_T=295.0, top=rs.uniform(0.0, 0.2, n),
                           bands=[(1, 515), (515, 516), (518, n)])
            check_raw_flux(ctx, k, [270.0] * L, [1e4] * L, mu, w, 0.7, reflection, I_source=rs.uniform(0.0, 0.2, n))


def test_raw_flux_128_layers_eight_angles(ctx, pyrad):
    rs = np.random.RandomState(37)
    L, n = 128, 1027
    k = synthetic_k(rs, L, n, tau_lo=-6.0, tau_hi=-5.0, huge=0.002)
    T = list(np.linspace(290.0, 180.0, L))
    depth = list(rs.uniform(0.5e4, 1e4, L))
    mu, w = pyrad.fluxAngles(8)
    e = rs.uniform(0.3, 1.0, n)
    for reflection in ("lambertian", "specular"):
        check_raw_flux(ctx, k, T, depth, mu, w, e, reflection, source_T=300.0, top=rs.uniform(0.0, 0.1, n))


def test_raw_flux_beyond_the_grid_stride_bound(ctx, pyrad):
    """1,024 workgroups of 1,024 points, then the grid-stride loop's second round, and a tail of 1 point (n = 4 q + 1)"""
    rs = np.random.RandomState(41)
    n = 1048576 + 1029
    k = synthetic_k(rs, 1, n)
    mu, w = pyrad.fluxAngles(3)
    check_raw_flux(ctx, k, [255.0], [1e4], mu, w, rs.uniform(0.3, 1.0, n), "lambertian", source_T=290.0,
                   top=rs.uniform(0.0, 0.1, n))


# ---- 4. physics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflection", ["lambertian", "specular"])
def test_isothermal_cavity_stays_planckian(pyrad, lines, reflection):
    from pyrad_amd import settings
    atm = column(pyrad, layers=tuple((d, 260, P) for d, _, P in LAYERS))
    x = atm[0].xAxis
    B = orc.planckWavenumber(x, 260)
    for angles in (3, [(1.0, 1.0), (0.3, 2.0), (0.75, 0.5)]):
        _, w = pyrad.fluxAngles(angles)
        want = np.full(len(atm) + 1, weight_sum(w) * np.sum(B) * settings.BASE_RESOLUTION)
        for e in (0.0, 0.37, 1.0, spectral_emissivity(x)):
            f = atm.fluxes(surfaceTemperature=260, topSpectrum=B, angles=angles, emissivity=e, reflection=reflection)
            print(reflection, np.ndim(e), rel_err(f.up, want), rel_err(f.down, want), np.max(np.abs(f.net)) / want[0])
            assert rel_err(f.up, want) <= TOL and rel_err(f.down, want) <= TOL
            assert np.max(np.abs(f.net)) <= TOL * want[0]


@pytest.mark.parametrize("reflection", ["lambertian", "specular"])
def test_perfect_mirror_under_a_transparent_column(pyrad, lines, reflection):
    atm = column(pyrad, co2=0, h2o=0)
    top = 0.3 * np.array(atm[0].planck(250))
    f = atm.fluxes(surfaceTemperature=288, topSpectrum=top, emissivity=0.0, reflection=reflection, spectra=True)
    assert np.all(f.down == f.down[-1]) and f.down[-1] > 0
    assert rel_err(f.up, f.down) <= TOL
    assert rel_err(f.upSurfaceSpectrum, f.downSpectrum) <= TOL_EXACT
    if reflection == "specular":                         # each angle gets back its own radiance
        assert np.array_equal(f.up, f.down) and np.array_equal(f.upSurfaceSpectrum, f.downSpectrum)


def test_lambertian_surface_conserves_energy(pyrad, lines):
    atm = column(pyrad)
    x = atm[0].xAxis
    Is = orc.planckWavenumber(x, 288)
    top = 0.3 * np.array(atm[0].planck(250))
    for angles in (1, 3, 8, [(1.0, 1.0), (0.3, 2.0), (0.75, 0.5)]):
        _, w = pyrad.fluxAngles(angles)
        for e in (0.0, 0.7, spectral_emissivity(x)):
            f = atm.fluxes(surfaceTemperature=288, topSpectrum=top, angles=angles, emissivity=e, spectra=True)
            want = e * weight_sum(w) * Is + (1 - e) * f.downSpectrum
            print(np.ndim(e), rel_err(f.upSurfaceSpectrum, want))
            assert rel_err(f.upSurfaceSpectrum, want) <= TOL_EXACT


def test_transparent_column_radiance(pyrad, lines):
    atm = column(pyrad, co2=0, h2o=0)
    x = atm[0].xAxis
    B = orc.planckWavenumber(x, 288)
    for e in (0.0, 0.65, spectral_emissivity(x)):
        for reflection in ("lambertian", "specular"):
            got = atm.radiance([atm.nadirPath(), atm.reflectedPath()], surfaceTemperature=288, emissivity=e,
                               reflection=reflection, transmittance=True)
            for r in range(2):
                assert rel_err(got.radiance[r], e * B) <= TOL_EXACT, (reflection, r)
            assert np.all(got.transmittance[0] == 1.0) and np.array_equal(got.transmittance[1], 1 - e * np.ones(x.size))


# ---- 5. independence and determinism -------------------------------------------------------------------------------------
def test_rays_are_independent_and_calls_deterministic(pyrad, lines):
    atm = column(pyrad, rng=(600, 610.07))
    e = spectral_emissivity(atm[0].xAxis)
    kw = dict(surfaceTemperature=288, transmittance=True, emissivity=e)
    paths = [atm.nadirPath(), atm.reflectedPath(), atm.reflectedPath(observerLevel=2), atm.zenithPath(), atm.limbPath(2.5e4),
             pyrad.Path([1, 0, 0, 2], [3e4, 2e4, 1e4, 7e3], source="surface", bounce=2)]
    a = atm.radiance(paths, **kw)
    I, Tt = a.radiance.copy(), a.transmittance.copy()
    b = atm.radiance(paths, **kw)
    assert np.array_equal(b.radiance, I) and np.array_equal(b.transmittance, Tt)
    rev = atm.radiance(paths[::-1], **kw)
    assert np.array_equal(rev.radiance[::-1], I) and np.array_equal(rev.transmittance[::-1], Tt)
    for r, p in enumerate(paths):
        alone = atm.radiance(p, **kw)
        assert np.array_equal(alone.radiance[0], I[r]) and np.array_equal(alone.transmittance[0], Tt[r]), r
    # four and five rays over one marked sequence travel as a bundle, in either position of it: the bits of each one alone
    mus = [1.0, 0.8, 0.6, 0.4, 0.25]
    band = atm.radiance([atm.reflectedPath(mu=m) for m in mus], **kw)
    shifted = atm.radiance([atm.reflectedPath(mu=m) for m in mus[1:] + mus[:1]], **kw)
    for r, m in enumerate(mus):
        alone = atm.radiance(atm.reflectedPath(mu=m), **kw)
        assert np.array_equal(alone.radiance[0], band.radiance[r]), m
        assert np.array_equal(alone.transmittance[0], band.transmittance[r]), m
        assert np.array_equal(alone.radiance[0], shifted.radiance[(r - 1) % 5]), m
    f = [atm.fluxes(surfaceTemperature=288, emissivity=e, spectra=True) for _ in range(2)]
    for name in ("up", "down", "upSpectrum", "downSpectrum", "upSurfaceSpectrum"):
        assert np.array_equal(getattr(f[0], name), getattr(f[1], name)), name


# ---- 6. refusals of the C entry points -----------------------------------------------------------------------------------
def test_ray_refusals(ctx):
    lib = ctx.lib
    rs = np.random.RandomState(3)
    L, n, R = 3, 1027, 2
    k = synthetic_k(rs, L, n)
    T = [288.0, 250.0, 215.0]
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    rad, trn, src = ctx.buffer(R * n), ctx.buffer(R * n), ctx.buffer(n).upload(np.full(n, 0.1))
    em, down = ctx.buffer(n).upload(np.full(n, 0.8)), ctx.buffer(n).upload(np.full(n, 0.3))
    short, n_short = ctx.buffer(R * n - 1), ctx.buffer(n - 1)
    i32, f64 = lambda v: (C.c_int32 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), T=f64(T), lo=600.0, hi=700.0, n=n,
                n_rays=R, ray_first=i32([0, 4, 6]), seg_layer=i32([0, MARKER, 1, 2, 2, 1]),
                seg_length=f64([1e4, 0.0, 2e4, 1e4, 3e4, 1e4]), source_kind=i32([1, 0]), I_source=src.h, source_T=0.0,
                emissivity=em.h, emissivity_all=0.5, surface_down=down.h, surface_down_norm=np.pi, radiance=rad.h,
                transmittance=trn.h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_ray_radiance_surface_dev(*[a[key] for key in good])

    bad = [dict(abs_coef=None), dict(T=None), dict(ray_first=None), dict(seg_layer=None), dict(seg_length=None),
           dict(source_kind=None), dict(radiance=None), dict(n_layers=0), dict(n=0), dict(n_rays=0),
           dict(ray_first=i32([1, 4, 6])), dict(ray_first=i32([0, 4, 3])),
           dict(seg_layer=i32([0, MARKER, 3, 2, 2, 1])), dict(seg_layer=i32([0, -2, 1, 2, 2, 1])),
           dict(seg_length=f64([1e4, 0.0, -1.0, 1e4, 3e4, 1e4])), dict(seg_length=f64([1e4, 0.0, float("nan"), 1e4, 3e4, 1e4])),
           dict(T=f64([288.0, 0.0, 215.0])), dict(source_kind=i32([2, 0])),
           # a marker with a length; a ray with a marker (the second, from space) and no surface source
           dict(seg_length=f64([1e4, 1.0, 2e4, 1e4, 3e4, 1e4])), dict(seg_length=f64([1e4, 1e-300, 2e4, 1e4, 3e4, 1e4])),
           dict(source_kind=i32([0, 0]), I_source=None, source_T=0.0),
           dict(source_kind=i32([0, 0]), I_source=None, source_T=0.0, seg_layer=i32([0, 1, 1, 2, 2, MARKER]),
                seg_length=f64([1e4, 1e4, 2e4, 1e4, 3e4, 0.0])),
           dict(emissivity=None, emissivity_all=-0.01), dict(emissivity=None, emissivity_all=1.01),
           dict(emissivity=None, emissivity_all=float("nan")), dict(emissivity=n_short.h),
           dict(surface_down=n_short.h), dict(surface_down_norm=0.0), dict(surface_down_norm=-1.0),
           dict(surface_down_norm=float("inf")), dict(surface_down_norm=float("nan")),
           dict(radiance=short.h), dict(transmittance=short.h), dict(I_source=n_short.h),
           dict(abs_coef=(C.c_void_p * L)(kb[0].h, n_short.h, kb[2].h))]
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
        # the black-surface entry points go on refusing the marker
        for name, tail in (("lbl_ray_radiance_dev", (rad.h, trn.h)), ("lbl_ray_jacobian_dev", (0, None, None, rad.h, trn.h))):
            lead = [good[key] for key in list(good)[:list(good).index("emissivity")]]
            assert getattr(lib, name)(*lead, *tail) == BAD_ARG, name
        # nothing was enqueued by a refused call: the outputs still hold the marker value, and the context goes on computing
        assert np.all(rad.download() == -7.0) and np.all(trn.download() == -7.0)
        # a norm is not looked at without surface_down, nor emissivity_all beside a buffer; rays from space without a
        # marker need no surface source
        assert call(surface_down=None, surface_down_norm=float("nan"), emissivity_all=7.0) == 0
        assert call(source_kind=i32([0, 0]), I_source=None, seg_layer=i32([0, 1, 1, 2, 2, 1]),
                    seg_length=f64([1e4, 1e4, 2e4, 1e4, 3e4, 1e4])) == 0
        assert call() == 0
        assert np.array_equal(rad.download(), want_I) and np.array_equal(trn.download(), want_T)
        x = np.linspace(600.0, 700.0, n)
        want = walk(x, k, T, [0, MARKER, 1, 2], [1e4, 0.0, 2e4, 1e4], 1, 0.8, np.full(n, 0.1), np.full(n, 0.3) / np.pi)
        assert rel_err(want_I[:n], want[0]) <= TOL and rel_err(want_T[:n], want[1], floor=1e-30) <= TOL
    finally:
        for b in kb + [rad, trn, src, em, down, short, n_short]:
            b.free()


def test_flux_refusals(ctx):
    from pyrad_amd import _native
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
    nmax = _native.limit("flux_angles")
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=(C.c_void_p * L)(*[b.h for b in kb]), T=f64([288.0, 250.0, 215.0]),
                depth=f64([1e4, 2e4, 1e4]), lo=600.0, hi=700.0, n=n, I_surface=src.h, surface_T=0.0, I_top=top.h, n_angles=2,
                mu=f64([1.0, 0.5]), weight=f64([1.0, 2.0]), n_bands=1, band_first=i64([0]), band_count=i64([n]),
                emissivity=em.h, emissivity_all=0.5, reflection=0, level_flux=level.h, up_top=ut.h, down_surface=ds.h,
                up_surface=us.h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_flux_surface_dev(*[a[key] for key in good])

    bad = [dict(abs_coef=None), dict(T=None), dict(depth=None), dict(mu=None), dict(weight=None), dict(band_first=None),
           dict(band_count=None), dict(level_flux=None), dict(n_layers=-1), dict(n_layers=_native.limit("layers_per_column") + 1),
           dict(n=-5), dict(n_angles=0), dict(n_angles=nmax + 1, mu=f64([0.5] * (nmax + 1)), weight=f64([1.0] * (nmax + 1))),
           dict(n_bands=0), dict(n_bands=_native.limit("flux_bands") + 1), dict(I_surface=None, surface_T=0.0),
           dict(band_count=i64([n + 1])), dict(band_first=i64([-1])), dict(band_count=i64([0])),
           dict(T=f64([288.0, 0.0, 215.0])), dict(depth=f64([1e4, -1.0, 1e4])), dict(mu=f64([1.0, 0.0])),
           dict(mu=f64([1.0, 1.5])), dict(weight=f64([1.0, float("inf")])),
           dict(level_flux=level_short.h), dict(I_surface=n_short.h), dict(I_top=n_short.h), dict(up_top=n_short.h),
           dict(down_surface=n_short.h), dict(abs_coef=(C.c_void_p * L)(kb[0].h, n_short.h, kb[2].h)),
           # the surface's own
           dict(reflection=2), dict(reflection=-1),
           dict(emissivity=None, emissivity_all=-0.01), dict(emissivity=None, emissivity_all=1.01),
           dict(emissivity=None, emissivity_all=float("nan")), dict(emissivity=n_short.h), dict(up_surface=n_short.h),
           dict(weight=f64([1.0, -1.0])), dict(weight=f64([1.0, -2.0])), dict(weight=f64([1e308, 1e308])),
           dict(weight=f64([1.0, float("nan")]))]
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
        assert call(up_top=None, down_surface=None, up_surface=None, I_top=None, emissivity=None, reflection=1) == 0
    finally:
        for b in kb + [level, ut, ds, us, src, top, em, level_short, n_short]:
            b.free()


# ---- 7. laziness -----------------------------------------------------------------------------------------------------------
def test_no_accumulate_after_transmission(pyrad, lines, ctx):
    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    ctx.profile_enable(["xsec_accumulate"])
    try:
        ctx.profile_reset()
        atm.radiance([atm.nadirPath(), atm.reflectedPath()], surfaceTemperature=288, emissivity=0.9)
        atm.fluxes(surfaceTemperature=288, emissivity=0.9)
        assert ctx.profile_read()["xsec_accumulate"][0] == 0
        atm[2].changeTemperature(250)                      # one layer due: the counter does count
        atm.fluxes(surfaceTemperature=288, emissivity=0.9)
        assert ctx.profile_read()["xsec_accumulate"][0] >= 1
        ctx.profile_reset()
        atm[1].changeTemperature(255)
        atm.radiance([atm.nadirPath(), atm.reflectedPath()], surfaceTemperature=288, emissivity=0.9)
        assert ctx.profile_read()["xsec_accumulate"][0] >= 1
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
