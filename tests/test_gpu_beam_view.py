"""GPU: scattered sunlight along a view (lbl_column_beam_radiance_dev, kernels K5o; Atmosphere.solarRadianceTwoStream)
against the float64 NumPy restatement of tests/beam_view_ref.py - its own grouping of the closed form, on the level fluxes of
twostream_ref, which solves the column in the other order than the kernels - on hand-made coefficients through the raw C
ABI; through the particular solution's pole and through mu == m; the identities (the two-stream angle, no scatterers, a layer
and its halves); the independence of a view from its neighbours, the pass size, two runs, the edge shapes, odd coefficients
and the refusals; and through the model.

Tolerance: absolute, in units of S0 / pi of the point.  Away from the pole (|1 - lam m| >= 0.05 in every layer, asserted of
the inputs) 1e-12, K5n's GPU bound, ten times the 1e-13 that tests/test_beam_view_cpu.py holds the restatement to against 50
digits.  Through the pole that file measures the restatement's own error (7.41e-13) and holds it to four times that; here
the bound is ten times the CPU one again, TOL_POLE = 10 POLE_BOUND = 2.96e-11.  No point is left out anywhere."""
import ctypes as C

import numpy as np
import pytest

import beam_view_ref as ref
from test_beam_view_cpu import (AWAY, CASES, MU3, POLE_BOUND, POLE_OFFSETS, VIEWS, away_from_the_pole, halved, hand_made,
                                mu_equal_m_views, pole_case, spectral_emissivity)
from test_gpu_flux import column, lines, pyrad  # noqa: F401
from test_gpu_twostream import run_raw as run_flux

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
TOL = 1e-12
TOL_POLE = 10 * POLE_BOUND
N, L4 = 1029, 4
LO, HI = 600.0, 700.0


@pytest.fixture()
def ctx(pyrad):
    from pyrad_amd import engine
    return engine.get_engine().ctx


def run_raw(ctx, k, depth, S0, beam_weight, slant, views, amount=(), numbers=(), delta=1, e=1.0, spectra=True, passes=None):
    """lbl_column_beam_radiance_dev on uploaded coefficients: (radiance (V, n), up_top, down_surface, direct_surface).
    ``passes``: None - a workspace for the whole grid; else the points of a pass (rounded up to whole tiles)"""
    k = np.asarray(k, dtype=np.float64)
    L, n = k.shape
    V = len(views)
    bufs = [ctx.buffer(max(n, 1)).upload(k[l]) for l in range(L)]
    rad, src = ctx.buffer(V * n), ctx.buffer(n).upload(np.asarray(S0, dtype=np.float64))
    work = ctx.buffer(ctx.column_beam_radiance_workspace(L, n if passes is None else passes))
    spec = [ctx.buffer(n) for _ in range(3)] if spectra else [None] * 3
    bufs += [rad, src, work] + [b for b in spec if b is not None]
    try:
        def dev(v):
            if np.ndim(v) == 0:
                return float(v)
            bufs.append(ctx.buffer(n).upload(np.asarray(v, dtype=np.float64)))
            return bufs[-1]
        cols = [[dev(v) for v in triple] for triple in numbers]
        ctx.column_beam_radiance_dev(bufs[:L], depth, LO, HI, n, src, beam_weight, slant, amount, [c[0] for c in cols],
                                     [c[1] for c in cols], [c[2] for c in cols], delta, [m for m, _ in views],
                                     [d for _, d in views], work, rad, emissivity=dev(e), up_top=spec[0], down_surface=spec[1],
                                     direct_surface=spec[2])
        return (rad.download(V * n).reshape(V, n),) + tuple(b.download(n) if b is not None else None for b in spec)
    finally:
        for b in bufs:
            b.free()


def restated(case, views, delta=1, e=1.0):
    """(radiance (V, n), up, dn, direct) of the restatement"""
    return ref.radiance(case["k"], case["depth"], case["S0"], case["beam_weight"], case["slant"], views, case["amount"],
                        case["numbers"], delta, e)[:4]


def check_raw(ctx, name, case, views=VIEWS, delta=1, e=1.0, tol=TOL, **kw):
    got, ut, ds, dr = run_raw(ctx, views=views, delta=delta, e=e, **case, **kw)
    want, up, dn, direct = restated(case, views, delta, e)
    assert np.all(np.isfinite(got))
    scale = case["S0"] / np.pi
    worst = np.max(np.abs(got - want) / scale, axis=1)
    flux_err = max(np.max(np.abs(ut - up[-1]) / scale), np.max(np.abs(ds - dn[0]) / scale),
                   np.max(np.abs(dr - direct[0]) / scale)) / np.pi
    print("%s: views %s of S0 / pi, the fluxes %.2e" % (name, " ".join("%.2e" % w for w in worst), flux_err))
    assert worst.max() <= tol and flux_err <= tol
    return got, ut, ds, dr


def case_kw(name, n=N):
    make, delta, e = CASES[name]
    case = hand_made(n=n, **make)
    assert away_from_the_pole(case, delta) >= AWAY
    return case, dict(delta=delta, e=spectral_emissivity(n) if isinstance(e, str) else e)


# ---- 1. against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(ctx, name):
    """spectral and constant scatterers, both scalings, e = 1, 0.3, 0 and a spectrum, slants that differ from layer to layer"""
    case, kw = case_kw(name)
    check_raw(ctx, name, case, **kw)


def test_against_the_restatement_with_spherical_slants(ctx, pyrad):
    case = hand_made(78, scatterers=2, spectral=(1,))
    case["slant"] = pyrad.solarSlants(case["depth"] * 3e2, 0.35, "spherical", 6.371e8)       # (shells 30 km thick)
    assert np.all(np.diff(case["slant"]) < 0) and away_from_the_pole(case, 1) >= AWAY
    check_raw(ctx, "spherical slants", case, e=0.3)
    case["slant"] = pyrad.solarSlants(case["depth"], 0.35, "plane")
    check_raw(ctx, "plane slants", case, e=0.3)


def test_through_the_pole(ctx):
    """lam m = 1 exactly and 1e-9, 1e-6, 1e-3, 1e-2 to either side in layer 1 of point 2: every point is compared"""
    for offset in POLE_OFFSETS:
        case, j = pole_case(offset)
        check_raw(ctx, "lam m = 1 %+.0e" % offset, case, e=0.4, tol=TOL_POLE)


def test_through_mu_equal_to_m(ctx):
    """down views at the sun's own cosine in layers 0 and 1, exactly and 1e-9, 1e-6, 1e-3 to either side: every point"""
    case = hand_made(81, L=3, scatterers=2, spectral=(1,), slant=[2.5, 1.0 / 0.43, 2.2])
    assert away_from_the_pole(case, 1) >= AWAY
    views = mu_equal_m_views(1.0 / case["slant"][0]) + mu_equal_m_views(1.0 / case["slant"][1])
    check_raw(ctx, "mu = m", case, views=views, e=0.3)


# ---- 2. the identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_at_the_two_stream_angle_the_radiance_is_the_flux(ctx, name):
    """mu = 1 / sqrt(3): pi Iu_L == up_L and pi Id_0 == dn_0 of the call's own spectra, which are K5l's bit for bit"""
    case, kw = case_kw(name)
    got, ut, ds, dr = run_raw(ctx, views=[(MU3, 0), (MU3, 1)], **case, **kw)
    err = max(np.max(np.abs(np.pi * got[0] - ut) / case["S0"]), np.max(np.abs(np.pi * got[1] - ds) / case["S0"]))
    print("%s: pi I at 1 / sqrt(3) within %.2e of S0 of the call's fluxes" % (name, err))
    assert err <= TOL
    flux_case = dict(case, beam_w=[case["beam_weight"]], slant=case["slant"][None, :])
    del flux_case["beam_weight"]
    _, f_ut, f_ds, f_dr, _ = run_flux(ctx, **flux_case, **kw)
    assert np.array_equal(ut, f_ut) and np.array_equal(ds, f_ds) and np.array_equal(dr, f_dr)


def test_no_scatterers_is_the_direct_beam_call(ctx):
    """n_scat = 0: an up view is lbl_column_solar_dev's Lambertian up_top / pi with the single angle (mu, pi); a down view
    is exactly 0"""
    case = hand_made(62)
    e = spectral_emissivity(N)
    got = run_raw(ctx, views=VIEWS, e=e, **case)[0]
    bufs = [ctx.buffer(N).upload(case["k"][l]) for l in range(L4)]
    src, eb, level, top = ctx.buffer(N).upload(case["S0"]), ctx.buffer(N).upload(e), ctx.buffer(2 * (L4 + 1)), ctx.buffer(N)
    try:
        worst = 0.0
        for v, (mu, down) in enumerate(VIEWS):
            if down:
                assert np.all(got[v] == 0.0)
                continue
            ctx.column_solar_dev(bufs, case["depth"], LO, HI, N, src, [case["beam_weight"]], case["slant"], [mu], [np.pi], [0],
                                 [N], level, emissivity=eb, reflection=0, up_top=top)
            worst = max(worst, np.max(np.abs(got[v] - top.download(N) / np.pi) / (case["S0"] / np.pi)))
    finally:
        for b in bufs + [src, eb, level, top]:
            b.free()
    print("no scatterers: within %.2e of S0 / pi of the direct-beam call" % worst)
    assert worst <= TOL


def test_a_layer_and_its_two_halves(ctx):
    case, kw = case_kw("four scatterers")
    whole, halves = run_raw(ctx, views=VIEWS, **case, **kw), run_raw(ctx, views=VIEWS, **halved(case), **kw)
    err = max(np.max(np.abs(a - b) / (case["S0"] / np.pi)) for a, b in zip(whole, halves))
    print("a layer and its two halves within %.2e of S0 / pi" % err)
    assert err <= TOL


def test_a_view_does_not_depend_on_the_other_views(ctx):
    """the same bits alone, among 16 views, and in another position of the list"""
    case = hand_made(82, scatterers=2, spectral=(0,))
    rs = np.random.RandomState(73)
    many = [(float(m), int(d)) for m, d in zip(rs.uniform(0.05, 1.0, 16), rs.randint(0, 2, 16))]
    many[3], many[11] = (0.37, 0), (0.37, 1)
    full = run_raw(ctx, views=many, e=0.4, **case)[0]
    for v in (3, 11, 15):
        alone = run_raw(ctx, views=[many[v]], e=0.4, **case)[0]
        assert np.array_equal(alone[0], full[v])
    moved = run_raw(ctx, views=[many[11], many[0], many[3]], e=0.4, **case)[0]
    assert np.array_equal(moved[0], full[11]) and np.array_equal(moved[1], full[0]) and np.array_equal(moved[2], full[3])


def test_the_pass_size_does_not_change_a_bit_and_two_runs_agree(ctx):
    case = hand_made(83, scatterers=2, spectral=(0,))
    kw = dict(views=VIEWS, e=0.4)
    whole = run_raw(ctx, **case, **kw)
    for other in (run_raw(ctx, passes=1, **case, **kw), run_raw(ctx, passes=300, **case, **kw), run_raw(ctx, **case, **kw)):
        for a, b in zip(whole, other):
            assert np.array_equal(a, b)


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------
def test_without_layers_one_layer_and_the_layer_limit(ctx):
    from pyrad_amd import _native
    # L = 0: an up view sees the surface's (1 - e) beam_weight S0 / pi exactly, a down view nothing
    S0 = np.array([2.0, 1.0, 0.5])
    got, ut, ds, dr = run_raw(ctx, np.zeros((0, 3)), [], S0, 0.3, [], [(0.3, 0), (1.0, 1), (0.7, 0)], e=0.6)
    want = ((1 - 0.6) * (0.3 * S0)) / np.pi
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want) and np.all(got[1] == 0.0)
    assert np.array_equal(ut, (1 - 0.6) * (0.3 * S0)) and np.all(ds == 0.0) and np.array_equal(dr, 0.3 * S0)
    case = hand_made(84, L=1, n=300, scatterers=2, spectral=(1,))
    check_raw(ctx, "one layer", case, e=0.5)
    L = _native.limit("layers_per_column")
    assert L == 128 and _native.limit("beam_views") == 16
    case = hand_made(85, L=L, n=257, scatterers=4, spectral=(0, 3))
    case["k"] *= 1e-2
    case["amount"] *= 1e-2
    assert away_from_the_pole(case, 1) >= AWAY
    rs = np.random.RandomState(74)
    views = [(float(m), int(d)) for m, d in zip(rs.uniform(0.05, 1.0, 16), rs.randint(0, 2, 16))]
    check_raw(ctx, "the layer limit, 16 views", case, views=views, e=spectral_emissivity(257))


def test_zero_huge_inf_and_nan_coefficients(ctx):
    """single points of 0, 1e300, inf and NaN: a point where some layer's optical depth is not finite is NaN in every
    output; 1e300 gives finite values, against the restatement; every other point keeps its bits"""
    case = hand_made(86, L=3, scatterers=1)
    k = case["k"]
    k[0, 5], k[1, 6], k[2, 7], k[1, 400] = 0.0, 1e300, np.inf, np.nan
    k[0, 1027], k[2, 1028], k[2, 514] = np.nan, np.inf, 1e300
    bad = [7, 400, 1027, 1028]
    with np.errstate(invalid="ignore"):
        clean = np.where(np.isfinite(k) & (k < 1e299), k, 1e-5)
    got = run_raw(ctx, views=VIEWS, e=0.5, **case)
    got2 = run_raw(ctx, views=VIEWS, e=0.5, **dict(case, k=clean))
    same = np.all(k == clean, axis=0)
    assert same.sum() == N - 6
    for a, b in zip(got, got2):
        a, b = np.atleast_2d(a), np.atleast_2d(b)
        assert np.all(np.isnan(a[:, bad])) and np.all(np.isfinite(a[:, [5, 6, 514]]))
        assert np.array_equal(a[:, same], b[:, same])
    good = np.array([5, 6, 514])
    want = restated(case, VIEWS, 1, 0.5)[0]
    assert np.max(np.abs(got[0][:, good] - want[:, good]) / (case["S0"][good] / np.pi)) <= TOL


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    L, n, V = 3, 1027, 3
    k = hand_made(87, L=L, n=n)["k"]
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    tile = ctx.column_beam_radiance_workspace(L, 1)
    rad, work = ctx.buffer(V * n), ctx.buffer(2 * tile)
    spec = [ctx.buffer(n) for _ in range(3)]
    S0, em, ext, ssa, asym = (ctx.buffer(n).upload(np.full(n, v)) for v in (1.1, 0.8, 1.5, 0.9, 0.7))
    rad_short, n_short, work_short = ctx.buffer(V * n - 1), ctx.buffer(n - 1), ctx.buffer(tile - 1)
    f64 = lambda v: (C.c_double * max(len(v), 1))(*v)
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    ptrs = lambda v: (C.c_void_p * max(len(v), 1))(*v)
    cmax, vmax = _native.limit("scatterers"), _native.limit("beam_views")
    inf, nan = float("inf"), float("nan")
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=ptrs([b.h for b in kb]), depth=f64([1e4, 2e4, 1e4]), lo=LO, hi=HI, n=n, S0=S0.h,
                beam_weight=0.4, slant=f64([2.5, 2.4, 2.3]), n_scat=2, scat_amount=f64([0.1, 0.0, 2.0, 1.0, 1.0, 1.0]),
                scat_ext=ptrs([ext.h, None]), scat_ext_all=f64([0.0, 2.0]), scat_ssa=ptrs([ssa.h, None]),
                scat_ssa_all=f64([0.0, 1.0]), scat_asym=ptrs([asym.h, None]), scat_asym_all=f64([0.0, -0.2]), delta_scaling=1,
                emissivity=em.h, emissivity_all=0.5, n_views=V, view_mu=f64([1.0, 0.5, 0.2]), view_down=i32([0, 1, 0]),
                workspace=work.h, radiance=rad.h, up_top=spec[0].h, down_surface=spec[1].h, direct_surface=spec[2].h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_beam_radiance_dev(*[a[key] for key in good])

    bad = [  # NULL arrays, negative counts
           dict(abs_coef=None), dict(depth=None), dict(slant=None), dict(scat_amount=None), dict(radiance=None), dict(S0=None),
           dict(workspace=None), dict(view_mu=None), dict(view_down=None),
           dict(n_layers=-1), dict(n=-5), dict(n=0), dict(n_scat=-1), dict(n_views=-1), dict(n_views=0),
           # counts beyond their limits
           dict(n_layers=_native.limit("layers_per_column") + 1),
           dict(n_scat=cmax + 1, scat_amount=f64([0.1] * (L * (cmax + 1))), scat_ext=None, scat_ext_all=f64([1.0] * (cmax + 1)),
                scat_ssa=None, scat_ssa_all=f64([1.0] * (cmax + 1)), scat_asym=None, scat_asym_all=f64([0.0] * (cmax + 1))),
           dict(n_views=vmax + 1, view_mu=f64([0.5] * (vmax + 1)), view_down=i32([0] * (vmax + 1))),
           # the views
           dict(view_mu=f64([1.0, 0.0, 0.2])), dict(view_mu=f64([1.0, 0.5, 1.0000001])), dict(view_mu=f64([-0.5, 0.5, 0.2])),
           dict(view_mu=f64([1.0, nan, 0.2])), dict(view_mu=f64([inf, 0.5, 0.2])),
           dict(view_down=i32([0, 2, 0])), dict(view_down=i32([-1, 1, 0])),
           # buffers shorter than they must be
           dict(radiance=rad_short.h), dict(S0=n_short.h), dict(up_top=n_short.h), dict(down_surface=n_short.h),
           dict(direct_surface=n_short.h), dict(emissivity=n_short.h),
           dict(abs_coef=ptrs([kb[0].h, n_short.h, kb[2].h])), dict(scat_ext=ptrs([n_short.h, None])),
           dict(scat_ssa=ptrs([ssa.h, n_short.h])), dict(scat_asym=ptrs([n_short.h, None])), dict(workspace=work_short.h),
           # depths, the beam
           dict(depth=f64([1e4, -1.0, 1e4])), dict(depth=f64([1e4, nan, 1e4])),
           dict(beam_weight=nan), dict(beam_weight=inf), dict(slant=f64([2.5, 0.0, 2.3])), dict(slant=f64([2.5, -1.0, 2.3])),
           dict(slant=f64([nan, 2.4, 2.3])), dict(slant=f64([2.5, 2.4, inf])),
           # amounts
           dict(scat_amount=f64([0.1, -1e-9, 2.0, 1.0, 1.0, 1.0])), dict(scat_amount=f64([0.1, 0.0, 2.0, 1.0, nan, 1.0])),
           dict(scat_amount=f64([inf, 0.0, 2.0, 1.0, 1.0, 1.0])),
           # the numbers of a scatterer without a buffer
           dict(scat_ext_all=f64([0.0, -1.0])), dict(scat_ext_all=f64([0.0, inf])), dict(scat_ext_all=f64([0.0, nan])),
           dict(scat_ext_all=None), dict(scat_ssa_all=f64([0.0, -0.01])), dict(scat_ssa_all=f64([0.0, 1.01])),
           dict(scat_ssa_all=f64([0.0, nan])), dict(scat_asym_all=f64([0.0, 1.0])), dict(scat_asym_all=f64([0.0, -1.0])),
           dict(scat_asym_all=f64([0.0, nan])), dict(scat_ext=None, scat_ext_all=f64([-1.0, 2.0])),
           # the switch and the surface
           dict(delta_scaling=2), dict(delta_scaling=-1),
           dict(emissivity=None, emissivity_all=-0.01), dict(emissivity=None, emissivity_all=1.01),
           dict(emissivity=None, emissivity_all=nan)]
    outs = [rad] + spec
    everything = kb + outs + [work, S0, em, ext, ssa, asym, rad_short, n_short, work_short]
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
        # what is allowed: no spectra, one emissivity, no scatterer, no scaling, and the view limit itself
        assert call() == 0
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        assert call(up_top=None, down_surface=None, direct_surface=None, emissivity=None) == 0
        assert call(n_scat=0, scat_amount=None, scat_ext=None, scat_ext_all=None, scat_ssa=None, scat_ssa_all=None,
                    scat_asym=None, scat_asym_all=None, delta_scaling=0) == 0
        wide = ctx.buffer(vmax * n)
        everything.append(wide)
        assert call(n_views=vmax, view_mu=f64([0.5] * vmax), view_down=i32([0, 1] * (vmax // 2)), radiance=wide.h) == 0
        wide.download()                                     # (the queue drains without an error)
    finally:
        for b in everything:
            b.free()


# ---- 5. the model ---------------------------------------------------------------------------------------------------------
def test_model_without_scatterers_is_solar_fluxes(pyrad, lines):
    atm = column(pyrad)
    views = [1.0, (0.6, "up"), (0.6, "down"), (1.0, "down")]
    kw = dict(solarTemperature=5772.0, mu0=0.5, emissivity=0.7)
    got = atm.solarRadianceTwoStream(views, **kw)
    n = atm[0].xAxis.size
    assert got.radiance.shape == (4, n) and list(got.direction) == ["up", "up", "down", "down"]
    assert list(got.mu) == [1.0, 0.6, 0.6, 1.0] and np.array_equal(got.wavenumber, atm[0].xAxis)
    assert np.all(got.radiance[2:] == 0.0)
    S0 = pyrad.solarIrradiance(atm[0].xAxis, 5772.0)
    for v, mu in ((0, 1.0), (1, 0.6)):
        one = atm.solarFluxes(angles=[(mu, np.pi)], spectra=True, **kw)
        worst = np.max(np.abs(got.radiance[v] - one.upSpectrum / np.pi) / (S0 / np.pi))
        print("mu %.1f: solarRadianceTwoStream without scatterers within %.2e of S0 / pi of solarFluxes()" % (mu, worst))
        assert worst <= TOL


def test_model_chunks_of_views_and_an_instrument(pyrad, lines):
    """17 views equal the same views in separate calls bit for bit; the channels are convolve() of the spectral result"""
    atm = column(pyrad)
    cloud = pyrad.Scatterer([0.0, 0.0, 2.0, 0.0], extinction=1.0, singleScatteringAlbedo=0.9, asymmetry=0.8, name="cloud")
    rs = np.random.RandomState(75)
    views = [(float(m), "down" if d else "up") for m, d in zip(rs.uniform(0.1, 1.0, 17), rs.randint(0, 2, 17))]
    kw = dict(scatterers=[cloud, pyrad.rayleighScatterer(atm)], solarTemperature=5772.0, mu0=0.6, geometry="spherical",
              emissivity=0.9)
    full = atm.solarRadianceTwoStream(views, **kw)
    assert full.radiance.shape == (17, atm[0].xAxis.size) and np.all(np.isfinite(full.radiance))
    for v in (0, 15, 16):
        alone = atm.solarRadianceTwoStream([views[v]], **kw)
        assert np.array_equal(alone.radiance[0], full.radiance[v])
    ins = pyrad.Instrument(np.arange(610.0, 690.0, 0.5), width=0.5)
    ch = atm.solarRadianceTwoStream(views, instrument=ins, **kw)
    first = atm[0]
    assert ch.radiance.shape == (17, len(ins)) and np.array_equal(ch.wavenumber, ins.centres)
    assert np.array_equal(ch.radiance, pyrad.convolve(ins, full.radiance, first.rangeMin, first.rangeMax))


def test_model_a_grey_cloud_in_the_top_layer(pyrad, lines):
    """a cloud in the top layer brightens the nadir window radiance over a black surface and dims it over a white one; both
    against the restatement on the model's own coefficients"""
    atm = column(pyrad)
    cloud = pyrad.Scatterer([0.0, 0.0, 0.0, 5.0], extinction=1.0, singleScatteringAlbedo=0.9, asymmetry=0.85, name="cloud")
    views = [(1.0, "up"), (1.0, "down"), (0.4, "up"), (0.4, "down")]
    x = atm[0].xAxis
    k = np.array([np.array(pyrad.getAbsCoef(Ly)) for Ly in atm])
    window = int(np.argmin(k.sum(axis=0)))                 # the most transparent point of the grid
    S0 = pyrad.solarIrradiance(x, 5772.0)
    depth = [Ly.depth for Ly in atm]
    for e, brighter in ((1.0, True), (0.0, False)):
        kw = dict(solarTemperature=5772.0, mu0=0.4, emissivity=e)
        clear = atm.solarRadianceTwoStream(views, **kw)
        cloudy = atm.solarRadianceTwoStream(views, [cloud], **kw)
        print("albedo %.2f: window at %.2f cm^-1, nadir radiance %.4g -> %.4g of S0 / pi" % (
            1 - e, x[window], clear.radiance[0, window] / (S0[window] / np.pi), cloudy.radiance[0, window] / (S0[window] / np.pi)))
        assert (cloudy.radiance[0, window] > clear.radiance[0, window]) == brighter
        assert cloudy.radiance[0, window] != clear.radiance[0, window]
        again = atm.solarRadianceTwoStream(views, [cloud], **kw)           # the kept state is sound
        assert np.array_equal(again.radiance, cloudy.radiance)
        want, _, _, _, pole = ref.radiance(k, depth, S0, 0.4, pyrad.solarSlants(depth, 0.4), [(m, int(d == "down")) for m, d in views],
                                           [cloud.amounts], [(1.0, 0.9, 0.85)], 1, e)
        assert np.all(pole >= AWAY)                         # (mu0 = 0.4: lam m <= 0.7)
        worst = np.max(np.abs(cloudy.radiance - want) / (S0 / np.pi))
        print("albedo %.2f: the model within %.2e of S0 / pi of the restatement" % (1 - e, worst))
        assert worst <= TOL
