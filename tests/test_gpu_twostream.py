"""GPU: two-stream multiple scattering of the solar beams (lbl_column_twostream_dev, kernels K5l;
Atmosphere.solarFluxesTwoStream) against the float64 NumPy restatement of tests/twostream_ref.py - which solves the column
in the other order than the kernels - on hand-made coefficients through the raw C ABI, in its limits (no scatterers: the
direct-beam call; no absorption: conservation; a layer and its halves), at the edge shapes, for independence of the
workspace's size, odd coefficients, determinism and the refusals; and through the model.

Tolerance: absolute, in units of the incident flux sum_s beam_weight_s S0 - per point for the spectra, summed over the
band's points for the band values: 1e-12, 40 times the error of the restatement itself against 60 digits (2.6e-14, the
issue's prototype; tests/test_twostream_cpu.py measures 1.6e-15 on its layers).  Points where some layer and beam has
|1 - lam m| < 1e-3 are near the pole of the particular solution, where float64 loses digits as 1e-17 / |1 - lam m|: they are
left out of the spectral comparison (at most 3 % of a case's points, none when every mu0 < 0.55) and held to 1e-6 of the
long-double restatement instead; a band's allowance is 1e-12 of the incident flux of its other points plus 1e-6 of theirs."""
import ctypes as C

import numpy as np
import pytest

import twostream_ref as ref
from pyrad_amd import synthetic
from test_gpu_flux import column, pyrad, source  # noqa: F401

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
TOL, TOL_POLE, NEAR_POLE = 1e-12, 1e-6, 1e-3
N, L4 = 1029, 4
BANDS = [(3, 517), (517, N)]


@pytest.fixture()
def ctx(pyrad):
    from pyrad_amd import engine
    return engine.get_engine().ctx


def hand_made(seed, L=L4, n=N, beams=1, scatterers=0, spectral=(), mu0=None):
    """k log-uniform with optical depths 1e-6 .. 1e2 over 1e4 cm; scatterer c has spectral numbers where c is in ``spectral``"""
    rs = np.random.RandomState(seed)
    k = 10.0 ** rs.uniform(-10, -2, (L, n))
    depth = np.full(L, 1e4)
    S0 = rs.uniform(0.5, 1.5, n)
    mu0 = rs.uniform(0.1, 1.0, beams) if mu0 is None else np.asarray(mu0, dtype=np.float64)
    slant = (1.0 / mu0)[:, None] * rs.uniform(0.9, 1.0, (beams, L))
    bw = rs.uniform(0.05, 0.3, beams)
    amount = 10.0 ** rs.uniform(-3, 1, (scatterers, L))
    numbers = []
    for c in range(scatterers):
        if c in spectral:
            numbers.append((rs.uniform(0.2, 2.0, n), rs.uniform(0.3, 1.0, n), rs.uniform(-0.3, 0.9, n)))
        else:
            numbers.append((float(rs.uniform(0.2, 2.0)), float(rs.uniform(0.5, 1.0)), float(rs.uniform(-0.3, 0.9))))
    return dict(k=k, depth=depth, S0=S0, beam_w=bw, slant=slant, amount=amount, numbers=numbers)


def run_raw(ctx, k, depth, S0, beam_w, slant, amount=(), numbers=(), delta=1, e=1.0, bands=None, spectra=True, passes=None):
    """lbl_column_twostream_dev on uploaded coefficients: (band sums [band, 3, level], the four spectra).  ``passes``: None -
    a workspace for the widest band; else the points of a pass (rounded up to whole tiles)"""
    k = np.asarray(k, dtype=np.float64)
    L, n = k.shape
    first, count = ([0], [n]) if bands is None else ([a for a, _ in bands], [b - a for a, b in bands])
    nb = len(first)
    bufs = [ctx.buffer(max(n, 1)).upload(k[l]) for l in range(L)]
    level, src = ctx.buffer(nb * 3 * (L + 1)), ctx.buffer(n).upload(np.asarray(S0, dtype=np.float64))
    work = ctx.buffer(ctx.column_twostream_workspace(L, max(count) if passes is None else passes))
    spec = [ctx.buffer(n) for _ in range(4)] if spectra else [None] * 4
    bufs += [level, src, work] + [b for b in spec if b is not None]
    try:
        def dev(v):
            if np.ndim(v) == 0:
                return float(v)
            bufs.append(ctx.buffer(n).upload(np.asarray(v, dtype=np.float64)))
            return bufs[-1]
        cols = [[dev(v) for v in triple] for triple in numbers]
        ctx.column_twostream_dev(bufs[:L], depth, 600.0, 700.0, n, src, beam_w, slant, amount, [c[0] for c in cols],
                                 [c[1] for c in cols], [c[2] for c in cols], delta, first, count, work, level,
                                 emissivity=dev(e), up_top=spec[0], down_surface=spec[1], direct_surface=spec[2],
                                 up_surface=spec[3])
        return (level.download(nb * 3 * (L + 1)).reshape(nb, 3, L + 1),) + tuple(
            b.download(n) if b is not None else None for b in spec)
    finally:
        for b in bufs:
            b.free()


_restated = {}


def restated(key, case, delta, e, dtype=np.float64):
    """the restatement of a case, made once and shared (never written to)"""
    key = (key, delta, "spectrum" if np.ndim(e) else float(e), np.dtype(dtype).name)
    if key not in _restated:
        _restated[key] = ref.column(case["k"], case["depth"], case["S0"], case["beam_w"], case["slant"], case["amount"],
                                    case["numbers"], delta, e, dtype=dtype)
    return _restated[key]


def check_raw(ctx, key, case, delta=1, e=1.0, bands=None, max_left_out=0.03, **kw):
    n = case["k"].shape[1]
    sums, *spec = run_raw(ctx, delta=delta, e=e, bands=bands, **case, **kw)
    up, dn, direct, pole = restated(key, case, delta, e)
    incident = np.sum(case["beam_w"]) * case["S0"]
    out = pole < NEAR_POLE
    share = out.mean()
    if out.any():                                      # the long-double restatement judges the points near the pole
        upl, dnl, directl, _ = restated(key, case, delta, e, np.longdouble)
        up, dn, direct = (np.where(out, b.astype(np.float64), a) for a, b in ((up, upl), (dn, dnl), (direct, directl)))
    idx = [(0, n)] if bands is None else bands
    inside = np.zeros(n, dtype=bool)
    for a, b in idx:
        inside[a:b] = True
    worst_band = 0.0
    for b, (lo, hi) in enumerate(idx):
        allow = TOL * incident[lo:hi][~out[lo:hi]].sum() + TOL_POLE * incident[lo:hi][out[lo:hi]].sum()
        for q, values in enumerate((up, dn, direct)):
            err = np.max(np.abs(sums[b, q] - ref.band_sums(values, lo, hi - lo))) / allow
            worst_band = max(worst_band, err)
    worst_spec = worst_pole = 0.0
    if spec[0] is not None:
        L = case["k"].shape[0]
        for got, want in zip(spec, (up[L], dn[0], direct[0], up[0])):
            assert np.all(got[~inside] == 0.0)
            err = np.abs(got - want) / incident
            worst_spec = max(worst_spec, np.max(err[inside & ~out], initial=0.0))
            worst_pole = max(worst_pole, np.max(err[inside & out], initial=0.0))
            assert np.all(np.isfinite(got[inside]))
    print("%s delta %d: near the pole %.2f %% of the points; band values %.2e of the allowance, spectra %.2e, near the pole "
          "%.2e of the incident flux" % (key, delta, 100 * share, worst_band, worst_spec, worst_pole))
    assert share <= max_left_out, share
    assert worst_band <= 1.0 and worst_spec <= TOL and worst_pole <= TOL_POLE
    return (sums,) + tuple(spec)


# ---- 1. against the restatement -----------------------------------------------------------------------------------------
def spectral_emissivity(n):
    return 0.55 + 0.4 * np.sin(0.37 * np.arange(n)) ** 2


EIGHT = [0.95, 0.7, 0.5, 0.4, 0.3, 0.2, 0.15, 0.1]           # two suns high enough to meet the pole
CASES = {
    # every mu0 < 0.55: lam <= sqrt(3) keeps lam m < 1 - no point may be left out
    "one beam, gas alone": (dict(seed=21, beams=1, mu0=[0.5]), 1, 1.0, None, 0.0),
    "one beam, low sun, four scatterers": (dict(seed=22, beams=1, mu0=[0.3], scatterers=4, spectral=(0, 2)), 1, 0.3, BANDS, 0.0),
    "three beams, a cloud": (dict(seed=23, beams=3, mu0=[0.9, 0.6, 0.15], scatterers=1), 1, 0.3, BANDS, 0.03),
    "three beams, a cloud, unscaled": (dict(seed=23, beams=3, mu0=[0.9, 0.6, 0.15], scatterers=1), 0, 0.0, None, 0.03),
    "eight beams, four scatterers": (dict(seed=24, beams=8, mu0=EIGHT, scatterers=4, spectral=(1, 3)), 0, "spectrum", BANDS, 0.03),
    "eight beams, four scatterers, scaled": (dict(seed=24, beams=8, mu0=EIGHT, scatterers=4, spectral=(1, 3)), 1, 0.0, BANDS, 0.03),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(ctx, name):
    make, delta, e, bands, max_left_out = CASES[name]
    case = hand_made(**make)
    if isinstance(e, str):
        e = spectral_emissivity(N)
    check_raw(ctx, name, case, delta, e, bands, max_left_out)


# ---- 2. the limits --------------------------------------------------------------------------------------------------------
def test_no_scatterers_is_the_direct_beam_call(ctx):
    """n_scat = 0: lbl_column_solar_dev over a Lambertian surface with the one diffuse angle mu = 1 / sqrt(3)"""
    case = hand_made(31, beams=3)
    e = spectral_emissivity(N)
    sums, ut, ds, dirs, us = run_raw(ctx, e=e, bands=BANDS, **case)
    bufs = [ctx.buffer(N).upload(case["k"][l]) for l in range(L4)]
    level, src, eb = ctx.buffer(2 * 2 * (L4 + 1)), ctx.buffer(N).upload(case["S0"]), ctx.buffer(N).upload(e)
    spec = [ctx.buffer(N) for _ in range(3)]
    try:
        ctx.column_solar_dev(bufs, case["depth"], 600.0, 700.0, N, src, case["beam_w"], case["slant"], [1.0 / np.sqrt(3.0)], [1.0],
                             [a for a, _ in BANDS], [b - a for a, b in BANDS], level, emissivity=eb, reflection=0,
                             up_top=spec[0], down_surface=spec[1], up_surface=spec[2])
        solar = level.download().reshape(2, 2, L4 + 1)
        s_ut, s_ds, s_us = (b.download(N) for b in spec)
    finally:
        for b in bufs + [level, src, eb] + spec:
            b.free()
    incident = np.sum(case["beam_w"]) * case["S0"]
    assert np.all(sums[:, 1] == 0.0) and np.all(ds == 0.0)          # nothing scatters: no diffuse light comes down
    for b, (lo, hi) in enumerate(BANDS):
        allow = TOL * incident[lo:hi].sum()
        assert np.max(np.abs(sums[b, 0] - solar[b, 0])) <= allow and np.max(np.abs(sums[b, 2] - solar[b, 1])) <= allow
    for got, want in ((ut, s_ut), (dirs, s_ds), (us, s_us)):
        assert np.max(np.abs(got - want) / incident) <= TOL


def test_conservation_without_absorption(ctx):
    """k = 0 and albedo 1 everywhere: the net flux is the same at every level, and what leaves at the top plus what the
    surface takes up is what came in"""
    case = hand_made(32, beams=3, scatterers=4, spectral=(0, 1))
    case["k"] = np.zeros_like(case["k"])
    case["numbers"] = [(ext, 1.0 if np.ndim(ssa) == 0 else np.ones(N), g) for ext, ssa, g in case["numbers"]]
    for e in (0.0, 0.35):
        sums, ut, ds, dirs, us = run_raw(ctx, e=e, **case)
        incident = np.sum(case["beam_w"]) * case["S0"]
        up, dn, direct = sums[0]
        net = (dn + direct) - up
        allow = TOL * incident.sum()
        print("e = %g: net flux constant to %.2e of the allowance" % (e, np.max(np.abs(net - net[L4])) / allow))
        assert np.max(np.abs(net - net[L4])) <= allow
        absorbed = (ds + dirs) - us
        assert np.max(np.abs((ut + absorbed) - incident) / incident) <= TOL
        if e == 0.0:
            assert np.max(np.abs(ut - incident) / incident) <= TOL


def test_a_layer_against_its_halves(ctx):
    case = hand_made(33, L=1, beams=2, scatterers=2, spectral=(1,), mu0=[0.5, 0.2])
    one = run_raw(ctx, e=0.3, **case)
    two = dict(case, k=np.vstack([case["k"]] * 2), depth=case["depth"].repeat(2) / 2, slant=np.hstack([case["slant"]] * 2),
               amount=np.hstack([case["amount"] / 2] * 2))
    halves = run_raw(ctx, e=0.3, **two)
    incident = np.sum(case["beam_w"]) * case["S0"]
    for q in range(3):
        assert np.max(np.abs(one[0][0, q, [0, 1]] - halves[0][0, q, [0, 2]])) <= TOL * incident.sum()
    for a, b in zip(one[1:], halves[1:]):
        assert np.max(np.abs(a - b) / incident) <= TOL


def test_at_the_pole_itself(ctx):
    """albedo 2 / 3 without asymmetry under an overhead sun: lam m = 1 to rounding in every layer, so every point takes the
    nudge m = (1 - 1e-6) / lam - finite, and within 1e-6 of the incident flux of the long-double restatement"""
    n = 70
    case = dict(k=np.zeros((2, n)), depth=np.full(2, 1e4), S0=np.linspace(0.5, 1.5, n), beam_w=np.array([0.8]),
                slant=np.ones((1, 2)), amount=np.array([[1e-3, 30.0]]),
                numbers=[(np.linspace(0.01, 3.0, n), 2.0 / 3.0, 0.0)])
    sums, *spec = run_raw(ctx, delta=0, e=0.2, **case)
    up, dn, direct, pole = ref.column(delta=0, emissivity=0.2, dtype=np.longdouble,
                                      **{("beam_weight" if key == "beam_w" else key): v for key, v in case.items()})
    assert np.all(pole < 1e-6)
    incident = 0.8 * case["S0"]
    for got, want in zip(spec, (up[2], dn[0], direct[0], up[0])):
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - want.astype(np.float64)) / incident) <= TOL_POLE
    assert np.all(np.isfinite(sums))


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------
def test_one_point_without_layers_and_the_layer_limit(ctx):
    from pyrad_amd import _native
    # n = 1, L = 0: every level is the source and the surface sends (1 - e) of it back
    sums, ut, ds, dirs, us = run_raw(ctx, np.zeros((0, 1)), [], [1.25], [0.3, 0.2], np.zeros((2, 0)), e=0.6)
    assert sums.shape == (1, 3, 1) and sums[0, 1, 0] == 0.0 and ds[0] == 0.0
    assert abs(dirs[0] - 0.5 * 1.25) <= 1e-15 and abs(us[0] - 0.4 * 0.5 * 1.25) <= 1e-15 and ut[0] == us[0]
    assert sums[0, 0, 0] == us[0] and sums[0, 2, 0] == dirs[0]
    L = _native.limit("layers_per_column")
    assert L == 128
    # (1,024 pairs of a layer and a beam per point: every mu0 < 0.55 keeps them all away from the pole)
    case = hand_made(34, L=L, n=300, beams=8, scatterers=4, spectral=(0, 3), mu0=np.linspace(0.1, 0.5, 8))
    case["k"] *= 1e-2
    case["amount"] *= 1e-2
    check_raw(ctx, "the layer limit", case, 1, spectral_emissivity(300), max_left_out=0.0)


def test_beyond_one_round_of_partial_slots(ctx):
    """4,101 tiles over 1,024 slots: a slot takes five tiles, and the last tile holds five points"""
    n = 1024 * 256 * 4 + 1029
    j = np.arange(n)
    case = dict(k=np.stack([1e-6 * (1 + (j % 7)), 1e-6 * (1 + ((j + 3) % 7))]), depth=np.array([2e5, 1e5]),
                S0=1.0 + 0.25 * ((j % 11) / 11.0), beam_w=np.array([0.5]), slant=np.array([[2.0, 1.9]]),
                amount=np.array([[0.3, 1.5]]), numbers=[(1.0, 0.95, 0.8)])
    check_raw(ctx, "one million points", case, 1, 0.7, max_left_out=0.0)


def test_the_pass_size_does_not_change_a_bit(ctx):
    case = hand_made(35, beams=3, scatterers=2, spectral=(0,))
    whole = run_raw(ctx, e=0.4, bands=BANDS, **case)
    tile = run_raw(ctx, e=0.4, bands=BANDS, passes=1, **case)
    two = run_raw(ctx, e=0.4, bands=BANDS, passes=300, **case)
    for other in (tile, two):
        for a, b in zip(whole, other):
            assert np.array_equal(a, b)


def test_zero_huge_inf_and_nan_coefficients(ctx):
    """single points of 0, 1e300, inf and NaN: a point where some layer's optical depth is not finite has NaN in the spectra
    and counts as 0 in the sums; 1e300 gives finite values; every other point keeps its bits"""
    case = hand_made(36, L=3, beams=2, scatterers=1)
    k = case["k"]
    k[0, 5], k[1, 6], k[2, 7], k[1, 400] = 0.0, 1e300, np.inf, np.nan
    k[0, 1027], k[2, 1028], k[2, 514] = np.nan, np.inf, 1e300
    bad = [7, 400, 1027, 1028]
    with np.errstate(invalid="ignore"):
        clean = np.where(np.isfinite(k) & (k < 1e299), k, 1e-5)
    sums, *spec = run_raw(ctx, e=0.5, **case)
    sums2, *spec2 = run_raw(ctx, e=0.5, **dict(case, k=clean))
    same = np.all(k == clean, axis=0)
    assert same.sum() == N - 6
    for a, b in zip(spec, spec2):
        assert np.all(np.isnan(a[bad])) and np.all(np.isfinite(a[[5, 6, 514]]))
        assert np.array_equal(a[same], b[same])
    assert np.all(np.isfinite(sums))
    # the sums are those of a column whose bad points shine no light
    dark = dict(case, k=np.where(np.isin(np.arange(N), bad), 1e-5, k), S0=np.where(np.isin(np.arange(N), bad), 0.0, case["S0"]))
    sums3 = run_raw(ctx, e=0.5, spectra=False, **dark)[0]
    assert np.array_equal(sums, sums3)


# ---- 4. determinism -------------------------------------------------------------------------------------------------------
def test_deterministic_and_a_beam_does_not_see_weightless_others(ctx):
    case = hand_made(37, beams=1, scatterers=2, spectral=(1,), mu0=[0.45])
    a = run_raw(ctx, e=0.3, bands=BANDS, **case)
    b = run_raw(ctx, e=0.3, bands=BANDS, **case)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    more = dict(case, beam_w=np.array([case["beam_w"][0], 0.0, 0.0]),
                slant=np.vstack([case["slant"], np.full((1, L4), 1.0 / 0.3), np.full((1, L4), 1.0 / 0.2)]))
    c = run_raw(ctx, e=0.3, bands=BANDS, **more)
    for x, y in zip(a, c):
        assert np.array_equal(x, y)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    L, n = 3, 1027
    k = hand_made(38, L=L, n=n)["k"]
    nv = 3 * (L + 1)
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    tile = ctx.column_twostream_workspace(L, 1)
    level, work = ctx.buffer(nv), ctx.buffer(2 * tile)
    spec = [ctx.buffer(n) for _ in range(4)]
    src, em, ext, ssa, asym = (ctx.buffer(n).upload(np.full(n, v)) for v in (1.1, 0.8, 1.5, 0.9, 0.7))
    level_short, n_short, work_short = ctx.buffer(nv - 1), ctx.buffer(n - 1), ctx.buffer(tile - 1)
    i64, f64 = lambda v: (C.c_int64 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    ptrs = lambda v: (C.c_void_p * max(len(v), 1))(*v)
    nmax, cmax = _native.limit("flux_angles"), _native.limit("scatterers")
    inf, nan = float("inf"), float("nan")
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=ptrs([b.h for b in kb]), depth=f64([1e4, 2e4, 1e4]), lo=600.0, hi=700.0, n=n,
                S0=src.h, n_beams=2, beam_weight=f64([0.5, 0.1]), slant=f64([2.0, 1.9, 1.8, 1.0, 1.0, 1.0]), n_scat=2,
                scat_amount=f64([0.1, 0.0, 2.0, 1.0, 1.0, 1.0]), scat_ext=ptrs([ext.h, None]), scat_ext_all=f64([0.0, 2.0]),
                scat_ssa=ptrs([ssa.h, None]), scat_ssa_all=f64([0.0, 1.0]), scat_asym=ptrs([asym.h, None]),
                scat_asym_all=f64([0.0, -0.2]), delta_scaling=1, n_bands=1, band_first=i64([0]), band_count=i64([n]),
                emissivity=em.h, emissivity_all=0.5, workspace=work.h, level_flux=level.h, up_top=spec[0].h,
                down_surface=spec[1].h, direct_surface=spec[2].h, up_surface=spec[3].h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_twostream_dev(*[a[key] for key in good])

    bad = [  # NULL arrays, negative counts
           dict(abs_coef=None), dict(depth=None), dict(S0=None), dict(beam_weight=None), dict(slant=None),
           dict(scat_amount=None), dict(band_first=None), dict(band_count=None), dict(level_flux=None), dict(workspace=None),
           dict(n_layers=-1), dict(n=-5), dict(n_beams=-1), dict(n_scat=-1), dict(n_bands=-1),
           # counts beyond their limits (and too few)
           dict(n_layers=_native.limit("layers_per_column") + 1), dict(n_beams=0),
           dict(n_beams=nmax + 1, beam_weight=f64([0.1] * (nmax + 1)), slant=f64([1.0] * (L * (nmax + 1)))),
           dict(n_scat=cmax + 1, scat_amount=f64([0.1] * (L * (cmax + 1))), scat_ext=None, scat_ext_all=f64([1.0] * (cmax + 1)),
                scat_ssa=None, scat_ssa_all=f64([1.0] * (cmax + 1)), scat_asym=None, scat_asym_all=f64([0.0] * (cmax + 1))),
           dict(n_bands=0), dict(n_bands=_native.limit("flux_bands") + 1),
           # buffers shorter than they must be
           dict(level_flux=level_short.h), dict(S0=n_short.h), dict(up_top=n_short.h), dict(down_surface=n_short.h),
           dict(direct_surface=n_short.h), dict(up_surface=n_short.h), dict(emissivity=n_short.h),
           dict(abs_coef=ptrs([kb[0].h, n_short.h, kb[2].h])), dict(scat_ext=ptrs([n_short.h, None])),
           dict(scat_ssa=ptrs([ssa.h, n_short.h])), dict(scat_asym=ptrs([n_short.h, None])), dict(workspace=work_short.h),
           # bands
           dict(band_count=i64([n + 1])), dict(band_first=i64([-1])), dict(band_count=i64([0])), dict(band_first=i64([n])),
           # depths, slants, beam weights
           dict(depth=f64([1e4, -1.0, 1e4])), dict(depth=f64([1e4, nan, 1e4])),
           dict(slant=f64([2.0, 1.9, 1.8, 1.0, 0.0, 1.0])), dict(slant=f64([2.0, 1.9, 1.8, 1.0, -1e-9, 1.0])),
           dict(slant=f64([2.0, inf, 1.8, 1.0, 1.0, 1.0])), dict(slant=f64([2.0, 1.9, 1.8, 1.0, 1.0, nan])),
           dict(beam_weight=f64([0.5, inf])), dict(beam_weight=f64([nan, 0.1])),
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
    outs = [level] + spec
    everything = kb + outs + [work, src, em, ext, ssa, asym, level_short, n_short, work_short]
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
        # not looked at beside a buffer: the numbers; and a NULL list of buffers means numbers throughout
        assert call(emissivity_all=7.0, scat_ext_all=f64([-1.0, 2.0]), scat_asym_all=f64([5.0, -0.2])) == 0
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        assert call(scat_ext=None, scat_ext_all=f64([1.5, 2.0]), scat_ssa=None, scat_ssa_all=f64([0.9, 1.0]), scat_asym=None,
                    scat_asym_all=f64([0.7, -0.2])) == 0
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        # what is allowed: no spectra, one emissivity, no scatterer (nothing of theirs is read)
        assert call(up_top=None, down_surface=None, direct_surface=None, up_surface=None, emissivity=None) == 0
        assert call(n_scat=0, scat_amount=None, scat_ext=None, scat_ext_all=None, scat_ssa=None, scat_ssa_all=None,
                    scat_asym=None, scat_asym_all=None) == 0
        assert call(beam_weight=f64([0.0, -1.0]), delta_scaling=0) == 0
        level.download()                                    # (the queue drains without an error)
    finally:
        for b in everything:
            b.free()


# ---- 6. the model ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def near_ir():
    source(co2=synthetic.make_lines(51, 800, 3480, 3620), h2o=synthetic.make_lines(52, 500, 3480, 3620))
    return 3500, 3600


def solar_source(x):
    return 0.8 + 0.5 * np.cos(0.21 * (x - x[0])) ** 2


def test_model_rayleigh_and_a_cloud(pyrad, near_ir):
    from pyrad_amd import settings
    atm = column(pyrad, rng=near_ir)
    x = atm[0].xAxis
    n, L = x.size, len(atm)
    air = pyrad.rayleighScatterer(atm)
    cloud = pyrad.Scatterer([0.0, 5.0, 0.0, 0.0], extinction=1.0, singleScatteringAlbedo=0.9, asymmetry=0.85, name="cloud")
    S0 = solar_source(x)
    e = spectral_emissivity(n)
    bands = [(3500, 3540), (3540, 3601)]
    got = atm.solarFluxesTwoStream([air, cloud], solarSpectrum=S0, mu0=[(0.5, 0.7), (0.25, 0.3)], geometry="spherical",
                                   emissivity=e, bands=bands, spectra=True)
    k = np.array([np.array(pyrad.getAbsCoef(Ly)) for Ly in atm])
    depth = [Ly.depth for Ly in atm]
    numbers = [(air.extinction, 1.0, 0.0), (1.0, 0.9, 0.85)]
    up, dn, direct, pole = ref.column(k, depth, S0, got.beamWeight, got.slant, [air.amounts, cloud.amounts], numbers, 1, e)
    assert np.all(pole >= NEAR_POLE)                    # (mu0 < 0.55)
    incident = np.sum(got.beamWeight) * S0
    res = settings.BASE_RESOLUTION
    idx = [(int(np.searchsorted(x, lo)), int(np.searchsorted(x, hi))) for lo, hi in bands]
    inside = np.zeros(n, dtype=bool)
    for b, (lo, hi) in enumerate(idx):
        inside[lo:hi] = True
        allow = TOL * incident[lo:hi].sum() * res
        want = [ref.band_sums(v, lo, hi - lo) * res for v in (up, dn + direct, direct)]
        errs = [np.max(np.abs(g[b] - w)) / allow for g, w in zip((got.up, got.down, got.direct), want)]
        print("band %d: up, down, direct %s of the allowance" % (b, " ".join("%.2e" % v for v in errs)))
        assert max(errs) <= 1.0
    for g, w in ((got.upSpectrum, up[L]), (got.downSpectrum, dn[0] + direct[0]), (got.directSpectrum, direct[0]),
                 (got.upSurfaceSpectrum, up[0])):
        assert np.max(np.abs(g - np.where(inside, w, 0.0)) / incident) <= TOL
    assert got.up.shape == got.down.shape == got.direct.shape == got.net.shape == (2, L + 1) and got.heatingRate.shape == (2, L)
    assert np.array_equal(got.net, got.up - got.down) and np.array_equal(got.absorbedSurface, got.down[:, 0] - got.up[:, 0])
    assert np.array_equal(got.heatingRate, pyrad.heatingRates(got.net, [Ly.P for Ly in atm], [Ly.T for Ly in atm], depth))
    assert np.all(got.direct <= got.down) and np.all(got.up[:, -1] > 0.0)          # the cloud sends light back to space
    print("reflected at the top / incident: %s" % (got.up[:, -1] / got.down[:, -1]))


def test_model_without_scatterers_is_solar_fluxes(pyrad, near_ir):
    atm = column(pyrad, rng=near_ir)
    x = atm[0].xAxis
    kw = dict(solarSpectrum=solar_source(x), mu0=[(0.6, 1.0), (0.2, 0.5)], emissivity=0.4, spectra=True)
    two = atm.solarFluxesTwoStream(**kw)
    one = atm.solarFluxes(angles=[(1.0 / np.sqrt(3.0), 1.0)], **kw)
    from pyrad_amd import settings
    incident = np.sum(two.beamWeight) * kw["solarSpectrum"]
    allow = TOL * incident.sum() * settings.BASE_RESOLUTION
    assert np.max(np.abs(two.up - one.up)) <= allow and np.max(np.abs(two.down - one.down)) <= allow
    assert np.array_equal(two.down, two.direct)
    assert np.array_equal(two.heatingRate, pyrad.heatingRates(two.net, [L.P for L in atm], [L.T for L in atm],
                                                              [L.depth for L in atm]))
    for a, b in ((two.upSpectrum, one.upSpectrum), (two.downSpectrum, one.downSpectrum),
                 (two.upSurfaceSpectrum, one.upSurfaceSpectrum)):
        assert np.max(np.abs(a - b) / incident) <= TOL


def test_model_other_calls_keep_their_bits(pyrad, near_ir, monkeypatch):
    from pyrad_amd import engine
    atm = column(pyrad, rng=near_ir)
    x = atm[0].xAxis
    thermal = dict(surfaceTemperature=288, emissivity=0.9, spectra=True)
    solar = dict(solarSpectrum=solar_source(x), mu0=0.5, emissivity=0.4, spectra=True)
    before = atm.fluxes(**thermal), atm.solarFluxes(**solar)
    # nothing is accumulated again after fluxes()
    ctx = engine.get_engine().ctx
    jobs = []
    for name in ("layers_merged_accumulate_dev", "layer_merged_step_dev", "xsec_accumulate_dev", "layer_step_dev",
                 "layer_sweep_dev"):
        orig = getattr(ctx, name)
        monkeypatch.setattr(ctx, name, lambda first, *a, _o=orig, _n=name, **kw: (jobs.append((_n, len(first))), _o(first, *a, **kw))[1])
    cloud = pyrad.Scatterer([0.0, 5.0, 0.0, 0.0], 1.0, 0.9, 0.85)
    a = atm.solarFluxesTwoStream([pyrad.rayleighScatterer(atm), cloud], bands=[(3500, 3550), (3550, 3601)], **solar)
    assert all(count == 0 for _, count in jobs), jobs
    after = atm.fluxes(**thermal), atm.solarFluxes(**solar)
    names = ("up", "down", "net", "heatingRate", "upSpectrum", "downSpectrum", "upSurfaceSpectrum")
    for x0, x1 in zip(before, after):
        for name in names:
            assert np.array_equal(getattr(x0, name), getattr(x1, name)), name
    b = atm.solarFluxesTwoStream([pyrad.rayleighScatterer(atm), cloud], bands=[(3500, 3550), (3550, 3601)], **solar)
    for name in names + ("direct", "directSpectrum", "absorbedSurface"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
