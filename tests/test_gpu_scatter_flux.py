"""GPU: thermal fluxes through scattering layers (lbl_column_flux_scatter_dev, kernels K5m; Atmosphere.fluxesTwoStream)
against the float64 NumPy restatement of tests/scatter_flux_ref.py - which solves the column in the other order than the
kernels - on hand-made coefficients through the raw C ABI; the identities (equal edges, no scatterers, the Kirchhoff cavity,
the pass size, two runs), the edge shapes, odd coefficients and the refusals; and through the model.

Tolerance: absolute, 1e-12 in units of the point's scale - pi times the largest of the Planck values and boundary radiances
that enter it; for band values summed over the band's points.  No point is left out: there is no beam and hence no pole, and
the restatement itself stays inside 1e-13 of 60 digits everywhere (tests/test_scatter_flux_cpu.py measures 3.7e-16)."""
import ctypes as C

import numpy as np
import pytest

import scatter_flux_ref as ref
from test_gpu_flux import column, lines, pyrad  # noqa: F401

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
TOL = 1e-12
N, L4 = 1029, 4
BANDS = [(3, 517), (517, N)]
LO, HI = 600.0, 700.0
MU, W = 1.0 / np.sqrt(3.0), np.pi


@pytest.fixture()
def ctx(pyrad):
    from pyrad_amd import engine
    return engine.get_engine().ctx


def grid(n):
    return np.linspace(LO, HI, n)


def spectral_emissivity(n):
    return 0.55 + 0.4 * np.sin(0.37 * np.arange(n)) ** 2


def hand_made(seed, L=L4, n=N, scatterers=0, spectral=(), linear=True, joined=True):
    """k log-uniform with optical depths 1e-6 .. 1e2 over 1e4 cm, temperatures 200 .. 300 K: one per layer, or the edges'
    (bottom, top) - those of L + 1 levels where ``joined``, else 2 L of their own; scatterer c has spectral numbers where c
    is in ``spectral``"""
    rs = np.random.RandomState(seed)
    k = 10.0 ** rs.uniform(-10, -2, (L, n))
    depth = np.full(L, 1e4)
    if not linear:
        T = rs.uniform(200, 300, L)
    elif joined:
        lev = rs.uniform(200, 300, L + 1)
        T = np.column_stack([lev[:-1], lev[1:]])
    else:
        T = rs.uniform(200, 300, (L, 2))
    amount = 10.0 ** rs.uniform(-3, 1, (scatterers, L))
    numbers = []
    for c in range(scatterers):
        if c in spectral:
            numbers.append((rs.uniform(0.2, 2.0, n), rs.uniform(0.3, 1.0, n), rs.uniform(-0.3, 0.9, n)))
        else:
            numbers.append((float(rs.uniform(0.2, 2.0)), float(rs.uniform(0.5, 1.0)), float(rs.uniform(-0.3, 0.9))))
    return dict(k=k, depth=depth, T=T, linear=linear, amount=amount, numbers=numbers)


def edges_of(case):
    """(L, 2) bottom and top edge temperatures of a case, whichever source it has"""
    T = np.asarray(case["T"], dtype=np.float64)
    return T.reshape(-1, 2) if case["linear"] else np.column_stack([T, T])


def run_raw(ctx, k, depth, T, linear, amount=(), numbers=(), delta=1, e=1.0, surface_T=0.0, I_surface=None, I_top=None,
            bands=None, spectra=True, passes=None):
    """lbl_column_flux_scatter_dev on uploaded coefficients: (band sums [band, 2, level], up_top, down_surface, up_surface).
    ``passes``: None - a workspace for the widest band; else the points of a pass (rounded up to whole tiles)"""
    k = np.asarray(k, dtype=np.float64)
    L, n = k.shape
    first, count = ([0], [n]) if bands is None else ([a for a, _ in bands], [b - a for a, b in bands])
    nb = len(first)
    bufs = [ctx.buffer(max(n, 1)).upload(k[l]) for l in range(L)]
    level = ctx.buffer(nb * 2 * (L + 1))
    work = ctx.buffer(ctx.column_flux_scatter_workspace(L, max(count) if passes is None else passes))
    spec = [ctx.buffer(n) for _ in range(3)] if spectra else [None] * 3
    bufs += [level, work] + [b for b in spec if b is not None]
    try:
        def dev(v):
            if v is None or np.ndim(v) == 0:
                return v if v is None else float(v)
            bufs.append(ctx.buffer(n).upload(np.asarray(v, dtype=np.float64)))
            return bufs[-1]
        cols = [[dev(v) for v in triple] for triple in numbers]
        ctx.column_flux_scatter_dev(bufs[:L], T, int(linear), depth, LO, HI, n, amount, [c[0] for c in cols],
                                    [c[1] for c in cols], [c[2] for c in cols], delta, first, count, work, level,
                                    emissivity=dev(e), I_surface=dev(I_surface), surface_T=surface_T, I_top=dev(I_top),
                                    up_top=spec[0], down_surface=spec[1], up_surface=spec[2])
        return (level.download(nb * 2 * (L + 1)).reshape(nb, 2, L + 1),) + tuple(
            b.download(n) if b is not None else None for b in spec)
    finally:
        for b in bufs:
            b.free()


def check_raw(ctx, name, case, delta=1, e=1.0, surface_T=0.0, I_surface=None, I_top=None, bands=None, points=None, **kw):
    """a run against the restatement, at every point or, with ``points``, at those (the band values are then not compared)"""
    L, n = case["k"].shape
    sums, *spec = run_raw(ctx, delta=delta, e=e, surface_T=surface_T, I_surface=I_surface, I_top=I_top, bands=bands, **case,
                          **kw)
    at = np.arange(n) if points is None else points
    pick = lambda v: v if v is None or np.ndim(v) == 0 else np.asarray(v)[at]
    numbers = [tuple(pick(v) for v in triple) for triple in case["numbers"]]
    nu = grid(n)[at]
    up, dn = ref.column(case["k"][:, at], case["depth"], nu, edges_of(case), case["amount"], numbers, delta, pick(e),
                        I_surface=pick(I_surface), surface_T=surface_T, I_top=pick(I_top))
    scale = ref.scale(nu, edges_of(case), I_surface=pick(I_surface), surface_T=surface_T, I_top=pick(I_top))
    idx = [(0, n)] if bands is None else bands
    inside = np.zeros(n, dtype=bool)
    for a, b in idx:
        inside[a:b] = True
    worst_band = 0.0
    if points is None:
        for b, (lo, hi) in enumerate(idx):
            allow = TOL * scale[lo:hi].sum()
            for q, values in enumerate((up, dn)):
                worst_band = max(worst_band, np.max(np.abs(sums[b, q] - ref.band_sums(values, lo, hi - lo))) / allow)
    worst_spec = 0.0
    if spec[0] is not None:
        for got, want in zip(spec, (up[L], dn[0], up[0])):
            assert np.all(got[~inside] == 0.0) and np.all(np.isfinite(got[inside]))
            worst_spec = max(worst_spec, np.max(np.abs(got[at] - want)[inside[at]] / scale[inside[at]], initial=0.0))
    print("%s: band values %.2e of the allowance, spectra %.2e of the scale" % (name, worst_band, worst_spec))
    assert worst_band <= 1.0 and worst_spec <= TOL
    return (sums,) + tuple(spec)


# ---- 1. against the restatement -----------------------------------------------------------------------------------------
def surface_radiance(n):
    return ref.planck(grid(n), 285.0) * (0.9 + 0.1 * np.cos(0.11 * np.arange(n)))


def sky_radiance(n):
    return ref.planck(grid(n), 180.0) * (1.0 + 0.5 * np.sin(0.23 * np.arange(n)) ** 2)


#        name: (hand_made's arguments, delta, e, surface ("T" or "I"), I_top?, bands)
CASES = {
    "gas alone, layer source": (dict(seed=51, linear=False), 1, 1.0, "T", False, None),
    "gas alone, linear source": (dict(seed=52, linear=True), 1, 0.3, "I", True, BANDS),
    "one scatterer, layer source, unscaled": (dict(seed=53, linear=False, scatterers=1), 0, 0.0, "T", True, None),
    "one spectral scatterer, linear source": (dict(seed=54, linear=True, scatterers=1, spectral=(0,)), 1, "spectrum", "T", False, BANDS),
    "four scatterers, layer source": (dict(seed=55, linear=False, scatterers=4, spectral=(0, 2)), 1, 0.3, "I", True, BANDS),
    "four scatterers, linear source, unscaled, edges apart": (
        dict(seed=56, linear=True, joined=False, scatterers=4, spectral=(1, 3)), 0, "spectrum", "T", False, None),
    "four scatterers, linear source, black surface": (dict(seed=57, linear=True, scatterers=4), 1, 1.0, "I", True, BANDS),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(ctx, name):
    make, delta, e, surface, top, bands = CASES[name]
    case = hand_made(**make)
    if isinstance(e, str):
        e = spectral_emissivity(N)
    check_raw(ctx, name, case, delta, e, surface_T=291.5 if surface == "T" else 0.0,
              I_surface=surface_radiance(N) if surface == "I" else None, I_top=sky_radiance(N) if top else None, bands=bands)


# ---- 2. the identities ----------------------------------------------------------------------------------------------------
def test_equal_edges_are_the_layer_source_bit_for_bit(ctx):
    case = hand_made(61, linear=False, scatterers=3, spectral=(1,))
    kw = dict(e=spectral_emissivity(N), surface_T=288.0, I_top=sky_radiance(N), bands=BANDS)
    layer = run_raw(ctx, **case, **kw)
    linear = run_raw(ctx, **dict(case, T=np.repeat(case["T"], 2), linear=True), **kw)
    for a, b in zip(layer, linear):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("linear", (False, True))
def test_no_scatterers_is_the_surface_call(ctx, linear):
    """n_scat = 0: lbl_column_flux_surface_dev (lbl_column_flux_linear_dev) over a Lambertian surface with the angle set
    {(1 / sqrt(3), pi)} - to the tolerance, not bit for bit: the Planck paths differ"""
    case = hand_made(62, linear=linear)
    e, I_top = spectral_emissivity(N), sky_radiance(N)
    sums, ut, ds, us = run_raw(ctx, e=e, surface_T=295.0, I_top=I_top, bands=BANDS, **case)
    bufs = [ctx.buffer(N).upload(case["k"][l]) for l in range(L4)]
    level, eb, tb = ctx.buffer(2 * 2 * (L4 + 1)), ctx.buffer(N).upload(e), ctx.buffer(N).upload(I_top)
    spec = [ctx.buffer(N) for _ in range(3)]
    try:
        call = ctx.column_flux_linear_dev if linear else ctx.column_flux_surface_dev
        call(bufs, case["T"], case["depth"], LO, HI, N, [MU], [W], [a for a, _ in BANDS], [b - a for a, b in BANDS], level,
             eb, reflection=0, surface_T=295.0, I_top=tb, up_top=spec[0], down_surface=spec[1], up_surface=spec[2])
        other = level.download().reshape(2, 2, L4 + 1)
        o_ut, o_ds, o_us = (b.download(N) for b in spec)
    finally:
        for b in bufs + [level, eb, tb] + spec:
            b.free()
    scale = ref.scale(grid(N), edges_of(case), surface_T=295.0, I_top=I_top)
    worst = 0.0
    for b, (lo, hi) in enumerate(BANDS):
        worst = max(worst, np.max(np.abs(sums[b] - other[b])) / (TOL * scale[lo:hi].sum()))
    worst_spec = max(np.max(np.abs(a - b) / scale) for a, b in ((ut, o_ut), (ds, o_ds), (us, o_us)))
    print("no scatterers, %s: band values %.2e of the allowance, spectra %.2e of the scale" % (
        "linear" if linear else "layer", worst, worst_spec))
    assert worst <= 1.0 and worst_spec <= TOL


@pytest.mark.parametrize("linear", (False, True))
def test_kirchhoff_cavity(ctx, linear):
    """one temperature everywhere, the sky included: up = dn = pi B(T0) at every level and no net flux"""
    T0 = 255.0
    case = hand_made(63, linear=linear, scatterers=4, spectral=(0, 3))
    case["T"] = np.full_like(case["T"], T0)
    B = ref.planck(grid(N), T0)
    for e in (0.0, 0.3, spectral_emissivity(N)):
        sums, ut, ds, us = run_raw(ctx, e=e, surface_T=T0, I_top=B, **case)
        allow = TOL * (np.pi * B).sum()
        up, dn = sums[0]
        print("cavity: up %.2e, dn %.2e, net %.2e of the allowance" % tuple(
            np.max(np.abs(v)) / allow for v in (up - (np.pi * B).sum(), dn - (np.pi * B).sum(), up - dn)))
        assert np.max(np.abs(up - (np.pi * B).sum())) <= allow and np.max(np.abs(dn - (np.pi * B).sum())) <= allow
        assert np.max(np.abs(up - dn)) <= allow
        for v in (ut, ds, us):
            assert np.max(np.abs(v / (np.pi * B) - 1.0)) <= TOL


def test_the_pass_size_does_not_change_a_bit(ctx):
    case = hand_made(64, scatterers=2, spectral=(0,))
    kw = dict(e=0.4, surface_T=290.0, I_top=sky_radiance(N), bands=BANDS)
    whole = run_raw(ctx, **case, **kw)
    tile = run_raw(ctx, passes=1, **case, **kw)
    two = run_raw(ctx, passes=300, **case, **kw)
    for other in (tile, two):
        for a, b in zip(whole, other):
            assert np.array_equal(a, b)


def test_deterministic(ctx):
    case = hand_made(65, scatterers=2, spectral=(1,))
    kw = dict(e=0.3, I_surface=surface_radiance(N), bands=BANDS)
    for x, y in zip(run_raw(ctx, **case, **kw), run_raw(ctx, **case, **kw)):
        assert np.array_equal(x, y)


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------
def test_one_point_without_layers_one_layer_and_the_layer_limit(ctx):
    from pyrad_amd import _native
    # n = 1, L = 0: the sky comes down unchanged and the surface emits e pi Is and sends (1 - e) of the sky back
    for linear in (0, 1):
        sums, ut, ds, us = run_raw(ctx, np.zeros((0, 1)), [], [], linear, e=0.6, I_surface=[2.0], I_top=[0.5])
        assert sums.shape == (1, 2, 1) and ds[0] == np.pi * 0.5 and ut[0] == us[0] == sums[0, 0, 0] and sums[0, 1, 0] == ds[0]
        assert abs(us[0] - (0.6 * np.pi * 2.0 + 0.4 * np.pi * 0.5)) <= 1e-15 * np.pi * 2.0
    for linear in (False, True):
        case = hand_made(66, L=1, n=300, scatterers=2, spectral=(1,), linear=linear)
        check_raw(ctx, "one layer", case, 1, 0.5, surface_T=280.0, I_top=sky_radiance(300))
    L = _native.limit("layers_per_column")
    assert L == 128
    case = hand_made(67, L=L, n=257, scatterers=4, spectral=(0, 3))
    case["k"] *= 1e-2
    case["amount"] *= 1e-2
    check_raw(ctx, "the layer limit", case, 1, spectral_emissivity(257), surface_T=300.0)


def test_beyond_one_round_of_partial_slots(ctx):
    """4,101 tiles over 1,024 slots: a slot takes five tiles, and the last tile holds five points; 4,096 points against the
    restatement, the band values against the device's own spectra"""
    n = 1024 * 256 * 4 + 1029
    j = np.arange(n)
    case = dict(k=np.stack([1e-6 * (1 + (j % 7)), 1e-6 * (1 + ((j + 3) % 7))]), depth=np.array([2e5, 1e5]),
                T=np.array([[288.0, 262.0], [262.0, 231.0]]), linear=True, amount=np.array([[0.3, 1.5]]),
                numbers=[(1.0, 0.6, 0.8)])
    points = np.unique(np.concatenate([[0, 1, 255, 256, n - 1029, n - 6, n - 5, n - 1],
                                       np.random.RandomState(68).randint(0, n, 4096 - 8)]))
    sums, ut, ds, us = check_raw(ctx, "one million points", case, 1, 0.7, surface_T=290.0, points=points)
    scale = ref.scale(grid(n), case["T"], surface_T=290.0)
    allow = TOL * scale.sum()
    assert abs(sums[0, 0, 2] - ut.sum()) <= allow and abs(sums[0, 1, 0] - ds.sum()) <= allow
    assert abs(sums[0, 0, 0] - us.sum()) <= allow


def test_zero_huge_inf_and_nan_coefficients(ctx):
    """single points of 0, 1e300, inf and NaN: a point where some layer's optical depth is not finite has NaN in the spectra
    and counts as 0 in the sums; 1e300 gives finite values; every other point keeps its bits"""
    case = hand_made(69, L=3, scatterers=1)
    k = case["k"]
    k[0, 5], k[1, 6], k[2, 7], k[1, 400] = 0.0, 1e300, np.inf, np.nan
    k[0, 1027], k[2, 1028], k[2, 514] = np.nan, np.inf, 1e300
    bad = [7, 400, 1027, 1028]
    with np.errstate(invalid="ignore"):
        clean = np.where(np.isfinite(k) & (k < 1e299), k, 1e-5)
    kw = dict(e=0.5, surface_T=285.0, I_top=sky_radiance(N))
    sums, *spec = run_raw(ctx, **case, **kw)
    sums2, *spec2 = run_raw(ctx, **dict(case, k=clean), **kw)
    same = np.all(k == clean, axis=0)
    assert same.sum() == N - 6
    for a, b in zip(spec, spec2):
        assert np.all(np.isnan(a[bad])) and np.all(np.isfinite(a[[5, 6, 514]]))
        assert np.array_equal(a[same], b[same])
    assert np.all(np.isfinite(sums))
    allow = TOL * ref.scale(grid(N), case["T"], surface_T=285.0, I_top=sky_radiance(N)).sum()
    for got, v in ((sums[0, 0, 3], spec[0]), (sums[0, 1, 0], spec[1]), (sums[0, 0, 0], spec[2])):
        assert abs(got - np.nansum(v)) <= allow
    # 1e300 against the restatement: the layer is opaque and emits at its edges
    good = np.array([5, 6, 514])
    up, dn = ref.column(k[:, good], case["depth"], grid(N)[good], case["T"], case["amount"], case["numbers"], 1, 0.5,
                        surface_T=285.0, I_top=sky_radiance(N)[good])
    scale = ref.scale(grid(N)[good], case["T"], surface_T=285.0, I_top=sky_radiance(N)[good])
    for got, want in zip(spec, (up[3], dn[0], up[0])):
        assert np.max(np.abs(got[good] - want) / scale) <= TOL


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    L, n = 3, 1027
    k = hand_made(70, L=L, n=n)["k"]
    nv = 2 * (L + 1)
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    tile = ctx.column_flux_scatter_workspace(L, 1)
    level, work = ctx.buffer(nv), ctx.buffer(2 * tile)
    spec = [ctx.buffer(n) for _ in range(3)]
    Is, It, em, ext, ssa, asym = (ctx.buffer(n).upload(np.full(n, v)) for v in (1.1, 0.2, 0.8, 1.5, 0.9, 0.7))
    level_short, n_short, work_short = ctx.buffer(nv - 1), ctx.buffer(n - 1), ctx.buffer(tile - 1)
    i64, f64 = lambda v: (C.c_int64 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    ptrs = lambda v: (C.c_void_p * max(len(v), 1))(*v)
    cmax = _native.limit("scatterers")
    inf, nan = float("inf"), float("nan")
    edges = [290.0, 280.0, 280.0, 260.0, 255.0, 240.0]
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=ptrs([b.h for b in kb]), T=f64(edges), planck_linear=1,
                depth=f64([1e4, 2e4, 1e4]), lo=LO, hi=HI, n=n, I_surface=Is.h, surface_T=0.0, I_top=It.h, n_scat=2,
                scat_amount=f64([0.1, 0.0, 2.0, 1.0, 1.0, 1.0]), scat_ext=ptrs([ext.h, None]), scat_ext_all=f64([0.0, 2.0]),
                scat_ssa=ptrs([ssa.h, None]), scat_ssa_all=f64([0.0, 1.0]), scat_asym=ptrs([asym.h, None]),
                scat_asym_all=f64([0.0, -0.2]), delta_scaling=1, n_bands=1, band_first=i64([0]), band_count=i64([n]),
                emissivity=em.h, emissivity_all=0.5, workspace=work.h, level_flux=level.h, up_top=spec[0].h,
                down_surface=spec[1].h, up_surface=spec[2].h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_flux_scatter_dev(*[a[key] for key in good])

    bad = [  # NULL arrays, negative counts
           dict(abs_coef=None), dict(T=None), dict(depth=None), dict(scat_amount=None), dict(band_first=None),
           dict(band_count=None), dict(level_flux=None), dict(workspace=None),
           dict(n_layers=-1), dict(n=-5), dict(n_scat=-1), dict(n_bands=-1),
           # counts beyond their limits (and too few)
           dict(n_layers=_native.limit("layers_per_column") + 1),
           dict(n_scat=cmax + 1, scat_amount=f64([0.1] * (L * (cmax + 1))), scat_ext=None, scat_ext_all=f64([1.0] * (cmax + 1)),
                scat_ssa=None, scat_ssa_all=f64([1.0] * (cmax + 1)), scat_asym=None, scat_asym_all=f64([0.0] * (cmax + 1))),
           dict(n_bands=0), dict(n_bands=_native.limit("flux_bands") + 1),
           # buffers shorter than they must be
           dict(level_flux=level_short.h), dict(I_surface=n_short.h), dict(I_top=n_short.h), dict(up_top=n_short.h),
           dict(down_surface=n_short.h), dict(up_surface=n_short.h), dict(emissivity=n_short.h),
           dict(abs_coef=ptrs([kb[0].h, n_short.h, kb[2].h])), dict(scat_ext=ptrs([n_short.h, None])),
           dict(scat_ssa=ptrs([ssa.h, n_short.h])), dict(scat_asym=ptrs([n_short.h, None])), dict(workspace=work_short.h),
           # bands
           dict(band_count=i64([n + 1])), dict(band_first=i64([-1])), dict(band_count=i64([0])), dict(band_first=i64([n])),
           # depths
           dict(depth=f64([1e4, -1.0, 1e4])), dict(depth=f64([1e4, nan, 1e4])),
           # the surface source and the temperatures, under both settings
           dict(I_surface=None, surface_T=0.0), dict(I_surface=None, surface_T=-3.0), dict(I_surface=None, surface_T=nan),
           dict(T=f64([290.0, 280.0, 280.0, 0.0, 255.0, 240.0])), dict(T=f64([290.0, 280.0, 280.0, 260.0, -1.0, 240.0])),
           dict(T=f64([nan, 280.0, 280.0, 260.0, 255.0, 240.0])), dict(T=f64([290.0, 280.0, 280.0, 260.0, 255.0, inf])),
           dict(planck_linear=0, T=f64([290.0, 0.0, 250.0])), dict(planck_linear=0, T=f64([290.0, nan, 250.0])),
           dict(planck_linear=0, T=f64([290.0, 270.0, inf])), dict(planck_linear=0, T=f64([-290.0, 270.0, 250.0])),
           dict(planck_linear=2), dict(planck_linear=-1),
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
    everything = kb + outs + [work, Is, It, em, ext, ssa, asym, level_short, n_short, work_short]
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
        assert call(emissivity_all=7.0, surface_T=-1.0, scat_ext_all=f64([-1.0, 2.0]), scat_asym_all=f64([5.0, -0.2])) == 0
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        assert call(scat_ext=None, scat_ext_all=f64([1.5, 2.0]), scat_ssa=None, scat_ssa_all=f64([0.9, 1.0]), scat_asym=None,
                    scat_asym_all=f64([0.7, -0.2])) == 0
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        # what is allowed: no spectra, one emissivity, a dark sky, a surface temperature, no scatterer, the layer source
        assert call(up_top=None, down_surface=None, up_surface=None, emissivity=None, I_top=None) == 0
        assert call(I_surface=None, surface_T=288.0) == 0
        assert call(n_scat=0, scat_amount=None, scat_ext=None, scat_ext_all=None, scat_ssa=None, scat_ssa_all=None,
                    scat_asym=None, scat_asym_all=None) == 0
        assert call(planck_linear=0, T=f64([290.0, 270.0, 250.0]), delta_scaling=0) == 0
        level.download()                                    # (the queue drains without an error)
    finally:
        for b in everything:
            b.free()


# ---- 5. the model ---------------------------------------------------------------------------------------------------------
def model_scale(pyrad, atm, surface_T, levels=None):
    x = atm[0].xAxis
    temps = [Ly.T for Ly in atm] + ([] if levels is None else list(levels))
    return ref.scale(x, temps, surface_T=surface_T)


@pytest.mark.parametrize("planck", ("layer", "linear"))
def test_model_without_scatterers_is_fluxes(pyrad, lines, planck):
    from pyrad_amd import settings
    atm = column(pyrad)
    x = atm[0].xAxis
    n = x.size
    bands = [(600, 640), (640, 701)]
    kw = dict(surfaceTemperature=290.0, topSpectrum=ref.planck(x, 150.0), planck=planck, bands=bands, spectra=True)
    two = atm.fluxesTwoStream(**kw)
    one = atm.fluxes(angles=[(MU, W)], emissivity=1.0, **kw)
    scale = np.maximum(model_scale(pyrad, atm, 290.0, atm.levelTemperatures()), np.pi * ref.planck(x, 150.0))
    res = settings.BASE_RESOLUTION
    idx = [(int(np.searchsorted(x, lo)), int(np.searchsorted(x, hi))) for lo, hi in bands]
    for b, (lo, hi) in enumerate(idx):
        allow = TOL * scale[lo:hi].sum() * res
        print("band %d: up %.2e, down %.2e of the allowance" % (
            b, np.max(np.abs(two.up[b] - one.up[b])) / allow, np.max(np.abs(two.down[b] - one.down[b])) / allow))
        assert np.max(np.abs(two.up[b] - one.up[b])) <= allow and np.max(np.abs(two.down[b] - one.down[b])) <= allow
    for a, b in ((two.upSpectrum, one.upSpectrum), (two.downSpectrum, one.downSpectrum),
                 (two.upSurfaceSpectrum, one.upSurfaceSpectrum)):
        assert np.max(np.abs(a - b) / scale) <= TOL
    assert list(two.mu) == [MU] and list(two.weight) == [W]
    assert two.up.shape == two.down.shape == two.net.shape == (2, len(atm) + 1) and two.heatingRate.shape == (2, len(atm))
    assert np.array_equal(two.net, two.up - two.down)
    assert np.array_equal(two.heatingRate, pyrad.heatingRates(two.net, [L.P for L in atm], [L.T for L in atm],
                                                              [L.depth for L in atm]))
    whole = atm.fluxesTwoStream(surfaceTemperature=290.0, topSpectrum=kw["topSpectrum"], planck=planck, spectra=True)
    assert whole.up.shape == (len(atm) + 1,)
    allow = TOL * scale.sum() * res
    assert np.max(np.abs(whole.up - two.up.sum(axis=0))) <= allow and np.max(np.abs(whole.down - two.down.sum(axis=0))) <= allow
    assert abs(whole.up[-1] - res * whole.upSpectrum.sum()) <= allow and abs(whole.down[0] - res * whole.downSpectrum.sum()) <= allow


@pytest.mark.parametrize("planck", ("layer", "linear"))
def test_model_a_grey_cloud_in_the_top_layer(pyrad, lines, planck):
    """a cloud over a column with a lapse rate is colder than what it hides: less leaves at the top, more comes down"""
    atm = column(pyrad)
    cloud = pyrad.Scatterer([0.0, 0.0, 0.0, 5.0], extinction=1.0, singleScatteringAlbedo=0.5, asymmetry=0.85, name="cloud")
    clear = atm.fluxesTwoStream(surfaceTemperature=288.0, planck=planck)
    cloudy = atm.fluxesTwoStream([cloud], surfaceTemperature=288.0, planck=planck, spectra=True)
    print("%s: up at the top %.4f -> %.4f, down at the surface %.4f -> %.4f W m^-2" % (
        planck, clear.up[-1], cloudy.up[-1], clear.down[0], cloudy.down[0]))
    assert cloudy.up[-1] < clear.up[-1] and cloudy.down[0] > clear.down[0]
    assert cloudy.down[-1] == 0.0 and np.all(np.isfinite(cloudy.heatingRate))
    again = atm.fluxesTwoStream([cloud], surfaceTemperature=288.0, planck=planck, spectra=True)      # the kept state is sound
    for a, b in ((again.up, cloudy.up), (again.down, cloudy.down), (again.upSpectrum, cloudy.upSpectrum),
                 (again.downSpectrum, cloudy.downSpectrum), (again.upSurfaceSpectrum, cloudy.upSurfaceSpectrum)):
        assert np.array_equal(a, b)
    # the restatement on the model's own absorption coefficients
    x = atm[0].xAxis
    k = np.array([np.array(pyrad.getAbsCoef(Ly)) for Ly in atm])
    lev = atm.levelTemperatures()
    edges = np.column_stack([lev[:-1], lev[1:]]) if planck == "linear" else np.column_stack([[Ly.T for Ly in atm]] * 2)
    up, dn = ref.column(k, [Ly.depth for Ly in atm], x, edges, [cloud.amounts], [(1.0, 0.5, 0.85)], 1, 1.0, surface_T=288.0)
    scale = model_scale(pyrad, atm, 288.0, lev)
    for got, want in ((cloudy.upSpectrum, up[-1]), (cloudy.downSpectrum, dn[0]), (cloudy.upSurfaceSpectrum, up[0])):
        assert np.max(np.abs(got - want) / scale) <= TOL
