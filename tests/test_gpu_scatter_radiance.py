"""GPU: radiances through scattering layers (lbl_column_radiance_scatter_dev, kernels K5n; Atmosphere.radianceTwoStream)
against the float64 NumPy restatement of tests/scatter_radiance_ref.py - its own grouping of the closed form, on the level
fluxes of scatter_flux_ref, which solves the column in the other order than the kernels - on hand-made coefficients through
the raw C ABI; the three identities (the two-stream angle, no scatterers, the cavity), the crossing of lam mu = 1, equal
edges, the independence of a view from its neighbours, the pass size, two runs, the edge shapes, odd coefficients and the
refusals; and through the model.

Tolerance: absolute, 1e-12 in units of the point's scale / pi - the largest of the Planck values and boundary radiances that
enter it.  No point is left out: the closed form has no pole at lam mu = 1.  The restatement itself stays inside 1e-13 of 50
digits in every regime (tests/test_scatter_radiance_cpu.py measures 4e-16, near-conservative layers included), so no regime
needs a wider bound."""
import ctypes as C

import numpy as np
import pytest

import scatter_flux_ref as flux
import scatter_radiance_ref as ref
import twostream_ref as two
from test_gpu_flux import column, lines, pyrad  # noqa: F401
from test_gpu_scatter_flux import CASES, LO, HI, edges_of, grid, hand_made, sky_radiance, spectral_emissivity, surface_radiance
from test_gpu_scatter_flux import run_raw as run_flux

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
TOL = 1e-12
N, L4 = 1029, 4
MU3 = 1.0 / np.sqrt(3.0)
VIEWS = [(1.0, 0), (0.5, 0), (MU3, 0), (0.2, 1), (1.0, 1)]


@pytest.fixture()
def ctx(pyrad):
    from pyrad_amd import engine
    return engine.get_engine().ctx


def run_raw(ctx, k, depth, T, linear, views, amount=(), numbers=(), delta=1, e=1.0, surface_T=0.0, I_surface=None, I_top=None,
            spectra=True, passes=None):
    """lbl_column_radiance_scatter_dev on uploaded coefficients: (radiance (V, n), up_top, down_surface).
    ``passes``: None - a workspace for the whole grid; else the points of a pass (rounded up to whole tiles)"""
    k = np.asarray(k, dtype=np.float64)
    L, n = k.shape
    V = len(views)
    bufs = [ctx.buffer(max(n, 1)).upload(k[l]) for l in range(L)]
    rad = ctx.buffer(V * n)
    work = ctx.buffer(ctx.column_radiance_scatter_workspace(L, n if passes is None else passes))
    spec = [ctx.buffer(n) for _ in range(2)] if spectra else [None] * 2
    bufs += [rad, work] + [b for b in spec if b is not None]
    try:
        def dev(v):
            if v is None or np.ndim(v) == 0:
                return v if v is None else float(v)
            bufs.append(ctx.buffer(n).upload(np.asarray(v, dtype=np.float64)))
            return bufs[-1]
        cols = [[dev(v) for v in triple] for triple in numbers]
        ctx.column_radiance_scatter_dev(bufs[:L], T, int(linear), depth, LO, HI, n, amount, [c[0] for c in cols],
                                        [c[1] for c in cols], [c[2] for c in cols], delta, [m for m, _ in views],
                                        [d for _, d in views], work, rad, emissivity=dev(e), I_surface=dev(I_surface),
                                        surface_T=surface_T, I_top=dev(I_top), up_top=spec[0], down_surface=spec[1])
        return (rad.download(V * n).reshape(V, n),) + tuple(b.download(n) if b is not None else None for b in spec)
    finally:
        for b in bufs:
            b.free()


def restated(case, views, delta=1, e=1.0, surface_T=0.0, I_surface=None, I_top=None, at=None):
    """the restatement of a case at the points ``at`` (None: all): (radiance (V, m), up, dn, scale / pi (m,))"""
    L, n = case["k"].shape
    at = np.arange(n) if at is None else np.asarray(at)
    pick = lambda v: v if v is None or np.ndim(v) == 0 else np.asarray(v)[at]
    numbers = [tuple(pick(v) for v in triple) for triple in case["numbers"]]
    nu = grid(n)[at]
    want, up, dn = ref.radiance(case["k"][:, at], case["depth"], nu, edges_of(case), views, case["amount"], numbers, delta,
                                pick(e), pick(I_surface), surface_T or None, pick(I_top))
    scale = flux.scale(nu, edges_of(case), pick(I_surface), surface_T or None, pick(I_top)) / np.pi
    return want, up, dn, scale


def check_raw(ctx, name, case, views=VIEWS, delta=1, e=1.0, surface_T=0.0, I_surface=None, I_top=None, **kw):
    got, ut, ds = run_raw(ctx, views=views, delta=delta, e=e, surface_T=surface_T, I_surface=I_surface, I_top=I_top, **case, **kw)
    want, up, dn, scale = restated(case, views, delta, e, surface_T, I_surface, I_top)
    assert np.all(np.isfinite(got))
    worst = np.max(np.abs(got - want) / scale, axis=1)
    flux_err = max(np.max(np.abs(ut - up[-1]) / scale), np.max(np.abs(ds - dn[0]) / scale)) / np.pi
    print("%s: views %s of the scale, the fluxes %.2e" % (name, " ".join("%.2e" % w for w in worst), flux_err))
    assert worst.max() <= TOL and flux_err <= TOL
    return got, ut, ds


def case_kw(name):
    make, delta, e, surface, top, _ = CASES[name]
    if isinstance(e, str):
        e = spectral_emissivity(N)
    return hand_made(**make), dict(delta=delta, e=e, surface_T=291.5 if surface == "T" else 0.0,
                                   I_surface=surface_radiance(N) if surface == "I" else None,
                                   I_top=sky_radiance(N) if top else None)


# ---- 1. against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(ctx, name):
    case, kw = case_kw(name)
    check_raw(ctx, name, case, **kw)


# ---- 2. the identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_at_the_two_stream_angle_the_radiance_is_the_flux(ctx, name):
    """mu = 1 / sqrt(3): pi Iu_L == up_L and pi Id_0 == dn_0 of the call's own spectra, which are K5m's bit for bit"""
    case, kw = case_kw(name)
    got, ut, ds = run_raw(ctx, views=[(MU3, 0), (MU3, 1)], **case, **kw)
    scale = flux.scale(grid(N), edges_of(case), kw["I_surface"], kw["surface_T"] or None, kw["I_top"])
    err = max(np.max(np.abs(np.pi * got[0] - ut) / scale), np.max(np.abs(np.pi * got[1] - ds) / scale))
    print("%s: pi I at 1 / sqrt(3) within %.2e of the scale of the call's fluxes" % (name, err))
    assert err <= TOL
    _, f_ut, f_ds, _ = run_flux(ctx, **case, **kw)
    assert np.array_equal(ut, f_ut) and np.array_equal(ds, f_ds)


@pytest.mark.parametrize("linear", (False, True))
def test_no_scatterers_is_the_ray_call(ctx, linear):
    """n_scat = 0: lbl_ray_radiance_surface_dev (_linear_dev) along the same cosines, the up rays from the Lambertian
    surface under the call's own downward flux, the down rays from cold space - to the tolerance, not bit for bit"""
    case = hand_made(62, linear=linear)
    e = spectral_emissivity(N)
    got, ut, ds = run_raw(ctx, views=VIEWS, e=e, surface_T=295.0, **case)
    depth = case["depth"]
    first, seg_layer, seg_len, seg_T, kind = [0], [], [], [], []
    edges = edges_of(case)
    for mu, down in VIEWS:
        order = range(L4 - 1, -1, -1) if down else range(L4)
        seg_layer += list(order)
        seg_len += [depth[l] / mu for l in order]
        seg_T += [(edges[l, 1], edges[l, 0]) if down else (edges[l, 0], edges[l, 1]) for l in order]
        first.append(len(seg_layer))
        kind.append(0 if down else 1)
    bufs = [ctx.buffer(N).upload(case["k"][l]) for l in range(L4)]
    out, eb, db = ctx.buffer(len(VIEWS) * N), ctx.buffer(N).upload(e), ctx.buffer(N).upload(ds)
    try:
        if linear:
            ctx.ray_radiance_linear_dev(bufs, seg_T, LO, HI, N, first, seg_layer, seg_len, kind, out, emissivity=eb,
                                        source_T=295.0, surface_down=db, surface_down_norm=np.pi)
        else:
            ctx.ray_radiance_surface_dev(bufs, case["T"], LO, HI, N, first, seg_layer, seg_len, kind, out, eb,
                                         source_T=295.0, surface_down=db, surface_down_norm=np.pi)
        other = out.download(len(VIEWS) * N).reshape(len(VIEWS), N)
    finally:
        for b in bufs + [out, eb, db]:
            b.free()
    scale = flux.scale(grid(N), edges, surface_T=295.0) / np.pi
    worst = np.max(np.abs(got - other) / scale)
    print("no scatterers, %s: within %.2e of the scale of the ray call" % ("linear" if linear else "layer", worst))
    assert worst <= TOL


@pytest.mark.parametrize("linear", (False, True))
def test_kirchhoff_cavity(ctx, linear):
    """one temperature everywhere, the sky included: I = B(T0) in every view"""
    T0 = 255.0
    case = hand_made(63, linear=linear, scatterers=4, spectral=(0, 3))
    case["T"] = np.full_like(case["T"], T0)
    B = flux.planck(grid(N), T0)
    for e in (0.0, 0.3, spectral_emissivity(N)):
        for delta in (0, 1):
            got, ut, ds = run_raw(ctx, views=VIEWS, delta=delta, e=e, surface_T=T0, I_top=B, **case)
            worst = np.max(np.abs(got / B - 1.0))
            print("cavity: every view within %.2e of B" % worst)
            assert worst <= TOL


def test_through_lam_mu_equal_to_one(ctx):
    """a view with mu = 1 / lam of point 500, layer 1, of a case whose lam varies over the grid from below to above 1 / mu:
    every point is compared, none is left out, and the values run smoothly through the crossing"""
    case = hand_made(71, scatterers=1, spectral=(0,))
    j = np.arange(N)
    case["k"][1] = 10.0 ** (-5.3 + 3.0 * j / N)             # the gas of layer 1: optical depth 0.05 .. 50, rising
    case["numbers"] = [(np.full(N, 1.0), np.full(N, 0.8), np.full(N, 0.5))]
    case["amount"] = np.array([[0.5, 1.0, 2.0, 0.1]])
    ta, ts, tsg = two.optical(case["k"], case["depth"], case["amount"], case["numbers"], 1)
    t = ta + ts
    lam = np.sqrt((ref.D * (ta / t)) * (ref.D * ((t - tsg) / t)))
    mu0 = float(1.0 / lam[1, 500])
    assert 0.0 < mu0 <= 1.0 and np.any(lam[1] * mu0 < 1 - 1e-3) and np.any(lam[1] * mu0 > 1 + 1e-3)
    assert (1.0 - lam[1, 500] * mu0) * t[1, 500] / mu0 == 0.0 or abs(1.0 - lam[1, 500] * mu0) <= 2.3e-16
    views = [(mu0, 0), (mu0, 1), (mu0 * (1 - 1e-9), 0), (min(mu0 * (1 + 1e-9), 1.0), 1)]
    check_raw(ctx, "lam mu = 1 at point 500", case, views=views, e=0.4, surface_T=290.0, I_top=sky_radiance(N))


def test_equal_edges_are_the_layer_source_bit_for_bit(ctx):
    case = hand_made(61, linear=False, scatterers=3, spectral=(1,))
    kw = dict(views=VIEWS, e=spectral_emissivity(N), surface_T=288.0, I_top=sky_radiance(N))
    layer = run_raw(ctx, **case, **kw)
    linear = run_raw(ctx, **dict(case, T=np.repeat(case["T"], 2), linear=True), **kw)
    for a, b in zip(layer, linear):
        assert np.array_equal(a, b)


def test_a_view_does_not_depend_on_the_other_views(ctx):
    """the same bits alone, among 16 views, and in another position of the list"""
    case = hand_made(72, scatterers=2, spectral=(0,))
    kw = dict(e=0.4, surface_T=290.0, I_top=sky_radiance(N))
    rs = np.random.RandomState(73)
    many = [(float(m), int(d)) for m, d in zip(rs.uniform(0.05, 1.0, 16), rs.randint(0, 2, 16))]
    many[3], many[11] = (0.37, 0), (0.37, 1)
    full = run_raw(ctx, views=many, **case, **kw)[0]
    for v in (3, 11, 15):
        alone = run_raw(ctx, views=[many[v]], **case, **kw)[0]
        assert np.array_equal(alone[0], full[v])
    moved = run_raw(ctx, views=[many[11], many[0], many[3]], **case, **kw)[0]
    assert np.array_equal(moved[0], full[11]) and np.array_equal(moved[1], full[0]) and np.array_equal(moved[2], full[3])


def test_the_pass_size_does_not_change_a_bit_and_two_runs_agree(ctx):
    case = hand_made(64, scatterers=2, spectral=(0,))
    kw = dict(views=VIEWS, e=0.4, surface_T=290.0, I_top=sky_radiance(N))
    whole = run_raw(ctx, **case, **kw)
    for other in (run_raw(ctx, passes=1, **case, **kw), run_raw(ctx, passes=300, **case, **kw), run_raw(ctx, **case, **kw)):
        for a, b in zip(whole, other):
            assert np.array_equal(a, b)


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------
def test_without_layers_one_layer_and_the_layer_limit(ctx):
    from pyrad_amd import _native
    # L = 0: an up view sees the surface's up_0 / pi, a down view the sky
    for linear in (0, 1):
        got, ut, ds = run_raw(ctx, np.zeros((0, 3)), [], [], linear, [(0.3, 0), (1.0, 1), (0.7, 0)], e=0.6,
                              I_surface=[2.0, 1.0, 0.5], I_top=[0.5, 0.25, 4.0])
        assert np.array_equal(got[1], [0.5, 0.25, 4.0]) and np.array_equal(got[0], ut / np.pi) and np.array_equal(got[2], got[0])
        assert np.array_equal(ds, np.pi * np.array([0.5, 0.25, 4.0]))
        assert np.max(np.abs(got[0] - (0.6 * np.array([2.0, 1.0, 0.5]) + 0.4 * np.array([0.5, 0.25, 4.0])))) <= 4e-15
    for linear in (False, True):
        case = hand_made(66, L=1, n=300, scatterers=2, spectral=(1,), linear=linear)
        check_raw(ctx, "one layer", case, e=0.5, surface_T=280.0, I_top=sky_radiance(300))
    L = _native.limit("layers_per_column")
    assert L == 128 and _native.limit("scatter_views") == 16
    case = hand_made(67, L=L, n=257, scatterers=4, spectral=(0, 3))
    case["k"] *= 1e-2
    case["amount"] *= 1e-2
    rs = np.random.RandomState(74)
    views = [(float(m), int(d)) for m, d in zip(rs.uniform(0.05, 1.0, 16), rs.randint(0, 2, 16))]
    check_raw(ctx, "the layer limit, 16 views", case, views=views, e=spectral_emissivity(257), surface_T=300.0,
              I_top=sky_radiance(257))


def test_zero_huge_inf_and_nan_coefficients(ctx):
    """single points of 0, 1e300, inf and NaN: a point where some layer's optical depth is not finite is NaN in every
    output; 1e300 gives finite values, against the restatement; every other point keeps its bits"""
    case = hand_made(69, L=3, scatterers=1)
    k = case["k"]
    k[0, 5], k[1, 6], k[2, 7], k[1, 400] = 0.0, 1e300, np.inf, np.nan
    k[0, 1027], k[2, 1028], k[2, 514] = np.nan, np.inf, 1e300
    bad = [7, 400, 1027, 1028]
    with np.errstate(invalid="ignore"):
        clean = np.where(np.isfinite(k) & (k < 1e299), k, 1e-5)
    kw = dict(views=VIEWS, e=0.5, surface_T=285.0, I_top=sky_radiance(N))
    got = run_raw(ctx, **case, **kw)
    got2 = run_raw(ctx, **dict(case, k=clean), **kw)
    same = np.all(k == clean, axis=0)
    assert same.sum() == N - 6
    for a, b in zip(got, got2):
        a, b = np.atleast_2d(a), np.atleast_2d(b)
        assert np.all(np.isnan(a[:, bad])) and np.all(np.isfinite(a[:, [5, 6, 514]]))
        assert np.array_equal(a[:, same], b[:, same])
    good = np.array([5, 6, 514])
    want, up, dn, scale = restated(case, VIEWS, 1, 0.5, 285.0, None, sky_radiance(N), at=good)
    assert np.max(np.abs(got[0][:, good] - want) / scale) <= TOL


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    L, n, V = 3, 1027, 3
    k = hand_made(70, L=L, n=n)["k"]
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    tile = ctx.column_radiance_scatter_workspace(L, 1)
    rad, work = ctx.buffer(V * n), ctx.buffer(2 * tile)
    spec = [ctx.buffer(n) for _ in range(2)]
    Is, It, em, ext, ssa, asym = (ctx.buffer(n).upload(np.full(n, v)) for v in (1.1, 0.2, 0.8, 1.5, 0.9, 0.7))
    rad_short, n_short, work_short = ctx.buffer(V * n - 1), ctx.buffer(n - 1), ctx.buffer(tile - 1)
    f64 = lambda v: (C.c_double * max(len(v), 1))(*v)
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    ptrs = lambda v: (C.c_void_p * max(len(v), 1))(*v)
    cmax, vmax = _native.limit("scatterers"), _native.limit("scatter_views")
    inf, nan = float("inf"), float("nan")
    edges = [290.0, 280.0, 280.0, 260.0, 255.0, 240.0]
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=ptrs([b.h for b in kb]), T=f64(edges), planck_linear=1,
                depth=f64([1e4, 2e4, 1e4]), lo=LO, hi=HI, n=n, I_surface=Is.h, surface_T=0.0, I_top=It.h, n_scat=2,
                scat_amount=f64([0.1, 0.0, 2.0, 1.0, 1.0, 1.0]), scat_ext=ptrs([ext.h, None]), scat_ext_all=f64([0.0, 2.0]),
                scat_ssa=ptrs([ssa.h, None]), scat_ssa_all=f64([0.0, 1.0]), scat_asym=ptrs([asym.h, None]),
                scat_asym_all=f64([0.0, -0.2]), delta_scaling=1, emissivity=em.h, emissivity_all=0.5, n_views=V,
                view_mu=f64([1.0, 0.5, 0.2]), view_down=i32([0, 1, 0]), workspace=work.h, radiance=rad.h, up_top=spec[0].h,
                down_surface=spec[1].h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_radiance_scatter_dev(*[a[key] for key in good])

    bad = [  # NULL arrays, negative counts
           dict(abs_coef=None), dict(T=None), dict(depth=None), dict(scat_amount=None), dict(radiance=None),
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
           dict(radiance=rad_short.h), dict(I_surface=n_short.h), dict(I_top=n_short.h), dict(up_top=n_short.h),
           dict(down_surface=n_short.h), dict(emissivity=n_short.h),
           dict(abs_coef=ptrs([kb[0].h, n_short.h, kb[2].h])), dict(scat_ext=ptrs([n_short.h, None])),
           dict(scat_ssa=ptrs([ssa.h, n_short.h])), dict(scat_asym=ptrs([n_short.h, None])), dict(workspace=work_short.h),
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
    outs = [rad] + spec
    everything = kb + outs + [work, Is, It, em, ext, ssa, asym, rad_short, n_short, work_short]
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
        # what is allowed: no spectra, one emissivity, a dark sky, a surface temperature, no scatterer, the layer source, and
        # the view limit itself
        assert call() == 0
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        assert call(up_top=None, down_surface=None, emissivity=None, I_top=None) == 0
        assert call(I_surface=None, surface_T=288.0) == 0
        assert call(n_scat=0, scat_amount=None, scat_ext=None, scat_ext_all=None, scat_ssa=None, scat_ssa_all=None,
                    scat_asym=None, scat_asym_all=None) == 0
        assert call(planck_linear=0, T=f64([290.0, 270.0, 250.0]), delta_scaling=0) == 0
        wide = ctx.buffer(vmax * n)
        everything.append(wide)
        assert call(n_views=vmax, view_mu=f64([0.5] * vmax), view_down=i32([0, 1] * (vmax // 2)), radiance=wide.h) == 0
        wide.download()                                     # (the queue drains without an error)
    finally:
        for b in everything:
            b.free()


# ---- 5. the model ---------------------------------------------------------------------------------------------------------
def model_scale(atm, surface_T, levels=None):
    x = atm[0].xAxis
    temps = [Ly.T for Ly in atm] + ([] if levels is None else list(levels))
    return flux.scale(x, temps, surface_T=surface_T) / np.pi


@pytest.mark.parametrize("planck", ("layer", "linear"))
def test_model_without_scatterers_is_radiance_and_observe(pyrad, lines, planck):
    atm = column(pyrad)
    lev = atm.levelTemperatures() if planck == "linear" else None
    views = [1.0, (0.6, "up"), (0.6, "down"), (1.0, "down")]
    got = atm.radianceTwoStream(views, surfaceTemperature=290.0, planck=planck)
    assert got.radiance.shape == (4, atm[0].xAxis.size) and list(got.direction) == ["up", "up", "down", "down"]
    assert list(got.mu) == [1.0, 0.6, 0.6, 1.0] and np.array_equal(got.wavenumber, atm[0].xAxis)
    paths = [atm.nadirPath(1.0, levelTemperatures=lev), atm.nadirPath(0.6, levelTemperatures=lev),
             atm.zenithPath(0.6, levelTemperatures=lev), atm.zenithPath(1.0, levelTemperatures=lev)]
    one = atm.radiance(paths, surfaceTemperature=290.0, planck=planck)
    scale = model_scale(atm, 290.0, lev)
    worst = np.max(np.abs(got.radiance - one.radiance) / scale)
    print("%s: radianceTwoStream without scatterers within %.2e of the scale of radiance()" % (planck, worst))
    assert worst <= TOL
    if planck == "layer":
        ins = pyrad.Instrument(np.arange(610.0, 690.0, 0.5), width=0.5)
        ch = atm.radianceTwoStream([0.6], surfaceTemperature=290.0, instrument=ins)
        obs = atm.observe(ins, surfaceTemperature=290.0, mu=0.6)
        assert ch.radiance.shape == (1, len(ins)) and np.array_equal(ch.wavenumber, ins.centres)
        assert np.max(np.abs(ch.radiance[0] - obs.radiance) / np.max(scale)) <= TOL


def test_model_chunks_of_views_and_an_instrument(pyrad, lines):
    """17 views equal the same views in separate calls bit for bit; the channels are convolve() of the spectral result"""
    atm = column(pyrad)
    cloud = pyrad.Scatterer([0.0, 0.0, 2.0, 0.0], extinction=1.0, singleScatteringAlbedo=0.9, asymmetry=0.8, name="cloud")
    rs = np.random.RandomState(75)
    views = [(float(m), "down" if d else "up") for m, d in zip(rs.uniform(0.1, 1.0, 17), rs.randint(0, 2, 17))]
    kw = dict(scatterers=[cloud, pyrad.rayleighScatterer(atm)], surfaceTemperature=288.0, emissivity=0.9, planck="linear")
    full = atm.radianceTwoStream(views, **kw)
    assert full.radiance.shape == (17, atm[0].xAxis.size) and np.all(np.isfinite(full.radiance))
    for v in (0, 15, 16):
        alone = atm.radianceTwoStream([views[v]], **kw)
        assert np.array_equal(alone.radiance[0], full.radiance[v])
    ins = pyrad.Instrument(np.arange(610.0, 690.0, 0.5), width=0.5)
    ch = atm.radianceTwoStream(views, instrument=ins, **kw)
    first = atm[0]
    assert np.array_equal(ch.radiance, pyrad.convolve(ins, full.radiance, first.rangeMin, first.rangeMax))
    assert np.all(pyrad.brightnessTemperature(ch.wavenumber, ch.radiance) > 100.0)


@pytest.mark.parametrize("planck", ("layer", "linear"))
def test_model_a_grey_cloud_in_the_top_layer(pyrad, lines, planck):
    """a cloud over a column with a lapse rate is colder than what it hides: the nadir brightness temperature of a window
    channel falls, and the zenith radiance at the surface rises; the restatement on the model's own coefficients"""
    atm = column(pyrad)
    cloud = pyrad.Scatterer([0.0, 0.0, 0.0, 5.0], extinction=1.0, singleScatteringAlbedo=0.5, asymmetry=0.85, name="cloud")
    views = [(1.0, "up"), (1.0, "down"), (0.4, "up"), (0.4, "down")]
    clear = atm.radianceTwoStream(views, surfaceTemperature=288.0, planck=planck)
    cloudy = atm.radianceTwoStream(views, [cloud], surfaceTemperature=288.0, planck=planck)
    x = atm[0].xAxis
    k = np.array([np.array(pyrad.getAbsCoef(Ly)) for Ly in atm])
    window = int(np.argmin(k.sum(axis=0)))                 # the most transparent point of the grid
    Tb_clear = pyrad.brightnessTemperature(x[window], clear.radiance[0, window])
    Tb_cloudy = pyrad.brightnessTemperature(x[window], cloudy.radiance[0, window])
    print("%s: window at %.2f cm^-1, nadir brightness temperature %.2f -> %.2f K, zenith radiance %.4g -> %.4g" % (
        planck, x[window], Tb_clear, Tb_cloudy, clear.radiance[1, window], cloudy.radiance[1, window]))
    assert Tb_cloudy < Tb_clear - 1.0 and cloudy.radiance[1, window] > clear.radiance[1, window]
    again = atm.radianceTwoStream(views, [cloud], surfaceTemperature=288.0, planck=planck)        # the kept state is sound
    assert np.array_equal(again.radiance, cloudy.radiance)
    lev = atm.levelTemperatures()
    edges = np.column_stack([lev[:-1], lev[1:]]) if planck == "linear" else np.column_stack([[Ly.T for Ly in atm]] * 2)
    want, _, _ = ref.radiance(k, [Ly.depth for Ly in atm], x, edges, [(m, int(d == "down")) for m, d in views],
                              [cloud.amounts], [(1.0, 0.5, 0.85)], 1, 1.0, surface_T=288.0)
    scale = model_scale(atm, 288.0, lev)
    worst = np.max(np.abs(cloudy.radiance - want) / scale)
    print("%s: the model within %.2e of the scale of the restatement" % (planck, worst))
    assert worst <= TOL
