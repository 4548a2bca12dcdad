"""GPU: Jacobians of the outgoing flux through scattering layers (lbl_column_jacobian_scatter_dev, kernels K5p;
Atmosphere.jacobiansTwoStream) against the float64 NumPy restatement of tests/scatter_jacobian_ref.py - layer partials by the
quotient rule, the column's derivative from the adjoint of the dense level system - on hand-made coefficients through the raw
C ABI; the forward bits, the identities (no scatterers, equal edges, the Kirchhoff cavity, additivity, the pass size, two
runs), the edge shapes, odd coefficients and the refusals; and through the model.

Tolerance: absolute, TOL in units of the point's scale (scatter_flux_ref.scale) for F, dF/de and every logarithmic
derivative, and of pi times the largest dB/dT that enters the point for the temperature rows; for band values summed over
the band's points.  TOL is four times the worst distance from the restatement measured on the device over this file's cases
(DESIGN.md "K5p"); the restatement itself stays inside 3.4e-15 of 50 digits (tests/test_scatter_jacobian_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import scatter_flux_ref as flux
import scatter_jacobian_ref as ref
from test_gpu_flux import column, lines, pyrad  # noqa: F401
from test_gpu_linear_jacobian import voigt_model  # noqa: F401
from test_gpu_scatter_flux import (BANDS, CASES, HI, L4, LO, MU, N, W, edges_of, grid, hand_made, sky_radiance,
                                   spectral_emissivity, surface_radiance)
from test_gpu_scatter_flux import run_raw as run_flux

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
MEASURED = 1.21e-15   # the worst of this file's comparisons with the restatement on the device
TOL = 4 * MEASURED


@pytest.fixture()
def ctx(pyrad):
    from pyrad_amd import engine
    return engine.get_engine().ctx


def unit_T(nu, edges, surface_T):
    """pi times the largest dB/dT that enters a point (n,)"""
    temps = list(np.unique(np.asarray(edges, dtype=np.float64))) + ([surface_T] if surface_T else [])
    return np.pi * np.max([ref.planck_dT(nu, T) for T in temps], axis=0)


def terms_of(case, seed, per_layer=2):
    """per_layer terms of every layer but the first, each a fraction of the layer's k, listed layer-descending then again
    ascending (not sorted): (terms (M, n), term_layer)"""
    rs = np.random.RandomState(seed)
    L = case["k"].shape[0]
    layers = [l for i in range(per_layer) for l in (range(L - 1, 0, -1) if i % 2 == 0 else range(1, L))]
    return np.array([rs.uniform(0.05, 0.6) * case["k"][l] for l in layers]).reshape(len(layers), -1), layers


def row_layout(L, NT, Cn, M):
    """the slices of jac's rows: tau, T, scat, term"""
    a = 3 + L
    b = a + NT * L
    c = b + Cn * L
    return slice(3, a), slice(a, b), slice(b, c), slice(c, c + M)


def run_raw(ctx, k, depth, T, linear, amount=(), numbers=(), delta=1, e=1.0, surface_T=0.0, I_surface=None, I_top=None,
            bands=None, spectra=True, passes=None, terms=(), term_layer=()):
    """lbl_column_jacobian_scatter_dev on uploaded coefficients: (jac [band, row], ln tau spectra (L, n), T spectra (NT L,
    n), up_top).  ``passes``: None - a workspace for the widest band; else the points of a pass"""
    k = np.asarray(k, dtype=np.float64)
    L, n = k.shape
    NT = 2 if linear else 1
    first, count = ([0], [n]) if bands is None else ([a for a, _ in bands], [b - a for a, b in bands])
    nb = len(first)
    nv = 3 + (1 + NT + len(numbers)) * L + len(terms)
    bufs = [ctx.buffer(max(n, 1)).upload(k[l]) for l in range(L)]
    tb = [ctx.buffer(n).upload(np.asarray(t, dtype=np.float64)) for t in terms]
    jac = ctx.buffer(nb * nv)
    work = ctx.buffer(ctx.column_jacobian_scatter_workspace(L, max(count) if passes is None else passes))
    spec = [ctx.buffer(max(L * n, 1)), ctx.buffer(max(NT * L * n, 1)), ctx.buffer(max(n, 1))] if spectra else [None] * 3
    bufs += tb + [jac, work] + [b for b in spec if b is not None]
    try:
        def dev(v):
            if v is None or np.ndim(v) == 0:
                return v if v is None else float(v)
            bufs.append(ctx.buffer(n).upload(np.asarray(v, dtype=np.float64)))
            return bufs[-1]
        cols = [[dev(v) for v in triple] for triple in numbers]
        ctx.column_jacobian_scatter_dev(bufs[:L], T, int(linear), depth, LO, HI, n, amount, [c[0] for c in cols],
                                        [c[1] for c in cols], [c[2] for c in cols], delta, first, count, work, jac,
                                        emissivity=dev(e), I_surface=dev(I_surface), surface_T=surface_T, I_top=dev(I_top),
                                        term_abs_coef=tb, term_layer=term_layer, ln_tau_spectra=spec[0], T_spectra=spec[1],
                                        up_top=spec[2])
        out = [jac.download(nb * nv).reshape(nb, nv)]
        if spectra:
            out += [spec[0].download(L * n).reshape(L, n), spec[1].download(NT * L * n).reshape(NT * L, n), spec[2].download(n)]
        else:
            out += [None] * 3
        return tuple(out)
    finally:
        for b in bufs:
            b.free()


def check_raw(ctx, name, case, delta=1, e=1.0, surface_T=0.0, I_surface=None, I_top=None, bands=None, points=None, **kw):
    """a run against the restatement, at every point or, with ``points``, at those (the band values are then not compared);
    returns the run and prints the worst distances in units of TOL"""
    L, n = case["k"].shape
    linear = case["linear"]
    NT = 2 if linear else 1
    terms, term_layer = kw.get("terms", ()), kw.get("term_layer", ())
    jac, tau_s, T_s, ut = run_raw(ctx, delta=delta, e=e, surface_T=surface_T, I_surface=I_surface, I_top=I_top, bands=bands,
                                  **case, **kw)
    at = np.arange(n) if points is None else points
    pick = lambda v: v if v is None or np.ndim(v) == 0 else np.asarray(v)[at]
    numbers = [tuple(pick(v) for v in triple) for triple in case["numbers"]]
    nu = grid(n)[at]
    J = ref.jacobian(case["k"][:, at], case["depth"], nu, edges_of(case), linear, case["amount"], numbers, delta, pick(e),
                     I_surface=pick(I_surface), surface_T=surface_T or None, I_top=pick(I_top),
                     terms=[np.asarray(t)[at] for t in terms], term_layer=term_layer)
    scale = flux.scale(nu, edges_of(case), I_surface=pick(I_surface), surface_T=surface_T or None, I_top=pick(I_top))
    uT = unit_T(nu, edges_of(case), surface_T)
    sl_tau, sl_T, sl_scat, sl_term = row_layout(L, NT, len(numbers), len(terms))
    idx = [(0, n)] if bands is None else bands
    inside = np.zeros(n, dtype=bool)
    for a, b in idx:
        inside[a:b] = True
    worst_band = 0.0
    if points is None:
        for b, (lo, hi) in enumerate(idx):
            want = ref.band_rows(J, lo, hi - lo)
            units = np.full(len(want), scale[lo:hi].sum())
            units[1] = uT[lo:hi].sum()
            units[sl_T] = uT[lo:hi].sum()
            worst_band = max(worst_band, np.max(np.abs(jac[b] - want) / units))
    worst_spec = 0.0
    if ut is not None:
        m = inside[at]
        for got, want, unit in ((ut[None], J["F"][None], scale), (tau_s, J["dtau"], scale), (T_s, J["dT"], uT)):
            assert np.all(got[:, ~inside] == 0.0) and np.all(np.isfinite(got[:, inside]))
            worst_spec = max(worst_spec, np.max(np.abs(got[:, at] - want)[:, m] / unit[m], initial=0.0))
    print("%s: band values %.3e, spectra %.3e of their units" % (name, worst_band, worst_spec))
    assert worst_band <= TOL and worst_spec <= TOL
    return jac, tau_s, T_s, ut


def boundaries(name):
    _, _, e, surface, top, bands = CASES[name]
    if isinstance(e, str):
        e = spectral_emissivity(N)
    return dict(e=e, surface_T=291.5 if surface == "T" else 0.0, I_surface=surface_radiance(N) if surface == "I" else None,
                I_top=sky_radiance(N) if top else None, bands=bands)


# ---- 1. against the restatement, and the forward bits ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement_and_forward_bits(ctx, name):
    make, delta = CASES[name][:2]
    case = hand_made(**make)
    terms, term_layer = terms_of(case, 7)
    kw = boundaries(name)
    jac, _, _, ut = check_raw(ctx, name, case, delta, terms=terms, term_layer=term_layer, **kw)
    sums, f_ut, _, _ = run_flux(ctx, delta=delta, **case, **kw)
    assert np.array_equal(jac[:, 0], sums[:, 0, L4]) and np.array_equal(ut, f_ut)


# ---- 2. the identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linear", (False, True))
def test_no_scatterers_is_the_surface_jacobian(ctx, linear):
    """n_scat = 0: lbl_column_jacobian_surface_dev (_linear_dev) with the angle set {(1 / sqrt(3), pi)} and Lambertian
    reflection: F, dF/dT_s, dF/de, d ln tau, the temperatures and the terms"""
    case = hand_made(62, linear=linear)
    terms, term_layer = terms_of(case, 8)
    e, I_top = spectral_emissivity(N), sky_radiance(N)
    jac = run_raw(ctx, e=e, surface_T=295.0, I_top=I_top, bands=BANDS, terms=terms, term_layer=term_layer, spectra=False,
                  **case)[0]
    bufs = [ctx.buffer(N).upload(case["k"][l]) for l in range(L4)]
    tb = [ctx.buffer(N).upload(t) for t in terms]
    nv = jac.shape[1]
    out, eb, top = ctx.buffer(2 * nv), ctx.buffer(N).upload(e), ctx.buffer(N).upload(I_top)
    try:
        call = ctx.column_jacobian_linear_dev if linear else ctx.column_jacobian_surface_dev
        call(bufs, case["T"], case["depth"], LO, HI, N, [MU], [W], [a for a, _ in BANDS], [b - a for a, b in BANDS], out, eb,
             reflection=0, surface_T=295.0, I_top=top, term_abs_coef=tb, term_layer=term_layer)
        other = out.download(2 * nv).reshape(2, nv)
    finally:
        for b in bufs + tb + [out, eb, top]:
            b.free()
    scale = flux.scale(grid(N), edges_of(case), surface_T=295.0, I_top=I_top)
    uT = unit_T(grid(N), edges_of(case), 295.0)
    sl_T = row_layout(L4, 2 if linear else 1, 0, len(terms))[1]
    worst = 0.0
    for b, (lo, hi) in enumerate(BANDS):
        units = np.full(nv, scale[lo:hi].sum())
        units[1] = units[sl_T] = uT[lo:hi].sum()
        worst = max(worst, np.max(np.abs(jac[b] - other[b]) / units))
    print("no scatterers, %s: %.3e of the units" % ("linear" if linear else "layer", worst))
    assert worst <= TOL


def test_equal_edges_are_the_layer_source(ctx):
    """planck_linear 1 with equal edge temperatures: the bottom and top rows sum to planck_linear 0's temperature row, and
    every other row is planck_linear 0's, to rounding"""
    case = hand_made(61, linear=False, scatterers=3, spectral=(1,))
    terms, term_layer = terms_of(case, 9)
    kw = dict(e=spectral_emissivity(N), surface_T=288.0, I_top=sky_radiance(N), bands=BANDS, terms=terms, term_layer=term_layer)
    layer = run_raw(ctx, **case, **kw)
    linear = run_raw(ctx, **dict(case, T=np.repeat(case["T"], 2), linear=True), **kw)
    scale = flux.scale(grid(N), edges_of(case), surface_T=288.0, I_top=sky_radiance(N))
    uT = unit_T(grid(N), edges_of(case), 288.0)
    tau0, T0, scat0, term0 = row_layout(L4, 1, 3, len(terms))
    tau1, T1, scat1, term1 = row_layout(L4, 2, 3, len(terms))
    assert np.array_equal(layer[3], linear[3]) and np.array_equal(layer[0][:, 0], linear[0][:, 0])
    for b, (lo, hi) in enumerate(BANDS):
        s, t = scale[lo:hi].sum(), uT[lo:hi].sum()
        a, c = layer[0][b], linear[0][b]
        assert abs(a[1] - c[1]) <= TOL * t and abs(a[2] - c[2]) <= TOL * s
        for x, y in ((tau0, tau1), (scat0, scat1), (term0, term1)):
            assert np.max(np.abs(a[x] - c[y])) <= TOL * s
        assert np.max(np.abs(a[T0] - c[T1].reshape(L4, 2).sum(axis=1))) <= TOL * t
    assert np.max(np.abs(layer[1] - linear[1]) / scale) <= TOL
    assert np.max(np.abs(layer[2] - linear[2].reshape(L4, 2, N).sum(axis=1)) / uT) <= TOL


@pytest.mark.parametrize("linear", (False, True))
def test_kirchhoff_cavity(ctx, linear):
    """one temperature everywhere, the sky included: no amount, term or emissivity changes the flux, whatever scatters"""
    T0 = 255.0
    case = hand_made(63, linear=linear, scatterers=4, spectral=(0, 3))
    case["T"] = np.full_like(case["T"], T0)
    terms, term_layer = terms_of(case, 10)
    B = flux.planck(grid(N), T0)
    tau, _, scat, term = row_layout(L4, 2 if linear else 1, 4, len(terms))
    for e in (0.0, 0.3, spectral_emissivity(N)):
        jac, tau_s, _, _ = run_raw(ctx, e=e, I_surface=B, I_top=B, terms=terms, term_layer=term_layer, **case)
        allow = TOL * (np.pi * B).sum()
        worst = max(np.max(np.abs(jac[0, x])) for x in (slice(2, 3), tau, scat, term)) / allow
        print("cavity: %.3e of the allowance" % worst)
        assert worst <= 1.0 and np.max(np.abs(tau_s) / (np.pi * B)) <= TOL


def test_a_scatterer_in_two_halves(ctx):
    """a scatterer split into two identical halves: the two rows sum to the whole's"""
    case = hand_made(71, scatterers=2, spectral=(0,))
    kw = dict(e=0.4, surface_T=290.0, I_top=sky_radiance(N), bands=BANDS, spectra=False)
    whole = run_raw(ctx, **case, **kw)[0]
    split = dict(case, amount=np.array([case["amount"][0] / 2, case["amount"][0] / 2, case["amount"][1]]),
                 numbers=[case["numbers"][0], case["numbers"][0], case["numbers"][1]])
    halves = run_raw(ctx, **split, **kw)[0]
    scale = flux.scale(grid(N), edges_of(case), surface_T=290.0, I_top=sky_radiance(N))
    s2, s3 = row_layout(L4, 2, 2, 0)[2], row_layout(L4, 2, 3, 0)[2]
    for b, (lo, hi) in enumerate(BANDS):
        a, c = whole[b][s2].reshape(2, L4), halves[b][s3].reshape(3, L4)
        assert np.max(np.abs(a[0] - (c[0] + c[1]))) <= TOL * scale[lo:hi].sum()
        assert np.max(np.abs(a[1] - c[2])) <= TOL * scale[lo:hi].sum()
        assert np.max(np.abs(whole[b][:s2.start] - halves[b][:s3.start])) <= TOL * scale[lo:hi].sum()


def test_the_pass_size_does_not_change_a_bit_and_two_runs_agree(ctx):
    case = hand_made(64, scatterers=2, spectral=(0,))
    terms, term_layer = terms_of(case, 11)
    kw = dict(e=0.4, surface_T=290.0, I_top=sky_radiance(N), bands=BANDS, terms=terms, term_layer=term_layer)
    whole = run_raw(ctx, **case, **kw)
    for other in (run_raw(ctx, passes=1, **case, **kw), run_raw(ctx, passes=300, **case, **kw), run_raw(ctx, **case, **kw)):
        for a, b in zip(whole, other):
            assert np.array_equal(a, b)


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------
def test_no_layer_one_layer_and_the_layer_limit(ctx):
    from pyrad_amd import _native
    # L = 0: the bare surface, F = e pi Is + (1 - e) pi I_top
    for linear in (0, 1):
        jac, _, _, ut = run_raw(ctx, np.zeros((0, 1)), [], [], linear, e=0.6, I_surface=[2.0], I_top=[0.5])
        assert jac.shape == (1, 3) and ut[0] == jac[0, 0] and jac[0, 1] == 0.0
        assert abs(jac[0, 2] - np.pi * (2.0 - 0.5)) <= 1e-15 * np.pi * 2.0
        jac = run_raw(ctx, np.zeros((0, 1)), [], [], linear, e=0.6, surface_T=280.0, spectra=False)[0]
        dB = np.pi * ref.planck_dT(np.array([LO]), 280.0)[0]
        assert abs(jac[0, 1] - 0.6 * dB) <= 1e-14 * dB
    for linear in (False, True):
        case = hand_made(66, L=1, n=300, scatterers=2, spectral=(1,), linear=linear)
        terms, term_layer = [0.3 * case["k"][0]], [0]
        check_raw(ctx, "one layer", case, 1, 0.5, surface_T=280.0, I_top=sky_radiance(300), terms=terms, term_layer=term_layer)
    L = _native.limit("layers_per_column")
    assert L == 128
    case = hand_made(67, L=L, n=256, scatterers=4, spectral=(0, 3))
    case["k"] *= 1e-2
    case["amount"] *= 1e-2
    terms, term_layer = terms_of(case, 12, per_layer=1)
    check_raw(ctx, "the layer limit", case, 1, spectral_emissivity(256), surface_T=300.0, terms=terms, term_layer=term_layer)


def test_beyond_one_round_of_partial_slots(ctx):
    """1,029 tiles over 1,024 slots: five slots take two tiles, and the last tile holds five points; 2,048 points against
    the restatement, the band values against the device's own spectra"""
    n = 1024 * 256 + 1029
    j = np.arange(n)
    case = dict(k=np.stack([1e-6 * (1 + (j % 7)), 1e-6 * (1 + ((j + 3) % 7))]), depth=np.array([2e5, 1e5]),
                T=np.array([[288.0, 262.0], [262.0, 231.0]]), linear=True, amount=np.array([[0.3, 1.5]]),
                numbers=[(1.0, 0.6, 0.8)])
    points = np.unique(np.concatenate([[0, 1, 255, 256, n - 1029, n - 6, n - 5, n - 1],
                                       np.random.RandomState(68).randint(0, n, 2048 - 8)]))
    jac, tau_s, T_s, ut = check_raw(ctx, "beyond one round", case, 1, 0.7, surface_T=290.0, points=points)
    s = flux.scale(grid(n), case["T"], surface_T=290.0).sum()
    t = unit_T(grid(n), case["T"], 290.0).sum()
    assert abs(jac[0, 0] - ut.sum()) <= TOL * s
    assert np.max(np.abs(jac[0, 3:5] - tau_s.sum(axis=1))) <= TOL * s and np.max(np.abs(jac[0, 5:9] - T_s.sum(axis=1))) <= TOL * t


def test_zero_huge_inf_and_nan_coefficients(ctx):
    """single points of 0, 1e300, inf and NaN: a point where some layer's optical depth is not finite is NaN in the spectra
    and counts as 0 in the sums; 1e300 gives finite values; every other point keeps its bits"""
    case = hand_made(69, L=3, scatterers=1)
    k = case["k"]
    k[0, 5], k[1, 6], k[2, 7], k[1, 400] = 0.0, 1e300, np.inf, np.nan
    k[0, 1027], k[2, 1028], k[2, 514] = np.nan, np.inf, 1e300
    bad = [7, 400, 1027, 1028]
    with np.errstate(invalid="ignore"):
        clean = np.where(np.isfinite(k) & (k < 1e299), k, 1e-5)
    terms, term_layer = [0.5 * clean[1], 0.25 * clean[2]], [1, 2]
    kw = dict(e=0.5, surface_T=285.0, I_top=sky_radiance(N), terms=terms, term_layer=term_layer)
    jac, *spec = run_raw(ctx, **case, **kw)
    jac2, *spec2 = run_raw(ctx, **dict(case, k=clean), **kw)
    same = np.all(k == clean, axis=0)
    for a, b in zip(spec, spec2):
        a, b = np.atleast_2d(a), np.atleast_2d(b)
        assert np.all(np.isnan(a[:, bad])) and np.all(np.isfinite(a[:, [5, 6, 514]]))
        assert np.array_equal(a[:, same], b[:, same])
    assert np.all(np.isfinite(jac))
    s = flux.scale(grid(N), case["T"], surface_T=285.0, I_top=sky_radiance(N)).sum()
    t = unit_T(grid(N), case["T"], 285.0).sum()
    assert abs(jac[0, 0] - np.nansum(spec[2])) <= TOL * s
    assert np.max(np.abs(jac[0, 3:6] - np.nansum(spec[0], axis=1))) <= TOL * s
    assert np.max(np.abs(jac[0, 6:12] - np.nansum(spec[1], axis=1))) <= TOL * t
    # 0 and 1e300 against the restatement
    good = np.array([5, 6, 514])
    J = ref.jacobian(k[:, good], case["depth"], grid(N)[good], case["T"], True, case["amount"], case["numbers"], 1, 0.5,
                     surface_T=285.0, I_top=sky_radiance(N)[good])
    scale = flux.scale(grid(N)[good], case["T"], surface_T=285.0, I_top=sky_radiance(N)[good])
    uT = unit_T(grid(N)[good], case["T"], 285.0)
    assert np.max(np.abs(spec[0][:, good] - J["dtau"]) / scale) <= TOL and np.max(np.abs(spec[1][:, good] - J["dT"]) / uT) <= TOL


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from pyrad_amd import _native
    lib = ctx.lib
    L, n, M = 3, 1027, 2
    k = hand_made(70, L=L, n=n)["k"]
    nv = 3 + (1 + 2 + 2) * L + M
    kb = [ctx.buffer(n).upload(k[l]) for l in range(L)]
    tile = ctx.column_jacobian_scatter_workspace(L, 1)
    jac, work = ctx.buffer(nv), ctx.buffer(2 * tile)
    spec = [ctx.buffer(L * n), ctx.buffer(2 * L * n), ctx.buffer(n)]
    Is, It, em, ext, ssa, asym, t0, t1 = (ctx.buffer(n).upload(np.full(n, v)) for v in (1.1, 0.2, 0.8, 1.5, 0.9, 0.7, 1e-7, 2e-7))
    jac_short, n_short, work_short = ctx.buffer(nv - 1), ctx.buffer(n - 1), ctx.buffer(tile - 1)
    tau_short, T_short = ctx.buffer(L * n - 1), ctx.buffer(2 * L * n - 1)
    i64, f64 = lambda v: (C.c_int64 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    ptrs = lambda v: (C.c_void_p * max(len(v), 1))(*v)
    cmax, tmax = _native.limit("scatterers"), _native.limit("jacobian_terms")
    inf, nan = float("inf"), float("nan")
    edges = [290.0, 280.0, 280.0, 260.0, 255.0, 240.0]
    good = dict(ctx=ctx.h, n_layers=L, abs_coef=ptrs([b.h for b in kb]), T=f64(edges), planck_linear=1,
                depth=f64([1e4, 2e4, 1e4]), lo=LO, hi=HI, n=n, I_surface=Is.h, surface_T=0.0, I_top=It.h, n_scat=2,
                scat_amount=f64([0.1, 0.0, 2.0, 1.0, 1.0, 1.0]), scat_ext=ptrs([ext.h, None]), scat_ext_all=f64([0.0, 2.0]),
                scat_ssa=ptrs([ssa.h, None]), scat_ssa_all=f64([0.0, 1.0]), scat_asym=ptrs([asym.h, None]),
                scat_asym_all=f64([0.0, -0.2]), delta_scaling=1, n_bands=1, band_first=i64([0]), band_count=i64([n]),
                emissivity=em.h, emissivity_all=0.5, n_terms=M, term_abs_coef=ptrs([t0.h, t1.h]), term_layer=i32([2, 0]),
                workspace=work.h, jac=jac.h, jac_ln_tau_spectra=spec[0].h, jac_T_spectra=spec[1].h, up_top=spec[2].h)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_column_jacobian_scatter_dev(*[a[key] for key in good])

    bad = [  # the shared arguments, as lbl_column_flux_scatter_dev refuses them
           dict(abs_coef=None), dict(T=None), dict(depth=None), dict(scat_amount=None), dict(band_first=None),
           dict(band_count=None), dict(jac=None), dict(workspace=None),
           dict(n_layers=-1), dict(n=-5), dict(n_scat=-1), dict(n_bands=-1),
           dict(n_layers=_native.limit("layers_per_column") + 1),
           dict(n_scat=cmax + 1, scat_amount=f64([0.1] * (L * (cmax + 1))), scat_ext=None, scat_ext_all=f64([1.0] * (cmax + 1)),
                scat_ssa=None, scat_ssa_all=f64([1.0] * (cmax + 1)), scat_asym=None, scat_asym_all=f64([0.0] * (cmax + 1))),
           dict(n_bands=0), dict(n_bands=_native.limit("flux_bands") + 1),
           dict(I_surface=n_short.h), dict(I_top=n_short.h), dict(up_top=n_short.h), dict(emissivity=n_short.h),
           dict(abs_coef=ptrs([kb[0].h, n_short.h, kb[2].h])), dict(scat_ext=ptrs([n_short.h, None])),
           dict(scat_ssa=ptrs([ssa.h, n_short.h])), dict(scat_asym=ptrs([n_short.h, None])),
           dict(band_count=i64([n + 1])), dict(band_first=i64([-1])), dict(band_count=i64([0])), dict(band_first=i64([n])),
           dict(depth=f64([1e4, -1.0, 1e4])), dict(depth=f64([1e4, nan, 1e4])),
           dict(I_surface=None, surface_T=0.0), dict(I_surface=None, surface_T=-3.0), dict(I_surface=None, surface_T=nan),
           dict(T=f64([290.0, 280.0, 280.0, 0.0, 255.0, 240.0])), dict(T=f64([nan, 280.0, 280.0, 260.0, 255.0, 240.0])),
           dict(T=f64([290.0, 280.0, 280.0, 260.0, 255.0, inf])),
           dict(planck_linear=0, T=f64([290.0, 0.0, 250.0])), dict(planck_linear=0, T=f64([290.0, nan, 250.0])),
           dict(planck_linear=0, T=f64([290.0, 270.0, inf])), dict(planck_linear=2), dict(planck_linear=-1),
           dict(scat_amount=f64([0.1, -1e-9, 2.0, 1.0, 1.0, 1.0])), dict(scat_amount=f64([0.1, 0.0, 2.0, 1.0, nan, 1.0])),
           dict(scat_amount=f64([inf, 0.0, 2.0, 1.0, 1.0, 1.0])),
           dict(scat_ext_all=f64([0.0, -1.0])), dict(scat_ext_all=f64([0.0, inf])), dict(scat_ext_all=None),
           dict(scat_ssa_all=f64([0.0, -0.01])), dict(scat_ssa_all=f64([0.0, 1.01])), dict(scat_asym_all=f64([0.0, 1.0])),
           dict(scat_asym_all=f64([0.0, nan])),
           dict(delta_scaling=2), dict(delta_scaling=-1),
           dict(emissivity=None, emissivity_all=-0.01), dict(emissivity=None, emissivity_all=1.01),
           # the terms, jac and the spectra, as lbl_column_jacobian_dev refuses them
           dict(jac=jac_short.h), dict(jac_ln_tau_spectra=tau_short.h), dict(jac_T_spectra=T_short.h),
           dict(n_terms=-1), dict(n_terms=tmax + 1), dict(term_abs_coef=None), dict(term_layer=None),
           dict(term_layer=i32([2, 3])), dict(term_layer=i32([-1, 0])), dict(term_abs_coef=ptrs([t0.h, n_short.h])),
           dict(term_abs_coef=ptrs([t0.h, None])),
           # the workspace: one tile of five numbers per level and point
           dict(workspace=work_short.h)]
    outs = [jac] + spec
    everything = kb + outs + [work, Is, It, em, ext, ssa, asym, t0, t1, jac_short, n_short, work_short, tau_short, T_short]
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
        # a workspace of K5m's size for one tile is too short: five numbers per level and point
        flux_tile = ctx.buffer(ctx.column_flux_scatter_workspace(L, 1))
        everything.append(flux_tile)
        assert call(workspace=flux_tile.h) == BAD_ARG
        assert call() == 0
        for b, w in zip(outs, want):
            assert np.array_equal(b.download(), w)
        # what is allowed: no spectra, no terms, no scatterer, the layer source
        assert call(jac_ln_tau_spectra=None, jac_T_spectra=None, up_top=None, emissivity=None, I_top=None) == 0
        assert call(n_terms=0, term_abs_coef=None, term_layer=None) == 0
        assert call(n_scat=0, scat_amount=None, scat_ext=None, scat_ext_all=None, scat_ssa=None, scat_ssa_all=None,
                    scat_asym=None, scat_asym_all=None) == 0
        assert call(planck_linear=0, T=f64([290.0, 270.0, 250.0]), delta_scaling=0) == 0
        jac.download()                                      # (the queue drains without an error)
    finally:
        for b in everything:
            b.free()


# ---- 5. the model ---------------------------------------------------------------------------------------------------------
def model_units(pyrad, atm, surface_T):
    x = atm[0].xAxis
    temps = [Ly.T for Ly in atm] + list(atm.levelTemperatures())
    return flux.scale(x, temps, surface_T=surface_T), unit_T(x, temps, surface_T)


@pytest.mark.parametrize("planck", ("layer", "linear"))
def test_model_without_scatterers_is_jacobians(pyrad, lines, planck):
    """jacobians() / jacobiansLinear() at the two-stream angle over a Lambertian surface: two kernels, each with an error of
    its own, so the allowance is the sum of this file's TOL and the other kernels' floor, 40 L 1e-16 of the scale per point
    (derived in tests/test_gpu_jacobian.py and tests/test_gpu_surface_jacobian.py: the unclamped A B + D carries about
    L 1e-16 of the radiance and d ln tau multiplies it by tau / mu, held below 40 by the clamp)"""
    from pyrad_amd import settings
    atm = column(pyrad)
    both = TOL + 40 * len(atm) * 1e-16
    kw = dict(surfaceTemperature=290.0, emissivity=0.8, bands=[(600, 640), (640, 701)], spectra=True)
    two = atm.jacobiansTwoStream(planck=planck, **kw)
    one = (atm.jacobiansLinear if planck == "linear" else atm.jacobians)(angles=[(MU, W)], reflection="lambertian", **kw)
    scale, uT = model_units(pyrad, atm, 290.0)
    x = atm[0].xAxis
    res = settings.BASE_RESOLUTION
    assert list(two.mu) == [MU] and list(two.weight) == [W] and two.scatterers.shape == (2, 0, len(atm))
    for b, (lo, hi) in enumerate([(int(np.searchsorted(x, a)), int(np.searchsorted(x, c))) for a, c in kw["bands"]]):
        s, t = both * scale[lo:hi].sum() * res, both * uT[lo:hi].sum() * res
        pairs = [(two.olr[b], one.olr[b], s), (two.emissivity[b], one.emissivity[b], s),
                 (two.opticalDepth[b], one.opticalDepth[b], s), (two.surfaceTemperature[b], one.surfaceTemperature[b], t),
                 (two.temperature[b], one.temperature[b], t)]
        pairs += [(a[b], c[b], s) for a, c in zip(two.molecules, one.molecules)]
        if planck == "linear":
            pairs += [(two.edgeTemperature[b], one.edgeTemperature[b], t), (two.levelTemperature[b], one.levelTemperature[b], t)]
        worst = max(np.max(np.abs(a - c)) / allow for a, c, allow in pairs)
        print("band %d: %.3e of the allowance" % (b, worst))
        assert worst <= 1.0
    a, c = ((two.levelTemperatureSpectrum, one.levelTemperatureSpectrum) if planck == "linear"
            else (two.temperatureSpectrum, one.temperatureSpectrum))
    worst = np.max(np.abs(two.opticalDepthSpectrum - one.opticalDepthSpectrum) / scale), np.max(np.abs(a - c) / uT)
    print("spectra: d ln tau %.3e of the scale, temperatures %.3e of pi dB/dT" % worst)
    assert worst[0] <= both and worst[1] <= 2 * both     # (a level's row is the sum of two edges' rows)


@pytest.mark.parametrize("planck", ("layer", "linear"))
def test_model_a_grey_cloud_against_central_differences(pyrad, lines, planck):
    """a cloud in the top layer: more of it, less leaves; opticalDepth, scatterers and surfaceTemperature against central
    differences of fluxesTwoStream() itself - relative steps h = 1e-4 in the amounts, 0.01 K - to the second-order truncation
    h^2 |f'''| / 6, taken as 10 h^2 times the largest value of the row (a logarithmic derivative's third derivative is of
    the order of the derivative itself, a factor of 60 allowed; for T_s the step is measured against 30 K, the scale on which
    the Planck function's derivatives change), plus 1e-12 / h of the band's scale"""
    from pyrad_amd import settings
    atm = column(pyrad)
    nl = len(atm)
    amounts = [0.0] * (nl - 1) + [5.0]
    cloud = lambda a: pyrad.Scatterer(a, extinction=1.0, singleScatteringAlbedo=0.5, asymmetry=0.85, name="cloud")
    kw = dict(surfaceTemperature=288.0, planck=planck)
    jac = atm.jacobiansTwoStream([cloud(amounts)], **kw)
    base = atm.fluxesTwoStream([cloud(amounts)], **kw)
    assert jac.olr == base.up[-1]
    assert jac.scatterers.shape == (1, nl) and jac.scatterers[0, -1] < 0 and not jac.scatterers[0, :-1].any()
    scale, _ = model_units(pyrad, atm, 288.0)
    s = scale.sum() * settings.BASE_RESOLUTION
    h = 1e-4
    top = lambda **k2: atm.fluxesTwoStream([cloud(k2.pop("amounts", amounts))], **dict(kw, **k2)).up[-1]
    d_cloud = (top(amounts=amounts[:-1] + [5.0 * (1 + h)]) - top(amounts=amounts[:-1] + [5.0 * (1 - h)])) / (2 * h)
    tol = h * h * np.max(np.abs(jac.scatterers)) * 10 + 1e-12 / h * s
    print("cloud: %.6e against %.6e, tolerance %.1e" % (jac.scatterers[0, -1], d_cloud, tol))
    assert abs(jac.scatterers[0, -1] - d_cloud) <= tol
    dT = 0.01
    d_Ts = (top(surfaceTemperature=288.0 + dT) - top(surfaceTemperature=288.0 - dT)) / (2 * dT)
    tol = (dT / 30.0) ** 2 * abs(jac.surfaceTemperature) * 10 + 1e-12 / dT * s
    print("T_s: %.6e against %.6e, tolerance %.1e" % (jac.surfaceTemperature, d_Ts, tol))
    assert abs(jac.surfaceTemperature - d_Ts) <= tol
    # the gas of one layer scaled: its depth scaled, which scales k depth and nothing else (the levels' temperatures held)
    l = nl // 2
    depth = atm[l].depth
    lev = dict(levelTemperatures=list(atm.levelTemperatures())) if planck == "linear" else {}
    ups = []
    for f in (1 + h, 1 - h):
        atm[l].changeDepth(depth * f)
        ups.append(atm.fluxesTwoStream([cloud(amounts)], **lev, **kw).up[-1])
    atm[l].changeDepth(depth)
    d_tau = (ups[0] - ups[1]) / (2 * h)
    tol = h * h * np.max(np.abs(jac.opticalDepth)) * 10 + 1e-12 / h * s
    print("tau: %.6e against %.6e, tolerance %.1e" % (jac.opticalDepth[l], d_tau, tol))
    assert abs(jac.opticalDepth[l] - d_tau) <= tol


def test_model_full_temperature_under_voigt(voigt_model):
    """temperature="full" under the Voigt setting adds dk/dT as a term of every layer, as jacobians() does: without
    scatterers the absorption part is jacobians()'s to rounding, and every other value is temperature="planck"'s"""
    from test_gpu_voigt_dT import LAYERS as VOIGT_LAYERS, _layer
    atm = voigt_model.Atmosphere("full")
    for depth, T, P in VOIGT_LAYERS:
        _layer(voigt_model, atm, depth, T, P)
    nl = len(atm)
    kw = dict(surfaceTemperature=288.0, emissivity=0.8)
    two = atm.jacobiansTwoStream(temperature="full", **kw)
    plain = atm.jacobiansTwoStream(**kw)
    one = atm.jacobians(angles=[(MU, W)], reflection="lambertian", temperature="full", **kw)
    assert plain.temperatureAbsorption is None and plain.temperatureFull is None
    for name in ("olr", "surfaceTemperature", "emissivity", "temperature", "opticalDepth"):
        assert np.array_equal(getattr(two, name), getattr(plain, name)), name
    assert two.temperatureAbsorption.shape == (nl,)
    assert np.array_equal(two.temperatureFull, two.temperature + two.temperatureAbsorption)
    # (dk/dT depth is not a part of the layer's optical depth: the unit is the largest value itself)
    worst = np.max(np.abs(two.temperatureAbsorption - one.temperatureAbsorption)) / np.max(np.abs(one.temperatureAbsorption))
    print("dk/dT terms: %.2e of the largest" % worst)
    assert worst <= 1e-9
    cloud = voigt_model.Scatterer([0.0] * (nl - 1) + [5.0], 1.0, 0.5, 0.85)
    cloudy = atm.jacobiansTwoStream([cloud], temperature="full", molecules=False, **kw)
    assert cloudy.molecules is None and np.all(np.isfinite(cloudy.temperatureAbsorption)) and cloudy.olr < two.olr
