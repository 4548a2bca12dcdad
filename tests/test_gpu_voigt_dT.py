"""GPU: dk/dT under the true Voigt line shape - lbl_voigt_gradient_dev and lbl_xsec_voigt_dt_dev (kernels K2v-T) against the
committed mpmath fixture tests/golden/V1_voigt_dT.npz (made by tests/golden/make_voigt_dT_golden.py; the cells' lines are
V0_voigt.npz's), the kernel's geometry and summation against sums formed in NumPy from the device function's own values,
determinism, the C ABI's refusals, Layer.absCoefDT, and Atmosphere.jacobians(temperature="full") against finite differences
of the model itself."""
import json
import sys

import numpy as np
import pytest

from conftest import GOLDEN, RTOL_BASE, load_golden
from oracle import pyrad_oracle as orc
from pyrad_amd import synthetic

sys.path.insert(0, GOLDEN)
import make_voigt_golden as mvg      # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG, STATE = -1, -6
RTOL = 1e-6                          # voigt_kgrad's contract: errors over K
Z0 = load_golden("V0_voigt")
Z1 = load_golden("V1_voigt_dT")
CASES = json.loads(str(Z1["cases"]))
BETA = synthetic.SPECIES["co2"]["beta"]


@pytest.fixture(scope="module")
def ctx():
    from pyrad_amd import _native as nat
    c = nat.Context(0)
    yield c
    c.close()


def job(ctx, case, shard=None):
    """(Lines, IsoParams, Grid, Buffer) of a fixture cell, and its grid"""
    from pyrad_amd import _native as nat, engine
    g = engine.layer_grid(case["P"], case["lo"], case["hi"], case["base_resolution"], case["dynamic"])
    molmass, q_T, q296, g_orc = mvg.case_physics(case)
    assert all(g[k] == g_orc[k] for k in ("n_work", "n_base", "W", "resolution"))
    L = ctx.lines(case["lines"])
    iso = nat.IsoParams(case["T"], case["P"], case["q"], molmass, q_T, q296)
    out = ctx.buffer(max(g["n_base"], 1)).fill(0.0)
    return (L, iso, engine.native_grid(g, shard), out), g


def dlnw(case):
    return -BETA / case["T"]             # -d ln Q / dT of pyrad_amd.synthetic's Q(T) = Q296 (T / 296)^beta, exactly


def run(ctx, case, shard=None):
    j, g = job(ctx, case, shard)
    ctx.xsec_voigt_dT_dev([j], [dlnw(case)])
    d = j[3].download(g["n_base"])
    j[0].free(); j[3].free()
    return d, g


def gradient_dev(ctx, x, y):
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    x, y = np.ascontiguousarray(x).ravel(), np.ascontiguousarray(y).ravel()
    bufs = [ctx.buffer(x.size).upload(x), ctx.buffer(x.size).upload(y)] + [ctx.buffer(x.size) for _ in range(3)]
    ctx.voigt_gradient_dev(bufs[0], bufs[1], x.size, *bufs[2:])
    out = [b.download(x.size) for b in bufs[2:]]
    ctx.voigt_function_dev(bufs[0], bufs[1], x.size, bufs[2])
    k = bufs[2].download(x.size)
    for b in bufs:
        b.free()
    return out, k


# ---- 1. the function ----------------------------------------------------------------------------------------------------
def test_function_on_the_fixture_sets(ctx):
    fx, fy = mvg.table_axes()
    X, Y = np.broadcast_arrays(fx[:, None], fy[None, :])
    rx, ry = mvg.random_pairs(2000)
    bx, by = mvg.band_points()
    for what, x, y, tag in (("table", X, Y, "f"), ("random pairs", rx, ry, "r"), ("bands", bx, by, "b")):
        (K, GX, GY), k = gradient_dev(ctx, x, y)
        rK, rGX, rGY = (Z1[tag + n].ravel() for n in ("K", "GX", "GY"))
        assert np.array_equal(K, k), "%s: K is not lbl_voigt_function_dev's value bit for bit" % what
        assert not (np.isnan(K).any() or np.isnan(GX).any() or np.isnan(GY).any())
        assert np.all(K >= 0) and np.all(GX <= 0)
        big = rK >= mvg.FLOOR
        assert np.all(K[~big] <= mvg.FLOOR)
        worst = [float(np.max(np.abs(g[big] - r[big]) / rK[big])) for g, r in ((K, rK), (GX, rGX), (GY, rGY))]
        print("device voigt_kgrad, %s: worst |dK|/K %.2e, |dGX|/K %.2e, |dGY|/K %.2e" % (what, *worst))
        assert max(worst) <= RTOL, (what, worst)
    nan = float("nan")
    (K, GX, GY), _ = gradient_dev(ctx, [nan, 1.0, nan, 20.0, 3.0], [1.0, nan, 0.0, nan, nan])
    assert np.isnan(K).all() and np.isnan(GX).all() and np.isnan(GY).all()


# ---- 2. the cells -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_derivative_against_the_fixture(ctx, name):
    """|got - ref| <= 1e-6 scale + 64 2^-53 abs3 at every point: K, GX, GY are each within 1e-6 K and their multipliers are
    |a|, 1 / (2 T) and |n_air + 1/2| / T (scale = sum amp K (|a| + (|n_air| + 1) / T)); the second term covers the summation
    of up to 200 lines and the last bits of amp, a, xs, y (abs3 = sum of the three terms' magnitudes)."""
    case = mvg.load_case(Z0, name)
    got, g = run(ctx, case)
    ref, scale, abs3 = (Z1["%s.%s" % (name, k)] for k in ("dxsec", "scale", "abs3"))
    assert got.shape == ref.shape
    assert np.array_equal(got == 0, ref == 0), "exact zeros must be matched by exact zeros"
    tol = RTOL * scale + 64 * 2.0 ** -53 * abs3
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, 0.0)
    print("%s: worst |err| / scale %.3e (W = %d, %d lines)" % (name, rel.max() if rel.size else 0.0, g["W"], len(case["lines"]["nu"])))
    assert np.all(err <= tol), (name, float(rel.max()))
    if name == "empty":
        assert not got.any()
    if name == "isolated":
        assert np.count_nonzero(got) == 2 * (g["W"] - 2) + 1


def test_cells_cover_what_the_kernel_can_get_wrong():
    W = {}
    for name in CASES:
        case = mvg.load_case(Z0, name)
        g = mvg.case_physics(case)[3]
        W[name] = g["W"]
        assert len(case["lines"]["nu"]) <= 200 and g["n_work"] <= 6000
    assert {1, 5, 50, 500} <= set(W.values())
    g = mvg.case_physics(mvg.load_case(Z0, "surface"))[3]
    assert g["n_work"] == 4000 and g["n_work"] % 512
    assert mvg.case_physics(mvg.load_case(Z0, "tiny"))[3]["n_work"] < 64
    g = mvg.case_physics(mvg.load_case(Z0, "wide"))[3]
    assert g["W"] - 2 > g["n_work"]
    g = mvg.case_physics(mvg.load_case(Z0, "regrid"))[3]
    assert g["n_work"] != g["n_base"]
    assert not mvg.load_case(Z0, "doppler")["lines"]["gamma_air"].any()


# ---- 3. geometry and summation, apart from the approximation -----------------------------------------------------------
@pytest.mark.parametrize("name", ["surface", "p100", "p1", "wide"])
def test_geometry_and_summation(ctx, name):
    """The kernel's sum against amp (a K + bx GX + by GY) summed in line order in NumPy, (K, GX, GY) from
    lbl_voigt_gradient_dev at the very x = |d| xs, y the kernel forms and a, by from the documented formulas in NumPy: what
    is left is the association of the multiply-adds and the last bits of amp and a.  The bound is the Voigt value test's
    (RTOL_BASE), against the sum of the three terms' magnitudes."""
    case = mvg.load_case(Z0, name)
    j, g = job(ctx, case)
    assert g["n_work"] == g["n_base"]
    q = ctx.line_quantities(j[0], j[1], j[2])
    ctx.xsec_voigt_dT_dev([j], [dlnw(case)])
    got = j[3].download(g["n_base"])
    j[0].free(); j[3].free()
    n, H, T = g["n_work"], max(g["W"] - 2, 0), case["T"]
    L = case["lines"]
    sx = g["resolution"] / q["ghw"]
    y = q["lhw"] / q["ghw"]
    amp = q["intensity"] * (1.0 / (q["ghw"] * np.sqrt(np.pi)))
    nus = L["nu"] + L["delta_air"] * case["P"] / orc.p0
    a = dlnw(case) + orc.c2 * L["elower"] / T ** 2 - (orc.c2 * nus / T ** 2) / np.expm1(orc.c2 * nus / T) - 0.5 / T
    bx, by = -0.5 / T, -(L["n_air"] + 0.5) / T
    spans = [(max(int(c) - H, 0), min(int(c) + H, n - 1)) for c in q["index"]]
    X = np.concatenate([np.abs(np.arange(lo, hi + 1) - int(c)).astype(np.float64) * sx[i] if hi >= lo else np.zeros(0)
                        for i, ((lo, hi), c) in enumerate(zip(spans, q["index"]))])
    Yv = np.concatenate([np.full(max(hi - lo + 1, 0), y[i]) for i, (lo, hi) in enumerate(spans)])
    (K, GX, GY), _ = gradient_dev(ctx, X, Yv)
    want, mag = np.zeros(n), np.zeros(n)
    at = 0
    for i, (lo, hi) in enumerate(spans):
        if hi < lo:
            continue
        s = slice(at, at + hi - lo + 1)
        want[lo:hi + 1] += amp[i] * (a[i] * K[s] + bx * GX[s] + by[i] * GY[s])
        mag[lo:hi + 1] += amp[i] * (np.abs(a[i] * K[s]) + np.abs(bx * GX[s]) + np.abs(by[i] * GY[s]))
        at = s.stop
    assert np.array_equal(got == 0, mag == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(mag > 0, np.abs(got - want) / mag, 0.0)
    print("%s: kernel against line-order sums of the device function's values: %.3e of the terms' magnitudes" % (name, rel.max()))
    assert rel.max() <= RTOL_BASE


# ---- 4. shards and batches ---------------------------------------------------------------------------------------------
def test_shard_equals_the_same_points_of_the_whole(ctx):
    case = mvg.load_case(Z0, "surface")
    whole, g = run(ctx, case)
    for first, count in ((130, 2777), (1, 63), (3999, 1)):           # off every tile, span and lane alignment
        part, _ = run(ctx, case, shard=(first, count))
        assert np.array_equal(part[first:first + count], whole[first:first + count])
        assert not part[:first].any() and not part[first + count:].any()      # nothing outside the shard is written


def test_same_bits_twice_and_whatever_the_batch(ctx):
    cases = [mvg.load_case(Z0, n) for n in ("p100", "surface", "p1")]
    alone = [run(ctx, c)[0] for c in cases]
    assert np.array_equal(run(ctx, cases[0])[0], alone[0])
    for order in ((0, 1, 2), (1, 2, 0), (2, 1, 0)):
        jobs = [job(ctx, cases[k])[0] for k in order]
        ctx.xsec_voigt_dT_dev(jobs, [dlnw(cases[k]) for k in order])
        for k, j in zip(order, jobs):
            assert np.array_equal(j[3].download(alone[k].size), alone[k]), order
            j[0].free(); j[3].free()


def test_values_and_regime_counts_are_left_alone(ctx):
    """The derivative batch shares the value batch's scratch and counts no regimes: lbl_last_regime_counts keeps describing
    the last value batch, and the values after a derivative batch are the values before it."""
    case = mvg.load_case(Z0, "p1")
    j, g = job(ctx, case)
    ctx.xsec_voigt_dev([j])
    before = j[3].download(g["n_base"])
    counts = tuple(ctx.last_regime_counts(1)[0])
    assert sum(counts) == len(case["lines"]["nu"])
    run(ctx, mvg.load_case(Z0, "surface"))
    assert tuple(ctx.last_regime_counts(1)[0]) == counts
    ctx.xsec_voigt_dev([j])
    assert np.array_equal(j[3].download(g["n_base"]), before)
    j[0].free(); j[3].free()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable(ctx):
    import ctypes as C
    from pyrad_amd import _native as nat, engine
    case = mvg.load_case(Z0, "tiny")
    good, _ = run(ctx, case)
    (L, iso, grid, out), g = job(ctx, case)
    lib, P = ctx.lib, nat._P
    one, isos, grids, outs = (P * 1)(L.h), (nat.IsoParams * 1)(iso), (nat.Grid * 1)(grid), (P * 1)(out.h)
    w = (C.c_double * 1)(dlnw(case))
    call = lambda *a: lib.lbl_xsec_voigt_dt_dev(*a)      # noqa: E731
    assert call(None, 1, one, isos, w, grids, outs) == BAD_ARG
    for k in range(5):                                     # every array argument NULL in turn
        a = [one, isos, w, grids, outs]
        a[k] = None
        assert call(ctx.h, 1, *a) == BAD_ARG
    assert call(ctx.h, -1, one, isos, w, grids, outs) == BAD_ARG
    assert call(ctx.h, 65537, one, isos, w, grids, outs) == BAD_ARG                # LBL_MAX_JOBS + 1
    assert b"jobs per batch" in lib.lbl_last_error(ctx.h)
    assert call(ctx.h, 0, None, None, None, None, None) == 0                       # an empty batch
    no_window = (nat.Grid * 1)(engine.native_grid(dict(g, W=0)))
    assert call(ctx.h, 1, one, isos, w, no_window, outs) == BAD_ARG and b"window" in lib.lbl_last_error(ctx.h)
    short = ctx.buffer(g["n_base"] - 1)
    assert call(ctx.h, 1, one, isos, w, grids, (P * 1)(short.h)) == BAD_ARG
    assert call(ctx.h, 1, one, isos, w, grids, (P * 1)(None)) == STATE
    assert call(ctx.h, 1, (P * 1)(None), isos, w, grids, outs) == STATE
    for field in range(4):                                 # T, P, molmass, Q_T <= 0
        v = [iso.T, iso.P, iso.q_frac, iso.molmass, iso.Q_T, iso.Q_296]
        v[(0, 1, 3, 4)[field]] = 0.0
        assert call(ctx.h, 1, one, (nat.IsoParams * 1)(nat.IsoParams(*v)), w, grids, outs) == BAD_ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(ctx.h, 1, one, isos, (C.c_double * 1)(bad), grids, outs) == BAD_ARG
        assert b"dlnw_dT" in lib.lbl_last_error(ctx.h)
    other = nat.Context(0)
    try:
        foreign = other.buffer(g["n_base"])
        assert call(ctx.h, 1, one, isos, w, grids, (P * 1)(foreign.h)) == STATE
        fl = other.lines(case["lines"])
        assert call(ctx.h, 1, (P * 1)(fl.h), isos, w, grids, outs) == STATE
        b = ctx.buffer(8)
        assert lib.lbl_voigt_gradient_dev(ctx.h, b.h, b.h, 8, b.h, b.h, foreign.h) == STATE
        fl.free(); foreign.free(); b.free()
    finally:
        other.close()
    b, small = ctx.buffer(8), ctx.buffer(7)
    fn = lib.lbl_voigt_gradient_dev
    assert fn(ctx.h, b.h, b.h, 9, b.h, b.h, b.h) == BAD_ARG
    for k in range(5):
        a = [b.h] * 5
        a[k] = small.h
        assert fn(ctx.h, a[0], a[1], 8, *a[2:]) == BAD_ARG
        a[k] = None
        assert fn(ctx.h, a[0], a[1], 8, *a[2:]) == BAD_ARG
    assert fn(ctx.h, b.h, b.h, -1, b.h, b.h, b.h) == BAD_ARG and fn(None, b.h, b.h, 8, b.h, b.h, b.h) == BAD_ARG
    assert fn(ctx.h, b.h, b.h, 0, b.h, b.h, b.h) == 0
    # nothing was enqueued by any of them, and the context works: the same bits as before
    assert not out.download(g["n_base"]).any()
    ctx.xsec_voigt_dT_dev([(L, iso, grid, out)], [dlnw(case)])
    assert np.array_equal(out.download(g["n_base"]), good)
    with pytest.raises(ValueError):
        ctx.xsec_voigt_dT_dev([(L, iso, grid, out)], [])
    for o in (L, out, short, b, small):
        o.free()


# ---- 6. the model -------------------------------------------------------------------------------------------------------
LO, HI = 600.0, 605.0                                     # 500 points at 0.01 cm^-1


@pytest.fixture()
def pyrad():
    from pyrad_amd import model, data, settings
    model.Layer.hasAtmosphere = False
    settings.set_layer_step("merged")
    settings.set_line_shape("voigt")
    data.set_source(data.synthetic_source(dict(co2=synthetic.make_lines(41, 150, 590, 615),
                                               h2o=synthetic.make_lines(42, 150, 590, 615))))
    yield model
    settings.set_line_shape("reference")
    data.set_source(None)
    model.Layer.hasAtmosphere = False


def _layer(pyrad, atm, depth, T, P):
    L = atm.addLayer(depth, T, P, LO, HI)
    L.addMolecule("co2", ppm=400)
    L.addMolecule("h2o", percentage=0.5)
    return L


def _abs_coef_dT_by_hand(pyrad, L):
    """(sum_m f_m sum_iso dsigma/dT - k / T, sum of the terms' magnitudes) from the ABI-level results in NumPy"""
    from pyrad_amd import engine
    ctx = engine.get_engine().ctx
    n = len(L.xAxis)
    total, mag = np.zeros(n), np.zeros(n)
    for m in L:
        d_m = np.zeros(n)
        for iso in m:
            q = iso.q
            dlnq = (q[L.T + 1] - q[L.T - 1]) / (2 * q[L.T])
            out = ctx.buffer(n).fill(0.0)
            lines = ctx.lines(iso._lines)
            ctx.xsec_voigt_dT_dev([(lines, pyrad._iso_params(iso), engine.native_grid(L._grid()), out)], [-dlnq])
            d_m = d_m + out.download(n)
            lines.free(); out.free()
        total = total + orc.abs_coef(d_m, m.concentration, L.P, L.T)
        mag = mag + np.abs(orc.abs_coef(d_m, m.concentration, L.P, L.T))
    k = np.array(L.absCoef)
    return total - k / L.T, mag + k / L.T


def test_abs_coef_dT_is_the_weighted_sum_and_follows_the_mutators(pyrad):
    from pyrad_amd import settings
    atm = pyrad.Atmosphere("dT")
    L = _layer(pyrad, atm, 2e4, 250, 100.0)
    assert len(L.xAxis) == 500 and len(L) == 2
    got = np.array(L.absCoefDT)
    assert np.array_equal(got, pyrad.getAbsCoefDT(L)) and got.any()
    want, mag = _abs_coef_dT_by_hand(pyrad, L)
    assert np.max(np.abs(got - want) / mag) <= 1e-13
    # (changePressure keeps the effective range the layer was built with, as the reference does: going DOWN in pressure the
    # changed layer holds a few lines more than a fresh one, all of them farther outside the range than the new window
    # reaches, so they add nothing and the bits agree)
    for change, args, fresh in ((L.changeTemperature, (251,), (2e4, 251, 100.0)), (L.changePressure, (80.0,), (2e4, 251, 80.0))):
        change(*args)
        moved = np.array(L.absCoefDT)
        assert not np.array_equal(moved, got)
        assert np.array_equal(moved, _layer(pyrad, pyrad.Atmosphere("fresh"), *fresh).absCoefDT)
        got = moved
    k = np.array(L.absCoef)
    settings.set_line_shape("reference")
    with pytest.raises(ValueError, match="discontinuous in T"):
        L.absCoefDT
    settings.set_line_shape("voigt")
    assert np.array_equal(L.absCoefDT, got) and np.array_equal(L.absCoef, k)
    L.changeTemperature(250.5)
    with pytest.raises(KeyError):
        L.absCoefDT


# ---- 7. end to end against finite differences ---------------------------------------------------------------------------
LAYERS = ((1e4, 288, 1013.25), (2e4, 250, 100.0), (5e4, 220, 10.0))


@pytest.mark.parametrize("angles", [1, 3])
def test_full_temperature_jacobian_against_finite_differences(pyrad, angles):
    """dF/dT_l of jacobians(temperature="full") against R = (4 D1 - D2) / 3 of the model's own olr, D1 and D2 the central
    differences at +-1 K and +-2 K; tolerance |D1 - D2| + 1e-6 |R|, the differences' own truncation estimate.  The column
    was sized on the CPU oracle (SciPy's wofz in the oracle's geometry, one angle): the absorption part is 1.8e3 and 1.0e3
    times |D1 - D2| in the two upper layers (the lowest one stands at the surface's temperature and has next to none)."""
    atm = pyrad.Atmosphere("fd")
    for depth, T, P in LAYERS:
        _layer(pyrad, atm, depth, T, P)
    kw = dict(surfaceTemperature=288, angles=angles)
    plain = atm.jacobians(**kw)
    planck = atm.jacobians(temperature="planck", **kw)
    for name in ("olr", "surfaceTemperature", "temperature", "opticalDepth"):
        assert np.array_equal(getattr(plain, name), getattr(planck, name)), name
    assert all(np.array_equal(a, b) for a, b in zip(plain.molecules, planck.molecules))
    assert planck.temperatureAbsorption is None and planck.temperatureFull is None and plain.temperatureFull is None
    full = atm.jacobians(temperature="full", **kw)
    for name in ("olr", "surfaceTemperature", "temperature", "opticalDepth"):
        assert np.array_equal(getattr(full, name), getattr(plain, name)), name
    assert all(np.array_equal(a, b) for a, b in zip(full.molecules, plain.molecules))
    assert full.temperatureAbsorption.shape == full.temperature.shape == (3,)
    assert np.array_equal(full.temperatureFull, full.temperature + full.temperatureAbsorption)
    lean = atm.jacobians(temperature="full", molecules=False, **kw)
    assert np.array_equal(lean.temperatureAbsorption, full.temperatureAbsorption) and lean.molecules is None
    told_apart = False
    for l, (L, (_, T, _)) in enumerate(zip(atm, LAYERS)):
        F = {}
        for d in (-2, -1, 1, 2):
            L.changeTemperature(T + d)
            F[d] = float(atm.jacobians(molecules=False, **kw).olr)
        L.changeTemperature(T)
        D1, D2 = (F[1] - F[-1]) / 2, (F[2] - F[-2]) / 4
        R = (4 * D1 - D2) / 3
        err = abs(full.temperatureFull[l] - R)
        print("layer %d, %d angle(s): full %.9e, Planck part %.9e, differences %.9e, |err| %.2e, |D1 - D2| %.2e"
              % (l, angles, full.temperatureFull[l], full.temperature[l], R, err, abs(D1 - D2)))
        assert err <= abs(D1 - D2) + 1e-6 * abs(R), (l, err, abs(D1 - D2))
        told_apart = told_apart or abs(full.temperatureAbsorption[l]) > 10 * abs(D1 - D2)
    assert told_apart, "the column cannot tell the full Jacobian from its Planck part"
    again = atm.jacobians(temperature="full", **kw)
    assert np.array_equal(again.temperatureAbsorption, full.temperatureAbsorption)


def test_too_many_terms_are_refused_before_the_device(pyrad):
    from pyrad_amd import _native as nat
    atm = pyrad.Atmosphere("terms")
    for depth, T, P in LAYERS:
        _layer(pyrad, atm, depth, T, P)
    limit = nat.limit("jacobian_terms")
    assert atm.jacobians(surfaceTemperature=288, temperature="full").temperatureFull.shape == (3,)      # 6 + 3 terms
    keep = nat.limit
    nat.limit = lambda name: 8 if name == "jacobian_terms" else keep(name)
    try:
        with pytest.raises(ValueError, match="dk/dT terms"):
            atm.jacobians(surfaceTemperature=288, temperature="full")
        assert atm.jacobians(surfaceTemperature=288).temperature.shape == (3,)                        # 6 terms pass
    finally:
        nat.limit = keep
    assert limit >= 9
