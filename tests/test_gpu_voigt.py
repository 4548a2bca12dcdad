"""GPU: the true Voigt line shape - lbl_voigt_function_dev and lbl_xsec_voigt_dev (kernels K2v) against the committed
fixture tests/golden/V0_voigt.npz (scipy.special.wofz through the Python oracle's geometry; made by
tests/golden/make_voigt_golden.py), the kernel's geometry and summation against sums formed in NumPy from the device
function's own values, determinism, the C ABI's refusals, and the model under settings.set_line_shape("voigt")."""
import json
import sys

import numpy as np
import pytest

from conftest import GOLDEN, RTOL_BASE, load_golden, point_tolerance, rel_err, rel_err_points
from oracle import pyrad_oracle as orc
from pyrad_amd import synthetic

sys.path.insert(0, GOLDEN)
import make_voigt_golden as mvg      # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG, STATE = -1, -6
Z = load_golden("V0_voigt")
CASES = json.loads(str(Z["cases"]))


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


def run(ctx, case, shard=None):
    j, g = job(ctx, case, shard)
    ctx.xsec_voigt_dev([j])
    xs = j[3].download(g["n_base"])
    j[0].free(); j[3].free()
    return xs, g


def function_dev(ctx, x, y):
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    bx, by, bo = ctx.buffer(x.size).upload(x), ctx.buffer(x.size).upload(y), ctx.buffer(x.size)
    ctx.voigt_function_dev(bx, by, x.size, bo)
    out = bo.download(x.size)
    for b in (bx, by, bo):
        b.free()
    return out


# ---- (a) the function ---------------------------------------------------------------------------------------------------
def test_function_on_the_fixture_table(ctx):
    X, Y = np.broadcast_arrays(Z["fx"][:, None], Z["fy"][None, :])
    worst = mvg.check_function(function_dev(ctx, X, Y), Z["fK"].ravel(), "table")
    worst = max(worst, mvg.check_function(function_dev(ctx, Z["rx"], Z["ry"]), Z["rK"], "random pairs"))
    worst = max(worst, mvg.check_function(function_dev(ctx, Z["bx"], Z["by"]), Z["bK"], "bands"))
    print("device voigt_k, worst relative error against the fixture: %.3e" % worst)
    nan = float("nan")
    assert np.isnan(function_dev(ctx, [nan, 1.0, nan, 20.0], [1.0, nan, 0.0, nan])).all()


# ---- (b) cross sections -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_cross_section_against_the_fixture(ctx, name):
    from pyrad_amd import engine
    case = mvg.load_case(Z, name)
    xs, g = run(ctx, case)
    ref = case["xsec"]
    assert xs.shape == ref.shape
    assert np.array_equal(xs == 0, ref == 0), "exact zeros must be matched by exact zeros"
    tol = 1e-6 + point_tolerance(engine.x_axis(case["lo"], case["hi"], case["base_resolution"]), case["T"], g["dfc"])
    err = rel_err_points(xs, ref)
    print("%s: worst relative error %.3e (W = %d, %d lines)" % (name, err.max(), g["W"], len(case["lines"]["nu"])))
    assert np.all(err <= tol), (name, float(err.max()))
    if name == "empty":
        assert not xs.any()
    if name == "isolated":
        assert np.count_nonzero(xs) == 2 * (g["W"] - 2) + 1


def test_regime_counts_keep_the_reference_meaning(ctx):
    case = mvg.load_case(Z, "p1")
    j, g = job(ctx, case)
    ctx.xsec_voigt_dev([j])
    molmass = mvg.case_physics(case)[0]
    lq = orc.line_quantities(case["lines"], case["T"], case["P"], case["q"], molmass, g["range_min"], g["resolution"])
    assert tuple(ctx.last_regime_counts(1)[0]) == tuple(np.bincount(lq["regime"], minlength=3))
    assert len(set(lq["regime"])) >= 2
    j[0].free(); j[3].free()


def test_shard_equals_the_same_points_of_the_whole(ctx):
    case = mvg.load_case(Z, "surface")
    whole, g = run(ctx, case)
    for first, count in ((130, 2777), (1, 63), (3999, 1)):           # off every tile, span and lane alignment
        part, _ = run(ctx, case, shard=(first, count))
        assert np.array_equal(part[first:first + count], whole[first:first + count])
        assert not part[:first].any() and not part[first + count:].any()      # nothing outside the shard is written


# ---- (c) geometry and summation, apart from the approximation ----------------------------------------------------------
@pytest.mark.parametrize("name", ["surface", "p100", "p1", "wide"])
def test_geometry_and_summation(ctx, name):
    """The kernel's sum against amp * K summed in line order in NumPy, K from lbl_voigt_function_dev at the very
    x = |d| * xs, y the kernel forms: what is left is the association of the kernel's multiply-add."""
    case = mvg.load_case(Z, name)
    j, g = job(ctx, case)
    assert g["n_work"] == g["n_base"]
    q = ctx.line_quantities(j[0], j[1], j[2])
    ctx.xsec_voigt_dev([j])
    xs = j[3].download(g["n_base"])
    j[0].free(); j[3].free()
    n, H = g["n_work"], max(g["W"] - 2, 0)
    sx = g["resolution"] / q["ghw"]
    y = q["lhw"] / q["ghw"]
    amp = q["intensity"] * (1.0 / (q["ghw"] * np.sqrt(np.pi)))
    spans = [(max(int(c) - H, 0), min(int(c) + H, n - 1)) for c in q["index"]]
    X = np.concatenate([np.abs(np.arange(lo, hi + 1) - int(c)).astype(np.float64) * sx[i] if hi >= lo else np.zeros(0)
                        for i, ((lo, hi), c) in enumerate(zip(spans, q["index"]))])
    Yv = np.concatenate([np.full(max(hi - lo + 1, 0), y[i]) for i, (lo, hi) in enumerate(spans)])
    K = function_dev(ctx, X, Yv)
    want = np.zeros(n)
    at = 0
    for i, (lo, hi) in enumerate(spans):
        if hi < lo:
            continue
        m = hi - lo + 1
        want[lo:hi + 1] += amp[i] * K[at:at + m]
        at += m
    worst = rel_err(xs, want)
    print("%s: kernel against line-order sums of the device function's values: %.3e" % (name, worst))
    assert worst <= RTOL_BASE


# ---- (d) determinism ---------------------------------------------------------------------------------------------------
def test_same_bits_twice_and_whatever_the_batch(ctx):
    cases = [mvg.load_case(Z, n) for n in ("p100", "surface", "p1")]
    alone = [run(ctx, c)[0] for c in cases]
    assert np.array_equal(run(ctx, cases[0])[0], alone[0])
    for order in ((0, 1, 2), (1, 2, 0), (2, 1, 0)):
        jobs = [job(ctx, cases[k])[0] for k in order]
        ctx.xsec_voigt_dev(jobs)
        for k, j in zip(order, jobs):
            assert np.array_equal(j[3].download(alone[k].size), alone[k]), order
            j[0].free(); j[3].free()


# ---- (e) refusals -------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable(ctx):
    from pyrad_amd import _native as nat, engine
    case = mvg.load_case(Z, "tiny")
    (L, iso, grid, out), g = job(ctx, case)
    lib, P = ctx.lib, nat._P
    one, isos, grids, outs = (P * 1)(L.h), (nat.IsoParams * 1)(iso), (nat.Grid * 1)(grid), (P * 1)(out.h)
    call = lambda *a: lib.lbl_xsec_voigt_dev(*a)      # noqa: E731
    assert call(None, 1, one, isos, grids, outs) == BAD_ARG
    for k in range(4):                                     # every array argument NULL in turn
        a = [one, isos, grids, outs]
        a[k] = None
        assert call(ctx.h, 1, *a) == BAD_ARG
    assert call(ctx.h, -1, one, isos, grids, outs) == BAD_ARG
    assert call(ctx.h, 65537, one, isos, grids, outs) == BAD_ARG                # LBL_MAX_JOBS + 1
    assert b"jobs per batch" in lib.lbl_last_error(ctx.h)
    assert call(ctx.h, 0, None, None, None, None) == 0                       # an empty batch, as lbl_xsec_accumulate_dev
    no_window = (nat.Grid * 1)(engine.native_grid(dict(g, W=0)))
    assert call(ctx.h, 1, one, isos, no_window, outs) == BAD_ARG and b"window" in lib.lbl_last_error(ctx.h)
    short = ctx.buffer(g["n_base"] - 1)
    assert call(ctx.h, 1, one, isos, grids, (P * 1)(short.h)) == BAD_ARG
    assert call(ctx.h, 1, one, isos, grids, (P * 1)(None)) == STATE
    assert call(ctx.h, 1, (P * 1)(None), isos, grids, outs) == STATE
    bad_iso = (nat.IsoParams * 1)(nat.IsoParams(0.0, iso.P, iso.q_frac, iso.molmass, iso.Q_T, iso.Q_296))
    assert call(ctx.h, 1, one, bad_iso, grids, outs) == BAD_ARG
    other = nat.Context(0)
    try:
        foreign = other.buffer(g["n_base"])
        assert call(ctx.h, 1, one, isos, grids, (P * 1)(foreign.h)) == STATE
        fl = other.lines(case["lines"])
        assert call(ctx.h, 1, (P * 1)(fl.h), isos, grids, outs) == STATE
        b = ctx.buffer(8)
        assert lib.lbl_voigt_function_dev(ctx.h, b.h, b.h, 8, foreign.h) == STATE
        fl.free(); foreign.free()
    finally:
        other.close()
    b, small = ctx.buffer(8), ctx.buffer(7)
    fn = lib.lbl_voigt_function_dev
    assert fn(ctx.h, b.h, b.h, 9, b.h) == BAD_ARG
    assert fn(ctx.h, b.h, small.h, 8, b.h) == BAD_ARG and fn(ctx.h, b.h, b.h, 8, small.h) == BAD_ARG
    assert fn(ctx.h, b.h, b.h, -1, b.h) == BAD_ARG and fn(ctx.h, None, b.h, 8, b.h) == BAD_ARG
    assert fn(None, b.h, b.h, 8, b.h) == BAD_ARG
    assert fn(ctx.h, b.h, b.h, 0, b.h) == 0
    # nothing was enqueued by any of them, and the context works
    assert not out.download(g["n_base"]).any()
    ctx.xsec_voigt_dev([(L, iso, grid, out)])
    assert np.all(rel_err_points(out.download(g["n_base"]), case["xsec"]) <= 2e-6)
    for o in (L, out, short, b, small):
        o.free()


# ---- (f) the model ------------------------------------------------------------------------------------------------------
LO, HI = 40.0, 40.004005                                  # 400 points at 1e-5 cm^-1
LAYERS = ((1e4, 288, 1013.25), (2e4, 250, 100.0), (5e4, 220, 0.05))
CENTRES = (40.001003, 40.002001, 40.003207)               # three lines inside the range, 100 and 120 points apart


def _narrow_lines(seed):
    """Far-infrared lines with small pressure widths: at 0.05 mbar lhw / ghw is about 5e-3 - the reference's Gaussian-only
    regime - while the window (23 points of 1e-5 cm^-1) reaches 4 to 6 Doppler widths, where exp(-x^2) has died and the
    Lorentz wing y / (sqrt(pi) x^2) is all there is."""
    L = synthetic.make_lines(seed, 40, 34.0, 46.0)
    inside = synthetic.make_lines(seed + 100, 3, 34.0, 46.0)
    inside["nu"] = np.array(CENTRES)
    L = mvg._concat(L, inside)
    L["gamma_air"] = L["gamma_air"] * 0.05
    L["gamma_self"] = L["gamma_self"] * 0.05
    return L


@pytest.fixture()
def pyrad():
    from pyrad_amd import model, data, settings
    model.Layer.hasAtmosphere = False
    settings.set_resolution_multiplier(.001)
    settings.set_layer_step("merged")
    settings.set_line_shape("reference")
    data.set_source(data.synthetic_source(dict(co2=_narrow_lines(31), h2o=_narrow_lines(32))))
    yield model
    settings.set_line_shape("reference")
    settings.set_resolution_multiplier(1)
    data.set_source(None)


def _column(pyrad):
    atm = pyrad.Atmosphere("voigt")
    for depth, T, P in LAYERS:
        L = atm.addLayer(depth, T, P, LO, HI, dynamicResolution=False)
        L.addMolecule("co2", ppm=400)
        L.addMolecule("h2o", percentage=0.5)
    return atm


def test_model_under_the_voigt_setting(pyrad):
    from pyrad_amd import settings, engine
    atm = _column(pyrad)
    n = len(atm[0].xAxis)
    assert n == 400 and len(atm) == 3
    ref_k = [np.array(L.absCoef) for L in atm]
    ref_t = np.array(atm.transmission(surfaceTemperature=288))
    ref_f = atm.fluxes(surfaceTemperature=288)
    counts = [iso.regimeCounts for m in atm[2] for iso in m]
    assert all(c[0] > 0 and c[1] == 0 and c[2] == 0 for c in counts)       # 0.05 mbar: the reference's Gaussian-only regime

    settings.set_line_shape("voigt")
    ctx = engine.get_engine().ctx
    k = [np.array(L.absCoef) for L in atm]
    # Layer.absCoef = sum_m f_m sum_iso of the ABI-level Voigt cross sections
    for L, got in zip(atm, k):
        want = np.zeros(n)
        for m in L:
            xs_m = np.zeros(n)
            for iso in m:
                out = ctx.buffer(n).fill(0.0)
                lines = ctx.lines(iso._lines)
                ctx.xsec_voigt_dev([(lines, pyrad._iso_params(iso), engine.native_grid(L._grid()), out)])
                xs_m = xs_m + out.download(n)
                lines.free(); out.free()
            want = want + orc.abs_coef(xs_m, m.concentration, L.P, L.T)
        assert rel_err(got, want) <= 1e-13
    # the fold over the downloaded coefficients
    x = atm[0].xAxis
    I = orc.planckWavenumber(x, 288)
    for L, kk in zip(atm, k):
        t = np.exp(-kk * L.depth)
        I = t * I + (1 - t) * orc.planckWavenumber(x, L.T)
    assert rel_err(atm.transmission(surfaceTemperature=288), I) <= 1e-13
    f = atm.fluxes(surfaceTemperature=288)
    assert np.isfinite(f.up).all() and f.up[-1] != ref_f.up[-1]
    print("F_up at the top: reference %.10e, voigt %.10e" % (ref_f.up[-1], f.up[-1]))
    # Between the lines of the 0.05 mbar layer: at x Doppler widths from a centre the Voigt profile stands above the bare
    # Gaussian by the factor 1 + y / (sqrt(pi) x^2 exp(-x^2)).  The widest line there is H2O's: ghw = 6.0e-5 cm^-1 (40 cm^-1,
    # 220 K, 18 u), y = lhw / ghw = 2.5e-3 .. 5e-3; for the smallest y the factor passes 10 at x = 3.3, and at x = 3.49 - 21
    # points of 1e-5 cm^-1 - it is 24 for H2O and far larger for CO2 (ghw = 3.8e-5, x = 5.5).  The window ends at 23 points.
    res = settings.BASE_RESOLUTION
    between = np.concatenate([int((c - LO) / res) + s * np.arange(21, 24) for c in CENTRES for s in (-1, 1)])
    assert np.all(ref_k[2][between] > 0)
    rise = k[2][between] / ref_k[2][between]
    print("0.05 mbar layer, between the lines: voigt / reference from %.3g to %.3g" % (rise.min(), rise.max()))
    assert np.all(rise > 10)
    assert [iso.regimeCounts for m in atm[2] for iso in m] == counts              # the counters stay the reference's

    settings.set_line_shape("reference")
    for L, before in zip(atm, ref_k):
        assert np.array_equal(L.absCoef, before)
    assert np.array_equal(atm.transmission(surfaceTemperature=288), ref_t)
    assert np.array_equal(atm.fluxes(surfaceTemperature=288).up, ref_f.up)
