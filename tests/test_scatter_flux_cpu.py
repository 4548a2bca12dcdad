"""Thermal fluxes through scattering layers (lbl_column_flux_scatter_dev, Atmosphere.fluxesTwoStream) without a device:
the layer sources of tests/scatter_flux_ref.py against mpmath at 60 digits, against N isothermal sub-layers and against the
linear source without scatterers; the Kirchhoff cavity, the limits, the adding solution against a dense solve and a layer
against its halves; the declarations, the binding, the kernels' resource report and the model's validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scatter_flux_ref as ref
import twostream_ref as two
from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
ARGUMENTS = ("ctx n_layers abs_coef T planck_linear depth range_min range_max n I_surface surface_T I_top n_scat scat_amount "
             "scat_ext scat_ext_all scat_ssa scat_ssa_all scat_asym scat_asym_all delta_scaling n_bands band_first band_count "
             "emissivity emissivity_all workspace level_flux up_top down_surface up_surface").split()
MIXES = ((0.5, 2.0, 0.3), (3.0, 10.0, 0.5), (0.01, 0.0, 0.0), (1e-3, 5.0, 0.2))        # (ta, ts, g)


# ---- the layer sources ---------------------------------------------------------------------------------------------------
def test_sources_against_mpmath():
    """P, Q against 60 digits in the ungrouped form: at most 1e-13 of max(Bt, Bb), 200 times the 4.9e-16 that h alone
    showed"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    rs = np.random.RandomState(11)
    count = 2000
    t = 10.0 ** rs.uniform(-10, np.log10(200.0), count)
    ta = t * 10.0 ** rs.uniform(-12, 0, count)
    ts = t - ta
    tsg = ts * rs.uniform(-0.3, 0.6, count)
    Bt = rs.uniform(0.5, 2.0, count)
    Bb = Bt * rs.uniform(0.3, 3.0, count)
    _, _, _, P, Q = ref.sources(ta, ts, tsg, Bt, Bb)
    worst = 0.0
    for i in range(count):
        wp, wq = ref.sources_scalar(ta[i], ts[i], tsg[i], Bt[i], Bb[i], mp.mpf, mp.sqrt, mp.exp, mp.expm1)
        err = max(abs(mp.mpf(float(P[i])) - wp), abs(mp.mpf(float(Q[i])) - wq)) / max(Bt[i], Bb[i])
        worst = max(worst, float(err))
    print("P, Q against 60 digits on %d layers: worst %.2e of max(Bt, Bb)" % (count, worst))
    assert worst <= 1e-13


def sublayers(ta, ts, g, Bt, Bb, N):
    """what N isothermal sub-layers, each at the Planck value of its optical-depth midpoint, emit together: (P, Q)"""
    one = np.ones((N, 1))
    frac = (N - np.arange(N) - 0.5) / N                  # sub-layer i from the bottom: its midpoint's share of the way down
    B = (Bt + (Bb - Bt) * frac)[:, None]
    R, T, _, P, Q = ref.sources(ta / N * one, ts / N * one, ts * g / N * one, B, B)
    up, dn = ref.solve(R, T, P, Q, 1.0, 0.0, 0.0)        # over a black, cold surface and under a dark sky
    return up[N, 0], dn[0, 0]


@pytest.mark.parametrize("mix", MIXES)
def test_sources_are_the_limit_of_isothermal_sublayers(mix):
    ta, ts, g = mix
    Bt, Bb = 1.0, 1.5
    _, _, _, P, Q = ref.sources([ta], [ts], [ts * g], [Bt], [Bb])
    err = []
    for N in (64, 256):
        p, q = sublayers(ta, ts, g, Bt, Bb, N)
        err.append(max(abs(p - P[0]), abs(q - Q[0])))
    print("(ta, ts, g) = %r: error %.3e at N = 64, %.3e at N = 256, ratio %.2f" % (mix, err[0], err[1], err[0] / err[1]))
    assert 12.0 <= err[0] / err[1] <= 20.0


def linear_source_g(tau):
    """g(tau) = 1 - (1 - exp(-tau)) / tau as the linear source forms it: the expression from 0.25 on, its series below"""
    tau = np.asarray(tau, dtype=np.float64)
    series = np.zeros_like(tau)
    fact = 1.0
    for m in range(2, 14):
        fact *= m
    for m in range(13, 1, -1):                           # tau (1/2 - tau (1/6 - tau (1/24 - ...)))
        series = 1.0 / fact - tau * series
        fact /= m
    with np.errstate(all="ignore"):
        return np.where(tau < 0.25, tau * series, 1.0 - -np.expm1(-tau) / np.where(tau == 0, 1.0, tau))


def test_without_scatterers_it_is_the_linear_source():
    """R = 0, T = exp(-D ta): P and Q are (1 - t) Ba + g(tau) (Bb - Ba) at tau = D ta, Ba where the light enters.  The form
    with h alone, no series, stays inside 1e-13 of max(Bt, Bb) from tau = 1e-8 to 50, across the linear source's switch"""
    tau = np.concatenate([10.0 ** np.linspace(-8, np.log10(50.0), 400), [0.25 * (1 - 1e-15), 0.25, 0.25 * (1 + 1e-15)]])
    ta = tau / ref.D
    rs = np.random.RandomState(12)
    Bt = rs.uniform(0.5, 2.0, len(tau))
    Bb = Bt * rs.uniform(0.3, 3.0, len(tau))
    R, T, Ab, P, Q = ref.sources(ta, 0 * ta, 0 * ta, Bt, Bb)
    assert np.all(R == 0.0)
    tr, g = np.exp(-(ref.D * ta)), linear_source_g(ref.D * ta)
    assert np.max(np.abs(T - tr)) <= 2e-16
    want_P = -np.expm1(-(ref.D * ta)) * Bb + g * (Bt - Bb)           # upward: in at the bottom edge, out at the top
    want_Q = -np.expm1(-(ref.D * ta)) * Bt + g * (Bb - Bt)
    err = np.maximum(np.abs(P - want_P), np.abs(Q - want_Q)) / np.maximum(Bt, Bb)
    print("no scatterers: worst %.2e of max(Bt, Bb), at tau = %.3g" % (err.max(), tau[err.argmax()]))
    assert err.max() <= 1e-13


# ---- the column ----------------------------------------------------------------------------------------------------------
def small_column(rs, L, n, C_=2):
    k = 10.0 ** rs.uniform(-10, -2, (L, n))
    depth = np.full(L, 1e4)
    amount = 10.0 ** rs.uniform(-3, 1, (C_, L))
    numbers = [(rs.uniform(0.2, 2.0, n), rs.uniform(0.3, 1.0, n), rs.uniform(-0.3, 0.9, n)) for _ in range(C_)]
    return k, depth, amount, numbers


def test_kirchhoff_cavity():
    """one temperature everywhere, the sky included: up = dn = pi B(T0) at every level, whatever scatters and whatever e
    (in the restatement the layer source is the linear one with equal edges, so this covers both Planck settings)"""
    rs = np.random.RandomState(13)
    L, n, T0 = 6, 300, 255.0
    nu = np.linspace(600.0, 700.0, n)
    k, depth, amount, numbers = small_column(rs, L, n)
    B = ref.planck(nu, T0)
    worst = worst_net = 0.0
    for e in (0.0, 0.3, 1.0, rs.uniform(0, 1, n)):
        for delta in (0, 1):
            up, dn = ref.column(k, depth, nu, np.full((L, 2), T0), amount, numbers, delta, e, surface_T=T0, I_top=B)
            worst = max(worst, np.max(np.abs(up / (ref.PI * B) - 1)), np.max(np.abs(dn / (ref.PI * B) - 1)))
            worst_net = max(worst_net, np.max(np.abs(up - dn) / up))
    print("cavity: up and dn within %.2e of pi B, the net flux within %.2e of up" % (worst, worst_net))
    assert worst <= 1e-14 and worst_net <= 1e-14


def test_limits():
    rs = np.random.RandomState(14)
    n = 200
    ts = 10.0 ** rs.uniform(-8, 2, n)
    tsg = ts * rs.uniform(-0.3, 0.6, n)
    Bt, Bb = rs.uniform(0.5, 2.0, n), rs.uniform(0.5, 2.0, n)
    R, T, Ab, P, Q = ref.sources(np.zeros(n), ts, tsg, Bt, Bb)          # nothing absorbs: nothing emits, exactly
    assert np.all(P == 0.0) and np.all(Q == 0.0) and np.all(Ab == 0.0)
    assert np.max(np.abs(R + T - 1)) <= 4e-16
    R, T, Ab, P, Q = ref.sources(np.zeros(n), np.zeros(n), np.zeros(n), Bt, Bb)     # an empty layer passes everything
    assert np.all(R == 0.0) and np.all(T == 1.0) and np.all(P == 0.0) and np.all(Q == 0.0)
    nu = np.linspace(600.0, 700.0, n)
    k = np.zeros((3, n))
    up, dn = ref.column(k, np.full(3, 1e4), nu, [[280, 270], [270, 250], [250, 240]], emissivity=0.4, surface_T=290.0,
                        I_top=ref.planck(nu, 100.0))
    assert np.all(dn == ref.PI * ref.planck(nu, 100.0)) and np.all(up == up[0])


def test_adding_against_a_dense_solve():
    rs = np.random.RandomState(15)
    L, n = 7, 40
    nu = np.linspace(600.0, 700.0, n)
    k, depth, amount, numbers = small_column(rs, L, n)
    edges = np.column_stack([np.linspace(295, 225, L), np.linspace(285, 215, L)])
    e = rs.uniform(0, 1, n)
    I_top = ref.planck(nu, 150.0)
    up, dn = ref.column(k, depth, nu, edges, amount, numbers, 1, e, surface_T=300.0, I_top=I_top)
    ta, ts, tsg = two.optical(k, depth, amount, numbers, 1)
    worst = 0.0
    for j in range(n):
        lay = [ref.sources(ta[l, j:j + 1], ts[l, j:j + 1], tsg[l, j:j + 1], ref.PI * ref.planck(nu[j], edges[l, 1]),
                           ref.PI * ref.planck(nu[j], edges[l, 0])) for l in range(L)]
        R, T, _, P, Q = (np.array([v[q][0] for v in lay]) for q in range(5))
        du, dd = ref.dense(R, T, P, Q, e[j], ref.PI * ref.planck(nu[j], 300.0), ref.PI * I_top[j])
        scale = ref.PI * ref.planck(nu[j], 300.0)
        worst = max(worst, np.max(np.abs(du - up[:, j])) / scale, np.max(np.abs(dd - dn[:, j])) / scale)
    print("adding against the dense solve: worst %.2e of the largest pi B" % worst)
    assert worst <= 1e-13


def test_a_layer_against_its_halves():
    """a layer and its two halves joined by adding emit the same: the isothermal layer, and the linear one with the Planck
    value of the optical-depth midpoint at the edge between the halves"""
    rs = np.random.RandomState(16)
    n = 500
    t = 10.0 ** rs.uniform(-6, 2, n)
    ta = t * 10.0 ** rs.uniform(-6, 0, n)
    ts = t - ta
    tsg = ts * rs.uniform(-0.3, 0.6, n)
    Bt = rs.uniform(0.5, 2.0, n)
    for Bb, name in ((Bt, "isothermal"), (Bt * rs.uniform(0.3, 3.0, n), "linear")):
        _, _, _, P, Q = ref.sources(ta, ts, tsg, Bt, Bb)
        Bm = 0.5 * (Bt + Bb)
        lo = ref.sources(ta / 2, ts / 2, tsg / 2, Bm, Bb)
        hi = ref.sources(ta / 2, ts / 2, tsg / 2, Bt, Bm)
        R, T, _, Ph, Qh = (np.stack([a, b]) for a, b in zip(lo, hi))
        up, dn = ref.solve(R, T, Ph, Qh, 1.0, 0.0, 0.0)
        err = np.maximum(np.abs(up[2] - P), np.abs(dn[0] - Q)) / np.maximum(Bt, Bb)
        print("%s layer against its halves: worst %.2e of max(Bt, Bb)" % (name, err.max()))
        assert err.max() <= 1e-13


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    m = re.search(r"int\s+lbl_column_flux_scatter_dev\s*\(([^;]*)\)\s*;", text)
    assert m, "lbl_column_flux_scatter_dev is not declared"
    params = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert params == ARGUMENTS
    assert hasattr(lib, "lbl_column_flux_scatter_dev") and hasattr(lib, "lbl_column_flux_scatter_workspace")
    assert len(_native.SIGNATURES["lbl_column_flux_scatter_dev"][1]) == len(ARGUMENTS)
    assert len(_native.SIGNATURES["lbl_column_flux_scatter_workspace"][1]) == 3
    assert hasattr(_native.Context, "column_flux_scatter_dev") and hasattr(_native.Context, "column_flux_scatter_workspace")
    assert lib.lbl_abi_version() == 5
    # the workspace: four numbers per level and point, whole tiles of 256 points, one at least
    out = C.c_int64()
    for L, points, want in ((0, 0, 4 * 256), (0, 1, 4 * 256), (4, 256, 4 * 5 * 256), (4, 257, 4 * 5 * 512),
                            (128, 1000, 4 * 129 * 1024)):
        assert lib.lbl_column_flux_scatter_workspace(L, points, C.byref(out)) == 0 and out.value == want, (L, points)
    for L, points in ((-1, 1), (129, 1), (3, -1)):
        assert lib.lbl_column_flux_scatter_workspace(L, points, C.byref(out)) == -1
    assert lib.lbl_column_flux_scatter_workspace(3, 1, None) == -1


def test_scatter_flux_kernels_in_the_resource_report():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    mine = {n: f for n, f in k.items() if "scatter_flux" in n}
    for n, f in mine.items():
        print(n, f["VGPRs"], f["Occupancy [waves/SIMD]"])
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0 and f.get("SGPRs Spill") == 0, (n, f)
    # what launch_scatter_pass uses (K5m): the downward kernel for the layer and the linear source, one upward kernel
    down = sorted(re.search(r"scatter_flux_down_kernelILb(\d)EE", n).group(1) for n in mine if "down" in n)
    assert down == ["0", "1"] and len(mine) == 3 and sum("scatter_flux_up_kernel" in n for n in mine) == 1, sorted(mine)


# ---- validation ----------------------------------------------------------------------------------------------------------
def _atmosphere(layers=LAYERS):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("scatter flux")
    for depth, T, P in layers:
        atm.addLayer(depth, T, P, 600, 610)
    return atm


@pytest.fixture()
def no_context(monkeypatch):
    """every check below must fail before the engine (and with it a device context) is asked for"""
    def refuse():
        raise AssertionError("the context was touched before the arguments were validated")
    monkeypatch.setattr(model, "_ctx", refuse)
    settings.set_resolution_multiplier(1)
    yield


def test_validation_before_any_device_work(no_context):
    atm = _atmosphere()
    n = len(atm[0].xAxis)
    nan = float("nan")
    S = model.Scatterer
    four = [1.0, 0.0, 2.0, 0.5]
    call = lambda **kw: atm.fluxesTwoStream(**{"surfaceTemperature": 288.0, **kw})
    for bad in ([S(four)] * 5, [S([1.0, 2.0])], [S(four), "haze"], 7, [None]):
        with pytest.raises(ValueError, match="scatterers"):
            call(scatterers=bad)
    with pytest.raises(ValueError, match="extinction"):
        call(scatterers=[S(four, extinction=-1.0)])
    with pytest.raises(ValueError, match="singleScatteringAlbedo"):
        call(scatterers=[S(four, singleScatteringAlbedo=np.full(n, 1.0001))])
    with pytest.raises(ValueError, match="asymmetry"):
        call(scatterers=[S(four, asymmetry=1.0)])
    for d in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="deltaScaling"):
            call(deltaScaling=d)
    # what fluxes() refuses of the arguments the two share
    with pytest.raises(ValueError, match="surfaceSpectrum or surfaceTemperature"):
        atm.fluxesTwoStream()
    with pytest.raises(ValueError, match="surfaceTemperature"):
        call(surfaceTemperature=0.0)
    with pytest.raises(ValueError, match="surfaceSpectrum"):
        call(surfaceSpectrum=np.ones(n - 1))
    with pytest.raises(ValueError, match="topSpectrum"):
        call(topSpectrum=np.ones(n + 1))
    for e in (-0.1, 1.1, nan, "black", None, np.full(n, 1.5), np.ones(n - 1)):
        with pytest.raises(ValueError, match="emissivity"):
            call(emissivity=e)
    for p in ("isothermal", 1, None):
        with pytest.raises(ValueError, match="planck"):
            call(planck=p)
    with pytest.raises(ValueError, match="levelTemperatures"):
        call(levelTemperatures=[300, 290, 280, 270, 260])
    for lev in ([300, 290, 280, 270], [300, 290, 280, 270, nan], [300, 290, 280, 270, 0.0], "warm"):
        with pytest.raises(ValueError, match="levelTemperatures"):
            call(planck="linear", levelTemperatures=lev)
    for b in ([], [(650.0, 660.0)], [(600.0,)], [(605.0, 605.0)]):
        with pytest.raises(ValueError, match="bands"):
            call(bands=b)
    # the surface is Lambertian and the angle is the two-stream one: neither is an argument
    for kw in (dict(reflection="specular"), dict(angles=3)):
        with pytest.raises(TypeError):
            call(**kw)
