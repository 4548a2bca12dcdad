"""CPU: two-stream multiple scattering (Atmosphere.solarFluxesTwoStream; lbl_column_twostream_dev, kernels K5l) without a
device - the NumPy restatement the GPU tests compare with (tests/twostream_ref.py) against mpmath, its energy balance, the
adding solution against a dense solve and a layer against its halves; the kernels' resource report, the binding, the
Rayleigh numbers and the host-side validation, which runs before anything touches a context.

Bounds of the restatement's own error (float64 against 60 digits, the issue's prototype on 6,000 layers: 2.6e-14 for Rb and
Tb, 5e-16 for R and T, growing as 1e-17 / |1 - lam m|, so 1e-14 at the 1e-3 kept here): 1e-13 for Rb, Tb and Td and 2e-15
for R and T - four times the prototype's figures, since other random layers are drawn here.  Measured worst of this file's
2,000 layers: R 3.5e-16, T 2.7e-16, Td 8.6e-17, Rb 5.9e-16, Tb 1.6e-15 (mpmath evaluates the form that is not regrouped)."""
import os
import re

import numpy as np
import pytest

import twostream_ref as ref
from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
ARGUMENTS = ("ctx n_layers abs_coef depth range_min range_max n S0 n_beams beam_weight slant n_scat scat_amount scat_ext "
             "scat_ext_all scat_ssa scat_ssa_all scat_asym scat_asym_all delta_scaling n_bands band_first band_count emissivity "
             "emissivity_all workspace level_flux up_top down_surface direct_surface up_surface").split()


def random_layers(rs, count):
    """the issue's ranges: t 1e-8 .. 200, absorbed share down to 1e-15, g -0.3 .. 0.6, m 0.02 .. 1"""
    t = 10.0 ** rs.uniform(-8, np.log10(200.0), count)
    share = 10.0 ** rs.uniform(-15, 0, count)
    ta = t * share
    ts = t - ta
    tsg = ts * rs.uniform(-0.3, 0.6, count)
    slant = 1.0 / rs.uniform(0.02, 1.0, count)
    return ta, ts, tsg, slant


def test_restatement_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    rs = np.random.RandomState(3)
    ta, ts, tsg, slant = random_layers(rs, 2000)
    worst = dict(R=0.0, T=0.0, Td=0.0, Rb=0.0, Tb=0.0)
    used = 0
    for i in range(len(ta)):
        R, T, Td, Rb, Tb, pole = ref.layer(ta[i:i + 1], ts[i:i + 1], tsg[i:i + 1], slant[i:i + 1])
        if pole[0, 0] < 1e-3:
            continue
        used += 1
        want = ref.layer_scalar(ta[i], ts[i], tsg[i], slant[i], mp.mpf, mp.sqrt, mp.exp, mp.expm1)
        got = dict(R=R[0], T=T[0], Td=Td[0, 0], Rb=Rb[0, 0], Tb=Tb[0, 0])
        for name, w in zip(("R", "T", "Td", "Rb", "Tb"), want):
            worst[name] = max(worst[name], float(abs(mp.mpf(float(got[name])) - w)))
    print("layers %d of %d," % (used, len(ta)), " ".join("%s %.2e" % kv for kv in worst.items()))
    assert used >= 0.97 * len(ta)
    assert worst["R"] <= 2e-15 and worst["T"] <= 2e-15, worst
    assert max(worst["Rb"], worst["Tb"], worst["Td"]) <= 1e-13, worst


def conservative_layers():
    rs = np.random.RandomState(4)
    count = 500
    ts = 10.0 ** rs.uniform(-8, np.log10(200.0), count)
    return count, ts, ts * rs.uniform(-0.3, 0.6, count), 1.0 / np.array([0.05, 0.3, 0.5, 1.0])


def test_diffuse_energy_is_conserved_without_absorption():
    """R + T == 1 within 2 ulp at ta = 0, 1e-300 and 1e-30 (measured: 1 ulp here, 2 ulp over 120,000 layers)"""
    count, ts, tsg, slant = conservative_layers()
    for ta in (0.0, 1e-300, 1e-30):
        R, T = ref.layer(np.full(count, ta), ts, tsg, slant)[:2]
        diffuse = np.max(np.abs((R + T) - 1.0))
        print("ta = %g: R + T - 1 %.2e (%.1f ulp of 1)" % (ta, diffuse, diffuse / 2.0 ** -52))
        assert diffuse <= 2 * 2.0 ** -52


def test_beam_energy_is_conserved_without_absorption():
    """Rb + Tb + Td == 1 within 2 ulp at ta = 0, 1e-300 and 1e-30 (measured: 1, 1 and 2 ulp here).  The header's regrouped
    form is what holds this: with Rb and Tb written out as three products of Cp and Cm each the sum was up to 3.3 ulp off."""
    count, ts, tsg, slant = conservative_layers()
    worst = 0.0
    for ta in (0.0, 1e-300, 1e-30):
        R, T, Td, Rb, Tb, pole = ref.layer(np.full(count, ta), ts, tsg, slant)
        assert np.all(pole >= 1e-3)
        beam = np.max(np.abs(((Rb + Tb) + Td) - 1.0))
        print("ta = %g: Rb + Tb + Td - 1 %.2e (%.1f ulp of 1)" % (ta, beam, beam / 2.0 ** -52))
        worst = max(worst, beam)
    assert worst <= 2 * 2.0 ** -52


def small_column(rs, L, n, S=2, C=2):
    k = 10.0 ** rs.uniform(-10, -2, (L, n))
    depth = rs.uniform(0.5e4, 2e4, L)
    amount = rs.uniform(0.0, 2.0, (C, L))
    numbers = [(rs.uniform(0.1, 2.0, n), rs.uniform(0.5, 1.0, n), rs.uniform(-0.2, 0.85, n)) for _ in range(C)]
    slant = 1.0 / rs.uniform(0.1, 0.55, (S, 1)) * np.ones((S, L))
    return k, depth, rs.uniform(0.5, 1.5, n), rs.uniform(0.1, 0.4, S), slant, amount, numbers


def test_adding_against_a_dense_solve():
    rs = np.random.RandomState(5)
    L, n = 6, 40
    k, depth, S0, bw, slant, amount, numbers = small_column(rs, L, n)
    e = rs.uniform(0.0, 1.0, n)
    up, dn, direct, _ = ref.column(k, depth, S0, bw, slant, amount, numbers, 1, e)
    ta, ts, tsg = ref.optical(k, depth, amount, numbers, 1)
    worst = 0.0
    for j in range(n):
        R, T, P, Q = (np.zeros(L) for _ in range(4))
        Sb = np.tile(S0[j], len(bw))
        for l in range(L - 1, -1, -1):
            r, t, Td, Rb, Tb, _ = ref.layer(ta[l, j:j + 1], ts[l, j:j + 1], tsg[l, j:j + 1], slant[:, l])
            R[l], T[l] = r[0], t[0]
            P[l], Q[l] = np.sum(Rb[:, 0] * bw * Sb), np.sum(Tb[:, 0] * bw * Sb)
            Sb = Td[:, 0] * Sb
        u, d = ref.dense(R, T, P, Q, e[j], direct[0, j])
        scale = np.sum(bw) * S0[j]
        worst = max(worst, np.max(np.abs(u - up[:, j])) / scale, np.max(np.abs(d - dn[:, j])) / scale)
    print("adding against numpy.linalg.solve: %.2e of the incident flux" % worst)
    assert worst <= 2e-14          # (the issue's prototype: 9e-16; a dense solve of 14 unknowns loses a digit more at worst)


def test_a_layer_against_its_halves_and_conservation():
    rs = np.random.RandomState(6)
    n = 200
    k, depth, S0, bw, slant, amount, numbers = small_column(rs, 1, n)
    e = 0.3
    one = ref.column(k, depth, S0, bw, slant, amount, numbers, 1, e)
    two = ref.column(np.vstack([k, k]), [depth[0] / 2] * 2, S0, bw, np.hstack([slant, slant]), np.hstack([amount / 2] * 2),
                     numbers, 1, e)
    scale = np.sum(bw) * S0
    worst = max(np.max(np.abs(one[q][i] - two[q][2 * i]) / scale) for q in range(3) for i in (0, 1))
    print("one layer against its halves: %.2e of the incident flux" % worst)
    assert worst <= 5e-14          # (the prototype: 7.7e-15)
    # no absorption anywhere: the net flux is the same at every level
    L = 5
    k, depth, S0, bw, slant, amount, numbers = small_column(rs, L, n)
    numbers = [(ext, 1.0, g) for ext, _, g in numbers]
    up, dn, direct, _ = ref.column(np.zeros((L, n)), depth, S0, bw, slant, amount, numbers, 1, 0.2)
    net = (dn + direct) - up
    worst = np.max(np.abs(net - net[L]) / (np.sum(bw) * S0))
    print("net flux over conservative columns: constant to %.2e" % worst)
    assert worst <= 1e-14          # (the prototype: 7e-16 on its columns)


def test_long_double_agrees_with_float64():
    """the restatement in long double (the judge of the points near the pole) is the float64 one to rounding elsewhere"""
    rs = np.random.RandomState(7)
    k, depth, S0, bw, slant, amount, numbers = small_column(rs, 4, 300)
    a = ref.column(k, depth, S0, bw, slant, amount, numbers, 1, 0.4)
    b = ref.column(k, depth, S0, bw, slant, amount, numbers, 1, 0.4, dtype=np.longdouble)
    for q in range(3):
        assert np.max(np.abs(a[q] - b[q].astype(np.float64))) <= 1e-13


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    m = re.search(r"int\s+lbl_column_twostream_dev\s*\(([^;]*)\)\s*;", text)
    assert m, "lbl_column_twostream_dev is not declared"
    params = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert params == ARGUMENTS
    assert hasattr(lib, "lbl_column_twostream_dev") and hasattr(lib, "lbl_column_twostream_workspace")
    assert len(_native.SIGNATURES["lbl_column_twostream_dev"][1]) == len(ARGUMENTS)
    assert len(_native.SIGNATURES["lbl_column_twostream_workspace"][1]) == 3
    assert hasattr(_native.Context, "column_twostream_dev") and hasattr(_native.Context, "column_twostream_workspace")
    assert lib.lbl_abi_version() == 5
    assert _native.limit("scatterers") == 4 == model.MAX_SCATTERERS
    # the workspace: five numbers per level and point, whole tiles of 256 points, one at least
    import ctypes as C
    out = C.c_int64()
    for L, points, want in ((0, 0, 5 * 256), (0, 1, 5 * 256), (4, 256, 5 * 5 * 256), (4, 257, 5 * 5 * 512),
                            (128, 1000, 5 * 129 * 1024)):
        assert lib.lbl_column_twostream_workspace(L, points, C.byref(out)) == 0 and out.value == want, (L, points)
    for L, points in ((-1, 1), (129, 1), (3, -1)):
        assert lib.lbl_column_twostream_workspace(L, points, C.byref(out)) == -1
    assert lib.lbl_column_twostream_workspace(3, 1, None) == -1


def test_twostream_kernels_in_the_resource_report():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    mine = {n: f for n, f in k.items() if "twostream" in n}
    assert sorted({re.search(r"twostream_\w+?_kernel", n).group(0) for n in mine}) == [
        "twostream_down_kernel", "twostream_up_kernel"]
    down = {}
    for n, f in mine.items():
        print(n, f["VGPRs"], f["Occupancy [waves/SIMD]"])
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (n, f)
        m = re.search(r"twostream_down_kernelILi(\d+)EE", n)
        if m:
            down[int(m.group(1))] = f
    # what launch_scatter_pass uses (K5l): one downward instantiation per beam count 1 .. 8, one upward kernel
    assert sorted(down) == list(range(1, 9)) and len(mine) == 9, sorted(mine)


# ---- Rayleigh ------------------------------------------------------------------------------------------------------------
def test_rayleigh_numbers():
    sigma = model.rayleighCrossSection(1e4 / 0.55)
    assert abs(float(sigma) - 4.51e-27) <= 0.005 * 4.51e-27, sigma
    x = np.array([0.0, 1000.0, 1e4 / 0.5, 1e4 / 0.4999, 1e4 / 0.3])
    s = model.rayleighCrossSection(x)
    assert s.shape == x.shape and s[0] == 0.0 and np.all(np.diff(s) > 0)
    assert abs(s[2] / s[3] - 1.0) < 2e-3                  # the two ranges meet at 0.5 micrometres
    # a 1013.25 mbar, 288 K column of 2.15e25 molecules cm^-2 (about 8.4 km): optical depth 0.097 at 0.55 micrometres
    model.Layer.hasAtmosphere = False
    settings.set_resolution_multiplier(1)
    atm = model.Atmosphere("air")
    per_cm = 100.0 * 1013.25 / (model.k * 288.0) * 1e-6
    atm.addLayer(2.15e25 / per_cm, 288, 1013.25, 18181, 18182)
    sc = model.rayleighScatterer(atm)
    assert sc.amounts.shape == (1,) and abs(sc.amounts[0] - 2.15e25) <= 1e-12 * 2.15e25
    assert sc.singleScatteringAlbedo == 1.0 and sc.asymmetry == 0.0
    depth = sc.amounts[0] * np.interp(1e4 / 0.55, atm[0].xAxis, sc.extinction)
    assert abs(depth - 0.097) <= 0.03 * 0.097, depth


# ---- validation ----------------------------------------------------------------------------------------------------------
def _atmosphere(layers=LAYERS):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("twostream")
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
    nan, inf = float("nan"), float("inf")
    S = model.Scatterer
    four = [1.0, 0.0, 2.0, 0.5]
    for amounts in ([1.0, -1.0, 0.0, 0.0], [1.0, nan, 0.0, 0.0], [inf, 0.0, 0.0, 0.0], "cloud", 3.0, [1.0, "a", 0.0, 0.0]):
        with pytest.raises(ValueError, match="amounts"):
            S(amounts)
    call = lambda **kw: atm.solarFluxesTwoStream(solarSpectrum=1.0, **kw)
    for bad in ([S(four)] * 5, [S([1.0, 2.0])], [S(four), "haze"], 7, [None]):
        with pytest.raises(ValueError, match="scatterers"):
            call(scatterers=bad)
    for ext in (-1.0, nan, inf, "thick", True, None, np.full(n, -1e-9), np.full(n - 1, 1.0), ([600.0, 605.0], [1.0, -1.0]),
                ([605.0, 600.0], [1.0, 1.0])):
        with pytest.raises(ValueError, match="extinction"):
            call(scatterers=[S(four, extinction=ext)])
    for ssa in (-0.01, 1.01, nan, "white", np.full(n, 1.0001), np.full((2, n), 0.5), ([600.0, 605.0], [0.5, 1.5])):
        with pytest.raises(ValueError, match="singleScatteringAlbedo"):
            call(scatterers=[S(four, singleScatteringAlbedo=ssa)])
    for g in (-1.0, 1.0, 1.5, nan, "forward", np.full(n, 1.0), np.full(n + 1, 0.5), ([600.0, 605.0], [0.5, -1.0])):
        with pytest.raises(ValueError, match="asymmetry"):
            call(scatterers=[S(four, asymmetry=g)])
    for d in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="deltaScaling"):
            call(deltaScaling=d)
    # what solarFluxes refuses of the arguments the two share
    with pytest.raises(ValueError, match="exactly one"):
        atm.solarFluxesTwoStream()
    with pytest.raises(ValueError, match="exactly one"):
        atm.solarFluxesTwoStream(solarSpectrum=1.0, solarTemperature=5772.0)
    for bad in (-1.0, nan, np.full(n - 1, 1.0)):
        with pytest.raises(ValueError, match="solarSpectrum"):
            atm.solarFluxesTwoStream(solarSpectrum=bad)
    with pytest.raises(ValueError, match="solarTemperature"):
        atm.solarFluxesTwoStream(solarTemperature=0.0)
    with pytest.raises(ValueError, match="distanceAU"):
        atm.solarFluxesTwoStream(solarTemperature=5772.0, distanceAU=0.0)
    for m in (0.0, 1.0001, nan, [], [(0.1 * (i + 1), 1.0) for i in range(9)], [(0.5, -1.0)]):
        with pytest.raises(ValueError, match="mu0"):
            call(mu0=m)
    with pytest.raises(ValueError, match="geometry"):
        call(geometry="sphere")
    with pytest.raises(ValueError, match="planetRadius"):
        call(geometry="spherical", planetRadius=0.0)
    for e in (-0.01, 1.5, nan, np.full(n - 1, 0.9)):
        with pytest.raises(ValueError, match="emissivity"):
            call(emissivity=e)
    with pytest.raises(ValueError, match="bands"):
        call(bands=[])
    with pytest.raises(ValueError, match="no layers"):
        model.Atmosphere("empty").solarFluxesTwoStream(solarSpectrum=1.0)
    for name in ("reflection", "angles"):              # Lambertian, one stream: neither is an argument
        with pytest.raises(TypeError):
            call(**{name: 3})
    # and a good call gets as far as the context
    cloud = S(four, extinction=np.full(n, 2.0), singleScatteringAlbedo=([600.0, 610.0], [0.9, 0.99]), asymmetry=0.85, name="cloud")
    for kw in (dict(), dict(scatterers=cloud), dict(scatterers=[model.rayleighScatterer(atm), cloud], deltaScaling=False,
                                                     mu0=[(0.5, 0.25), (0.25, 0.75)], geometry="spherical",
                                                     emissivity=([600.0, 610.0], [0.9, 0.8]), bands=[(600, 605), (605, 611)],
                                                     spectra=True)):
        with pytest.raises(AssertionError, match="context"):
            call(**kw)
