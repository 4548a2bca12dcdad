"""CPU: the direct solar beam (Atmosphere.solarFluxes; lbl_column_solar_dev, kernels K5k) without a device - the C ABI
surface, the kernels' resource report, the host arithmetic (solarIrradiance, solarSlants) and the host-side validation,
which runs before anything touches a context."""
import os
import re

import numpy as np
import pytest

from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
DEPTHS = (1e4, 2e4, 5e4, 1e5)
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
ARGUMENTS = ("ctx n_layers abs_coef depth range_min range_max n S0 n_beams beam_weight slant n_angles mu weight n_bands "
             "band_first band_count emissivity emissivity_all reflection level_flux up_top down_surface up_surface").split()


def test_entry_point_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    m = re.search(r"int\s+lbl_column_solar_dev\s*\(([^;]*)\)\s*;", text)
    assert m, "lbl_column_solar_dev is not declared"
    params = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert params == ARGUMENTS
    assert hasattr(lib, "lbl_column_solar_dev")
    assert len(_native.SIGNATURES["lbl_column_solar_dev"][1]) == len(ARGUMENTS)
    assert hasattr(_native.Context, "column_solar_dev")
    assert lib.lbl_abi_version() == 5
    assert re.search(r"#define\s+LBL_ABI_VERSION\s+5\b", text)


def _template_args(name, kernel):
    m = re.search(kernel + r"I((?:Li\d+E)+)E", name)
    assert m, name
    return tuple(int(v) for v in re.findall(r"Li(\d+)E", m.group(1)))


def test_solar_kernels_in_the_resource_report():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    assert sorted({re.search(r"solar_\w+?_kernel", n).group(0) for n in k if "solar" in n}) == [
        "solar_beam_kernel", "solar_diffuse_kernel"]
    for sub in ("solar_beam_kernel", "solar_diffuse_kernel"):
        found = {_template_args(n, sub): f for n, f in k.items() if sub in n}
        # what launch_solar uses: 4 points per thread and 1 (head and tail) for 1..8 beams or angles, nothing else
        assert sorted(found) == [(np_, nb) for np_ in (1, 4) for nb in range(1, 9)], (sub, sorted(found))
        for args, f in found.items():
            print(sub, args, f["VGPRs"], f["Occupancy [waves/SIMD]"])
            assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (sub, args, f)
            # no source term to carry: four waves per SIMD at least, where K5g's eight-angle kernel has two
            assert f["Occupancy [waves/SIMD]"] >= 4, (sub, args, f)


# ---- host arithmetic ---------------------------------------------------------------------------------------------------
def test_solar_constant():
    """sigma T^4 (R_SUN / AU)^2 = 1361 W m^-2 at 5772 K: the sum over 1 .. 100000 cm^-1 at step 1 lies within 0.5 %"""
    assert (model.R_SUN, model.AU) == (6.957e8, 1.495978707e11)
    x = np.arange(1.0, 100001.0)
    S = model.solarIrradiance(x, 5772.0)
    assert S.shape == x.shape and np.all(np.isfinite(S)) and np.all(S >= 0)
    total = float(np.sum(S)) * 1.0
    assert abs(total - 1361.0) <= 0.005 * 1361.0, total
    assert np.array_equal(S, model.planckWavenumber(x, 5772.0) * np.pi * (model.R_SUN / model.AU) ** 2)
    # the inverse square of the distance, and the default temperature
    assert np.allclose(model.solarIrradiance(x, 5772.0, 2.0), S / 4.0, rtol=1e-15, atol=0.0)
    assert np.array_equal(model.solarIrradiance(x), S)
    assert model.solarIrradiance([0.0, 1000.0])[0] == 0.0
    for bad in (dict(temperature=0.0), dict(temperature=float("nan")), dict(distanceAU=0.0), dict(distanceAU=-1.0),
                dict(distanceAU=float("inf")), dict(temperature="hot")):
        with pytest.raises(ValueError):
            model.solarIrradiance(x, **bad)


def _slants_direct(depths, mu0, R):
    """the issue's formula in long double: (q(z_(l+1)) - q(z_l)) / depth_l, q(z) = sqrt(z (2 R + z) + R^2 mu0^2)"""
    z = np.concatenate([[0.0], np.cumsum(np.asarray(depths, dtype=np.longdouble))])
    R, m = np.longdouble(R), np.longdouble(mu0)
    q = np.sqrt(z * (2 * R + z) + R * R * m * m)
    return ((q[1:] - q[:-1]) / np.asarray(depths, dtype=np.longdouble)).astype(np.float64)


def test_solar_slants():
    L = len(DEPTHS)
    for geometry in model.SOLAR_GEOMETRIES:
        one = model.solarSlants(DEPTHS, 1.0, geometry)
        assert one.shape == (L,) and one.dtype == np.float64 and np.all(one == 1.0), (geometry, one)
        assert np.all(model.solarSlants(DEPTHS, 1, geometry, planetRadius=1.7e8) == 1.0)
    for mu0 in (0.9, 0.5, 0.2, 0.05, 1e-3):
        plane = model.solarSlants(DEPTHS, mu0)
        assert np.array_equal(plane, np.full(L, 1.0 / mu0))
        for R in (6.371e8, 3.4e8, 7e9):
            sph = model.solarSlants(DEPTHS, mu0, "spherical", R)
            assert sph.shape == (L,)
            assert np.all(sph <= 1.0 / mu0) and np.all(sph >= 1.0), (mu0, R, sph)
            assert np.all(np.diff(sph) < 0)                  # the higher the shell, the nearer the ray is to its normal
            # the factored form is the formula of the documentation (long double carries the difference of the distances)
            assert np.allclose(sph, _slants_direct(DEPTHS, mu0, R), rtol=1e-9, atol=0.0), (mu0, R)
    # the plane is the limit of a large planet
    for mu0 in (1.0, 0.8, 0.5):
        far = model.solarSlants(DEPTHS, mu0, "spherical", 1e15)
        assert np.all(np.abs(far * mu0 - 1.0) <= 1e-9), (mu0, far)
    # a list of beams gives a table, pairs as solarFluxes takes them
    table = model.solarSlants(DEPTHS, [(0.5, 1.0), (0.25, 3.0)], "spherical")
    assert table.shape == (2, L)
    assert np.array_equal(table[0], model.solarSlants(DEPTHS, 0.5, "spherical"))
    assert np.array_equal(table[1], model.solarSlants(DEPTHS, 0.25, "spherical"))
    assert model.solarSlants(DEPTHS, [(0.5, 1.0)]).shape == (1, L)


def _atmosphere(layers=LAYERS):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("solar")
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
    # both or neither source
    with pytest.raises(ValueError, match="exactly one"):
        atm.solarFluxes()
    with pytest.raises(ValueError, match="exactly one"):
        atm.solarFluxes(solarSpectrum=1.0, solarTemperature=5772.0)
    # the spectrum: negative, NaN, infinite, wrong shape, a bad table
    for S in (-1.0, nan, float("inf"), "sun", True, np.full(n, -1e-9), np.where(np.arange(n) == 5, np.nan, 1.0),
              np.full(n - 1, 1.0), np.full((2, n), 1.0), ([600.0, 605.0], [1.0, -1.0]), ([605.0, 600.0], [1.0, 1.0]),
              ([600.0, 605.0, 610.0], [1.0, 1.0]), ([600.0, 605.0], [1.0, nan])):
        with pytest.raises(ValueError, match="solarSpectrum"):
            atm.solarFluxes(solarSpectrum=S)
    for T in (0.0, -5.0, nan):
        with pytest.raises(ValueError, match="solarTemperature"):
            atm.solarFluxes(solarTemperature=T)
    with pytest.raises(ValueError, match="distanceAU"):
        atm.solarFluxes(solarTemperature=5772.0, distanceAU=0.0)
    # the beams
    nine = [(0.1 * (i + 1), 1.0) for i in range(9)]
    for m in (0.0, 1.0001, -0.5, nan, "noon", True, [], nine, [(0.5, nan)], [(0.5, -1.0)], [(0.5, float("inf"))], [(0.0, 1.0)],
              [(1.5, 1.0)], [0.5, 0.25, 0.1]):
        with pytest.raises(ValueError, match="mu0"):
            atm.solarFluxes(solarSpectrum=1.0, mu0=m)
    for g in ("sphere", "Plane", 0, None):
        with pytest.raises(ValueError, match="geometry"):
            atm.solarFluxes(solarSpectrum=1.0, geometry=g)
    for R in (0.0, -1.0, nan, float("inf"), "earth"):
        with pytest.raises(ValueError, match="planetRadius"):
            atm.solarFluxes(solarSpectrum=1.0, geometry="spherical", planetRadius=R)
    for e in (-0.01, 1.5, nan, "sand", np.full(n, 1.01), np.full(n - 1, 0.9), ([600.0, 605.0], [0.9, 1.2])):
        with pytest.raises(ValueError, match="emissivity"):
            atm.solarFluxes(solarSpectrum=1.0, emissivity=e)
    for r in ("mirror", "Lambertian", 0, None):
        with pytest.raises(ValueError, match="reflection"):
            atm.solarFluxes(solarSpectrum=1.0, reflection=r)
    for a in (0, 9, "gauss", [(1.5, 1.0)], [], [(0.5, 1.0), (0.25, -1.0)], [(0.5, 0.0)]):
        with pytest.raises(ValueError, match="angles"):
            atm.solarFluxes(solarSpectrum=1.0, emissivity=0.8, angles=a)
    x = atm[0].xAxis
    with pytest.raises(ValueError, match="bands"):
        atm.solarFluxes(solarSpectrum=1.0, bands=[(x[i], x[i + 1]) for i in range(65)])
    with pytest.raises(ValueError, match="bands"):
        atm.solarFluxes(solarSpectrum=1.0, bands=[])
    with pytest.raises(ValueError, match="no layers"):
        model.Atmosphere("empty").solarFluxes(solarSpectrum=1.0)
    # and a good call gets as far as the context, whichever way the source is given
    for kw in (dict(solarSpectrum=2.0), dict(solarTemperature=5772.0), dict(solarSpectrum=np.full(n, 1.0)),
               dict(solarSpectrum=([600.0, 610.0], [1.0, 2.0]), mu0=[(0.5, 0.25), (0.25, 0.75)], geometry="spherical",
                    emissivity=([600.0, 610.0], [0.9, 0.8]), reflection="specular", angles="diffusivity",
                    bands=[(600, 605), (605, 611)], spectra=True)):
        with pytest.raises(AssertionError, match="context"):
            atm.solarFluxes(**kw)


def test_solar_spectrum_forms(no_context):
    atm = _atmosphere()
    x = np.asarray(atm[0].xAxis)
    n = x.size
    S = model._solar_spectrum(3.0, None, 1.0, x)
    assert S.dtype == np.float64 and S.flags.c_contiguous and np.array_equal(S, np.full(n, 3.0))
    arr = np.linspace(0.0, 2.0, n)
    assert np.array_equal(model._solar_spectrum(arr, None, 1.0, x), arr)
    nu, val = [598.0, 603.0, 604.0, 612.0], [1.0, 0.5, 0.75, 0.1]
    assert np.array_equal(model._solar_spectrum((nu, val), None, 1.0, x), np.interp(x, nu, val))
    assert np.array_equal(model._solar_spectrum(None, 5000.0, 1.5, x), model.solarIrradiance(x, 5000.0, 1.5))
    mu, w = model._solar_beams(0.25)
    assert np.array_equal(mu, [0.25]) and np.array_equal(w, [1.0])
    mu, w = model._solar_beams([(0.5, 0.25), (1.0, 0.0)])
    assert np.array_equal(mu, [0.5, 1.0]) and np.array_equal(w, [0.25, 0.0])
