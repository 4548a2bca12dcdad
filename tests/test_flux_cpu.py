"""CPU: the level-flux feature (Atmosphere.fluxes, lbl_column_flux_dev) without a device - the C ABI surface, the kernels'
resource report, the angle sets, the heating-rate arithmetic and the host-side validation, which runs before anything
touches a context."""
import os
import re

import numpy as np
import pytest

from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")


def test_entry_point_declared_exported_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    assert re.search(r"int\s+lbl_column_flux_dev\s*\(", text)
    lib = _native.load()
    assert hasattr(lib, "lbl_column_flux_dev")
    assert lib.lbl_abi_version() == 5
    assert _native.limit("flux_angles") == 8
    assert _native.limit("flux_bands") == 64


def test_flux_kernels_use_no_scratch_and_do_not_spill():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    flux = {n: f for n, f in k.items() if "column_flux_kernel" in n}
    final = {n: f for n, f in k.items() if "column_flux_final_kernel" in n}
    assert len(flux) == 16, sorted(flux)             # 4 and 1 points per thread x 1..8 angles
    assert len(final) == 1
    for n, f in {**flux, **final}.items():
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (n, f)
    one_angle = [f for n, f in flux.items() if "ILi4ELi1E" in n]
    assert one_angle and one_angle[0]["VGPRs"] <= 128     # the fold's occupancy class: four waves per SIMD


@pytest.mark.parametrize("N", range(1, 9))
def test_gauss_angles_integrate_polynomials_exactly(N):
    mu, w = model.fluxAngles(N)
    assert mu.shape == w.shape == (N,)
    assert np.all((mu > 0) & (mu <= 1))
    assert w.sum() == pytest.approx(np.pi, rel=1e-14)
    for m in range(0, 2 * N - 1):
        # sum_k W_k mu_k^m = 2 pi int_0^1 mu^m mu dmu = 2 pi / (m + 2)
        assert np.sum(w * mu ** m) == pytest.approx(2 * np.pi / (m + 2), rel=1e-13), m


def test_default_diffusivity_and_explicit_angle_sets():
    mu3, w3 = model.fluxAngles()
    assert np.array_equal(mu3, model.fluxAngles(3)[0]) and np.array_equal(w3, model.fluxAngles(3)[1])
    mu, w = model.fluxAngles("diffusivity")
    assert mu.tolist() == [1 / 1.66] and w.tolist() == [np.pi]
    mu, w = model.fluxAngles([(1.0, np.pi), (0.5, 0.25)])
    assert mu.tolist() == [1.0, 0.5] and w.tolist() == [np.pi, 0.25]


def test_heating_rate_against_a_hand_computation():
    net = np.array([240.0, 236.5, 231.0, 220.0])           # W m^-2 at levels 0..3
    P = [1000.0, 700.0, 300.0]                             # mbar
    T = [288.0, 260.0, 230.0]
    depth = [3.0e5, 4.0e5, 6.0e5]                          # cm
    got = model.heatingRates(net, P, T, depth)
    assert got.shape == (3,)
    for l in range(3):
        rho = 100.0 * P[l] / (287.05 * T[l])               # kg m^-3
        mass = rho * depth[l] / 100.0                      # kg m^-2
        want = -(net[l + 1] - net[l]) / (1004.0 * mass) * 86400.0
        assert got[l] == pytest.approx(want, rel=1e-15)
    # the net upward flux shrinks with height: every layer keeps energy and warms
    assert np.all(got > 0)
    # bands: the same per band
    two = model.heatingRates(np.stack([net, 2 * net]), P, T, depth)
    assert two.shape == (2, 3) and np.allclose(two[1], 2 * got, rtol=1e-15)
    assert (model.CP_AIR, model.R_DRY_AIR) == (1004.0, 287.05)


def _atmosphere(ranges=((600, 700), (600, 700))):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("validation")
    for i, (lo, hi) in enumerate(ranges):
        atm.addLayer(1e4 * (i + 1), 280 - 10 * i, 1000.0 / (i + 1), lo, hi)
    return atm


@pytest.fixture()
def no_context(monkeypatch):
    """every check below must fail before the engine (and with it a device context) is asked for"""
    def refuse():
        raise AssertionError("fluxes() touched the context before validating its arguments")
    monkeypatch.setattr(model, "_ctx", refuse)
    settings.set_resolution_multiplier(1)
    yield


def test_validation_before_any_device_work(no_context):
    with pytest.raises(ValueError, match="no layers"):
        model.Atmosphere("empty").fluxes(surfaceTemperature=288)
    with pytest.raises(ValueError, match="range"):
        _atmosphere(((600, 700), (600, 710))).fluxes(surfaceTemperature=288)
    atm = _atmosphere()
    with pytest.raises(ValueError, match="surface"):
        atm.fluxes()
    with pytest.raises(ValueError, match="surface"):
        atm.fluxes(topSpectrum=np.zeros(10000))
    for bad in (0, 9, -1, "isotropic", [(0.0, 1.0)], [(1.2, 1.0)], [(-0.5, 1.0)], [(0.5, 1.0)] * 9, [], [(0.5,)]):
        with pytest.raises(ValueError, match="angles"):
            atm.fluxes(surfaceTemperature=288, angles=bad)
    for bad in ([(500, 650)], [(650, 650)], [(650, 640)], [(701, 800)], [(650.0001, 650.0002)], [], [(650, 660)] * 65):
        with pytest.raises(ValueError, match="band"):
            atm.fluxes(surfaceTemperature=288, bands=bad)
    with pytest.raises(ValueError, match="surfaceSpectrum"):
        atm.fluxes(surfaceSpectrum=np.zeros(17))
    with pytest.raises(ValueError, match="topSpectrum"):
        atm.fluxes(surfaceTemperature=288, topSpectrum=np.zeros(17))


def test_band_index_ranges():
    n = 10000
    x = np.linspace(600, 700, n)
    first, count = model._flux_bands(600, 700, n, None)
    assert (first, count) == ([0], [n])
    first, count = model._flux_bands(600, 700, n, [(600, 650), (x[5001], x[5002]), (650, np.inf)])
    assert first == [0, 5001, int(np.searchsorted(x, 650))]
    assert count[1] == 1
    assert first[2] + count[2] == n                        # a band that ends beyond the range keeps the last point
    assert np.all(x[first[0]:first[0] + count[0]] < 650) and x[first[2]] >= 650
