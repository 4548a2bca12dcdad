"""CPU: the instrument-channel feature (Instrument, convolve, brightnessTemperature, Atmosphere.observe,
lbl_ils_convolve_dev) without a device - the C ABI surface, the kernels' resource report, the host-side validation, which
runs before anything touches a context, the channel supports and the inverse Planck function."""
import os
import re

import numpy as np
import pytest

from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")


def test_entry_point_declared_exported_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    assert re.search(r"int\s+lbl_ils_convolve_dev\s*\(", text)
    lib = _native.load()
    assert hasattr(lib, "lbl_ils_convolve_dev")
    assert lib.lbl_abi_version() == 5
    assert _native.limit("ils_rows") == 512
    assert _native.limit("ils_channels") == 65536
    assert _native.limit("ils_table") == 4096
    with open(os.path.join(_native.CSRC, "lbl_device.h")) as fh:
        assert re.search(r"kIlsRowBlock\s*=\s*%d\s*;" % _native.ILS_ROW_BLOCK, fh.read())


def test_ils_kernels_use_no_scratch_and_do_not_spill():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    ils = {n: f for n, f in k.items() if "ils_convolve_kernel" in n}
    assert len(ils) == 10, sorted(ils)                 # five shapes x (one row, a block of rows)
    for n, f in ils.items():
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (n, f)
        assert f["VGPRs"] <= 128, (n, f)               # four waves per SIMD at least


@pytest.fixture()
def no_context(monkeypatch):
    """every check below must fail before the engine (and with it a device context) is asked for"""
    def refuse():
        raise AssertionError("the context was touched before the arguments were validated")
    monkeypatch.setattr(model, "_ctx", refuse)
    settings.set_resolution_multiplier(1)
    yield


def _atmosphere(lo=600, hi=700):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("validation")
    for i in range(2):
        atm.addLayer(1e4 * (i + 1), 280 - 10 * i, 1000.0 / (i + 1), lo, hi)
    return atm


def test_instrument_validation():
    I = model.Instrument
    for bad in ([], [[600.0, 601.0]], [600.0, np.nan], [np.inf], "abc"):
        with pytest.raises(ValueError, match="centres"):
            I(bad, width=0.5)
    for bad in (0.0, -1.0, np.nan, [0.5, 0.0], [0.5, 0.5, 0.5]):
        with pytest.raises(ValueError, match="width"):
            I([650.0, 651.0], width=bad)
    with pytest.raises(ValueError, match="width"):
        I([650.0])
    with pytest.raises(ValueError, match="cutoff"):
        I([650.0], shape="sinc", width=0.25)
    with pytest.raises(ValueError, match="cutoff"):
        I([650.0], width=0.25, cutoff=0.0)
    with pytest.raises(ValueError, match="shape"):
        I([650.0], shape="lorentz", width=0.25)
    x = np.linspace(-1, 1, 21)
    for offsets in (np.r_[x[:-1], 1.05], x ** 3, x + 0.1, x[::-1], x[:1]):
        with pytest.raises(ValueError, match="table"):
            I([650.0], shape="table", table=(offsets, np.ones(offsets.size)))
    with pytest.raises(ValueError, match="table"):
        I([650.0], shape="table")
    with pytest.raises(ValueError, match="table"):
        I([650.0], shape="table", table=(x, np.ones(20)))
    with pytest.raises(ValueError, match="table"):
        I([650.0], shape="gaussian", width=0.5, table=(x, np.ones(21)))
    # the defaults
    assert I([650.0], width=0.5).cutoff.tolist() == [1.5]
    assert I([650.0], shape="triangle", width=0.5).cutoff.tolist() == [0.5]
    assert I([650.0], shape="boxcar", width=0.5).cutoff.tolist() == [0.25]
    assert I([650.0, 660.0], shape="sinc", width=[0.5, 0.25], cutoff=4).cutoff.tolist() == [4.0, 4.0]
    t = I([650.0], shape="table", table=(x, 1 - x * x))
    assert t.cutoff.tolist() == [1.0] and t.tableHalf == 1.0 and t.width is None


def test_channels_must_lie_inside_the_range():
    n = 10000
    for centres, which in (([650.0, 600.7], 1), ([699.3, 650.0], 0), ([650.0, 650.0, 599.0], 2), ([701.0], 0)):
        with pytest.raises(ValueError, match="channel %d " % which):
            model.Instrument(centres, width=0.5).support(600, 700, n)
    # a cutoff that misses every grid point
    with pytest.raises(ValueError, match="channel 1 .*no grid point"):
        x = np.linspace(600, 700, n)
        model.Instrument([x[5000], 0.5 * (x[5000] + x[5001])], shape="boxcar", width=0.002).support(600, 700, n)


def test_observe_validation_before_any_device_work(no_context):
    ins = model.Instrument(np.arange(610.0, 690.0, 0.5), width=0.5)
    with pytest.raises(ValueError, match="no layers"):
        model.Atmosphere("empty").observe(ins, surfaceTemperature=288)
    atm = _atmosphere()
    with pytest.raises(ValueError, match="instrument"):
        atm.observe([650.0], surfaceTemperature=288)
    with pytest.raises(ValueError, match="surface"):
        atm.observe(ins)
    with pytest.raises(ValueError, match="surfaceTemperature"):
        atm.observe(ins, surfaceTemperature=0)
    with pytest.raises(ValueError, match="surfaceSpectrum"):
        atm.observe(ins, surfaceSpectrum=np.zeros(17))
    for bad in (0, 0.0, -0.5, 1.0001, np.nan, "nadir"):
        with pytest.raises(ValueError, match="mu"):
            atm.observe(ins, surfaceTemperature=288, mu=bad)
    for centres in ([600.5], [699.5], [650.0, 720.0]):
        with pytest.raises(ValueError, match="channel"):
            atm.observe(model.Instrument(centres, width=0.5), surfaceTemperature=288, jacobians=True)
    with pytest.raises(ValueError, match="instrument"):
        model.convolve(None, np.zeros(100), 600, 700)
    with pytest.raises(ValueError, match="spectra"):
        model.convolve(ins, np.zeros((2, 3, 100)), 600, 700)
    with pytest.raises(ValueError, match="channel"):
        model.convolve(model.Instrument([600.5], width=0.5), np.zeros(10000), 600, 700)


def _brute_force(x, centre, cutoff):
    inside = np.flatnonzero(np.abs(x - centre) <= cutoff)
    assert inside.size and np.array_equal(inside, np.arange(inside[0], inside[-1] + 1))
    return int(inside[0]), int(inside.size)


@pytest.mark.parametrize("lo,hi,n", [(600.0, 604.0, 4001), (600.0, 700.0, 10000), (100.0, 2500.0, 24000)])
def test_support_against_a_brute_force_mask(lo, hi, n):
    x = np.linspace(lo, hi, n)
    step = (hi - lo) / (n - 1)
    j = n // 3
    cases = [
        (x[j], 0.4 * step),                            # a cutoff below one step around a grid point: that point alone
        (x[j], 5 * step),                              # a centre exactly on a grid point, the ends on grid points too
        (x[j], 5.5 * step),
        (0.5 * (x[j] + x[j + 1]), 0.6 * step),         # a centre midway between two grid points: both of them
        (0.5 * (x[j] + x[j + 1]), 10.25 * step),
        (lo + 0.0625, 0.0625),                         # a support touching point 0 ...
        (hi - 0.0625, 0.0625),                         # ... and point n - 1
    ]
    centres = np.array([c for c, _ in cases])
    cutoff = np.array([k for _, k in cases])
    ins = model.Instrument(centres, shape="boxcar", width=2 * cutoff)
    assert np.array_equal(ins.cutoff, cutoff)
    position, first, count = ins.support(lo, hi, n)
    assert np.array_equal(position, (centres - lo) / step)
    for c in range(len(cases)):
        assert (int(first[c]), int(count[c])) == _brute_force(x, centres[c], cutoff[c]), cases[c]
    assert (first[0], count[0]) == (j, 1)
    assert (first[3], count[3]) == (j, 2)
    assert first[5] == 0 and first[6] + count[6] == n
    # a one-step cutoff between two points holds none: refused, and the channel is named
    with pytest.raises(ValueError, match="channel 0 "):
        model.Instrument([0.5 * (x[j] + x[j + 1])], shape="boxcar", width=0.5 * step).support(lo, hi, n)


@pytest.mark.parametrize("nu", [100.0, 667.0, 2500.0])
@pytest.mark.parametrize("T", [180.0, 288.0, 320.0])
def test_brightness_temperature_inverts_planck(nu, T):
    assert model.brightnessTemperature(nu, model.planckWavenumber(nu, T)) == pytest.approx(T, rel=1e-12)


def test_brightness_temperature_arrays_and_non_positive_radiance():
    from oracle import pyrad_oracle as orc
    nu = np.array([100.0, 667.0, 2500.0])
    assert np.array_equal(model.planckWavenumber(nu, 288.0), orc.planckWavenumber(nu, 288.0))
    Tb = model.brightnessTemperature(nu, model.planckWavenumber(nu, np.array([180.0, 288.0, 320.0])))
    assert np.allclose(Tb, [180.0, 288.0, 320.0], rtol=1e-12, atol=0)
    got = model.brightnessTemperature(nu, [0.0, -1e-3, np.nan])
    assert got.shape == (3,) and np.all(np.isnan(got))
