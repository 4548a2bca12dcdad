"""CPU: the ray-path feature (Atmosphere.radiance, lbl_ray_radiance_dev) without a device - the C ABI surface, the kernel's
resource report, the path geometry and the host-side validation, which runs before anything touches a context."""
import math
import os
import re

import numpy as np
import pytest

from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
DEPTHS = (1e4, 2e4, 5e4, 1e5)                      # the 4-layer column of tests/test_gpu_flux.py
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
R_PLANET = 6.371e8


def test_entry_point_declared_exported_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    assert re.search(r"int\s+lbl_ray_radiance_dev\s*\(", text)
    lib = _native.load()
    assert hasattr(lib, "lbl_ray_radiance_dev")
    assert lib.lbl_abi_version() == 5
    assert _native.limit("ray_paths") == 512 == _native.limit("ils_rows")
    assert _native.limit("ray_segments") == 65536


def test_ray_kernel_uses_no_scratch_and_does_not_spill():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    ray = {n: f for n, f in k.items() if "ray_radiance_kernel" in n}
    # 4 points per thread for bundles of 4 rays and for single rays, 1 point per thread (head and tail) for single rays
    assert len(ray) == 3, sorted(ray)
    for n, f in ray.items():
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (n, f)
        assert f.get("LDS Size [bytes/block]") == 0, (n, f)


def _atmosphere(layers=LAYERS, ranges=None):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("paths")
    for i, (depth, T, P) in enumerate(layers):
        lo, hi = ranges[i] if ranges else (600, 610)
        atm.addLayer(depth, T, P, lo, hi)
    return atm


@pytest.fixture()
def no_context(monkeypatch):
    """every check below must fail before the engine (and with it a device context) is asked for"""
    def refuse():
        raise AssertionError("the context was touched before the arguments were validated")
    monkeypatch.setattr(model, "_ctx", refuse)
    settings.set_resolution_multiplier(1)
    yield


def test_nadir_and_zenith_paths(no_context):
    atm = _atmosphere()
    p = atm.nadirPath()
    assert (p.layers, p.lengths, p.source, len(p)) == ((0, 1, 2, 3), DEPTHS, "surface", 4)
    p = atm.nadirPath(mu=0.4)
    assert p.layers == (0, 1, 2, 3) and p.lengths == tuple(d / 0.4 for d in DEPTHS)
    p = atm.nadirPath(observerLevel=2)
    assert (p.layers, p.lengths, p.source) == ((0, 1), (1e4, 2e4), "surface")
    p = atm.nadirPath(mu=0.5, observerLevel=0)
    assert (p.layers, p.lengths, len(p)) == ((), (), 0)
    p = atm.zenithPath()
    assert (p.layers, p.lengths, p.source) == ((3, 2, 1, 0), DEPTHS[::-1], "space")
    p = atm.zenithPath(mu=0.3, observerLevel=2)
    assert (p.layers, p.lengths, p.source) == ((3, 2), (1e5 / 0.3, 5e4 / 0.3), "space")
    p = atm.zenithPath(observerLevel=4)
    assert len(p) == 0 and p.source == "space"
    with pytest.raises(AttributeError):
        p.source = "surface"


@pytest.mark.parametrize("zt, m", [(0.0, 0), (5e3, 0), (1e4, 1), (2.5e4, 1), (1.7999e5, 3)])
def test_limb_path(no_context, zt, m):
    atm = _atmosphere()
    p = atm.limbPath(zt)
    nl = len(DEPTHS)
    above = list(range(nl - 1, m, -1))
    assert list(p.layers) == above + [m] + above[::-1]          # the tangent layer once
    assert p.source == "space" and len(p) == 2 * (nl - 1 - m) + 1
    assert p.lengths == p.lengths[::-1]                         # symmetric
    assert all(x > 0 for x in p.lengths)
    zL = sum(DEPTHS)
    chord = 2 * math.sqrt((zL - zt) * (2 * R_PLANET + zL + zt))
    assert math.fsum(p.lengths) == pytest.approx(chord, rel=1e-13)
    # a layer's half chord is at least the layer's vertical extent above the tangent height
    z = np.concatenate([[0.0], np.cumsum(DEPTHS)])
    for l, x in zip(p.layers[:len(above)], p.lengths):
        assert x >= z[l + 1] - z[l]
    # another planet: longer chords around a larger one
    assert sum(atm.limbPath(zt, planetRadius=4 * R_PLANET).lengths) > sum(p.lengths)


def test_path_validation(no_context):
    assert len(model.Path([], [])) == 0
    p = model.Path([2, 0, 2], [1.0, 0.0, 3], source="space", name="x")
    assert (p.layers, p.lengths, p.source, p.name, len(p)) == ((2, 0, 2), (1.0, 0.0, 3.0), "space", "x", 3)
    for lay, lens in (([0], [-1.0]), ([0], [float("nan")]), ([0], [float("inf")]), ([0, 1], [1.0]), ([-1], [1.0]),
                      ([0.5], [1.0]), (["a"], [1.0]), ([0], ["b"])):
        with pytest.raises(ValueError):
            model.Path(lay, lens)
    with pytest.raises(ValueError, match="source"):
        model.Path([0], [1.0], source="sun")


def test_validation_before_any_device_work(no_context):
    atm = _atmosphere()
    for bad in (0, 0.0, -0.5, 1.0001, float("nan"), "down"):
        with pytest.raises(ValueError, match="mu"):
            atm.nadirPath(mu=bad)
        with pytest.raises(ValueError, match="mu"):
            atm.zenithPath(mu=bad)
    for bad in (-1, 5, 1.5, "top"):
        with pytest.raises(ValueError, match="observerLevel"):
            atm.nadirPath(observerLevel=bad)
        with pytest.raises(ValueError, match="observerLevel"):
            atm.zenithPath(observerLevel=bad)
    for bad in (-1.0, 1.8e5, 2e5, float("nan")):
        with pytest.raises(ValueError, match="tangentHeight"):
            atm.limbPath(bad)
    with pytest.raises(ValueError, match="no layers"):
        model.Atmosphere("empty").limbPath(0.0)
    with pytest.raises(ValueError, match="range"):
        _atmosphere(ranges=((600, 610),) * 3 + ((600, 620),)).radiance(atm.zenithPath())
    with pytest.raises(ValueError, match="paths"):
        atm.radiance([])
    with pytest.raises(ValueError, match="paths"):
        atm.radiance([atm.zenithPath(), "limb"])
    with pytest.raises(ValueError, match="paths"):
        atm.radiance([atm.zenithPath()] * 513)
    with pytest.raises(ValueError, match="layer 4"):
        atm.radiance(model.Path([4], [1.0], source="space"))
    with pytest.raises(ValueError, match="segments"):
        atm.radiance([model.Path([0] * 129, [1.0] * 129, source="space")] * 509)
    with pytest.raises(ValueError, match="surface"):
        atm.radiance([atm.zenithPath(), atm.nadirPath()])
    with pytest.raises(ValueError, match="surfaceTemperature"):
        atm.radiance(atm.nadirPath(), surfaceTemperature=0)
    with pytest.raises(ValueError, match="surfaceSpectrum"):
        atm.radiance(atm.nadirPath(), surfaceSpectrum=np.zeros(17))
    ins = model.Instrument(np.arange(602.0, 608.0, 0.5), width=0.5)
    with pytest.raises(ValueError, match="instrument"):
        atm.radiance(atm.zenithPath(), instrument="iasi")
    with pytest.raises(ValueError, match="rows"):
        atm.radiance([atm.zenithPath()] * 257, instrument=ins, transmittance=True)
