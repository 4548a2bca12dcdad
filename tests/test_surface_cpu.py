"""CPU: the reflecting surface (Atmosphere.fluxes and radiance with an emissivity; lbl_column_flux_surface_dev,
lbl_ray_radiance_surface_dev, kernels K5g) without a device - the C ABI surface, the kernels' resource report, the paths
with a bounce and the host-side validation, which runs before anything touches a context."""
import os
import re

import numpy as np
import pytest

from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
DEPTHS = (1e4, 2e4, 5e4, 1e5)
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
SYMBOLS = ("lbl_column_flux_surface_dev", "lbl_ray_radiance_surface_dev")


def test_entry_points_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"int\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    assert len(_native.SIGNATURES["lbl_column_flux_surface_dev"][1]) == len(_native.SIGNATURES["lbl_column_flux_dev"][1]) + 4
    assert len(_native.SIGNATURES["lbl_ray_radiance_surface_dev"][1]) == len(_native.SIGNATURES["lbl_ray_radiance_dev"][1]) + 4
    assert lib.lbl_abi_version() == 5


def _template_args(name, kernel):
    m = re.search(kernel + r"I((?:Li\d+E)+)E", name)
    assert m, name
    return tuple(int(v) for v in re.findall(r"Li(\d+)E", m.group(1)))


def test_surface_kernels_in_the_resource_report():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    by_args = lambda sub: {_template_args(n, sub): f for n, f in k.items() if sub in n}
    flux, black = by_args("surface_flux_kernel"), by_args("column_flux_kernel")
    ray, plain = by_args("ray_surface_kernel"), by_args("ray_radiance_kernel")
    # 4 points per thread and 1 (head and tail) for 1..8 angles; bundles of 4 rays, single rays, head and tail
    assert sorted(flux) == [(np_, na) for np_ in (1, 4) for na in range(1, 9)], sorted(flux)
    assert sorted(ray) == [(1, 1), (4, 1), (4, 4)], sorted(ray)
    for new, old in ((flux, black), (ray, plain)):
        for args, f in new.items():
            assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (args, f)
            # never fewer waves per SIMD than the black-surface kernel of the same shape
            print(args, f["VGPRs"], f["Occupancy [waves/SIMD]"], old[args]["VGPRs"], old[args]["Occupancy [waves/SIMD]"])
            assert f["Occupancy [waves/SIMD]"] >= old[args]["Occupancy [waves/SIMD]"], (args, f, old[args])
    for args, f in ray.items():
        assert f.get("LDS Size [bytes/block]") == 0, (args, f)


def _atmosphere(layers=LAYERS):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("surface")
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


def test_path_with_a_bounce(no_context):
    p = model.Path([1, 0, 0], [1.0, 2.0, 3.0], source="space", name="x", bounce=2)
    assert (p.layers, p.lengths, p.source, p.name, p.bounce, len(p)) == ((1, 0, 0), (1.0, 2.0, 3.0), "space", "x", 2, 3)
    assert p._segments() == ((1, 0, -1, 0), (1.0, 2.0, 0.0, 3.0))
    assert model.Path([1], [1.0], bounce=0)._segments() == ((-1, 1), (0.0, 1.0))
    assert model.Path([1], [1.0], bounce=1)._segments() == ((1, -1), (1.0, 0.0))
    assert model.Path([], [], source="space", bounce=0)._segments() == ((-1,), (0.0,))
    assert "bounce=2" in repr(p)
    # without a bounce: today's object
    q = model.Path([1, 0], [1.0, 2.0])
    assert q.bounce is None and q._segments() == ((1, 0), (1.0, 2.0)) and "bounce" not in repr(q)
    for attr in ("bounce", "layers"):
        with pytest.raises(AttributeError):
            setattr(p, attr, 1)
    for bad in (-1, 4, 1.0, "1", True):
        with pytest.raises(ValueError, match="bounce"):
            model.Path([1, 0, 0], [1.0, 2.0, 3.0], bounce=bad)
    with pytest.raises(ValueError):                       # the marker exists only in the lists handed to the C call
        model.Path([-1], [1.0])
    with pytest.raises(ValueError):
        model.Path([0, -1], [1.0, 0.0], bounce=1)


@pytest.mark.parametrize("mu", [1.0, 0.4])
@pytest.mark.parametrize("level", [None, 2, 0])
def test_reflected_path(no_context, mu, level):
    atm = _atmosphere()
    L = len(DEPTHS)
    p = atm.reflectedPath(mu=mu, observerLevel=level)
    lev = L if level is None else level
    lay = tuple(range(L - 1, -1, -1)) + tuple(range(lev))
    assert p.layers == lay
    assert p.lengths == tuple(DEPTHS[l] / mu for l in lay)
    assert p.bounce == L and p.source == "space" and len(p) == L + lev
    with pytest.raises(AttributeError):
        p.bounce = 0


def test_emissivity_table_is_np_interp(no_context):
    atm = _atmosphere()
    x = np.asarray(atm[0].xAxis)
    nu = np.array([598.0, 601.5, 603.0, 604.25, 607.0, 608.5])
    val = np.array([0.99, 0.97, 0.7, 0.82, 0.91, 0.95])
    e = model._surface_emissivity((nu, val), x)
    assert e.dtype == np.float64 and e.flags.c_contiguous and np.array_equal(e, np.interp(x, nu, val))
    # the end values held beyond the table
    e = model._surface_emissivity(([603.0, 604.0], [0.5, 0.75]), x)
    assert np.array_equal(e, np.interp(x, [603.0, 604.0], [0.5, 0.75]))
    assert np.all(e[x <= 603.0] == 0.5) and np.all(e[x >= 604.0] == 0.75)
    arr = np.linspace(0.0, 1.0, x.size)
    assert np.array_equal(model._surface_emissivity(arr, x), arr)
    assert np.array_equal(model._surface_emissivity(list(arr), x), arr)
    for v in (0, 1, 0.5, np.float64(0.25)):
        assert model._surface_emissivity(v, x) == float(v) and isinstance(model._surface_emissivity(v, x), float)


def test_validation_before_any_device_work(no_context):
    atm = _atmosphere()
    n = len(atm[0].xAxis)
    nadir, mirror = atm.nadirPath(), atm.reflectedPath()
    bad_e = (-0.01, 1.5, float("nan"), "water", True, np.full(n, 1.01), np.full(n, -1e-9), np.full(n - 1, 0.9),
             np.full((2, n), 0.9), np.where(np.arange(n) == 7, np.nan, 0.9), ([600.0, 605.0], [0.9, 1.2]),
             ([600.0, 605.0], [0.9, float("nan")]), ([605.0, 600.0], [0.9, 0.8]), ([600.0, 605.0, 610.0], [0.9, 0.8]))
    for e in bad_e:
        with pytest.raises(ValueError, match="emissivity"):
            atm.fluxes(surfaceTemperature=288, emissivity=e)
        with pytest.raises(ValueError, match="emissivity"):
            atm.radiance(nadir, surfaceTemperature=288, emissivity=e)
    for r in ("mirror", "Lambertian", 0, None):
        with pytest.raises(ValueError, match="reflection"):
            atm.fluxes(surfaceTemperature=288, emissivity=0.9, reflection=r)
        with pytest.raises(ValueError, match="reflection"):
            atm.radiance(nadir, surfaceTemperature=288, emissivity=0.9, reflection=r)
    with pytest.raises(ValueError, match="reflection"):
        atm.fluxes(surfaceTemperature=288, reflection="mirror")          # also without an emissivity
    # a path with a bounce: needs an emissivity, a surface source, and has no weighting functions
    with pytest.raises(ValueError, match="emissivity"):
        atm.radiance(mirror, surfaceTemperature=288)
    with pytest.raises(ValueError, match="emissivity"):
        atm.radiance([nadir, mirror], surfaceTemperature=288)
    with pytest.raises(ValueError, match="surface"):
        atm.radiance(mirror, emissivity=0.9)
    with pytest.raises(ValueError, match="surfaceTemperature"):
        atm.radiance(mirror, emissivity=0.9, surfaceTemperature=0)
    with pytest.raises(ValueError, match="bounce"):
        atm.pathJacobians(mirror, surfaceTemperature=288)
    with pytest.raises(ValueError, match="bounce"):
        atm.pathJacobians([nadir, mirror], surfaceTemperature=288)
    for i in (-1, 9):
        with pytest.raises(ValueError, match="bounce"):
            model.Path(mirror.layers, mirror.lengths, source="space", bounce=i)
    for a in (0, 9, "gauss", [(1.5, 1.0)], [], [(0.5, 1.0), (0.25, -1.0)], [(0.5, 0.0)]):
        with pytest.raises(ValueError, match="angles"):
            atm.radiance(nadir, surfaceTemperature=288, emissivity=0.9, angles=a)
    for a in ([(0.5, 1.0), (0.25, -1.0)], [(0.5, 0.0)]):                  # weights that do not add up to more than 0
        with pytest.raises(ValueError, match="angles"):
            atm.fluxes(surfaceTemperature=288, emissivity=0.9, angles=a)
    # ... which a black surface still takes (today's behaviour): it gets as far as the context
    with pytest.raises(AssertionError, match="context"):
        atm.fluxes(surfaceTemperature=288, angles=[(0.5, 0.0)])
    # and what radiance() refused before, it refuses with an emissivity too
    with pytest.raises(ValueError, match="surface"):
        atm.radiance(nadir, emissivity=0.9)
    with pytest.raises(ValueError, match="layer 4"):
        atm.radiance(model.Path([4], [1.0], source="space", bounce=1), surfaceTemperature=288, emissivity=0.9)
