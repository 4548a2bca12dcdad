"""CPU: ray-path Jacobians (Atmosphere.pathJacobians, lbl_ray_jacobian_dev, lbl_ray_jacobian_rows; kernel K5f) without a
device - the C ABI surface, the row layout, the kernel's resource report and the host-side validation, which runs before
anything touches a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyrad_amd import _native, model, settings

ROOT = os.path.join(os.path.dirname(_native.CSRC), "..")
HEADER = os.path.join(ROOT, "include", "pyrad_hip.h")
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
BAD_ARG = -1


def test_entry_points_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    for name in ("lbl_ray_jacobian_rows", "lbl_ray_jacobian_dev"):
        assert re.search(r"int\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    assert hasattr(_native.Context, "ray_jacobian_dev") and callable(_native.ray_jacobian_rows)
    assert lib.lbl_abi_version() == 5
    assert "#define LBL_ABI_VERSION 5" in text


# ---- the row layout --------------------------------------------------------------------------------------------------------
def layout(rays, terms=(), n_layers=4):
    """the layout as include/pyrad_hip.h states it: per ray 1 + 2 c + m rows, c distinct layers, m terms in one of them"""
    first = [0]
    for lay in rays:
        first.append(first[-1] + 1 + 2 * len(set(lay)) + sum(1 for l in terms if l in set(lay)))
    return first


def rows_of(rays, terms=(), n_layers=4):
    ray_first = np.cumsum([0] + [len(r) for r in rays])
    return _native.ray_jacobian_rows(n_layers, ray_first, [l for r in rays for l in r], terms)


def test_rows_of_a_nadir_a_limb_and_an_empty_ray():
    nadir, limb, empty = [0, 1, 2, 3], [3, 2, 1, 2, 3], []
    first, rows = rows_of([nadir])
    assert list(first) == [0, 9] and rows == 9
    first, rows = rows_of([limb])                      # the tangent layer once, the others twice: three distinct layers
    assert list(first) == [0, 7] and rows == 7
    first, rows = rows_of([empty])
    assert list(first) == [0, 1] and rows == 1
    rays = [nadir, limb, empty, [1, 1, 0, 1], nadir]
    first, rows = rows_of(rays)
    assert list(first) == layout(rays) == [0, 9, 16, 17, 22, 31] and rows == 31


def test_rows_with_terms_in_layers_crossed_and_not():
    rays = [[0, 1, 2, 3], [3, 2, 1, 2, 3], [], [1, 1, 0, 1]]
    terms = [0, 0, 1, 3, 3, 2, 0]                        # three terms in layer 0, one in 1, one in 2, two in 3
    first, rows = rows_of(rays, terms)
    assert list(first) == layout(rays, terms) == [0, 16, 27, 28, 37] and rows == 37
    # a term in a layer no ray crosses adds no row
    assert rows_of([[3, 2, 3]], [0, 1])[1] == 5 and rows_of([[3, 2, 3]], [0, 2])[1] == 6


def test_rows_without_row_first_and_refusals():
    lib = _native.load()
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    rows = C.c_int64(-1)
    first = (C.c_int64 * 3)()
    good = dict(n_layers=4, n_rays=2, ray_first=i32([0, 4, 9]), seg_layer=i32([0, 1, 2, 3, 3, 2, 1, 2, 3]), n_terms=2,
                term_layer=i32([1, 0]), row_first=first, rows=C.byref(rows))

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.lbl_ray_jacobian_rows(*[a[k] for k in good])

    assert call() == 0 and rows.value == 11 + 8 and list(first) == [0, 11, 19]
    rows.value = -1
    assert call(row_first=None) == 0 and rows.value == 19
    assert call(n_terms=0, term_layer=None) == 0 and rows.value == 16
    for kw in (dict(seg_layer=i32([0, 1, 2, 4, 3, 2, 1, 2, 3])), dict(seg_layer=i32([0, -1, 2, 3, 3, 2, 1, 2, 3])),
               dict(ray_first=i32([1, 4, 9])), dict(ray_first=i32([0, 5, 4])), dict(n_rays=0), dict(n_layers=0),
               dict(n_rays=_native.limit("ray_paths") + 1, ray_first=i32([0] * (_native.limit("ray_paths") + 2))),
               dict(n_layers=_native.limit("layers_per_column") + 1),
               dict(term_layer=i32([1, 4])), dict(term_layer=i32([-1, 0])), dict(term_layer=None),
               dict(n_terms=-1), dict(n_terms=_native.limit("jacobian_terms") + 1),
               dict(ray_first=None), dict(seg_layer=None), dict(rows=None)):
        assert call(**kw) == BAD_ARG, sorted(kw)
    with pytest.raises(_native.LblError):
        _native.ray_jacobian_rows(4, [0, 1], [4])


# ---- the kernel's resources --------------------------------------------------------------------------------------------------
def test_ray_jacobian_kernel_uses_no_scratch_no_lds_and_does_not_spill():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    jac = {n: f for n, f in k.items() if "ray_jacobian_kernel" in n}
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        m = re.search(r"K5f[^\n]*\n(?:.*\n)*?.*?(\d+) instantiations of `ray_jacobian_kernel`", fh.read())
    assert m, "DESIGN.md states the number of ray_jacobian_kernel instantiations"
    # 4 points per thread for bundles of 4 rays (with and without the term loop) and for single rays, 1 point per thread
    # (the tail) for single rays
    assert len(jac) == int(m.group(1)) == 4, sorted(jac)
    for n, f in jac.items():
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (n, f)
        assert f.get("LDS Size [bytes/block]") == 0, (n, f)


# ---- validation before any device work -----------------------------------------------------------------------------------------
class _Counted(list):
    """stands in for a Molecule where molecules are only counted: the term limit is checked before any of them is used"""
    name, exotic = "x", True


def _atmosphere(layers=LAYERS, ranges=None, molecules=0):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("path jacobians")
    for i, (depth, T, P) in enumerate(layers):
        lo, hi = ranges[i] if ranges else (600, 610)
        L = atm.addLayer(depth, T, P, lo, hi)
        for m in range(molecules):
            L.append(_Counted())
    return atm


@pytest.fixture()
def no_context(monkeypatch):
    """every check below must fail before the engine (and with it a device context) is asked for"""
    def refuse():
        raise AssertionError("the context was touched before the arguments were validated")
    monkeypatch.setattr(model, "_ctx", refuse)
    settings.set_resolution_multiplier(1)
    yield
    settings.set_line_shape("reference")


def test_validation_before_any_device_work(no_context):
    atm = _atmosphere()
    nadir, zenith = atm.nadirPath(), atm.zenithPath()
    with pytest.raises(ValueError, match="temperature"):
        atm.pathJacobians(zenith, temperature="absorption")
    with pytest.raises(ValueError, match="range"):
        _atmosphere(ranges=((600, 610),) * 3 + ((600, 620),)).pathJacobians(zenith)
    with pytest.raises(ValueError, match="paths"):
        atm.pathJacobians([])
    with pytest.raises(ValueError, match="paths"):
        atm.pathJacobians([zenith, "limb"])
    with pytest.raises(ValueError, match="paths"):
        atm.pathJacobians([zenith] * 513)
    with pytest.raises(ValueError, match="layer 4"):
        atm.pathJacobians(model.Path([4], [1.0], source="space"))
    with pytest.raises(ValueError, match="segments"):
        atm.pathJacobians([model.Path([0] * 129, [1.0] * 129, source="space")] * 509)
    with pytest.raises(ValueError, match="surface"):
        atm.pathJacobians([zenith, nadir])
    with pytest.raises(ValueError, match="surfaceTemperature"):
        atm.pathJacobians(nadir, surfaceTemperature=0)
    with pytest.raises(ValueError, match="surfaceSpectrum"):
        atm.pathJacobians(nadir, surfaceSpectrum=np.zeros(17))
    with pytest.raises(ValueError, match="instrument"):
        atm.pathJacobians(zenith, instrument="iasi")
    with pytest.raises(ValueError, match="not inside the range"):
        atm.pathJacobians(zenith, instrument=model.Instrument([700.0], width=0.5))
    # temperature="full" needs the Voigt line shape ...
    settings.set_line_shape("reference")
    with pytest.raises(ValueError, match="discontinuous in T"):
        atm.pathJacobians(zenith, temperature="full")
    # ... and its terms count against the limit beside the molecules'
    assert _native.limit("jacobian_terms") == 512
    with pytest.raises(ValueError, match="molecule terms"):
        _atmosphere(molecules=129).pathJacobians(zenith, molecules=True)             # 516 terms
    settings.set_line_shape("voigt")
    with pytest.raises(ValueError, match="dk/dT terms"):
        _atmosphere(molecules=128).pathJacobians(zenith, molecules=True, temperature="full")      # 512 + 4 terms
