"""CPU: the k-distribution feature (gIntervals, kDistribution, Atmosphere.kDistribution, lbl_rank_order_dev,
lbl_ranked_means_dev) without a device - the C ABI surface, the kernels' resource report, the rank edges and the host-side
validation, which runs before anything touches a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")


def test_entry_points_declared_exported_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    for name in ("lbl_rank_order_dev", "lbl_rank_order_workspace", "lbl_ranked_means_dev", "lbl_ranked_means_workspace"):
        assert re.search(r"int\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    assert lib.lbl_abi_version() == 5


def test_limits_and_tile():
    assert _native.limit("kdist_rows") == 512
    assert _native.limit("kdist_intervals") == 256
    with open(os.path.join(_native.CSRC, "lbl_device.h")) as fh:
        assert re.search(r"kKdistTile\s*=\s*%d\s*;" % _native.KDIST_TILE, fh.read())
    import pyrad_amd
    assert pyrad_amd.gIntervals is model.gIntervals and pyrad_amd.kDistribution is model.kDistribution
    assert pyrad_amd.KDistribution is model.KDistribution


def test_workspace_function_without_a_device():
    """no context is needed to size the work space: none for bands of one tile, 3 doubles per ranked point beyond"""
    lib = _native.load()
    T = _native.KDIST_TILE
    v = C.c_int64(-1)

    def ws(n_rows, n, counts):
        a = (C.c_int64 * len(counts))(*counts)
        return lib.lbl_rank_order_workspace(n_rows, n, len(counts), a, C.byref(v)), v.value

    assert ws(3, 10 * T, [T, 1, 63]) == (0, 0)
    assert ws(3, 10 * T, [T + 1, 5]) == (0, 3 * 3 * (T + 6))
    assert ws(0, 10 * T, [5])[0] == -1
    assert ws(513, 10 * T, [5])[0] == -1
    assert ws(1, 10, [11])[0] == -1
    assert ws(1, 10, [0])[0] == -1


def test_kdist_kernels_use_no_scratch_and_do_not_spill():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    kd = {n: f for n, f in k.items() if "kdist_" in n}
    assert len(kd) == 4, sorted(kd)                    # tile sort, merge pass, partial sums, means
    for n, f in kd.items():
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0 and f.get("SGPRs Spill") == 0, (n, f)
        assert f["VGPRs"] <= 128, (n, f)               # four waves per SIMD at least


# ---- gIntervals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3, 16])
def test_integer_g_is_cumulative_gauss_legendre(G):
    count = 10000
    g = np.r_[0, np.cumsum(np.polynomial.legendre.leggauss(G)[1] / 2)]
    g[-1] = 1.0
    want = [int(np.rint(v * count)) for v in g]
    e = model.gIntervals(G, count)
    assert e.dtype == np.int64 and e.tolist() == want
    assert e[0] == 0 and e[-1] == count and np.all(np.diff(e) > 0)


def test_explicit_g_edges():
    e = model.gIntervals([0, 0.25, 0.5, 0.9, 1], 1001)
    assert e.tolist() == [0, 250, 500, 901, 1001]
    assert model.gIntervals(np.linspace(0, 1, 257), 256).tolist() == list(range(257))      # one point each
    assert model.gIntervals(256, 100000)[-1] == 100000


def test_g_refusals():
    for bad in (0, 257, -1, True, None, "many", 2.5):
        with pytest.raises(ValueError, match="g"):
            model.gIntervals(bad, 10000)
    for bad in ([0, 0.6, 0.4, 1], [0, 0.5, 0.5, 1], [0.1, 0.5, 1], [0, 0.5, 0.9], [0, 0.5, 1.1], [0], [0, np.nan, 1],
                [[0, 1], [0, 1]], np.linspace(0, 1, 258)):
        with pytest.raises(ValueError, match="g"):
            model.gIntervals(bad, 10000)
    with pytest.raises(ValueError, match="interval 0 .*holds no"):
        model.gIntervals(16, 8)
    with pytest.raises(ValueError, match="holds no"):
        model.gIntervals([0, 0.5, 0.51, 1], 10)
    for bad in (0, -5, None):
        with pytest.raises(ValueError, match="count"):
            model.gIntervals(4, bad)


# ---- validation before any device work ----------------------------------------------------------------------------------
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


def test_host_rows_validation(no_context):
    rows = np.ones((3, 10000))
    for bad in (3, -1, 1.0, "0", True, [0]):
        with pytest.raises(ValueError, match="reference"):
            model.kDistribution(rows, 600, 700, reference=bad)
    with pytest.raises(ValueError, match="reference"):
        model.kDistribution(rows[0], 600, 700, reference=1)
    for bad in ([], [(650, 640)], [(500, 650)], [(600, 650)] * 65, [650], [(710, 720)]):
        with pytest.raises(ValueError, match="bands"):
            model.kDistribution(rows, 600, 700, bands=bad)
    for bad in (0, 257, [0, 0.5], [0, 0.7, 0.3, 1]):
        with pytest.raises(ValueError, match="g"):
            model.kDistribution(rows, 600, 700, g=bad)
    with pytest.raises(ValueError, match="holds no"):
        model.kDistribution(rows, 600, 700, bands=[(600, 650), (650, 650.05)], g=16)      # 16 intervals of a 5-point band
    for bad in (np.ones((2, 3, 100)), np.ones(1), np.ones((3, 1)), np.ones((0, 100)), 1.0):
        with pytest.raises(ValueError, match="spectra"):
            model.kDistribution(bad, 600, 700)
    with pytest.raises(ValueError, match="rows"):
        model.kDistribution(np.ones((513, 64)), 600, 700, g=4)


def test_atmosphere_validation(no_context):
    with pytest.raises(ValueError, match="no layers"):
        model.Atmosphere("empty").kDistribution()
    atm = _atmosphere()
    for bad in (2, -1, 0.0, "top", True):
        with pytest.raises(ValueError, match="reference"):
            atm.kDistribution(reference=bad)
    for bad in ([], [(650, 640)], [(500, 650)], [(600, 650)] * 65, [(710, 720)]):
        with pytest.raises(ValueError, match="bands"):
            atm.kDistribution(bands=bad)
    for bad in (0, 257, [0, 0.5], [0, 0.7, 0.3, 1], "sixteen"):
        with pytest.raises(ValueError, match="g"):
            atm.kDistribution(g=bad, planck=True)
    with pytest.raises(ValueError, match="holds no"):
        atm.kDistribution(bands=[(650, 650.05)], g=16)
    mixed = _atmosphere()
    mixed.addLayer(1e4, 250, 100.0, 600, 650)
    with pytest.raises(ValueError, match="share one wavenumber range"):
        mixed.kDistribution()
