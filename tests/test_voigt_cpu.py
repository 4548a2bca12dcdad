"""CPU: the Voigt function of pyrad_amd/csrc/lbl_voigt_func.h, compiled with g++ from the very text the device compiles,
against scipy.special.wofz and against the committed fixture; the fixture against its generator; the compiler's report
for the new kernels; the setting."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_golden
from pyrad_amd import _native

sys.path.insert(0, GOLDEN)
import make_voigt_golden as mvg      # noqa: E402

HEADER = os.path.join(_native.CSRC, "lbl_voigt_func.h")


@pytest.fixture(scope="module")
def voigt_k(tmp_path_factory):
    """voigt_k(x, y) over arrays, from a small shared library built from the header with g++"""
    d = tmp_path_factory.mktemp("voigt")
    src = d / "voigt_k.cpp"
    src.write_text('#include "%s"\n'
                   'extern "C" void voigt_k_array(const double* x, const double* y, long n, double* out) {\n'
                   '    for (long i = 0; i < n; ++i) out[i] = lbl::voigt_k(x[i], y[i]);\n'
                   '}\n' % HEADER)
    lib = d / "libvoigt_k.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(lib), str(src)])
    fn = ctypes.CDLL(str(lib)).voigt_k_array
    P = ctypes.POINTER(ctypes.c_double)
    fn.argtypes = [P, P, ctypes.c_long, P]
    fn.restype = None

    def call(x, y):
        x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        out = np.empty(x.shape)
        fn(x.ctypes.data_as(P), y.ctypes.data_as(P), x.size, out.ctypes.data_as(P))
        return out
    return call


def test_against_wofz_on_the_table_random_pairs_and_every_switch_over(voigt_k):
    """Measured with g++ -O2: table 2.4e-10 (y = 1e-5, x = 7.4: the near branch where only y / (sqrt(pi) x^2) is left),
    random pairs 2e-10, bands 2.9e-10 (s = 100 at y = 1e-5) and 3.2e-11 (s = 400)."""
    wofz = pytest.importorskip("scipy.special").wofz
    x, y = mvg.table_axes()
    assert x.size == 401 and y.size == 38
    worst = mvg.check_function(voigt_k(x[:, None], y[None, :]), wofz(x[:, None] + 1j * y[None, :]).real, "table")
    rx, ry = mvg.random_pairs(10000)
    worst = max(worst, mvg.check_function(voigt_k(rx, ry), wofz(rx + 1j * ry).real, "random pairs"))
    b = mvg.boundaries()
    assert set(b) == {"S_FAR", "S_MID"} and len(re.findall(r"#define\s+LBL_VOIGT_S_", open(HEADER).read())) == len(b)
    bx, by = mvg.band_points()
    # every band does cross its switch-over
    s = bx * bx + by * by
    for v in b.values():
        assert (s < v).any() and (s >= v).any() and np.sum(np.abs(s / v - 1) < 0.03) >= 201
    worst = max(worst, mvg.check_function(voigt_k(bx, by), wofz(bx + 1j * by).real, "bands"))
    print("worst relative error against wofz: %.3e" % worst)


def test_against_the_fixture(voigt_k):
    z = load_golden("V0_voigt")
    mvg.check_function(voigt_k(z["fx"][:, None], z["fy"][None, :]), z["fK"], "table")
    mvg.check_function(voigt_k(z["rx"], z["ry"]), z["rK"], "random pairs")
    mvg.check_function(voigt_k(z["bx"], z["by"]), z["bK"], "bands")


def test_edges_of_the_domain(voigt_k):
    nan, inf = float("nan"), float("inf")
    assert np.isnan(voigt_k([nan, 1.0, nan, nan, 50.0, 3.0], [1.0, nan, 0.0, nan, nan, nan])).all()
    # far beyond the table: never negative, under the floor where the true value is
    x = np.array([1e8, 1e150, 1e160, 1e300, inf, 30.0, 1e5, inf])
    y = np.array([1e-5, 1.0, 1e4, 1e4, 1.0, 0.0, 0.0, 0.0])
    k = voigt_k(x, y)
    assert np.all(k >= 0) and np.all(k[1:] <= 1e-290)
    assert abs(k[0] / (1e-5 / np.sqrt(np.pi) / 1e16) - 1) < 1e-12
    assert voigt_k([0.0], [0.0])[0] == 1.0
    # y == 0 is exp(-x^2) itself
    xs = np.linspace(0, 27, 500)
    assert np.allclose(voigt_k(xs, 0.0), np.exp(-xs * xs), rtol=1e-14, atol=0)


def test_below_the_domain_in_y(voigt_k):
    """0 < y < 1e-5 is outside the contract; what the header documents, within a factor of two: the relative error grows
    like 1 / y where only the Lorentz wing is left (measured 2.5e-9, 2.8e-8, 2.5e-7 at y = 1e-6, 1e-7, 1e-8)."""
    wofz = pytest.importorskip("scipy.special").wofz
    x = np.logspace(-3, 5, 2000)
    for y, bound in ((1e-6, 5e-9), (1e-7, 6e-8), (1e-8, 5e-7)):
        ref = wofz(x + 1j * y).real
        assert np.max(np.abs(voigt_k(x, y) - ref) / ref) <= bound


def test_generator_reproduces_the_fixture(tmp_path):
    pytest.importorskip("scipy")
    made = np.load(mvg.main(str(tmp_path)))
    kept = load_golden("V0_voigt")
    assert sorted(made.files) == sorted(kept.files)
    for k in kept.files:
        assert made[k].shape == kept[k].shape and made[k].dtype == kept[k].dtype, k
        if kept[k].dtype.kind == "f":
            # (cross sections and table values go through libm's and SciPy's functions: their last bits may differ between builds)
            assert np.allclose(made[k], kept[k], rtol=1e-12, atol=0, equal_nan=True), k
            assert np.array_equal(made[k] == 0, kept[k] == 0), k
        else:
            assert np.array_equal(made[k], kept[k]), k
    assert os.path.getsize(os.path.join(GOLDEN, mvg.NAME)) < 600 * 1024
    names = json.loads(str(kept["cases"]))
    assert len(names) == 10
    for n in names:
        c = mvg.load_case(kept, n)
        g = mvg.case_physics(c)[3]
        assert len(c["lines"]["nu"]) <= 200 and g["n_work"] <= 6000 and c["xsec"].size == g["n_base"]


def test_new_kernels_use_no_scratch():
    """The compiler's report for the production build: voigt_prep_kernel 34 VGPRs, 8 waves per SIMD, 48 B of LDS;
    voigt_accumulate_kernel 71 VGPRs, 7 waves per SIMD, 8 KB of LDS per workgroup (2 KB per wave); voigt_function_kernel 18
    VGPRs, 8 waves per SIMD.  No scratch, no spilled vector register."""
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB): the report beside the production objects is not its own")
    import test_kernel_resources_cpu as res
    kernels = res._kernels(res._remarks("lbl_kernels"))
    for sub in ("voigt_prep_kernel", "voigt_accumulate_kernel", "voigt_function_kernel"):
        hit = [f for n, f in kernels.items() if sub in n]
        assert len(hit) == 1, (sub, len(hit))
        f = hit[0]
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0, (sub, f)
        assert f["VGPRs"] <= 128 and f["Occupancy [waves/SIMD]"] >= 4, (sub, f)
    # the names the accumulate kernels' occupancy test looks up by substring still have one owner each
    assert not any("voigt" in n and ("xsec_accumulate_lds_kernel" in n or "xsec_accumulate_skew_kernel" in n) for n in kernels)


def test_set_line_shape_refuses_unknown_names():
    from pyrad_amd import settings
    assert settings.LINE_SHAPE == "reference"
    for bad in ("Voigt", "lorentz", "", None, 1):
        with pytest.raises(ValueError):
            settings.set_line_shape(bad)
    assert settings.LINE_SHAPE == "reference"
    settings.set_line_shape("voigt")
    try:
        assert settings.LINE_SHAPE == "voigt"
    finally:
        settings.set_line_shape("reference")
    assert settings.LINE_SHAPE == "reference"


def test_binding_lists_the_new_symbols():
    with open(os.path.join(REPO, "include", "pyrad_hip.h")) as f:
        header = f.read()
    for name in ("lbl_xsec_voigt_dev", "lbl_voigt_function_dev"):
        assert name in _native.SIGNATURES and re.search(r"\bint %s\(" % name, header)
    assert "#define LBL_ABI_VERSION 5" in header
