"""CPU: voigt_kgrad of pyrad_amd/csrc/lbl_voigt_func.h (K, x dK/dx, y dK/dy), compiled with g++ from the very text the
device compiles, against the committed mpmath fixture tests/golden/V1_voigt_dT.npz; the fixture against its generator; the
compiler's report for the K2v-T kernels; the new symbols; what the model refuses without a device."""
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
RTOL = 1e-6                          # the contract, in the form the kernel consumes it: errors over K
FLOOR = mvg.FLOOR


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    """(voigt_kgrad, voigt_k) over arrays, from a small shared library built from the header with g++"""
    d = tmp_path_factory.mktemp("voigt_dT")
    src = d / "voigt_kgrad.cpp"
    src.write_text('#include "%s"\n'
                   'extern "C" void kgrad_array(const double* x, const double* y, long n, double* K, double* GX, double* GY) {\n'
                   '    for (long i = 0; i < n; ++i) lbl::voigt_kgrad(x[i], y[i], K + i, GX + i, GY + i);\n'
                   '}\n'
                   'extern "C" void k_array(const double* x, const double* y, long n, double* out) {\n'
                   '    for (long i = 0; i < n; ++i) out[i] = lbl::voigt_k(x[i], y[i]);\n'
                   '}\n' % HEADER)
    so = d / "libvoigt_kgrad.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(so), str(src)])
    dll = ctypes.CDLL(str(so))
    P = ctypes.POINTER(ctypes.c_double)
    dll.kgrad_array.argtypes = [P, P, ctypes.c_long, P, P, P]
    dll.k_array.argtypes = [P, P, ctypes.c_long, P]
    dll.kgrad_array.restype = dll.k_array.restype = None

    def prep(x, y):
        x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        return np.ascontiguousarray(x), np.ascontiguousarray(y)

    def kgrad(x, y):
        x, y = prep(x, y)
        out = [np.empty(x.shape) for _ in range(3)]
        dll.kgrad_array(x.ctypes.data_as(P), y.ctypes.data_as(P), x.size, *[o.ctypes.data_as(P) for o in out])
        return out

    def k(x, y):
        x, y = prep(x, y)
        out = np.empty(x.shape)
        dll.k_array(x.ctypes.data_as(P), y.ctypes.data_as(P), x.size, out.ctypes.data_as(P))
        return out
    return kgrad, k


def point_sets(z):
    """name -> (x, y, (K, GX, GY) of the fixture)"""
    fx, fy = mvg.table_axes()
    X, Y = np.broadcast_arrays(fx[:, None], fy[None, :])
    rx, ry = mvg.random_pairs(2000)
    bx, by = mvg.band_points()
    return {"table": (X, Y, (z["fK"], z["fGX"], z["fGY"])), "random pairs": (rx, ry, (z["rK"], z["rGX"], z["rGY"])),
            "bands": (bx, by, (z["bK"], z["bGX"], z["bGY"]))}


def branch_of(x, y):
    s = x * x + y * y
    b = mvg.boundaries()
    return np.where(y == 0, "y == 0", np.where(s >= b["S_FAR"], "far", np.where(s >= b["S_MID"], "mid", "near")))


def contract_errors(got, ref, x, y, what):
    """Asserts the three bounds wherever the true K >= FLOOR; returns {branch: (worst dK/K, dGX/K, dGY/K)}"""
    K, GX, GY = (np.asarray(v, dtype=np.float64).ravel() for v in got)
    rK, rGX, rGY = (np.asarray(v, dtype=np.float64).ravel() for v in ref)
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    assert K.shape == rK.shape == x.shape
    assert not (np.isnan(K).any() or np.isnan(GX).any() or np.isnan(GY).any()), what
    assert np.all(K >= 0) and np.all(GX <= 0), what
    assert np.all(GX[x == 0] == 0) and np.all(GY[y == 0] == 0), what
    big = rK >= FLOOR
    assert np.all(K[~big] <= FLOOR), what
    br = branch_of(x, y)
    worst = {}
    for name in np.unique(br[big]):
        m = big & (br == name)
        worst[str(name)] = tuple(float(np.max(np.abs(g[m] - r[m]) / rK[m])) for g, r in ((K, rK), (GX, rGX), (GY, rGY)))
    for name, w in worst.items():
        print("%s, %s branch: worst |dK|/K %.2e, |dGX|/K %.2e, |dGY|/K %.2e" % (what, name, *w))
        assert max(w) <= RTOL, (what, name, w)
    return worst


def test_contract_on_the_table_random_pairs_and_every_switch_over(lib):
    """Measured with g++ -O2 (errors over K): near branch dK 2.8e-10, dGX 5.6e-8 (y = 1e-5, s just below 100: voigt_k's worst
    zone times 2 x^2), dGY 1.0e-13; mid branch all three below 2e-15; far branch dK 3.2e-11, dGX 3.9e-10, dGY 3.2e-11 (s = 400,
    the first neglected term of the five-term series); y == 0: dK 5.1e-14, dGX 5.3e-11 (exp's rounded argument times 2 x^2)."""
    kgrad, _ = lib
    z = load_golden("V1_voigt_dT")
    seen = set()
    for what, (x, y, ref) in point_sets(z).items():
        assert np.shape(ref[0]) == np.shape(x), what
        seen |= set(contract_errors(kgrad(x, y), ref, x, y, what))
    assert seen == {"y == 0", "near", "mid", "far"}


def test_K_is_voigt_k_bit_for_bit(lib):
    kgrad, k = lib
    for what, (x, y, _) in point_sets(load_golden("V1_voigt_dT")).items():
        assert np.array_equal(kgrad(x, y)[0], k(x, y)), what
    x = np.concatenate([np.logspace(-8, 9, 3000), [0.0, 1e160, 1e300, np.inf]])
    for y in (0.0, 1e-9, 1e-5, 0.3, 7.0, 1e4, 1e7):
        assert np.array_equal(kgrad(x, y)[0], k(x, y)), y


def test_edges_of_the_domain(lib):
    kgrad, _ = lib
    nan, inf = float("nan"), float("inf")
    for out in kgrad([nan, 1.0, nan, nan, 50.0, 3.0], [1.0, nan, 0.0, nan, nan, nan]):
        assert np.isnan(out).all()
    # y == 0: K = exp(-x^2), GX = -2 x^2 K, GY = 0
    xs = np.linspace(0, 27, 500)
    K, GX, GY = kgrad(xs, 0.0)
    assert np.allclose(K, np.exp(-xs * xs), rtol=1e-14, atol=0) and np.array_equal(GX, -2.0 * (xs * xs) * K) and not GY.any()
    assert [float(v[0]) for v in kgrad([0.0], [0.0])] == [1.0, 0.0, 0.0]
    # x == 0: GX = 0, and GY = y dK/dy of K(0, y) = exp(y^2) erfc(y): 2 y^2 K - 2 y / sqrt(pi)
    ys = np.logspace(-5, 4, 200)
    K, GX, GY = kgrad(0.0, ys)
    assert not GX.any() and np.all(GY < 0)
    near = ys < 5
    assert np.allclose(GY[near], 2 * ys[near] ** 2 * K[near] - 2 * ys[near] / np.sqrt(np.pi), rtol=0, atol=1e-12)
    # x^2 overflowing: all three are 0
    for y in (0.0, 1e-5, 1.0, 1e4):
        for out in kgrad([1e160, 1e300, inf], y):
            assert not out.any() and not np.isnan(out).any()
    # far beyond the table: GX <= 0, nothing NaN, GX -> -2 K and GY -> K of the Lorentz wing y / (sqrt(pi) x^2)
    K, GX, GY = kgrad([1e8, 1e150], [1e-5, 1.0])
    assert abs(GX[0] / (-2 * K[0]) - 1) < 1e-12 and abs(GY[0] / K[0] - 1) < 1e-12 and GX[1] <= 0 and np.isfinite(GY[1])
    # GX <= 0 everywhere, also off the fixture's points
    rng = np.random.default_rng(5)
    x, y = 10.0 ** rng.uniform(-6, 8, 200000), 10.0 ** rng.uniform(-9, 6, 200000)
    assert np.all(kgrad(x, y)[1] <= 0) and np.all(kgrad(x, 0.0)[1] <= 0)


def test_below_the_domain_in_y(lib):
    """0 < y < 1e-5 is outside the contract: the results are finite and GX <= 0; the errors over K are printed, not
    bounded (the near branch's absolute error of about 2e-16 against K = y / (sqrt(pi) x^2) grows like 1 / y, times 2 x^2
    in GX)."""
    mpmath = pytest.importorskip("mpmath")
    import make_voigt_dT_golden as mk
    kgrad, _ = lib
    x = np.logspace(-3, 5, 60)
    for y in (1e-6, 1e-7, 1e-8):
        K, GX, GY = kgrad(x, y)
        assert np.isfinite(K).all() and np.isfinite(GX).all() and np.isfinite(GY).all() and np.all(GX <= 0) and np.all(K >= 0)
        ref = np.array([[float(v) for v in mk.w_grad(xi, y)] for xi in x])
        err = [float(np.max(np.abs(g - ref[:, k]) / ref[:, 0])) for k, g in enumerate((K, GX, GY))]
        print("y = %g: worst |dK|/K %.2e, |dGX|/K %.2e, |dGY|/K %.2e" % (y, *err))
    assert mpmath.mp.dps >= 40


CELLS_REPRODUCED = ("p1", "p005", "doppler", "tiny", "isolated", "empty")     # the quick ones: W = 1 and 5, y = 0, H = 48
THIN = 23


def test_generator_reproduces_the_fixture():
    """A fixed subset (every 23rd function point, six of the ten cells, 20 self-check pairs each), in this process: the whole
    takes minutes of mpmath on one core."""
    pytest.importorskip("mpmath")
    import make_voigt_dT_golden as mk
    kept = load_golden("V1_voigt_dT")
    made = mk.build(cells=CELLS_REPRODUCED, thin=THIN, selfcheck_pairs=20, processes=0)
    names = json.loads(str(kept["cases"]))
    assert names == list(mvg.cases()) and len(names) == 10
    assert json.loads(str(made["cases"])) == [n for n in names if n in CELLS_REPRODUCED]
    assert sorted(kept.files) == sorted(["cases"] + [t + k for t in "frb" for k in ("K", "GX", "GY")]
                                        + ["%s.%s" % (n, k) for n in names for k in ("dxsec", "scale", "abs3")])
    for k in made:
        if k == "cases":
            continue
        want = kept[k].ravel()[::THIN] if k[0] in "frb" and "." not in k else kept[k]
        assert made[k].shape == want.shape and made[k].dtype == want.dtype == np.float64, k
        # (mpmath's values rounded once to fp64, sums formed in mpmath: the same bits wherever mpmath is the same)
        assert np.allclose(made[k], want, rtol=1e-13, atol=0, equal_nan=True), k
        assert np.array_equal(made[k] == 0, want == 0), k
    assert os.path.getsize(os.path.join(GOLDEN, mk.NAME)) < 1000 * 1024
    v0 = load_golden("V0_voigt")
    for n in names:
        c = mvg.load_case(v0, n)
        g = mvg.case_physics(c)[3]
        assert kept["%s.dxsec" % n].shape == kept["%s.scale" % n].shape == kept["%s.abs3" % n].shape == (g["n_base"],)
        assert np.all(kept["%s.scale" % n] >= 0) and np.all(np.abs(kept["%s.dxsec" % n]) <= kept["%s.abs3" % n] * (1 + 1e-12))
        # the derivative is non-zero exactly where the cross section is
        assert np.array_equal(kept["%s.abs3" % n] == 0, c["xsec"] == 0), n
    # the fixture's K is V0's (SciPy's wofz) to far better than the contract
    for t in "frb":
        big = kept[t + "K"] >= FLOOR
        assert np.allclose(kept[t + "K"][big], v0[t + "K"][big], rtol=1e-9, atol=0)


def test_new_kernels_use_no_scratch():
    """The compiler's report for the production build: voigt_dT_prep_kernel 37 VGPRs, 8 waves per SIMD, no LDS;
    voigt_dT_accumulate_kernel 90 VGPRs, 5 waves per SIMD, 12 KB of LDS per workgroup (3 KB per wave);
    voigt_gradient_kernel 30 VGPRs, 8 waves per SIMD.  No scratch, no spilled vector register."""
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB): the report beside the production objects is not its own")
    import test_kernel_resources_cpu as res
    kernels = res._kernels(res._remarks("lbl_kernels"))
    for sub, lds in (("voigt_dT_prep_kernel", 0), ("voigt_dT_accumulate_kernel", 4 * 64 * 48), ("voigt_gradient_kernel", 0)):
        hit = [f for n, f in kernels.items() if sub in n]
        assert len(hit) == 1, (sub, len(hit))
        f = hit[0]
        assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0, (sub, f)
        assert f["VGPRs"] <= 128 and f["Occupancy [waves/SIMD]"] >= 4, (sub, f)
        assert f["LDS Size [bytes/block]"] == lds, (sub, f)
    # K2v's kernels are found by the same substrings as before
    for sub in ("voigt_prep_kernel", "voigt_accumulate_kernel", "voigt_function_kernel"):
        assert len([n for n in kernels if sub in n]) == 1, sub


def test_binding_lists_the_new_symbols():
    with open(os.path.join(REPO, "include", "pyrad_hip.h")) as f:
        header = f.read()
    lib = _native.load()
    for name in ("lbl_xsec_voigt_dt_dev", "lbl_voigt_gradient_dev"):
        assert name in _native.SIGNATURES and re.search(r"\bint %s\(" % name, header) and hasattr(lib, name)
    assert "#define LBL_ABI_VERSION 5" in header and lib.lbl_abi_version() == 5
    assert callable(_native.Context.xsec_voigt_dT_dev) and callable(_native.Context.voigt_gradient_dev)
    # voigt_k's text is the one K2v was measured with
    text = open(HEADER).read()
    assert text.count("LBL_VOIGT_FN double voigt_k(") == 1 and text.count("LBL_VOIGT_FN void voigt_kgrad(") == 1


class _Stub:
    exotic = False
    name = "stub"


def test_model_refusals_need_no_device():
    from pyrad_amd import model, settings
    assert settings.LINE_SHAPE == "reference"
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("dT")
    layer = atm.addLayer(1e4, 288, 1013.25, 600, 601)
    with pytest.raises(ValueError, match="discontinuous in T"):
        layer.absCoefDT
    with pytest.raises(ValueError, match="discontinuous in T"):
        model.getAbsCoefDT(layer)
    with pytest.raises(ValueError, match="temperature"):
        atm.jacobians(surfaceTemperature=288, temperature="bogus")
    with pytest.raises(ValueError, match="discontinuous in T"):
        atm.jacobians(surfaceTemperature=288, temperature="full")
    settings.set_line_shape("voigt")
    try:
        xsc = _Stub()
        xsc.exotic = True
        list.append(layer, xsc)
        with pytest.raises(ValueError, match="measured cross-section table"):
            layer._check_abs_coef_dT()
        list.pop(layer)
        layer._check_abs_coef_dT()
    finally:
        settings.set_line_shape("reference")
        model.Layer.hasAtmosphere = False


def test_dlnq_dT_from_the_table():
    from pyrad_amd import model

    class Iso:
        pass
    iso = Iso()
    iso.layer = Iso()
    iso.q = {T: 100.0 * (T / 296.0) ** 1.5 for T in range(200, 301)}
    iso.layer.T = 250
    assert model._dlnq_dT(iso) == (iso.q[251] - iso.q[249]) / (2 * iso.q[250])
    assert abs(model._dlnq_dT(iso) - 1.5 / 250) < 1e-7
    iso.layer.T = 200
    assert model._dlnq_dT(iso) == (iso.q[201] - iso.q[200]) / iso.q[200]
    iso.layer.T = 300
    assert model._dlnq_dT(iso) == (iso.q[300] - iso.q[299]) / iso.q[300]
    iso.layer.T = 250.5
    with pytest.raises(KeyError):
        model._dlnq_dT(iso)
