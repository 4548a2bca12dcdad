"""CPU: the Jacobian feature (Atmosphere.jacobians, lbl_column_jacobian_dev) without a device - the C ABI surface, the
kernels' resource report, the host-side validation, and the NumPy restatement of the semantics that the GPU tests compare
against, checked here against central finite differences of a NumPy fold."""
import os
import re

import numpy as np
import pytest

from oracle import pyrad_oracle as orc
from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")


# ---- the semantics, restated in NumPy (the exact form: every level's radiance stored) -------------------------------------
def planck_dT(x, T):
    """dB/dT of planckWavenumber: B b e^b / ((e^b - 1) T), b = 100 h c x / (k T)"""
    b = 100 * orc.h * orc.c * np.asarray(x, dtype=np.float64) / orc.k / float(T)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return orc.planckWavenumber(x, T) * b * np.exp(b) / ((np.exp(b) - 1) * float(T))


def fold(x, k, T, depth, mu, w, surface_T=None, surface=None, planck=orc.planckWavenumber):
    """upward spectral flux at the top, sum_k W_k I_Lk"""
    I0 = np.array(surface, dtype=np.float64) if surface is not None else planck(x, surface_T)
    F = np.zeros(x.size)
    for m, wk in zip(mu, w):
        I = I0.copy()
        for l in range(len(k)):
            t = np.exp(-k[l] * depth[l] / m)
            I = t * I + (1 - t) * planck(x, T[l])
        F += wk * I
    return F


def jacobian_reference(x, k, T, depth, mu, w, surface_T=None, surface=None, terms=(), idx=None, res=1.0):
    """dict of band values (leading band axis) and spectra, from the formulas of include/pyrad_hip.h with every I_lk stored.
    terms: (layer, k_m) pairs."""
    L, n = len(k), x.size
    idx = [(0, n)] if idx is None else idx
    B = [orc.planckWavenumber(x, T[l]) for l in range(L)]
    dB = [planck_dT(x, T[l]) for l in range(L)]
    I0 = np.array(surface, dtype=np.float64) if surface is not None else orc.planckWavenumber(x, surface_T)
    F = np.zeros(n)
    dtau = np.zeros((L, n))
    dT = np.zeros((L, n))
    dTs = np.zeros(n)
    core = np.zeros((L, n))            # sum_k (W_k / mu_k) A_lk t_lk (B_l - I_lk)
    for m, wk in zip(mu, w):
        t = [np.exp(-k[l] * depth[l] / m) for l in range(L)]
        I = [I0]
        for l in range(L):
            I.append(t[l] * I[l] + (1 - t[l]) * B[l])
        A = [None] * L
        a = np.ones(n)
        for l in range(L - 1, -1, -1):
            A[l] = a
            a = a * t[l]
        F += wk * I[L]
        for l in range(L):
            c = A[l] * t[l] * (B[l] - I[l])
            core[l] += (wk / m) * c
            dtau[l] += wk * (k[l] * depth[l] / m) * c
            dT[l] += wk * A[l] * (1 - t[l]) * dB[l]
        if surface is None:
            dTs += wk * a * planck_dT(x, surface_T)
    band = lambda y: np.array([res * np.sum(np.nan_to_num(y[..., i:j]), axis=-1) for i, j in idx])
    out = dict(olr=band(F), surfaceTemperature=band(dTs), opticalDepth=band(dtau), temperature=band(dT),
               opticalDepthSpectrum=dtau, temperatureSpectrum=dT)
    out["terms"] = np.stack([band(km * depth[l] * core[l]) for l, km in terms], axis=-1) if terms else None
    return out


def _tiny_column(seed=3):
    rng = np.random.default_rng(seed)
    x = np.linspace(600.0, 700.0, 211)
    k_m = [[rng.uniform(0, 2e-5, x.size) * (1 + np.sin(x / (3 + l + m))) for m in range(2)] for l in range(3)]
    k = [sum(km) for km in k_m]
    T = [288.0, 262.0, 231.0]
    depth = [1.5e4, 4e4, 9e4]
    return x, k_m, k, T, depth


@pytest.mark.parametrize("angles", [1, 3, [(1.0, 1.0), (0.35, 2.0)]])
def test_numpy_restatement_against_finite_differences(angles):
    x, k_m, k, T, depth = _tiny_column()
    mu, w = model.fluxAngles(angles)
    Ts = 295.0
    terms = [(l, km) for l in range(len(k)) for km in k_m[l]]
    idx = [(0, 100), (100, x.size)]
    ref = jacobian_reference(x, k, T, depth, mu, w, surface_T=Ts, terms=terms, idx=idx)

    def bands(F):
        return np.array([np.sum(F[i:j]) for i, j in idx])

    def close(a, b):
        assert np.all(np.abs(a - b) <= 1e-6 * np.abs(b) + 1e-12 * ref["olr"]), (a, b)

    assert np.allclose(ref["olr"], bands(fold(x, k, T, depth, mu, w, surface_T=Ts)), rtol=1e-14, atol=0)
    eps, h = 1e-4, 1e-2
    for l in range(len(k)):
        d = [list(depth), list(depth)]
        d[0][l] *= np.exp(eps)
        d[1][l] *= np.exp(-eps)
        fd = (bands(fold(x, k, T, d[0], mu, w, surface_T=Ts)) - bands(fold(x, k, T, d[1], mu, w, surface_T=Ts))) / (2 * eps)
        close(ref["opticalDepth"][:, l], fd)
        # Planck part: B(T_l +- h) with k fixed
        Tp, Tm = list(T), list(T)
        Tp[l] += h
        Tm[l] -= h
        fd = (bands(fold(x, k, Tp, depth, mu, w, surface_T=Ts)) - bands(fold(x, k, Tm, depth, mu, w, surface_T=Ts))) / (2 * h)
        close(ref["temperature"][:, l], fd)
    for t, (l, km) in enumerate(terms):
        kp, kn = list(k), list(k)
        kp[l] = k[l] + eps * km
        kn[l] = k[l] - eps * km
        fd = (bands(fold(x, kp, T, depth, mu, w, surface_T=Ts)) - bands(fold(x, kn, T, depth, mu, w, surface_T=Ts))) / (2 * eps)
        close(ref["terms"][:, t], fd)
    fd = (bands(fold(x, k, T, depth, mu, w, surface_T=Ts + h)) - bands(fold(x, k, T, depth, mu, w, surface_T=Ts - h))) / (2 * h)
    close(ref["surfaceTemperature"], fd)
    # the analytic dB/dT itself
    for TT in (200.0, 288.0):
        fd = (orc.planckWavenumber(x, TT + h) - orc.planckWavenumber(x, TT - h)) / (2 * h)
        assert np.allclose(planck_dT(x, TT), fd, rtol=1e-7, atol=0)
    # molecule terms of a layer add up to its optical-depth term
    for l in range(len(k)):
        assert np.allclose(ref["terms"][:, 2 * l] + ref["terms"][:, 2 * l + 1], ref["opticalDepth"][:, l], rtol=1e-12, atol=0)


def test_entry_point_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    assert re.search(r"int\s+lbl_column_jacobian_dev\s*\(", text)
    assert "lbl_column_jacobian_dev" in _native.SIGNATURES
    lib = _native.load()
    assert hasattr(lib, "lbl_column_jacobian_dev")
    assert lib.lbl_abi_version() == 5
    assert hasattr(_native.Context, "column_jacobian_dev")


def test_jacobian_terms_limit():
    assert _native.limit("jacobian_terms") == 512


def test_jacobian_kernels_use_no_scratch_and_do_not_spill():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    jac = {n: f for n, f in k.items() if "column_jacobian" in n}
    assert len(jac) == 16, sorted(jac)               # NP points per thread and 1 (head and tail) x 1..8 angles
    for n, f in jac.items():
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (n, f)


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
        raise AssertionError("jacobians() touched the context before validating its arguments")
    monkeypatch.setattr(model, "_ctx", refuse)
    settings.set_resolution_multiplier(1)
    yield


def test_validation_before_any_device_work(no_context, monkeypatch):
    with pytest.raises(ValueError, match="no layers"):
        model.Atmosphere("empty").jacobians(surfaceTemperature=288)
    with pytest.raises(ValueError, match="range"):
        _atmosphere(((600, 700), (600, 710))).jacobians(surfaceTemperature=288)
    atm = _atmosphere()
    with pytest.raises(ValueError, match="surface"):
        atm.jacobians()
    with pytest.raises(ValueError, match="surfaceTemperature"):
        atm.jacobians(surfaceTemperature=0)
    for bad in (0, 9, -1, "isotropic", [(0.0, 1.0)], [(1.2, 1.0)], [(0.5, 1.0)] * 9, [], [(0.5,)]):
        with pytest.raises(ValueError, match="angles"):
            atm.jacobians(surfaceTemperature=288, angles=bad)
    for bad in ([(500, 650)], [(650, 650)], [(701, 800)], [], [(650, 660)] * 65):
        with pytest.raises(ValueError, match="band"):
            atm.jacobians(surfaceTemperature=288, bands=bad)
    with pytest.raises(ValueError, match="surfaceSpectrum"):
        atm.jacobians(surfaceSpectrum=np.zeros(17))
    # more molecule terms than the library takes
    monkeypatch.setattr(model.Layer, "__len__", lambda self: 300)
    with pytest.raises(ValueError, match="molecule terms"):
        atm.jacobians(surfaceTemperature=288)
