"""CPU: Jacobians over a reflecting surface (Atmosphere.jacobians, pathJacobians and observe with an emissivity;
lbl_column_jacobian_surface_dev, lbl_ray_jacobian_surface_dev, lbl_ray_jacobian_surface_rows; kernels K5h) without a device -
the NumPy restatements of both semantics that the GPU tests compare against, checked here against central finite differences
of a NumPy forward model; the C ABI surface, the kernels' resource report, the row layout and the host-side validation, which
runs before anything touches a context."""
import os
import re

import numpy as np
import pytest

from oracle import pyrad_oracle as orc
from pyrad_amd import _native, model, settings
from test_jacobian_cpu import planck_dT

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
SYMBOLS = ("lbl_column_jacobian_surface_dev", "lbl_ray_jacobian_surface_dev", "lbl_ray_jacobian_surface_rows")
MARKER = -1           # the segment layer of a surface marker
BAD_ARG = -1


# ---- the column's semantics, restated in NumPy (the exact form: every level's radiance stored) ----------------------------
def weight_sum(w):
    total = 0.0
    for v in w:
        total += float(v)
    return total


def surface_flux(x, k, T, depth, mu, w, e, reflection, surface_T=None, surface=None, top=None, planck=orc.planckWavenumber):
    """upward spectral flux at the top over a surface of emissivity e: lbl_column_flux_surface_dev's forward model"""
    L = len(k)
    Is = np.array(surface, dtype=np.float64) if surface is not None else planck(x, surface_T)
    D = []
    for m in mu:
        I = np.zeros(x.size) if top is None else np.array(top, dtype=np.float64)
        for l in range(L - 1, -1, -1):
            t = np.exp(-k[l] * depth[l] / m)
            I = t * I + (1 - t) * planck(x, T[l])
        D.append(I)
    F0 = sum(wk * Dk for wk, Dk in zip(w, D))
    F = np.zeros(x.size)
    for m, wk, Dk in zip(mu, w, D):
        I = e * Is + (1 - e) * (F0 / weight_sum(w) if reflection == "lambertian" else Dk)
        for l in range(L):
            t = np.exp(-k[l] * depth[l] / m)
            I = t * I + (1 - t) * planck(x, T[l])
        F = F + wk * I
    return F


def surface_jacobian_reference(x, k, T, depth, mu, w, e, reflection, surface_T=None, surface=None, top=None, terms=(),
                               idx=None, res=1.0):
    """dict of band values (leading band axis) and spectra, from the formulas of include/pyrad_hip.h with every level
    radiance of both directions stored.  e: a number or x.size values; terms: (layer, k_m) pairs."""
    L, n = len(k), x.size
    idx = [(0, n)] if idx is None else idx
    e = e * np.ones(n)
    B = [orc.planckWavenumber(x, T[l]) for l in range(L)]
    dB = [planck_dT(x, T[l]) for l in range(L)]
    Is = np.array(surface, dtype=np.float64) if surface is not None else orc.planckWavenumber(x, surface_T)
    dBs = np.zeros(n) if surface is not None else planck_dT(x, surface_T)
    Wsum = weight_sum(w)
    with np.errstate(under="ignore"):
        t = [[np.exp(-k[l] * depth[l] / m) for l in range(L)] for m in mu]
        Id, Ttot = [], []
        for tk in t:                                   # Id[l + 1] enters layer l from above
            lev = [None] * (L + 1)
            lev[L] = np.zeros(n) if top is None else np.array(top, dtype=np.float64)
            for l in range(L - 1, -1, -1):
                lev[l] = tk[l] * lev[l + 1] + (1 - tk[l]) * B[l]
            Id.append(lev)
            Ttot.append(np.prod(tk, axis=0) if L else np.ones(n))
        F0 = sum(wk * lev[0] for wk, lev in zip(w, Id))
        S = sum(wk * tt for wk, tt in zip(w, Ttot))
        F, dTs, de = np.zeros(n), np.zeros(n), np.zeros(n)
        dtau, dT, core = np.zeros((L, n)), np.zeros((L, n)), np.zeros((L, n))
        for a, (m, wk) in enumerate(zip(mu, w)):
            R = F0 / Wsum if reflection == "lambertian" else Id[a][0]
            Q = (1 - e) * wk * (S / Wsum if reflection == "lambertian" else Ttot[a])
            Iu = [e * Is + (1 - e) * R]
            for l in range(L):
                Iu.append(t[a][l] * Iu[l] + (1 - t[a][l]) * B[l])
            A, C = [None] * L, [None] * L
            acc = np.ones(n)
            for l in range(L - 1, -1, -1):
                A[l] = acc
                acc = acc * t[a][l]
            acc = np.ones(n)
            for l in range(L):
                C[l] = acc
                acc = acc * t[a][l]
            F += wk * Iu[L]
            for l in range(L):
                gu = A[l] * t[a][l] * (B[l] - Iu[l])
                gd = C[l] * t[a][l] * (B[l] - Id[a][l + 1])
                core[l] += (wk * gu + Q * gd) / m
                dtau[l] += (k[l] * depth[l] / m) * (wk * gu + Q * gd)
                dT[l] += (wk * A[l] + Q * C[l]) * (1 - t[a][l]) * dB[l]
            dTs += e * wk * Ttot[a] * dBs
            de += wk * Ttot[a] * (Is - R)
    band = lambda y: np.array([res * np.sum(np.nan_to_num(y[..., i:j]), axis=-1) for i, j in idx])
    out = dict(olr=band(F), surfaceTemperature=band(dTs), emissivity=band(de), opticalDepth=band(dtau), temperature=band(dT),
               opticalDepthSpectrum=dtau, temperatureSpectrum=dT, emissivitySpectrum=de, olrSpectrum=F)
    out["terms"] = np.stack([band(km * depth[l] * core[l]) for l, km in terms], axis=-1) if terms else None
    return out


# ---- the rays' semantics ----------------------------------------------------------------------------------------------------
def surface_ray(x, k, T, layers, lengths, kind, e, surface_T=None, surface=None, planck=orc.planckWavenumber):
    """radiance of one ray of lbl_ray_radiance_surface_dev without surface_down: kind 1 starts with e Is, kind 0 in cold space;
    a layer of MARKER is where the ray meets the surface"""
    Is = None
    if surface is not None or surface_T is not None:
        Is = np.array(surface, dtype=np.float64) if surface is not None else planck(x, surface_T)
    I = e * Is * np.ones(x.size) if kind == 1 else np.zeros(x.size)
    with np.errstate(under="ignore"):
        for l, s in zip(layers, lengths):
            if l == MARKER:
                I = e * Is + (1 - e) * I
                continue
            t = np.exp(-k[l] * s)
            I = t * I + (1 - t) * planck(x, T[l])
    return I


def surface_path_jacobian_reference(x, k, T, layers, lengths, kind, e, surface_T=None, surface=None, terms=()):
    """dict(radiance, sourceTemperature, emissivity, opticalDepth {layer: row}, temperature {layer: row}, terms {term index:
    row}) of one ray, by the direct forms of include/pyrad_hip.h with the radiance arriving at every element stored"""
    n = x.size
    e = e * np.ones(n)
    Is = dBs = np.zeros(n)
    if surface is not None:
        Is = np.array(surface, dtype=np.float64)
    elif surface_T is not None:
        Is, dBs = orc.planckWavenumber(x, surface_T), planck_dT(x, surface_T)
    with np.errstate(under="ignore"):
        I = [e * Is if kind == 1 else np.zeros(n)]                 # I[s] arrives at element s
        f = []                                                     # what element s passes on of it
        for l, s in zip(layers, lengths):
            if l == MARKER:
                f.append(1 - e)
                I.append(e * Is + f[-1] * I[-1])
            else:
                f.append(np.exp(-k[l] * s))
                I.append(f[-1] * I[-1] + (1 - f[-1]) * orc.planckWavenumber(x, T[l]))
        crossed = sorted(set(l for l in layers if l != MARKER))
        dtau, dT = {l: np.zeros(n) for l in crossed}, {l: np.zeros(n) for l in crossed}
        rows = {m: np.zeros(n) for m, (l, km) in enumerate(terms) if l in crossed}
        dTs, de = np.zeros(n), np.zeros(n)
        A = np.ones(n)
        for s in range(len(layers) - 1, -1, -1):
            l, length = layers[s], lengths[s]
            if l == MARKER:
                dTs += A * e * dBs
                de += A * (Is - I[s])
            else:
                core = A * f[s] * (orc.planckWavenumber(x, T[l]) - I[s])
                dtau[l] += k[l] * length * core
                dT[l] += A * (1 - f[s]) * planck_dT(x, T[l])
                for m, (lm, km) in enumerate(terms):
                    if lm == l:
                        rows[m] += km * length * core
            A = A * f[s]
        if kind == 1:
            dTs += A * e * dBs
            de += A * Is
    return dict(radiance=I[-1], sourceTemperature=dTs, emissivity=de, opticalDepth=dtau, temperature=dT, terms=rows)


# ---- both restatements against central differences of the forward models ---------------------------------------------------
def _tiny_column(seed=5):
    """4 layers, 7 points, two molecules per layer, optical depths from thin to a few"""
    rng = np.random.default_rng(seed)
    x = np.linspace(640.0, 700.0, 7)
    k_m = [[rng.uniform(1e-6, 4e-5, x.size) for m in range(2)] for l in range(4)]
    k = [sum(km) for km in k_m]
    return x, k_m, k, [288.0, 262.0, 231.0, 214.0], [1.5e4, 4e4, 9e4, 7e4]


def _near(a, fd, scale, what):
    assert np.all(np.abs(a - fd) <= 1e-6 * np.abs(fd) + 1e-9 * scale), (what, a, fd)


@pytest.mark.parametrize("reflection", ["lambertian", "specular"])
def test_column_restatement_against_finite_differences(reflection):
    x, k_m, k, T, depth = _tiny_column()
    mu, w = model.fluxAngles(3)
    Ts = 295.0
    e = np.linspace(0.35, 0.95, x.size)
    top = 0.4 * orc.planckWavenumber(x, 250.0)
    terms = [(l, km) for l in range(len(k)) for km in k_m[l]]
    ref = surface_jacobian_reference(x, k, T, depth, mu, w, e, reflection, surface_T=Ts, top=top, terms=terms)
    scale = np.max(ref["olrSpectrum"])

    def F(k=k, T=T, depth=depth, e=e, Ts=Ts):
        return surface_flux(x, k, T, depth, mu, w, e, reflection, surface_T=Ts, top=top)

    assert np.allclose(ref["olrSpectrum"], F(), rtol=1e-14, atol=0)
    eps, h = 1e-4, 1e-2
    for l in range(len(k)):
        dp, dm = list(depth), list(depth)
        dp[l] *= np.exp(eps)
        dm[l] *= np.exp(-eps)
        _near(ref["opticalDepthSpectrum"][l], (F(depth=dp) - F(depth=dm)) / (2 * eps), scale, "ln tau %d" % l)
        Tp, Tm = list(T), list(T)
        Tp[l] += h
        Tm[l] -= h
        _near(ref["temperatureSpectrum"][l], (F(T=Tp) - F(T=Tm)) / (2 * h), scale, "T %d" % l)
    for t, (l, km) in enumerate(terms):
        kp, kn = list(k), list(k)
        kp[l] = k[l] + eps * km
        kn[l] = k[l] - eps * km
        _near(ref["terms"][0, t], np.sum((F(k=kp) - F(k=kn)) / (2 * eps)), scale, "term %d" % t)
    _near(ref["surfaceTemperature"][0], np.sum((F(Ts=Ts + h) - F(Ts=Ts - h)) / (2 * h)), scale, "T_s")
    # F is affine in e: the difference quotient is exact up to rounding
    fd = (F(e=e + 0.04) - F(e=e - 0.04)) / 0.08
    assert np.all(np.abs(ref["emissivitySpectrum"] - fd) <= 1e-12 * scale), (ref["emissivitySpectrum"], fd)
    for l in range(len(k)):
        assert np.allclose(ref["terms"][:, 2 * l] + ref["terms"][:, 2 * l + 1], ref["opticalDepth"][:, l], rtol=1e-12, atol=0)
    # over a black surface it is test_jacobian_cpu's restatement
    from test_jacobian_cpu import jacobian_reference
    black = jacobian_reference(x, k, T, depth, mu, w, surface_T=Ts, terms=terms)
    one = surface_jacobian_reference(x, k, T, depth, mu, w, 1.0, reflection, surface_T=Ts, top=top, terms=terms)
    for name in ("olr", "surfaceTemperature", "opticalDepth", "temperature", "terms"):
        assert np.allclose(one[name], black[name], rtol=1e-13, atol=0), name


RAYS = (([3, 2, 1, 0, MARKER, 0, 1, 2, 3], 0), ([3, 2, 1, 0, MARKER, 0, 1], 0), ([1, 0, MARKER, 0, 2], 1), ([MARKER, 0, 1, 2, 3], 0),
        ([2, 1, MARKER], 1), ([1, 0, MARKER, 0, MARKER, 0, 1], 0), ([MARKER], 0), ([MARKER], 1), ([0, 1, 2, 3], 1), ([], 1))


@pytest.mark.parametrize("ray", range(len(RAYS)))
def test_ray_restatement_against_finite_differences(ray):
    x, k_m, k, T, depth = _tiny_column()
    layers, kind = RAYS[ray]
    rs = np.random.RandomState(ray)
    lengths = [0.0 if l == MARKER else float(rs.uniform(1e4, 6e4)) for l in layers]
    Ts = 295.0
    e = np.linspace(0.35, 0.95, x.size)
    terms = [(l, km) for l in range(len(k)) for km in k_m[l]]
    ref = surface_path_jacobian_reference(x, k, T, layers, lengths, kind, e, surface_T=Ts, terms=terms)

    def I(k=k, T=T, lengths=lengths, e=e, Ts=Ts):
        return surface_ray(x, k, T, layers, lengths, kind, e, surface_T=Ts)

    scale = max(np.max(ref["radiance"]), 1e-300)
    assert np.allclose(ref["radiance"], I(), rtol=1e-14, atol=0)
    eps, h = 1e-4, 1e-2
    for l in range(len(k)):
        if l not in ref["opticalDepth"]:
            assert l not in layers
            continue
        lp = [s * np.exp(eps) if ll == l else s for ll, s in zip(layers, lengths)]
        lm = [s * np.exp(-eps) if ll == l else s for ll, s in zip(layers, lengths)]
        _near(ref["opticalDepth"][l], (I(lengths=lp) - I(lengths=lm)) / (2 * eps), scale, "ln tau %d" % l)
        Tp, Tm = list(T), list(T)
        Tp[l] += h
        Tm[l] -= h
        _near(ref["temperature"][l], (I(T=Tp) - I(T=Tm)) / (2 * h), scale, "T %d" % l)
    for t, (l, km) in enumerate(terms):
        assert (t in ref["terms"]) == (l in layers)
        if t in ref["terms"]:
            kp, kn = list(k), list(k)
            kp[l] = k[l] + eps * km
            kn[l] = k[l] - eps * km
            _near(ref["terms"][t], (I(k=kp) - I(k=kn)) / (2 * eps), scale, "term %d" % t)
    _near(ref["sourceTemperature"], (I(Ts=Ts + h) - I(Ts=Ts - h)) / (2 * h), scale, "T_s")
    # (with two markers the radiance is quadratic in e: a central difference is still exact for it)
    fd = (I(e=e + 0.04) - I(e=e - 0.04)) / 0.08
    assert np.all(np.abs(ref["emissivity"] - fd) <= 1e-12 * scale), (ref["emissivity"], fd)
    # a given source spectrum has no temperature
    given = surface_path_jacobian_reference(x, k, T, layers, lengths, kind, e, surface=orc.planckWavenumber(x, Ts))
    assert np.all(given["sourceTemperature"] == 0.0) and np.allclose(given["emissivity"], ref["emissivity"], rtol=1e-14)


# ---- the C ABI surface -------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r"int\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    sig = _native.SIGNATURES
    # the black-surface call's arguments plus I_top, the emissivity pair, the reflection and the dF/de spectrum
    assert len(sig["lbl_column_jacobian_surface_dev"][1]) == len(sig["lbl_column_jacobian_dev"][1]) + 5
    assert len(sig["lbl_ray_jacobian_surface_dev"][1]) == len(sig["lbl_ray_jacobian_dev"][1]) + 2
    assert sig["lbl_ray_jacobian_surface_rows"][1] == sig["lbl_ray_jacobian_rows"][1]
    assert hasattr(_native.Context, "column_jacobian_surface_dev") and hasattr(_native.Context, "ray_jacobian_surface_dev")
    assert lib.lbl_abi_version() == 5 and "#define LBL_ABI_VERSION 5" in text


def _template_args(name, kernel):
    m = re.search(kernel + r"I((?:L[ib]\d+E)+)E", name)
    assert m, name
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))


def test_surface_jacobian_kernels_in_the_resource_report():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    column = {_template_args(n, "surface_jacobian_kernel"): f for n, f in k.items()
              if "surface_jacobian_kernel" in n and "ray_surface_jacobian_kernel" not in n}
    rays = {_template_args(n, "ray_surface_jacobian_kernel"): f for n, f in k.items() if "ray_surface_jacobian_kernel" in n}
    # the head-and-tail kernel of one point per thread for 1..8 angles; K5d's 4 points per thread for 1 and 2 angles (its
    # groups of points: what makes a black surface return its bits), 2 beyond
    assert sorted(column) == sorted([(1, na) for na in range(1, 9)] + [(4, 1), (4, 2)] + [(2, na) for na in range(3, 9)])
    # bundles of 4 rays with and without the term loop, single rays, the tail: always 4 points per thread on the body
    assert sorted(rays) == [(1, 1, 1), (4, 1, 1), (4, 4, 0), (4, 4, 1)]
    for args, f in list(column.items()) + list(rays.items()):
        print(args, f["VGPRs"], f.get("AGPRs"), f["Occupancy [waves/SIMD]"], f.get("LDS Size [bytes/block]"))
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (args, f)
    for args, f in rays.items():
        assert f.get("LDS Size [bytes/block]") == 0, (args, f)


# ---- the row layout ----------------------------------------------------------------------------------------------------------
def layout(rays, terms=()):
    """per ray 2 + 2 c + m rows: c distinct layers (a marker is none), m terms in one of them"""
    first = [0]
    for lay in rays:
        crossed = set(lay) - {MARKER}
        first.append(first[-1] + 2 + 2 * len(crossed) + sum(1 for l in terms if l in crossed))
    return first


def rows_of(rays, terms=(), n_layers=4, surface=True):
    ray_first = np.cumsum([0] + [len(r) for r in rays])
    return _native.ray_jacobian_rows(n_layers, ray_first, [l for r in rays for l in r], terms, surface=surface)


def test_rows_of_rays_with_markers():
    mirror = [3, 2, 1, 0, MARKER, 0, 1, 2, 3]                # every layer crossed twice: four distinct layers
    first, rows = rows_of([mirror])
    assert list(first) == [0, 10] and rows == 10
    first, rows = rows_of([[MARKER]])                       # a marker alone: dI/dT_source and dI/de
    assert list(first) == [0, 2] and rows == 2
    first, rows = rows_of([[]])
    assert list(first) == [0, 2] and rows == 2
    rays = [mirror, [MARKER], [], [0, 1, 2, 3], [MARKER, MARKER], [2, 1, MARKER, 1], [1, 0, MARKER, 0, MARKER, 0, 1]]
    first, rows = rows_of(rays)
    assert list(first) == layout(rays) == [0, 10, 12, 14, 24, 26, 32, 38] and rows == 38
    terms = [0, 0, 1, 3, 3, 2, 0]
    first, rows = rows_of(rays, terms)
    assert list(first) == layout(rays, terms) and rows == layout(rays, terms)[-1]
    # one row more per ray than the black-surface layout wherever that one exists
    plain = [[0, 1, 2, 3], [3, 2, 1, 2, 3], [], [1, 1, 0, 1]]
    a, b = rows_of(plain, terms, surface=False), rows_of(plain, terms)
    assert list(b[0] - a[0]) == [0, 1, 2, 3, 4] and b[1] == a[1] + 4
    # the black-surface layout goes on refusing the marker; both refuse a layer that is neither
    with pytest.raises(_native.LblError):
        rows_of([mirror], surface=False)
    for bad in ([0, -2, 1], [0, 4, 1]):
        with pytest.raises(_native.LblError) as err:
            rows_of([bad])
        assert err.value.code == BAD_ARG


# ---- validation before any device work -------------------------------------------------------------------------------------
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


def test_validation_before_any_device_work(no_context):
    atm = _atmosphere()
    n = len(atm[0].xAxis)
    nadir, mirror = atm.nadirPath(), atm.reflectedPath()
    ins = model.Instrument(np.arange(601.5, 608.6, 0.25), width=0.5)
    bad_e = (-0.01, 1.5, float("nan"), "water", True, np.full(n, 1.01), np.full(n, -1e-9), np.full(n - 1, 0.9),
             np.full((2, n), 0.9), np.where(np.arange(n) == 7, np.nan, 0.9), ([600.0, 605.0], [0.9, 1.2]),
             ([605.0, 600.0], [0.9, 0.8]), ([600.0, 605.0, 610.0], [0.9, 0.8]))
    for e in bad_e:
        with pytest.raises(ValueError, match="emissivity"):
            atm.jacobians(surfaceTemperature=288, emissivity=e)
        with pytest.raises(ValueError, match="emissivity"):
            atm.pathJacobians(mirror, surfaceTemperature=288, emissivity=e, reflection="specular")
        with pytest.raises(ValueError, match="emissivity"):
            atm.observe(ins, surfaceTemperature=288, emissivity=e)
    for r in ("mirror", "Lambertian", 0, None):
        with pytest.raises(ValueError, match="reflection"):
            atm.jacobians(surfaceTemperature=288, emissivity=0.9, reflection=r)
        with pytest.raises(ValueError, match="reflection"):
            atm.pathJacobians(mirror, surfaceTemperature=288, emissivity=0.9, reflection=r)
    with pytest.raises(ValueError, match="reflection"):
        atm.jacobians(surfaceTemperature=288, reflection="mirror")            # also without an emissivity
    with pytest.raises(ValueError, match="reflection"):
        atm.pathJacobians(nadir, surfaceTemperature=288, reflection="mirror")
    # the top spectrum: only over a surface that reflects it, and n values
    with pytest.raises(ValueError, match="topSpectrum"):
        atm.jacobians(surfaceTemperature=288, topSpectrum=np.zeros(n))
    with pytest.raises(ValueError, match="topSpectrum"):
        atm.jacobians(surfaceTemperature=288, emissivity=0.9, topSpectrum=np.zeros(n - 1))
    # weights that do not add up to more than 0: refused over a reflecting surface only
    for a in ([(0.5, 1.0), (0.25, -1.0)], [(0.5, 0.0)]):
        with pytest.raises(ValueError, match="angles"):
            atm.jacobians(surfaceTemperature=288, emissivity=0.9, angles=a)
    with pytest.raises(AssertionError, match="context"):
        atm.jacobians(surfaceTemperature=288, angles=[(0.5, 0.0)])
    # a path from the surface under the diffuse reflection: its sky term is not differentiated
    for paths in (nadir, [mirror, nadir]):
        with pytest.raises(ValueError, match="lambertian"):
            atm.pathJacobians(paths, surfaceTemperature=288, emissivity=0.9)
        with pytest.raises(ValueError, match="lambertian"):
            atm.pathJacobians(paths, surfaceTemperature=288, emissivity=0.9, reflection="lambertian")
    # ... which "specular" takes, as "lambertian" takes paths that do not start at the surface: as far as the context
    with pytest.raises(AssertionError, match="context"):
        atm.pathJacobians([mirror, nadir], surfaceTemperature=288, emissivity=0.9, reflection="specular")
    with pytest.raises(AssertionError, match="context"):
        atm.pathJacobians([mirror, atm.zenithPath()], surfaceTemperature=288, emissivity=0.9)
    # a bounce without an emissivity
    with pytest.raises(ValueError, match="bounce"):
        atm.pathJacobians(mirror, surfaceTemperature=288)
    with pytest.raises(ValueError, match="bounce"):
        atm.pathJacobians([nadir, mirror], surfaceTemperature=288, reflection="specular")
    # a bounce needs the surface source, with an emissivity too
    with pytest.raises(ValueError, match="surface"):
        atm.pathJacobians(mirror, emissivity=0.9)
    # and what the three refused before, they refuse with an emissivity too
    with pytest.raises(ValueError, match="surface"):
        atm.jacobians(emissivity=0.9)
    with pytest.raises(ValueError, match="temperature"):
        atm.jacobians(surfaceTemperature=288, emissivity=0.9, temperature="all")
    with pytest.raises(ValueError, match="mu"):
        atm.observe(ins, surfaceTemperature=288, emissivity=0.9, mu=0.0)
    with pytest.raises(ValueError, match="layer 4"):
        atm.pathJacobians(model.Path([4], [1.0], source="space", bounce=1), surfaceTemperature=288, emissivity=0.9)


def test_result_objects_carry_the_emissivity_fields():
    j = model.Jacobians(1.0, 2.0, np.zeros(2), np.zeros(2), None, [], [1.0], [1.0])
    assert j.emissivity is None and j.emissivitySpectrum is None
    j = model.Jacobians(1.0, 2.0, np.zeros(2), np.zeros(2), None, [], [1.0], [1.0], emissivity=3.0, emissivitySpectrum=np.ones(4))
    assert j.emissivity == 3.0 and j.emissivitySpectrum.shape == (4,)
    p = model.PathJacobians(np.ones(3), np.ones((1, 3)), np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), None, None, [], [])
    assert p.emissivity is None
    p = model.PathJacobians(np.ones(3), np.ones((1, 3)), np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), None, None, [], [],
                            emissivity=np.ones((1, 3)))
    assert p.emissivity.shape == (1, 3)
    o = model.Observation(np.array([650.0]), np.array([0.1]), 1.0)
    assert o.emissivityJacobian is None
    o = model.Observation(np.array([650.0]), np.array([0.1]), 1.0, emissivityJacobian=np.array([0.2]))
    assert o.emissivityJacobian[0] == 0.2
