"""Radiances through scattering layers (lbl_column_radiance_scatter_dev, Atmosphere.radianceTwoStream) without a device:
the restatement of tests/scatter_radiance_ref.py against mpmath at 50 digits - the column's fluxes solved there, the ODE's
exact solution inside every layer and the layer integral by mpmath.quad of the defined source function, no closed form -
on K5m's seven cases, at lam mu = 1 and beside it, in conservative layers, in very thin and very thick layers and without
layers; the three identities; the declarations and the binding; the model's validation.

Measured (this file prints every figure): the restatement stays within 3.6e-16 of the point's scale / pi of the 50-digit
values on the seven cases, 1.4e-16 through lam mu = 1, 3.8e-16 in the conservative layers and 2.9e-16 in the thin and thick
ones.  The bound asserted is 1e-13, what the GPU tests' 1e-12 rests on, in every regime: no float64 regime needed a wider one
(near-conservative layers included: the sinh-ratio basis tends to the linear solution), so the GPU tolerance is 1e-12
throughout and the factor ten between the two covers the kernel's other order of operations and its exp."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scatter_flux_ref as flux
import scatter_radiance_ref as ref
import twostream_ref as two
from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
ARGUMENTS = ("ctx n_layers abs_coef T planck_linear depth range_min range_max n I_surface surface_T I_top n_scat scat_amount "
             "scat_ext scat_ext_all scat_ssa scat_ssa_all scat_asym scat_asym_all delta_scaling emissivity emissivity_all "
             "n_views view_mu view_down workspace radiance up_top down_surface").split()
LO, HI = 600.0, 700.0
MU3 = 1.0 / np.sqrt(3.0)
VIEWS = [(1.0, 0), (0.5, 0), (MU3, 0), (0.2, 1), (1.0, 1)]
BOUND = 1e-13


# ---- the same column as K5m's GPU tests build, without importing a GPU test ----------------------------------------------
def hand_made(seed, L=4, n=1029, scatterers=0, spectral=(), linear=True, joined=True):
    rs = np.random.RandomState(seed)
    k = 10.0 ** rs.uniform(-10, -2, (L, n))
    depth = np.full(L, 1e4)
    if not linear:
        T = rs.uniform(200, 300, L)
    elif joined:
        lev = rs.uniform(200, 300, L + 1)
        T = np.column_stack([lev[:-1], lev[1:]])
    else:
        T = rs.uniform(200, 300, (L, 2))
    amount = 10.0 ** rs.uniform(-3, 1, (scatterers, L))
    numbers = []
    for c in range(scatterers):
        if c in spectral:
            numbers.append((rs.uniform(0.2, 2.0, n), rs.uniform(0.3, 1.0, n), rs.uniform(-0.3, 0.9, n)))
        else:
            numbers.append((float(rs.uniform(0.2, 2.0)), float(rs.uniform(0.5, 1.0)), float(rs.uniform(-0.3, 0.9))))
    T = np.asarray(T, dtype=np.float64)
    edges = T.reshape(-1, 2) if linear else np.column_stack([T, T])
    return dict(k=k, depth=depth, edges=edges, amount=amount, numbers=numbers)


CASES = {
    "gas alone, layer source": (dict(seed=51, linear=False), 1, 1.0, "T", False),
    "gas alone, linear source": (dict(seed=52, linear=True), 1, 0.3, "I", True),
    "one scatterer, layer source, unscaled": (dict(seed=53, linear=False, scatterers=1), 0, 0.0, "T", True),
    "one spectral scatterer, linear source": (dict(seed=54, linear=True, scatterers=1, spectral=(0,)), 1, "spectrum", "T", False),
    "four scatterers, layer source": (dict(seed=55, linear=False, scatterers=4, spectral=(0, 2)), 1, 0.3, "I", True),
    "four scatterers, linear source, unscaled, edges apart": (
        dict(seed=56, linear=True, joined=False, scatterers=4, spectral=(1, 3)), 0, "spectrum", "T", False),
    "four scatterers, linear source, black surface": (dict(seed=57, linear=True, scatterers=4), 1, 1.0, "I", True),
}


def boundaries(name, n):
    """the surface and the sky of a case: (e, I_surface, surface_T, I_top), as K5m's GPU tests set them"""
    _, _, e, surface, top = CASES[name]
    nu = np.linspace(LO, HI, n)
    if isinstance(e, str):
        e = 0.55 + 0.4 * np.sin(0.37 * np.arange(n)) ** 2
    Is = flux.planck(nu, 285.0) * (0.9 + 0.1 * np.cos(0.11 * np.arange(n))) if surface == "I" else None
    It = flux.planck(nu, 180.0) * (1.0 + 0.5 * np.sin(0.23 * np.arange(n)) ** 2) if top else None
    return e, Is, (291.5 if surface == "T" else None), It


# ---- 50 digits -----------------------------------------------------------------------------------------------------------
def mp_point(mp, k, depth, edges, nu, amount, numbers, delta, e, Is, It, views):
    """One grid point at 50 digits: k (L,), numbers as scalars, Is and It radiances (floats).  The Planck values are the
    float64 ones, taken as data.  Returns the radiances of ``views`` and (up, dn)."""
    f = mp.mpf
    L = len(k)
    Bb = [f(float(np.pi * flux.planck(nu, edges[l][0]))) for l in range(L)]
    Bt = [f(float(np.pi * flux.planck(nu, edges[l][1]))) for l in range(L)]
    ta, ts, tsg = [], [], []
    for l in range(L):
        a_, s_, g_ = f(float(k[l])) * f(float(depth[l])), f(0), f(0)
        for c, (ext, ssa, g) in enumerate(numbers):
            ext, ssa, g = f(float(ext)), f(float(ssa)), f(float(g))
            fd = g * g if delta else f(0)
            am = f(float(amount[c][l]))
            a_, s_, g_ = a_ + am * (ext * (1 - ssa)), s_ + am * ((ext * ssa) * (1 - fd)), g_ + am * ((ext * ssa) * (g - fd))
        ta.append(a_), ts.append(s_), tsg.append(g_)
    R, T, P, Q = [], [], [], []
    for l in range(L):
        r, t_ = two.layer_scalar(ta[l], ts[l], tsg[l], 1.0, f, mp.sqrt, mp.exp, mp.expm1)[:2]
        if ta[l] + ts[l] == 0 or ta[l] == 0:
            p, q = f(0), f(0)
        else:
            p, q = flux.sources_scalar(ta[l], ts[l], tsg[l], Bt[l], Bb[l], f, mp.sqrt, mp.exp, mp.expm1)
        R.append(r), T.append(t_), P.append(p), Q.append(q)
    # adding from the surface upwards, then down from the top (scatter_flux_ref.solve's relations)
    e = f(float(e))
    A, G = [1 - e], [e * mp.pi * f(float(Is))]
    for l in range(L):
        c = 1 - A[l] * R[l]
        A.append(R[l] + T[l] * T[l] * A[l] / c)
        G.append(P[l] + T[l] * (G[l] + A[l] * Q[l]) / c)
    dn = [None] * (L + 1)
    up = [None] * (L + 1)
    dn[L] = mp.pi * f(float(It))
    up[L] = A[L] * dn[L] + G[L]
    for l in range(L - 1, -1, -1):
        dn[l] = (T[l] * dn[l + 1] + Q[l] + R[l] * G[l]) / (1 - A[l] * R[l])
        up[l] = A[l] * dn[l] + G[l]
    out = []
    for mu, down in views:
        mu = f(float(mu))
        I = f(float(It)) if down else up[0] / mp.pi
        for l in (range(L - 1, -1, -1) if down else range(L)):
            t = ta[l] + ts[l]
            if t == 0:
                continue
            F, t, a, w, g, lam = ref.layer_scalar(ta[l], ts[l], tsg[l], Bt[l], Bb[l], up[l], dn[l + 1], f, mp.sqrt, mp.exp,
                                                  mp.expm1)
            S = ref.source_scalar(F, t, a, w, g, Bt[l], Bb[l], mu, down, f, mp.sqrt)
            # y: the way from the edge where the light leaves (t = 1e300 has no digits left for t - y)
            reach = min(t, 125 * mu) if t > 250 * mu else t     # (beyond: below exp(-125) of the scale)
            panels = int(mp.ceil(reach * (1 / mu + 2) / 10)) + 1
            pts = [reach * i / panels for i in range(panels + 1)]
            if down:
                J = mp.quad(lambda y: S(t - y, y) * mp.exp(-y / mu), pts) / mu
            else:
                J = mp.quad(lambda y: S(y, t - y) * mp.exp(-y / mu), pts) / mu
            I = I * mp.exp(-t / mu) + J / mp.pi
        out.append(I)
    return out, up, dn


def against_mp(mp, k, depth, edges, nu, amount, numbers, delta, e, Is, surface_T, It, views, points, per_point=None):
    """the restatement at every point of the given column against 50 digits at ``points``: the worst error of a radiance
    in units of the point's scale / pi.  ``per_point``: that many of the views at each point, taken in turn."""
    n = k.shape[1]
    got, up, dn = ref.radiance(k, depth, nu, edges, views, amount, numbers, delta, e, Is, surface_T, It)
    scale = flux.scale(nu, edges, Is, surface_T, It) / np.pi
    Es = Is if Is is not None else flux.planck(nu, surface_T)
    top = It if It is not None else np.zeros(n)
    ev = np.broadcast_to(np.asarray(e, dtype=np.float64), (n,))
    worst = 0.0
    for j in points:
        nums = [tuple(float(np.broadcast_to(v, (n,))[j]) for v in triple) for triple in numbers]
        pick = range(len(views)) if per_point is None else [(j * per_point + i) % len(views) for i in range(per_point)]
        want, _, _ = mp_point(mp, k[:, j], depth, edges, nu[j], amount, nums, delta, ev[j], Es[j], top[j],
                              [views[v] for v in pick])
        for i, v in enumerate(pick):
            worst = max(worst, float(abs(mp.mpf(float(got[v, j])) - want[i]) / scale[j]))
    return worst


@pytest.fixture(scope="module")
def mp():
    m = pytest.importorskip("mpmath")
    m.mp.dps = 50
    return m


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_mpmath_on_the_seven_cases(mp, name):
    """24 points of each case, the five views in turn from point to point (a quadrature at 50 digits per layer and view is
    what this file's time goes into): within 1e-13 of the scale (measured: at most 3.6e-16)"""
    make, delta = CASES[name][:2]
    n = 24
    case = hand_made(n=n, **make)
    e, Is, Ts, It = boundaries(name, n)
    nu = np.linspace(LO, HI, n)
    worst = against_mp(mp, case["k"], case["depth"], case["edges"], nu, case["amount"], case["numbers"], delta, e, Is, Ts, It,
                       VIEWS, range(n), per_point=1)
    print("%s: the restatement within %.2e of the scale of 50 digits" % (name, worst))
    assert worst <= BOUND


def lam_of(k, depth, amount, numbers, delta):
    ta, ts, tsg = two.optical(k, depth, amount, numbers, delta)
    t = ta + ts
    return np.sqrt((ref.D * (ta / t)) * (ref.D * ((t - tsg) / t)))


def test_restatement_through_lam_mu_equal_to_one(mp):
    """views whose mu is 1 / lam of a chosen layer and point, exactly and 1e-9, 1e-6, 1e-3 to either side, up and down:
    no point is left out (measured: at most 1.4e-16 of the scale)"""
    n = 8
    rs = np.random.RandomState(21)
    L = 3
    depth = np.full(L, 1e4)
    t_gas = 10.0 ** rs.uniform(-2, 1, (L, n))
    k = t_gas / depth[:, None]
    amount = np.array([[0.5, 2.0, 0.1]])
    numbers = [(1.0, 0.6, 0.5)]
    edges = np.array([[290.0, 275.0], [275.0, 250.0], [250.0, 230.0]])
    nu = np.linspace(LO, HI, n)
    lam = lam_of(k, depth, amount, numbers, 1)
    assert np.all((lam[1] > 1.0) & (lam[1] < ref.D))
    worst = 0.0
    for j, layer in ((2, 1), (5, 0)):
        mu0 = 1.0 / lam[layer, j]
        assert 0 < mu0 <= 1
        views = []
        for d in (0.0, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3):
            views += [(mu0 * (1 + d), 0), (mu0 * (1 + d), 1)]
        assert (1.0 - lam[layer, j] * mu0) * 1.0 == 0.0 or abs(1.0 - lam[layer, j] * mu0) < 3e-16
        worst = max(worst, against_mp(mp, k, depth, edges, nu, amount, numbers, 1, 0.4, None, 295.0,
                                      flux.planck(nu, 170.0), views, [j]))
    print("lam mu = 1 and beside it: the restatement within %.2e of the scale of 50 digits" % worst)
    assert worst <= BOUND


def test_restatement_in_conservative_layers(mp):
    """ssa == 1 with gas optical depths 1e-6 and 0 (the den == 0 branch), cloud optical depths 1e-3 .. 30 (measured: at most
    3.8e-16 of the scale)"""
    n = 6
    L = 3
    depth = np.full(L, 1e4)
    nu = np.linspace(LO, HI, n)
    edges = np.array([[285.0, 270.0], [270.0, 240.0], [240.0, 225.0]])
    amount = np.array([[1e-3, 30.0, 1.0]])
    numbers = [(1.0, 1.0, 0.7)]
    worst = 0.0
    for t_gas in (1e-6, 0.0):
        k = np.full((L, n), t_gas / 1e4)
        for delta in (0, 1):
            worst = max(worst, against_mp(mp, k, depth, edges, nu, amount, numbers, delta, 0.7, None, 290.0,
                                          flux.planck(nu, 150.0), VIEWS, [0, n - 1]))
    print("conservative layers: the restatement within %.2e of the scale of 50 digits" % worst)
    assert worst <= BOUND


def test_restatement_in_very_thin_and_very_thick_layers(mp):
    """layers of t = 1e-12, 1e3 and 1e300 among ordinary ones, and a column without layers (measured: at most 2.9e-16 of
    the scale; without layers the values are the boundary's, exactly)"""
    n = 4
    nu = np.linspace(LO, HI, n)
    depth = np.full(3, 1e4)
    edges = np.array([[285.0, 270.0], [270.0, 240.0], [240.0, 225.0]])
    amount = np.array([[0.3, 1.0, 0.5]])
    numbers = [(1.0, 0.9, 0.6)]
    worst = 0.0
    for t_odd in (1e-12, 1e3, 1e300):
        for where in range(3):
            k = np.full((3, n), 0.2 / 1e4)
            k[where] = t_odd / 1e4
            am = amount.copy()
            am[0, where] = t_odd * 2.0
            worst = max(worst, against_mp(mp, k, depth, edges, nu, am, numbers, 1, 0.5, None, 290.0,
                                          flux.planck(nu, 160.0), VIEWS, [1]))
    print("t = 1e-12, 1e3, 1e300: the restatement within %.2e of the scale of 50 digits" % worst)
    assert worst <= BOUND
    It, Is = flux.planck(nu, 160.0), flux.planck(nu, 290.0)
    got, up, dn = ref.radiance(np.zeros((0, n)), [], nu, np.zeros((0, 2)), VIEWS, emissivity=0.5, I_surface=Is, I_top=It)
    for v, (mu, down) in enumerate(VIEWS):
        assert np.array_equal(got[v], It if down else up[0] / np.pi)
    assert np.allclose(up[0], 0.5 * np.pi * Is + 0.5 * np.pi * It, rtol=1e-15)


# ---- the identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_at_the_two_stream_angle_the_radiance_is_the_flux(name):
    """mu = 1 / sqrt(3): pi Iu_L == up_L and pi Id_0 == dn_0, to 1e-13 of the scale"""
    make, delta = CASES[name][:2]
    n = 300
    case = hand_made(n=n, **make)
    e, Is, Ts, It = boundaries(name, n)
    nu = np.linspace(LO, HI, n)
    got, up, dn = ref.radiance(case["k"], case["depth"], nu, case["edges"], [(MU3, 0), (MU3, 1)], case["amount"],
                               case["numbers"], delta, e, Is, Ts, It)
    scale = flux.scale(nu, case["edges"], Is, Ts, It)
    err = max(np.max(np.abs(np.pi * got[0] - up[-1]) / scale), np.max(np.abs(np.pi * got[1] - dn[0]) / scale))
    print("%s: pi I at 1 / sqrt(3) within %.2e of the scale of the fluxes" % (name, err))
    assert err <= BOUND


@pytest.mark.parametrize("linear", (False, True))
def test_without_scatterers_it_is_the_ray(linear):
    """S = B: the fold I <- t I + (1 - t) Ba + g(tau) (Bb - Ba), restated here directly, Ba where the light enters"""
    n = 300
    case = hand_made(62, n=n, linear=linear)
    nu = np.linspace(LO, HI, n)
    e = 0.55 + 0.4 * np.sin(0.37 * np.arange(n)) ** 2
    It = flux.planck(nu, 180.0)
    got, up, dn = ref.radiance(case["k"], case["depth"], nu, case["edges"], VIEWS, emissivity=e, surface_T=295.0, I_top=It)
    scale = flux.scale(nu, case["edges"], None, 295.0, It) / np.pi
    L = len(case["depth"])
    worst = 0.0
    for v, (mu, down) in enumerate(VIEWS):
        I = It.copy() if down else up[0] / np.pi
        for l in (range(L - 1, -1, -1) if down else range(L)):
            tau = case["k"][l] * case["depth"][l] / mu
            tr = np.exp(-tau)
            Bbot, Btop = flux.planck(nu, case["edges"][l, 0]), flux.planck(nu, case["edges"][l, 1])
            Ba, Bb = (Btop, Bbot) if down else (Bbot, Btop)
            I = tr * I + (1 - tr) * Ba + ref.g_linear(tau) * (Bb - Ba)
        worst = max(worst, np.max(np.abs(got[v] - I) / scale))
    print("no scatterers, %s source: within %.2e of the scale of the fold" % ("linear" if linear else "layer", worst))
    assert worst <= BOUND


def test_kirchhoff_cavity():
    """one temperature everywhere, the sky included: I = B(T0) for every view, whatever scatters and whatever e"""
    rs = np.random.RandomState(13)
    L, n, T0 = 6, 300, 255.0
    nu = np.linspace(LO, HI, n)
    k = 10.0 ** rs.uniform(-10, -2, (L, n))
    depth = np.full(L, 1e4)
    amount = 10.0 ** rs.uniform(-3, 1, (2, L))
    numbers = [(rs.uniform(0.2, 2.0, n), rs.uniform(0.3, 1.0, n), rs.uniform(-0.3, 0.9, n)) for _ in range(2)]
    B = flux.planck(nu, T0)
    worst = 0.0
    for e in (0.0, 0.3, 1.0, rs.uniform(0, 1, n)):
        for delta in (0, 1):
            got, _, _ = ref.radiance(k, depth, nu, np.full((L, 2), T0), VIEWS, amount, numbers, delta, e, surface_T=T0, I_top=B)
            worst = max(worst, np.max(np.abs(got / B - 1)))
    print("cavity: every view within %.2e of B" % worst)
    assert worst <= BOUND


def test_the_weights():
    """W0 + W1 + (what 1 - r0 - r1 takes) = W; at lam = 0 the weights are the linear interpolation's; all lie in [0, 1]"""
    rs = np.random.RandomState(31)
    u = np.concatenate([[0.0], 10.0 ** rs.uniform(-12, 3, 4000)])
    tau = 10.0 ** rs.uniform(-12, 3, u.size)
    W, W0, W1, Wh = ref.weights(u, tau, u / tau)
    assert np.all((W0 >= -1e-15) & (W0 <= 1 + 1e-15) & (W1 >= -1e-15) & (W1 <= 1 + 1e-15))
    assert np.all(W0 + W1 <= W + 1e-15) and np.max(np.abs(W - W0 - W1 - Wh)) <= 2e-15
    assert np.all(Wh >= -4e-16 * W) and np.all(Wh <= W)
    W, W0, W1, Wh = ref.weights(np.zeros(tau.size), tau, np.zeros(tau.size))
    assert np.all(np.abs(Wh) <= 3e-16 * W)
    G = W - ref.g_linear(tau)
    assert np.max(np.abs(W1 - G)) <= 1e-15 and np.max(np.abs(W0 - (W - G))) <= 1e-15


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    m = re.search(r"int\s+lbl_column_radiance_scatter_dev\s*\(([^;]*)\)\s*;", text)
    assert m, "lbl_column_radiance_scatter_dev is not declared"
    params = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert params == ARGUMENTS
    assert re.search(r"int\s+lbl_column_radiance_scatter_workspace\s*\(", text)
    assert hasattr(lib, "lbl_column_radiance_scatter_dev") and hasattr(lib, "lbl_column_radiance_scatter_workspace")
    assert len(_native.SIGNATURES["lbl_column_radiance_scatter_dev"][1]) == len(ARGUMENTS)
    assert len(_native.SIGNATURES["lbl_column_radiance_scatter_workspace"][1]) == 3
    assert hasattr(_native.Context, "column_radiance_scatter_dev")
    assert hasattr(_native.Context, "column_radiance_scatter_workspace")
    assert lib.lbl_abi_version() == 5
    assert _native.limit("scatter_views") == 16
    # the workspace is K5m's: four numbers per level and point, whole tiles of 256 points, one at least
    out, other = C.c_int64(), C.c_int64()
    for L, points in ((0, 0), (0, 1), (4, 256), (4, 257), (128, 1000)):
        assert lib.lbl_column_radiance_scatter_workspace(L, points, C.byref(out)) == 0
        assert lib.lbl_column_flux_scatter_workspace(L, points, C.byref(other)) == 0 and out.value == other.value
    for L, points in ((-1, 1), (129, 1), (3, -1)):
        assert lib.lbl_column_radiance_scatter_workspace(L, points, C.byref(out)) == -1
    assert lib.lbl_column_radiance_scatter_workspace(3, 1, None) == -1


def test_scatter_radiance_kernels_in_the_resource_report():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    mine = {n: f for n, f in k.items() if "scatter_radiance_up_kernel" in n}
    for n, f in sorted(mine.items()):
        print(n, f["VGPRs"], f["Occupancy [waves/SIMD]"])
        # (the views' cosines and directions are workgroup-uniform; those that do not fit the scalar file are kept in lanes of
        # a vector register, which touches no memory)
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (n, f)
    # the layer and the linear source, each for 1, 2, 4, 8 and 16 views
    assert len(mine) == 10, sorted(mine)


# ---- validation ----------------------------------------------------------------------------------------------------------
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))


@pytest.fixture()
def no_context(monkeypatch):
    """every check below must fail before the engine (and with it a device context) is asked for"""
    def refuse():
        raise AssertionError("the context was touched before the arguments were validated")
    monkeypatch.setattr(model, "_ctx", refuse)
    settings.set_resolution_multiplier(1)
    yield


def test_validation_before_any_device_work(no_context):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("scatter radiance")
    for depth, T, P in LAYERS:
        atm.addLayer(depth, T, P, 600, 610)
    n = len(atm[0].xAxis)
    nan = float("nan")
    S = model.Scatterer
    four = [1.0, 0.0, 2.0, 0.5]
    call = lambda views=(1.0,), **kw: atm.radianceTwoStream(views, **{"surfaceTemperature": 288.0, **kw})
    for bad in ((), [], 1.0, None, [0.0], [1.5], [nan], [-0.5], ["up"], [(0.5, "sideways")], [(0.5, "up", 1)], [(0.5,)],
                [(0.0, "down")], [(nan, "up")]):
        with pytest.raises(ValueError, match="views"):
            call(bad)
    for bad in ([S(four)] * 5, [S([1.0, 2.0])], [S(four), "haze"], 7, [None]):
        with pytest.raises(ValueError, match="scatterers"):
            call(scatterers=bad)
    with pytest.raises(ValueError, match="asymmetry"):
        call(scatterers=[S(four, asymmetry=1.0)])
    for d in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="deltaScaling"):
            call(deltaScaling=d)
    with pytest.raises(ValueError, match="surfaceSpectrum or surfaceTemperature"):
        atm.radianceTwoStream([1.0])
    with pytest.raises(ValueError, match="surfaceTemperature"):
        call(surfaceTemperature=0.0)
    with pytest.raises(ValueError, match="surfaceSpectrum"):
        call(surfaceSpectrum=np.ones(n - 1))
    with pytest.raises(ValueError, match="topSpectrum"):
        call(topSpectrum=np.ones(n + 1))
    for e in (-0.1, 1.1, nan, "black", None, np.full(n, 1.5), np.ones(n - 1)):
        with pytest.raises(ValueError, match="emissivity"):
            call(emissivity=e)
    for p in ("isothermal", 1, None):
        with pytest.raises(ValueError, match="planck"):
            call(planck=p)
    with pytest.raises(ValueError, match="levelTemperatures"):
        call(levelTemperatures=[300, 290, 280, 270, 260])
    for lev in ([300, 290, 280, 270], [300, 290, 280, 270, nan], "warm"):
        with pytest.raises(ValueError, match="levelTemperatures"):
            call(planck="linear", levelTemperatures=lev)
    with pytest.raises(ValueError, match="instrument"):
        call(instrument="a radiometer")
    for kw in (dict(bands=[(600.0, 605.0)]), dict(angles=3)):
        with pytest.raises(TypeError):
            call(**kw)
    assert hasattr(model, "ScatterRadiance")
    import pyrad_amd
    assert pyrad_amd.ScatterRadiance is model.ScatterRadiance
