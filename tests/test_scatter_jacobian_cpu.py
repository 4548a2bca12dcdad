"""lbl_column_jacobian_scatter_dev / Atmosphere.jacobiansTwoStream without a GPU: the restatement of
tests/scatter_jacobian_ref.py (closed-form layer partials, the adjoint of the dense level system) against mpmath at 50 digits
- the column in scalar arithmetic (twostream_ref.layer_scalar, scatter_flux_ref.sources_scalar, adding), differentiated by
central differences whose truncation is below 1e-25, and exactly where the flux is linear (the Planck values, the surface's
emission) - then the declarations, the bindings, the kernels' resources and the model's validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scatter_flux_ref as flux
import scatter_jacobian_ref as ref
import twostream_ref as two
from pyrad_amd import _native, model, settings
from test_scatter_radiance_cpu import CASES, HI, LO, boundaries, hand_made

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
ARGUMENTS = ("ctx n_layers abs_coef T planck_linear depth range_min range_max n I_surface surface_T I_top n_scat scat_amount "
             "scat_ext scat_ext_all scat_ssa scat_ssa_all scat_asym scat_asym_all delta_scaling n_bands band_first band_count "
             "emissivity emissivity_all n_terms term_abs_coef term_layer workspace jac jac_ln_tau_spectra jac_T_spectra "
             "up_top").split()
# four times the worst distance of the restatement from 50 digits measured on this file's cases (DESIGN.md "K5p")
MEASURED = 8.3e-16
BOUND = 4 * MEASURED
BAD_ARG = -1          # LBL_ERR_BAD_ARG
STEP = 1e-15            # relative step of the central differences at 50 digits: truncation ~ STEP^2 |f'''| / 6 < 1e-29


@pytest.fixture(scope="module")
def mp():
    m = pytest.importorskip("mpmath")
    m.mp.dps = 50
    return m


def mp_rows(mp, k, depth, edges, nu, linear, amount, numbers, delta, e, Es, It):
    """One grid point at 50 digits: (F, dF/dEs, dF/de, dF/d ln tau (L), dF/dB (L x [bottom, top]; layer source: their sum in
    [0]), dF/d ln amount (C x L)).  k (L,), numbers scalars, Es = pi Is and It floats.  The Planck values are the float64
    ones, taken as data: F is linear in them."""
    f = mp.mpf
    L, Cn = len(k), len(numbers)
    Bb0 = [f(float(np.pi * flux.planck(nu, edges[l][0]))) for l in range(L)]
    Bt0 = [f(float(np.pi * flux.planck(nu, edges[l][1]))) for l in range(L)]
    coef = []
    for ext, ssa, g in numbers:
        ext, ssa, g = f(float(ext)), f(float(ssa)), f(float(g))
        fd = g * g if delta else f(0)
        coef.append((ext * (1 - ssa), (ext * ssa) * (1 - fd), (ext * ssa) * (g - fd)))

    def F(gas=None, am=None, e_=None, Es_=None, Bb=Bb0, Bt=Bt0):
        ta, ts, tsg = [], [], []
        for l in range(L):
            a_ = f(float(k[l])) * f(float(depth[l])) * (gas[l] if gas else 1)
            s_, g_ = f(0), f(0)
            for c, (al, si, et) in enumerate(coef):
                x = f(float(amount[c][l])) * (am[c][l] if am else 1)
                a_, s_, g_ = a_ + x * al, s_ + x * si, g_ + x * et
            ta.append(a_), ts.append(s_), tsg.append(g_)
        return ref.column_scalar(ta, ts, tsg, Bb, Bt, f(float(e)) if e_ is None else e_, f(float(Es)) if Es_ is None else Es_,
                                 mp.pi * f(float(It)), linear, f, mp.sqrt, mp.exp, mp.expm1)

    h = f(STEP)
    ones = [f(1)] * L
    base = F()
    dEs = F(Es_=f(float(Es)) + 1) - base
    de = (F(e_=f(float(e)) + h) - F(e_=f(float(e)) - h)) / (2 * h)
    dtau, dB, dam = [], [], []
    for l in range(L):
        up_, dn_ = list(ones), list(ones)
        up_[l], dn_[l] = mp.exp(h), mp.exp(-h)
        dtau.append((F(gas=up_) - F(gas=dn_)) / (2 * h))
        Bb, Bt = list(Bb0), list(Bt0)
        Bb[l] += 1
        if linear:
            Bt[l] += 1
            dB.append((F(Bb=Bb) - base, F(Bt=Bt) - base))
        else:
            dB.append((F(Bb=Bb) - base, f(0)))
    for c in range(Cn):
        row = []
        for l in range(L):
            up_ = [list(ones) for _ in range(Cn)]
            dn_ = [list(ones) for _ in range(Cn)]
            up_[c][l], dn_[c][l] = mp.exp(h), mp.exp(-h)
            row.append((F(am=up_) - F(am=dn_)) / (2 * h))
        dam.append(row)
    return base, dEs, de, dtau, dB, dam


def against_mp(mp, k, depth, edges, nu, linear, amount, numbers, delta, e, Is, surface_T, It, points):
    """the restatement against 50 digits at ``points``: the worst error of F, dF/de and the logarithmic derivatives in units
    of the point's scale, and of the temperature rows in units of pi times the largest dB/dT that enters the point"""
    n = k.shape[1]
    L = len(depth)
    J = ref.jacobian(k, depth, nu, edges, linear, amount, numbers, delta, e, Is, surface_T, It)
    for v in J.values():
        assert np.all(np.isfinite(v))
    scale = flux.scale(nu, edges, Is, surface_T, It)
    temps = list(np.unique(edges)) + ([surface_T] if Is is None else [])
    unit_T = np.pi * np.max([ref.planck_dT(nu, T) for T in temps], axis=0)
    Es = np.pi * (Is if Is is not None else flux.planck(nu, surface_T))
    dEs_dT = np.pi * ref.planck_dT(nu, surface_T) if Is is None else np.zeros(n)
    top = It if It is not None else np.zeros(n)
    ev = np.broadcast_to(np.asarray(e, dtype=np.float64), (n,))
    worst, worst_T = 0.0, 0.0
    for j in points:
        nums = [tuple(float(np.broadcast_to(v, (n,))[j]) for v in triple) for triple in numbers]
        F, dEs, de, dtau, dB, dam = mp_rows(mp, k[:, j], depth, edges, nu[j], linear, amount, nums, delta, ev[j], Es[j], top[j])
        err = lambda got, want: float(abs(mp.mpf(float(got)) - want))
        errs = [err(J["F"][j], F), err(J["de"][j], de)]
        errs += [err(J["dtau"][l, j], dtau[l]) for l in range(L)]
        errs += [err(J["dscat"][c, l, j], dam[c][l]) for c in range(len(nums)) for l in range(L)]
        worst = max(worst, max(errs) / scale[j])
        errs_T = [err(J["dTs"][j], dEs * mp.mpf(float(dEs_dT[j])))]
        for l in range(L):
            dBb, dBt = np.pi * ref.planck_dT(nu[j], edges[l][0]), np.pi * ref.planck_dT(nu[j], edges[l][1])
            if linear:
                errs_T += [err(J["dT"][2 * l, j], dB[l][0] * mp.mpf(float(dBb))), err(J["dT"][2 * l + 1, j], dB[l][1] * mp.mpf(float(dBt)))]
            else:
                errs_T.append(err(J["dT"][l, j], dB[l][0] * mp.mpf(float(dBb))))
        worst_T = max(worst_T, max(errs_T) / unit_T[j])
    return worst, worst_T


def check(mp, what, case, linear, delta, e, Is, Ts, It, n):
    nu = np.linspace(LO, HI, n)
    worst, worst_T = against_mp(mp, case["k"], case["depth"], case["edges"], nu, linear, case["amount"], case["numbers"], delta,
                                e, Is, Ts, It, range(n))
    print("%s: the restatement within %.2e of the scale and %.2e of pi dB/dT of 50 digits" % (what, worst, worst_T))
    assert worst <= BOUND and worst_T <= BOUND


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_mpmath_on_the_seven_cases(mp, name):
    """24 points of each of K5m's seven kinds of case: both sources, 0, 1 and 4 scatterers, scaled and not, e = 1, 0, 0.3 and
    spectral, with and without I_top"""
    make, delta = CASES[name][:2]
    n = 24
    e, Is, Ts, It = boundaries(name, n)
    check(mp, name, hand_made(n=n, **make), make["linear"], delta, e, Is, Ts, It, n)


def special(n, L, t, numbers_of, k_depth, seed, linear):
    """L layers of extinction depth about t by one scatterer of amount t whose numbers numbers_of(rs) gives, over a gas of
    optical depth k_depth(rs, n)"""
    rs = np.random.RandomState(seed)
    depth = np.full(L, 1e4)
    k = np.array([k_depth(rs, n) for _ in range(L)]) / 1e4
    lev = rs.uniform(200, 300, L + 1)
    edges = np.column_stack([lev[:-1], lev[1:]]) if linear else np.column_stack([lev[:-1], lev[:-1]])
    amount = np.array([t * rs.uniform(0.5, 2.0, L)])
    return dict(k=k, depth=depth, edges=edges, amount=amount, numbers=[numbers_of(rs)])


@pytest.mark.parametrize("linear", (False, True))
def test_restatement_in_conservative_layers(mp, linear):
    """albedo 1 - 1e-12 over a gas of optical depth 1e-14, and albedo exactly 1 over no gas at all (the den == 0 branch,
    P = Q = 0): every derivative finite, the gas's exactly 0 in the second"""
    n = 24
    near = special(n, 3, 2.0, lambda rs: (1.0, 1.0 - 1e-12, 0.6), lambda rs, n: np.full(n, 1e-14), 61, linear)
    check(mp, "nearly conservative", near, linear, 1, 0.3, None, 290.0, None, n)
    exact = special(n, 3, 2.0, lambda rs: (1.0, 1.0, 0.6), lambda rs, n: np.zeros(n), 62, linear)
    check(mp, "conservative", exact, linear, 1, 0.3, None, 290.0, None, n)
    J = ref.jacobian(exact["k"], exact["depth"], np.linspace(LO, HI, n), exact["edges"], linear, exact["amount"],
                     exact["numbers"], 1, 0.3, None, 290.0, None)
    assert not J["dtau"].any() and not J["dT"].any()


@pytest.mark.parametrize("linear", (False, True))
def test_restatement_in_very_thin_and_very_thick_layers(mp, linear):
    """t = 1e-12 and t = 1e4: finite everywhere, and below the opaque layers exactly 0 or negligible"""
    n = 24
    thin = special(n, 3, 1e-12, lambda rs: (1.0, 0.7, 0.5), lambda rs, n: 10.0 ** rs.uniform(-14, -12, n), 63, linear)
    check(mp, "thin", thin, linear, 1, 0.3, None, 290.0, None, n)
    thick = special(n, 3, 1e4, lambda rs: (1.0, 0.7, 0.5), lambda rs, n: 10.0 ** rs.uniform(2, 4, n), 64, linear)
    check(mp, "thick", thick, linear, 1, 0.3, None, 290.0, None, n)
    nu = np.linspace(LO, HI, n)
    J = ref.jacobian(thick["k"], thick["depth"], nu, thick["edges"], linear, thick["amount"], thick["numbers"], 1, 0.3, None,
                     290.0, None)
    scale = flux.scale(nu, thick["edges"], None, 290.0, None)
    assert np.all(np.abs(J["dtau"][:2]) <= 1e-300 * scale) and np.all(np.abs(J["dscat"][:, :2]) <= 1e-300 * scale)
    assert np.all(np.abs(J["dTs"]) <= 1e-300) and np.all(np.abs(J["de"]) <= 1e-300 * scale)


@pytest.mark.parametrize("linear", (False, True))
def test_restatement_where_q_is_small(mp, linear):
    """an unscaled scatterer with g = 1 - 1e-9 and albedo 1 - 1e-9: q = D (t - tsg) is 1e-9 of t"""
    n = 24
    case = special(n, 3, 3.0, lambda rs: (1.0, 1.0 - 1e-9, 1.0 - 1e-9), lambda rs, n: 10.0 ** rs.uniform(-10, -8, n), 65, linear)
    check(mp, "q small", case, linear, 0, 0.3, None, 290.0, flux.planck(np.linspace(LO, HI, n), 180.0), n)


def test_planck_dT_against_mpmath(mp):
    f = mp.mpf
    for nu, T in ((600.0, 200.0), (650.0, 250.0), (700.0, 300.0), (10.0, 300.0), (3000.0, 180.0)):
        B = lambda t: 2E8 * f(flux.H) * f(flux.C) ** 2 * f(nu) ** 3 / mp.expm1(100 * f(flux.H) * f(flux.C) * f(nu) / f(flux.KB) / t)
        want = mp.diff(B, f(T))
        assert abs(f(float(ref.planck_dT(nu, T))) - want) <= 1e-14 * abs(want)


def test_adjoint_against_central_differences_of_the_forward_restatement():
    """the whole Jacobian against central differences of scatter_flux_ref.column in float64, to the differences' noise"""
    name = "four scatterers, linear source, unscaled, edges apart"
    make, delta = CASES[name][:2]
    n = 16
    case = hand_made(n=n, **make)
    e, Is, Ts, It = boundaries(name, n)
    nu = np.linspace(LO, HI, n)
    J = ref.jacobian(case["k"], case["depth"], nu, case["edges"], True, case["amount"], case["numbers"], delta, e, Is, Ts, It)
    scale = flux.scale(nu, case["edges"], Is, Ts, It)
    top = lambda **kw: flux.column(kw.get("k", case["k"]), case["depth"], nu, kw.get("edges", case["edges"]),
                                   kw.get("amount", case["amount"]), case["numbers"], delta, e, Is, Ts, It)[0][-1]
    h = 1e-6
    for l in range(4):
        k2, k1 = case["k"].copy(), case["k"].copy()
        k2[l] *= 1 + h
        k1[l] *= 1 - h
        assert np.all(np.abs((top(k=k2) - top(k=k1)) / (2 * h) - J["dtau"][l]) <= 1e-8 * scale)
        for c in range(4):
            a2, a1 = case["amount"].copy(), case["amount"].copy()
            a2[c, l] *= 1 + h
            a1[c, l] *= 1 - h
            assert np.all(np.abs((top(amount=a2) - top(amount=a1)) / (2 * h) - J["dscat"][c, l]) <= 1e-8 * scale)
        for i in range(2):
            e2, e1 = case["edges"].copy(), case["edges"].copy()
            e2[l, i] += 1e-3
            e1[l, i] -= 1e-3
            unit = np.pi * ref.planck_dT(nu, 300.0)
            assert np.all(np.abs((top(edges=e2) - top(edges=e1)) / 2e-3 - J["dT"][2 * l + i]) <= 1e-7 * unit)


# ---- declarations, bindings, resources -----------------------------------------------------------------------------------
def test_entry_points_declared_exported_bound_and_abi_unchanged():
    text = open(HEADER).read()
    m = re.search(r"int lbl_column_jacobian_scatter_dev\((.*?)\);", text, re.S)
    assert m, "lbl_column_jacobian_scatter_dev is not declared in include/pyrad_hip.h"
    declared = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [re.split(r"[\s\*]+", a.strip())[-1] for a in declared.split(",")]
    assert names == ARGUMENTS
    assert re.search(r"int lbl_column_jacobian_scatter_workspace\(int n_layers, int64_t points, int64_t\* doubles\);", text)
    assert re.search(r"#define LBL_ABI_VERSION 5\b", text)
    assert len(_native.SIGNATURES["lbl_column_jacobian_scatter_dev"][1]) == len(ARGUMENTS)
    lib = _native.load()
    assert lib.lbl_abi_version() == 5
    out = C.c_int64()
    assert lib.lbl_column_jacobian_scatter_workspace(4, 1, C.byref(out)) == 0 and out.value == 5 * 5 * 256
    assert lib.lbl_column_jacobian_scatter_workspace(4, 257, C.byref(out)) == 0 and out.value == 5 * 5 * 512
    assert lib.lbl_column_jacobian_scatter_workspace(129, 1, C.byref(out)) == BAD_ARG
    assert lib.lbl_column_jacobian_scatter_workspace(4, 1, None) == BAD_ARG
    entry = lib.lbl_column_jacobian_scatter_dev
    saved = entry.argtypes
    entry.argtypes = None           # (a NULL context is refused before any other argument is read)
    try:
        assert entry(None, *([0] * (len(ARGUMENTS) - 1))) == BAD_ARG
    finally:
        entry.argtypes = saved


def test_scatter_jacobian_kernels_in_the_resource_report():
    """both instantiations of both kernels are in the build's resource report, without scratch and without spilled VGPRs"""
    report = open(os.path.join(os.path.dirname(_native.LIB_PATH), "lbl_kernels.remarks")).read()
    for kernel in ("scatter_jacobian_down_kernel", "scatter_jacobian_up_kernel"):
        blocks = re.findall(r"Function Name: (_ZN3lbl\d+%sILb[01]E\w*)(.*?)(?=Function Name:|\Z)" % kernel, report, re.S)
        assert len({b[0] for b in blocks}) == 2, kernel
        for _, body in blocks:
            assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", body) and re.search(r"VGPRs Spill: 0\b", body)


# ---- the model's validation ----------------------------------------------------------------------------------------------
@pytest.fixture()
def no_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the device was touched before validation finished")
    monkeypatch.setattr(model, "_ctx", refuse)


def test_validation_before_any_device_work(no_context):
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("validation")
    atm.addLayer(1e4, 280.0, 900.0, LO, HI)
    atm.addLayer(1e4, 250.0, 500.0, LO, HI)
    cloud = model.Scatterer([0.0, 1.0], 1.0, 0.9, 0.8)
    for kw in (dict(), dict(surfaceTemperature=290.0, temperature="all"), dict(surfaceTemperature=290.0, planck="cubic"),
               dict(surfaceTemperature=290.0, levelTemperatures=[300, 270, 240]),
               dict(surfaceTemperature=290.0, emissivity=1.5), dict(surfaceTemperature=290.0, deltaScaling=1),
               dict(surfaceTemperature=290.0, scatterers=[model.Scatterer([1.0], 1.0, 0.9, 0.8)]),
               dict(surfaceTemperature=290.0, scatterers=[cloud] * 5), dict(surfaceTemperature=290.0, topSpectrum=[1.0, 2.0]),
               dict(surfaceTemperature=290.0, bands=[(650.0, 600.0)])):
        with pytest.raises(ValueError):
            atm.jacobiansTwoStream(**kw)
    assert model.Jacobians(1.0, 2.0, None, np.zeros(2), None, [], [1.0], [1.0]).scatterers is None
