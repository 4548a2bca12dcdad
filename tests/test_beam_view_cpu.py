"""Scattered sunlight along a view (lbl_column_beam_radiance_dev, Atmosphere.solarRadianceTwoStream) without a device: the
restatement of tests/beam_view_ref.py against mpmath at 50 digits - the column's fluxes solved there, the in-layer ODE with
the beam source solved by its modes and the layer integral by mpmath.quad of the defined source function, no closed form - on
hand-made columns away from the particular solution's pole, on a grid of suns through the pole, at mu == m and beside it for
a down view, in conservative layers and in very thin and very thick ones; the three identities and the thin-layer limit; the
declarations and the binding; the model's validation.

Measured (this file prints every figure), in units of S0 / pi of the point: away from the pole (|1 - lam m| >= 0.05, which
the tests assert of their inputs) the restatement stays within 3.9e-17 of the 50-digit values on the hand-made cases
(the radiances themselves are a few hundredths of S0 / pi), 1.3e-18 through mu == m, 9.5e-17 in the conservative layers and
3.2e-17 in the thin and thick ones; the bound asserted there is
K5n's 1e-13, what the GPU tests' 1e-12 rests on.  Through the pole (lam m = 1 exactly and 1e-9, 1e-6, 1e-3, 1e-2 to either
side) Cp and u reach 1e6 and cancel against the homogeneous part: measured worst POLE_MEASURED = 7.41e-13 (at -1e-6, the
nearest point where m is kept; 1.2e-13 .. 5.0e-13 where it is moved; 3.0e-16 at 1e-3), and the bound asserted is
POLE_BOUND = 4 POLE_MEASURED, the factor for the libm differences of another machine; the GPU tests take ten times that, the
ratio of K5n's two bounds.  To keep this file near a minute, each point of a case checks one of the five views in turn
against mpmath where a test says so."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import beam_view_ref as ref
import twostream_ref as two
from pyrad_amd import _native, model, settings

HEADER = os.path.join(os.path.dirname(_native.CSRC), "..", "include", "pyrad_hip.h")
ARGUMENTS = ("ctx n_layers abs_coef depth range_min range_max n S0 beam_weight slant n_scat scat_amount scat_ext scat_ext_all "
             "scat_ssa scat_ssa_all scat_asym scat_asym_all delta_scaling emissivity emissivity_all n_views view_mu view_down "
             "workspace radiance up_top down_surface direct_surface").split()
SIGNATURE = _native.SIGNATURES["lbl_column_beam_radiance_dev"]     # (a KeyError without the feature: this file is about it)
MU3 = 1.0 / np.sqrt(3.0)
VIEWS = [(1.0, 0), (0.5, 0), (MU3, 0), (0.2, 1), (1.0, 1)]
BOUND = 1e-13
AWAY = 0.05                     # |1 - lam m| of every layer of the cases that BOUND is asserted on
POLE_MEASURED = 7.41e-13        # the restatement's worst error through the pole, of S0 / pi (test_restatement_through_the_pole)
POLE_BOUND = 4 * POLE_MEASURED
POLE_OFFSETS = (0.0, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3, 1e-2, -1e-2)


def hand_made(seed, L=4, n=1029, scatterers=0, spectral=(), mu0=0.4, slant=None):
    """k log-uniform with optical depths 1e-6 .. 1e2 over 1e4 cm; scatterer c has spectral numbers where c is in
    ``spectral``; one sun of cosine mu0 <= 0.45 with slants up to a tenth shorter (or ``slant``), so that lam m <= 0.87"""
    rs = np.random.RandomState(seed)
    k = 10.0 ** rs.uniform(-10, -2, (L, n))
    depth = np.full(L, 1e4)
    S0 = rs.uniform(0.5, 1.5, n)
    sl = (1.0 / mu0) * rs.uniform(0.9, 1.0, L)
    bw = float(rs.uniform(0.05, 0.3))
    amount = 10.0 ** rs.uniform(-3, 1, (scatterers, L))
    numbers = []
    for c in range(scatterers):
        if c in spectral:
            numbers.append((rs.uniform(0.2, 2.0, n), rs.uniform(0.3, 1.0, n), rs.uniform(-0.3, 0.9, n)))
        else:
            numbers.append((float(rs.uniform(0.2, 2.0)), float(rs.uniform(0.5, 1.0)), float(rs.uniform(-0.3, 0.9))))
    return dict(k=k, depth=depth, S0=S0, beam_weight=bw, slant=sl if slant is None else np.asarray(slant, dtype=np.float64),
                amount=amount, numbers=numbers)


def spectral_emissivity(n):
    return 0.55 + 0.4 * np.sin(0.37 * np.arange(n)) ** 2


# name: (hand_made's arguments, delta scaling, emissivity)
CASES = {
    "gas alone, black surface": (dict(seed=71), 1, 1.0),
    "gas alone, bright surface": (dict(seed=72, mu0=0.3), 1, 0.3),
    "one scatterer, unscaled, mirror-bright surface": (dict(seed=73, scatterers=1), 0, 0.0),
    "one spectral scatterer": (dict(seed=74, scatterers=1, spectral=(0,), mu0=0.45), 1, "spectrum"),
    "four scatterers": (dict(seed=75, scatterers=4, spectral=(0, 2), mu0=0.25), 1, 0.3),
    "four scatterers, unscaled": (dict(seed=76, scatterers=4, spectral=(1, 3)), 0, "spectrum"),
    "four constant scatterers, black surface": (dict(seed=77, scatterers=4, mu0=0.15), 1, 1.0),
}


def case_of(name, n):
    make, delta, e = CASES[name]
    case = hand_made(n=n, **make)
    return case, delta, spectral_emissivity(n) if isinstance(e, str) else e


def away_from_the_pole(case, delta):
    """the smallest |1 - lam m| of the case over its layers and points"""
    return float(ref.moved(case["k"], case["depth"], case["slant"], case["amount"], case["numbers"], delta)[1].min())


# ---- 50 digits -----------------------------------------------------------------------------------------------------------
def mp_point(mp, k, depth, S0, bw, slant, amount, numbers, delta, e, views, moved):
    """One grid point at 50 digits: k (L,), numbers as scalars, moved (L,) the float64 decisions at the pole.  Returns the
    radiances of ``views`` and (up, dn)."""
    f = mp.mpf
    L = len(k)
    ta, ts, tsg = [], [], []
    for l in range(L):
        a_, s_, g_ = f(float(k[l])) * f(float(depth[l])), f(0), f(0)
        for c, (ext, ssa, g) in enumerate(numbers):
            ext, ssa, g = f(float(ext)), f(float(ssa)), f(float(g))
            fd = g * g if delta else f(0)
            am = f(float(amount[c][l]))
            a_, s_, g_ = a_ + am * (ext * (1 - ssa)), s_ + am * ((ext * ssa) * (1 - fd)), g_ + am * ((ext * ssa) * (g - fd))
        ta.append(a_), ts.append(s_), tsg.append(g_)
    R, T, Rb, Tb = [], [], [], []
    S = [None] * L + [f(float(S0))]
    for l in range(L - 1, -1, -1):
        sl = f(float(slant[l]))
        if ta[l] + ts[l] == 0:
            r, t_, rb, tb, td = f(0), f(1), f(0), f(0), f(1)
        else:
            r, t_ = two.layer_scalar(ta[l], ts[l], tsg[l], sl, f, mp.sqrt, mp.exp, mp.expm1)[:2]
            _, t, _, _, _, Cp, Cm, Tdm = ref.layer_scalar(ta[l], ts[l], tsg[l], sl, bool(moved[l]), 0, 0, 0, f, mp.sqrt, mp.exp)
            rb, tb = Cp - r * Cm - t_ * Cp * Tdm, Cm * Tdm - t_ * Cm - r * Cp * Tdm
            td = mp.exp(-t * sl)
        R.insert(0, r), T.insert(0, t_), Rb.insert(0, rb), Tb.insert(0, tb)
        S[l] = td * S[l + 1]
    Fd = [f(float(bw)) * s for s in S]
    P, Q = [Rb[l] * Fd[l + 1] for l in range(L)], [Tb[l] * Fd[l + 1] for l in range(L)]
    # adding from the surface upwards, then down from the top (twostream_ref.column's relations)
    e = f(float(e))
    A, G = [1 - e], [(1 - e) * Fd[0]]
    for l in range(L):
        c = 1 - A[l] * R[l]
        A.append(R[l] + T[l] * T[l] * A[l] / c)
        G.append(P[l] + T[l] * (G[l] + A[l] * Q[l]) / c)
    dn, up = [None] * (L + 1), [None] * (L + 1)
    dn[L], up[L] = f(0), G[L]
    for l in range(L - 1, -1, -1):
        dn[l] = (T[l] * dn[l + 1] + Q[l] + R[l] * G[l]) / (1 - A[l] * R[l])
        up[l] = A[l] * dn[l] + G[l]
    out = []
    for mu, down in views:
        mu = f(float(mu))
        I = f(0) if down else up[0] / mp.pi
        for l in (range(L - 1, -1, -1) if down else range(L)):
            if ta[l] + ts[l] == 0:
                continue
            F, t, w, g, m, _, _, _ = ref.layer_scalar(ta[l], ts[l], tsg[l], float(slant[l]), bool(moved[l]), Fd[l + 1], up[l],
                                                      dn[l + 1], f, mp.sqrt, mp.exp)
            Sf = ref.source_scalar(F, w, g, m, mu, down, f, mp.sqrt)
            # y: the way from the edge where the light leaves (t = 1e300 has no digits left for t - y)
            reach = min(t, 125 * mu) if t > 250 * mu else t     # (beyond: below exp(-125) of the scale)
            panels = int(mp.ceil(reach * (1 / mu + 1 / m + 2) / 10)) + 1
            pts = [reach * i / panels for i in range(panels + 1)]
            if down:
                J = mp.quad(lambda y: Sf(t - y, y) * mp.exp(-y / mu), pts) / mu
            else:
                J = mp.quad(lambda y: Sf(y, t - y) * mp.exp(-y / mu), pts) / mu
            I = I * mp.exp(-t / mu) + J / mp.pi
        out.append(I)
    return out, up, dn


def against_mp(mp, case, delta, e, views, points, per_point=None):
    """the restatement at every point of the given column against 50 digits at ``points``: the worst error of a radiance
    in units of S0 / pi of the point.  ``per_point``: that many of the views at each point, taken in turn."""
    n = len(case["S0"])
    got = ref.radiance(case["k"], case["depth"], case["S0"], case["beam_weight"], case["slant"], views, case["amount"],
                       case["numbers"], delta, e)[0]
    moved = ref.moved(case["k"], case["depth"], case["slant"], case["amount"], case["numbers"], delta)[0]
    ev = np.broadcast_to(np.asarray(e, dtype=np.float64), (n,))
    worst = 0.0
    for j in points:
        nums = [tuple(float(np.broadcast_to(v, (n,))[j]) for v in triple) for triple in case["numbers"]]
        pick = range(len(views)) if per_point is None else [(j * per_point + i) % len(views) for i in range(per_point)]
        want, _, _ = mp_point(mp, case["k"][:, j], case["depth"], case["S0"][j], case["beam_weight"], case["slant"],
                              case["amount"], nums, delta, ev[j], [views[v] for v in pick], moved[:, j])
        for i, v in enumerate(pick):
            worst = max(worst, float(abs(mp.mpf(float(got[v, j])) - want[i]) / (case["S0"][j] / np.pi)))
    return worst


@pytest.fixture(scope="module")
def mp():
    m = pytest.importorskip("mpmath")
    m.mp.dps = 50
    return m


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_mpmath_on_the_hand_made_cases(mp, name):
    """L = 4 at 24 points, the five views in turn from point to point: within 1e-13 of S0 / pi (measured: at most 3.9e-17)"""
    n = 24
    case, delta, e = case_of(name, n)
    assert away_from_the_pole(case, delta) >= AWAY
    worst = against_mp(mp, case, delta, e, VIEWS, range(n), per_point=1)
    print("%s: the restatement within %.2e of S0 / pi of 50 digits" % (name, worst))
    assert worst <= BOUND


def pole_case(offset, n=6):
    """a column of three layers under an overhead-like sun whose m in layer 1 is (1 + offset) / lam of point 2: lam m runs
    through 1 there as the offsets do.  Returns the case and the point."""
    rs = np.random.RandomState(23)
    L, j = 3, 2
    depth = np.full(L, 1e4)
    k = 10.0 ** rs.uniform(-2, 1, (L, n)) / depth[:, None]
    amount = np.array([[0.5, 2.0, 0.1]])
    numbers = [(1.0, 0.6, 0.5)]
    lam = ref.layer_numbers(*two.optical(k, depth, amount, numbers, 1))[6]
    assert np.all((lam[1] > 1.0) & (lam[1] < ref.D))             # (so that m = 1 / lam is a sun's cosine)
    slant = np.array([1.3, lam[1, j] / (1.0 + offset), 1.25])
    return dict(k=k, depth=depth, S0=rs.uniform(0.5, 1.5, n), beam_weight=0.8, slant=slant, amount=amount, numbers=numbers), j


def test_restatement_through_the_pole(mp):
    """lam m = 1 exactly and 1e-9, 1e-6, 1e-3, 1e-2 to either side, all five views: Cp reaches 1e6 and cancels against the
    homogeneous part, so 1e-13 does not hold here; the bound is four times the worst error measured (7.41e-13 of S0 / pi)"""
    worst = 0.0
    for offset in POLE_OFFSETS:
        case, j = pole_case(offset)
        moved, pole = ref.moved(case["k"], case["depth"], case["slant"], case["amount"], case["numbers"], 1)
        assert abs(pole[1, j] - abs(offset)) <= 1e-15 + 1e-9 * abs(offset)
        assert moved[1, j] == (pole[1, j] < two.NUDGE)
        err = against_mp(mp, case, 1, 0.4, VIEWS, [j])
        print("lam m = 1 %+.0e (m %s): the restatement within %.2e of S0 / pi of 50 digits"
              % (offset, "moved" if moved[1, j] else "kept", err))
        worst = max(worst, err)
    print("through the pole: worst %.2e, bound %.2e" % (worst, POLE_BOUND))
    assert worst <= POLE_BOUND


def mu_equal_m_views(m):
    return [(m * (1 + d), 1) for d in (0.0, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3)]


def test_restatement_through_mu_equal_to_m(mp):
    """down views whose mu is the sun's m in a chosen layer, exactly and 1e-9, 1e-6, 1e-3 to either side: Xd is smooth,
    no point is left out (measured: at most 1.3e-18 of S0 / pi)"""
    n = 6
    case = hand_made(81, L=3, n=n, scatterers=2, spectral=(1,), slant=[2.5, 1.0 / 0.43, 2.2])
    assert away_from_the_pole(case, 1) >= AWAY
    worst = 0.0
    for layer in (0, 1):
        m = 1.0 / case["slant"][layer]
        views = mu_equal_m_views(m)
        assert 1.0 - views[0][0] * case["slant"][layer] == 0.0 or abs(1.0 - views[0][0] * case["slant"][layer]) < 3e-16
        worst = max(worst, against_mp(mp, case, 1, 0.3, views, [1, 4]))
    print("mu = m and beside it: the restatement within %.2e of S0 / pi of 50 digits" % worst)
    assert worst <= BOUND


def test_restatement_in_conservative_layers(mp):
    """ssa == 1 with gas optical depths 1e-6 and 0 (the den == 0 branch), cloud optical depths 1e-3 .. 30 (measured: at most
    9.5e-17 of S0 / pi)"""
    n, L = 6, 3
    worst = 0.0
    for t_gas in (1e-6, 0.0):
        case = dict(k=np.full((L, n), t_gas / 1e4), depth=np.full(L, 1e4), S0=np.linspace(0.6, 1.4, n), beam_weight=0.4,
                    slant=np.array([2.5, 2.4, 2.3]), amount=np.array([[1e-3, 30.0, 1.0]]), numbers=[(1.0, 1.0, 0.7)])
        for delta in (0, 1):
            assert away_from_the_pole(case, delta) >= AWAY
            worst = max(worst, against_mp(mp, case, delta, 0.7, VIEWS, [0, n - 1]))
    print("conservative layers: the restatement within %.2e of S0 / pi of 50 digits" % worst)
    assert worst <= BOUND


def test_restatement_in_very_thin_and_very_thick_layers(mp):
    """layers of t = 1e-12, 1e3 and 1e300 in every position among ordinary ones, and a column without layers (measured: at
    most 3.2e-17 of S0 / pi; without layers an up view is (1 - e) beam_weight S0 / pi and a down view 0, exactly)"""
    n = 4
    amount = np.array([[0.3, 1.0, 0.5]])
    worst = 0.0
    for t_odd in (1e-12, 1e3, 1e300):
        for where in range(3):
            k = np.full((3, n), 0.2 / 1e4)
            k[where] = t_odd / 1e4
            am = amount.copy()
            am[0, where] = t_odd * 2.0
            case = dict(k=k, depth=np.full(3, 1e4), S0=np.linspace(0.7, 1.3, n), beam_weight=0.35,
                        slant=np.array([2.6, 2.5, 2.45]), amount=am, numbers=[(1.0, 0.9, 0.6)])
            assert away_from_the_pole(case, 1) >= AWAY
            worst = max(worst, against_mp(mp, case, 1, 0.5, VIEWS, [1]))
    print("t = 1e-12, 1e3, 1e300: the restatement within %.2e of S0 / pi of 50 digits" % worst)
    assert worst <= BOUND
    S0 = np.linspace(0.7, 1.3, n)
    got = ref.radiance(np.zeros((0, n)), [], S0, 0.35, [], VIEWS, emissivity=0.25)[0]
    for v, (mu, down) in enumerate(VIEWS):
        assert np.array_equal(got[v], np.zeros(n) if down else ((1 - 0.25) * (0.35 * S0)) / np.pi)


# ---- the identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_at_the_two_stream_angle_the_radiance_is_the_flux(name):
    """mu = 1 / sqrt(3): pi Iu_L == up_L and pi Id_0 == dn_0 (diffuse), K5l's own spectra, to 1e-13 of S0"""
    n = 300
    case, delta, e = case_of(name, n)
    assert away_from_the_pole(case, delta) >= AWAY
    got, up, dn, _, _ = ref.radiance(case["k"], case["depth"], case["S0"], case["beam_weight"], case["slant"],
                                     [(MU3, 0), (MU3, 1)], case["amount"], case["numbers"], delta, e)
    err = max(np.max(np.abs(np.pi * got[0] - up[-1]) / case["S0"]), np.max(np.abs(np.pi * got[1] - dn[0]) / case["S0"]))
    print("%s: pi I at 1 / sqrt(3) within %.2e of S0 of the fluxes" % (name, err))
    assert err <= BOUND


def test_without_scatterers_it_is_the_attenuated_surface():
    """w = 0, every J exactly 0: an up view is up_0 / pi attenuated along the view - lbl_column_solar_dev's Lambertian
    up_top / pi with the single angle (mu, pi) - and a down view is exactly 0"""
    n = 300
    case = hand_made(62, n=n)
    e = spectral_emissivity(n)
    got, up, dn, direct, _ = ref.radiance(case["k"], case["depth"], case["S0"], case["beam_weight"], case["slant"], VIEWS,
                                          emissivity=e)
    worst = 0.0
    for v, (mu, down) in enumerate(VIEWS):
        if down:
            assert np.all(got[v] == 0.0)
            continue
        I = ((1 - e) * direct[0]) / np.pi
        for l in range(len(case["depth"])):
            I = I * np.exp(-(case["k"][l] * case["depth"][l]) / mu)
        worst = max(worst, np.max(np.abs(got[v] - I) / (case["S0"] / np.pi)))
    print("no scatterers: an up view within %.2e of S0 / pi of the attenuated surface" % worst)
    assert worst <= BOUND


def halved(case):
    """every layer split into two of half the amounts and depth"""
    twice = lambda a: np.repeat(np.asarray(a, dtype=np.float64), 2, axis=-1)
    return dict(case, k=np.repeat(case["k"], 2, axis=0), depth=twice(case["depth"]) / 2, slant=twice(case["slant"]),
                amount=twice(case["amount"]) / 2 if len(case["amount"]) else case["amount"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_layer_and_its_two_halves(name):
    n = 300
    case, delta, e = case_of(name, n)
    args = lambda c: (c["k"], c["depth"], c["S0"], c["beam_weight"], c["slant"], VIEWS, c["amount"], c["numbers"], delta, e)
    whole, halves = ref.radiance(*args(case))[0], ref.radiance(*args(halved(case)))[0]
    err = np.max(np.abs(whole - halves) / (case["S0"] / np.pi))
    print("%s: a layer and its two halves within %.2e of S0 / pi" % (name, err))
    assert err <= BOUND


def test_thin_layer_limit():
    """one layer of t = 1e-8 over a black surface: (t / mu) S+-(0), where F+ and F- are O(t) and the beam's single
    scattering is all of S: (t / mu) (w / (2 sqrt(3) m)) (1 -+ 3 g mu m) beam_weight S0 / pi, to first order in t"""
    n = 5
    S0 = np.linspace(0.5, 1.5, n)
    ext, ssa, g, bw, slant, t = 1.0, 0.8, 0.6, 0.7, 1.6, 1e-8
    got = ref.radiance(np.zeros((1, n)), [1e4], S0, bw, [slant], VIEWS, [[t]], [(ext, ssa, g)], 0, 1.0)[0]
    m = 1.0 / slant
    for v, (mu, down) in enumerate(VIEWS):
        want = (t / mu) * (ssa / (2 * ref.D * m)) * (1 - (-1 if down else 1) * 3 * g * mu * m) * bw * S0 / np.pi
        assert np.max(np.abs(got[v] / want - 1)) <= 1e-6, (mu, down)


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_bound_and_abi_unchanged():
    with open(HEADER) as fh:
        text = fh.read()
    lib = _native.load()
    m = re.search(r"int\s+lbl_column_beam_radiance_dev\s*\(([^;]*)\)\s*;", text)
    assert m, "lbl_column_beam_radiance_dev is not declared"
    params = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert params == ARGUMENTS
    assert re.search(r"int\s+lbl_column_beam_radiance_workspace\s*\(", text)
    assert hasattr(lib, "lbl_column_beam_radiance_dev") and hasattr(lib, "lbl_column_beam_radiance_workspace")
    assert len(SIGNATURE[1]) == len(ARGUMENTS)
    assert len(_native.SIGNATURES["lbl_column_beam_radiance_workspace"][1]) == 3
    assert hasattr(_native.Context, "column_beam_radiance_dev")
    assert hasattr(_native.Context, "column_beam_radiance_workspace")
    assert hasattr(model.Atmosphere, "solarRadianceTwoStream")
    assert lib.lbl_abi_version() == 5
    assert _native.limit("beam_views") == 16


def test_the_workspace_is_the_two_stream_call_s():
    """five numbers per level and point, whole tiles of 256 points, one at least"""
    lib = _native.load()
    out, other = C.c_int64(), C.c_int64()
    for L, points in ((0, 0), (0, 1), (4, 256), (4, 257), (128, 1000)):
        assert lib.lbl_column_beam_radiance_workspace(L, points, C.byref(out)) == 0
        assert lib.lbl_column_twostream_workspace(L, points, C.byref(other)) == 0 and out.value == other.value
    assert out.value == 5 * 129 * 1024
    for L, points in ((-1, 1), (129, 1), (3, -1)):
        assert lib.lbl_column_beam_radiance_workspace(L, points, C.byref(out)) == -1
    assert lib.lbl_column_beam_radiance_workspace(3, 1, None) == -1


def test_beam_view_kernels_in_the_resource_report():
    from test_kernel_resources_cpu import _kernels, _remarks
    if "PYRAD_HIP_LIB" in os.environ:
        pytest.skip("an experiment build is selected (PYRAD_HIP_LIB)")
    k = _kernels(_remarks("lbl_kernels"))
    mine = {n: f for n, f in k.items() if "beam_view_kernel" in n}
    for n, f in sorted(mine.items()):
        print(n, f["VGPRs"], f["Occupancy [waves/SIMD]"])
        # (the views' cosines and directions are workgroup-uniform; those that do not fit the scalar file are kept in lanes of
        # a vector register, which touches no memory)
        assert f.get("ScratchSize [bytes/lane]") == 0 and f.get("VGPRs Spill") == 0, (n, f)
    # 1, 2, 4, 8 and 16 views
    assert len(mine) == 5, sorted(mine)
    for nv in (1, 2, 4, 8, 16):
        assert any("beam_view_kernelILi%dEE" % nv in n or "beam_view_kernel<%d>" % nv in n for n in mine), (nv, sorted(mine))


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
    atm = model.Atmosphere("beam view")
    for depth, T, P in LAYERS:
        atm.addLayer(depth, T, P, 600, 610)
    n = len(atm[0].xAxis)
    nan = float("nan")
    S = model.Scatterer
    four = [1.0, 0.0, 2.0, 0.5]
    call = lambda views=(1.0,), **kw: atm.solarRadianceTwoStream(views, **{"solarTemperature": 5772.0, **kw})
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
    for bad in ([(0.5, 1.0)], [(0.5, 0.5), (0.3, 0.5)], [0.5], (0.5,), 0, 0.0, 1.5, nan, -0.2, "noon", None, True):
        with pytest.raises(ValueError, match="mu0"):
            call(mu0=bad)
    for e in (-0.1, 1.1, nan, "black", None, np.full(n, 1.5), np.ones(n - 1)):
        with pytest.raises(ValueError, match="emissivity"):
            call(emissivity=e)
    with pytest.raises(ValueError, match="instrument"):
        call(instrument="a radiometer")
    with pytest.raises(ValueError, match="exactly one of solarSpectrum and solarTemperature"):
        atm.solarRadianceTwoStream([1.0])
    with pytest.raises(ValueError, match="exactly one of solarSpectrum and solarTemperature"):
        call(solarSpectrum=1.0)
    with pytest.raises(ValueError, match="solarSpectrum"):
        atm.solarRadianceTwoStream([1.0], solarSpectrum=np.ones(n - 1))
    with pytest.raises(ValueError, match="geometry"):
        call(geometry="round")
    with pytest.raises(ValueError, match="planetRadius"):
        call(geometry="spherical", planetRadius=0.0)
    for kw in (dict(bands=[(600.0, 605.0)]), dict(angles=3), dict(surfaceTemperature=288.0)):
        with pytest.raises(TypeError):
            call(**kw)
    with pytest.raises(ValueError, match="no layers"):
        model.Atmosphere("empty").solarRadianceTwoStream([1.0], solarTemperature=5772.0)
