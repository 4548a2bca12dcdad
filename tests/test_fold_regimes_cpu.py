"""CPU: the arithmetic regimes of the column fold I <- t I + (1 - t) B(nu, T_layer), defined once for this file and for
tests/test_gpu_fold_arithmetic.py.

In the default arithmetic the fold exists in two forms, chosen per wave of 64 threads (four grid points per thread) by
fold_fast_path (K5c / K5d / K5e) and its hand-written twin in column_step_kernel<4, true, *> (K5b): the ONE-EXP form (one
exp per thread and layer, a degree-4 polynomial for the thread's other points, the update as one fma) where EVERY lane of
the wave is "plain", the GENERAL form (planck_budget's selects and IEEE division, the update as product and sum) otherwise.
This file restates that predicate in NumPy (wave_classes), fixes the grids ("regimes") on which the GPU tests exercise each
form and each switch-over, states the error bound the GPU tests hold the kernels to, and checks here, without a device,
that the regimes contain the wave classes they are meant to and that the reference's own fp64 expression stays inside
the bound.

The error bound.  u = 2^-53, b = nu pbkT, E = exp(b), B = pa nu^3 / (E - 1).

    S_B(b) = u ((B_ROUNDINGS b + 2) E / (E - 1) + 4)          relative error of B

  * b carries B_ROUNDINGS = 5 roundings of at most u each, which the exponential multiplies by b: the reference's
    100 h c n / k / T is five operations, the kernel's n * (100 h c / k / T) is four on the host and one on the device.
    (Counting one rounding here is too tight for the reference itself: measured against long double, its fp64 expression
    reaches 1.3 - 1.5 x that shape at b = 3 .. 5 and 2.4 x at b = 690, and 0.47 - 0.53 x the shape with the derived five;
    test_reference_planck_is_inside_its_bound prints both figures per regime.)
  * exp and the one-exp form's polynomial factor cost one rounding of E each (the 2), and E / (E - 1) is the cancellation
    in E - 1: near b = 1e-6 the one-exp form may lose u E / (E - 1) ~ 1e-10 relative, as much as the reference's
    exp(b) - 1 does.
  * the reciprocal and the three roundings of pa nu^3 are the 4.

Propagated through a column (column_bound): layer l adds (1 - t_l) B_l S_B(b_l) + 2.5 u |I_l - B_l| + 4 u I_(l+1) - the error
of B, half an ulp of t = exp(-tau) carried by (I - B) (the constant of test_gpu_abi.py's faint-radiance test), the update's
own roundings - and what the layers below contributed arrives multiplied by t_l, the update being a convex combination."""
import functools

import numpy as np
import pytest

from oracle import pyrad_oracle as orc

U = 2.0 ** -53
B_ROUNDINGS = 5
PB_K = 100 * orc.h * orc.c / orc.k            # 100 h c / k; the host's bracket is this / T, in this order
TINY = 1e-290                                 # below: compared absolutely (the reference's own products go subnormal)
LAYER_COUNTS = (1, 2, 5, 7, 13)
SURFACE_T = {"hot_exponent": 62.0, "beyond_700": 62.0, "across_700": 62.0}        # (every other regime: 288 K)

_EARTH = (288.0, 270.0, 240.0, 220.0)
_COLD = (60.0, 50.0, 41.0, 40.0)


def pbkT(T):
    return PB_K / np.asarray(T, dtype=np.float64)


def _step_threshold_n(lo, hi, T, ratio):
    """the n at which 3 step pbkT_max = ratio * 1e-3 (rounded to an integer: `ratio` is 'about')"""
    return int(round(1 + 3 * (hi - lo) * float(np.max(pbkT(T))) / (ratio * 1e-3)))


# name -> (lo, hi, n, layer temperatures)
REGIMES = {
    "fine": (600.0, 700.0, 8001, _EARTH),
    "coarse": (600.0, 700.0, _step_threshold_n(600.0, 700.0, _EARTH, 1.10) + 2, _EARTH),     # (+ 2: a three-point tail)
    "coarse_edge_below": (600.0, 700.0, _step_threshold_n(600.0, 700.0, _EARTH, 0.90), _EARTH),
    "coarse_edge_above": (600.0, 700.0, _step_threshold_n(600.0, 700.0, _EARTH, 1.10), _EARTH),
    # nu pbkT_max = 690 at 19,183 cm^-1
    "hot_exponent": (19160.0, 19200.0, 8001, _COLD),
    # b = 707.5 .. 710.04 for the coldest layer at a step the third condition accepts (3 step pbkT_max = 9.4e-4): all general
    # because of the 690 alone.  (n - 1) / 3 * 1e-3 = 2.7 is the widest span of b such a grid can have, so a grid cannot reach
    # from below 700 to above 709 AND be fine enough: across_700 is the one that starts below 700, at a coarse step.
    "beyond_700": (19670.0, 19740.0, 8001, _COLD),
    "across_700": (19440.0, 19740.0, 8001, _COLD),
    # nu pbkT_min = 1e-6 at nu = 2.0e-4, which is point 20 of 0 .. 0.04 in 4,001 points: the FIRST wave (points 0 .. 255) is
    # the mixed one and there is no all-general wave; near_zero_fine puts the threshold into the third wave
    "near_zero": (0.0, 0.04, 4001, _EARTH),
    "near_zero_fine": (0.0, 0.0012, 4001, _EARTH),
}

# the wave classes each regime must contain: (plain, mixed, general) as "0" (none), "+" (at least one), "1" (exactly one)
EXPECTED_CLASSES = {
    "fine": "+00", "coarse": "00+", "coarse_edge_below": "+00", "coarse_edge_above": "00+", "hot_exponent": "+1+",
    "near_zero": "+10", "near_zero_fine": "+1+", "across_700": "00+", "beyond_700": "00+",
}


def axis(lo, hi, n):
    """The grid of every kernel (linspace_at: j * step + lo, the last point hi), which is np.linspace's arithmetic and so
    engine.x_axis's and the oracle's x_axis."""
    return np.linspace(lo, hi, int(n), endpoint=True)


def wave_classes(lo, hi, n, first, count, layer_T):
    """The kernels' predicate per aligned group of 4 grid points of the window [first, first + count) (count 0: to the end
    of the grid), then per wave = 64 consecutive groups counted from the window's first aligned point.  Returns a dict:
    plain / mixed / general (numbers of waves), kind (per wave: 0 plain, 1 mixed, 2 general), start (per wave: its first
    grid point), end (one past its last), group_plain (per group).  (K5b sends a window whose `first` is no multiple of 4
    to its two- and one-point instantiations, which have no groups of 4: this describes the kernels that do.)"""
    nu = axis(lo, hi, n)
    count = n - first if count == 0 else count
    q0 = (first + 3) & ~3
    groups = max(first + count - q0, 0) // 4
    p = pbkT(layer_T)
    pmin, pmax = float(np.min(p)), float(np.max(p))
    g0, g3 = nu[q0:q0 + 4 * groups:4], nu[q0 + 3:q0 + 4 * groups:4]
    d = g3 - g0
    plain = (g0 * pmin >= 1e-6) & (g3 * pmax <= 690.0) & (d * pmax <= 1e-3) & (d >= 0.0)
    n_waves = (groups + 63) // 64
    kind = np.empty(n_waves, dtype=np.int64)
    for w in range(n_waves):
        pw = plain[64 * w:64 * (w + 1)]
        kind[w] = 0 if pw.all() else (1 if pw.any() else 2)
    start = q0 + 256 * np.arange(n_waves)
    return dict(plain=int(np.sum(kind == 0)), mixed=int(np.sum(kind == 1)), general=int(np.sum(kind == 2)), kind=kind,
                start=start, end=np.minimum(start + 256, q0 + 4 * groups), group_plain=plain)


def regime_classes(name, n_layers=None):
    lo, hi, n, T = REGIMES[name]
    return wave_classes(lo, hi, n, 0, 0, T if n_layers is None else layer_temperatures(name, n_layers))


# ---- the reference in long double and its bound -------------------------------------------------------------------------------
def planck_long(nu, T):
    """pyradPlanck.planckWavenumber's expression (oracle.pyrad_oracle.planckWavenumber), every operation in long double"""
    L = np.longdouble
    n = np.asarray(nu, dtype=np.float64).astype(L)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = L(2E8) * L(orc.h) * L(orc.c) ** 2 * n ** 3
        b = L(100) * L(orc.h) * L(orc.c) * n / L(orc.k) / L(float(T))
        return a / (np.exp(b) - 1)


def planck_shape(nu, T, b_roundings=B_ROUNDINGS):
    """S_B(b): the relative error allowed to B(nu, T) (module docstring); E / (E - 1) as 1 / (1 - exp(-b)), finite for any b"""
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.asarray(nu, dtype=np.float64) * float(pbkT(T))
        return U * ((b_roundings * b + 2.0) / -np.expm1(-b) + 4.0)


def fold_long(nu, layer_T, tau, I0=None, surface_T=0.0, trans=None):
    """The column fold in long double with its propagated bound.  tau[l]: the optical depths the kernel sees, k_l * depth_l
    formed here in long double from the fp64 factors (a 2-tuple (k, depth)) or given as an array; trans[l] (optional): the
    transmittances themselves, where the kernel reads them (column_sweep).  Returns (I, bound) as long double and float64."""
    L = np.longdouble
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        if I0 is not None:
            I, bound = np.asarray(I0, dtype=np.float64).astype(L), np.zeros(len(nu), dtype=L)
        else:
            I = planck_long(nu, surface_T)
            bound = I * planck_shape(nu, surface_T).astype(L)
        for l, T in enumerate(layer_T):
            if trans is not None:
                t = np.asarray(trans[l], dtype=np.float64).astype(L)
            else:
                x = tau[l]
                x = x[0].astype(L) * L(float(x[1])) if isinstance(x, tuple) else np.asarray(x).astype(L)
                t = np.exp(-x)
            B = planck_long(nu, T)
            I_out = t * I + (1 - t) * B
            bound = t * bound + ((1 - t) * B * planck_shape(nu, T).astype(L) + 2.5 * U * np.abs(I - B) + 4 * U * I_out)
            I = I_out
    return I, np.asarray(bound, dtype=np.float64)


def fold_fp64(nu, layer_T, tau, I0=None, surface_T=0.0):
    """The reference's own fold: planckWavenumber, np.exp and cls:784-787 in plain fp64"""
    with np.errstate(invalid="ignore", under="ignore"):
        I = np.asarray(I0, dtype=np.float64) if I0 is not None else orc.planckWavenumber(nu, surface_T)
        for l, T in enumerate(layer_T):
            k, depth = tau[l]
            I = orc.transmission(np.exp(-(k * depth)), I, orc.planckWavenumber(nu, T))
    return I


def compare(got, want, bound, factor):
    """|got - want| against factor * bound pointwise.  NaN where the reference is NaN (nu = 0); where the reference is below
    TINY, TINY is added to the allowance.  Returns (worst ratio over the points compared relatively, index of the worst,
    number of NaN points, number compared absolutely, ok, the ratio per point)."""
    got = np.asarray(got, dtype=np.float64)
    nan = np.isnan(np.asarray(want, dtype=np.float64))
    tiny = ~nan & (np.asarray(want, dtype=np.float64) < TINY)
    rel = ~nan & ~tiny
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        err = np.asarray(np.abs(got.astype(np.longdouble) - want), dtype=np.float64)
        ok = bool(np.all(np.isnan(got[nan])) and np.all(np.isfinite(got[~nan])) and np.all(err[rel] <= factor * bound[rel])
                  and np.all(err[tiny] <= TINY + factor * bound[tiny]))
        ratio = np.zeros(len(got))
        some = rel & (bound > 0)
        ratio[some] = err[some] / bound[some]
        ratio[rel & (bound == 0) & (err > 0)] = np.inf
    worst = int(np.argmax(ratio))
    return float(ratio[worst]), worst, int(nan.sum()), int(tiny.sum()), ok, ratio


# ---- the columns the GPU tests run --------------------------------------------------------------------------------------------
def layer_temperatures(name, n_layers):
    """n_layers temperatures from the regime's, coldest AND warmest among them from two layers on (so that pbkT_min and
    pbkT_max, and with them the wave classes, are the regime's); a single layer is the coldest"""
    T = REGIMES[name][3]
    order = (T[3], T[0], T[1], T[2])
    return tuple(order[l % 4] for l in range(n_layers))


def special_groups(n):
    """first point of the two adjacent aligned groups of 4: optical depth 0 exactly on the first, 900 (above the 800 at
    which exp_neg_budget clamps) on the second"""
    return ((n // 2) & ~3)


@functools.lru_cache(maxsize=None)
def column(name, n_layers, seed=20):
    """A column on regime `name`: per layer the temperature, a depth and host-made absorption coefficients k with optical
    depths k * depth log-uniform in 1e-12 .. 30 (0 and 900 on the two special groups).  Arrays are read-only."""
    lo, hi, n, _ = REGIMES[name]
    rng = np.random.default_rng([seed, n_layers, n])
    nu = axis(lo, hi, n)
    T = layer_temperatures(name, n_layers)
    depth = tuple(1000.0 * (1 + (3 * l) % 7) for l in range(n_layers))
    g = special_groups(n)
    ks = []
    for l in range(n_layers):
        tau = 10.0 ** rng.uniform(-12.0, np.log10(30.0), n)
        tau[g:g + 4] = 0.0
        tau[g + 4:g + 8] = 900.0
        k = tau / depth[l]
        k[g + 4:g + 8] = 900.0 * 1.0000001 / depth[l]
        k.setflags(write=False)
        ks.append(k)
    nu.setflags(write=False)
    return dict(name=name, lo=lo, hi=hi, n=n, nu=nu, T=T, depth=depth, k=tuple(ks),
                surface_T=SURFACE_T.get(name, 288.0))


@functools.lru_cache(maxsize=None)
def incoming(name, n_layers=1, seed=5):
    """An incoming radiance as in the faint-radiance test: B(nu, warmest layer) x 10^U(-20, 0)"""
    col = column(name, n_layers)
    rng = np.random.default_rng([seed, col["n"]])
    with np.errstate(invalid="ignore"):
        I = np.asarray(planck_long(col["nu"], max(REGIMES[name][3])), dtype=np.float64) * 10.0 ** rng.uniform(-20, 0, col["n"])
    I.setflags(write=False)
    return I


@functools.lru_cache(maxsize=None)
def reference(name, n_layers, source):
    """(I in long double, bound) of column(name, n_layers) from `source`: "surface" (B(nu, surface_T)) or "incoming"."""
    col = column(name, n_layers)
    tau = [(k, d) for k, d in zip(col["k"], col["depth"])]
    if source == "incoming":
        I, bound = fold_long(col["nu"], col["T"], tau, I0=incoming(name, n_layers))
    else:
        I, bound = fold_long(col["nu"], col["T"], tau, surface_T=col["surface_T"])
    I.setflags(write=False)
    bound.setflags(write=False)
    return I, bound


# ---- tests ----------------------------------------------------------------------------------------------------------------------
def _matches(count, spec):
    return {"0": count == 0, "+": count >= 1, "1": count == 1}[spec]


@pytest.mark.parametrize("name", sorted(REGIMES))
def test_regime_has_its_wave_classes(name):
    lo, hi, n, T = REGIMES[name]
    assert n <= 8200
    for n_layers in (None, 1, 2, 5, 7, 13):
        c = regime_classes(name, n_layers)
        print("%s (%s layers): %d points, waves plain / mixed / general = %d / %d / %d"
              % (name, n_layers or "regime", n, c["plain"], c["mixed"], c["general"]))
        want = EXPECTED_CLASSES[name]
        if n_layers == 1 and name.startswith("near_zero"):
            continue            # (one layer is the coldest: its threshold nu pbkT = 1e-6 lies lower, in another wave)
        assert all(_matches(c[k], s) for k, s in zip(("plain", "mixed", "general"), want)), (name, n_layers, want, c)
        assert c["plain"] + c["mixed"] + c["general"] == (n // 4 + 63) // 64


def test_step_threshold_counts():
    """3 step pbkT_max against 1e-3: the two edge regimes lie about 10 % to either side (not on adjacent counts, where this
    fp64 predicate and the kernel's might round differently), and a whole wave changes class between them"""
    p = float(np.max(pbkT(_EARTH)))
    for name, side in (("coarse_edge_below", -1), ("coarse_edge_above", +1), ("coarse", +1)):
        lo, hi, n, _ = REGIMES[name]
        x = 3 * (hi - lo) / (n - 1) * p / 1e-3
        print("%s: n = %d, 3 step pbkT_max = %.4f e-3" % (name, n, x))
        assert 0.07 <= side * (x - 1) <= 0.13
    assert REGIMES["coarse"][2] % 4 == 3 and REGIMES["fine"][2] % 4 == 1


def test_hot_and_cold_ends_cross_their_thresholds():
    lo, hi, n, T = REGIMES["hot_exponent"]
    b = axis(lo, hi, n) * float(np.max(pbkT(T)))
    assert b[0] < 690 < b[-1] and abs(b[n // 2] - 690) < 0.2 and 3 * (hi - lo) / (n - 1) * float(np.max(pbkT(T))) <= 1e-3
    lo, hi, n, T = REGIMES["beyond_700"]
    b = axis(lo, hi, n) * float(np.max(pbkT(T)))
    assert b[0] > 700 and b[-1] > 709.8 and np.sum(b > 709.8) >= 256 and 3 * (hi - lo) / (n - 1) * float(np.max(pbkT(T))) <= 1e-3
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(b[-1])) and orc.planckWavenumber(axis(lo, hi, n), min(T))[-1] == 0.0       # a / inf
    lo, hi, n, T = REGIMES["across_700"]
    b = axis(lo, hi, n) * float(np.max(pbkT(T)))
    assert b[0] < 700 and np.sum((b > 700) & (b < 709)) > 0 and b[-1] > 709.8
    for name in ("near_zero", "near_zero_fine"):
        lo, hi, n, T = REGIMES[name]
        b = axis(lo, hi, n) * float(np.min(pbkT(T)))
        assert b[0] == 0.0 and b[1] < 1e-6 < b[-1]


@pytest.mark.parametrize("name", sorted(REGIMES))
def test_reference_planck_is_inside_its_bound(name):
    """oracle.pyrad_oracle.planckWavenumber in fp64 against the same expression in long double, every point and every
    temperature of the regime (and its surface): r_ref = max |dB| / (B S_B) <= 1.  Also printed with ONE rounding of b
    instead of the derived five: that shape is too tight for the reference itself at large b."""
    lo, hi, n, T = REGIMES[name]
    nu = axis(lo, hi, n)
    r_ref = r_one = 0.0
    for t in tuple(T) + (SURFACE_T.get(name, 288.0),):
        want = planck_long(nu, t)
        got = orc.planckWavenumber(nu, t)
        ok = np.isfinite(np.asarray(want, dtype=np.float64)) & (np.asarray(want, dtype=np.float64) >= TINY)
        with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
            rel = np.asarray(np.abs(got.astype(np.longdouble) - want) / want, dtype=np.float64)[ok]
        if rel.size:
            r_ref = max(r_ref, float(np.max(rel / planck_shape(nu, t)[ok])))
            r_one = max(r_one, float(np.max(rel / planck_shape(nu, t, 1)[ok])))
        assert np.array_equal(np.isnan(got), np.isnan(np.asarray(want, dtype=np.float64)))
    print("%s: r_ref = %.3f (with one rounding of b: %.3f)" % (name, r_ref, r_one))
    assert r_ref <= 1.0


@pytest.mark.parametrize("name", sorted(REGIMES))
def test_fp64_fold_is_inside_the_propagated_bound(name):
    """The reference's fp64 fold of the columns the GPU tests use stays inside the propagated bound (factor 1)"""
    for n_layers, source in ((1, "incoming"), (7, "surface"), (13, "surface")):
        col = column(name, n_layers)
        tau = [(k, d) for k, d in zip(col["k"], col["depth"])]
        want, bound = reference(name, n_layers, source)
        got = fold_fp64(col["nu"], col["T"], tau, I0=incoming(name, n_layers) if source == "incoming" else None,
                        surface_T=col["surface_T"])
        ratio, worst, n_nan, n_tiny, ok, _ = compare(got, want, bound, 1.0)
        print("%s, %d layers from %s: worst |err| / bound = %.3f at point %d; %d NaN, %d below %g"
              % (name, n_layers, source, ratio, worst, n_nan, n_tiny, TINY))
        assert ok, (name, n_layers, source, ratio, worst)
        assert n_nan == (1 if name.startswith("near_zero") else 0)


def test_bound_would_catch_a_truncated_polynomial_and_needs_no_slack_for_it():
    """What the GPU tests' 4 x bound leaves room for: expm1_tiny cut to degree 2 errs by x^3 / 6 of E at x = (nu_3 - nu_0)
    pbkT, which on `fine` and `coarse_edge_below` is far above 4 S_B - the bound cannot hide it"""
    for name in ("fine", "coarse_edge_below"):
        lo, hi, n, T = REGIMES[name]
        x = 3 * (hi - lo) / (n - 1) * float(np.max(pbkT(T)))
        assert x ** 3 / 6 > 100 * 4 * float(np.max(planck_shape(axis(lo, hi, n), min(T))))
