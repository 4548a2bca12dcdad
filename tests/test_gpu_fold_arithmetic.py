"""GPU: both arithmetic forms of the column fold I <- t I + (1 - t) B (the one-exp form and the general form, chosen per wave
at run time), every switch-over between them and every route that claims the same bits, on the regimes, columns, long-double
reference and error bound of tests/test_fold_regimes_cpu.py.  Everything goes through Context; absorption coefficients and
cross sections are made on the host and uploaded.

Accuracy is |got - reference| <= FACTOR x bound pointwise, bound the propagated bound of the CPU file.  FACTOR = 4 allows for
what the kernels add to the reference's expression - the host-made bracket 100 h c / k / T, the Newton reciprocal, the
polynomial factor - each already counted once in the bound's shape, so 4 cannot hide a lost digit.

test_fold_accuracy prints the worst |err| / bound per regime, form and wave class.  No figure from an MI355X is recorded here
yet: these tests were written without access to one.  What is known is the reference's own fp64 fold of the same columns,
0.30 - 0.51 of the bound (tests/test_fold_regimes_cpu.py prints it), and that cutting expm1_tiny to degree 2 would exceed
4 x the bound a hundredfold on `fine` and `coarse_edge_below` (asserted there)."""
import numpy as np
import pytest

import test_fold_regimes_cpu as reg

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SENTINEL = -7.25
ALL = sorted(reg.REGIMES)
BELOW_690 = ("fine", "coarse", "coarse_edge_below", "coarse_edge_above")


@pytest.fixture(scope="module")
def ctx():
    from pyrad_amd import _native as nat
    c = nat.Context(0)
    c.fold_cache = {}
    yield c
    c.close()


def same_bits(a, b):
    """equal as bit patterns, any NaN equal to any NaN"""
    num = ~np.isnan(a)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[num]), np.signbit(b[num]))


def k_buffers(ctx, name, n_layers):
    """the absorption coefficients of reg.column(name, n_layers) on the device, uploaded once"""
    key = ("k", name, n_layers)
    if key not in ctx.fold_cache:
        col = reg.column(name, n_layers)
        ctx.fold_cache[key] = [ctx.buffer(col["n"]).upload(k) for k in col["k"]]
    return ctx.fold_cache[key]


def fold(ctx, name, n_layers, source, first=0, count=0, trans=None, prefill=None):
    """lbl_column_fold_dev on reg.column(name, n_layers); returns the whole I_out buffer (pre-filled with `prefill`)"""
    col = reg.column(name, n_layers)
    n = col["n"]
    out = ctx.buffer(n)
    I_in = ctx.buffer(n).upload(reg.incoming(name, n_layers)) if source == "incoming" else None
    try:
        if prefill is not None:
            out.fill(prefill)
        ctx.column_fold_dev(k_buffers(ctx, name, n_layers), col["T"], col["depth"], col["lo"], col["hi"], n, out, I_in=I_in,
                            surface_T=0.0 if source == "incoming" else col["surface_T"], trans=trans, first=first, count=count)
        return out.download(n)
    finally:
        out.free()
        if I_in is not None:
            I_in.free()


def fold_whole(ctx, name, n_layers, source):
    """the whole-grid fold, run once per (regime, layers, source) and shared between the tests"""
    key = ("I", name, n_layers, source)
    if key not in ctx.fold_cache:
        got = fold(ctx, name, n_layers, source)
        got.setflags(write=False)
        ctx.fold_cache[key] = got
    return ctx.fold_cache[key]


def per_class(name, n_layers, ratio):
    """worst ratio over the points of the plain, mixed and general waves (the tail points behind the last group of 4 are
    general: they go to the one-point instantiation)"""
    c = reg.regime_classes(name, n_layers)
    worst = [0.0, 0.0, 0.0]
    for kind, a, b in zip(c["kind"], c["start"], c["end"]):
        worst[kind] = max(worst[kind], float(np.max(ratio[a:b])))
    tail = ratio[int(c["end"][-1]):]
    if tail.size:
        worst[2] = max(worst[2], float(np.max(tail)))
    return c, worst


# ---- 1. accuracy of K5b per regime ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,n_layers", [("incoming", 1), ("surface", 7)])
@pytest.mark.parametrize("name", ALL)
def test_fold_accuracy(ctx, name, source, n_layers):
    """lbl_column_fold_dev against the long-double fold: one layer behind a faint incoming radiance (as in test_gpu_abi.py's
    faint-radiance test) and seven layers from the surface.  nu = 0 gives NaN on both sides; where the reference is below
    1e-290 the comparison is absolute; how many points either rule takes is asserted."""
    got = fold_whole(ctx, name, n_layers, source)
    want, bound = reg.reference(name, n_layers, source)
    ratio, worst, n_nan, n_tiny, ok, r = reg.compare(got, want, bound, FACTOR)
    c, by_class = per_class(name, n_layers, r)
    print("%s, %d layer(s) from %s: worst |err| / bound = %.3f at point %d (plain %.3f, mixed %.3f, general %.3f waves: %d / %d / %d); "
          "%d NaN, %d compared absolutely" % (name, n_layers, source, ratio, worst, *by_class, c["plain"], c["mixed"],
                                               c["general"], n_nan, n_tiny))
    assert ok, (name, source, ratio, worst, float(got[worst]), float(want[worst]))
    if name.startswith("near_zero"):
        assert (n_nan, n_tiny) == (1, 0) and np.isnan(got[0])
    elif name in BELOW_690:
        assert (n_nan, n_tiny) == (0, 0)
    else:
        # by construction: the opaque group of a single cold layer, whose result is that layer's B < 1e-290
        g = reg.special_groups(reg.REGIMES[name][2])
        assert n_nan == 0 and n_tiny == (4 if n_layers == 1 else 0)
        assert n_tiny == 0 or np.all(np.asarray(want[g + 4:g + 8], dtype=np.float64) < reg.TINY)
    # the two special groups: optical depth 0 hands the incoming radiance on unchanged, 900 leaves the top layer's B
    g = reg.special_groups(reg.REGIMES[name][2])
    if source == "incoming":
        assert same_bits(got[g:g + 4], reg.incoming(name, n_layers)[g:g + 4])


# ---- 2. the two forms agree across every switch --------------------------------------------------------------------------------
def test_both_sides_of_the_step_threshold(ctx):
    """The same layers 10 % below and 10 % above 3 step pbkT_max = 1e-3: one grid runs the one-exp form in every wave, the
    other the general form, each inside the same bound of the long-double fold on its own grid."""
    worst = {}
    for name, cls in (("coarse_edge_below", "plain"), ("coarse_edge_above", "general")):
        c = reg.regime_classes(name, 7)
        assert c[cls] == len(c["kind"]) > 0, (name, c)
        got = fold_whole(ctx, name, 7, "surface")
        want, bound = reg.reference(name, 7, "surface")
        ratio, at, n_nan, n_tiny, ok, _ = reg.compare(got, want, bound, FACTOR)
        worst[name] = ratio
        assert ok and n_nan == 0 and n_tiny == 0, (name, ratio, at)
    print("step threshold: worst |err| / bound below %.3f (one-exp form), above %.3f (general form)"
          % (worst["coarse_edge_below"], worst["coarse_edge_above"]))


@pytest.mark.parametrize("name", ["hot_exponent", "near_zero", "near_zero_fine"])
def test_plain_mixed_and_general_waves_share_one_bound(ctx, name):
    """Inside one call: the waves before the threshold, the mixed wave on it (which must fall back as a whole) and the waves
    behind it all stay within the bound; the first and the last point of every mixed wave by name."""
    got = fold_whole(ctx, name, 7, "surface")
    want, bound = reg.reference(name, 7, "surface")
    _, _, _, _, _, r = reg.compare(got, want, bound, FACTOR)
    c, by_class = per_class(name, 7, r)
    assert c["mixed"] >= 1
    print("%s: worst |err| / bound in plain / mixed / general waves = %.3f / %.3f / %.3f" % (name, *by_class))
    nu = reg.column(name, 7)["nu"]
    for w in np.flatnonzero(c["kind"] == 1):
        a, b = int(c["start"][w]), int(c["end"][w]) - 1
        for j in (a, b):
            if np.isnan(want[j]):
                assert np.isnan(got[j]), "mixed wave %d, point %d (nu = %r): not NaN" % (w, j, nu[j])
                continue
            assert np.isfinite(got[j]) and r[j] <= FACTOR, \
                "mixed wave %d (points %d .. %d): point %d (nu = %r) is %.3f x the bound" % (w, a, b, j, nu[j], r[j])
    assert max(by_class) <= FACTOR, (name, by_class)


# ---- 4. windows -----------------------------------------------------------------------------------------------------------------
def windows(n):
    k = 300                                  # (4 k + 1 .. 3 points: more than one workgroup of quads, then a tail launch)
    return [(0, n), (4, n - 4), (1, n - 1), (2, n - 2), (3, 7), (0, 4 * k + 1), (0, 4 * k + 2), (0, 4 * k + 3), (n - 3, 3),
            (n - 1, 1)]


def check_window(got, want, bound, first, count, what):
    n = len(got)
    inside = np.zeros(n, dtype=bool)
    inside[first:first + count] = True
    assert np.all(got[~inside] == SENTINEL), "%s: wrote outside its window at %r" % (what, np.flatnonzero(~inside & (got != SENTINEL))[:8])
    ratio, at, _, _, ok, _ = reg.compare(got[inside], want[inside], bound[inside], FACTOR)
    assert ok, "%s: %.3f x the bound at point %d" % (what, ratio, first + at)


def step_layers(name, n_layers, n_iso=lambda l: 1):
    """reg.column(name, n_layers) as cross sections for lbl_column_step_dev / lbl_layer_sweep_dev: layer l has n_iso(l) = 1..3
    cross-section arrays in one or two molecules.  Returns (layers without buffers, k): k[l] is the absorption coefficient
    the kernel forms from them, restated in NumPy operation for operation (zeros + arrays per molecule, times the molecule's
    host-made factor conc P / 1E4 / k_B / T, summed over molecules)."""
    col = reg.column(name, n_layers)
    rng = np.random.default_rng([9, n_layers])
    layers, ks = [], []
    for l in range(n_layers):
        ni = n_iso(l)
        iso_mol = {1: [0], 2: [0, 0], 3: [0, 0, 1]}[ni]
        conc = [4e-4, 1.2e-2][:max(iso_mol) + 1]
        P, T = 1013.25 / (l + 1), col["T"][l]
        f = [c * P / 1E4 / reg.orc.k / T for c in conc]
        w = rng.uniform(0.2, 1.0, ni)
        w /= w.sum()
        xs = [col["k"][l] * w[i] / f[iso_mol[i]] for i in range(ni)]
        kk = np.zeros(col["n"])
        for m in range(len(conc)):
            s = np.zeros(col["n"])
            for i in range(ni):
                if iso_mol[i] == m:
                    s = s + xs[i]
            kk = kk + s * f[m]
        layers.append(dict(xsec=xs, iso_mol=iso_mol, conc=conc, P=P, T=T, depth=col["depth"][l]))
        ks.append(kk)
    return layers, ks


def upload_layers(ctx, layers, n):
    return [dict(L, xsec=[ctx.buffer(n).upload(x) for x in L["xsec"]], abs_coef=None, trans=None) for L in layers]


def free_all(bufs):
    for b in bufs:
        if b is not None:
            b.free()


@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_fold_windows(ctx, name):
    """lbl_column_fold_dev on windows on and off the 4-point alignment: inside within the bound, outside untouched bit for bit;
    (0, n) and (4, n - 4) send the same aligned quads to the same instantiation: the same bits.  A window that starts on an
    odd point runs the one-point instantiation, which has only the general form: on every regime it repeats lbl_column_sweep_dev
    over the transmittances it wrote bit for bit (on `fine` it would not if it were sent to the four-point kernel)."""
    col = reg.column(name, 5)
    n = col["n"]
    want, bound = reg.reference(name, 5, "surface")
    got = {}
    for first, count in windows(n):
        got[first, count] = fold(ctx, name, 5, "surface", first, count, prefill=SENTINEL)
        check_window(got[first, count], want, bound, first, count, "fold %s (%d, %d)" % (name, first, count))
    assert same_bits(got[0, n][4:], got[4, n - 4][4:])
    assert same_bits(got[0, n], fold_whole(ctx, name, 5, "surface"))          # (count 0 means the whole grid)
    trans = [ctx.buffer(n).fill(SENTINEL) for _ in range(5)]
    out = ctx.buffer(n).fill(SENTINEL)
    try:
        odd = fold(ctx, name, 5, "surface", 1, n - 1, trans=trans, prefill=SENTINEL)
        assert same_bits(odd, got[1, n - 1])
        ctx.column_sweep_dev(trans, col["T"], col["lo"], col["hi"], n, out, surface_T=col["surface_T"], first=1, count=n - 1)
        assert same_bits(out.download(n), odd)
    finally:
        free_all(trans + [out])


@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_step_and_sweep_windows(ctx, name):
    """The same windows through lbl_column_step_dev (five layers from cross sections), lbl_layer_sweep_dev (one layer: two
    points per thread on an even first point, one on an odd) and lbl_column_sweep_dev (two layers from transmittances)."""
    col5, col2, col1 = reg.column(name, 5), reg.column(name, 2), reg.column(name, 1)
    n = col5["n"]
    layers5, k5 = step_layers(name, 5)
    layers1, k1 = step_layers(name, 1)
    want5, bound5 = reg.fold_long(col5["nu"], col5["T"], list(zip(k5, col5["depth"])), surface_T=col5["surface_T"])
    want1, bound1 = reg.fold_long(col1["nu"], col1["T"], list(zip(k1, col1["depth"])), surface_T=col1["surface_T"])
    t2 = [np.exp(-(k * d)) for k, d in zip(col2["k"], col2["depth"])]
    want2, bound2 = reg.fold_long(col2["nu"], col2["T"], None, surface_T=col2["surface_T"], trans=t2)
    dev5, dev1 = upload_layers(ctx, layers5, n), upload_layers(ctx, layers1, n)
    tb = [ctx.buffer(n).upload(t) for t in t2]
    out = ctx.buffer(n)
    try:
        step = {}
        for first, count in windows(n):
            out.fill(SENTINEL)
            ctx.column_step_dev(dev5, col5["lo"], col5["hi"], n, out, surface_T=col5["surface_T"], first=first, count=count)
            step[first, count] = out.download(n)
            check_window(step[first, count], want5, bound5, first, count, "step %s (%d, %d)" % (name, first, count))
            out.fill(SENTINEL)
            L = dev1[0]
            ctx.layer_sweep_dev(L["xsec"], L["iso_mol"], L["conc"], L["P"], L["T"], L["depth"], col1["lo"], col1["hi"], n,
                                surface_T=col1["surface_T"], I_out=out, first=first, count=count)
            check_window(out.download(n), want1, bound1, first, count, "layer sweep %s (%d, %d)" % (name, first, count))
            out.fill(SENTINEL)
            ctx.column_sweep_dev(tb, col2["T"], col2["lo"], col2["hi"], n, out, surface_T=col2["surface_T"], first=first,
                                 count=count)
            check_window(out.download(n), want2, bound2, first, count, "column sweep %s (%d, %d)" % (name, first, count))
        assert same_bits(step[0, n][4:], step[4, n - 4][4:])
    finally:
        free_all([b for L in dev5 + dev1 for b in L["xsec"]] + tb + [out])


# ---- 5. routes that claim the same bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_routes_give_the_same_bits(ctx, name):
    """Five layers.  (a) lbl_column_step_dev from one cross section per layer, asked for the layers' abs_coef and trans, and
    lbl_column_fold_dev over those abs_coef: I_out and every trans (KFOLD against the general term walk, with and without
    per-layer arrays).  (b) up_top of lbl_column_flux_dev with the single angle mu = 1, weight 1; (c) a vertical surface ray of
    lbl_ray_radiance_dev through all layers; (d) F of lbl_column_jacobian_dev with the same angle and one band over the whole
    grid against level_flux[up][top] of (b).  All bit for bit, in every regime."""
    nl = 5
    col = reg.column(name, nl)
    n, lo, hi, T, depth, Ts = col["n"], col["lo"], col["hi"], col["T"], col["depth"], col["surface_T"]
    layers, ks = step_layers(name, nl)
    dev = upload_layers(ctx, layers, n)
    kb, tb, tf = ([ctx.buffer(n) for _ in range(nl)] for _ in range(3))
    for l in range(nl):
        dev[l]["abs_coef"], dev[l]["trans"] = kb[l], tb[l]
    out_step, out_fold, out_bare, up_top, rad = (ctx.buffer(n) for _ in range(5))
    level, jac = ctx.buffer(2 * (nl + 1)), ctx.buffer(2 + 2 * nl)
    try:
        ctx.column_step_dev(dev, lo, hi, n, out_step, surface_T=Ts)
        ctx.column_fold_dev(kb, T, depth, lo, hi, n, out_fold, surface_T=Ts, trans=tf)
        ctx.column_fold_dev(kb, T, depth, lo, hi, n, out_bare, surface_T=Ts)
        I_step, I_fold = out_step.download(n), out_fold.download(n)
        assert same_bits(kb[0].download(n), ks[0]) and same_bits(kb[nl - 1].download(n), ks[nl - 1])
        want, bound = reg.fold_long(col["nu"], T, list(zip(ks, depth)), surface_T=Ts)
        ratio, at, _, _, ok, _ = reg.compare(I_fold, want, bound, FACTOR)
        assert ok, (name, ratio, at)
        assert same_bits(I_step, I_fold), (name, "(a) I_out", np.flatnonzero(I_step != I_fold)[:8])
        assert same_bits(out_bare.download(n), I_fold), (name, "(a) I_out with and without per-layer arrays")
        for l in range(nl):
            assert same_bits(tb[l].download(n), tf[l].download(n)), (name, "(a) trans", l)
        ctx.column_flux_dev(kb, T, depth, lo, hi, n, [1.0], [1.0], [0], [n], level, surface_T=Ts, up_top=up_top)
        I_flux = up_top.download(n)
        assert same_bits(I_flux, I_fold), (name, "(b)", np.flatnonzero(I_flux != I_fold)[:8])
        ctx.ray_radiance_dev(kb, T, lo, hi, n, [0, nl], list(range(nl)), list(depth), [1], rad, source_T=Ts)
        I_ray = rad.download(n)
        assert same_bits(I_ray, I_fold), (name, "(c)", np.flatnonzero(I_ray != I_fold)[:8])
        ctx.column_jacobian_dev(kb, T, depth, lo, hi, n, [1.0], [1.0], [0], [n], jac, surface_T=Ts)
        F_jac, F_flux = jac.download(1)[0], level.download(2 * (nl + 1))[nl]
        assert F_jac == F_flux and np.isfinite(F_flux), (name, "(d)", F_jac, F_flux)
    finally:
        free_all([b for L in dev for b in L["xsec"]] + kb + tb + tf + [out_step, out_fold, out_bare, up_top, rad, level, jac])


# ---- 6. layer counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_layers", reg.LAYER_COUNTS)
@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_layer_counts(ctx, name, n_layers):
    """1, 2, 5, 7 and 13 layers (n_terms % NB for NB = 2 and 6, an empty and a non-empty remainder, more than one
    double-buffered batch) through lbl_column_fold_dev and, with one to three cross sections per layer (13 .. 25 terms for 13
    layers), through lbl_column_step_dev; trans asked for on some layers and not on others."""
    col = reg.column(name, n_layers)
    n, lo, hi, T, depth, Ts = col["n"], col["lo"], col["hi"], col["T"], col["depth"], col["surface_T"]
    U = reg.U

    def check_trans(buf, k, d, what):
        t = np.exp(-(k.astype(np.longdouble) * np.longdouble(d)))
        err = np.asarray(np.abs(buf.download(n).astype(np.longdouble) - t), dtype=np.float64)
        assert np.all(err <= 2.5 * U), (what, float(np.max(err)) / U)

    # the fold: trans on the even layers (the first among them, the last too when it is even)
    want, bound = reg.reference(name, n_layers, "surface")
    trans = [ctx.buffer(n) if l % 2 == 0 else None for l in range(n_layers)]
    try:
        got = fold(ctx, name, n_layers, "surface", trans=trans)
        ratio, at, _, _, ok, _ = reg.compare(got, want, bound, FACTOR)
        assert ok, ("fold", name, n_layers, ratio, at)
        assert same_bits(got, fold_whole(ctx, name, n_layers, "surface"))        # per-layer arrays do not change the radiance
        for l in (0, n_layers - 1):
            if trans[l] is not None:
                check_trans(trans[l], col["k"][l], depth[l], ("fold", l))
    finally:
        free_all(trans)
    # the step from cross sections: trans on the odd layers (neither the first nor, for an odd count, the last)
    layers, ks = step_layers(name, n_layers, n_iso=lambda l: 1 + l % 3)
    assert n_layers != 13 or 13 <= sum(len(L["xsec"]) for L in layers) <= 30
    dev = upload_layers(ctx, layers, n)
    trans = [ctx.buffer(n) if l % 2 == 1 else None for l in range(n_layers)]
    out = ctx.buffer(n)
    try:
        for l in range(n_layers):
            dev[l]["trans"] = trans[l]
        ctx.column_step_dev(dev, lo, hi, n, out, surface_T=Ts)
        want, bound = reg.fold_long(col["nu"], T, list(zip(ks, depth)), surface_T=Ts)
        ratio, at, _, _, ok, _ = reg.compare(out.download(n), want, bound, FACTOR)
        print("%s, %d layers, %d terms: step worst |err| / bound = %.3f" % (name, n_layers, sum(len(L["xsec"]) for L in layers), ratio))
        assert ok, ("step", name, n_layers, ratio, at)
        if n_layers > 1:
            check_trans(trans[1], ks[1], depth[1], ("step", 1))
    finally:
        free_all([b for L in dev for b in L["xsec"]] + trans + [out])
