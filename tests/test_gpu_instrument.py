"""GPU: instrument channels (K8 ils_convolve_kernel, lbl_ils_convolve_dev, model.convolve, Atmosphere.observe) against a
NumPy restatement of the definition (written out below, summed with math.fsum), for exact constants, boxcar means,
independence of rows and calls, identity with the spectral entry points it composes, laziness and the C ABI's refusals."""
import math

import numpy as np
import pytest

from pyrad_amd import synthetic

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
SHAPES = ("gaussian", "triangle", "boxcar", "sinc", "table")
LO, HI = 600.0, 604.0
SUPPORTS = (1, 2, 63, 64, 65, 255, 256, 257, 1025)          # across every lane, wave and workgroup stride
U = 2.0 ** -52


@pytest.fixture()
def pyrad():
    from pyrad_amd import model, data, settings
    model.Layer.hasAtmosphere = False
    settings.set_resolution_multiplier(1)
    settings.set_layer_step("merged")
    yield model
    settings.set_layer_step("merged")
    settings.set_resolution_multiplier(1)
    data.set_source(None)


# ---- the definition, restated in NumPy ---------------------------------------------------------------------------------
def weights(ins, c, position, first, count, step):
    """(w_cj, e_cj) over the support of channel c: x = (j - p) * step, t = x / width, w = shape(t), in that order"""
    j = np.arange(first[c], first[c] + count[c]).astype(np.float64)
    x = (j - position[c]) * step
    if ins.shape == "table":
        nt, half = ins.table.size, ins.tableHalf
        u = (x + half) * ((nt - 1) / (2.0 * half))
        i = np.clip(u.astype(np.int64), 0, nt - 2)
        w = ins.table[i] + (u - i) * (ins.table[i + 1] - ins.table[i])
        w = np.where((x >= -half) & (x <= half), w, 0.0)
        return w, np.abs(w)
    t = x / ins.width[c]
    if ins.shape == "gaussian":
        w = np.exp(-2.772588722239781 * (t * t))
    elif ins.shape == "triangle":
        w = np.maximum(0.0, 1.0 - np.abs(t))
    elif ins.shape == "boxcar":
        w = np.where(np.abs(t) <= 0.5, 1.0, 0.0)
    else:
        pt = np.pi * t
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(pt == 0.0, 1.0, np.sin(pt) / pt)
            return w, np.minimum(1.0, 1.0 / np.abs(pt))
    return w, np.abs(w)


def restate(ins, rows, lo, hi):
    """(value, bound) per row and channel: fsum(w S) / fsum(w) and
    4 * 2^-52 * sum_j (count |w_j| + 64 e_j) |S_j| / |sum_j w_j|"""
    n = rows.shape[1]
    step = (hi - lo) / (n - 1)
    position, first, count = ins.support(lo, hi, n)
    want = np.empty((rows.shape[0], len(ins)))
    bound = np.empty_like(want)
    for c in range(len(ins)):
        w, e = weights(ins, c, position, first, count, step)
        den = math.fsum(w)
        for r in range(rows.shape[0]):
            S = rows[r, first[c]:first[c] + count[c]]
            want[r, c] = math.fsum(w * S) / den
            bound[r, c] = 4 * U * math.fsum((count[c] * np.abs(w) + 64 * e) * np.abs(S)) / abs(den)
    return want, bound


def grid():
    from pyrad_amd import settings
    settings.set_resolution_multiplier(0.1)
    n = int((HI - LO) / settings.BASE_RESOLUTION)           # as Layer._grid counts the base grid
    settings.set_resolution_multiplier(1)
    assert 3990 <= n <= 4010
    return n, np.linspace(LO, HI, n), (HI - LO) / (n - 1)


def instrument(pyrad, shape, n, x, step):
    """Unsorted channels whose supports hold exactly SUPPORTS points, one on the first and one on the last grid point"""
    j0 = n // 2
    centres, cutoff = [], []
    for k in SUPPORTS:
        centres.append(x[j0] if k % 2 else 0.5 * (x[j0] + x[j0 + 1]))
        cutoff.append(((k - 1) / 2.0 + 0.3) * step)
    centres += [LO + 0.0625, HI - 0.0625, x[n // 5] + 0.37 * step]
    cutoff += [0.0625, 0.0625, 40.2 * step]
    order = np.random.default_rng(5).permutation(len(centres))
    centres, cutoff = np.array(centres)[order], np.array(cutoff)[order]
    if shape == "table":
        off = np.linspace(-0.6, 0.6, 41)
        ins = pyrad.Instrument(centres, shape="table", cutoff=cutoff,
                               table=(off, np.exp(-(off / 0.3) ** 2) * (1.0 + 0.4 * off) + 0.01))
    else:
        width = np.maximum({"gaussian": cutoff / 2.5, "triangle": cutoff * 1.1, "boxcar": cutoff * 2.0,
                            "sinc": cutoff / 3.3}[shape], 0.5 * step)
        ins = pyrad.Instrument(centres, shape=shape, width=width, cutoff=cutoff)
    _, first, count = ins.support(LO, HI, n)
    assert set(SUPPORTS) <= set(count.tolist())
    assert first.min() == 0 and (first + count).max() == n
    return ins


def spectra(n, M):
    rng = np.random.default_rng(11)
    rows = 10.0 ** rng.uniform(-3.0, 3.0, (M, n))                      # positive, six decades
    rows[M // 2] *= np.where(rng.random(n) < 0.5, -1.0, 1.0)           # one row with sign changes
    return rows


_cache = {}


def case(pyrad, shape):
    """the instrument, 2 x the row block + 1 rows and the restatement of them, computed once per shape"""
    if shape not in _cache:
        from pyrad_amd import _native
        n, x, step = grid()
        ins = instrument(pyrad, shape, n, x, step)
        rows = spectra(n, 2 * _native.ILS_ROW_BLOCK + 1)
        want, bound = restate(ins, rows, LO, HI)
        for a in (rows, want, bound):
            a.setflags(write=False)
        _cache[shape] = (ins, rows, want, bound)
    return _cache[shape]


# ---- 1. parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_restatement(pyrad, shape):
    """Measured on an MI355X: the worst |error| / bound over all rows, channels and row counts is recorded in DESIGN.md
    (K8); the bound is derived in the issue, not measured."""
    from pyrad_amd import _native
    ins, rows, want, bound = case(pyrad, shape)
    B = _native.ILS_ROW_BLOCK
    worst = 0.0
    for M in (1, B, B + 1, 2 * B + 1):
        got = pyrad.convolve(ins, rows[:M], LO, HI)
        assert got.shape == (M, len(ins))
        ratio = np.abs(got - want[:M]) / bound[:M]
        worst = max(worst, float(ratio.max()))
        print("ils parity %s rows=%d worst |err|/bound = %.3e" % (shape, M, ratio.max()))
        assert np.all(np.abs(got - want[:M]) <= bound[:M]), (shape, M, float(ratio.max()))
    one = pyrad.convolve(ins, rows[3], LO, HI)
    assert one.shape == (len(ins),) and np.all(np.abs(one - want[3]) <= bound[3])


# ---- 2. exact properties --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_constant_row_returns_the_constant(pyrad, shape):
    ins, rows, _, _ = case(pyrad, shape)
    n = rows.shape[1]
    const = np.stack([np.full(n, 3.5), rows[0], np.full(n, 3.5)])      # alone in its block and beside another row
    assert np.all(pyrad.convolve(ins, const[0], LO, HI) == 3.5)
    got = pyrad.convolve(ins, const, LO, HI)
    assert np.all(got[0] == 3.5) and np.all(got[2] == 3.5)


def test_boxcar_is_the_mean_of_its_points(pyrad):
    n, x, step = grid()
    rows = spectra(n, 3)
    ks = (1, 2, 7, 64, 65, 300, 1025)
    j0 = n // 3
    centres = np.array([x[j0] if k % 2 else 0.5 * (x[j0] + x[j0 + 1]) for k in ks])
    width = np.array([2 * ((k - 1) / 2.0 + 0.3) * step for k in ks])
    ins = pyrad.Instrument(centres, shape="boxcar", width=width)
    _, first, count = ins.support(LO, HI, n)
    assert count.tolist() == list(ks)
    got = pyrad.convolve(ins, rows, LO, HI)
    for c, k in enumerate(ks):
        for r in range(3):
            S = rows[r, first[c]:first[c] + k]
            assert abs(got[r, c] - math.fsum(S) / k) <= k * U * np.mean(np.abs(S)), (r, k)


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_and_calls_are_independent(pyrad, shape):
    ins, rows, _, _ = case(pyrad, shape)
    together = pyrad.convolve(ins, rows, LO, HI)
    assert np.array_equal(together, pyrad.convolve(ins, rows, LO, HI))
    for r in range(rows.shape[0]):
        assert np.array_equal(together[r], pyrad.convolve(ins, rows[r], LO, HI)), r
    assert np.array_equal(together[5:8], pyrad.convolve(ins, rows[5:8], LO, HI))


# ---- 3. Atmosphere.observe --------------------------------------------------------------------------------------------------
RNG = (648, 652)
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0))


def column(pyrad, layers=LAYERS, co2=400):
    from pyrad_amd import data
    data.set_source(data.synthetic_source(dict(co2=synthetic.make_lines(51, 300, 640, 660))))
    atm = pyrad.Atmosphere("col")
    for depth, T, P in layers:
        atm.addLayer(depth, T, P, *RNG).addMolecule('co2', ppm=co2)
    return atm


def channels(pyrad, **kw):
    return pyrad.Instrument(np.r_[np.arange(649.0, 651.01, 0.125), 648.75, 651.25], width=0.2, **kw)


def test_observe_is_convolve_of_the_spectral_entry_points(pyrad):
    atm = column(pyrad)
    ins = channels(pyrad)
    nl, C = len(atm), len(ins)
    toa = np.array(atm.transmission(surfaceTemperature=288))
    ob = atm.observe(ins, surfaceTemperature=288)
    assert ob.mu == 1.0 and ob.radiance.shape == (C,) and np.array_equal(ob.wavenumber, ins.centres)
    assert ob.temperatureJacobian is None and ob.opticalDepthJacobian is None and ob.brightnessTemperatureJacobian is None
    assert np.array_equal(ob.radiance, pyrad.convolve(ins, toa, *RNG))
    assert np.array_equal(ob.brightnessTemperature, pyrad.brightnessTemperature(ins.centres, ob.radiance))
    assert np.all((ob.brightnessTemperature > 200) & (ob.brightnessTemperature < 300))
    # a slant view, from a surface spectrum
    surf = atm[0].planck(300)
    ob = atm.observe(ins, surfaceSpectrum=surf, mu=0.5)
    f = atm.fluxes(surfaceSpectrum=surf, angles=[(0.5, 1.0)], spectra=True)
    assert ob.mu == 0.5 and np.array_equal(ob.radiance, pyrad.convolve(ins, f.upSpectrum, *RNG))
    # the weighting functions
    for mu in (1.0, 0.5):
        ob = atm.observe(ins, surfaceTemperature=288, mu=mu, jacobians=True)
        j = atm.jacobians(surfaceTemperature=288, angles=[(mu, 1.0)], molecules=False, spectra=True)
        f = atm.fluxes(surfaceTemperature=288, angles=[(mu, 1.0)], spectra=True)
        assert np.array_equal(ob.radiance, pyrad.convolve(ins, f.upSpectrum, *RNG))
        assert ob.temperatureJacobian.shape == ob.opticalDepthJacobian.shape == (nl, C)
        assert np.array_equal(ob.temperatureJacobian, pyrad.convolve(ins, j.temperatureSpectrum, *RNG))
        assert np.array_equal(ob.opticalDepthJacobian, pyrad.convolve(ins, j.opticalDepthSpectrum, *RNG))
        assert np.all(ob.temperatureJacobian > 0)
        Tb = pyrad.brightnessTemperature(ins.centres, ob.radiance)
        b = 100 * pyrad.h * pyrad.c * ins.centres / pyrad.k / Tb
        dBdT = pyrad.planckWavenumber(ins.centres, Tb) * b * np.exp(b) / ((np.exp(b) - 1) * Tb)
        assert np.array_equal(ob.brightnessTemperature, Tb)
        assert np.array_equal(ob.brightnessTemperatureJacobian, ob.temperatureJacobian / dBdT)


def test_isothermal_column_has_its_temperature(pyrad):
    T = 260.0
    atm = column(pyrad, layers=tuple((d, T, P) for d, _, P in LAYERS))
    ins = channels(pyrad)
    ob = atm.observe(ins, surfaceTemperature=T)
    x = atm[0].xAxis
    assert x.size == int((RNG[1] - RNG[0]) / 0.01)
    planck = pyrad.planckWavenumber(x, T)
    want, bound = restate(ins, planck[None, :], *RNG)
    Tb = pyrad.brightnessTemperature(ins.centres, want[0])
    b = 100 * pyrad.h * pyrad.c * ins.centres / pyrad.k / Tb
    dBdT = want[0] * b * np.exp(b) / ((np.exp(b) - 1) * Tb)
    print("isothermal worst |dTb| / tolerance = %.3e" % np.max(np.abs(ob.brightnessTemperature - Tb) / (bound[0] / dBdT)))
    assert np.all(np.abs(ob.brightnessTemperature - Tb) <= bound[0] / dBdT)
    assert np.all(np.abs(ob.brightnessTemperature - T) < 1e-3)          # (the Planck curve bends little over a channel)


def test_no_accumulate_after_transmission(pyrad, monkeypatch):
    from pyrad_amd import engine
    atm = column(pyrad)
    ins = channels(pyrad)
    atm.transmission(surfaceTemperature=288)
    ctx = engine.get_engine().ctx
    jobs = []
    for name in ("layers_merged_accumulate_dev", "layer_merged_step_dev", "xsec_accumulate_dev", "layer_step_dev",
                 "layer_sweep_dev"):
        orig = getattr(ctx, name)
        monkeypatch.setattr(ctx, name, lambda first, *a, _o=orig, _n=name, **kw: (jobs.append((_n, len(first))), _o(first, *a, **kw))[1])
    atm.observe(ins, surfaceTemperature=288)
    atm.observe(ins, surfaceTemperature=288, mu=0.7, jacobians=True)
    assert all(count == 0 for _, count in jobs), jobs


# ---- 4. refusals of the C entry point ---------------------------------------------------------------------------------------
def test_refusals(pyrad):
    from pyrad_amd import _native, engine
    ctx = engine.get_engine().ctx
    ins, rows, want, bound = case(pyrad, "gaussian")
    n, C = rows.shape[1], len(ins)
    position, first, count = ins.support(LO, HI, n)
    src = ctx.buffer(2 * n).upload(np.ascontiguousarray(rows[:2]).reshape(-1))
    out = ctx.buffer(2 * C)
    short = ctx.buffer(2 * C - 1)
    table = np.ones(8)
    G = _native.ILS_SHAPES["gaussian"]
    TBL = _native.ILS_SHAPES["table"]

    def call(rows_=None, position_=position, width_=ins.width, first_=first, count_=count, shape=G, out_=out, **kw):
        ctx.ils_convolve_dev(LO, HI, n, [(src, 0), (src, n)] if rows_ is None else rows_, position_, width_, first_,
                             count_, shape, out_, **kw)

    def changed(a, i, v):
        a = np.array(a)
        a[i] = v
        return a

    try:
        bad = [
            dict(rows_=[]),
            dict(rows_=[(src, 0)] * (_native.limit("ils_rows") + 1)),
            dict(position_=position[:0], width_=ins.width[:0], first_=first[:0], count_=count[:0]),
            dict(count_=changed(count, 2, 0)),
            dict(first_=changed(first, 1, -1)),
            dict(first_=changed(first, 4, n - count[4] + 1)),
            dict(width_=changed(ins.width, 0, 0.0)),
            dict(width_=changed(ins.width, 3, np.nan)),
            dict(shape=5),
            dict(shape=-1),
            dict(shape=TBL, table=np.ones(1), table_half=0.5),
            dict(shape=TBL, table=np.ones(_native.limit("ils_table") + 1), table_half=0.5),
            dict(shape=TBL, table=table, table_half=0.0),
            dict(shape=TBL, table=table, table_half=np.nan),
            dict(rows_=[(src, 0), (None, 0)]),
            dict(out_=None),
            dict(rows_=[(src, 0), (src, n + 1)]),
            dict(rows_=[(src, -1), (src, n)]),
            dict(out_=short),
        ]
        many = _native.limit("ils_channels") + 1
        bad.append(dict(position_=np.full(many, position[0]), width_=np.full(many, ins.width[0]),
                        first_=np.full(many, first[0]), count_=np.full(many, count[0])))
        for kw in bad:
            with pytest.raises(_native.LblError) as e:
                call(**kw)
            assert e.value.code == BAD_ARG, kw
        out.upload(np.zeros(2 * C))
        call()                                                           # and a valid call still answers
        got = out.download(2 * C).reshape(2, C)
        assert np.all(np.abs(got - want[:2]) <= bound[:2])
    finally:
        for b in (src, out, short):
            b.free()
