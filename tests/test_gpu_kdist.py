"""GPU: k-distributions (K9 kdist_* kernels, lbl_rank_order_dev, lbl_ranked_means_dev, model.kDistribution,
Atmosphere.kDistribution) against NumPy: the order and the sorted values bit for bit against numpy.argsort(kind="stable"),
the means against math.fsum within the bound of any fixed-order sum, the mapped mode, independence of rows and calls, the
column's resident coefficients and the C ABI's refusals."""
import math

import numpy as np
import pytest

from pyrad_amd import _native

pytestmark = pytest.mark.gpu

BAD_ARG = -1          # LBL_ERR_BAD_ARG
T = _native.KDIST_TILE
U = 2.0 ** -52
PLANCK_REL = 1e-13    # per-point tolerance of the device's Planck term against planckWavenumber (tests/test_gpu_flux.py: the
#                       spectral fluxes, and the transparent and isothermal columns, which are that term alone)
# (first, count): every length around a wave, a tile and two tiles, one that spans many workgroups; no start a multiple of 4
BANDS = ((1, 1), (3, 2), (9, 63), (77, 64), (145, 65), (215, T - 1), (2301, T), (4403, T + 1), (6501, 2 * T + 1), (5, 300001))
N = 300011


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


@pytest.fixture()
def ctx(pyrad):
    from pyrad_amd import engine
    return engine.get_engine().ctx


# ---- the definition, restated in NumPy ---------------------------------------------------------------------------------
def np_order(x, first, count):
    return first + np.argsort(x[first:first + count], kind="stable")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def np_means(x, order, edges):
    """(mean, bound, lower) of row x over the intervals of `order`: fsum / count, and count * 2^-52 * (sum |x_j| / count) -
    what any fixed-order sum of `count` terms stays inside"""
    v = x[order]
    mean = np.array([math.fsum(v[a:b]) / (b - a) for a, b in zip(edges[:-1], edges[1:])])
    bound = np.array([(b - a) * U * (math.fsum(np.abs(v[a:b])) / (b - a)) for a, b in zip(edges[:-1], edges[1:])])
    return mean, bound, np.r_[v[edges[:-1]], v[-1]]


def contents(kind, seed, n=N):
    rng = np.random.default_rng(seed)
    logu = 10.0 ** rng.uniform(-300.0, 300.0, n)
    if kind == "loguniform":
        return logu
    if kind == "denormals":
        x = rng.integers(1, 2 ** 52, n, dtype=np.uint64).view(np.float64)
        x[::7] = x[3]                                       # ties among them
        return x
    if kind == "equal":
        return np.full(n, 3.25)
    if kind == "ascending":
        return np.sort(np.round(np.log10(logu), 3))         # with runs of ties
    if kind == "descending":
        return np.sort(np.round(np.log10(logu), 3))[::-1].copy()
    if kind == "negative":
        return np.where(rng.random(n) < 0.7, -logu, logu)
    assert kind == "specials"
    x = np.where(rng.random(n) < 0.5, -logu, logu)
    where = rng.permutation(n)
    k = n // 50
    nan_payload = np.array([0x7FF8000000000123, 0xFFF8000000000456, 0x7FF0000000000001], dtype=np.uint64).view(np.float64)
    for i, v in enumerate((0.0, -0.0, np.inf, -np.inf, np.nan, np.copysign(np.nan, -1.0), *nan_payload)):
        x[where[i * k:(i + 1) * k]] = v
    x[:16] = [0.0, -0.0, np.nan, -0.0, 0.0, np.inf, np.copysign(np.nan, -1.0), 1.0, -0.0, np.nan, 0.0, -1.0, np.inf, 0.0, -0.0, 0.0]
    return x


KINDS = ("loguniform", "denormals", "equal", "ascending", "descending", "specials", "negative")


def rank(ctx, rows, first, count):
    """(order, sorted) of lbl_rank_order_dev, (rows, S_total) each, order as the doubles it travels as"""
    rows = np.atleast_2d(rows)
    M, n = rows.shape
    S = int(sum(count))
    need = ctx.rank_order_workspace(M, n, count)
    bufs = [ctx.buffer(M * n).upload(rows.reshape(-1)), ctx.buffer(M * S), ctx.buffer(M * S)]
    if need:
        bufs.append(ctx.buffer(need))
    try:
        ctx.rank_order_dev(n, [(bufs[0], r * n) for r in range(M)], first, count, bufs[1], sorted=bufs[2],
                           work=bufs[3] if need else None)
        return bufs[1].download(M * S).reshape(M, S), bufs[2].download(M * S).reshape(M, S)
    finally:
        for b in bufs:
            b.free()


# ---- 1. order and sorted values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_order_and_sorted_are_numpys_stable_argsort(ctx, kind, n_rows):
    rows = np.stack([contents(kind, 100 + r) for r in range(n_rows)])
    first, count = [f for f, _ in BANDS], [c for _, c in BANDS]
    order, srt = rank(ctx, rows, first, count)
    at = 0
    for f, c in BANDS:
        for r in range(n_rows):
            want = np_order(rows[r], f, c)
            got = order[r, at:at + c]
            assert np.array_equal(got, want.astype(np.float64)), (kind, r, f, c)
            assert np.array_equal(bits(srt[r, at:at + c]), bits(rows[r][want])), (kind, r, f, c)
        at += c


# ---- 2. several bands in one call -------------------------------------------------------------------------------------------
def test_three_bands_in_one_call(ctx):
    x = contents("specials", 7, n=3 * T + 50)
    bands = ((11, 2 * T + 3), (2 * T - 90, T + 70), (3 * T + 41, 1))        # the second overlaps the first; one point
    order, srt = rank(ctx, x, [f for f, _ in bands], [c for _, c in bands])
    assert order.shape == (1, sum(c for _, c in bands))
    at = 0
    for f, c in bands:
        o1, s1 = rank(ctx, x, [f], [c])
        assert np.array_equal(order[0, at:at + c], o1[0]) and np.array_equal(bits(srt[0, at:at + c]), bits(s1[0]))
        assert np.array_equal(o1[0], np_order(x, f, c).astype(np.float64))
        at += c


# ---- 3. means ------------------------------------------------------------------------------------------------------------
def spectra(n, M, seed=11):
    rng = np.random.default_rng(seed)
    rows = 10.0 ** rng.uniform(-3.0, 3.0, (M, n))                      # positive, six decades
    rows[M // 2] *= np.where(rng.random(n) < 0.5, -1.0, 1.0)           # one row with sign changes
    return rows


def index_grid(n):
    """a range whose grid points are their own indices, so that band (a, b) is the points [a, b)"""
    return 0.0, float(n - 1)


_cache = {}


def means_case():
    """four rows, two bands (one of many tiles, one inside a tile) and their NumPy orders, computed once"""
    if not _cache:
        n = 5 * T + 77
        rows = spectra(n, 4)
        bands = [(3, 3 + 4 * T + 9), (4 * T + 21, 4 * T + 21 + 500)]
        orders = [[np_order(rows[r], a, b - a) for a, b in bands] for r in range(4)]
        rows.setflags(write=False)
        _cache["case"] = (n, rows, bands, orders)
    return _cache["case"]


def one_point_edges(count):
    return [0.0, 1.0 / count, 2.0 / count, 0.5, (count - 1.0) / count, 1.0]


@pytest.mark.parametrize("g", [1, 16, "one-point"])
def test_means_against_fsum(pyrad, g):
    n, rows, bands, orders = means_case()
    lo, hi = index_grid(n)
    worst = 0.0
    for b, (a, e) in enumerate(bands):
        gg = one_point_edges(e - a) if g == "one-point" else g
        kd = pyrad.kDistribution(rows, lo, hi, bands=[(a, e)], g=gg, spectra=True)
        edges = pyrad.gIntervals(gg, e - a)
        assert np.array_equal(kd.edges[0], edges) and np.array_equal(kd.weight[0], np.diff(edges) / (e - a))
        assert kd.k[0].shape == (4, edges.size - 1) and kd.kLower[0].shape == (4, edges.size)
        for r in range(4):
            assert np.array_equal(kd.order[0][r], orders[r][b])
            mean, bound, lower = np_means(rows[r], orders[r][b], edges)
            err = np.abs(kd.k[0][r] - mean)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (g, b, r, float(np.max(err / bound)))
            assert np.array_equal(bits(kd.kLower[0][r]), bits(lower))
            assert np.array_equal(bits(kd.kLower[0][r][:-1]), bits(kd.sorted[0][r][edges[:-1]]))
            one = np.flatnonzero(np.diff(edges) == 1)
            assert np.array_equal(bits(kd.k[0][r][one]), bits(kd.sorted[0][r][edges[one]]))      # a one-point interval: exact
            if g == "one-point":
                assert one.tolist() == [0, 1, 4]
    print("kdist means g=%s worst |err|/bound = %.3e" % (g, worst))


def test_one_interval_per_point_returns_the_sorted_values(pyrad):
    n = 700
    rows = spectra(n, 3, seed=5)
    rows[0, 40:44] = [0.0, -0.0, -0.0, 0.0]
    lo, hi = index_grid(n)
    for count in (256, 200, 1):
        kd = pyrad.kDistribution(rows, lo, hi, bands=[(13, 13 + count)], g=np.linspace(0.0, 1.0, count + 1), spectra=True)
        assert kd.edges[0].tolist() == list(range(count + 1))
        assert np.array_equal(bits(kd.k[0]), bits(kd.sorted[0]))
        assert np.array_equal(bits(kd.kLower[0][:, :-1]), bits(kd.sorted[0])) and np.array_equal(bits(kd.kLower[0][:, -1]), bits(kd.sorted[0][:, -1]))


def test_inf_and_nan_pass_through(pyrad):
    n = 3 * T
    rows = spectra(n, 3, seed=9)
    rows[1] = np.abs(rows[1])
    rows[0, 100] = np.inf                                   # the last interval of row 0 holds +inf: its mean is inf
    rows[2, 200] = np.inf
    rows[2, 2 * T + 5] = np.nan                             # that of row 2 +inf and a NaN: NaN
    lo, hi = index_grid(n)
    kd = pyrad.kDistribution(rows, lo, hi, g=16)
    assert kd.k.shape == (3, 16)
    assert kd.k[0, -1] == np.inf and np.isnan(kd.k[2, -1])
    assert np.all(np.isfinite(kd.k[:, :-1])) and np.all(np.isfinite(kd.k[1]))
    assert kd.kLower[0, -1] == np.inf and np.isnan(kd.kLower[2, -1]) and np.all(np.isfinite(kd.kLower[:, :-1]))
    edges = pyrad.gIntervals(16, n)
    for r in range(3):
        v = rows[r][np_order(rows[r], 0, n)]
        with np.errstate(invalid="ignore"):
            want = np.array([np.sum(v[a:b]) / (b - a) for a, b in zip(edges[:-1], edges[1:])])
        assert np.array_equal(np.isnan(kd.k[r]), np.isnan(want)) and np.array_equal(np.isinf(kd.k[r]), np.isinf(want))


# ---- 4. mapped mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [0, 2])
def test_mapped_mode(pyrad, ref):
    n, rows, bands, orders = means_case()
    lo, hi = index_grid(n)
    own = pyrad.kDistribution(rows, lo, hi, bands=bands, g=16)
    kd = pyrad.kDistribution(rows, lo, hi, bands=bands, g=16, reference=ref, spectra=True)
    assert kd.reference == ref and own.reference is None
    for b, (a, e) in enumerate(bands):
        edges = kd.edges[b]
        assert np.array_equal(kd.order[b], orders[ref][b]) and kd.order[b].shape == (e - a,)
        assert np.array_equal(bits(kd.sorted[b]), bits(rows[ref][orders[ref][b]]))
        assert np.array_equal(bits(kd.k[b][ref]), bits(own.k[b][ref]))
        assert np.array_equal(bits(kd.kLower[b][ref]), bits(own.kLower[b][ref]))
        for r in range(4):
            mean, bound, lower = np_means(rows[r], orders[ref][b], edges)
            assert np.all(np.abs(kd.k[b][r] - mean) <= bound), (b, r)
            assert np.array_equal(bits(kd.kLower[b][r]), bits(lower))
            # the weighted means add up to the band mean, whichever order they were taken over
            band = rows[r, a:e]
            total = math.fsum(w * m for w, m in zip(kd.weight[b], kd.k[b][r]))
            assert abs(total - math.fsum(band) / (e - a)) <= (e - a) * U * (math.fsum(np.abs(band)) / (e - a)), (b, r)
            total = math.fsum(w * m for w, m in zip(own.weight[b], own.k[b][r]))
            assert abs(total - math.fsum(band) / (e - a)) <= (e - a) * U * (math.fsum(np.abs(band)) / (e - a)), (b, r)


# ---- 5. reproducibility and independence -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [None, 1])
def test_calls_and_rows_are_independent(pyrad, ref):
    n, rows, bands, _ = means_case()
    lo, hi = index_grid(n)
    three = rows[:3]

    def same(p, q, rp=slice(None), rq=slice(None)):
        for b in range(len(bands)):
            assert np.array_equal(bits(p.k[b][rp]), bits(q.k[b][rq])) and np.array_equal(bits(p.kLower[b][rp]), bits(q.kLower[b][rq]))

    a = pyrad.kDistribution(three, lo, hi, bands=bands, g=16, reference=ref, spectra=True)
    b = pyrad.kDistribution(three, lo, hi, bands=bands, g=16, reference=ref, spectra=True)
    same(a, b)
    for i in range(len(bands)):
        assert np.array_equal(a.order[i], b.order[i]) and np.array_equal(bits(a.sorted[i]), bits(b.sorted[i]))
    alone = pyrad.kDistribution(three[1], lo, hi, bands=bands, g=16, reference=None if ref is None else 0, spectra=True)
    same(alone, a, rq=slice(1, 2))
    for i in range(len(bands)):
        assert np.array_equal(alone.order[i].reshape(-1), a.order[i][1] if ref is None else a.order[i])


# ---- 6. Atmosphere.kDistribution ---------------------------------------------------------------------------------------------
def test_column_against_numpy(pyrad):
    from pyrad_amd import settings
    from test_gpu_instrument import column
    settings.set_resolution_multiplier(0.1)                 # 0.001 cm^-1: 4,000 points (the fixture sets it back)
    atm = column(pyrad)
    bands = [(648.0, 650.0), (649.5, 653.0)]                # the second overlaps the first, ends with the last point and is longer than a tile
    x = atm[0].xAxis
    n = x.size
    assert 3990 <= n <= 4010
    k = [np.array(pyrad.getAbsCoef(L)) for L in atm]
    idx = [(int(np.searchsorted(x, lo)), int(np.searchsorted(x, hi))) for lo, hi in bands]
    assert idx[1][1] == n and idx[1][1] - idx[1][0] > T
    for ref in (None, 1):
        kd = atm.kDistribution(bands=bands, g=8, reference=ref, planck=True, spectra=True)
        for b, (a, e) in enumerate(idx):
            edges = pyrad.gIntervals(8, e - a)
            assert np.array_equal(kd.edges[b], edges) and kd.k[b].shape == kd.planck[b].shape == (len(atm), 8)
            for l, L in enumerate(atm):
                order = np_order(k[l if ref is None else ref], a, e - a)
                got = kd.order[b][l] if ref is None else kd.order[b]
                srt = kd.sorted[b][l] if ref is None else kd.sorted[b]
                assert np.array_equal(got, order)
                assert np.array_equal(bits(srt), bits(k[l if ref is None else ref][order]))
                mean, bound, lower = np_means(k[l], order, edges)
                assert np.array_equal(bits(kd.kLower[b][l]), bits(lower))
                assert np.all(np.abs(kd.k[b][l] - mean) <= bound), (ref, b, l)
                B = pyrad.planckWavenumber(x, L.T)
                mean, bound, _ = np_means(B, order, edges)
                assert np.all(np.abs(kd.planck[b][l] - mean) <= bound + PLANCK_REL * mean), (ref, b, l)
    whole = atm.kDistribution(g=4)
    assert whole.k.shape == (len(atm), 4) and whole.planck is None and whole.order is None and whole.sorted is None
    mean, bound, lower = np_means(k[2], np_order(k[2], 0, n), pyrad.gIntervals(4, n))
    assert np.all(np.abs(whole.k[2] - mean) <= bound) and np.array_equal(bits(whole.kLower[2]), bits(lower))


def test_no_accumulate_after_transmission(pyrad, monkeypatch):
    from pyrad_amd import engine
    from test_gpu_instrument import column
    atm = column(pyrad)
    atm.transmission(surfaceTemperature=288)
    ctx = engine.get_engine().ctx
    jobs = []
    for name in ("layers_merged_accumulate_dev", "layer_merged_step_dev", "xsec_accumulate_dev", "layer_step_dev",
                 "layer_sweep_dev"):
        orig = getattr(ctx, name)
        monkeypatch.setattr(ctx, name, lambda first, *a, _o=orig, _n=name, **kw: (jobs.append((_n, len(first))), _o(first, *a, **kw))[1])
    atm.kDistribution(g=8)
    atm.kDistribution(bands=[(648.0, 650.0), (650.0, 653.0)], g=8, reference=0, planck=True, spectra=True)
    assert all(count == 0 for _, count in jobs), jobs


# ---- 7. refusals of the C entry points ----------------------------------------------------------------------------------------
def test_refusals(ctx):
    n = 2 * T + 40
    rows = spectra(n, 2, seed=3)
    first, count = [5, 100], [T + 30, 64]
    S = sum(count)
    edges = [np.array([0, 10, T + 30]), np.array([0, 1, 64])]
    G = 4
    need = ctx.rank_order_workspace(2, n, count)
    assert need == 3 * 2 * S
    mneed = ctx.ranked_means_workspace(2, count, edges)
    assert mneed == 2 * (1 + 2 + 1 + 1)
    src = ctx.buffer(2 * n).upload(rows.reshape(-1))
    order, srt, work = ctx.buffer(2 * S), ctx.buffer(2 * S), ctx.buffer(need)
    short_order, short_work = ctx.buffer(2 * S - 1), ctx.buffer(need - 1)
    mwork, mean, lower = ctx.buffer(mneed), ctx.buffer(2 * G), ctx.buffer(2 * (G + 2))
    short_mwork, short_mean = ctx.buffer(mneed - 1), ctx.buffer(2 * G - 1)
    two = [(src, 0), (src, n)]

    def do_rank(rows_=two, first_=first, count_=count, order_=order, sorted_=srt, work_=work):
        ctx.rank_order_dev(n, rows_, first_, count_, order_, sorted=sorted_, work=work_)

    def do_means(rows_=two, orders_=None, first_=first, count_=count, edges_=edges, work_=mwork, mean_=mean, lower_=lower, **kw):
        ctx.ranked_means_dev(n, rows_, [(order, 0), (order, S)] if orders_ is None else orders_, first_, count_, edges_,
                             work_, mean_, lower=lower_, **kw)

    many_rows = [(src, 0)] * (_native.limit("kdist_rows") + 1)
    many_edges = [np.arange(_native.limit("kdist_intervals") + 2), edges[1]]
    try:
        do_rank()
        bad_rank = [
            dict(first_=[5, n - 63]),                       # a band beyond n
            dict(count_=[T + 30, 0]),
            dict(first_=[-1, 100]),
            dict(order_=short_order),                       # an order buffer too short
            dict(sorted_=short_order),
            dict(work_=short_work),                         # a work space one double too small
            dict(work_=None),
            dict(order_=None),
            dict(rows_=many_rows),                          # 513 rows
            dict(rows_=[]),
            dict(rows_=[(src, 0), (None, 0)]),
            dict(rows_=[(src, 0), (src, n + 1)]),
            dict(rows_=[(src, -1), (src, n)]),
            dict(first_=[5] * 65, count_=[10] * 65),
        ]
        for kw in bad_rank:
            with pytest.raises(_native.LblError) as e:
                do_rank(**kw)
            assert e.value.code == BAD_ARG, kw
        bad_means = [
            dict(first_=[5, n - 63]),                       # a band beyond n
            dict(edges_=[np.array([0, 10, 10, T + 30]), edges[1]]),      # equal consecutive edges
            dict(edges_=[np.array([0, 20, 10, T + 30]), edges[1]]),
            dict(edges_=[np.array([1, 10, T + 30]), edges[1]]),
            dict(edges_=[np.array([0, 10, T + 29]), edges[1]]),
            dict(orders_=[(order, 0), (order, S + 1)]),     # an order that does not fit its buffer
            dict(orders_=[(short_order, 0), (short_order, S)]),
            dict(orders_=[(order, 0), (None, 0)]),
            dict(work_=short_mwork),                        # a work space one double too small
            dict(work_=None),
            dict(mean_=short_mean),
            dict(mean_=None),
            dict(mean_offset=1),
            dict(mean_offset=-1),
            dict(lower_offset=1),
            dict(rows_=many_rows, orders_=[(order, 0)] * len(many_rows)),      # 513 rows
            dict(count_=[257, 64], edges_=many_edges),      # 257 intervals
        ]
        for kw in bad_means:
            with pytest.raises(_native.LblError) as e:
                do_means(**kw)
            assert e.value.code == BAD_ARG, kw
        # after every refusal the context still serves valid calls
        do_rank()
        do_means()
        got_order = order.download(2 * S).reshape(2, S)
        got_mean = mean.download(2 * G).reshape(2, G)
        got_lower = lower.download(2 * (G + 2)).reshape(2, G + 2)
        for r in range(2):
            at = g0 = 0
            for b in range(2):
                o = np_order(rows[r], first[b], count[b])
                assert np.array_equal(got_order[r, at:at + count[b]], o.astype(np.float64))
                m, bound, lw = np_means(rows[r], o, edges[b])
                assert np.all(np.abs(got_mean[r, g0:g0 + 2] - m) <= bound)
                assert np.array_equal(bits(got_lower[r, g0 + b:g0 + b + 3]), bits(lw))
                at += count[b]
                g0 += 2
    finally:
        for b in (src, order, srt, work, short_order, short_work, mwork, mean, lower, short_mwork, short_mean):
            b.free()
