"""GPU: the far loop's span-level bound on the Gaussian reach, its peeled last chunk and its record addresses (K2).

K1 writes the largest Gaussian cut-off of every block of 256 prepared records; a wave of the far-field kernel takes the
maximum over the blocks that meet its span's interior range once, and a far chunk that lies beyond that distance skips the
per-record reach test.  lbl_set_option "accum_reach_skip" 0 makes the kernel ignore the bound (every chunk forms the test,
as before the bound existed), so 0 against 1 must agree bit for bit wherever the bound is right:

(a) 600 lines on an 8,192-point grid at 1013.25 mbar (window 5,000 points: far chunks on both sides of most spans), the
    per-list and the merged step, 16- and 32-point Gaussian runs;
(b) the same grid at 5 atm (hot gas, 800 K: at 296 K every line there is pure Lorentz and has no Gaussian part to reach
    anything): profiles several times as wide, Gaussian reaches beyond 8 half-spans, so far records beyond the cap keep
    the far loop's four-point pass whenever the bound says they can reach; also against the all-direct kernel
    (accum_variant 0) inside conftest.point_tolerance;
(c) one very wide record (gamma_air 0.5) among narrow ones, in the last position of a K1 block and in the first position
    of the next, with a span whose interior range starts exactly at that record (a grid at 5000 cm^-1, half an atmosphere
    and 150 K: there such a line is still pseudo-Voigt and its Gaussian cut-off exceeds the window);
(d) far calls of 1, 63, 64, 65 and 129 records (a lone partial chunk, a full one, full chunks followed by a partial one),
    against the all-direct kernel inside the bound and bit for bit against "accum_reach_skip" 0.

Every cell first asserts on the host (K1's formulas on the oracle's line quantities, scripts/far_gauss_model.py) that it
holds what it is meant to hold.
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO, point_tolerance, rel_err_points
from pyrad_amd import synthetic

pytestmark = pytest.mark.gpu

RMIN, RMAX, RES = 1000.0, 1008.192, 0.001
SPAN = 256
FAR_POINTS = 3 * 128          # the series takes a record from 3 half-spans of the span centre on (4 in the 16-point build)


def _load_model():
    spec = importlib.util.spec_from_file_location("far_gauss_model", os.path.join(REPO, "scripts", "far_gauss_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


model = _load_model()


@pytest.fixture(scope="module")
def ctx():
    from pyrad_amd import _native as nat
    c = nat.Context(0)
    yield c
    c.close()


def make_cell(species, conc, T, P, lines, rmin=RMIN):
    from oracle import pyrad_oracle as orc
    grid = orc.layer_grid(P, rmin, rmin + (RMAX - RMIN), RES, False)
    assert 8191 <= grid["n_work"] <= 8192 and grid["resolution"] == RES
    lines = orc.select_window(lines, grid["eff_min"], grid["eff_max"])
    sp = synthetic.SPECIES[species]
    idx, dgi = model.cell_records(lines, T, P, conc, sp["molmass"], grid)
    return dict(species=species, conc=conc, T=T, P=P, sp=sp, grid=grid, lines=lines, idx=idx, dgi=dgi, H=grid["W"] - 2)


def placed_lines(idx, sw, gamma, n_air=0.7, rmin=RMIN):
    """lines at the given centre indices (the middle of a grid cell, so the index is exact)"""
    idx = np.asarray(idx, dtype=np.float64)
    n = len(idx)
    lines = {
        "nu": rmin + (idx + 0.5) * RES,
        "sw": np.broadcast_to(np.asarray(sw, dtype=np.float64), (n,)),
        "a": np.full(n, 1.0),
        "gamma_air": np.broadcast_to(np.asarray(gamma, dtype=np.float64), (n,)),
        "gamma_self": np.broadcast_to(np.asarray(gamma, dtype=np.float64), (n,)),
        "n_air": np.full(n, n_air),
        "delta_air": np.zeros(n),
        "elower": np.linspace(100.0, 1200.0, n),
    }
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in lines.items()}


def far_counts(c):
    """per span: interior records at least FAR_POINTS + 128 points left / right of the span (far in either build)"""
    idx, H, n = c["idx"], c["H"], c["grid"]["n_work"]
    left, right = [], []
    for wlo in range(0, n, SPAN):
        whi = min(wlo + SPAN - 1, n - 1)
        interior = (idx >= whi - H) & (idx <= wlo + H)
        left.append(int((interior & (idx <= wlo + 127 - FAR_POINTS - 128)).sum()))
        right.append(int((interior & (idx >= wlo + 128 + FAR_POINTS + 128)).sum()))
    return np.array(left), np.array(right)


def device_xsec(ctx, c, variant, runs=0, skip=1, LS=1):
    """the cell through Context.xsec_accumulate; variant 5 on the far-field kernel's shapes with 4 points per lane"""
    from pyrad_amd import _native as nat, engine
    iso = nat.IsoParams(float(c["T"]), float(c["P"]), float(c["conc"]), c["sp"]["molmass"],
                        synthetic.q_value(c["species"], c["T"]), c["sp"]["q296"])
    ctx.set_option("accum_variant", variant)
    ctx.set_option("accum_gauss_run", runs)
    ctx.set_option("accum_reach_skip", skip)
    if variant == 5:
        ctx.set_option("accum_points_per_lane", 4)
        ctx.set_option("accum_line_split", LS)
    try:
        return ctx.xsec_accumulate(c["lines"], iso, engine.native_grid(c["grid"]))
    finally:
        ctx.set_option("accum_variant", 5)
        ctx.set_option("accum_gauss_run", 0)
        ctx.set_option("accum_reach_skip", 1)
        ctx.set_option("accum_points_per_lane", 0)
        ctx.set_option("accum_line_split", 0)


def assert_skip_changes_nothing(ctx, c, shapes=((16, 1), (32, 1), (16, 2))):
    """accum_reach_skip 0 against 1, bit for bit; -> the last (runs 32 where asked) result with the bound in use"""
    out = None
    for runs, LS in shapes:
        on, counts_on = device_xsec(ctx, c, 5, runs, 1, LS)
        off, counts_off = device_xsec(ctx, c, 5, runs, 0, LS)
        assert np.all(np.isfinite(on)) and np.any(on > 0)
        assert tuple(counts_on) == tuple(counts_off)
        assert np.array_equal(on, off), (runs, LS, int(np.count_nonzero(on != off)))
        if LS == 1:
            out = on
    return out


def assert_inside_bound(c, xs, direct):
    nu = c["grid"]["range_min"] + np.arange(c["grid"]["n_work"]) * RES
    tol = point_tolerance(nu, c["T"], c["grid"]["dfc"])
    e = rel_err_points(xs, direct, floor=float(np.max(np.abs(direct))) * 1e-250)
    print("against the all-direct kernel: %.3g (bound %.3g)" % (float(e.max()), float(tol.min())))
    assert np.all(e <= tol), float(e.max())


# ---- (a) ------------------------------------------------------------------------------------------------------------
def cell_a():
    from oracle import pyrad_oracle as orc
    g = orc.layer_grid(1013.25, RMIN, RMAX, RES, False)
    return make_cell("co2", 400e-6, 296, 1013.25, synthetic.make_lines(21, 600, g["eff_min"], g["eff_max"]))


def test_reach_skip_per_list_step(ctx):
    c = cell_a()
    assert c["H"] == 4998 and 500 <= len(c["idx"]) <= 600
    left, right = far_counts(c)
    assert int(((left > 0) & (right > 0)).sum()) > len(left) // 2          # far chunks on both sides of most spans
    assert c["dgi"].max() < c["H"] - SPAN                                   # and chunks beyond every cut-off: the bound skips
    assert_skip_changes_nothing(ctx, c)


def test_reach_skip_merged_step(ctx):
    """the list dealt to three species' lists, through the merged layer step: every output array"""
    from pyrad_amd import engine
    from oracle import pyrad_oracle as orc
    T, P = 296, 1013.25
    g = orc.layer_grid(P, RMIN, RMAX, RES, False)
    lines = synthetic.make_lines(21, 600, g["eff_min"], g["eff_max"])
    parts = [{k: np.ascontiguousarray(v[i::3]) for k, v in lines.items()} for i in range(3)]
    names = (("co2", 400e-6), ("h2o", 0.01), ("ch4", 1.8e-6))
    mols = [dict(conc=cc, isotopologues=[dict(lines=p, molmass=synthetic.SPECIES[s]["molmass"], q_T=synthetic.q_value(s, T),
                                              q296=synthetic.SPECIES[s]["q296"])]) for p, (s, cc) in zip(parts, names)]
    L = engine.ResidentLayer(ctx, 10.0, T, P, RMIN, RMAX, mols, RES, False)
    try:
        ctx.set_option("accum_points_per_lane", 4)
        ctx.set_option("accum_line_split", 1)
        for runs in (16, 32):
            ctx.set_option("accum_gauss_run", runs)
            got = {}
            for skip in (1, 0):
                ctx.set_option("accum_reach_skip", skip)
                for b in (L.abs_coef, L.trans, L.I_out):
                    b.fill(float("nan"))
                L.enqueue(surface_T=288.0, merged=True)
                got[skip] = L.results()
            assert sorted(got[1]) == ["abs_coef", "transmission", "transmittance"]
            for k in got[1]:
                assert np.all(np.isfinite(got[1][k])), (runs, k)
                assert np.array_equal(got[1][k], got[0][k]), (runs, k)
            assert np.any(got[1]["abs_coef"] > 0)
    finally:
        ctx.set_option("accum_reach_skip", 1)
        ctx.set_option("accum_gauss_run", 0)
        ctx.set_option("accum_points_per_lane", 0)
        ctx.set_option("accum_line_split", 0)
        L.free()


# ---- (b) ------------------------------------------------------------------------------------------------------------
def test_reach_skip_wide_profiles(ctx):
    from oracle import pyrad_oracle as orc
    P = 5 * 1013.25
    g = orc.layer_grid(P, RMIN, RMAX, RES, False)
    c = make_cell("ch4", 1.8e-6, 800, P, synthetic.make_lines(22, 1800, g["eff_min"], g["eff_max"]))
    pairs = model.far_gauss_pairs(c["idx"], c["dgi"], c["grid"]["n_work"])
    assert c["dgi"].max() > 8 * 128 and int(pairs["beyond"].sum()) > 100      # far records beyond the cap that still reach
    left, right = far_counts(c)
    assert left.max() > 64 and right.max() > 64
    xs = assert_skip_changes_nothing(ctx, c)
    direct, _ = device_xsec(ctx, c, 0)
    assert_inside_bound(c, xs, direct)


# ---- (c) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [255, 256], ids=["last-of-block", "first-of-block"])
def test_reach_skip_wide_record_at_block_boundary(ctx, pos):
    """Records 0 .. pos - 1 are narrow lines just left of the wide one (record `pos`); span S0's interior range starts exactly
    at the wide record, H - 255 points away - within its Gaussian cut-off (cold gas: a profile of about 500 points), far
    beyond everybody else's."""
    T, P, S0, rmin = 150, 506.625, 14, 5000.0
    H = 2498
    whi = S0 * SPAN + SPAN - 1
    cw = whi - H
    idx = np.concatenate([cw - 2 * np.arange(pos, 0, -1), [cw], cw + 300 + 67 * np.arange(100)])
    sw = np.full(len(idx), 1e-22)
    sw[pos] = 1e-19
    gamma = np.full(len(idx), 0.01)
    gamma[pos] = 0.5
    c = make_cell("ch4", 1.8e-6, T, P, placed_lines(idx, sw, gamma, n_air=1.0, rmin=rmin), rmin=rmin)
    assert c["H"] == H and np.array_equal(c["idx"], idx)
    assert int((c["idx"] < whi - H).sum()) == pos                      # span S0: the interior range starts at record `pos`
    assert c["dgi"][pos] > H - SPAN + 1 + 200                          # ... whose Gaussian part reaches the span
    assert np.delete(c["dgi"], pos).max() < FAR_POINTS - 128           # no other record's part reaches any span as a far record
    assert_skip_changes_nothing(ctx, c, shapes=((16, 1), (32, 1)))


# ---- (d) ------------------------------------------------------------------------------------------------------------
_direct_d = {}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_far_call_lengths(ctx, n):
    """n records left of spans 4 .. 20 and n records right of spans 11 .. 27, nothing else: the far calls of spans 11 .. 20
    hold exactly n records on either side.  Profiles of about 100 points, cut-offs of about 600: spans 4 and 27, 385 points
    from the nearest record, are within reach of a partial chunk's records."""
    idx = np.concatenate([640 - n + np.arange(n), 7552 + np.arange(n)])
    sw = 10.0 ** np.linspace(-22.0, -20.0, len(idx))
    c = make_cell("ch4", 1.8e-6, 296, 1013.25, placed_lines(idx, sw, 0.10))
    assert np.array_equal(c["idx"], idx)
    left, right = far_counts(c)
    assert np.all(left[4:21] == n) and np.all(right[11:28] == n)
    assert c["dgi"].min() > 400                                         # spans 4 and 27 are within reach
    xs = assert_skip_changes_nothing(ctx, c)
    direct, _ = device_xsec(ctx, c, 0)
    assert_inside_bound(c, xs, direct)
