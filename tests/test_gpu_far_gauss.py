"""GPU: far lines whose Gaussian part still reaches the span (K2, the far-field kernel's production shape R = 4, unsplit).

A record at least 4 half-spans (512 points) from a span's centre takes its Lorentz term from the series; where K1's cut-off
says its Gaussian part still matters on the span, the records inside 8 half-spans are noted by the far loop and evaluated
by the near walk's transposed runs, the ones beyond keep the far loop's four-point pass.  Every case first counts on the
host (scripts/far_gauss_model.py, K1's formulas on the oracle's line quantities) how many (record, span) pairs of either
kind it holds and asserts the counts, so that a change of the synthetic generator cannot quietly empty it.  Then, with
16-point and 32-point runs, the changed shape (accum_points_per_lane 4, accum_line_split 1) and the line-split shape that
keeps the old path (accum_line_split 2) against the all-direct kernel (5e-14, the bound of
test_gpu_parity.test_far_field_random_against_direct_kernel) and the NumPy oracle (1e-11 with test_gpu_parity's floor);
regime counts equal; reruns bit-identical.
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO, rel_err
from pyrad_amd import synthetic

pytestmark = pytest.mark.gpu

RTOL_DIRECT = 5e-14
RTOL_ORACLE = 1e-11
FLOOR_REL = 1e-250


def _load_model():
    spec = importlib.util.spec_from_file_location("far_gauss_model", os.path.join(REPO, "scripts", "far_gauss_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


model = _load_model()


def hand_placed_lines(rmin, res):
    """Twelve wide lines (gamma 0.10 at 2 atm: a = 200 points, cut-off about 1,200) in two groups with nothing between them.
    Span 4 (points 1024-1279) has no near line and far Gaussian records on its left only, span 8 (2048-2303) on its right
    only.  Centres 383 / 384: the first far and the last near record of span 3 (768 - 385, 768 - 384) and the first record
    beyond and the last inside the cap of span 5 (1280 - 897, 1280 - 896); 2943 / 2944 do the same on the right of spans 9
    (2304 + 639, + 640) and 7 (1792 + 1151, + 1152).  A centre sits in the middle of its grid cell, so its index is exact."""
    idx = np.array([-200, 290, 300, 310, 383, 384, 2943, 2944, 3000, 3010, 3020, 3900], dtype=np.float64)
    n = len(idx)
    lines = {
        "nu": rmin + (idx + 0.5) * res,
        "sw": 10.0 ** np.linspace(-22.0, -20.0, n),
        "a": np.full(n, 1.0),
        "gamma_air": np.full(n, 0.10),
        "gamma_self": np.full(n, 0.10),
        "n_air": np.full(n, 0.7),
        "delta_air": np.zeros(n),
        "elower": np.linspace(100.0, 1200.0, n),
    }
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in lines.items()}


# name: (species, conc, T, P, rmin, rmax, lines (n, seed) or None for the hand-placed list, (pairs inside the cap, beyond))
CELLS = {
    "co2_2000": ("co2", 400e-6, 296, 1013.25, 1000, 1016, (2000, 11), (654, 0)),
    "co2_12000": ("co2", 400e-6, 296, 1013.25, 1000, 1016, (12000, 12), (4006, 0)),
    "ch4_2atm": ("ch4", 1.8e-6, 250, 2026.5, 2500, 2508, (800, 15), (847, 250)),
    "ch4_4atm": ("ch4", 1.8e-6, 296, 4053.0, 2500, 2516, (1500, 14), (1604, 2721)),
    "hand_placed": ("ch4", 1.8e-6, 296, 2026.5, 2500, 2504, None, None),
}
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from pyrad_amd import _native as nat
    c = nat.Context(0)
    yield c
    c.close()


def device_xsec(ctx, cell, variant, LS=None):
    """the cell through Context.xsec_accumulate; variant 5 with R = 4 and the given line split pinned, variant 3 as the
    library shapes it"""
    from pyrad_amd import _native as nat, engine
    c = cell
    iso = nat.IsoParams(float(c["T"]), float(c["P"]), float(c["conc"]), c["sp"]["molmass"],
                        synthetic.q_value(c["species"], c["T"]), c["sp"]["q296"])
    ctx.set_option("accum_variant", variant)
    if LS is not None:
        ctx.set_option("accum_points_per_lane", 4)
        ctx.set_option("accum_line_split", LS)
    try:
        return ctx.xsec_accumulate(c["lines"], iso, engine.native_grid(c["grid"]))
    finally:
        ctx.set_option("accum_variant", 5)
        ctx.set_option("accum_points_per_lane", 0)
        ctx.set_option("accum_line_split", 0)


def cell_of(name, ctx):
    """lines, grid, the host's count of the class, the oracle's and the all-direct kernel's cross sections: once per cell"""
    if name in _cache:
        return _cache[name]
    from oracle import pyrad_oracle as orc
    species, conc, T, P, rmin, rmax, gen, expect = CELLS[name]
    grid = orc.layer_grid(P, rmin, rmax, 0.001, False)
    if gen is None:
        lines = hand_placed_lines(rmin, grid["resolution"])
    else:
        lines = synthetic.make_lines(gen[1], gen[0], grid["eff_min"], grid["eff_max"])
    lines = orc.select_window(lines, grid["eff_min"], grid["eff_max"])
    sp = synthetic.SPECIES[species]
    idx, dgi = model.cell_records(lines, T, P, conc, sp["molmass"], grid)
    pairs = model.far_gauss_pairs(idx, dgi, grid["n_work"])
    ref, ref_counts = orc.create_cross_section(lines, T, P, conc, sp["molmass"], synthetic.q_value(species, T), sp["q296"], grid)
    c = dict(name=name, species=species, conc=conc, T=T, P=P, sp=sp, grid=grid, lines=lines, idx=idx, dgi=dgi, pairs=pairs,
             expect=expect, ref=ref, ref_counts=tuple(int(v) for v in ref_counts))
    c["direct"], c["direct_counts"] = device_xsec(ctx, c, 3)
    _cache[name] = c
    return c


def assert_precondition(c):
    p = c["pairs"]
    inside = int(p["inside_left"].sum() + p["inside_right"].sum())
    beyond = int(p["beyond"].sum())
    if c["expect"] is not None:
        assert (inside, beyond) == c["expect"], (c["name"], inside, beyond)
    both = int(((p["inside_left"] > 0) & (p["inside_right"] > 0)).sum())
    most = int((p["inside_left"] + p["inside_right"]).max())
    if c["name"] == "co2_2000":
        assert both >= 62 and len(p["near"]) == 63                    # the class on both sides of (almost) every span
    if c["name"] == "co2_12000":
        assert int(((p["inside_left"] + p["inside_right"]) > 64).sum()) >= 32 and most > 64      # the extension crosses chunks
    if c["name"] == "hand_placed":
        idx = c["idx"]
        assert np.array_equal(idx, [-199, 290, 300, 310, 383, 384, 2943, 2944, 3000, 3010, 3020, 3900])      # (-199.5 truncates to -199)
        assert c["dgi"].min() > 897                                   # 383 reaches span 5 (1280 - 383), 2944 span 7 (2944 - 2047)
        near, il, ir, by = p["near"], p["inside_left"], p["inside_right"], p["beyond"]
        # span 4: no near line, far Gaussian records on the left only; span 8: on the right only (the range is pure extension)
        assert (near[4], il[4], ir[4], by[4]) == (0, 5, 0, 0)
        assert (near[8], il[8], ir[8], by[8]) == (0, 0, 5, 0)
        # span 3: 383 is its first far record on the left (384 is near); span 9: 2944 on the right (2943 is near)
        assert (near[3], il[3]) == (1, 4) and (near[9], ir[9]) == (1, 4)
        # span 5: 384 is the last record inside the cap, 383 the first beyond; span 7: 2943 inside, 2944 beyond
        assert (il[5], by[5]) == (1, 4) and (ir[7], by[7]) == (1, 4)


def check_oracle(a, b):
    floor = float(np.max(np.abs(b))) * FLOOR_REL
    e = rel_err(a, b, floor=floor)
    assert e <= RTOL_ORACLE, e


@pytest.mark.parametrize("runs", [0, 16], ids=["runs:auto", "runs:16"])
@pytest.mark.parametrize("name", list(CELLS))
def test_far_gauss_cell(ctx, name, runs):
    c = cell_of(name, ctx)
    assert_precondition(c)
    assert c["direct_counts"] == c["ref_counts"]
    check_oracle(c["direct"], c["ref"])
    ctx.set_option("accum_gauss_run", runs)
    try:
        for LS in (1, 2):            # 1: the shape that routes the class through the near walk; 2: the untouched path
            xs, counts = device_xsec(ctx, c, 5, LS)
            e_direct = rel_err(xs, c["direct"])
            print("%s runs %d LS %d: against the all-direct kernel %.3g" % (name, runs, LS, e_direct))
            assert tuple(counts) == c["direct_counts"]
            assert np.all(np.isfinite(xs)) and np.all(xs >= 0)
            assert e_direct <= RTOL_DIRECT, (name, runs, LS, e_direct)
            check_oracle(xs, c["ref"])
            again, _ = device_xsec(ctx, c, 5, LS)
            assert np.array_equal(xs, again), (name, runs, LS)
    finally:
        ctx.set_option("accum_gauss_run", 0)


@pytest.mark.parametrize("runs", [0, 16], ids=["runs:auto", "runs:16"])
def test_far_gauss_merged_step(ctx, runs):
    """The first cell's list dealt to three species lists, through the merged layer step (one job over the merged records)
    on the changed shape, against the per-list step on the all-direct kernel."""
    from pyrad_amd import engine
    from oracle import pyrad_oracle as orc
    species, conc, T, P, rmin, rmax, gen, _ = CELLS["co2_2000"]
    grid = orc.layer_grid(P, rmin, rmax, 0.001, False)
    lines = synthetic.make_lines(gen[1], gen[0], grid["eff_min"], grid["eff_max"])
    parts = [{k: np.ascontiguousarray(v[i::3]) for k, v in lines.items()} for i in range(3)]
    names = (("co2", 400e-6), ("h2o", 0.01), ("ch4", 1.8e-6))
    # the class is still there once the lists carry their own species' widths
    recs = [model.cell_records(orc.select_window(p, grid["eff_min"], grid["eff_max"]), T, P, cc, synthetic.SPECIES[s]["molmass"], grid)
            for p, (s, cc) in zip(parts, names)]
    idx = np.concatenate([r[0] for r in recs]); dgi = np.concatenate([r[1] for r in recs])
    o = np.argsort(idx, kind="stable")
    pairs = model.far_gauss_pairs(idx[o], dgi[o], grid["n_work"])
    assert int(pairs["inside_left"].sum() + pairs["inside_right"].sum()) >= 500
    mols = [dict(conc=cc, isotopologues=[dict(lines=p, molmass=synthetic.SPECIES[s]["molmass"], q_T=synthetic.q_value(s, T),
                                              q296=synthetic.SPECIES[s]["q296"])]) for p, (s, cc) in zip(parts, names)]
    L = engine.ResidentLayer(ctx, 10.0, T, P, rmin, rmax, mols, 0.001, False)
    try:
        ctx.set_option("accum_variant", 3)
        L.enqueue(surface_T=288.0)
        ref = L.results()["abs_coef"]
        L.abs_coef.fill(float("nan"))
        ctx.set_option("accum_variant", 5)
        ctx.set_option("accum_gauss_run", runs)
        ctx.set_option("accum_points_per_lane", 4)
        ctx.set_option("accum_line_split", 1)
        L.enqueue(surface_T=288.0, merged=True)
        got = L.results()["abs_coef"]
        e = rel_err(got, ref)
        print("merged step runs %d: against the per-list all-direct sum %.3g" % (runs, e))
        assert np.all(np.isfinite(got)) and np.any(ref > 0)
        assert e <= RTOL_DIRECT, e
        L.enqueue(surface_T=288.0, merged=True)
        assert np.array_equal(L.results()["abs_coef"], got)
    finally:
        ctx.set_option("accum_variant", 5)
        ctx.set_option("accum_gauss_run", 0)
        ctx.set_option("accum_points_per_lane", 0)
        ctx.set_option("accum_line_split", 0)
        L.free()
