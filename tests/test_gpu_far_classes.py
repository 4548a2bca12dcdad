"""GPU: the far-field series' distance classes (`kFarClassExact`, one class per distinct term count) and the edge series'
term count from the same table (K2), against the plain-C oracle at the per-point bound of tests/test_gpu_whole_spectrum.py.

A chunk of 64 far lines is classed by its NEAREST line (`far_chunk`: a descent generated from the table, farthest first,
that leaves at the stops of `LBL_FAR_STOPS` and takes the count of the table class of the stop it leaves at); a job's edge
series takes the count of the class of `H - 32 R`.  A table row or a stop that no chunk of a test ever met would hide a
wrong count, so every cell first restates the kernel's rule in NumPy over its own line positions (`chunk_classes`: the
span's far ranges as `wave_line_ranges_far` bounds them, chunks of 64 as `far_field_lines` forms them,
`dmin2 = 2 |c - xc|` of a chunk's nearest line against `2 d 32 R`) and asserts that every class of the table and every
stop of the build occurs.  The histograms and the largest relative error are printed.

(a) MAIN: a one-atmosphere cell (window 5,000 points, H = 4,998) on 12,288 points = 48 spans, 3 x 1,170 seeded lines of
    CO2, H2O and CH4 spread over the grid and 5 cm^-1 on either side (0.16 lines per point: pseudo-Voigt profiles, Gaussian
    runs, about 80 edge lines per interior span).  Interior spans see far chunks at every distance from 3 to 38 half-spans
    on both sides, and the edge lines are H - 128 = 4,870 points = 38 half-spans away: the merged step takes
    `series_edges` with 11 terms.  Merged and per-list steps, the 32-run build (`<4, 1, 38, 32>`, classes from 3
    half-spans) and the 16-run build (`<4, *, 30, 16>`, classes from 4), and the 16-run build with two waves per span
    (`accum_line_split` 2: whole far chunks are dealt to the waves, the class is per chunk there too).
(b) FEW: twelve lines on the same grid - no span has enough edge lines for the series' cost rule: `skew_edges`.
(c) SHORT: a window of 1,000 points (H = 998 < 8 half-spans + 128): the edge series is not entered whatever the count,
    and the far chunks are all in the four nearest classes.

Two runs of every shape are bit-identical.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import REPO, point_tolerance, rel_err_points
from pyrad_amd import synthetic

pytestmark = pytest.mark.gpu

RMIN, RMAX, RES = 1000.0, 1012.288, 0.001
SPAN, HALF = 256, 128            # R = 4: spans of 256 points, half-spans of 128
EDGE_MIN = 8                     # half-spans from which the edge series is entered (FF_EDGE_MIN)
SPECIES = (("co2", 400e-6), ("h2o", 0.01), ("ch4", 1.8e-6))
FIRST = {32: 0, 16: 1}           # Gaussian-run build -> its first row of the table (series from 3 / from 4 half-spans)


def _load_model():
    spec = importlib.util.spec_from_file_location("far_gauss_model", os.path.join(REPO, "scripts", "far_gauss_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


model = _load_model()


def table():
    from pyrad_amd import _native
    with open(os.path.join(_native.CSRC, "lbl_kernels.hip")) as fh:
        m = re.search(r"constexpr int kFarClassExact\[(\d+)\]\[2\] = \{(.*)\};", fh.read())
    pairs = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", m.group(2))]
    assert len(pairs) == int(m.group(1))
    return pairs


def stops():
    from pyrad_amd import _native
    with open(os.path.join(_native.CSRC, "lbl_kernels.hip")) as fh:
        m = re.search(r"#define LBL_FAR_STOPS \{([\d, ]+)\}", fh.read())
    return [int(x) for x in m.group(1).split(",")]


def span_ranges(idx, n_work, H, near):
    """per span: (wlo, iA, iB, iN1, iN2, iC, iD) as wave_line_ranges_far bounds them; near: the build's first class"""
    out = []
    for wlo in range(0, n_work, SPAN):
        whi = min(wlo + SPAN - 1, n_work - 1)
        iA, iB, iC, iD = (int(np.searchsorted(idx, t, "left")) for t in (wlo - H, whi - H, wlo + H + 1, whi + H + 1))
        if whi - H >= wlo + H + 1:
            iB = iC = iD
        iN1 = min(max(int(np.searchsorted(idx, wlo + HALF - near * HALF, "left")), iB), iC)
        iN2 = min(max(int(np.searchsorted(idx, wlo + HALF + near * HALF, "left")), iN1), iC)
        out.append((wlo, iA, iB, iN1, iN2, iC, iD))
    return out


def chunk_classes(idx, n_work, H, first):
    """histograms of the far chunks of every span (far_field_lines, far_chunk) over the table's rows and over the stops"""
    pairs, st = table(), stops()
    hist, hist_stop = np.zeros(len(pairs), np.int64), np.zeros(len(st), np.int64)
    for wlo, _, iB, iN1, iN2, iC, _ in span_ranges(idx, n_work, H, pairs[first][0]):
        for m0, m1 in ((iB, iN1), (iN2, iC)):
            for c0 in range(m0, m1, 64):
                ca, cb = int(idx[c0]), int(idx[min(c0 + 64, m1) - 1])
                dmin2 = min(abs(2 * (ca - wlo) - (SPAN - 1)), abs(2 * (cb - wlo) - (SPAN - 1)))
                assert dmin2 >= 2 * pairs[first][0] * HALF
                row = first
                while row + 1 < len(pairs) and dmin2 >= 2 * pairs[row + 1][0] * HALF:
                    row += 1
                hist[row] += 1
                hist_stop[[i for i, d in enumerate(st) if dmin2 >= 2 * d * HALF][-1]] += 1
    return hist, hist_stop


def edge_rule(idx, n_work, H):
    """-> (the edge series' term count for this window or None where it is not entered, edge lines per span)"""
    pairs = table()
    dmin = H - HALF
    nte = None
    if dmin >= EDGE_MIN * HALF:
        nte = [nt for d, nt in pairs if d >= EDGE_MIN and dmin >= d * HALF][-1]
    n_edge = np.array([(iB - iA) + (iD - iC) for _, iA, iB, _, _, iC, iD in span_ranges(idx, n_work, H, 4)])
    return nte, n_edge


@pytest.fixture(scope="module")
def ctx():
    from pyrad_amd import _native as nat
    c = nat.Context(0)
    yield c
    c.close()


_cells = {}


def cell(name):
    """grid, line lists, merged record positions and the oracle's cross sections and absorption coefficient (computed once)"""
    if name in _cells:
        return _cells[name]
    from oracle import c_oracle, pyrad_oracle as orc
    c_oracle.load()
    T = 296
    P = 202.65 if name == "short" else 1013.25
    g = orc.layer_grid(P, RMIN, RMAX, RES, False)
    assert 12287 <= g["n_work"] <= 12288 and g["resolution"] == RES
    per_list = {"main": ((31, 1170), (32, 1170), (33, 1160)), "few": ((34, 12),), "short": ((35, 700), (36, 700), (37, 600))}[name]
    mols, idx, xs_ref = [], [], []
    k_ref = np.zeros(g["n_base"])
    for (s, conc), (seed, n) in zip(SPECIES, per_list):
        sp = synthetic.SPECIES[s]
        lines = synthetic.make_lines(seed, n, g["eff_min"], g["eff_max"])
        q_T = synthetic.q_value(s, T)
        mols.append(dict(conc=conc, species=s, isotopologues=[dict(lines=lines, molmass=sp["molmass"], q_T=q_T, q296=sp["q296"])]))
        idx.append(model.cell_records(lines, T, P, conc, sp["molmass"], g)[0])
        xs = c_oracle.create_cross_section_work(lines, T, P, conc, sp["molmass"], q_T, sp["q296"], g)[0]
        xs_ref.append(xs)
        k_ref = k_ref + orc.abs_coef(np.zeros(g["n_base"]) + xs, conc, P, T)
    nu = orc.x_axis(RMIN, RMAX, RES)
    _cells[name] = dict(T=T, P=P, grid=g, mols=mols, H=g["W"] - 2, idx=np.sort(np.concatenate(idx)), idx_lists=idx,
                        xs_ref=xs_ref, k_ref=k_ref, tol=point_tolerance(nu, T, g["dfc"]))
    return _cells[name]


def worst(tag, got, ref, tol):
    e = rel_err_points(got, ref)
    i = int(np.argmax(e / tol))
    print("%s: max rel err %.3e (point %d of %d, tolerance there %.1e)" % (tag, float(e.max()), i, e.size, tol[i]))
    assert np.all(e <= tol), (tag, float(e.max()), i)


def layer_steps(ctx, c, runs, LS, steps=("merged", "per-list")):
    """the cell through the layer step(s) on the far-field kernel with 4 points per lane -> {step: abs_coef}, run twice"""
    from pyrad_amd import engine
    L = engine.ResidentLayer(ctx, 10.0, c["T"], c["P"], RMIN, RMAX, c["mols"], RES, False)
    out = {}
    try:
        ctx.set_option("accum_points_per_lane", 4)
        ctx.set_option("accum_line_split", LS)
        ctx.set_option("accum_gauss_run", runs)
        for step in steps:
            got = []
            for _ in range(2):
                for b in (L.abs_coef, L.trans, L.I_out):
                    b.fill(float("nan"))
                L.enqueue(surface_T=288.0, merged=(step == "merged"))
                got.append(L.results()["abs_coef"])
            assert np.all(np.isfinite(got[0])) and np.any(got[0] > 0)
            assert np.array_equal(got[0], got[1]), (step, runs, LS)                 # reruns are bit-identical
            out[step] = got[0]
    finally:
        ctx.set_option("accum_points_per_lane", 0)
        ctx.set_option("accum_line_split", 0)
        ctx.set_option("accum_gauss_run", 0)
        L.free()
    return out


def report_classes(tag, hists, first):
    pairs, st = table(), stops()
    hist, hist_stop = hists
    print("%s: far chunks per class %s" % (tag, ", ".join("%d:%d terms x %d" % (d, nt, n) for (d, nt), n in zip(pairs, hist))))
    print("%s: far chunks per stop %s" % (tag, ", ".join("%d x %d" % (d, n) for d, n in zip(st, hist_stop))))
    assert np.all(hist[first:] > 0), (tag, hist.tolist())                            # every row of the build occurs
    assert np.all(hist[:first] == 0)
    assert np.all(hist_stop[first:] > 0) and np.all(hist_stop[:first] == 0), (tag, hist_stop.tolist())


# ---- (a) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("runs,LS", [(32, 1), (16, 1), (16, 2)], ids=["runs32", "runs16", "runs16-split2"])
def test_every_class_and_the_eleven_term_edge_series(ctx, runs, LS):
    c = cell("main")
    pairs = table()
    assert c["H"] == 4998
    # what the shape holds, on the host: every class of the build among the merged job's far chunks (the three lists' own,
    # shorter calls - the per-list step - are reported only), the edge series with the table's last count on the merged job
    report_classes("merged, %d-point runs" % runs, chunk_classes(c["idx"], c["grid"]["n_work"], c["H"], FIRST[runs]), FIRST[runs])
    per_list = sum(chunk_classes(i, c["grid"]["n_work"], c["H"], FIRST[runs])[0] for i in c["idx_lists"])
    print("per-list, %d-point runs: far chunks per class %s" % (runs, per_list.tolist()))
    nte, n_edge = edge_rule(c["idx"], c["grid"]["n_work"], c["H"])
    assert nte == pairs[-1][1] == 11 and c["H"] - HALF >= pairs[-1][0] * HALF
    taken = int((n_edge * 21 >= 52 * nte + 250).sum())
    print("edge series: %d terms, taken on %d of %d spans (edge lines per span %d .. %d)" % (nte, taken, len(n_edge), n_edge.min(), n_edge.max()))
    assert n_edge.min() >= 39 and taken == len(n_edge)
    got = layer_steps(ctx, c, runs, LS)
    for step in ("merged", "per-list"):
        worst("main %s (Gaussian runs: %d, waves per span: %d) abs_coef" % (step, runs, LS), got[step], c["k_ref"], c["tol"])


# ---- (b) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("runs", [32, 16])
def test_few_lines_keep_the_skewed_edge_walk(ctx, runs):
    from pyrad_amd import _native as nat, engine
    c = cell("few")
    nte, n_edge = edge_rule(c["idx"], c["grid"]["n_work"], c["H"])
    assert nte == 11 and np.all(n_edge * 21 < 52 * nte + 250) and n_edge.max() > 0
    assert chunk_classes(c["idx"], c["grid"]["n_work"], c["H"], FIRST[runs])[0].sum() > 0        # (partial chunks of a few lines)
    m = c["mols"][0]
    iso = m["isotopologues"][0]
    p = nat.IsoParams(float(c["T"]), float(c["P"]), float(m["conc"]), iso["molmass"], iso["q_T"], iso["q296"])
    ctx.set_option("accum_variant", 5)
    ctx.set_option("accum_points_per_lane", 4)
    ctx.set_option("accum_line_split", 1)
    ctx.set_option("accum_gauss_run", runs)
    try:
        a, _ = ctx.xsec_accumulate(iso["lines"], p, engine.native_grid(c["grid"]))
        b, _ = ctx.xsec_accumulate(iso["lines"], p, engine.native_grid(c["grid"]))
    finally:
        ctx.set_option("accum_points_per_lane", 0)
        ctx.set_option("accum_line_split", 0)
        ctx.set_option("accum_gauss_run", 0)
    assert np.array_equal(a, b)
    worst("few lines (Gaussian runs: %d) xsec" % runs, a, c["xs_ref"][0], c["tol"])


# ---- (c) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("runs", [32, 16])
def test_short_window_does_not_enter_the_edge_series(ctx, runs):
    c = cell("short")
    pairs = table()
    assert 640 <= c["H"] == 998 < EDGE_MIN * HALF + HALF
    nte, n_edge = edge_rule(c["idx"], c["grid"]["n_work"], c["H"])
    assert nte is None and int((n_edge * 21 >= 52 * pairs[-1][1] + 250).sum()) > 0            # enough lines, too near
    hist = chunk_classes(c["idx"], c["grid"]["n_work"], c["H"], FIRST[runs])[0]
    far = [i for i, (d, _) in enumerate(pairs) if d * HALF <= c["H"] - HALF]                  # classes inside the window
    print("short window, %d-point runs: far chunks per class %s" % (runs, hist.tolist()))
    assert hist[FIRST[runs]] > 0 and hist[FIRST[runs] + 1:].sum() > 0 and np.all(hist[far[-1] + 1:] == 0)
    got = layer_steps(ctx, c, runs, 1, steps=("merged",))
    worst("short window merged (Gaussian runs: %d) abs_coef" % runs, got["merged"], c["k_ref"], c["tol"])
