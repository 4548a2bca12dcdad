"""CPU: the G13 fixture (mutator chains recorded from the reference's own Layer / Molecule / Atmosphere objects,
tests/golden/make_golden.py g13) is consistent with its own recorded state.

For every recorded step the absorption coefficient is rebuilt with the project's oracle from what the step recorded: the lines
strictly inside the RECORDED effective window (which changePressure leaves alone, cls:745-752), the recorded T, P, resolution,
range and concentrations.  That holds the fixture to the oracle at the tolerance of tests/test_oracle_golden.py without a GPU,
and shows that the two cases the chains were written for are in it: a window kept too narrow after the pressure went up, and
lines far outside a grid whose reach shrank when the pressure went down."""
import json

import numpy as np
import pytest

from conftest import load_golden, rel_err
from g13_chains import Chain, LAYER_CHAINS, SEEDED_CHAINS, COLUMN_CHAINS
from oracle import pyrad_oracle as orc
from pyrad_amd import synthetic

TOL = 1e-12          # tests/test_oracle_golden.py: the restatement evaluates the reference's expressions in the reference's order


def oracle_abs_coef(chain, step, window=None):
    s = chain.scalars[step]
    base = chain.build["base_resolution"]
    T, P = int(s["T"]), s["P"]
    rmin, rmax = s["rangeMin"], s["rangeMax"]
    lo, hi = window if window is not None else (s["effectiveRangeMin"], s["effectiveRangeMax"])
    grid = dict(dfc=s["distanceFromCenter"], eff_min=lo, eff_max=hi, resolution=s["resolution"], base_resolution=base,
                n_base=int((rmax - rmin) / base), n_work=int((rmax - rmin) / s["resolution"]),
                W=len(np.arange(0, s["distanceFromCenter"], s["resolution"])), range_min=rmin, range_max=rmax)
    k = np.zeros(grid["n_base"])
    per_molecule, n_lines = {}, []
    for m, species in chain.species():
        sp = synthetic.SPECIES[species]
        conc = chain.concentration[step][m]
        sel = orc.select_window(chain.lines[species], lo, hi)
        n_lines.append(len(sel["nu"]))
        xs, _ = orc.create_cross_section(sel, T, P, conc, sp["molmass"], synthetic.q_value(species, T), sp["q296"], grid)
        per_molecule[m] = per_molecule.get(m, np.zeros(grid["n_base"])) + xs                 # cls:566-571
    for m in sorted(per_molecule):
        k = k + orc.abs_coef(per_molecule[m], chain.concentration[step][m], P, T)            # cls:709-712
    return k, per_molecule, n_lines, grid


@pytest.fixture(scope="module")
def g13():
    return load_golden("G13_mutator_chains")


def test_the_fixture_holds_the_chains_the_tests_name(g13):
    assert json.loads(str(g13["layer_chains_json"])) == LAYER_CHAINS
    assert json.loads(str(g13["column_chains_json"])) == COLUMN_CHAINS
    for name in LAYER_CHAINS:
        assert len(Chain(g13, "layer." + name).ops) == 12
    for name in COLUMN_CHAINS:
        assert len(Chain(g13, "column." + name).ops) == 8


@pytest.mark.parametrize("name", LAYER_CHAINS)
def test_every_recorded_step_is_what_the_oracle_makes_of_the_recorded_state(g13, name):
    chain = Chain(g13, "layer." + name)
    for step in range(12):
        k, per_molecule, n_lines, _ = oracle_abs_coef(chain, step)
        assert n_lines == list(chain.lengths[step]), (name, step)                 # the lines of the RECORDED window
        assert rel_err(k, chain.get("s%d.abs_coef" % step, step)) <= TOL, (name, step)
        assert rel_err(per_molecule[0], chain.get("s%d.mol0_xsec" % step)) <= TOL, (name, step)
    s = chain.scalars[11]
    tr = orc.transmittance(k, s["depth"])
    assert rel_err(tr, chain.get("end.transmittance")) <= TOL
    x = orc.x_axis(s["rangeMin"], s["rangeMax"], chain.build["base_resolution"])
    spec = orc.transmission(tr, orc.planckWavenumber(x, 288), orc.planckWavenumber(x, int(s["T"])))
    assert rel_err(spec, chain.get("end.transmission")) <= TOL


def test_the_layer_cross_section_is_the_first_one_for_the_whole_chain(g13):
    """getCrossSection(layer) is computed once and nothing resets it (cls:39): every later step repeats step 0's array, even
    after the range has moved and the array no longer has the layer's length."""
    for name in LAYER_CHAINS:
        chain = Chain(g13, "layer." + name)
        first = chain.stored_key("s0.layer_xsec")
        assert all(chain.stored_key("s%d.layer_xsec" % s) == first for s in range(12)), name
        assert any(o["op"] == "changeRange" for o in chain.ops), name


def test_up_chain_keeps_the_narrow_window_after_the_pressure_rise(g13):
    chain = Chain(g13, "layer.up")
    assert chain.build["P"] == 300.0 and chain.ops[0] == dict(op="changePressure", args=[1013.25])
    s = chain.scalars[0]
    assert s["distanceFromCenter"] == 5.0
    assert (s["effectiveRangeMin"], s["effectiveRangeMax"]) == (s["rangeMin"] - 300.0 / 1013.25 * 5, s["rangeMax"] + 300.0 / 1013.25 * 5)
    fresh, _, n_fresh, _ = oracle_abs_coef(chain, 0, window=(s["rangeMin"] - 5.0, s["rangeMax"] + 5.0))
    assert sum(n_fresh) > sum(chain.lengths[0])
    stale = chain.get("s0.abs_coef", 0)
    worst = float(np.max(np.abs(stale - fresh) / fresh))
    assert worst > 0.01, worst                          # (measured when the fixture was made: see DESIGN.md)
    healed = chain.scalars[2]                           # the changeRange of step 2 refreshes the window
    assert (healed["effectiveRangeMin"], healed["effectiveRangeMax"]) == (healed["rangeMin"] - 5.0, healed["rangeMax"] + 5.0)


def test_down_chain_hands_the_kernels_lines_far_outside_the_grid(g13):
    chain = Chain(g13, "layer.down")
    assert chain.build["P"] == 10132.5 and chain.ops[0] == dict(op="changePressure", args=[50.0])
    s = chain.scalars[0]
    _, _, n_lines, grid = oracle_abs_coef(chain, 0)
    assert grid["W"] == 25 and s["resolution"] == 0.01
    assert s["effectiveRangeMax"] - s["rangeMax"] == pytest.approx(50.0)           # the window of 10132.5 mbar
    sel = orc.select_window(chain.lines["co2"], s["effectiveRangeMin"], s["effectiveRangeMax"])
    index = ((sel["nu"] - s["rangeMin"]) / s["resolution"]).astype(np.int64)
    outside = np.maximum(-index, index - (grid["n_work"] - 1))
    assert int(outside.max()) > 100 * grid["W"] and n_lines == list(chain.lengths[0])


@pytest.mark.parametrize("name", SEEDED_CHAINS)
def test_seeded_chains_take_the_pressure_to_both_sides_of_the_start(g13, name):
    """at an unscripted position the pressure rises above the one the chain started at while the window is still the one of a
    lower pressure (no changeRange since: narrower than the lines' reach, and fewer lines than a fresh window holds), and at
    another it falls below the start"""
    chain = Chain(g13, "layer." + name)
    P0 = chain.build["P"]
    rises = [i for i, (op, s) in enumerate(zip(chain.ops, chain.scalars))
             if op["op"] == "changePressure" and s["P"] > P0 and s["effectiveRangeMax"] - s["rangeMax"] < s["distanceFromCenter"]]
    assert rises and any(s["P"] < P0 for s in chain.scalars), [s["P"] for s in chain.scalars]
    step = rises[0]
    s = chain.scalars[step]
    fresh, _, n_fresh, _ = oracle_abs_coef(chain, step, window=(s["rangeMin"] - s["distanceFromCenter"], s["rangeMax"] + s["distanceFromCenter"]))
    assert sum(n_fresh) > sum(chain.lengths[step])
    assert not np.array_equal(fresh, chain.get("s%d.abs_coef" % step, step))


def test_fine_chain_switches_the_resolution(g13):
    chain = Chain(g13, "layer.fine")
    assert chain.build["base_resolution"] == 0.001
    assert {s["resolution"] for s in chain.scalars} == {0.01, 0.001}
    assert {s["P"] for s in chain.scalars} >= {1013.25, 101.0, 50.0}
