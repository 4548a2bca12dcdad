"""GPU: pyrad_amd.model replays the mutator chains of the G13 fixture, which tests/golden/make_golden.py recorded from the
reference's own Layer / Molecule / Atmosphere objects, and is compared with the reference after EVERY operation.

tests/test_gpu_model.py compares a mutated object with a fresh object of the same build; a wrong invalidation shared by both
passes there.  Here the state carried from one call to the next is held to the reference itself:
  * the effective window that changePressure keeps and only changeRange refreshes (cls:734-752): too narrow after the pressure
    went up (chain "up": the absorption coefficient is far from a fresh layer's), too wide after it went down (chain "down":
    K1 / K2 receive lines thousands of grid points outside a grid with a 25-point reach);
  * the resolution switching between 0.01 and 0.001 under BASE_RESOLUTION 0.001 (chain "fine");
  * the four setters on three molecules, two isotopologues, a copy read at once (chain "mix"); seeded draws ("r0", "r1") in
    which the pressure rises above the start on a window still made for a lower pressure, and falls below it;
  * the layer's own cross section, computed once and never reset (cls:39), even after the range has moved;
  * the dirty flags of the layer, every molecule and every isotopologue before and after the getters;
  * the resident column handle of Atmosphere.transmission across eight operations on one live atmosphere.

Deliberate deviation that the chains keep out by construction:
Layer.returnCopy binds the copy's molecules to the NEW layer (the reference binds them to the old one, cls:539, 771), so a copy
is read immediately, while the old layer's window is the fresh one, and never mutated.

Worst relative error seen per chain on an MI355X: up 2.1e-14, down 4.5e-15, fine 2.4e-15, mix 1.1e-14, r0 6.6e-15, r1 1.7e-13,
columns 1.3e-15 (each test prints its own)."""
import json

import numpy as np
import pytest

from conftest import load_golden, rel_err
from g13_chains import Chain, LAYER_CHAINS, COLUMN_CHAINS

pytestmark = pytest.mark.gpu
RTOL = 1e-11          # tests/test_gpu_model.py, conftest.py: what the goldens are held to


@pytest.fixture(scope="module")
def g13():
    return load_golden("G13_mutator_chains")


@pytest.fixture()
def pyrad():
    from pyrad_amd import model, data, settings
    model.Layer.hasAtmosphere = False
    settings.set_resolution_multiplier(1)
    yield model
    settings.set_resolution_multiplier(1)
    data.set_source(None)


def use_lines(chain):
    from pyrad_amd import data
    data.set_source(data.synthetic_source({sp: {f: np.ascontiguousarray(v) for f, v in l.items()} for sp, l in chain.lines.items()}))


def add_molecules(layer, molecules):
    for species, depth, kind, value in molecules:
        layer.addMolecule(species, isotopeDepth=depth, **{kind: value})


def apply(layer, op):
    if op["op"].startswith("set"):
        getattr(layer[op["mol"]], op["op"])(*op["args"])
    else:
        getattr(layer, op["op"])(*op["args"])


def flags(layer):
    return [bool(layer.progressCrossSection)] + [bool(m.progressCrossSection) for m in layer] + \
        [bool(i.progressCrossSection) for m in layer for i in m]


def check_step(pyrad, chain, z, layer, tag, step, row, rec_prefix, worst):
    """One recorded state against ``layer``: flags before, the three getters in the recorded order, flags after, lengths,
    scalars and concentrations.  Returns the layer's cross section as read."""
    where = (chain.prefix, tag)
    assert flags(layer) == list(z[rec_prefix + ".flags_before"][row]), where
    k = np.array(pyrad.getAbsCoef(layer))
    layer_xs = np.array(pyrad.getCrossSection(layer))
    mol_xs = np.array(pyrad.getCrossSection(layer[0]))
    assert flags(layer) == list(z[rec_prefix + ".flags_after"][row]), where
    for name, got, want in (("abs_coef", k, chain.get(tag + ".abs_coef", step)), ("layer_xsec", layer_xs, chain.get(tag + ".layer_xsec")),
                            ("mol0_xsec", mol_xs, chain.get(tag + ".mol0_xsec"))):
        e = rel_err(got, want)
        worst[0] = max(worst[0], e)
        print("%s %s %s rel_err %.3g" % (chain.prefix, tag, name, e))
        assert e <= RTOL, (where, name, e)
    assert [len(i) for m in layer for i in m] == list(z[rec_prefix + ".lengths"][row]), where
    names = json.loads(str(z["scalar_names_json"]))
    assert [float(getattr(layer, s)) for s in names] == list(z[rec_prefix + ".scalars"][row]), where
    assert [float(m.concentration) for m in layer] == list(z[rec_prefix + ".concentration"][row]), where
    return layer_xs


@pytest.mark.parametrize("name", LAYER_CHAINS)
def test_layer_chain_follows_the_reference_after_every_operation(pyrad, g13, name):
    from pyrad_amd import settings
    chain = Chain(g13, "layer." + name)
    b = chain.build
    if b["base_resolution"] != 0.01:
        settings.set_resolution_multiplier(0.1)
        assert settings.BASE_RESOLUTION == b["base_resolution"]
    use_lines(chain)
    layer = pyrad.Layer(b["depth"], b["T"], b["P"], b["range_min"], b["range_max"], name=name)
    add_molecules(layer, b["molecules"])
    worst, seen, copies = [0.0], [], 0
    for step, op in enumerate(chain.ops):
        if op["op"] == "returnCopy":
            copy = layer.returnCopy()
            check_step(pyrad, chain, g13, copy, "s%d.copy" % step, step, copies, chain.prefix + ".copy", worst)
            copies += 1
        else:
            apply(layer, op)
        seen.append(check_step(pyrad, chain, g13, layer, "s%d" % step, step, step, chain.prefix, worst))
        # the IDENTITY of the stale cross section: the very array of the step the reference repeats, and of no other
        keys = [chain.stored_key("s%d.layer_xsec" % s) for s in range(step + 1)]
        for s in range(step):
            same = seen[s].shape == seen[step].shape and np.array_equal(seen[s], seen[step])
            assert same == (keys[s] == keys[step]), (name, step, s)
    spec = layer.transmission(layer.planck(288))
    tr = pyrad.getTransmittance(layer)
    for what, got, want in (("transmission", spec, chain.get("end.transmission")), ("transmittance", tr, chain.get("end.transmittance"))):
        e = rel_err(got, want)
        worst[0] = max(worst[0], e)
        assert e <= RTOL, (name, what, e)
    print("chain %s: worst relative error %.3g" % (name, worst[0]))


@pytest.mark.parametrize("name", COLUMN_CHAINS)
def test_column_chain_follows_the_reference_after_every_operation(pyrad, g13, name):
    """One live Atmosphere: Atmosphere.transmission after EVERY operation (the resident column handle lives across the chain),
    against the spectrum the reference's fold of Layer.transmission gave, and against the same fold on the same objects."""
    chain = Chain(g13, "column." + name)
    use_lines(chain)
    atm = pyrad.Atmosphere(name)
    for L in json.loads(str(g13[chain.prefix + ".layers_json"])):
        add_molecules(atm.addLayer(L["depth"], L["T"], L["P"], L["range_min"], L["range_max"]), L["molecules"])
    atm.transmission(surfaceTemperature=288)                                    # the handle exists before the first operation
    assert "_column_fast" in atm.__dict__
    worst = 0.0
    for step, op in enumerate(chain.ops):
        assert atm.__dict__.get("_column_fast") is not None, (name, step)         # (rebuilt by the call after a new grid or layer)
        handle = atm.__dict__["_column_fast"]["col"]
        if op["op"] == "addLayer":
            add_molecules(atm.addLayer(*op["args"]), op["molecules"])
        elif op["layer"] == "all":
            for layer in atm:
                apply(layer, op)
        else:
            apply(atm[op["layer"]], op)
        want = chain.get("s%d.spectrum" % step)
        got = np.array(atm.transmission(surfaceTemperature=288))
        # a new grid or another list of layers rebuilds the handle; every other operation goes THROUGH the one that is there
        # (the layer loop of the step before included: it must not have knocked it out)
        if op["op"] not in ("changeRange", "addLayer"):
            assert atm.__dict__["_column_fast"]["col"] is handle, (name, step, op)
        spec = atm[0].planck(288)
        for layer in atm:
            spec = layer.transmission(spec)
        e, e_loop = rel_err(got, want), rel_err(spec, want)
        worst = max(worst, e, e_loop)
        print("column %s step %d: resident %.3g, layer loop %.3g" % (name, step, e, e_loop))
        assert e <= RTOL and e_loop <= RTOL, (name, step, op, e, e_loop)
    print("column %s: worst relative error %.3g" % (name, worst))
