"""Reader of the G13 fixture (mutator chains recorded from the reference, tests/golden/make_golden.py g13), shared by
tests/test_mutator_chains_cpu.py and tests/test_gpu_mutator_chains.py."""
import json

from pyrad_amd import synthetic

LAYER_CHAINS = ["up", "down", "fine", "mix", "r0", "r1"]
SEEDED_CHAINS = ["r0", "r1"]
COLUMN_CHAINS = ["a", "b"]


class Chain:
    """One chain of the fixture: ``get(key)`` follows the aliases and the derived absorption coefficients."""

    def __init__(self, z, prefix):
        self.z, self.prefix = z, prefix
        self.alias = json.loads(str(z[prefix + ".alias_json"]))
        self.derived = json.loads(str(z[prefix + ".derived_json"]))
        self.ops = json.loads(str(z[prefix + ".ops_json"]))
        self.lines = {sp: {f: z["lines.%s.%s" % (key, f)] for f in synthetic.FIELDS}
                      for sp, key in json.loads(str(z[prefix + ".lines_json"])).items()}
        if prefix.startswith("layer."):
            self.build = json.loads(str(z[prefix + ".build_json"]))
            self.scalars = [dict(zip(json.loads(str(z["scalar_names_json"])), row)) for row in z[prefix + ".scalars"]]
            self.concentration = z[prefix + ".concentration"]
            self.lengths = z[prefix + ".lengths"]

    def stored_key(self, key):
        return self.alias.get(key, key)

    def get(self, key, step=None):
        if key in self.derived:            # one-molecule layer: cls:583 added to zeros (cls:709-711)
            s = self.scalars[step]
            return self.get(self.derived[key]) * self.concentration[step][0] * s["P"] / 1E4 / float(self.z["k_boltzmann"]) / s["T"]
        return self.z["%s.%s" % (self.prefix, self.stored_key(key))]

    def species(self):
        """[(molecule index, species key)] per isotopologue, in the layer's order, as the generator read them off the
        reference's objects"""
        return [(int(m), sp) for m, sp in json.loads(str(self.z[self.prefix + ".species_json"]))]
