#!/usr/bin/env python3
"""Times Atmosphere.jacobians on the config-5 column (30 layers x 2.4e6 points, 3 molecules per layer, built as
scripts/flux_time.py builds it): calls with every absorption coefficient resident, with molecules=False and True, for 1 and
3 angles, beside fluxes() for comparison, and the first call after changeTemperature on one layer (its layer job, its
molecule jobs and the Jacobian kernels).  Each call returns host arrays, so the wall time of a call is device-synchronised.
Two warm-up calls, then the median of `--reps`.  Run on the GPU box; kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flux_time import column, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    atm, Ts = column()
    atm.transmission(surfaceTemperature=Ts)            # first call: uploads, schedules, every absorption coefficient resident
    atm.jacobians(surfaceTemperature=Ts)               # the molecule terms' first accumulate jobs
    res = {"layers": len(atm), "points": int(atm[0].xAxis.size), "molecule_terms": sum(len(L) for L in atm)}
    for angles in (1, 3):
        med, lo = timed(lambda: atm.fluxes(surfaceTemperature=Ts, angles=angles), args.reps)
        res["fluxes_resident_ms[%s]" % angles] = dict(median=med, min=lo)
        for mol in (False, True):
            med, lo = timed(lambda: atm.jacobians(surfaceTemperature=Ts, angles=angles, molecules=mol), args.reps)
            res["jacobians_resident_ms[%s, molecules=%s]" % (angles, mol)] = dict(median=med, min=lo)
    L = atm[len(atm) // 2]

    def after_change():
        L.changeTemperature(L.T)                        # marks the layer's cross sections dirty (cls:741-743)
        atm.jacobians(surfaceTemperature=Ts, angles=3)
    med, lo = timed(after_change, args.reps)
    res["jacobians_after_changeTemperature_ms[3, molecules=True]"] = dict(median=med, min=lo)
    for k, v in res.items():
        print("%-56s %s" % (k, ("%.3f ms (min %.3f)" % (v["median"], v["min"])) if isinstance(v, dict) else v))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
