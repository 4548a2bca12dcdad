#!/usr/bin/env python3
"""Times Atmosphere.fluxes on the config-5 column (30 layers x 2.4e6 points, built the way bench.api_path_column builds it):
a call with every absorption coefficient resident, for the angle sets 1, 3 and "diffusivity", and a call after
changeTemperature on one layer (its accumulate job + the flux kernels).  Each call returns host arrays, so the wall time
of a call is device-synchronised.  Two warm-up calls, then the median of `--reps`.  Run on the GPU box; kernel times come
from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrad_amd import model, data, settings, synthetic  # noqa: E402


def column():
    cfg = synthetic.config_c5()
    c0 = cfg["layers"][0]
    settings.set_resolution_multiplier(c0["base_resolution"] / .01)
    data.set_source(data.synthetic_source({m["species"]: m["lines"] for m in c0["molecules"]}))
    model.Layer.hasAtmosphere = False
    atm = model.Atmosphere("flux column")
    for c in cfg["layers"]:
        L = atm.addLayer(c["depth"], c["T"], c["P"], c["range_min"], c["range_max"], name=c["name"],
                         dynamicResolution=c.get("dynamic_resolution", True))
        for m in c["molecules"]:
            L.addMolecule(m["species"], **m["conc"])
    return atm, cfg["surface_T"]


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    atm, Ts = column()
    atm.transmission(surfaceTemperature=Ts)            # first call: uploads, schedules, every absorption coefficient resident
    res = {"layers": len(atm), "points": int(atm[0].xAxis.size)}
    med, lo = timed(lambda: atm.transmission(surfaceTemperature=Ts), args.reps)
    res["transmission_resident_ms"] = dict(median=med, min=lo)
    for angles in (1, 3, "diffusivity"):
        med, lo = timed(lambda: atm.fluxes(surfaceTemperature=Ts, angles=angles), args.reps)
        res["fluxes_resident_ms[%s]" % angles] = dict(median=med, min=lo)
    L = atm[len(atm) // 2]

    def after_change():
        L.changeTemperature(L.T)                        # marks the layer's cross sections dirty (cls:741-743)
        atm.fluxes(surfaceTemperature=Ts, angles=3)
    med, lo = timed(after_change, args.reps)
    res["fluxes_after_changeTemperature_ms[3]"] = dict(median=med, min=lo)
    for k, v in res.items():
        print("%-40s %s" % (k, ("%.3f ms (min %.3f)" % (v["median"], v["min"])) if isinstance(v, dict) else v))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
