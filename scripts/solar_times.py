#!/usr/bin/env python3
"""Times lbl_column_solar_dev (kernels K5k) on the config-5 column of scripts/flux_time.py (30 layers x 2.4e6 points) with
HIP events on the context's stream, beside the thermal call that moves the same bytes.

  solar     Atmosphere.solarFluxes(mu0=0.5, angles=3, emissivity=0.9): one beam down, three diffuse angles up (Lambertian)
  specular  the same beam over a mirror: one beam down and up in one kernel
  flux      Atmosphere.fluxes(angles=3, emissivity=0.9) on the same resident coefficients (lbl_column_flux_surface_dev)

What is timed with events is the C call each of them makes, with every absorption coefficient resident and nothing copied;
`*_call_ms` is the wall time of the whole model call, which ends in a download and so in a synchronise.  A leg runs in a
process of its own (`--leg`) under a time limit of its own: without `--leg` this script starts the legs as child processes,
alternating, `--rounds` times each, and prints every leg's median, its scatter (the spread of its windows over all
rounds, min .. max), the bytes a call has to move - two reads of every layer's coefficients, the source, and F_down at the
surface written and read between the walks - and the share of the HBM's peak rate (8.0 TB/s) those bytes over the median
are.  The criterion (DESIGN.md "K5k"): solar is not slower than flux beyond the scatter of flux's own windows.
Times from two boxes do not compare: run all legs in one call on one box."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

LEGS = ("solar", "specular", "flux")
HBM_PEAK = 8.0e12         # bytes per second


def leg(which, reps):
    from flux_time import column
    from surface_times import event_ms
    from pyrad_amd import _native, engine, model
    atm, Ts = column()
    atm.transmission(surfaceTemperature=Ts)            # uploads, schedules, every absorption coefficient resident
    ctx = engine.get_engine().ctx
    layers, n = atm._column_layers()
    kbufs, _ = atm._column_abs_coef(ctx, layers, n)
    T, depth = [L.T for L in layers], [L.depth for L in layers]
    lo, hi = layers[0].rangeMin, layers[0].rangeMax
    mu, w = model.fluxAngles(3)
    nl = len(layers)
    res = {"leg": which, "lib": _native.LIB_PATH, "device": ctx.device_info()["name"], "layers": nl, "points": n}
    level = ctx.buffer(2 * (nl + 1))
    bufs = [level]
    try:
        if which == "flux":
            res["bytes"] = 8 * n * 2 * nl
            call = lambda: ctx.column_flux_surface_dev(kbufs, T, depth, lo, hi, n, mu, w, [0], [n], level, 0.9, reflection=0,
                                                       surface_T=Ts)
            whole = lambda: atm.fluxes(surfaceTemperature=Ts, angles=3, emissivity=0.9)
        else:
            S0 = ctx.buffer(n).upload(model.solarIrradiance(layers[0].xAxis))
            bufs.append(S0)
            slant = model.solarSlants(depth, [(0.5, 1.0)])
            specular = which == "specular"
            res["bytes"] = 8 * n * (2 * nl + 1 + (0 if specular else 2))
            call = lambda: ctx.column_solar_dev(kbufs, depth, lo, hi, n, S0, [0.5], slant, () if specular else mu,
                                                () if specular else w, [0], [n], level, emissivity=0.9,
                                                reflection=1 if specular else 0)
            whole = lambda: atm.solarFluxes(solarTemperature=5772.0, mu0=0.5, angles=3, emissivity=0.9,
                                            reflection="specular" if specular else "lambertian")
        res["ms"] = event_ms(ctx, call, reps)
        whole(); whole()
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            whole()
            wall.append(1e3 * (time.perf_counter() - t0))
        res["call_ms"] = wall
    finally:
        for b in bufs:
            b.free()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS, default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds a leg's process may take")
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.reps)
    runs = []
    for _ in range(args.rounds):
        for which in LEGS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps)],
                               stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
            if p.returncode != 0:
                sys.exit("leg %s ended with status %d: nothing more is started" % (which, p.returncode))
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for which in LEGS:
        mine = [r for r in runs if r["leg"] == which]
        ts = [t for r in mine for t in r["ms"]]
        med = statistics.median(ts)
        summary[which] = dict(median_ms=med, min_ms=min(ts), max_ms=max(ts), windows=len(ts), bytes=mine[0]["bytes"],
                              hbm_peak_share=mine[0]["bytes"] / (1e-3 * med) / HBM_PEAK,
                              call_median_ms=statistics.median([t for r in mine for t in r["call_ms"]]))
    flux = summary["flux"]
    for which in ("solar", "specular"):
        summary[which]["over_flux"] = summary[which]["median_ms"] / flux["median_ms"]
    # the criterion: not slower than flux beyond the scatter of flux's own windows
    summary["criterion_met"] = bool(summary["solar"]["median_ms"] <= flux["max_ms"])
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)
    if not summary["criterion_met"]:
        sys.exit("solarFluxes is slower than fluxes beyond the scatter of the fluxes timing")


if __name__ == "__main__":
    main()
