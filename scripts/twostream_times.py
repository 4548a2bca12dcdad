#!/usr/bin/env python3
"""Times lbl_column_twostream_dev (kernels K5l) on the config-5 column of scripts/flux_time.py (30 layers x 2.4e6 points) with
HIP events on the context's stream, beside the direct-beam call on the same resident coefficients and library.

  twostream  Atmosphere.solarFluxesTwoStream(rayleighScatterer + one cloud, mu0=0.5, emissivity=0.9): one beam, two scatterers
  solar      Atmosphere.solarFluxes(mu0=0.5, angles=[(1 / sqrt(3), 1)], emissivity=0.9): one beam down, one diffuse angle up

What is timed with events is the C call each of them makes, with every absorption coefficient resident and nothing copied;
`*_call_ms` is the wall time of the whole model call, which ends in a download and so in a synchronise.  A leg runs in a
process of its own (`--leg`) under a time limit of its own: without `--leg` this script starts the legs as child processes,
alternating, `--rounds` times each, and prints every leg's median, its scatter (min .. max over all windows), the bytes a call
has to move - twostream: one read of every layer's coefficients, the Rayleigh cross section and the source, and five numbers
per level written and read through the workspace - the share of the HBM's peak rate (8.0 TB/s) those bytes over the median
are, the workspace's size and the passes it makes the band take, and the ratio of the two medians.  There is no pass mark:
before K5l no call did this work.  Times from two boxes do not compare: run both legs in one call on one box."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

LEGS = ("twostream", "solar")
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
    depth = [L.depth for L in layers]
    lo, hi = layers[0].rangeMin, layers[0].rangeMax
    nl = len(layers)
    x = layers[0].xAxis
    res = {"leg": which, "lib": _native.LIB_PATH, "device": ctx.device_info()["name"], "layers": nl, "points": n}
    S0 = ctx.buffer(n).upload(model.solarIrradiance(x))
    slant = model.solarSlants(depth, [(0.5, 1.0)])
    bufs = [S0]
    try:
        if which == "solar":
            level = ctx.buffer(2 * (nl + 1))
            bufs.append(level)
            res["bytes"] = 8 * n * (2 * nl + 1 + 2)
            call = lambda: ctx.column_solar_dev(kbufs, depth, lo, hi, n, S0, [0.5], slant, [1.0 / math.sqrt(3.0)], [1.0], [0], [n],
                                                level, emissivity=0.9, reflection=0)
            whole = lambda: atm.solarFluxes(solarTemperature=5772.0, mu0=0.5, angles=[(1.0 / math.sqrt(3.0), 1.0)], emissivity=0.9)
        else:
            air = model.rayleighScatterer(atm)
            cloud = model.Scatterer([5.0 if l == 3 else 0.0 for l in range(nl)], 1.0, 0.9, 0.85, name="cloud")
            tile = ctx.column_twostream_workspace(nl, 1)
            doubles = min(ctx.column_twostream_workspace(nl, n), model.TWOSTREAM_WORKSPACE_BYTES // 8 // tile * tile)
            level, work, sigma = ctx.buffer(3 * (nl + 1)), ctx.buffer(doubles), ctx.buffer(n).upload(air.extinction)
            bufs += [level, work, sigma]
            per_pass = doubles // tile * 256
            res["workspace_bytes"] = 8 * doubles
            res["passes"] = -(-n // per_pass)
            res["bytes"] = 8 * n * (nl + 2 + 2 * 5 * (nl + 1))
            call = lambda: ctx.column_twostream_dev(kbufs, depth, lo, hi, n, S0, [0.5], slant, [air.amounts, cloud.amounts],
                                                    [sigma, 1.0], [1.0, 0.9], [0.0, 0.85], 1, [0], [n], work, level,
                                                    emissivity=0.9)
            whole = lambda: atm.solarFluxesTwoStream([air, cloud], solarTemperature=5772.0, mu0=0.5, emissivity=0.9)
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
    for key in ("workspace_bytes", "passes"):
        summary["twostream"][key] = [r for r in runs if r["leg"] == "twostream"][0][key]
    summary["twostream"]["over_solar"] = summary["twostream"]["median_ms"] / summary["solar"]["median_ms"]
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
