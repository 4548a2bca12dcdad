#!/usr/bin/env python3
"""Times lbl_column_flux_scatter_dev (kernels K5m) on the config-5 column of scripts/flux_time.py (30 layers x 2.4e6 points)
with HIP events on the context's stream, for both Planck settings, beside the one-beam solar two-stream call and the thermal
surface call with one angle on the same resident coefficients, scatterers and library.

  scatter_layer   lbl_column_flux_scatter_dev, planck_linear 0: rayleighScatterer + one cloud, emissivity 0.9
  scatter_linear  the same with planck_linear 1 and levelTemperatures()
  twostream       lbl_column_twostream_dev: one beam (mu0 = 0.5), the same two scatterers, emissivity 0.9
  surface         lbl_column_flux_surface_dev: the angle set {(1 / sqrt(3), pi)}, Lambertian, emissivity 0.9 (no scatterers)

What is timed with events is the C call, with every absorption coefficient resident and nothing copied.  A leg runs in a
process of its own (`--leg`) under a time limit of its own: without `--leg` this script starts the legs as child processes,
alternating, `--rounds` times each, and prints every leg's median, its spread (min .. max over all windows), the bytes a call
has to move - the scatter legs: one read of every layer's coefficients and of the Rayleigh cross section, and four numbers per
level written and read through the workspace - the share of the HBM's peak rate (8.0 TB/s) those bytes over the median are,
the workspace's size and passes, and each scatter leg's ratio to the two-stream leg, the yardstick.  There is no pass mark.
Times from two boxes do not compare: run all legs in one call on one box."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

LEGS = ("scatter_layer", "twostream", "scatter_linear", "surface")
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
    air = model.rayleighScatterer(atm)
    cloud = model.Scatterer([5.0 if l == 3 else 0.0 for l in range(nl)], 1.0, 0.9, 0.85, name="cloud")
    scat = ([air.amounts, cloud.amounts], None, [1.0, 0.9], [0.0, 0.85])
    bufs = []
    try:
        if which == "surface":
            level = ctx.buffer(2 * (nl + 1))
            bufs.append(level)
            res["bytes"] = 8 * n * 2 * nl
            call = lambda: ctx.column_flux_surface_dev(kbufs, [L.T for L in layers], depth, lo, hi, n, [1.0 / math.sqrt(3.0)],
                                                       [math.pi], [0], [n], level, 0.9, reflection=0, surface_T=Ts)
        else:
            solar = which == "twostream"
            q = 5 if solar else 4
            size = ctx.column_twostream_workspace if solar else ctx.column_flux_scatter_workspace
            tile = size(nl, 1)
            doubles = min(size(nl, n), model.TWOSTREAM_WORKSPACE_BYTES // 8 // tile * tile)
            level, work, sigma = ctx.buffer(3 * (nl + 1)), ctx.buffer(doubles), ctx.buffer(n).upload(air.extinction)
            bufs += [level, work, sigma]
            res["workspace_bytes"] = 8 * doubles
            res["passes"] = -(-n // (doubles // tile * 256))
            res["bytes"] = 8 * n * (nl + 1 + (1 if solar else 0) + 2 * q * (nl + 1))
            if solar:
                S0 = ctx.buffer(n).upload(model.solarIrradiance(x))
                bufs.append(S0)
                slant = model.solarSlants(depth, [(0.5, 1.0)])
                call = lambda: ctx.column_twostream_dev(kbufs, depth, lo, hi, n, S0, [0.5], slant, scat[0], [sigma, 1.0], scat[2],
                                                        scat[3], 1, [0], [n], work, level, emissivity=0.9)
            else:
                linear = which == "scatter_linear"
                lev = atm.levelTemperatures()
                T = [t for pair in zip(lev[:-1], lev[1:]) for t in pair] if linear else [L.T for L in layers]
                call = lambda: ctx.column_flux_scatter_dev(kbufs, T, int(linear), depth, lo, hi, n, scat[0], [sigma, 1.0], scat[2],
                                                           scat[3], 1, [0], [n], work, level, emissivity=0.9, surface_T=Ts)
        res["ms"] = event_ms(ctx, call, reps)
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
                              hbm_peak_share=mine[0]["bytes"] / (1e-3 * med) / HBM_PEAK)
        for key in ("workspace_bytes", "passes"):
            if key in mine[0]:
                summary[which][key] = mine[0][key]
    for which in ("scatter_layer", "scatter_linear"):
        summary[which]["over_twostream"] = summary[which]["median_ms"] / summary["twostream"]["median_ms"]
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
