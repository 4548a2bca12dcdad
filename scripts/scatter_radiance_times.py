#!/usr/bin/env python3
"""Times lbl_column_radiance_scatter_dev (kernels K5n) with 1, 4 and 16 views on the config-5 column of scripts/flux_time.py
(30 layers x 2.4e6 points) with HIP events on the context's stream, beside lbl_column_flux_scatter_dev (K5m) on the same
resident coefficients, scatterers (rayleighScatterer + one cloud), surface (emissivity 0.9), Planck setting (the linear
source with levelTemperatures()) and library.

  flux          lbl_column_flux_scatter_dev, one band over the grid
  radiance_1    lbl_column_radiance_scatter_dev, the view (1.0, up)
  radiance_4    ... the views (1.0, up), (0.5, up), (0.5, down), (1.0, down)
  radiance_16   ... sixteen views, eight up and eight down, mu = 0.1 .. 1.0

What is timed with events is the C call, with every absorption coefficient resident and nothing copied.  A leg runs in a
process of its own (`--leg`) under a time limit of its own: without `--leg` this script starts the legs as child processes,
alternating, `--rounds` times each, and prints every leg's median and spread (min .. max over all windows), the workspace's
size and passes, each radiance leg's ratio to the flux leg and the cost per added view, (t_16 - t_1) / 15 and
(t_4 - t_1) / 3.  There is no pass mark.  Times from two boxes do not compare: run all legs in one call on one box."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

LEGS = ("flux", "radiance_1", "radiance_4", "radiance_16")
VIEWS = {
    "radiance_1": [(1.0, 0)],
    "radiance_4": [(1.0, 0), (0.5, 0), (0.5, 1), (1.0, 1)],
    "radiance_16": [(0.1 + 0.9 * i / 7, d) for d in (0, 1) for i in range(8)],
}


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
    res = {"leg": which, "lib": _native.LIB_PATH, "device": ctx.device_info()["name"], "layers": nl, "points": n}
    air = model.rayleighScatterer(atm)
    cloud = model.Scatterer([5.0 if l == 3 else 0.0 for l in range(nl)], 1.0, 0.9, 0.85, name="cloud")
    amounts, ssa, asym = [air.amounts, cloud.amounts], [1.0, 0.9], [0.0, 0.85]
    lev = atm.levelTemperatures()
    T = [t for pair in zip(lev[:-1], lev[1:]) for t in pair]
    tile = ctx.column_flux_scatter_workspace(nl, 1)
    doubles = min(ctx.column_flux_scatter_workspace(nl, n), model.TWOSTREAM_WORKSPACE_BYTES // 8 // tile * tile)
    work, sigma = ctx.buffer(doubles), ctx.buffer(n).upload(air.extinction)
    bufs = [work, sigma]
    res["workspace_bytes"] = 8 * doubles
    res["passes"] = -(-n // (doubles // tile * 256))
    try:
        if which == "flux":
            level = ctx.buffer(2 * (nl + 1))
            bufs.append(level)
            call = lambda: ctx.column_flux_scatter_dev(kbufs, T, 1, depth, lo, hi, n, amounts, [sigma, 1.0], ssa, asym, 1, [0],
                                                       [n], work, level, emissivity=0.9, surface_T=Ts)
        else:
            views = VIEWS[which]
            rad = ctx.buffer(len(views) * n)
            bufs.append(rad)
            res["views"] = len(views)
            call = lambda: ctx.column_radiance_scatter_dev(kbufs, T, 1, depth, lo, hi, n, amounts, [sigma, 1.0], ssa, asym, 1,
                                                           [m for m, _ in views], [d for _, d in views], work, rad,
                                                           emissivity=0.9, surface_T=Ts)
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
        summary[which] = dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), windows=len(ts),
                              workspace_bytes=mine[0]["workspace_bytes"], passes=mine[0]["passes"])
    for which in LEGS[1:]:
        summary[which]["over_flux"] = summary[which]["median_ms"] / summary["flux"]["median_ms"]
    t1, t4, t16 = (summary[w]["median_ms"] for w in LEGS[1:])
    summary["ms_per_added_view"] = {"1_to_4": (t4 - t1) / 3, "1_to_16": (t16 - t1) / 15}
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
