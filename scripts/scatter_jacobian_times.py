#!/usr/bin/env python3
"""Times lbl_column_jacobian_scatter_dev (kernels K5p) on the config-5 column of scripts/flux_time.py (30 layers x 2.4e6
points) with HIP events on the context's stream, for both Planck settings, with and without the molecule terms, beside the
forward call lbl_column_flux_scatter_dev on the same resident coefficients and scatterers.

  jac_layer         lbl_column_jacobian_scatter_dev, planck_linear 0: rayleighScatterer + one cloud, emissivity 0.9, no terms
  jac_layer_terms   the same with the molecule terms of Atmosphere.jacobians
  jac_linear        planck_linear 1 and levelTemperatures(), no terms
  jac_linear_terms  the same with the molecule terms
  flux_layer        lbl_column_flux_scatter_dev, planck_linear 0 (scripts/scatter_flux_times.py's scatter_layer)
  flux_linear       the same with planck_linear 1

What is timed with events is the C call, with every absorption coefficient (and every term) resident and nothing copied.  A
leg runs in a process of its own (`--leg`) under a time limit of its own: without `--leg` this script starts the legs as
child processes, alternating, `--rounds` times each; `--flux-tree` names a checkout of this repository, built, whose package
and library the two flux legs import in place of this one's (an earlier commit's, to measure against it).  Per leg: the
median, the spread (min .. max over all windows), the rows per band; per Jacobian leg its ratio to the flux leg of its Planck setting, the number of forward calls
that central differences of the same rows would take - one for F and two for every other row - and that number times the
flux leg's median.  There is no pass mark.  Times from two boxes do not compare: run all legs in one call on one box."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.environ.get("SCATTER_JACOBIAN_TIMES_TREE") or os.path.dirname(HERE)      # (a flux leg under --flux-tree: that tree)
sys.path.insert(0, os.path.join(TREE, "scripts"))
sys.path.insert(0, TREE)

LEGS = ("jac_layer", "flux_layer", "jac_layer_terms", "jac_linear", "flux_linear", "jac_linear_terms")


def leg(which, reps):
    from flux_time import column
    from surface_times import event_ms
    from pyrad_amd import _native, engine, model
    atm, Ts = column()
    atm.transmission(surfaceTemperature=Ts)            # uploads, schedules, every absorption coefficient resident
    ctx = engine.get_engine().ctx
    layers, n = atm._column_layers()
    kbufs, plan = atm._column_abs_coef(ctx, layers, n)
    depth = [L.depth for L in layers]
    lo, hi = layers[0].rangeMin, layers[0].rangeMax
    nl = len(layers)
    res = {"leg": which, "lib": _native.LIB_PATH, "device": ctx.device_info()["name"], "layers": nl, "points": n}
    air = model.rayleighScatterer(atm)
    cloud = model.Scatterer([5.0 if l == 3 else 0.0 for l in range(nl)], 1.0, 0.9, 0.85, name="cloud")
    scat = ([air.amounts, cloud.amounts], None, [1.0, 0.9], [0.0, 0.85])
    linear = "linear" in which
    lev = atm.levelTemperatures()
    T = [t for pair in zip(lev[:-1], lev[1:]) for t in pair] if linear else [L.T for L in layers]
    jacobian = which.startswith("jac")
    size = ctx.column_jacobian_scatter_workspace if jacobian else ctx.column_flux_scatter_workspace
    tile = size(nl, 1)
    doubles = min(size(nl, n), model.TWOSTREAM_WORKSPACE_BYTES // 8 // tile * tile)
    bufs = []
    try:
        work, sigma = ctx.buffer(doubles), ctx.buffer(n).upload(air.extinction)
        bufs += [work, sigma]
        res["workspace_bytes"] = 8 * doubles
        res["passes"] = -(-n // (doubles // tile * 256))
        if jacobian:
            terms, where = atm._jacobian_terms(ctx, layers, n, plan) if which.endswith("terms") else ([], [])
            rows = 3 + (1 + (2 if linear else 1) + 2) * nl + len(terms)
            jac = ctx.buffer(rows)
            bufs.append(jac)
            res["rows"], res["terms"] = rows, len(terms)
            call = lambda: ctx.column_jacobian_scatter_dev(kbufs, T, int(linear), depth, lo, hi, n, scat[0], [sigma, 1.0], scat[2],
                                                           scat[3], 1, [0], [n], work, jac, emissivity=0.9, surface_T=Ts,
                                                           term_abs_coef=terms, term_layer=where)
        else:
            level = ctx.buffer(2 * (nl + 1))
            bufs.append(level)
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
    ap.add_argument("--flux-tree", default=None, help="a built checkout whose package the flux legs import (default: this one)")
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.reps)
    runs = []
    for _ in range(args.rounds):
        for which in LEGS:
            env = dict(os.environ)
            if args.flux_tree and which.startswith("flux"):
                env["SCATTER_JACOBIAN_TIMES_TREE"] = os.path.abspath(args.flux_tree)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps)],
                               stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout, env=env)
            if p.returncode != 0:
                sys.exit("leg %s ended with status %d: nothing more is started" % (which, p.returncode))
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for which in LEGS:
        mine = [r for r in runs if r["leg"] == which]
        ts = [t for r in mine for t in r["ms"]]
        summary[which] = dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), windows=len(ts),
                              lib=mine[0]["lib"], workspace_bytes=mine[0]["workspace_bytes"], passes=mine[0]["passes"])
        for key in ("rows", "terms"):
            if key in mine[0]:
                summary[which][key] = mine[0][key]
    for which in LEGS:
        if which.startswith("jac"):
            s, forward = summary[which], summary["flux_linear" if "linear" in which else "flux_layer"]["median_ms"]
            s["over_flux"] = s["median_ms"] / forward
            s["difference_calls"] = 1 + 2 * (s["rows"] - 1)
            s["difference_ms"] = s["difference_calls"] * forward
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
