#!/usr/bin/env python3
"""Times the linear-in-optical-depth Planck source (kernels K5i) on the config-5 column of scripts/flux_time.py (30 layers x
2.4e6 points, the absorption coefficients resident) with HIP events on the context's stream, against the layer source of
the parent commit's library:

  (a) linear:  ONE lbl_column_flux_linear_dev call (three angles, Lambertian, emissivity 0.9, the default level temperatures),
               and ONE lbl_ray_radiance_linear_dev call with the nine test paths (nadir, zenith and limb views, built with
               level temperatures; the limb paths then cross their tangent layer in two segments).
  (b) layer:   lbl_column_flux_surface_dev with the same arguments and the layers' temperatures, and
               lbl_ray_radiance_surface_dev with the same nine paths built without level temperatures.

What (a) does more per layer (segment) and point: a second Planck value, from a second exp per thread on the fast path,
and per angle (ray) one g(tau) - a division and an 11-term polynomial.  There is no pass mark.

A leg runs in a process of its own (`--leg linear|layer`), so that (b) can run on another build of the library: without
`--leg` this script starts the legs as child processes under a time limit each, alternating (a) on the library of this tree
and (b) on `--baseline-lib` (the parent commit's libpyrad_hip.so, selected for the child through PYRAD_HIP_LIB), `--rounds`
times each, and prints the medians and their ratios.  Every leg first makes the absorption coefficients resident
(Atmosphere.transmission), warms its calls up twice, then times `--reps` calls between two events each.  Times from two boxes
do not compare: run both legs in one call on one box."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from surface_times import event_ms  # noqa: E402

NEW_SYMBOLS = ("lbl_column_flux_linear_dev", "lbl_ray_radiance_linear_dev")
EMISSIVITY = 0.9


def nine_paths(atm, lev):
    """tests/test_gpu_paths.py's nine views, at heights in proportion to this column's"""
    nl = len(atm)
    top = sum(L.depth for L in atm)
    kw = {} if lev is None else dict(levelTemperatures=lev)
    return [atm.nadirPath(**kw), atm.nadirPath(mu=0.4, **kw), atm.nadirPath(observerLevel=nl // 2, **kw),
            atm.zenithPath(**kw), atm.zenithPath(mu=0.3, **kw), atm.zenithPath(observerLevel=nl // 2, **kw),
            atm.limbPath(0.03 * top, **kw), atm.limbPath(0.15 * top, **kw), atm.limbPath(0.9 * top, **kw)]


def leg(which, reps):
    from pyrad_amd import _native
    if which == "layer":
        # (a baseline build does not export the new entry points; this leg does not call them)
        for name in NEW_SYMBOLS:
            _native.SIGNATURES.pop(name, None)
    import numpy as np
    from flux_time import column
    from pyrad_amd import engine, model
    atm, Ts = column()
    atm.transmission(surfaceTemperature=Ts)            # uploads, schedules, every absorption coefficient resident
    ctx = engine.get_engine().ctx
    layers, n = atm._column_layers()
    kbufs, _ = atm._column_abs_coef(ctx, layers, n)
    T, depth = [L.T for L in layers], [L.depth for L in layers]
    lo, hi = layers[0].rangeMin, layers[0].rangeMax
    mu, weight = model.fluxAngles(3)
    lev = atm.levelTemperatures()
    paths = nine_paths(atm, lev if which == "linear" else None)
    first = np.cumsum([0] + [len(p) for p in paths])
    seg_layer, seg_length = [l for p in paths for l in p.layers], [x for p in paths for x in p.lengths]
    kinds = [model.Path.SOURCES.index(p.source) for p in paths]
    res = {"leg": which, "lib": _native.LIB_PATH, "device": ctx.device_info()["name"], "layers": len(layers), "points": n,
           "segments": int(first[-1])}
    level, rad = ctx.buffer(2 * (len(layers) + 1)), ctx.buffer(len(paths) * n)
    try:
        if which == "linear":
            edges = np.column_stack([lev[:-1], lev[1:]])
            res["flux_ms"] = event_ms(ctx, lambda: ctx.column_flux_linear_dev(
                kbufs, edges, depth, lo, hi, n, mu, weight, [0], [n], level, EMISSIVITY, reflection=0, surface_T=Ts), reps)
            seg_T = [t for p in paths for t in p.temperatures]
            res["rays_ms"] = event_ms(ctx, lambda: ctx.ray_radiance_linear_dev(
                kbufs, seg_T, lo, hi, n, first, seg_layer, seg_length, kinds, rad, EMISSIVITY, source_T=Ts), reps)
        else:
            res["flux_ms"] = event_ms(ctx, lambda: ctx.column_flux_surface_dev(
                kbufs, T, depth, lo, hi, n, mu, weight, [0], [n], level, EMISSIVITY, reflection=0, surface_T=Ts), reps)
            res["rays_ms"] = event_ms(ctx, lambda: ctx.ray_radiance_surface_dev(
                kbufs, T, lo, hi, n, first, seg_layer, seg_length, kinds, rad, EMISSIVITY, source_T=Ts), reps)
        res["up_top"] = float(level.download(2 * (len(layers) + 1))[len(layers)])
    finally:
        level.free()
        rad.free()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("linear", "layer"), default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds one leg may take")
    ap.add_argument("--baseline-lib", default=None, help="libpyrad_hip.so of the parent commit, for the layer leg")
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.reps)
    runs = []
    for _ in range(args.rounds):
        for which in ("linear", "layer"):
            env = dict(os.environ)
            if which == "layer" and args.baseline_lib:
                env["PYRAD_HIP_LIB"] = os.path.abspath(args.baseline_lib)
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps)], env=env,
                                   stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
            except subprocess.TimeoutExpired:
                sys.exit("leg %s ran into its time limit: nothing more is started" % which)
            if p.returncode != 0:
                sys.exit("leg %s ended with status %d: nothing more is started" % (which, p.returncode))
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for key in ("flux_ms", "rays_ms"):
        for which in ("linear", "layer"):
            summary["%s_%s" % (which, key)] = statistics.median([t for r in runs if r["leg"] == which for t in r[key]])
        summary["linear_over_layer_" + key[:-3]] = summary["linear_" + key] / summary["layer_" + key]
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
