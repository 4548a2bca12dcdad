#!/usr/bin/env python3
"""Times the Jacobians of the linear-in-optical-depth Planck source (kernels K5j) against the layer source's Jacobians over a
reflecting surface (K5h) as the PARENT commit's library runs them, on the config-5 column of scripts/flux_time.py (30 layers
x 2.4e6 points, three angles, the absorption coefficients resident) with HIP events on the context's stream.  Plain numbers
for DESIGN.md, no threshold:

  column_linear    ONE lbl_column_jacobian_linear_dev call (Lambertian, emissivity 0.9, no terms, no spectra; the default
                   level temperatures)
  column_surface   ONE lbl_column_jacobian_surface_dev call on the same column, --baseline-lib's
  rays_linear      ONE lbl_ray_jacobian_linear_dev call with 16 reflectedPath rays, secants spread evenly over 1..4
                   (four bundles; 61 elements and 2 + 30 + 120 rows each)
  rays_surface     the same rays through lbl_ray_jacobian_surface_dev (62 rows each), --baseline-lib's

A leg runs in a process of its own (`--leg NAME`) under its own time limit; the two baseline legs load --baseline-lib (a
libpyrad_hip.so built from the parent commit) in place of this tree's library.  Without `--leg` this script starts the four
legs as child processes one after another and prints their medians and the two ratios.  A leg that fails or runs into its
limit ends the script: nothing more is started.  Every leg first makes the absorption coefficients resident
(Atmosphere.transmission), warms its call up twice, then times `--reps` calls between two events."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

LEGS = ("column_linear", "column_surface", "rays_linear", "rays_surface")
BASELINE = ("column_surface", "rays_surface")
EMISSIVITY = 0.9


def leg(which, reps):
    from flux_time import column
    from surface_times import event_ms
    from pyrad_amd import _native, engine, model
    if which in BASELINE:
        # the parent's library does not export this change's entry points: leave them unbound instead of failing to load
        import ctypes
        have = ctypes.CDLL(_native.LIB_PATH)
        for name in [name for name in _native.SIGNATURES if not hasattr(have, name)]:
            del _native.SIGNATURES[name]
    atm, Ts = column()
    atm.transmission(surfaceTemperature=Ts)            # uploads, schedules, every absorption coefficient resident
    ctx = engine.get_engine().ctx
    layers, n = atm._column_layers()
    kbufs, _ = atm._column_abs_coef(ctx, layers, n)
    nl = len(layers)
    T, depth = [L.T for L in layers], [L.depth for L in layers]
    lo, hi = layers[0].rangeMin, layers[0].rangeMax
    mu, weight = model.fluxAngles(3)
    res = {"leg": which, "device": ctx.device_info()["name"], "library": _native.LIB_PATH, "layers": nl, "points": n}
    bufs = []
    try:
        if which == "column_linear":
            lev = atm.levelTemperatures()
            jac = ctx.buffer(3 + 3 * nl)
            bufs.append(jac)
            edges = [(lev[l], lev[l + 1]) for l in range(nl)]
            call = lambda: ctx.column_jacobian_linear_dev(kbufs, edges, depth, lo, hi, n, mu, weight, [0], [n], jac, EMISSIVITY,
                                                          reflection=0, surface_T=Ts)
            res["ms"] = event_ms(ctx, call, reps)
            res["olr"] = float(jac.download(1)[0])
        elif which == "column_surface":
            jac = ctx.buffer(3 + 2 * nl)
            bufs.append(jac)
            call = lambda: ctx.column_jacobian_surface_dev(kbufs, T, depth, lo, hi, n, mu, weight, [0], [n], jac, EMISSIVITY,
                                                           reflection=0, surface_T=Ts)
            res["ms"] = event_ms(ctx, call, reps)
            res["olr"] = float(jac.download(1)[0])
        else:
            linear = which == "rays_linear"
            secants = [1.0 + 3.0 * i / 15.0 for i in range(16)]
            paths = [atm.reflectedPath(mu=1.0 / s, levelTemperatures=True if linear else None) for s in secants]
            segs = [p._segments() for p in paths]
            first = [0]
            for lay, _ in segs:
                first.append(first[-1] + len(lay))
            seg_layer, seg_length = [l for lay, _ in segs for l in lay], [x for _, lens in segs for x in lens]
            rad = ctx.buffer(16 * n)
            bufs.append(rad)
            if linear:
                rows = _native.ray_jacobian_rows(nl, first, seg_layer, linear=True)[1]
                seg_T = [t for p in paths for t in p._segment_temperatures()]
            else:
                rows = _native.ray_jacobian_rows(nl, first, seg_layer, surface=True)[1]
            jac = ctx.buffer(rows * n)
            bufs.append(jac)
            res["rows"] = rows
            if linear:
                call = lambda: ctx.ray_jacobian_linear_dev(kbufs, seg_T, lo, hi, n, first, seg_layer, seg_length, [0] * 16, jac,
                                                           EMISSIVITY, source_T=Ts, radiance=rad)
            else:
                call = lambda: ctx.ray_jacobian_surface_dev(kbufs, T, lo, hi, n, first, seg_layer, seg_length, [0] * 16, jac,
                                                            EMISSIVITY, source_T=Ts, radiance=rad)
            res["ms"] = event_ms(ctx, call, reps)
            res["radiance0"] = float(rad.download(1)[0])
    finally:
        for b in bufs:
            b.free()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS, default=None)
    ap.add_argument("--baseline-lib", default=None, help="libpyrad_hip.so of the parent commit, for the two surface legs")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds one leg may take")
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.reps)
    if not args.baseline_lib or not os.path.isfile(args.baseline_lib):
        sys.exit("--baseline-lib: the parent commit's libpyrad_hip.so is needed for the two surface legs")
    runs = []
    for which in LEGS:
        env = dict(os.environ)
        if which in BASELINE:
            env["PYRAD_HIP_LIB"] = os.path.abspath(args.baseline_lib)
        else:
            env.pop("PYRAD_HIP_LIB", None)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps)],
                               stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout, env=env)
        except subprocess.TimeoutExpired:
            sys.exit("leg %s ran into its time limit: nothing more is started" % which)
        if p.returncode != 0:
            sys.exit("leg %s ended with status %d: nothing more is started" % (which, p.returncode))
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(runs[-1]), flush=True)
    summary = {r["leg"] + "_ms": statistics.median(r["ms"]) for r in runs}
    summary["column_linear_over_surface"] = summary["column_linear_ms"] / summary["column_surface_ms"]
    summary["rays_linear_over_surface"] = summary["rays_linear_ms"] / summary["rays_surface_ms"]
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
