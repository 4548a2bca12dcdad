#!/usr/bin/env python3
"""Times the Jacobians over a reflecting surface (kernels K5h) on the config-5 column of scripts/flux_time.py (30 layers x
2.4e6 points, three angles, the absorption coefficients resident) with HIP events on the context's stream.  Plain numbers
for DESIGN.md, no threshold:

  column_surface   ONE lbl_column_jacobian_surface_dev call (Lambertian, emissivity 0.9, no terms, no spectra)
  column_black     ONE lbl_column_jacobian_dev call on the same column over the black surface
  rays_jacobian    ONE lbl_ray_jacobian_surface_dev call with 16 reflectedPath rays, secants spread evenly over 1..4
                   (four bundles, 61 elements and 62 rows each)
  rays_radiance    the same rays through lbl_ray_radiance_surface_dev

A leg runs in a process of its own (`--leg NAME`) under its own time limit: without `--leg` this script starts the four legs
as child processes one after another and prints their medians and the two ratios.  A leg that fails or runs into its limit
ends the script: nothing more is started.  Every leg first makes the absorption coefficients resident
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

from surface_times import event_ms  # noqa: E402

LEGS = ("column_surface", "column_black", "rays_jacobian", "rays_radiance")
EMISSIVITY = 0.9


def leg(which, reps):
    from flux_time import column
    from pyrad_amd import _native, engine, model
    atm, Ts = column()
    atm.transmission(surfaceTemperature=Ts)            # uploads, schedules, every absorption coefficient resident
    ctx = engine.get_engine().ctx
    layers, n = atm._column_layers()
    kbufs, _ = atm._column_abs_coef(ctx, layers, n)
    nl = len(layers)
    T, depth = [L.T for L in layers], [L.depth for L in layers]
    lo, hi = layers[0].rangeMin, layers[0].rangeMax
    mu, weight = model.fluxAngles(3)
    res = {"leg": which, "device": ctx.device_info()["name"], "layers": nl, "points": n}
    bufs = []
    try:
        if which.startswith("column"):
            jac = ctx.buffer(3 + 2 * nl)
            bufs.append(jac)
            if which == "column_surface":
                call = lambda: ctx.column_jacobian_surface_dev(kbufs, T, depth, lo, hi, n, mu, weight, [0], [n], jac, EMISSIVITY,
                                                               reflection=0, surface_T=Ts)
            else:
                call = lambda: ctx.column_jacobian_dev(kbufs, T, depth, lo, hi, n, mu, weight, [0], [n], jac, surface_T=Ts)
            res["ms"] = event_ms(ctx, call, reps)
            res["olr"] = float(jac.download(1)[0])
        else:
            secants = [1.0 + 3.0 * i / 15.0 for i in range(16)]
            segs = [atm.reflectedPath(mu=1.0 / s)._segments() for s in secants]
            first = [0]
            for lay, _ in segs:
                first.append(first[-1] + len(lay))
            seg_layer, seg_length = [l for lay, _ in segs for l in lay], [x for _, lens in segs for x in lens]
            rad = ctx.buffer(16 * n)
            bufs.append(rad)
            if which == "rays_jacobian":
                rows = _native.ray_jacobian_rows(nl, first, seg_layer, surface=True)[1]
                jac = ctx.buffer(rows * n)
                bufs.append(jac)
                res["rows"] = rows
                call = lambda: ctx.ray_jacobian_surface_dev(kbufs, T, lo, hi, n, first, seg_layer, seg_length, [0] * 16, jac,
                                                            EMISSIVITY, source_T=Ts, radiance=rad)
            else:
                call = lambda: ctx.ray_radiance_surface_dev(kbufs, T, lo, hi, n, first, seg_layer, seg_length, [0] * 16, rad,
                                                            EMISSIVITY, source_T=Ts)
            res["ms"] = event_ms(ctx, call, reps)
            res["radiance0"] = float(rad.download(1)[0])
    finally:
        for b in bufs:
            b.free()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS, default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds one leg may take")
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.reps)
    runs = []
    for which in LEGS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps)],
                               stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("leg %s ran into its time limit: nothing more is started" % which)
        if p.returncode != 0:
            sys.exit("leg %s ended with status %d: nothing more is started" % (which, p.returncode))
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(runs[-1]), flush=True)
    summary = {r["leg"] + "_ms": statistics.median(r["ms"]) for r in runs}
    summary["column_surface_over_black"] = summary["column_surface_ms"] / summary["column_black_ms"]
    summary["rays_jacobian_over_radiance"] = summary["rays_jacobian_ms"] / summary["rays_radiance_ms"]
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
