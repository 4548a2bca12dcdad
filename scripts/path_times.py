#!/usr/bin/env python3
"""Times lbl_ray_radiance_dev (kernel K5e) on the config-5 column of scripts/flux_time.py (30 layers x 2.4e6 points) with
HIP events on the context's stream, against the only way a library without it gets the same spectra.

  (a) rays:  ONE lbl_ray_radiance_dev call with 16 nadir rays, secants spread evenly over 1..4; also, as a plain number
             without a baseline, one call with a 30-ray limb scan (tangent heights at every layer's mid height).
  (b) flux:  16 calls of lbl_column_flux_dev, one angle and up_top each - what a library before K5e has to do.

A leg runs in a process of its own (`--leg rays|flux`), so that (b) can run on another build of the library: without
`--leg` this script starts the legs as child processes, alternating (a) on the library of this tree and (b) on
`--baseline-lib` (the parent commit's libpyrad_hip.so, selected for the child through PYRAD_HIP_LIB), `--rounds` times
each, and prints the medians and the ratio.  Every leg first makes the absorption coefficients resident
(Atmosphere.transmission), warms its calls up twice, then times `--reps` windows of the whole leg between two events.
Times from two boxes do not compare: run both legs in one call on one box."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


from path_jacobian_times import event_ms  # noqa: E402  (HIP events on the context's stream, through ctypes)


def leg(which, reps):
    from pyrad_amd import _native
    if which == "flux":
        # (a baseline build does not export the new entry point; this leg does not call it)
        _native.SIGNATURES.pop("lbl_ray_radiance_dev", None)
    from flux_time import column
    from pyrad_amd import engine
    from pyrad_amd.model import Path
    atm, Ts = column()
    atm.transmission(surfaceTemperature=Ts)            # uploads, schedules, every absorption coefficient resident
    ctx = engine.get_engine().ctx
    layers, n = atm._column_layers()
    kbufs, _ = atm._column_abs_coef(ctx, layers, n)
    T, depth = [L.T for L in layers], [L.depth for L in layers]
    lo, hi = layers[0].rangeMin, layers[0].rangeMax
    secants = [1.0 + 3.0 * i / 15.0 for i in range(16)]
    res = {"leg": which, "lib": _native.LIB_PATH, "device": ctx.device_info()["name"], "layers": len(layers), "points": n}
    bufs = []
    try:
        if which == "rays":
            def pack(paths):
                first = [0]
                for p in paths:
                    first.append(first[-1] + len(p))
                return (first, [l for p in paths for l in p.layers], [x for p in paths for x in p.lengths],
                        [Path.SOURCES.index(p.source) for p in paths])
            nadir = pack([atm.nadirPath(mu=1.0 / s) for s in secants])
            z = 0.0
            mids = []
            for d in depth:
                mids.append(z + 0.5 * d)
                z += d
            limb = pack([atm.limbPath(h) for h in mids])
            rad = ctx.buffer(30 * n)
            bufs.append(rad)
            res["nadir16_ms"] = event_ms(ctx, lambda: ctx.ray_radiance_dev(kbufs, T, lo, hi, n, *nadir, rad, source_T=Ts), reps)
            res["limb30_ms"] = event_ms(ctx, lambda: ctx.ray_radiance_dev(kbufs, T, lo, hi, n, *limb, rad, source_T=Ts), reps)
            res["limb30_segments"] = len(limb[1])
        else:
            level, up_top = ctx.buffer(2 * (len(layers) + 1)), ctx.buffer(n)
            bufs += [level, up_top]

            def sixteen():
                for s in secants:
                    ctx.column_flux_dev(kbufs, T, depth, lo, hi, n, [1.0 / s], [1.0], [0], [n], level, surface_T=Ts,
                                        up_top=up_top)
            res["flux16_ms"] = event_ms(ctx, sixteen, reps)
    finally:
        for b in bufs:
            b.free()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("rays", "flux"), default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None, help="libpyrad_hip.so of the parent commit, for the flux leg")
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.reps)
    runs = []
    for _ in range(args.rounds):
        for which in ("rays", "flux"):
            env = dict(os.environ)
            if which == "flux" and args.baseline_lib:
                env["PYRAD_HIP_LIB"] = os.path.abspath(args.baseline_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps)], env=env,
                               stdout=subprocess.PIPE, text=True, timeout=420)
            if p.returncode != 0:
                sys.exit("leg %s ended with status %d: nothing more is started" % (which, p.returncode))
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), flush=True)
    med = lambda key: statistics.median([t for r in runs if key in r for t in r[key]])
    summary = {key: med(key) for key in ("nadir16_ms", "flux16_ms", "limb30_ms")}
    summary["nadir16_over_flux16"] = summary["nadir16_ms"] / summary["flux16_ms"]
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
