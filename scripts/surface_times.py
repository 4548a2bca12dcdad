#!/usr/bin/env python3
"""Times lbl_column_flux_surface_dev (kernel K5g) on the config-5 column of scripts/flux_time.py (30 layers x 2.4e6 points,
three angles, the absorption coefficients resident) with HIP events on the context's stream, against the only way a library
without it gets level fluxes over a reflecting surface.

  (a) surface:     ONE lbl_column_flux_surface_dev call (Lambertian, emissivity 0.9).  Also, as a plain number without a
                   baseline, one lbl_ray_radiance_surface_dev call with 16 reflectedPath rays, secants spread evenly over 1..4.
  (b) workaround:  lbl_column_flux_dev with down_surface, the download of down_surface, e B + (1 - e) F_down / pi on the
                   host, the upload of that as I_surface, and lbl_column_flux_dev again - two passes over all the k_l and a
                   round trip through the host.

A leg runs in a process of its own (`--leg surface|workaround`), so that (b) can run on another build of the library: without
`--leg` this script starts the legs as child processes under a time limit each, alternating (a) on the library of this tree
and (b) on `--baseline-lib` (the parent commit's libpyrad_hip.so, built with scripts/make_variant_lib.sh and selected for
the child through PYRAD_HIP_LIB), `--rounds` times each, and prints the medians, their ratio and the bar: (a) not slower
than (b), the allowance being the scatter of (b) over its own repeats.  Every leg first makes the absorption coefficients
resident (Atmosphere.transmission), warms its calls up twice, then times `--reps` windows of the whole leg between two
events.  Times from two boxes do not compare: run both legs in one call on one box."""
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


def hip_runtime():
    """the HIP runtime the library itself runs on, for the events"""
    import ctypes
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return ctypes.CDLL(name)
        except OSError:
            pass
    sys.exit("libamdhip64.so was not found")


def event_ms(ctx, fn, reps, warmup=2):
    """[ms] of fn() between two HIP events recorded on the context's stream, `reps` times after `warmup` untimed calls"""
    import ctypes
    hip = hip_runtime()
    stream = ctypes.c_void_p(ctx.stream())
    t0, t1 = ctypes.c_void_p(), ctypes.c_void_p()

    def ok(rc):
        if rc != 0:
            sys.exit("a HIP event call returned %d" % rc)
    ok(hip.hipEventCreate(ctypes.byref(t0)))
    ok(hip.hipEventCreate(ctypes.byref(t1)))
    for _ in range(warmup):
        fn()
    ctx.sync()
    out = []
    for _ in range(reps):
        ok(hip.hipEventRecord(t0, stream))
        fn()
        ok(hip.hipEventRecord(t1, stream))
        ok(hip.hipEventSynchronize(t1))
        ms = ctypes.c_float()
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), t0, t1))
        out.append(float(ms.value))
    ok(hip.hipEventDestroy(t0))
    ok(hip.hipEventDestroy(t1))
    return out


NEW_SYMBOLS = ("lbl_column_flux_surface_dev", "lbl_ray_radiance_surface_dev")
EMISSIVITY = 0.9


def leg(which, reps):
    from pyrad_amd import _native
    if which == "workaround":
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
    res = {"leg": which, "lib": _native.LIB_PATH, "device": ctx.device_info()["name"], "layers": len(layers), "points": n}
    level, down = ctx.buffer(2 * (len(layers) + 1)), ctx.buffer(n)
    bufs = [level, down]
    try:
        if which == "surface":
            res["surface_ms"] = event_ms(ctx, lambda: ctx.column_flux_surface_dev(
                kbufs, T, depth, lo, hi, n, mu, weight, [0], [n], level, EMISSIVITY, reflection=0, surface_T=Ts,
                down_surface=down), reps)
            res["net_surface"] = float(np.subtract(*level.download(2 * (len(layers) + 1)).reshape(2, -1)[:, 0]))
            secants = [1.0 + 3.0 * i / 15.0 for i in range(16)]
            segs = [atm.reflectedPath(mu=1.0 / s)._segments() for s in secants]
            first = [0]
            for lay, _ in segs:
                first.append(first[-1] + len(lay))
            rad = ctx.buffer(16 * n)
            bufs.append(rad)
            res["reflected16_ms"] = event_ms(ctx, lambda: ctx.ray_radiance_surface_dev(
                kbufs, T, lo, hi, n, first, [l for lay, _ in segs for l in lay], [x for _, lens in segs for x in lens],
                [0] * 16, rad, EMISSIVITY, source_T=Ts), reps)
        else:
            B = model.planckWavenumber(np.asarray(layers[0].xAxis), Ts)
            source = ctx.buffer(n)
            bufs.append(source)

            def workaround():
                ctx.column_flux_dev(kbufs, T, depth, lo, hi, n, mu, weight, [0], [n], level, surface_T=Ts, down_surface=down)
                source.upload(EMISSIVITY * B + (1.0 - EMISSIVITY) * down.download(n) / math.pi)
                ctx.column_flux_dev(kbufs, T, depth, lo, hi, n, mu, weight, [0], [n], level, I_surface=source)
            res["workaround_ms"] = event_ms(ctx, workaround, reps)
            res["net_surface"] = float(np.subtract(*level.download(2 * (len(layers) + 1)).reshape(2, -1)[:, 0]))
    finally:
        for b in bufs:
            b.free()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("surface", "workaround"), default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds one leg may take")
    ap.add_argument("--baseline-lib", default=None, help="libpyrad_hip.so of the parent commit, for the workaround leg")
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.reps)
    runs = []
    for _ in range(args.rounds):
        for which in ("surface", "workaround"):
            env = dict(os.environ)
            if which == "workaround" and args.baseline_lib:
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
    times = lambda key: [t for r in runs if key in r for t in r[key]]
    summary = {key: statistics.median(times(key)) for key in ("surface_ms", "workaround_ms", "reflected16_ms")}
    b = times("workaround_ms")
    summary["workaround_scatter"] = (max(b) - min(b)) / summary["workaround_ms"]
    summary["surface_over_workaround"] = summary["surface_ms"] / summary["workaround_ms"]
    summary["not_slower"] = summary["surface_ms"] <= summary["workaround_ms"] * (1.0 + summary["workaround_scatter"])
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)
    if not summary["not_slower"]:
        sys.exit("lbl_column_flux_surface_dev is slower than the workaround")


if __name__ == "__main__":
    main()
