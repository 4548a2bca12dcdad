#!/usr/bin/env python3
"""Times lbl_ray_jacobian_dev (kernel K5f) on the config-5 column of scripts/flux_time.py (30 layers x 2.4e6 points) with
HIP events on the context's stream, against the only way a library without it gets the same rows.

  (a) rays:  ONE lbl_ray_jacobian_dev call with 8 nadir rays at 8 cosines (two bundles of four), no terms: 8 x 61 rows.
             Also, as plain numbers without a baseline: one call with a 30-ray limb scan (tangent heights at every layer's
             mid height, 30 layer sequences, no bundles), and Atmosphere.pathJacobians for the 8 nadir rays with a 16-channel
             instrument (device-synchronised wall time of the whole call).
  (b) flux:  8 calls of lbl_column_jacobian_dev, one angle and both spectra outputs each (60 rows a call) - what a library
             before K5f has to do.  Both legs write the same number of bytes up to the 8 source rows.

A leg runs in a process of its own (`--leg rays|flux`), so that (b) can run on another build of the library: without
`--leg` this script starts the legs as child processes, alternating (a) on the library of this tree and (b) on
`--baseline-lib` (the parent commit's libpyrad_hip.so from scripts/make_variant_lib.sh, selected for the child through
PYRAD_HIP_LIB), `--rounds` times each, every child under a time limit of its own, and prints the medians, the ratio and
the scatter of (b) over its own repeats, which is the allowance for "(a) is not slower".  Every leg first makes the
absorption coefficients resident (Atmosphere.transmission), warms its calls up twice, then times `--reps` windows of the
whole leg between two events.  Times from two boxes do not compare: run both legs in one call on one box."""
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


def event_ms(ctx, fn, reps, warmup=2):
    """[ms] of fn() between two HIP events recorded on the context's stream, `reps` times after `warmup` untimed calls
    (the HIP runtime the library itself is linked against, through ctypes)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p(ctx.stream())

    def ok(rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)
    t0, t1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(t0)))
    ok(hip.hipEventCreate(C.byref(t1)))
    for _ in range(warmup):
        fn()
    ctx.sync()
    out = []
    try:
        for _ in range(reps):
            ok(hip.hipEventRecord(t0, stream))
            fn()
            ok(hip.hipEventRecord(t1, stream))
            ok(hip.hipEventSynchronize(t1))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), t0, t1))
            out.append(float(ms.value))
    finally:
        hip.hipEventDestroy(t0)
        hip.hipEventDestroy(t1)
    return out


NEW = ("lbl_ray_jacobian_dev", "lbl_ray_jacobian_rows")


def leg(which, reps):
    from pyrad_amd import _native
    if which == "flux":
        # (a baseline build does not export the new entry points; this leg does not call them)
        for name in NEW:
            _native.SIGNATURES.pop(name, None)
    from flux_time import column
    from pyrad_amd import engine, model
    atm, Ts = column()
    atm.transmission(surfaceTemperature=Ts)            # uploads, schedules, every absorption coefficient resident
    ctx = engine.get_engine().ctx
    layers, n = atm._column_layers()
    kbufs, _ = atm._column_abs_coef(ctx, layers, n)
    T, depth = [L.T for L in layers], [L.depth for L in layers]
    lo, hi = layers[0].rangeMin, layers[0].rangeMax
    nl = len(layers)
    cosines = [1.0 / (1.0 + 3.0 * i / 7.0) for i in range(8)]
    res = {"leg": which, "lib": _native.LIB_PATH, "device": ctx.device_info()["name"], "layers": nl, "points": n}
    bufs = []
    try:
        if which == "rays":
            def pack(paths):
                first = [0]
                for p in paths:
                    first.append(first[-1] + len(p))
                return (first, [l for p in paths for l in p.layers], [x for p in paths for x in p.lengths],
                        [model.Path.SOURCES.index(p.source) for p in paths])
            nadir_paths = [atm.nadirPath(mu=m) for m in cosines]
            nadir = pack(nadir_paths)
            z, mids = 0.0, []
            for d in depth:
                mids.append(z + 0.5 * d)
                z += d
            limb = pack([atm.limbPath(h) for h in mids])
            rows_nadir = _native.ray_jacobian_rows(nl, nadir[0], nadir[1])[1]
            rows_limb = _native.ray_jacobian_rows(nl, limb[0], limb[1])[1]
            jac, rad = ctx.buffer(max(rows_nadir, rows_limb) * n), ctx.buffer(30 * n)
            bufs += [jac, rad]
            res["nadir8_ms"] = event_ms(ctx, lambda: ctx.ray_jacobian_dev(kbufs, T, lo, hi, n, *nadir, jac, source_T=Ts,
                                                                            radiance=rad), reps)
            res["nadir8_rows"] = rows_nadir
            res["limb30_ms"] = event_ms(ctx, lambda: ctx.ray_jacobian_dev(kbufs, T, lo, hi, n, *limb, jac, source_T=Ts,
                                                                           radiance=rad), reps)
            res["limb30_rows"], res["limb30_segments"] = rows_limb, len(limb[1])
            ins = model.Instrument([lo + (i + 0.5) * (hi - lo) / 16.0 for i in range(16)], width=0.1 * (hi - lo) / 16.0)
            call = lambda: atm.pathJacobians(nadir_paths, surfaceTemperature=Ts, instrument=ins)
            call(), call()
            wall = []
            for _ in range(reps):
                ctx.sync()
                t0 = time.perf_counter()
                call()
                ctx.sync()
                wall.append(1e3 * (time.perf_counter() - t0))
            res["channels16_call_ms"] = wall
        else:
            jac, ln_tau, T_spec = ctx.buffer(2 + 2 * nl), ctx.buffer(nl * n), ctx.buffer(nl * n)
            bufs += [jac, ln_tau, T_spec]

            def eight():
                for m in cosines:
                    ctx.column_jacobian_dev(kbufs, T, depth, lo, hi, n, [m], [1.0], [0], [n], jac, surface_T=Ts,
                                            ln_tau_spectra=ln_tau, T_spectra=T_spec)
            res["jacobian8_ms"] = event_ms(ctx, eight, reps)
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
                               stdout=subprocess.PIPE, text=True, timeout=240)
            if p.returncode != 0:
                sys.exit("leg %s ended with status %d: nothing more is started" % (which, p.returncode))
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), flush=True)
    every = lambda key: [t for r in runs if key in r for t in r[key]]
    summary = {key: statistics.median(every(key)) for key in ("nadir8_ms", "jacobian8_ms", "limb30_ms", "channels16_call_ms")}
    b = every("jacobian8_ms")
    summary["jacobian8_min_max_ms"] = [min(b), max(b)]
    summary["jacobian8_scatter"] = (max(b) - min(b)) / summary["jacobian8_ms"]      # the allowance, from (b) alone
    summary["nadir8_over_jacobian8"] = summary["nadir8_ms"] / summary["jacobian8_ms"]
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"runs": runs, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
