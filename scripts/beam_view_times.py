#!/usr/bin/env python3
"""Times lbl_column_beam_radiance_dev (kernels K5o) with 1, 4 and 16 views on the config-5 column of scripts/flux_time.py
(30 layers x 2.4e6 points) with HIP events on the context's stream, beside lbl_column_twostream_dev (K5l, one beam) and
lbl_column_radiance_scatter_dev (K5n, the same views) on the same resident coefficients, scatterers (rayleighScatterer + one
cloud), surface (emissivity 0.9) and library.

  twostream     lbl_column_twostream_dev, one sun (mu0 = 0.5, plane), one band over the grid
  beam_1        lbl_column_beam_radiance_dev, the same sun, the view (1.0, up)
  beam_4        ... the views (1.0, up), (0.5, up), (0.5, down), (1.0, down)
  beam_16       ... sixteen views, eight up and eight down, mu = 0.1 .. 1.0
  thermal_1/4/16   lbl_column_radiance_scatter_dev with those views (the linear source with levelTemperatures())

What is timed with events is the C call, with every absorption coefficient resident and nothing copied.  All legs run in one
process on one column, each warmed up on its own shapes, `--rounds` times in alternation, `--reps` windows a round; printed
are every leg's median and spread (min .. max over all windows), the workspaces' sizes and passes, each beam leg's ratio to
the two-stream call and to the thermal leg of the same views, and the cost per added view of both families,
(t_16 - t_1) / 15 and (t_4 - t_1) / 3.  There is no pass mark.  Times from two boxes do not compare."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

VIEWS = {
    1: [(1.0, 0)],
    4: [(1.0, 0), (0.5, 0), (0.5, 1), (1.0, 1)],
    16: [(0.1 + 0.9 * i / 7, d) for d in (0, 1) for i in range(8)],
}
LEGS = ("twostream",) + tuple("%s_%d" % (f, v) for f in ("beam", "thermal") for v in VIEWS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
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
    air = model.rayleighScatterer(atm)
    cloud = model.Scatterer([5.0 if l == 3 else 0.0 for l in range(nl)], 1.0, 0.9, 0.85, name="cloud")
    amounts, ssa, asym = [air.amounts, cloud.amounts], [1.0, 0.9], [0.0, 0.85]
    lev = atm.levelTemperatures()
    T = [t for pair in zip(lev[:-1], lev[1:]) for t in pair]
    mu0 = 0.5
    slant = model.solarSlants(depth, mu0)

    def workspace(sizing):
        tile = sizing(nl, 1)
        doubles = min(sizing(nl, n), model.TWOSTREAM_WORKSPACE_BYTES // 8 // tile * tile)
        return ctx.buffer(doubles), dict(workspace_bytes=8 * doubles, passes=-(-n // (doubles // tile * 256)))

    work5, info5 = workspace(ctx.column_twostream_workspace)
    work4, info4 = workspace(ctx.column_radiance_scatter_workspace)
    sigma, S0 = ctx.buffer(n).upload(air.extinction), ctx.buffer(n).fill(1.0)
    level, rad = ctx.buffer(3 * (nl + 1)), ctx.buffer(16 * n)
    bufs = [work5, work4, sigma, S0, level, rad]
    scat = (amounts, [sigma, 1.0], ssa, asym, 1)
    calls = {"twostream": lambda: ctx.column_twostream_dev(kbufs, depth, lo, hi, n, S0, [mu0], slant, *scat, [0], [n], work5,
                                                           level, emissivity=0.9)}
    for v, views in VIEWS.items():
        mus, downs = [m for m, _ in views], [d for _, d in views]
        calls["beam_%d" % v] = lambda mus=mus, downs=downs: ctx.column_beam_radiance_dev(
            kbufs, depth, lo, hi, n, S0, mu0, slant, *scat, mus, downs, work5, rad, emissivity=0.9)
        calls["thermal_%d" % v] = lambda mus=mus, downs=downs: ctx.column_radiance_scatter_dev(
            kbufs, T, 1, depth, lo, hi, n, *scat, mus, downs, work4, rad, emissivity=0.9, surface_T=Ts)
    head = {"lib": _native.LIB_PATH, "device": ctx.device_info()["name"], "layers": nl, "points": n,
            "workspace": {"twostream, beam": info5, "thermal": info4}}
    print(json.dumps(head), flush=True)
    ms = {which: [] for which in LEGS}
    try:
        for _ in range(args.rounds):
            for which in LEGS:
                ms[which] += event_ms(ctx, calls[which], args.reps)
                print(json.dumps({"leg": which, "ms": ms[which][-args.reps:]}), flush=True)
    finally:
        for b in bufs:
            b.free()
    summary = {w: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), windows=len(t)) for w, t in ms.items()}
    med = lambda w: summary[w]["median_ms"]
    for v in VIEWS:
        summary["beam_%d" % v]["over_twostream"] = med("beam_%d" % v) / med("twostream")
        summary["beam_%d" % v]["over_thermal"] = med("beam_%d" % v) / med("thermal_%d" % v)
    summary["ms_per_added_view"] = {f: {"1_to_4": (med(f + "_4") - med(f + "_1")) / 3, "1_to_16": (med(f + "_16") - med(f + "_1")) / 15}
                                    for f in ("beam", "thermal")}
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"head": head, "ms": ms, "summary": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
