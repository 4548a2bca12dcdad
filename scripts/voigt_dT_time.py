#!/usr/bin/env python3
"""Times the Voigt temperature-derivative accumulate (lbl_xsec_voigt_dt_dev, K2v-T) beside the Voigt value accumulate
(lbl_xsec_voigt_dev, K2v) on BASELINE config 2: CO2, 500-900 cm^-1 at 0.001 cm^-1, 1 atm, 296 K, 65,536 synthetic lines as
bench.py makes them (one job; 400,000 points, window 5,000 points, about 6.5e8 (line, point) pairs).  Both run in ONE
library and one context, alternating call by call.

Times are the library's own HIP events on the context's stream around the accumulate launches (lbl_profile_read, class
"xsec_accumulate"; the line prep is read separately), `--warmup` untimed rounds, then the median and minimum of `--reps`
rounds.  Also prints a sanity check that both computed the same cell: d(sigma)/dT over sigma / T is a number of order 1 to
20 wherever sigma is not tiny.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrad_amd import _native as nat, engine, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lines", type=int, default=65536)
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    cfg = synthetic.config_c2(n_lines=args.lines)
    mol = cfg["molecules"][0]
    sp = synthetic.SPECIES[mol["species"]]
    g = engine.layer_grid(cfg["P"], cfg["range_min"], cfg["range_max"], cfg["base_resolution"], cfg["dynamic_resolution"])
    pairs = engine.eval_count(mol["lines"]["nu"], g["range_min"], g["resolution"], g["W"], g["n_work"])
    ctx = nat.Context(0)
    L = ctx.lines(mol["lines"])
    T = float(cfg["T"])
    iso = nat.IsoParams(T, cfg["P"], 400e-6, sp["molmass"], synthetic.q_value(mol["species"], cfg["T"]), sp["q296"])
    grid = engine.native_grid(g)
    order = ("voigt", "voigt_dT")
    out = {k: ctx.buffer(g["n_base"]) for k in order}

    def call(which):
        if which == "voigt":
            ctx.xsec_voigt_dev([(L, iso, grid, out[which])])
        else:
            ctx.xsec_voigt_dT_dev([(L, iso, grid, out[which])], [-sp["beta"] / T])

    for _ in range(max(args.warmup, 1)):
        for w in order:
            call(w)
    ctx.sync()
    ctx.profile_enable(["line_prep", "xsec_accumulate"])
    ctx.profile_reserve(4 * len(order) * (args.reps + 1))
    times = {w: dict(accumulate=[], prep=[]) for w in order}
    for _ in range(args.reps):
        for w in order:
            ctx.profile_reset()
            call(w)
            ctx.sync()
            p = ctx.profile_read()
            times[w]["accumulate"].append(p["xsec_accumulate"][1])
            times[w]["prep"].append(p["line_prep"][1])
    ctx.profile_enable(False)
    xs = {w: out[w].download(g["n_base"]) for w in order}
    res = dict(device=ctx.device_info()["name"], lines=int(args.lines), points=int(g["n_work"]), window=int(g["W"]), pairs=int(pairs),
               reps=args.reps)
    for w in order:
        acc, prep = np.array(times[w]["accumulate"]), np.array(times[w]["prep"])
        res[w] = dict(accumulate_ms_median=float(np.median(acc)), accumulate_ms_min=float(acc.min()),
                      prep_ms_median=float(np.median(prep)), pairs_per_s=float(pairs / (np.median(acc) * 1e-3)))
    res["dT_over_voigt_accumulate"] = res["voigt_dT"]["accumulate_ms_median"] / res["voigt"]["accumulate_ms_median"]
    with np.errstate(divide="ignore", invalid="ignore"):
        logd = np.abs(xs["voigt_dT"]) * T / xs["voigt"]
    res["dlnsigma_dlnT_median"] = float(np.nanmedian(logd))
    for w in order:
        r = res[w]
        print("%-9s accumulate %8.3f ms median (min %8.3f)   prep %6.3f ms   %.3e pairs/s"
              % (w, r["accumulate_ms_median"], r["accumulate_ms_min"], r["prep_ms_median"], r["pairs_per_s"]))
    print("pairs %d; derivative / value accumulate time %.3f; median |d ln sigma / d ln T| %.2f"
          % (pairs, res["dT_over_voigt_accumulate"], res["dlnsigma_dlnT_median"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    for b in out.values():
        b.free()
    L.free()
    ctx.close()


if __name__ == "__main__":
    main()
