#!/usr/bin/env python3
"""Times Atmosphere.kDistribution on the config-5 column of scripts/flux_time.py (30 layers x 2.4e6 points), G = 16, for one
band of the whole range and for ten equal bands, with reference=None (every layer ranked by itself) and reference=0 (one
sort, 30 gathers): the call with every absorption coefficient resident, and what it replaces on the same box - the
getAbsCoef downloads, numpy.argsort(kind="stable") per layer and band and the same means in NumPy.  Each call returns host
arrays, so its wall time is device-synchronised.  Two warm-up calls, then the median of `--reps` (the host legs run once).
Run on the GPU box; the per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script with
--skip-host."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flux_time import column, timed  # noqa: E402
from pyrad_amd import _native, model  # noqa: E402


def host_kdist(k, first, count, edges, reference):
    """the definition in NumPy on downloaded rows: (L, G) means per band"""
    out = []
    for f, c, e in zip(first, count, edges):
        orders = {}
        mean = np.empty((len(k), e.size - 1))
        for l, row in enumerate(k):
            r = l if reference is None else reference
            if r not in orders:
                orders[r] = f + np.argsort(k[r][f:f + c], kind="stable")
            mean[l] = np.add.reduceat(row[orders[r]], e[:-1]) / np.diff(e)
            if reference is None:
                orders.clear()
        out.append(mean)
    return out


def once(fn):
    t0 = time.perf_counter()
    v = fn()
    return 1e3 * (time.perf_counter() - t0), v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-host", action="store_true", help="only the kDistribution() calls (profiler runs)")
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    atm, Ts = column()
    lo, hi = atm[0].rangeMin, atm[0].rangeMax
    atm.transmission(surfaceTemperature=Ts)             # first call: uploads, schedules, every absorption coefficient resident
    n = int(atm[0].xAxis.size)
    ten = [(lo + (hi - lo) * i / 10.0, lo + (hi - lo) * (i + 1) / 10.0 + (1.0 if i == 9 else 0.0)) for i in range(10)]
    res = {"layers": len(atm), "points": n, "intervals": 16, "tile": _native.KDIST_TILE}
    fmt = lambda m: dict(median=m[0], min=m[1])
    for name, bands in (("one_band", None), ("ten_bands", ten)):
        for ref in (None, 0):
            key = "%s_reference_%s" % (name, ref)
            res[key + "_ms"] = fmt(timed(lambda: atm.kDistribution(bands=bands, g=16, reference=ref), args.reps))
    if not args.skip_host:
        ms, k = once(lambda: [np.array(model.getAbsCoef(L)) for L in atm])
        res["getAbsCoef_downloads_ms"] = ms
        for name, bands in (("one_band", None), ("ten_bands", ten)):
            first, count = model._flux_bands(lo, hi, n, bands)
            edges = [model.gIntervals(16, c) for c in count]
            for ref in (None, 0):
                ms, want = once(lambda: host_kdist(k, first, count, edges, ref))
                res["numpy_%s_reference_%s_ms" % (name, ref)] = ms
                kd = atm.kDistribution(bands=bands, g=16, reference=ref)
                got = [kd.k] if bands is None else kd.k
                res["%s_reference_%s_max_rel_diff" % (name, ref)] = float(max(
                    np.max(np.abs(g - w) / np.abs(w)) for g, w in zip(got, want)))
    for key, v in res.items():
        print("%-44s %s" % (key, ("%.3f ms (min %.3f)" % (v["median"], v["min"])) if isinstance(v, dict) else v))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
