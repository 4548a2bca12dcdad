#!/usr/bin/env python3
"""Times Atmosphere.observe on the config-5 column of scripts/flux_time.py (30 layers x 2.4e6 points) for a Gaussian
instrument, FWHM 0.5 cm^-1, a channel every 0.25 cm^-1 over the range, default cutoff (about 9,600 channels with supports
of about 3,000 points): the call with every absorption coefficient resident, with and without Jacobians, and what it
replaces on the same box - transmission() / jacobians(spectra=True) and the same convolution of the downloaded rows in
NumPy.  Each call returns host arrays, so its wall time is device-synchronised.  Two warm-up calls, then the median of
`--reps` (the host legs run once).  Run on the GPU box; K8's kernel time comes from a separate `rocprofv3 --kernel-trace
--stats` run of this script with --skip-host, its FETCH_SIZE from a counters-only `--pmc FETCH_SIZE` run of the same."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flux_time import column, timed  # noqa: E402
from pyrad_amd import model  # noqa: E402


def host_convolve(ins, rows, lo, hi):
    """the definition of lbl_ils_convolve_dev in NumPy: one weight vector per channel, used for every row"""
    rows = np.atleast_2d(rows)
    n = rows.shape[1]
    step = (hi - lo) / (n - 1)
    position, first, count = ins.support(lo, hi, n)
    out = np.empty((rows.shape[0], len(ins)))
    for c in range(len(ins)):
        t = (np.arange(first[c], first[c] + count[c], dtype=np.float64) - position[c]) * step / ins.width[c]
        w = np.exp(-2.772588722239781 * (t * t))
        out[:, c] = rows[:, first[c]:first[c] + count[c]] @ w / w.sum()
    return out


def once(fn):
    t0 = time.perf_counter()
    v = fn()
    return 1e3 * (time.perf_counter() - t0), v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-host", action="store_true", help="only the observe() calls (profiler runs)")
    ap.add_argument("--out", default=None, help="also write the results as JSON here")
    args = ap.parse_args()
    atm, Ts = column()
    lo, hi = atm[0].rangeMin, atm[0].rangeMax
    fwhm = 0.5
    ins = model.Instrument(np.arange(lo + 3 * fwhm, hi - 3 * fwhm + 1e-9, 0.25), width=fwhm)
    toa = atm.transmission(surfaceTemperature=Ts)       # first call: uploads, schedules, every absorption coefficient resident
    n = int(atm[0].xAxis.size)
    _, _, count = ins.support(lo, hi, n)
    res = {"layers": len(atm), "points": n, "channels": len(ins), "support_points": int(np.median(count))}
    fmt = lambda m: dict(median=m[0], min=m[1])
    res["observe_ms"] = fmt(timed(lambda: atm.observe(ins, surfaceTemperature=Ts), args.reps))
    res["observe_jacobians_ms"] = fmt(timed(lambda: atm.observe(ins, surfaceTemperature=Ts, jacobians=True), args.reps))
    res["fluxes_1_angle_ms"] = fmt(timed(lambda: atm.fluxes(surfaceTemperature=Ts, angles=[(1.0, 1.0)]), args.reps))
    if not args.skip_host:
        res["transmission_resident_ms"] = fmt(timed(lambda: atm.transmission(surfaceTemperature=Ts), args.reps))
        ob = atm.observe(ins, surfaceTemperature=Ts, jacobians=True)
        ms, want = once(lambda: host_convolve(ins, toa, lo, hi))
        res["numpy_convolution_1_row_ms"] = ms
        res["radiance_max_rel_diff"] = float(np.max(np.abs(ob.radiance - want[0]) / np.abs(want[0])))
        ms, jac = once(lambda: atm.jacobians(surfaceTemperature=Ts, angles=[(1.0, 1.0)], molecules=False, spectra=True))
        res["jacobians_spectra_ms"] = ms
        ms, want = once(lambda: host_convolve(ins, jac.temperatureSpectrum, lo, hi))
        res["numpy_convolution_%d_rows_ms" % len(atm)] = ms
        scale = np.max(np.abs(want), axis=1, keepdims=True)
        res["temperature_jacobian_max_diff_over_row_max"] = float(np.max(np.abs(ob.temperatureJacobian - want) / scale))
    for key, v in res.items():
        print("%-44s %s" % (key, ("%.3f ms (min %.3f)" % (v["median"], v["min"])) if isinstance(v, dict) else v))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
