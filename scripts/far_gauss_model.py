"""CPU model of the far lines whose Gaussian part still reaches a span of the far-field kernel (K2, R = 4: spans of 256 points).

A record at least 4 half-spans (512 points) from a span's centre is a far line: its Lorentz term goes through the series.
Where its Gaussian part still reaches the span (K1's cut-off ``dgi``) that part has to be evaluated too - either by the
four-point pass of the far loop (51 wave-instructions per record, two exp per four points) or, since the records inside
8 half-spans are routed there, by the transposed runs of the near walk (142 per eight records with 32-point runs).

``gauss_cutoff`` restates K1's formulas for a = hw / res and dgi in NumPy (double precision where K1 uses single with a
margin: the counts of pairs agree except for records within a point of the cut-off); ``far_gauss_pairs`` counts the
(record, span) pairs of the class per span; run as a program it prints the counts and the instruction model for the
bench's C3 cell:

    python scripts/far_gauss_model.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SPAN = 256              # points per span (R = 4)
FAR = 4                 # half-spans from the span centre at which a line is far (FF_FAR)
CAP = 8                 # half-spans inside which a far record's Gaussian part goes to the near walk (FF_GAUSS_CAP)
GAUSS_CUT = 2.0 ** 54   # exact mode: the Gaussian part counts while it is above 2^-54 of the Lorentz part


def gauss_cutoff(lhw, ghw, ratio, res):
    """K1's profile width a (points) and Gaussian cut-off dgi (points, floored; 0: no Gaussian part that is cut against a
    Lorentz part) of pseudo-Voigt lines, from the oracle's line_quantities."""
    pv = (ratio >= .01) & (ratio <= 100.0)
    g, l = 2 * ghw, 2 * lhw
    f = (g**5 + 2.69269 * g**4 * l + 2.42843 * g**3 * l**2 + 4.47163 * g**2 * l**3 + .07842 * g * l**4 + l**5) ** .2
    x = l / f
    eta = 1.36603 * x - .47719 * x * x + .11116 * x**3
    a = np.where(pv, f / 2, np.where(ratio > 100, lhw, ghw)) / res
    # KG / (KL b) = (1 - eta) / eta * sqrt(pi): the ratio of the two parts at the centre; u^2 = v + 1, v = ln C + ln(1 + v)
    with np.errstate(divide="ignore", invalid="ignore"):
        C = np.abs((1 - eta) / eta) * np.sqrt(np.pi) * GAUSS_CUT
    dgi = np.zeros_like(a)
    ok = pv & (C > 1)
    lnC = np.log(C[ok])
    v = lnC.copy()
    for _ in range(3):
        v = lnC + np.log1p(v)
    dgi[ok] = np.floor(np.sqrt(v * 1.00001 + 1.01) * 1.000001 * a[ok] + 2)
    return a, dgi


def cell_records(lines, T, P, conc, molmass, grid):
    """(centre index, dgi) of a line list on a layer grid, sorted by centre as K1 leaves them."""
    from oracle import pyrad_oracle as orc
    lq = orc.line_quantities(lines, T, P, conc, molmass, grid["range_min"], grid["resolution"])
    _, dgi = gauss_cutoff(lq["lhw"], lq["ghw"], lq["ratio"], grid["resolution"])
    idx = lq["index"].astype(np.int64)
    o = np.argsort(idx, kind="stable")
    return idx[o], dgi[o]


def far_gauss_pairs(idx, dgi, n_work):
    """Per span of 256 points: the far records whose Gaussian part reaches it, inside and beyond the cap, by side.
    -> dict of int arrays (one entry per span): inside_left, inside_right, beyond, near (lines nearer than FAR half-spans)."""
    nspan = (n_work + SPAN - 1) // SPAN
    out = {k: np.zeros(nspan, np.int64) for k in ("inside_left", "inside_right", "beyond", "near")}
    for s in range(nspan):
        wlo, whi = s * SPAN, min(s * SPAN + SPAN - 1, n_work - 1)
        dist = np.maximum(0, np.maximum(idx - whi, wlo - idx))
        dc2 = np.abs(2 * (idx - wlo) - (SPAN - 1))                 # 2 |c - xc|, an odd integer
        far = dc2 >= 2 * FAR * (SPAN // 2)
        gf = (dist < dgi) & far
        inside = gf & (dc2 < 2 * CAP * (SPAN // 2))
        out["inside_left"][s] = (inside & (idx < wlo)).sum()
        out["inside_right"][s] = (inside & (idx > whi)).sum()
        out["beyond"][s] = (gf & ~inside).sum()
        out["near"][s] = (~far).sum()
    return out


def _passes(first, last, idx, dgi, wlo, whi, per_pass=8):
    """run passes and staged chunks of a near walk over the records [first, last)"""
    tot = chunks = 0
    for c0 in range(first, last, 64):
        c1 = min(c0 + 64, last)
        dist = np.maximum(0, np.maximum(idx[c0:c1] - whi, wlo - idx[c0:c1]))
        tot += -(-int((dist < dgi[c0:c1]).sum()) // per_pass)
        chunks += 1
    return tot, chunks


def main():
    from pyrad_amd import synthetic
    from oracle import pyrad_oracle as orc
    cfg = synthetic.config_c3()
    grid = orc.layer_grid(cfg["P"], cfg["range_min"], cfg["range_max"], cfg["base_resolution"], cfg.get("dynamic_resolution", True))
    recs = []
    for mol in cfg["molecules"]:
        sp = synthetic.SPECIES[mol["species"]]
        lines = orc.select_window(mol["lines"], grid["eff_min"], grid["eff_max"])
        recs.append(cell_records(lines, cfg["T"], cfg["P"], orc.concentration(**mol["conc"]), sp["molmass"], grid))
    idx = np.concatenate([r[0] for r in recs])
    dgi = np.concatenate([r[1] for r in recs])
    o = np.argsort(idx, kind="stable")
    idx, dgi = idx[o], dgi[o]
    n = grid["n_work"]
    nspan = (n + SPAN - 1) // SPAN
    print("C3: %d records, %d spans, dgi median %.0f points" % (len(idx), nspan, np.median(dgi[dgi > 0])))
    half = SPAN // 2
    run = far = 0
    hist = []
    old_p = new_p = old_c = new_c = far_recs = far_chunks = 0
    sample = range(0, nspan, 7)
    for s in range(nspan):
        wlo, whi = s * SPAN, min(s * SPAN + SPAN - 1, n - 1)
        lo, hi = np.searchsorted(idx, wlo - 5000), np.searchsorted(idx, whi + 5000)
        ci, dg = idx[lo:hi], dgi[lo:hi]
        dist = np.maximum(0, np.maximum(ci - whi, wlo - ci))
        isfar = (ci <= wlo + half - 1 - FAR * half) | (ci >= wlo + half + FAR * half)
        g = dist < dg
        hist.append(int((g & isfar).sum()))
        far += hist[-1]
        run += int((g & ~isfar).sum())
        if s not in sample:
            continue
        iF1 = int(np.searchsorted(idx, wlo + half - FAR * half))
        iF2 = int(np.searchsorted(idx, wlo + half + FAR * half))
        k = np.nonzero(g & (np.abs(2 * (ci - wlo) - (SPAN - 1)) < 2 * CAP * half))[0] + lo
        kfar = k[(k < iF1) | (k >= iF2)]
        far_recs += len(kfar)
        iG1 = min(iF1, int(k.min())) if len(k) else iF1
        iG2 = max(iF2, int(k.max()) + 1) if len(k) else iF2
        p, c = _passes(iF1, iF2, idx, dgi, wlo, whi); old_p += p; old_c += c
        p, c = _passes(iG1, iG2, idx, dgi, wlo, whi); new_p += p; new_c += c
        far_chunks += len(set((int(j) - lo) // 64 for j in kfar[kfar < iF1])) + len(set((int(j) - iF2) // 64 for j in kfar[kfar >= iF2]))
    hist = np.array(hist)
    m = len(sample)
    print("Gaussian (record, span) pairs per span: near walk %.1f, far lines %.1f (median %d, 90th percentile %d, max %d, none in %.0f %% of the spans)"
          % (run / nspan, far / nspan, np.median(hist), np.percentile(hist, 90), hist.max(), 100 * (hist == 0).mean()))
    print("every 7th span: %.1f far records inside the cap in %.2f far chunks; run passes %.2f -> %.2f, staged near chunks %.2f -> %.2f"
          % (far_recs / m, far_chunks / m, old_p / m, new_p / m, old_c / m, new_c / m))
    old_cost = far_recs / m * 53 + far_chunks / m * 25
    new_cost = (new_p - old_p) / m * 142 + (new_c - old_c) / m * 40
    print("wave-instructions per span: four-point pass %.0f, through the runs %.0f, saved %.0f" % (old_cost, new_cost, old_cost - new_cost))


if __name__ == "__main__":
    main()
