"""Writes tests/golden/V0_voigt.npz: what the true-Voigt tests compare with (tests/test_voigt_cpu.py, tests/test_gpu_voigt.py).

    python tests/golden/make_voigt_golden.py [output directory]

Two parts, both from scipy.special.wofz (the GPU tests run where SciPy may be missing, hence a fixture):

* the function K(x, y) = Re w(x + i y) on a table (f*), on seeded random pairs (r*) and in dense bands across the
  switch-overs of pyrad_amd/csrc/lbl_voigt_func.h (b*; the boundaries are read from the header's #defines);
* cross sections of small cells: oracle.pyrad_oracle.create_cross_section - line_quantities, intensityFactor, the scatter
  geometry, the regrid - with its _right_curve replaced by wofz((x + 1j lhw) / ghw).real / (ghw sqrt(pi)).

The cells (CASES) are small enough for the Python oracle and chosen for what can break in the accumulate kernel: see each
one's comment.  Everything is seeded: running the script twice gives the same file, byte for byte in its arrays.
"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import pyrad_oracle as orc          # noqa: E402
from pyrad_amd import synthetic                 # noqa: E402

NAME = "V0_voigt.npz"
FLOOR = 1e-290            # where the true value is below it, any result in [0, FLOOR] is right
RTOL_FUNCTION = 1e-6      # the function's contract (lbl_voigt_func.h)


def boundaries():
    """{name: s} of the header's switch-overs in s = x^2 + y^2"""
    with open(os.path.join(REPO, "pyrad_amd", "csrc", "lbl_voigt_func.h")) as f:
        text = f.read()
    return {m.group(1): float(m.group(2)) for m in re.finditer(r"#define\s+LBL_VOIGT_(S_\w+)\s+([0-9.eE+-]+)", text)}


def table_axes():
    x = np.concatenate([[0.0], np.logspace(-3, 5, 400)])
    y = np.concatenate([[0.0], np.logspace(-5, 4, 37)])
    return x, y


def random_pairs(n, seed=20240):
    rng = np.random.default_rng(seed)
    x = 10.0 ** rng.uniform(-3, 5, n)
    y = 10.0 ** rng.uniform(-5, 4, n)
    x[:: 50] = 0.0
    y[25:: 50] = 0.0
    return x, y


def band_points():
    """+-1 % in 200 steps across every switch-over, walking x at fixed y and y at fixed x"""
    xs, ys = [], []
    t = np.linspace(0.99, 1.01, 201)
    for s in boundaries().values():
        for y in (1e-5, 1e-3, 1e-1, 1.0, 5.0):
            if y * y < s:
                xs.append(np.sqrt(s - y * y) * t)
                ys.append(np.full(t.size, y))
        for x in (0.0, 1.0, 5.0):
            if x * x < s:
                ys.append(np.sqrt(s - x * x) * t)
                xs.append(np.full(t.size, x))
    return np.concatenate(xs), np.concatenate(ys)


def check_function(got, ref, what=""):
    """The function's contract against reference values: relative error <= RTOL_FUNCTION where the true value is at least
    FLOOR, a result in [0, FLOOR] below it, never negative.  Returns the worst relative error."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert not np.isnan(got).any(), what
    assert np.all(got >= 0), "%s: negative value" % what
    small = ref < FLOOR
    assert np.all(got[small] <= FLOOR), "%s: above the floor where the true value is below it" % what
    err = np.abs(got[~small] - ref[~small]) / ref[~small]
    worst = float(err.max()) if err.size else 0.0
    assert worst <= RTOL_FUNCTION, "%s: relative error %.3e" % (what, worst)
    return worst


# ---- the cells ---------------------------------------------------------------------------------------------------------
def _lines(seed, n, lo, hi, **scale):
    L = synthetic.make_lines(seed, n, lo, hi)
    for k, f in scale.items():
        L[k] = L[k] * f
    return L


def _concat(*lists):
    out = {f: np.concatenate([np.asarray(L[f]) for L in lists]) for f in lists[0]}
    order = np.argsort(out["nu"], kind="stable")
    return {f: v[order] for f, v in out.items()}


def _empty():
    return {f: np.zeros(0) for f in synthetic.make_lines(1, 2, 600, 601)}


def cases():
    """name -> dict(lines, T, P, q, lo, hi, base_resolution, dynamic).  All CO2 (molmass, partition sums of
    pyrad_amd.synthetic); at most 200 lines and 6,000 work points each."""
    c = {}
    # W = 500, y about 75-150; lines from below range_min and above range_max reach in; 4,000 points: no multiple of the
    # workgroup's 512; 110 lines inside 619-623, more than one LDS chunk of 64 in every window there; five lines on one
    # centre index (620.500 .. 620.509 at 0.01)
    five = _lines(7, 5, 600, 640)
    five["nu"] = 620.5 + np.array([0.0011, 0.0032, 0.0051, 0.0074, 0.0093])
    c["surface"] = dict(lines=_concat(_lines(1, 80, 594, 646), _lines(2, 110, 619, 623), five),
                        T=296.0, P=1013.25, lo=600, hi=640, base_resolution=.01, dynamic=True)
    # W = 50, y about 10; lines up to 1.5 cm^-1 outside the range: wings that reach in, and whole windows that miss the grid
    c["p100"] = dict(lines=_concat(_lines(3, 150, 598.5, 641.5), _lines(4, 20, 598.5, 600.0), _lines(5, 20, 640.0, 641.5)),
                     T=250.0, P=100.0, lo=600, hi=640, base_resolution=.01, dynamic=True)
    # resolution multiplier 0.1.  1 mbar: W = 5, y about 0.1 and (half the lines, widths x 0.002) 2e-4
    c["p1"] = dict(lines=_concat(_lines(6, 100, 599.99, 605.01), _lines(8, 100, 599.99, 605.01, gamma_air=.002, gamma_self=.002)),
                   T=220.0, P=1.0, lo=600, hi=605, base_resolution=.001, dynamic=True)
    # 0.05 mbar: W = 1 (the centre point alone), y about 5e-3 and (widths x 0.02) 1e-4
    c["p005"] = dict(lines=_concat(_lines(9, 100, 600, 605), _lines(10, 100, 600, 605, gamma_air=.02, gamma_self=.02)),
                     T=200.0, P=0.05, lo=600, hi=605, base_resolution=.001, dynamic=True)
    # y exactly 0: no pressure broadening at all (W = 5: x up to 3 xs, about 5)
    c["doppler"] = dict(lines=_lines(11, 150, 599.99, 605.01, gamma_air=0.0, gamma_self=0.0),
                        T=296.0, P=1.0, lo=600, hi=605, base_resolution=.001, dynamic=True)
    # work grid (0.01) coarser than the base grid (0.001): 500 work points regridded onto 5,000; H = 498 of 500
    c["regrid"] = dict(lines=_lines(12, 60, 596, 609), T=296.0, P=1013.25, lo=600, hi=605, base_resolution=.001, dynamic=True)
    # fewer than 64 points (50), H = 48
    c["tiny"] = dict(lines=_lines(13, 30, 599.6, 600.9), T=296.0, P=100.0, lo=600, hi=600.5, base_resolution=.01, dynamic=True)
    # H (498) larger than the grid (200 points)
    c["wide"] = dict(lines=_lines(14, 40, 596, 606), T=296.0, P=1013.25, lo=600, hi=602, base_resolution=.01, dynamic=True)
    # one isolated line (H = 48): a dropped or an extra edge point shows at full size, everything else is exactly zero
    one = _lines(15, 1, 600, 640)
    one["nu"] = np.array([620.003])
    c["isolated"] = dict(lines=one, T=296.0, P=100.0, lo=600, hi=640, base_resolution=.01, dynamic=True)
    c["empty"] = dict(lines=_empty(), T=296.0, P=100.0, lo=600, hi=640, base_resolution=.01, dynamic=True)
    for v in c.values():
        v["q"] = 4e-4
    return c


def case_physics(case):
    """(molmass, Q(T), Q(296), grid) of a cell"""
    sp = synthetic.SPECIES["co2"]
    g = orc.layer_grid(case["P"], case["lo"], case["hi"], case["base_resolution"], case["dynamic"])
    return sp["molmass"], synthetic.q_value("co2", int(case["T"])), sp["q296"], g


def voigt_curve(regime, ghw, lhw, xValues):
    from scipy.special import wofz
    return wofz((xValues + 1j * lhw) / ghw).real / (ghw * np.sqrt(np.pi))


def voigt_cross_section(case):
    molmass, q_T, q296, g = case_physics(case)
    keep = orc._right_curve
    orc._right_curve = voigt_curve
    try:
        xs, _ = orc.create_cross_section(case["lines"], case["T"], case["P"], case["q"], molmass, q_T, q296, g)
    finally:
        orc._right_curve = keep
    return xs


def build():
    from scipy.special import wofz
    out = {}
    fx, fy = table_axes()
    out["fx"], out["fy"] = fx, fy
    out["fK"] = wofz(fx[:, None] + 1j * fy[None, :]).real
    rx, ry = random_pairs(2000)
    out["rx"], out["ry"], out["rK"] = rx, ry, wofz(rx + 1j * ry).real
    bx, by = band_points()
    out["bx"], out["by"], out["bK"] = bx, by, wofz(bx + 1j * by).real
    cs = cases()
    out["cases"] = np.array(json.dumps(list(cs)))
    for name, case in cs.items():
        for f, v in case["lines"].items():
            out["%s.%s" % (name, f)] = np.ascontiguousarray(v, dtype=np.float64)
        out["%s.params" % name] = np.array([case["T"], case["P"], case["q"], case["lo"], case["hi"], case["base_resolution"],
                                            1.0 if case["dynamic"] else 0.0])
        out["%s.xsec" % name] = voigt_cross_section(case)
    return out


def load_case(z, name):
    """a cell of the fixture as cases() describes it, with its expected cross section"""
    T, P, q, lo, hi, base, dyn = (float(v) for v in z["%s.params" % name])
    lines = {f: np.ascontiguousarray(z["%s.%s" % (name, f)]) for f in synthetic.FIELDS}
    return dict(lines=lines, T=T, P=P, q=q, lo=lo, hi=hi, base_resolution=base, dynamic=bool(dyn), xsec=z["%s.xsec" % name])


def main(outdir=HERE):
    path = os.path.join(outdir, NAME)
    np.savez_compressed(path, **build())
    return path


if __name__ == "__main__":
    print(main(sys.argv[1] if len(sys.argv) > 1 else HERE))
