"""Writes tests/golden/V1_voigt_dT.npz: what the dk/dT tests compare with (tests/test_voigt_dT_cpu.py, tests/test_gpu_voigt_dT.py).

    python tests/golden/make_voigt_dT_golden.py [output directory]

Everything comes from mpmath at DPS digits: w = exp(-z^2) erfc(-i z) and w' = -2 z w + 2 i / sqrt(pi), whose cancellation
in the far field (about 1e-16 s in fp64) is harmless at that precision.

* the function: K = Re w, GX = x dK/dx = x Re w', GY = y dK/dy = -y Im w' on make_voigt_golden's table (f*), random pairs
  (r*) and bands across the switch-overs (b*): the points are V0's, imported, and not stored again;
* the cells: for each of make_voigt_golden.cases() (the lines stay in V0_voigt.npz) the temperature derivative of the
  cross section on the base grid, "<cell>.dxsec", with dlnw_dT = -beta / T (pyrad_amd.synthetic's Q(T) = Q296 (T / 296)^beta),
  over the scatter geometry of oracle.pyrad_oracle (centre indices, window, regrid); "<cell>.scale" =
  sum_lines amp K (|a| + (|n_air| + 1) / T) and "<cell>.abs3" = sum_lines (|amp a K| + |amp bx GX| + |amp by GY|), both
  through the same regrid (its weights are non-negative, so a pointwise bound survives it).

Per pair the derivative is the chain rule  amp (a K + bx GX + by GY)  with
    a = -beta / T + c2 E / T^2 - (c2 nu' / T^2) / expm1(c2 nu' / T) - 1 / (2 T),   bx = -1 / (2 T),   by = -(n_air + 1/2) / T
and the generator checks it on SELFCHECK seeded pairs per cell against mpmath.diff of the whole per-pair expression in T
(intensity factor, widths, w itself): that check knows none of the formulas above.

Seeded and reproducible; the work is spread over the machine's cores, the sums are formed in one fixed order.
"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mpmath                                   # noqa: E402
from mpmath import mpf, mpc                     # noqa: E402

import make_voigt_golden as mvg                 # noqa: E402
from oracle import pyrad_oracle as orc          # noqa: E402
from pyrad_amd import synthetic                 # noqa: E402

NAME = "V1_voigt_dT.npz"
DPS = 50
SELFCHECK = 200
SELFCHECK_RTOL = 1e-20
RTOL = 1e-6               # the contract of voigt_kgrad: |dK|, |dGX|, |dGY| <= RTOL K wherever K >= mvg.FLOOR
mpmath.mp.dps = DPS


def w_grad(x, y):
    """(K, GX, GY) at one point, mpf"""
    x, y = mpf(x), mpf(y)
    z = mpc(x, y)
    w = mpmath.exp(-z * z) * mpmath.erfc(mpc(y, -x))
    wp = -2 * z * w + mpc(0, 2) / mpmath.sqrt(mpmath.pi)
    return w.real, x * wp.real, -y * wp.imag


def _w_grad_f(xy):
    return tuple(float(v) for v in w_grad(*xy))


def function_values(pool, x, y):
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    got = np.array(pool.map(_w_grad_f, list(zip(x.ravel().tolist(), y.ravel().tolist())), chunksize=64)).reshape(x.shape + (3,))
    return got[..., 0], got[..., 1], got[..., 2]


def check_gradient(K, GX, GY, ref, what=""):
    """voigt_kgrad's contract against (K, GX, GY) reference arrays; returns the three worst errors over K"""
    rK, rGX, rGY = (np.asarray(v, dtype=np.float64) for v in ref)
    K, GX, GY = (np.asarray(v, dtype=np.float64) for v in (K, GX, GY))
    worst_k = mvg.check_function(K, rK, what)
    assert not (np.isnan(GX).any() or np.isnan(GY).any()), what
    assert np.all(GX <= 0), "%s: positive GX" % what
    big = rK >= mvg.FLOOR
    out = [worst_k]
    for name, got, ref_ in (("GX", GX, rGX), ("GY", GY, rGY)):
        err = np.abs(got[big] - ref_[big]) / rK[big]
        worst = float(err.max()) if err.size else 0.0
        assert worst <= RTOL, "%s: %s error over K %.3e" % (what, name, worst)
        out.append(worst)
    return tuple(out)


# ---- the cells ---------------------------------------------------------------------------------------------------------
def line_constants(case, i):
    """what a line's pair expression needs, as exact (mpf) images of the fp64 inputs"""
    L = case["lines"]
    sp = synthetic.SPECIES["co2"]
    return dict(nu=mpf(float(L["nu"][i])), sw=mpf(float(L["sw"][i])), E=mpf(float(L["elower"][i])),
                ga=mpf(float(L["gamma_air"][i])), gs=mpf(float(L["gamma_self"][i])), n=mpf(float(L["n_air"][i])),
                delta=mpf(float(L["delta_air"][i])), P=mpf(case["P"]), q=mpf(case["q"]), molmass=mpf(sp["molmass"]),
                q296=mpf(sp["q296"]), beta=mpf(sp["beta"]))


def line_state(c, T):
    """(nu', ghw, lhw, amp) of a line at temperature T: pyradClasses.py:252-263, pyradIntensity.py:16-32 in mpf"""
    c2, t0, p0 = mpf(orc.c2), mpf(orc.t0), mpf(orc.p0)
    nus = c["nu"] + c["delta"] * c["P"] / p0
    lhw = ((1 - c["q"]) * c["ga"] + c["q"] * c["gs"]) * (c["P"] / p0) * (t0 / T) ** c["n"]
    m = c["molmass"] / 1000 / mpf(orc.avo)
    ghw = nus * mpmath.sqrt(2 * mpf(orc.k) * T / m / mpf(orc.c) ** 2)
    qT = c["q296"] * (T / 296) ** c["beta"]
    stim = (1 - mpmath.exp(-c2 * nus / T)) / (1 - mpmath.exp(-c2 * nus / t0))
    boltz = mpmath.exp(-c2 * c["E"] / T) / mpmath.exp(-c2 * c["E"] / t0)
    amp = c["sw"] * (c["q296"] / qT) * stim * boltz / (ghw * mpmath.sqrt(mpmath.pi))
    return nus, ghw, lhw, amp


def pair_value(c, T, dist):
    """one line's contribution at distance dist (cm^-1) from its centre point, at temperature T"""
    _, ghw, lhw, amp = line_state(c, T)
    z = mpc(dist / ghw, lhw / ghw)
    return amp * (mpmath.exp(-z * z) * mpmath.erfc(mpc(z.imag, -z.real))).real


def line_derivative(c, T):
    """(xs per cm^-1, y, amp, a, bx, by) of the chain rule"""
    T = mpf(T)
    nus, ghw, lhw, amp = line_state(c, T)
    c2 = mpf(orc.c2)
    u = c2 * nus / T
    a = -c["beta"] / T + c2 * c["E"] / T ** 2 - (c2 * nus / T ** 2) / mpmath.expm1(u) - 1 / (2 * T)
    return 1 / ghw, lhw / ghw, amp, a, -1 / (2 * T), -(c["n"] + mpf(1) / 2) / T


def pair_terms(c, T, dist):
    """(derivative, scale term, three-term absolute sum) of one pair"""
    inv_ghw, y, amp, a, bx, by = line_derivative(c, T)
    K, GX, GY = w_grad(abs(dist) * inv_ghw, y)
    return (amp * (a * K + bx * GX + by * GY), amp * K * (abs(a) + (abs(c["n"]) + 1) / mpf(T)),
            amp * (abs(a * K) + abs(bx * GX) + abs(by * GY)))


def cell_geometry(case):
    g = mvg.case_physics(case)[3]
    lq = orc.line_quantities(case["lines"], case["T"], case["P"], case["q"], synthetic.SPECIES["co2"]["molmass"],
                             g["range_min"], g["resolution"])
    return g, lq["index"].astype(np.int64), max(g["W"] - 2, 0)


def _line_task(args):
    case, i, cidx, H, n_work, res = args
    c = line_constants(case, i)
    lo, hi = max(cidx - H, 0), min(cidx + H, n_work - 1)
    out = []
    for p in range(lo, hi + 1):
        out.append(pair_terms(c, case["T"], abs(p - cidx) * res))
    return lo, out


def cell_arrays(pool, case):
    """(dxsec, scale, abs3) of a cell on its base grid"""
    g, cidx, H = cell_geometry(case)
    n = g["n_work"]
    tasks = [(case, i, int(cidx[i]), H, n, g["resolution"]) for i in range(len(cidx))
             if not (cidx[i] + H < 0 or cidx[i] - H > n - 1)]
    sums = [[mpf(0)] * n for _ in range(3)]
    for lo, terms in pool.map(_line_task, tasks, chunksize=1):
        for k, t in enumerate(terms):
            for j in range(3):
                sums[j][lo + k] = sums[j][lo + k] + t[j]
    return tuple(orc.regrid_to_base(np.array([float(v) for v in s]), g) for s in sums)


def _selfcheck_task(args):
    case, i, dist = args
    c = line_constants(case, i)
    chain = pair_terms(c, case["T"], dist)[0]
    direct = mpmath.diff(lambda T: pair_value(c, T, dist), mpf(case["T"]))
    return float(abs(chain - direct) / abs(direct)) if direct != 0 else float(abs(chain))


def selfcheck(pool, name, case, n_pairs):
    """chain rule against mpmath.diff of the whole per-pair expression; returns the worst relative difference"""
    g, cidx, H = cell_geometry(case)
    if len(cidx) == 0 or n_pairs == 0:
        return 0.0
    rng = np.random.default_rng(sum(name.encode()) + 4711)
    lines = rng.integers(0, len(cidx), n_pairs)
    d = rng.integers(0, H + 1, n_pairs)
    worst = max(pool.map(_selfcheck_task, [(case, int(i), float(k) * g["resolution"]) for i, k in zip(lines, d)], chunksize=4))
    assert worst <= SELFCHECK_RTOL, "%s: chain rule against mpmath.diff: %.3e" % (name, worst)
    return worst


class _Serial:
    """multiprocessing.Pool's map in this process (processes=0: a test that must not fork)"""

    def map(self, f, items, chunksize=1):
        return [f(i) for i in items]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def build(cells=None, thin=1, selfcheck_pairs=SELFCHECK, processes=None):
    """The fixture's arrays.  cells: a subset by name; thin: every thin-th point of the function sets (the tests reproduce
    a part of the file in seconds); processes: worker processes (None: the machine's cores, at most 16; 0: none)."""
    out = {}
    with (_Serial() if processes == 0 else multiprocessing.Pool(processes or min(16, os.cpu_count() or 1))) as pool:
        fx, fy = mvg.table_axes()
        gx, gy = np.broadcast_arrays(fx[:, None], fy[None, :])
        shape = gx.shape
        gx, gy = gx.ravel()[::thin], gy.ravel()[::thin]
        vals = function_values(pool, gx, gy)
        for k, v in zip(("fK", "fGX", "fGY"), vals):
            out[k] = v if thin > 1 else v.reshape(shape)
        rx, ry = mvg.random_pairs(2000)
        bx, by = mvg.band_points()
        for tag, (x, y) in (("r", (rx, ry)), ("b", (bx, by))):
            for k, v in zip(("K", "GX", "GY"), function_values(pool, x[::thin], y[::thin])):
                out[tag + k] = v
        cs = mvg.cases()
        names = [n for n in cs if cells is None or n in cells]
        out["cases"] = np.array(json.dumps(names))
        worst = {}
        for name in names:
            worst[name] = selfcheck(pool, name, cs[name], selfcheck_pairs)
            out["%s.dxsec" % name], out["%s.scale" % name], out["%s.abs3" % name] = cell_arrays(pool, cs[name])
        print("chain rule against mpmath.diff, worst per cell: %s" % json.dumps(worst), file=sys.stderr)
    return out


def main(outdir=HERE):
    path = os.path.join(outdir, NAME)
    np.savez_compressed(path, **build())
    return path


if __name__ == "__main__":
    print(main(sys.argv[1] if len(sys.argv) > 1 else HERE))
