#!/usr/bin/env python3
"""Every column transport entry point (K5c - K5k: fluxes, Jacobians, ray paths, reflecting surface, linear source, solar
beam) through _native.Context on synthetic, seeded absorption coefficients, every output saved as .npy (one file per call,
its outputs concatenated): run once per library build (PYRAD_HIP_LIB) and compare the files bit for bit
(scripts/bitcmp_libs.sh <lib a> <lib b> dump_transport.py).  No line lists are needed.  The shapes are the smallest at
which the kernels' frames can go wrong: bands with head, aligned and tail points, a band of three points, a grid-stride
second round in some workgroups only, every angle count on each side of the points-per-thread switch, both Planck paths,
bundled and single rays with a surface marker, a tail launch.  usage: dump_transport.py <out dir>"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrad_amd import _native as nat

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
if os.listdir(out):
    sys.exit("%s is not empty: files of an earlier dump would be compared with this one's" % out)
ctx =nat.Context(0)
rng = np.random.default_rng(20240917)
held = []
tally = [0, 0, 0]            # files, values, values that are finite and not zero


def dev(data):
    b = ctx.buffer(len(data), np.ascontiguousarray(data, dtype=np.float64))
    held.append(b)
    return b


def empty(n):
    b = ctx.buffer(int(n))
    b.fill(0.0)
    held.append(b)
    return b


def save(name, *bufs):
    """one file per call: the call's output buffers, concatenated"""
    ctx.sync()
    values = np.concatenate([b.download(b.n) for b in bufs])
    np.save(os.path.join(out, name + ".npy"), values)
    tally[0] += 1
    tally[1] += values.size
    tally[2] += int(np.count_nonzero(np.isfinite(values) & (values != 0.0)))


def angles(na):
    mu = [(k + 0.5) / na for k in range(na)]
    return mu, [2.0 * np.pi * m / na for m in mu]


class Column:
    """L layers of seeded absorption coefficients (optical depths 1e-3 .. 5 per layer) on n points from `lo` in steps of `res`"""
    def __init__(self, L, n, lo, res):
        self.L, self.n, self.lo, self.hi = L, n, lo, lo + (n - 1) * res
        self.depth = [1.0e5 * (l + 1) for l in range(L)]
        self.T = [288.0 - 20.0 * l for l in range(L)]
        self.edge_T = [(t + 8.0, t - 9.0) for t in self.T]
        self.k = [dev(np.exp(rng.uniform(np.log(1e-3), np.log(5.0), n)) / d) for d in self.depth]
        self.term_k = [dev(np.exp(rng.uniform(np.log(1e-4), np.log(1.0), n)) / self.depth[l]) for l in (0, L - 1)]
        self.term_layer = [0, L - 1]
        spectrum = rng.uniform(0.0, 0.2, n)
        spectrum[[1, n // 2]] = np.nan, np.inf          # nan_to_num in the level sums
        self.I_surface = dev(spectrum)
        self.I_top = dev(rng.uniform(0.0, 0.02, n))
        self.emissivity = dev(rng.uniform(0.5, 1.0, n))
        self.S0 = dev(rng.uniform(0.5, 1.5, n))

    def args(self):
        return self.lo, self.hi, self.n


def bands_of(n):
    # head + aligned + tail (starts off a multiple of 4, ends on one); 3 points, no aligned part; the whole grid
    return [5, 101, 0], [(n - 7) - 5, 3, n]


def column_calls(tag, c, na, surface):
    L, n = c.L, c.n
    mu, w = angles(na)
    first, count = bands_of(n)
    nb = len(first)
    src = dict(I_surface=c.I_surface) if surface == "spectrum" else dict(surface_T=291.5)
    levels = empty(nb * 2 * (L + 1))
    up_top, down_surface, up_surface = empty(n), empty(n), empty(n)
    tag = "%s_L%d_a%d_%s" % (tag, L, na, surface)
    # K5c
    ctx.column_flux_dev(c.k, c.T, c.depth, *c.args(), mu, w, first, count, levels, up_top=up_top, down_surface=down_surface,
                        I_top=c.I_top, **src)
    save(tag + "_flux", levels, up_top, down_surface)
    # K5g, K5i: emissivity as a number and as an array, both reflections, with and without the spectrum at the top
    for e_name, e in (("e0.7", 0.7), ("earr", c.emissivity)):
        for refl in (0, 1):
            for top in (None, c.I_top):
                t = "%s_%s_r%d_%s" % (tag, e_name, refl, "top" if top else "notop")
                ctx.column_flux_surface_dev(c.k, c.T, c.depth, *c.args(), mu, w, first, count, levels, e, refl, I_top=top,
                                            up_top=up_top, down_surface=down_surface, up_surface=up_surface, **src)
                save(t + "_surface", levels, up_top, down_surface, up_surface)
                ctx.column_flux_linear_dev(c.k, c.edge_T, c.depth, *c.args(), mu, w, first, count, levels, e, refl, I_top=top,
                                           up_top=up_top, down_surface=down_surface, up_surface=up_surface, **src)
                save(t + "_linear", levels, up_top, down_surface, up_surface)
    ctx.column_flux_linear_dev(c.k, [(t, t) for t in c.T], c.depth, *c.args(), mu, w, first, count, levels, c.emissivity, 0,
                               I_top=c.I_top, up_top=up_top, down_surface=down_surface, up_surface=up_surface, **src)
    save(tag + "_linear_equal", levels, up_top, down_surface, up_surface)
    # K5d, K5h, K5j: two terms on different layers and none, spectra on
    ln_tau, T_spec, T_edge, e_spec = empty(L * n), empty(L * n), empty(2 * L * n), empty(n)
    for terms in (0, 2):
        tk = dict(term_abs_coef=c.term_k[:terms], term_layer=c.term_layer[:terms])
        t = "%s_t%d" % (tag, terms)
        jac = empty(nb * (3 + 3 * L + terms))
        ctx.column_jacobian_dev(c.k, c.T, c.depth, *c.args(), mu, w, first, count, jac, ln_tau_spectra=ln_tau,
                                T_spectra=T_spec, **tk, **src)
        save(t + "_jacobian", jac, ln_tau, T_spec)
        for refl in (0, 1):
            ctx.column_jacobian_surface_dev(c.k, c.T, c.depth, *c.args(), mu, w, first, count, jac, c.emissivity, refl,
                                            I_top=c.I_top, ln_tau_spectra=ln_tau, T_spectra=T_spec, e_spectrum=e_spec, **tk,
                                            **src)
            save("%s_r%d_jacobian_surface" % (t, refl), jac, ln_tau, T_spec, e_spec)
            ctx.column_jacobian_linear_dev(c.k, c.edge_T, c.depth, *c.args(), mu, w, first, count, jac, 0.7, refl,
                                           I_top=c.I_top, ln_tau_spectra=ln_tau, T_edge_spectra=T_edge, e_spectrum=e_spec,
                                           **tk, **src)
            save("%s_r%d_jacobian_linear" % (t, refl), jac, ln_tau, T_edge, e_spec)


def solar_calls(tag, c):
    L, n = c.L, c.n
    first, count = bands_of(n)
    levels = empty(len(first) * 2 * (L + 1))
    up_top, down_surface, up_surface = empty(n), empty(n), empty(n)
    mu, w = angles(3)
    for beams in (1, 3):
        bw = [1.0 / (s + 1) for s in range(beams)]
        slant = [[1.0 + 0.5 * s + 0.1 * l for l in range(L)] for s in range(beams)]
        for refl, e in ((0, c.emissivity), (1, 0.6)):
            ctx.column_solar_dev(c.k, c.depth, *c.args(), c.S0, bw, slant, mu if refl == 0 else [], w if refl == 0 else [],
                                 first, count, levels, e, refl, up_top=up_top, down_surface=down_surface, up_surface=up_surface)
            save("%s_L%d_b%d_r%d_solar" % (tag, L, beams, refl), levels, up_top, down_surface, up_surface)


def ray_calls(tag, c):
    """Six rays: four nadir rays up from the surface through the same layers (one bundle), a single ray from space down to the
    surface, reflected there (a marker in mid-path) and up again, and a single limb ray from space.  The entry points
    without a surface get the same rays without the marker."""
    L, n = c.L, c.n
    up, down = list(range(L)), list(range(L - 1, -1, -1))
    paths = [(up, [d / m for d in c.depth], 1) for m in (1.0, 0.8, 0.6, 0.4)]
    paths.append((down + [-1] + up, [c.depth[l] * 1.3 for l in down] + [0.0] + [c.depth[l] * 1.1 for l in up], 0))
    paths.append((down[:-1] + up[1:] if L > 1 else up, [2.5 * c.depth[l] for l in (down[:-1] + up[1:] if L > 1 else up)], 0))
    src = dict(I_source=c.I_surface)

    def pack(markers):
        first, lay, length, kind, seg_T = [0], [], [], [], []
        for layers, lengths, k in paths:
            keep = [i for i, l in enumerate(layers) if markers or l >= 0]
            lay += [layers[i] for i in keep]
            length += [lengths[i] for i in keep]
            first.append(len(lay))
            kind.append(k)
        for s, l in enumerate(lay):                     # entry and exit temperatures in the order of travel
            seg_T.append((1.0, 1.0) if l < 0 else (c.T[l] + 5.0 + 0.01 * (s % 3), c.T[l] - 4.0))
        for s in range(first[1], first[4]):             # (the bundle's rays share them)
            seg_T[s] = seg_T[s - first[1]]
        return first, lay, length, kind, seg_T
    nr = len(paths)
    rad, tr = empty(nr * n), empty(nr * n)
    f, lay, length, kind, seg_T = pack(False)
    ctx.ray_radiance_dev(c.k, c.T, *c.args(), f, lay, length, kind, rad, transmittance=tr, **src)
    save(tag + "_rays", rad, tr)
    ctx.ray_radiance_dev(c.k, c.T, *c.args(), f, lay, length, kind, rad, transmittance=tr, source_T=290.0)
    save(tag + "_rays_T", rad, tr)
    for terms in (0, 2):
        tk = dict(term_abs_coef=c.term_k[:terms], term_layer=c.term_layer[:terms])
        rows = nat.ray_jacobian_rows(L, f, lay, tk["term_layer"])[1]
        jac = empty(rows * n)
        ctx.ray_jacobian_dev(c.k, c.T, *c.args(), f, lay, length, kind, jac, radiance=rad, source_T=290.0, **tk)
        save("%s_t%d_ray_jacobian" % (tag, terms), jac, rad)
    f, lay, length, kind, seg_T = pack(True)
    for e_name, e in (("e0.7", 0.7), ("earr", c.emissivity)):
        t = "%s_%s" % (tag, e_name)
        ctx.ray_radiance_surface_dev(c.k, c.T, *c.args(), f, lay, length, kind, rad, e, surface_down=c.I_top,
                                     surface_down_norm=np.pi, transmittance=tr, **src)
        save(t + "_rays_surface", rad, tr)
        ctx.ray_radiance_linear_dev(c.k, seg_T, *c.args(), f, lay, length, kind, rad, e, surface_down=c.I_top,
                                    surface_down_norm=np.pi, transmittance=tr, source_T=290.0)
        save(t + "_rays_linear", rad, tr)
        for terms in (0, 2):
            tk = dict(term_abs_coef=c.term_k[:terms], term_layer=c.term_layer[:terms])
            rows = nat.ray_jacobian_rows(L, f, lay, tk["term_layer"], surface=True)[1]
            jac = empty(rows * n)
            ctx.ray_jacobian_surface_dev(c.k, c.T, *c.args(), f, lay, length, kind, jac, e, radiance=rad, source_T=290.0, **tk)
            save("%s_t%d_ray_jacobian_surface" % (t, terms), jac, rad)
            rows = nat.ray_jacobian_rows(L, f, lay, tk["term_layer"], linear=True)[1]
            jac = empty(rows * n)
            ctx.ray_jacobian_linear_dev(c.k, seg_T, *c.args(), f, lay, length, kind, jac, e, radiance=rad, source_T=290.0, **tk)
            save("%s_t%d_ray_jacobian_linear" % (t, terms), jac, rad)
        # the source given as a spectrum (with its NaN and infinity), two terms
        rows = nat.ray_jacobian_rows(L, f, lay, tk["term_layer"], surface=True)[1]
        jac = empty(rows * n)
        ctx.ray_jacobian_surface_dev(c.k, c.T, *c.args(), f, lay, length, kind, jac, e, radiance=rad, **tk, **src)
        save(t + "_spectrum_ray_jacobian_surface", jac, rad)
        rows = nat.ray_jacobian_rows(L, f, lay, tk["term_layer"], linear=True)[1]
        jac = empty(rows * n)
        ctx.ray_jacobian_linear_dev(c.k, seg_T, *c.args(), f, lay, length, kind, jac, e, radiance=rad, **tk, **src)
        save(t + "_spectrum_ray_jacobian_linear", jac, rad)


def release():
    ctx.sync()
    while held:
        held.pop().free()


# fine grid: every wave of a group of four points takes the one-exp Planck path; coarse grid (1 cm^-1): none does
GRIDS = (("fast", 600.0, 0.01), ("general", 100.0, 1.0))
n_points = 4 * 256 * 2 + 7
for grid, lo, res in GRIDS:
    for L in (1, 3):
        col = Column(L, n_points, lo, res)
        for na in (1, 2, 3, 5, 8):
            for surface in ("T", "spectrum"):
                column_calls(grid, col, na, surface)
        solar_calls(grid, col)
        release()
    col = Column(3, 4 * 256 + 3, lo, res)
    ray_calls(grid, col)
    release()

# grid-stride: a second round of the point loop in some workgroups and not in others
col = Column(2, 1024 * 256 * 4 + 1024 + 3, 600.0, 1e-4)
n = col.n
mu, w = angles(1)
levels, up_top = empty(2 * 3), empty(n)
ctx.column_flux_dev(col.k, col.T, col.depth, *col.args(), mu, w, [0], [n], levels, up_top=up_top, surface_T=288.0)
save("stride_flux", levels, up_top)
mu, w = angles(3)
jac, ln_tau = empty(2 + 2 * 2), empty(2 * n)
ctx.column_jacobian_dev(col.k, col.T, col.depth, *col.args(), mu, w, [0], [n], jac, ln_tau_spectra=ln_tau, surface_T=288.0)
save("stride_jacobian", jac, ln_tau)
release()
ctx.close()
print("dumped to %s: %d files, %d values, %d of them finite and not zero" % (out, *tally))
