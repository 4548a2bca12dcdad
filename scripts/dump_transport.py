#!/usr/bin/env python3
"""Every column transport entry point (K5c - K5p: fluxes, Jacobians, ray paths, reflecting surface, linear source, solar
beam, the two-stream family) through _native.Context on synthetic, seeded absorption coefficients, every output saved as .npy (one file per call,
its outputs concatenated): run once per library build (PYRAD_HIP_LIB) and compare the files bit for bit
(scripts/bitcmp_libs.sh <lib a> <lib b> dump_transport.py).  No line lists are needed.  The shapes are the smallest at
which the kernels' frames can go wrong: bands with head, aligned and tail points, a band of three points, a grid-stride
second round in some workgroups only, every angle count (1 to 8: each is an instantiation of its own), both Planck paths,
bundled and single rays with a surface marker, a tail launch; for the two-stream family (K5l - K5p) see
scatter_calls and pole_column.  Every output buffer of the family's two youngest (K5o, K5p) must hold a finite value that is
not zero, or the script fails: a dump of zeros compares equal and says nothing.  Per entry point of that family refusals_<name>.npy holds, as bytes, the return code and lbl_last_error of
calls with one defect and with two: which of two defects is reported is part of what two builds must agree on.
usage: dump_transport.py <out dir>"""
import ctypes as C
import itertools, os, sys
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


def save(name, *bufs, live=False, zero=()):
    """one file per call: the call's output buffers, concatenated.  live: every buffer must hold a finite value that is not
    zero, but for those in `zero`, which the call's arguments make zero throughout"""
    ctx.sync()
    parts = [b.download(b.n) for b in bufs]
    for i, (b, v) in enumerate(zip(bufs, parts)):
        if live and not any(b is z for z in zero) and not np.any(np.isfinite(v) & (v != 0.0)):
            sys.exit("%s: output buffer %d holds no finite value that is not zero" % (name, i))
    values = np.concatenate(parts)
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
    # the source given as a spectrum (with its NaN and infinity), two terms
    ctx.ray_jacobian_dev(c.k, c.T, *c.args(), f, lay, length, kind, jac, radiance=rad, **tk, **src)
    save(tag + "_spectrum_ray_jacobian", jac, rad)
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


# ---- K5l - K5p: solar and thermal fluxes and radiances through scattering layers ------------------------------------------
class ScatterColumn:
    """L layers (optical depths 1e-3 .. tau_hi each) on n points from 600 cm^-1 in steps of 0.01, with four scatterers whose
    numbers come as buffers and as plain numbers, mixed.  `special`: layer 1 empty (t = 0), layer 2 conservative (no gas, the
    one scatterer in it with albedo 1) and one point of layer 0 with an infinite coefficient (the NaN rule)."""
    def __init__(self, L, n, tau_hi=5.0, special=False):
        self.L, self.n, self.lo, self.hi = L, n, 600.0, 600.0 + (n - 1) * 0.01
        self.depth = [1.0e5 * (l % 7 + 1) for l in range(L)]
        k = [np.exp(rng.uniform(np.log(1e-3), np.log(tau_hi), n)) / d for d in self.depth]
        self.amount = [[0.05 * (c + 1) * (1 + (l + c) % 3) for l in range(L)] for c in range(4)]
        if special:
            k[1][:], k[2][:] = 0.0, 0.0
            k[0][min(7, n - 1)] = np.inf
            for c in range(4):
                self.amount[c][1] = 0.0
                self.amount[c][2] = 0.8 if c == 1 else 0.0
        self.k = [dev(v) for v in k]
        # two molecule terms, as Column's (K5p)
        self.term_layer = [0, L - 1] if L else []
        self.term_k = [dev(np.exp(rng.uniform(np.log(1e-4), np.log(1.0), n)) / self.depth[l]) for l in self.term_layer]
        self.T = [288.0 - 0.5 * l for l in range(L)]
        # (bottom edge, top edge): two of three top edges are the next layer's bottom edge, the third is 0.3 K off it
        bottom = [292.0 - 0.5 * l for l in range(L + 1)]
        self.edge_T = [(bottom[l], bottom[l + 1] - (0.3 if l % 3 == 2 else 0.0)) for l in range(L)]
        self.S0 = dev(rng.uniform(0.5, 1.5, n))
        self.I_surface = dev(rng.uniform(0.05, 0.2, n))
        self.I_top = dev(rng.uniform(0.001, 0.02, n))
        self.emissivity = dev(rng.uniform(0.5, 0.98, n))
        ext, ssa, asym = (dev(rng.uniform(*r, n)) for r in ((0.2, 2.0), (0.3, 0.999), (-0.3, 0.85)))
        self.ext = [ext, 1.3, dev(rng.uniform(0.1, 1.0, n)), 0.4]
        self.ssa = [0.92, 1.0 if special else 0.97, 0.6, ssa]
        self.asym = [asym, 0.1, -0.25, dev(rng.uniform(0.0, 0.9, n))]

    def scat(self, count):
        return [a[:count] for a in (self.amount, self.ext, self.ssa, self.asym)]


class PoleColumn(ScatterColumn):
    """The column of pole_case (tests/test_beam_view_cpu.py) at L = 2 and n = 259: one scatterer of plain numbers, and the
    first beam's slant in layer 1 is lam of point 2 there, so that lam m = 1 to rounding at that point - and at every fourth
    point, which has its coefficient: K5l and K5o move m there (|1 - lam m| < 1e-6) and keep it at the other points."""
    def __init__(self):
        L, n, j = 2, 259, 2
        super().__init__(L, n)
        k = 10.0 ** rng.uniform(-2, 1, (L, n)) / np.array(self.depth)[:, None]
        k[1, j % 4::4] = k[1, j]
        self.k = [dev(v) for v in k]
        self.amount = [[0.5, 2.0]]
        self.ext, self.ssa, self.asym = [1.0], [0.6], [0.5]
        # lam as twostream_layer forms it (delta scaling on)
        ext, ssa, g = self.ext[0], self.ssa[0], self.asym[0]
        f = g * g
        al, si, et = ext * (1.0 - ssa), (ext * ssa) * (1.0 - f), (ext * ssa) * (g - f)
        am = self.amount[0][1]
        ta, ts, tsg = k[1] * self.depth[1] + am * al, am * si, am * et
        t = ta + ts
        D = 1.7320508075688772
        lam = np.sqrt((D * (ta / t)) * (D * ((t - tsg) / t)))
        assert 1.0 < lam[j] < D, lam[j]                  # (so that m = 1 / lam is a sun's cosine)
        self.slant0 = [1.3, float(lam[j])]
        self.in_window = int(np.count_nonzero(np.abs(1.0 - lam * (1.0 / self.slant0[1])) < 1e-6))


SCATTER_WORKSPACE = dict(twostream=ctx.column_twostream_workspace, flux_scatter=ctx.column_flux_scatter_workspace,
                         radiance_scatter=ctx.column_radiance_scatter_workspace,
                         beam_radiance=ctx.column_beam_radiance_workspace,
                         jacobian_scatter=ctx.column_jacobian_scatter_workspace)


def mixed_views(count):
    return [1.0 / (1.0 + 0.37 * v) for v in range(count)], [(v % 3 == 1) * 1 for v in range(count)]


def scatter_calls(tag, c, bands=None, n_scat=4, delta=1, e="arr", surface="spectrum", top=True, spectra=True, ws="wide",
                  linear=(1,), beams=(2,), views=(3,)):
    """K5l for every beam count in `beams`, K5o with one beam for every view count in `views`, K5m, K5p and K5n for both
    or one Planck setting in `linear`, K5n for every view count in `views`; ws: a workspace of one tile ("tile") or one that
    holds the widest band ("wide").  A column's `slant0` is the first beam's slants."""
    L, n = c.L, c.n
    first, count = bands if bands else ([0], [n])
    nb = len(first)
    e = c.emissivity if e == "arr" else e
    src = dict(I_surface=c.I_surface) if surface == "spectrum" else dict(surface_T=291.5)
    src["I_top"] = c.I_top if top else None
    spec = [empty(n) if spectra else None for _ in range(4)]
    kept = [b for b in spec if b is not None]

    def work(family, points):
        return empty(SCATTER_WORKSPACE[family](L, 1 if ws == "tile" else points))
    def slants(ns):
        slant = [[1.0 + 0.5 * s + 0.1 * (l % 5) for l in range(L)] for s in range(ns)]
        return [getattr(c, "slant0", slant[0])] + slant[1:]
    for ns in beams:
        bw = [1.0 / (s + 1) for s in range(ns)]
        slant = slants(ns)
        levels = empty(nb * 3 * (L + 1))
        ctx.column_twostream_dev(c.k, c.depth, c.lo, c.hi, n, c.S0, bw, slant, *c.scat(n_scat), delta, first, count,
                                 work("twostream", max(count)), levels, emissivity=e, up_top=spec[0], down_surface=spec[1],
                                 direct_surface=spec[2], up_surface=spec[3])
        save("%s_b%d_twostream" % (tag, ns), levels, *kept)
    for nv in views:
        mu, down = mixed_views(nv)
        rad = empty(nv * n)
        for b in kept:                  # (what an earlier call left there must not pass for this call's)
            b.fill(0.0)
        ctx.column_beam_radiance_dev(c.k, c.depth, c.lo, c.hi, n, c.S0, 0.8, slants(1)[0], *c.scat(n_scat), delta, mu, down,
                                     work("beam_radiance", n), rad, emissivity=e, up_top=spec[0], down_surface=spec[1],
                                     direct_surface=spec[2])
        # (no layer or no scatterer: nothing is scattered down to the surface)
        save("%s_v%d_beam_radiance" % (tag, nv), rad, *kept[:3], live=True, zero=kept[1:2] if L == 0 or n_scat == 0 else ())
    for lin in linear:
        T = c.edge_T if lin else c.T
        levels = empty(nb * 2 * (L + 1))
        ctx.column_flux_scatter_dev(c.k, T, lin, c.depth, c.lo, c.hi, n, *c.scat(n_scat), delta, first, count,
                                    work("flux_scatter", max(count)), levels, emissivity=e, up_top=spec[0],
                                    down_surface=spec[1], up_surface=spec[3], **src)
        save("%s_p%d_flux_scatter" % (tag, lin), levels, *kept[:2], *kept[3:])
        nt = 2 if lin else 1
        jac = empty(nb * (3 + (1 + nt + n_scat) * L + len(c.term_k)))
        # (no layer: no rows of spectra)
        ln_tau, T_spec = (empty(L * n), empty(nt * L * n)) if spectra and L else (None, None)
        for b in kept[:1]:
            b.fill(0.0)
        ctx.column_jacobian_scatter_dev(c.k, T, lin, c.depth, c.lo, c.hi, n, *c.scat(n_scat), delta, first, count,
                                        work("jacobian_scatter", max(count)), jac, emissivity=e, term_abs_coef=c.term_k,
                                        term_layer=c.term_layer, ln_tau_spectra=ln_tau, T_spectra=T_spec, up_top=spec[0],
                                        **src)
        save("%s_p%d_jacobian_scatter" % (tag, lin), jac, *[b for b in (ln_tau, T_spec) if b is not None], *kept[:1],
             live=True)
        for nv in views:
            mu, down = mixed_views(nv)
            rad = empty(nv * n)
            ctx.column_radiance_scatter_dev(c.k, T, lin, c.depth, c.lo, c.hi, n, *c.scat(n_scat), delta, mu, down,
                                            work("radiance_scatter", n), rad, emissivity=e, up_top=spec[0],
                                            down_surface=spec[1], **src)
            save("%s_p%d_v%d_radiance_scatter" % (tag, lin, nv), rad, *kept[:2])
    release()


def scatter_family():
    n = 515
    c = lambda **kw: ScatterColumn(3, n, **kw)
    scatter_calls("base", c(), bands=bands_of(n), linear=(0, 1), beams=range(1, 9), views=(1, 2, 3, 4, 5, 8, 9, 16))
    scatter_calls("onetile", c(), bands=bands_of(n), ws="tile", linear=(0, 1))
    scatter_calls("scat0", c(), bands=bands_of(n), n_scat=0)
    scatter_calls("scat1", c(), bands=bands_of(n), n_scat=1, delta=0)
    scatter_calls("delta0", c(), delta=0, linear=(0, 1))
    scatter_calls("plain", c(), e=0.7, surface="T", top=False, spectra=False, linear=(0, 1))
    scatter_calls("e0.7", c(), e=0.7)
    scatter_calls("surfaceT", c(), surface="T")
    scatter_calls("notop", c(), top=False)
    scatter_calls("nospectra", c(), spectra=False)
    for delta in (0, 1):
        scatter_calls("special_d%d" % delta, c(special=True), bands=bands_of(n), delta=delta, linear=(0, 1), views=(2,))
        scatter_calls("special_onetile_d%d" % delta, c(special=True), ws="tile", delta=delta, linear=(0, 1), views=(5,))
    scatter_calls("empty", ScatterColumn(0, 1), linear=(0, 1), views=(1, 3))
    scatter_calls("deep", ScatterColumn(nat.limit("layers_per_column"), 259, tau_hi=0.3), linear=(0, 1), beams=(1, 8),
                  views=(1, 16))
    scatter_calls("deep_onetile", ScatterColumn(nat.limit("layers_per_column"), 259, tau_hi=0.3), ws="tile", n_scat=2)
    scatter_calls("wrap", ScatterColumn(1, 256 * 1025 + 7), linear=(0, 1), views=(2,))
    pole = PoleColumn()
    print("pole column: lam m within 1e-6 of 1 at %d of %d points of layer 1" % (pole.in_window, pole.n))
    if pole.in_window == 0:
        sys.exit("the pole column has no point inside |1 - lam m| < 1e-6")
    scatter_calls("pole", pole, n_scat=1, linear=(), beams=(1, 2), views=(1, 3))


def refusal_calls():
    """Per entry point of the family: calls with one defect and with two (every pair of defects that touch different
    arguments, so each is paired with those checked behind it), the return code and the error text of each."""
    L, n, V = 3, 515, 3
    c = ScatterColumn(L, n)
    i64, f64 = lambda v: (C.c_int64 * max(len(v), 1))(*v), lambda v: (C.c_double * max(len(v), 1))(*v)
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    ptrs = lambda v: (C.c_void_p * max(len(v), 1))(*v)
    inf, nan = float("inf"), float("nan")
    n_short, spec = empty(n - 1), [empty(n) for _ in range(4)]
    ext, ssa, asym = c.ext[0], c.ssa[3], c.asym[0]
    scat = dict(n_scat=2, scat_amount=f64([0.1, 0.0, 2.0, 1.0, 1.0, 1.0]), scat_ext=ptrs([ext.h, None]),
                scat_ext_all=f64([0.0, 2.0]), scat_ssa=ptrs([ssa.h, None]), scat_ssa_all=f64([0.0, 1.0]),
                scat_asym=ptrs([asym.h, None]), scat_asym_all=f64([0.0, -0.2]), delta_scaling=1)
    head = dict(ctx=ctx.h, n_layers=L, abs_coef=ptrs([b.h for b in c.k]))
    grid = dict(depth=f64([1e4, 2e4, 1e4]), lo=c.lo, hi=c.hi, n=n)
    thermal = dict(I_surface=c.I_surface.h, surface_T=0.0, I_top=c.I_top.h)
    bands = dict(n_bands=1, band_first=i64([0]), band_count=i64([n]))
    surface = dict(emissivity=c.emissivity.h, emissivity_all=0.5)
    edges = dict(T=f64([290.0, 280.0, 280.0, 260.0, 255.0, 240.0]), planck_linear=1)
    tiles = {f: SCATTER_WORKSPACE[f](L, 1) for f in SCATTER_WORKSPACE}
    good = dict(
        twostream=dict(**head, **grid, S0=c.S0.h, n_beams=2, beam_weight=f64([0.5, 0.1]),
                       slant=f64([2.0, 1.9, 1.8, 1.0, 1.0, 1.0]), **scat, **bands, **surface,
                       workspace=empty(2 * tiles["twostream"]).h, level_flux=empty(3 * (L + 1)).h, up_top=spec[0].h,
                       down_surface=spec[1].h, direct_surface=spec[2].h, up_surface=spec[3].h),
        flux_scatter=dict(**head, **edges, **grid, **thermal, **scat, **bands, **surface,
                          workspace=empty(2 * tiles["flux_scatter"]).h, level_flux=empty(2 * (L + 1)).h, up_top=spec[0].h,
                          down_surface=spec[1].h, up_surface=spec[3].h),
        radiance_scatter=dict(**head, **edges, **grid, **thermal, **scat, **surface, n_views=V, view_mu=f64([1.0, 0.5, 0.2]),
                              view_down=i32([0, 1, 0]), workspace=empty(2 * tiles["radiance_scatter"]).h,
                              radiance=empty(V * n).h, up_top=spec[0].h, down_surface=spec[1].h),
        beam_radiance=dict(**head, **grid, S0=c.S0.h, beam_weight=0.5, slant=f64([2.0, 1.9, 1.8]), **scat, **surface,
                           n_views=V, view_mu=f64([1.0, 0.5, 0.2]), view_down=i32([0, 1, 0]),
                           workspace=empty(2 * tiles["beam_radiance"]).h, radiance=empty(V * n).h, up_top=spec[0].h,
                           down_surface=spec[1].h, direct_surface=spec[2].h),
        jacobian_scatter=dict(**head, **edges, **grid, **thermal, **scat, **bands, **surface, n_terms=2,
                              term_abs_coef=ptrs([b.h for b in c.term_k]), term_layer=i32(c.term_layer),
                              workspace=empty(2 * tiles["jacobian_scatter"]).h, jac=empty(3 + 5 * L + 2).h,
                              ln_tau_spectra=empty(L * n).h, T_spectra=empty(2 * L * n).h, up_top=spec[0].h))
    # the defect kinds of the three test_refusals, by the argument they spoil
    shared = [dict(abs_coef=None), dict(depth=None), dict(scat_amount=None), dict(workspace=None), dict(n_layers=-1),
              dict(n_layers=nat.limit("layers_per_column") + 1), dict(n=-5), dict(n_scat=-1),
              dict(n_scat=nat.limit("scatterers") + 1), dict(up_top=n_short.h), dict(down_surface=n_short.h),
              dict(emissivity=n_short.h), dict(abs_coef=ptrs([c.k[0].h, n_short.h, c.k[2].h])),
              dict(scat_ext=ptrs([n_short.h, None])), dict(scat_ssa=ptrs([ssa.h, n_short.h])),
              dict(scat_asym=ptrs([n_short.h, None])), dict(depth=f64([1e4, -1.0, 1e4])), dict(depth=f64([1e4, nan, 1e4])),
              dict(scat_amount=f64([0.1, -1e-9, 2.0, 1.0, 1.0, 1.0])), dict(scat_amount=f64([inf, 0.0, 2.0, 1.0, 1.0, 1.0])),
              dict(scat_ext_all=f64([0.0, -1.0])), dict(scat_ext_all=None), dict(scat_ssa_all=f64([0.0, 1.01])),
              dict(scat_asym_all=f64([0.0, 1.0])), dict(scat_asym_all=f64([0.0, nan])), dict(delta_scaling=2),
              dict(emissivity=None, emissivity_all=1.01), dict(emissivity=None, emissivity_all=nan)]
    banded = [dict(band_first=None), dict(band_count=None), dict(level_flux=None), dict(n_bands=0),
              dict(n_bands=nat.limit("flux_bands") + 1), dict(level_flux=n_short.h), dict(up_surface=n_short.h),
              dict(band_count=i64([n + 1])), dict(band_first=i64([-1])), dict(band_count=i64([0]))]
    heated = [dict(T=None), dict(I_surface=n_short.h), dict(I_top=n_short.h), dict(I_surface=None, surface_T=0.0),
              dict(I_surface=None, surface_T=nan), dict(T=f64([290.0, 280.0, 280.0, 0.0, 255.0, 240.0])),
              dict(T=f64([nan, 280.0, 280.0, 260.0, 255.0, 240.0])), dict(planck_linear=0, T=f64([290.0, nan, 250.0])),
              dict(planck_linear=0, T=f64([290.0, 270.0, inf])), dict(planck_linear=2)]
    viewed = [dict(radiance=None), dict(view_mu=None), dict(view_down=None), dict(n=0), dict(n_views=0),
              dict(view_mu=f64([1.0, 0.0, 0.2])), dict(view_mu=f64([1.0, nan, 0.2])), dict(view_down=i32([0, 2, 0])),
              dict(radiance=n_short.h)]
    own = dict(
        twostream=banded + [dict(S0=None), dict(beam_weight=None), dict(slant=None), dict(n_beams=0), dict(S0=n_short.h),
                            dict(n_beams=nat.limit("flux_angles") + 1), dict(direct_surface=n_short.h),
                            dict(workspace=empty(tiles["twostream"] - 1).h),
                            dict(slant=f64([2.0, 1.9, 1.8, 1.0, 0.0, 1.0])), dict(slant=f64([2.0, inf, 1.8, 1.0, 1.0, 1.0])),
                            dict(beam_weight=f64([0.5, inf]))],
        flux_scatter=banded + heated + [dict(workspace=empty(tiles["flux_scatter"] - 1).h)],
        radiance_scatter=heated + viewed + [dict(n_views=nat.limit("scatter_views") + 1),
                                            dict(workspace=empty(tiles["radiance_scatter"] - 1).h)],
        beam_radiance=viewed + [dict(n_views=nat.limit("beam_views") + 1), dict(S0=None), dict(slant=None), dict(S0=n_short.h),
                                dict(direct_surface=n_short.h), dict(workspace=empty(tiles["beam_radiance"] - 1).h),
                                dict(slant=f64([2.0, 0.0, 1.8])), dict(slant=f64([2.0, inf, 1.8])), dict(beam_weight=inf),
                                dict(beam_weight=-0.5)],
        jacobian_scatter=banded + heated + [dict(workspace=empty(tiles["jacobian_scatter"] - 1).h), dict(jac=None),
                                            dict(jac=empty(3 + 5 * L + 1).h), dict(n_terms=-1),
                                            dict(n_terms=nat.limit("jacobian_terms") + 1), dict(term_abs_coef=None),
                                            dict(term_layer=None), dict(term_layer=i32([0, L])), dict(term_layer=i32([-1, 0])),
                                            dict(term_abs_coef=ptrs([n_short.h, c.term_k[1].h])),
                                            dict(ln_tau_spectra=n_short.h), dict(T_spectra=n_short.h)])
    for name, base in good.items():
        entry = getattr(ctx.lib, "lbl_column_%s_dev" % name)
        absent = {"level_flux", "down_surface", "up_surface"} if name == "jacobian_scatter" else set()   # (K5p: jac, up_top)
        defects = [d for d in shared + own[name] if not set(d) & absent]
        assert all(set(d) <= set(base) for d in defects), name
        calls = [{}] + defects + [dict(a, **b) for a, b in itertools.combinations(defects, 2) if not set(a) & set(b)]
        record = bytearray()
        for kw in calls:
            rc = entry(*[dict(base, **kw)[key] for key in base])
            record += b"%d %s\n" % (rc, (ctx.lib.lbl_last_error(ctx.h) or b"") if rc else b"")
        assert entry(*base.values()) == 0 and len(calls) > 500, name
        ctx.sync()
        np.save(os.path.join(out, "refusals_%s.npy" % name), np.frombuffer(bytes(record), dtype=np.uint8))
        tally[0] += 1
        tally[1] += len(record)
        tally[2] += len(record)
    release()


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
        for na in range(1, 9):            # every angle count has kernels of its own
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
scatter_family()
refusal_calls()
ctx.close()
print("dumped to %s: %d files, %d values, %d of them finite and not zero (%.2f %%)" % (out, *tally, 100.0 * tally[2] / tally[1]))
