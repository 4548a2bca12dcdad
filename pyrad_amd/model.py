"""The Layer / Molecule / Isotope / Line / Atmosphere object model of pyradClasses, kept so
that PyRad-style drivers (pyradInteractive, main.py) run unchanged on top of the MI355X
engine.  Names, argument meaning, units, the lazy ``progressCrossSection`` protocol and the
error behaviour follow the reference; every number comes from the HIP kernels behind
include/pyrad_hip.h.  There is no CPU fallback: without libpyrad_hip.so or without a GPU the
first computation raises.

Reference map (cls = pyradClasses.py):
    Line cls:237-263 · Isotope cls:266-442 · Molecule cls:445-642 · Layer cls:645-787 ·
    Atmosphere cls:790-821 · getters cls:32-88 · reset protocol cls:38-58 ·
    converters cls:121-156 · integrateSpectrum cls:26-29 · returnPlot cls:824-839.
Measured cross-section ("xsc") molecules (cls:466-505, mergeArray cls:165-233) are host-side
table handling in the reference and here; their array then feeds the same device sweep.
Not carried over (out of scope): the HITRAN download, the curve cache, the
interactive menu.
"""
from __future__ import annotations

import math
import types
import weakref

import numpy as np

from . import _native as nat
from . import data as _data
from . import engine as _engine
from . import settings

utils = settings          # the reference spells it utils.BASE_RESOLUTION

c = 299792458.0
k = 1.38064852E-23
h = 6.62607004e-34
pi = 3.141592653589793
t0 = 296
p0 = 1013.25
avo = 6.022140857E23

# Atmosphere.fluxes: heat capacity of air at constant pressure and gas constant of dry air (J kg^-1 K^-1), for the heating
# rate of a layer from its mass per unit area (change them here to use other values)
CP_AIR = 1004.0
R_DRY_AIR = 287.05

VERSION = settings.VERSION
VERBOSE = False           # the reference prints progress bars; set True to see the regime line


def _say(*a, **kw):
    if VERBOSE:
        print(*a, **kw)


# ----------------------------------------------------------------------------------------
# tables (content of cls:951-1022 stored compactly)
# ----------------------------------------------------------------------------------------
_MOLECULES = ("h2o co2 o3 n2o co ch4 o2 no so2 no2 nh3 hno3 oh hf hcl hbr hi clo ocs h2co hocl n2 hcn ch3cl "
              "h2o2 c2h2 c2h6 ph3 cof2 sf6 h2s hcooh ho2 o clono2 no+ hobr c2h4 ch3oh ch3br ch3cn cf4 c4h2 hc3n "
              "h2 cs so3 c2n2 cocl2").split()
MOLECULE_ID = {name: i + 1 for i, name in enumerate(_MOLECULES)}

_GLOBAL_ISO_ROWS = (
    "1 2 3 4 5 6 129|7 8 9 10 11 12 13 14 121 15 120 122|16 17 18 19 20|21 22 23 24 25|26 27 28 29 30 31|"
    "32 33 34 35|36 37 38|39 40 41|42 43|44|45 46|47 117|48 49 50|51 110|52 53 107 108|19 11 111 112|56 113|"
    "57 58|59 60 61 62 63|64 65 66|67 68|69 118|70 71 72|73 74|75|76 77 105|78 106|79|80 119|126|81 82 83|84|85|"
    "86|127 128|87|88 89|90 91|92|93 94|95|96|116|109|103 115|97 98 99 100|114|123|124 125")
HITRAN_GLOBAL_ISO = {m + 1: {i + 1: int(g) for i, g in enumerate(row.split())}
                     for m, row in enumerate(_GLOBAL_ISO_ROWS.split("|"))}

COLOR_LIST = ['xkcd:white', 'xkcd:bright orange', 'xkcd:seafoam green', 'xkcd:bright blue', 'xkcd:salmon',
              'xkcd:light violet', 'xkcd:green yellow']
EXOTIC_IDS = _data.EXOTIC_IDS          # cls:1024; filled by data.set_xsc_source


# ----------------------------------------------------------------------------------------
# module-level helpers (cls:26-162)
# ----------------------------------------------------------------------------------------
def _ctx() -> nat.Context:
    return _engine.get_engine().ctx


def integrateSpectrum(spectrum, unitAngle=pi, res=settings.BASE_RESOLUTION):
    """cls:26-29 on the device (K6): sum(nan_to_num(spectrum)) * unitAngle * res.  Like the
    reference, the default ``res`` is frozen at import time."""
    spectrum = np.ascontiguousarray(spectrum, dtype=np.float64)
    ctx = _ctx()
    buf = ctx.buffer(max(spectrum.size, 1))
    try:
        buf.upload(spectrum)
        return ctx.band_integral(buf, spectrum.size, unitAngle, res)
    finally:
        buf.free()


def getCrossSection(obj):
    if not obj.progressCrossSection:
        obj.createCrossSection()
    return obj.crossSection


def resetCrossSection(obj):
    """cls:38-45: marks every Isotope/Molecule below ``obj`` dirty (a Layer itself is skipped)."""
    if not isinstance(obj, Layer):
        if not obj.exotic:
            n = int((obj.rangeMax - obj.rangeMin) / utils.BASE_RESOLUTION)
            type(obj).crossSection.defer(obj, lambda n=n: np.zeros(n))      # the zeros of cls:41, made when read
            if isinstance(obj, Isotope):
                obj._host_array_assigned("_crossSection_host", installed=False)      # (the zeros above are the reference's reset, not somebody's array)
                obj._inputs_version += 1             # (a merged layer step computed from this isotopologue is stale too)
            obj.progressCrossSection = False
    if isinstance(obj, Isotope):
        return                      # its children are Lines (the reference walks them and skips each one)
    for child in obj:
        if not isinstance(child, Line):
            resetCrossSection(child)


def resetData(obj):
    """cls:48-58: drop and reload the line data below ``obj`` (range or pressure changed)."""
    for child in obj:
        if isinstance(child, Isotope):
            child.clear_lines()
            child.getData()
        else:
            resetData(child)
    resetCrossSection(obj)


def getAbsCoef(obj):
    if not obj.progressCrossSection:
        obj.createCrossSection()
    return obj.absCoef


def getAbsCoefDT(layer):
    """dk/dT of a Layer under the Voigt line shape (Layer.absCoefDT; beyond the reference)."""
    return layer.absCoefDT


def getTransmittance(obj):
    if not obj.progressCrossSection:
        obj.createCrossSection()
    return obj.transmittance


def getOpticalDepth(obj):
    if not obj.progressCrossSection:
        obj.createCrossSection()
    return obj.opticalDepth                         # -log(transmittance), cls:76


def getAbsorbance(obj):
    if not obj.progressCrossSection:
        obj.createCrossSection()
    return obj.absorbance


def getEmissivity(obj):
    if not obj.progressCrossSection:
        obj.createCrossSection()
    return obj.emissivity


def getGlobalIsotope(ID, isotopeDepth):
    return [HITRAN_GLOBAL_ISO[ID][i] for i in range(1, isotopeDepth + 1)]


def totalConcentration(layer):
    total = 0
    for molecule in layer:
        total += molecule.concentration
    return total


def totalLineList(obj):
    if isinstance(obj, Isotope):
        return obj.linelist()
    fullList = []
    for item in obj:
        fullList += totalLineList(item)
    return fullList


def convertLength(value, units):
    if units == 'cm':
        return value
    if units in ['m', 'meter']:
        return value * 100
    if units in ['ft', 'feet']:
        return value * 30.48
    if units in ['in', 'inch']:
        return value * 2.54


def convertPressure(value, units):
    if units == 'mbar':
        return value
    if units in ['atm', 'atmospheres', 'atmosphere']:
        return value * 1013.25
    if units in ['b', 'bar']:
        return value * 1000
    if units in ['pa', 'pascal', 'pascals']:
        return value / 100


def convertRange(value, units):
    if units == 'cm-1':
        return value
    if units in ['um', 'micrometers', 'micrometer']:
        return 10000 / value


def convertTemperature(value, units):
    u = units[0].upper()
    if u == 'K':
        return value
    if u == 'C':
        return value + 273            # 273, not 273.15 (cls:154)
    if u == 'F':
        return (value - 32) * 5 / 9 + 273


def interpolateArray(hiResXAxis, loResXAxis, loResYValues):
    """cls:159-162 (used by the reference only inside createCrossSection, where the device
    regrid kernel replaces it; kept for callers)."""
    return np.interp(hiResXAxis, loResXAxis, loResYValues)


def isBetween(test, minValue, maxValue):
    return minValue <= test <= maxValue


def mergeArray(newX, oldX, oldY):
    """cls:165-233: lay a measured cross section (oldX, oldY) onto the layer axis newX by matching
    abscissae rounded to 0.01 cm^-1; zeros outside the overlap.  Kept as the reference has it:
    the last overlapping sample is dropped, positions are matched only at the first overlapping
    point (the copy is then index-for-index), a start value missing from the rounded axis raises
    ValueError, and a partial overlap returns an array longer than newX."""
    as_list = lambda v: v if isinstance(v, list) else v.tolist()
    oldY = as_list(oldY)
    nx = [round(x, 2) for x in as_list(newX)]
    ox = [round(x, 2) for x in as_list(oldX)]
    n_lo, n_hi, o_lo, o_hi = min(nx), max(nx), min(ox), max(ox)
    if n_hi < o_lo or n_lo > o_hi:
        return np.zeros(len(nx))
    if n_lo <= o_lo:
        lead, src = nx.index(o_lo), 0
    else:
        lead, src = 0, ox.index(n_lo)
    if n_hi >= o_hi:
        last_new, src_end = lead + len(ox) - 1, len(ox) - 1
    else:
        last_new, src_end = len(nx) - 1, src + len(nx) - 1
    if src < src_end and src_end > len(oldY):
        raise IndexError("list index out of range")
    return np.asarray([0] * lead + oldY[src:max(src_end, src)] + [0] * (len(nx) - last_new))


def concentration_from_kwargs(**abundance):
    """The volume fraction Molecule.__init__ derives from its keyword (cls:453-463, 543-560),
    including ppb -> x1e-8 (cls:554)."""
    conc = 0
    for key, v in abundance.items():
        if key == 'ppm':
            conc = v * 10**-6
        elif key == 'ppb':
            conc = v * 10**-8
        elif key in ('percentage', 'perc', '%'):
            conc = v / 100
        elif key == 'concentration':
            conc = (v * 1E6) * 10**-6
        else:
            print('Invalid concentration type. Use ppm, ppb, percentage, or concentration.')
    return conc


# ----------------------------------------------------------------------------------------
# device residency: cross sections and swept spectra stay in HBM between getters
# ----------------------------------------------------------------------------------------
class _LazyArray:
    """Attribute whose host copy is fetched from the device on first read.  The reference keeps
    plain NumPy arrays in ``crossSection`` / ``lineSurvey``; here the device owns the data and a
    host array is made only when somebody looks at it (a getter chain that ends in absCoef never
    does).  Assigning a host array drops the loader."""

    def __init__(self, name):
        self.host, self.loader = "_%s_host" % name, "_%s_loader" % name

    def __get__(self, obj, owner=None):
        if obj is None:
            return self
        load = obj.__dict__.get(self.loader)
        if load is not None:
            obj.__dict__[self.host] = load()
            obj.__dict__[self.loader] = None
        return obj.__dict__.get(self.host)

    def __set__(self, obj, value):
        obj.__dict__[self.host] = value
        obj.__dict__[self.loader] = None
        hook = getattr(obj, "_host_array_assigned", None)
        if hook is not None:
            hook(self.host)

    def defer(self, obj, loader):
        obj.__dict__[self.host] = None
        obj.__dict__[self.loader] = loader


def _zeros_later(descriptor, obj, n):
    """``obj.<array> = np.zeros(n)`` without making the array until somebody reads it (a 2.4e6-point layer with three
    molecules would otherwise write 150 MB of zeros at construction, most of which nobody ever looks at)"""
    loader = lambda n=int(n): np.zeros(n)
    descriptor.defer(obj, loader)
    obj.__dict__[descriptor.host + "_zeros"] = loader


def _copy_of_layer_cross_section(descriptor, obj, layer):
    """``obj.crossSection = np.copy(layer.crossSection)`` (cls:290, 512): while the layer's array is still its initial
    zeros the copy is zeros made on first read; a computed array is copied now, as the reference does"""
    d = Layer.crossSection
    pending = layer.__dict__.get(d.loader)
    if pending is not None and pending is layer.__dict__.get(d.host + "_zeros"):
        _zeros_later(descriptor, obj, int((layer.rangeMax - layer.rangeMin) / utils.BASE_RESOLUTION))
    else:
        setattr(obj, "crossSection", np.copy(layer.crossSection))


def _free_buffers(bufs):
    for b in bufs.values():
        try:
            if b.ctx.h:
                b.free()
        except Exception:
            pass
    bufs.clear()


class _SweepState:
    """Device buffers of one object's property chain (absorption coefficient, transmittance and
    scratch) and the key of what they were computed from; a getter re-sweeps only when the key
    (member cross-section versions, concentrations, P, T, depth, grid) has changed."""

    def __init__(self, owner):
        self.bufs = {}
        self.n = -1
        self.key = None
        import weakref
        weakref.finalize(owner, _free_buffers, self.bufs)

    def reserve(self, ctx, n):
        """buffers for n grid points: kept when they are large enough (a range change that shrinks the grid re-uses them:
        five hipFree + hipMalloc of 19 MB are 1.2 ms), what they held is stale either way"""
        if any(b.h is None or b.ctx is not ctx or b.n < n for b in self.bufs.values()):
            _free_buffers(self.bufs)
            self.key = None
        if self.n != n:
            self.n, self.key = n, None
        return self

    def buf(self, ctx, name):
        b = self.bufs.get(name)
        if b is None:
            b = self.bufs[name] = ctx.buffer(max(self.n, 1))
        return b


def _kept_state(owner, key):
    """The _SweepState kept in owner.__dict__[key], made on first use."""
    st = owner.__dict__.get(key)
    if st is None:
        st = owner.__dict__[key] = _SweepState(owner)
    return st


def _iso_params(iso):
    layer = iso.layer
    q_T = iso.q[layer.T]                       # KeyError for a non-integer temperature, as cls:389
    return nat.IsoParams(float(layer.T), float(layer.P), float(iso.molecule.concentration), float(iso.molmass),
                         float(q_T), float(iso.q296))


def _dlnq_dT(iso):
    """d ln Q / dT of an isotopologue at its layer's temperature, from the integer-kelvin table: the central difference
    (Q[T+1] - Q[T-1]) / (2 Q[T]), one-sided at a table end; KeyError when T itself is missing (as _iso_params)."""
    T = iso.layer.T
    q_T = iso.q[T]
    try:
        below, above = iso.q.get(T - 1), iso.q.get(T + 1)
    except AttributeError:                      # (a table that is no dict: only item access)
        below = iso.q[T - 1] if (T - 1) in iso.q else None
        above = iso.q[T + 1] if (T + 1) in iso.q else None
    if below is not None and above is not None:
        return (float(above) - float(below)) / (2.0 * float(q_T))
    if above is not None:
        return (float(above) - float(q_T)) / float(q_T)
    if below is not None:
        return (float(q_T) - float(below)) / float(q_T)
    raise KeyError(T + 1)


def _check_window(g):
    if g["W"] < 1:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")     # rightCurve[0], cls:393


def _mark_computed(ctx, isotopes, n):
    for iso in isotopes:
        iso._xs_version += 1
        iso._dev_xsec_valid = True
        iso._xs_deferred = False
        iso._xs_installed = False
        Isotope.crossSection.defer(iso, (lambda b=iso._dev_xsec, n=n: b.download(n, pinned=True)))
        iso._regime_counts = None
        iso.progressCrossSection = True
    if VERBOSE:
        for iso in isotopes:
            _say('\ngaussian only: %s\t lorentz only: %s\t voigt: %s\n' % iso.regimeCounts, end='\r')


def _compute_cross_sections(isotopes):
    """Batched Isotope.createCrossSection (cls:361-407) for every dirty isotopologue in the
    list: one prep launch + one accumulate launch for all of them.  The cross sections stay on
    the device; ``iso.crossSection`` downloads on first read."""
    dirty = [i for i in isotopes if (not i.progressCrossSection or i._xs_deferred) and not i.exotic]
    if not dirty:
        return
    ctx = _ctx()
    jobs = []
    for iso in dirty:
        g = iso.layer._grid()
        _check_window(g)
        jobs.append((iso._device_lines(ctx), _iso_params(iso), _engine.native_grid(g), iso._device_xsec(ctx, g["n_base"])))
    if settings.LINE_SHAPE == "voigt":
        ctx.xsec_voigt_dev(jobs)                # the true Voigt profile for every line (lbl_xsec_voigt_dev)
    else:
        ctx.xsec_accumulate_dev(jobs)
    _mark_computed(ctx, dirty, dirty[0].layer._grid()["n_base"])


def _merged_route(ctx):
    """The merged layer jobs (settings.LAYER_STEP "merged") evaluate the reference's line shape in the default arithmetic:
    any other setting takes the per-line-list routes."""
    return settings.LAYER_STEP == "merged" and settings.LINE_SHAPE == "reference" and not ctx.option("sweep_ieee_divisions")


_live_layers = []       # weak references to every Layer (settings.set_line_shape marks their cross sections dirty)


def _line_shape_changed():
    """settings.set_line_shape: every line-by-line cross section below every live Layer is of the other shape."""
    alive = []
    for ref in _live_layers:
        layer = ref()
        if layer is not None:
            alive.append(ref)
            resetCrossSection(layer)
    _live_layers[:] = alive


class _OpticalMixin:
    """The property chain shared by Isotope, Molecule and Layer (cls:322-340, 581-606, 707-732,
    784-787).  ``_sweep_members`` says which isotopologues and concentrations take part; the
    swept arrays live in a per-object _SweepState on the device and a getter downloads only the
    array it returns."""

    def _sweep_members(self):
        raise NotImplementedError

    def _ensure_swept(self):
        """(state, n) with absorption coefficient and transmittance of the CURRENT members resident.
        When every line-by-line member is dirty (first use, or after a temperature / pressure / range
        change) the whole layer step runs as one fused launch sequence (lbl_layer_step_dev: line
        prep, accumulate, sweep in the accumulate kernel's output stage); otherwise only the dirty
        isotopologues are accumulated and the sweep kernel runs if anything it reads has changed."""
        ctx = _ctx()
        layer = self._layer()
        g = layer._grid()
        n = g["n_base"]
        members, conc = self._sweep_members()
        flat = [iso for isos in members for iso in isos]
        st = _kept_state(self, "_sweep_state")
        st.reserve(ctx, n)
        lbl = [i for i in flat if not i.exotic]
        dirty = [i for i in lbl if not i.progressCrossSection]
        fusable = (dirty and len(dirty) == len(flat) and g["resolution"] == g["base_resolution"]
                   and g["n_work"] == n and len(flat) <= nat.limit("arrays_per_layer")
                   and settings.LINE_SHAPE == "reference")         # (the fused step's accumulate kernels are the reference's shape)
        if self._merged_step_applies(flat, lbl):
            # A LAYER whose line lists are due (any of them dirty): ONE accumulate job over the merged, factor-weighted
            # line lists - the absorption coefficient sum_m f_m sum_iso xs_iso (cls:707-712, 581-583, 566-571) accumulated
            # directly, the transmittance in the kernel's output stage.  No isotopologue cross section is written, and none
            # is marked computed: getCrossSection(isotope | molecule) produces it when asked (the reference's lazy
            # protocol, cls:32-88), and the layer's arrays are found again through the key below until an input changes.
            key = self._merged_key(flat, conc, layer, g)
            if st.key != key and isinstance(st.key, tuple) and st.key[:-1] == key[:-1]:
                # only the depth changed (changeDepth resets nothing, cls:754-755): the absorption coefficient stands,
                # the transmittance exp(-k depth) (cls:714-716) is redone from it
                ctx.column_fold_dev([st.bufs["abs_coef"]], [layer.T], [layer.depth], layer.rangeMin, layer.rangeMax, n,
                                    st.buf(ctx, "tmp"), surface_T=float(layer.T), trans=[st.buf(ctx, "trans")])
                st.key = key
            elif st.key != key:
                _check_window(g)
                iso_mol = [m for m, isos in enumerate(members) for _ in isos]
                ctx.layer_merged_step_dev([i._device_lines(ctx) for i in flat], [_iso_params(i) for i in flat],
                                          _engine.native_grid(g), iso_mol, conc, layer.depth,
                                          abs_coef=st.buf(ctx, "abs_coef"), trans=st.buf(ctx, "trans"))
                st.key = key
            for iso in flat:
                iso._defer_cross_section()
            self._members_ready()
            return st, n
        if fusable:
            _check_window(g)
            iso_mol = [m for m, isos in enumerate(members) for _ in isos]
            ctx.layer_step_dev([i._device_lines(ctx) for i in flat], [_iso_params(i) for i in flat],
                               _engine.native_grid(g), [i._device_xsec(ctx, n) for i in flat], iso_mol, conc,
                               layer.depth, abs_coef=st.buf(ctx, "abs_coef"), trans=st.buf(ctx, "trans"))
            _mark_computed(ctx, flat, n)
            st.key = self._sweep_key(flat, conc, layer, g)
        else:
            _compute_cross_sections(dirty)
            key = self._sweep_key(flat, conc, layer, g)
            if st.key != key:
                xs = [iso._device_xsec_current(ctx, n) for iso in flat]
                iso_mol = [m for m, isos in enumerate(members) for _ in isos]
                ctx.layer_sweep_dev(xs, iso_mol, conc, layer.P, layer.T, layer.depth, layer.rangeMin, layer.rangeMax, n,
                                    abs_coef=st.buf(ctx, "abs_coef"), trans=st.buf(ctx, "trans"))
                st.key = self._sweep_key(flat, conc, layer, g)
        self._members_ready()
        return st, n

    def _merged_step_applies(self, flat, lbl):
        return False                    # (Layer overrides: isotopologues and molecules keep the per-line-list path)

    @staticmethod
    def _merged_key(flat, conc, layer, g):
        return ("merged", tuple((id(i), i._inputs_version) for i in flat), tuple(float(c) for c in conc), layer.P, layer.T,
                layer.rangeMin, layer.rangeMax, g["n_base"], g["resolution"], settings.ACCURACY, settings.LINE_SHAPE,
                layer.depth)     # (depth last)

    @staticmethod
    def _sweep_key(flat, conc, layer, g):
        return (tuple((id(i), i._xs_version) for i in flat), tuple(float(c) for c in conc), layer.P, layer.T, layer.depth,
                layer.rangeMin, layer.rangeMax, g["n_base"], settings.LINE_SHAPE)

    def _members_ready(self):
        """hook: a Layer / Molecule marks the molecule sums it stands for as computed (cls:566-571)"""

    @property
    def absCoef(self):
        st, n = self._ensure_swept()
        return st.bufs["abs_coef"].download(n, pinned=True)

    @property
    def transmittance(self):
        st, n = self._ensure_swept()
        return st.bufs["trans"].download(n, pinned=True)

    def _optical(self, kind):
        st, n = self._ensure_swept()
        ctx = _ctx()
        out = st.buf(ctx, "tmp")
        ctx.optical_dev(st.bufs["trans"], n, kind, out)
        return out.download(n, pinned=True)

    @property
    def emissivity(self):
        return self._optical(0)                 # 1 - transmittance (cls:330-332)

    @property
    def emittance(self):
        return self.emissivity

    @property
    def absorbance(self):
        return self._optical(1)                 # log10(1 / transmittance) (cls:338-340)

    @property
    def opticalDepth(self):
        return self._optical(2)                 # -log(transmittance) (cls:73-76)

    def planck(self, temperature):
        return self._layer().planck(temperature)

    def transmission(self, surfaceSpectrum):
        """transmittance * surfaceSpectrum + emittance * planck(T)  (cls:784-787): the resident
        transmittance folded with the uploaded spectrum by the column kernel (one layer)."""
        st, n = self._ensure_swept()
        ctx = _ctx()
        layer = self._layer()
        I_in = np.ascontiguousarray(surfaceSpectrum, dtype=np.float64)
        if I_in.shape != (n,):
            raise ValueError("operands could not be broadcast together with shapes (%d,) %s" % (n, I_in.shape))
        src = st.buf(ctx, "I_in").upload(I_in)
        out = st.buf(ctx, "tmp")
        ctx.column_sweep_dev([st.bufs["trans"]], [layer.T], layer.rangeMin, layer.rangeMax, n, out, I_in=src)
        return out.download(n, pinned=True)


# ----------------------------------------------------------------------------------------
# Line (cls:237-263)
# ----------------------------------------------------------------------------------------
class Line:
    def __init__(self, wavenumber, intensity, einsteinA, airHalfWidth,
                 selfHalfWidth, lowerEnergy, tempExponent, pressureShift, parent):
        self.isotope = parent
        self.molecule = self.isotope.molecule
        self.layer = self.molecule.layer
        self.wavenumber = wavenumber
        self.intensity = intensity
        self.einsteinA = einsteinA
        self.airHalfWidth = airHalfWidth
        self.selfHalfWidth = selfHalfWidth
        self.lowerEnergy = lowerEnergy
        self.tempExponent = tempExponent
        self.pressureShift = pressureShift

    # introspection only: the device computes these per line in K1 (lbl_line_quantities)
    @property
    def broadenedLine(self):
        return self.wavenumber + self.pressureShift * self.layer.P / p0

    @property
    def lorentzHW(self):
        return (float((1 - self.molecule.concentration) * self.airHalfWidth + self.molecule.concentration
                      * self.selfHalfWidth) * (self.layer.P / p0) * (t0 / self.layer.T) ** self.tempExponent)

    @property
    def gaussianHW(self):
        return self.broadenedLine * math.sqrt(2 * k * self.layer.T / self.isotope.molMass / c ** 2)


# ----------------------------------------------------------------------------------------
# Isotope (cls:266-442): a list of Line, stored as a structure of arrays
# ----------------------------------------------------------------------------------------
class Isotope(_OpticalMixin, list):
    _FIELDS = ("nu", "sw", "a", "gamma_air", "gamma_self", "elower", "n_air", "delta_air")
    crossSection = _LazyArray("crossSection")      # device-resident after createCrossSection; downloaded on read
    lineSurvey = _LazyArray("lineSurvey")          # computed (K7) and downloaded on first read

    def __init__(self, number, molecule):
        super().__init__()
        self.molecule = molecule
        self.layer = self.molecule.layer
        self._dev_lines = None
        self._dev_xsec = None
        self._dev_xsec_valid = False
        self._xs_version = 0
        self._xs_deferred = False        # marked computed by a merged layer step: the array itself is made when somebody reads it
        self._xs_installed = False       # somebody assigned ``crossSection`` an array of their own (and nothing has recomputed it since):
                                         # the layer's sums must use THAT array, as the reference's getters do (cls:32-35, 566-571)
        self._inputs_version = 0         # bumped by everything that marks the cross section dirty (resetCrossSection, new lines)
        self._struct_version = 0         # bumped when the line list itself changes or somebody installs a cross section: a resident
                                         # column (Atmosphere._column_fast) then re-reads this layer's blocks
        self._regime_counts = (0, 0, 0)
        _copy_of_layer_cross_section(Isotope.crossSection, self, self.layer)
        self.exotic = molecule.exotic
        self._lines = {f: np.zeros(0) for f in self._FIELDS}
        if number not in EXOTIC_IDS:
            params = _data.get_source().readMolParams(number)
            self.globalIsoNumber = params[0]
            self.shortName = params[1]
            self.name = 'Isotope %s' % self.globalIsoNumber
            self.molNum = params[2]
            self.isoN = params[3]
            self.abundance = params[4]
            self.q296 = params[5]
            self.gj = params[6]
            self.molmass = params[7]
            self.q = {}
            _zeros_later(Isotope.lineSurvey, self, int((self.layer.rangeMax - self.layer.rangeMin) / utils.BASE_RESOLUTION))
            self.progressCrossSection = False

    # -- list protocol over the SoA ------------------------------------------------------
    def __len__(self):
        return int(self._lines["nu"].size)

    def __bool__(self):
        return True

    def _line(self, i):
        L = self._lines
        return Line(float(L["nu"][i]), float(L["sw"][i]), float(L["a"][i]), float(L["gamma_air"][i]),
                    float(L["gamma_self"][i]), float(L["elower"][i]), float(L["n_air"][i]),
                    float(L["delta_air"][i]), self)

    def __iter__(self):
        for i in range(len(self)):
            yield self._line(i)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._line(j) for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("list index out of range")
        return self._line(i)

    def append(self, line):
        vals = (line.wavenumber, line.intensity, line.einsteinA, line.airHalfWidth, line.selfHalfWidth,
                line.lowerEnergy, line.tempExponent, line.pressureShift)
        for f, v in zip(self._FIELDS, vals):
            self._lines[f] = np.append(self._lines[f], float(v))
        self._invalidate_lines()

    def pop(self, index=-1):
        line = self[index]
        n = len(self)
        keep = np.ones(n, dtype=bool)
        keep[index] = False
        self._lines = {f: v[keep] for f, v in self._lines.items()}
        self._invalidate_lines()
        return line

    def clear_lines(self):
        self._lines = {f: np.zeros(0) for f in self._FIELDS}
        self._invalidate_lines()

    def set_lines(self, lines: dict):
        """Install a structure-of-arrays line list (nu, sw, a, elower, gamma_air, gamma_self, n_air, delta_air)."""
        self._lines = {f: np.ascontiguousarray(lines[f], dtype=np.float64) if f in lines
                       else np.zeros(len(lines["nu"])) for f in self._FIELDS}
        self._invalidate_lines()

    def _invalidate_lines(self):
        if self._dev_lines is not None:
            self._dev_lines.free()
            self._dev_lines = None
        self.progressCrossSection = False
        self._inputs_version += 1
        self._struct_version += 1

    def _host_array_assigned(self, which, installed=True):
        if which == "_crossSection_host":           # somebody installed a host array: the device copy is stale
            self._dev_xsec_valid = False
            self._xs_deferred = False
            self._xs_version += 1
            self._xs_installed = bool(installed)
            if installed:
                self._struct_version += 1

    def _defer_cross_section(self):
        """A merged layer step (one accumulate job over all the layer's line lists, settings.LAYER_STEP) has just produced
        the layer's absorption coefficient WITHOUT this isotopologue's cross-section array.  The reference's protocol
        (cls:32-88) says the cross section is now computed: progressCrossSection is set as createCrossSection would, and
        the array is made by the per-line-list path when somebody reads ``crossSection`` (or a device-side consumer asks
        for it): getCrossSection(isotope), the molecule sums and the per-molecule getters all go through here."""
        if self.exotic or (self.progressCrossSection and not self._xs_deferred):
            return                                  # a computed, current array exists
        self._xs_deferred = True
        self._xs_installed = False                  # (what stands now is computed from the lines)
        self._dev_xsec_valid = False
        self._xs_version += 1
        self._regime_counts = None
        self.progressCrossSection = True
        Isotope.crossSection.defer(self, self._materialise_cross_section)

    def _materialise_cross_section(self):
        _compute_cross_sections([self])             # K1 + K2 for this line list; leaves the download deferred
        return self.crossSection

    @property
    def regimeCounts(self):
        """(gaussian, lorentz, voigt) line counts as printed at cls:406, from the device's regime
        select (lbl_line_quantities) - fetched when asked for, not on every createCrossSection."""
        if self._regime_counts is None:
            ctx = _ctx()
            g = self.layer._grid()
            q = ctx.line_quantities(self._device_lines(ctx), _iso_params(self), _engine.native_grid(dict(g, W=max(g["W"], 1))))
            c = np.bincount(q["regime"], minlength=3)
            self._regime_counts = (int(c[0]), int(c[1]), int(c[2]))
        return self._regime_counts

    # -- device residency ----------------------------------------------------------------
    def _device_lines(self, ctx):
        if self._dev_lines is None or self._dev_lines.h is None:
            # a window handed out by a MemorySource is a slice of a registered list: a VIEW of that list's one resident
            # copy (lbl_lines_view) instead of another upload - the 30 layers of a column, or a layer whose range or
            # pressure keeps changing, re-window the same three lists
            pooled = _engine.get_engine().pooled_lines(self._lines)
            self._dev_lines = pooled if pooled is not None else ctx.lines(self._lines)
        return self._dev_lines

    def _device_xsec(self, ctx, n):
        if self._dev_xsec is None or self._dev_xsec.h is None or self._dev_xsec.n < n or self._dev_xsec.ctx is not ctx:
            if self._dev_xsec is not None and self._dev_xsec.h is not None and self._dev_xsec.ctx.h:
                self._dev_xsec.free()
            self._dev_xsec = ctx.buffer(max(n, 1))
            import weakref
            weakref.finalize(self, _free_buffers, {"xsec": self._dev_xsec})
        return self._dev_xsec

    def _device_xsec_current(self, ctx, n):
        """Device copy of self.crossSection (uploaded if a host array was installed since)."""
        if self._xs_deferred:
            _compute_cross_sections([self])         # promised by a merged layer step: made now, on the device
        if (self._dev_xsec_valid and self._dev_xsec is not None and self._dev_xsec.h is not None
                and self._dev_xsec.ctx is ctx):
            return self._dev_xsec
        xs = np.ascontiguousarray(self.crossSection, dtype=np.float64)
        if xs.shape != (n,):
            raise ValueError("cross section has %s points, layer grid has %d" % (xs.shape, n))
        buf = self._device_xsec(ctx, n)
        buf.upload(xs)
        self._dev_xsec_valid = True
        return buf

    # -- reference surface ---------------------------------------------------------------
    def _layer(self):
        return self.layer

    def _sweep_members(self):
        return [[self]], [self.molecule.concentration]          # cls:324 uses the molecule's concentration

    P = property(lambda self: self.layer.P)
    T = property(lambda self: self.layer.T)
    depth = property(lambda self: self.layer.depth)
    rangeMin = property(lambda self: self.layer.rangeMin)
    rangeMax = property(lambda self: self.layer.rangeMax)
    resolution = property(lambda self: self.layer.resolution)
    distanceFromCenter = property(lambda self: self.layer.distanceFromCenter)
    yAxis = property(lambda self: np.copy(self.layer.yAxis))
    xAxis = property(lambda self: np.copy(self.layer.xAxis))

    @property
    def molMass(self):
        return self.molmass / 1000 / avo

    def getData(self):
        _say('Getting data for %s, isotope %s' % (self.molecule.name, self.globalIsoNumber))
        src = _data.get_source()
        lines = src.gatherData(self.globalIsoNumber, self.layer.effectiveRangeMin, self.layer.effectiveRangeMax)
        self.q = src.getQData(self.globalIsoNumber)
        self.set_lines(lines)
        _ctx()                                            # the reference computes the survey here (cls:359): fail now without a GPU
        Isotope.lineSurvey.defer(self, self.createLineSurvey)      # ... the histogram itself on first read

    def createCrossSection(self):
        """cls:361-407 on the device: K1 line prep, K2 owner-computes accumulate, K3 regrid."""
        self.progressCrossSection = False
        _compute_cross_sections([self])

    def createLineSurvey(self):
        """cls:409-428 on the device (K7)."""
        ctx = _ctx()
        g = self.layer._grid()
        n = int((self.rangeMax - self.rangeMin) / utils.BASE_RESOLUTION)
        out = ctx.buffer(max(n, 1))
        try:
            grid = _engine.native_grid(dict(g, n_base=n, W=max(g["W"], 1)))
            ctx.line_survey_dev(self._device_lines(ctx), grid, out)
            survey = out.download(n)
        finally:
            out.free()
        self.lineSurvey = survey
        return survey

    def linelist(self):
        return list(self)


# ----------------------------------------------------------------------------------------
# Molecule (cls:445-642)
# ----------------------------------------------------------------------------------------
class Molecule(_OpticalMixin, list):
    crossSection = _LazyArray("crossSection")      # sum of the isotopologue cross sections, summed and downloaded on read

    def __init__(self, shortNameOrMolNum, layer, isotopeDepth=1, **abundance):
        super().__init__()
        self.layer = layer
        self.concText = ''
        self.concentration = 0
        self.exotic = False
        for key in abundance:
            if key == 'ppm':
                self.setPPM(abundance[key])
            elif key == 'ppb':
                self.setPPB(abundance[key])
            elif key == 'percentage' or key == 'perc' or key == '%':
                self.setPercentage(abundance[key])
            elif key == 'concentration':
                self.setConcentration(abundance[key])
            else:
                print('Invalid concentration type. Use ppm, ppb, percentage, or concentration.')
        self._xsc_member = None
        if type(shortNameOrMolNum) is dict:
            self._init_from_xsc(shortNameOrMolNum)
            return
        self.isotopeDepth = isotopeDepth
        _copy_of_layer_cross_section(Molecule.crossSection, self, layer)
        try:
            int(shortNameOrMolNum)
            self.ID = int(shortNameOrMolNum)
            self.name = False
            self._by_number = True
        except ValueError:
            self.name = shortNameOrMolNum
            self.ID = MOLECULE_ID[self.name]
            self._by_number = False
        for isotope in getGlobalIsotope(self.ID, isotopeDepth):
            isoClass = Isotope(isotope, self)
            self.append(isoClass)
            if not self.name:
                self.name = isoClass.shortName
        self.progressCrossSection = False
        self.exotic = False

    def _init_from_xsc(self, spec):
        """cls:466-505: a molecule given as {name: xsc file name or index}.  The file fixes the
        layer's temperature and pressure (Torr / 0.75006 -> mbar), its table is brought to
        0.01 cm^-1 if coarser and merged onto the layer axis; the molecule holds no isotopologues
        and its cross section is never invalidated (cls:40)."""
        name = list(spec.keys())[0]
        filename = list(spec.values())[0]
        if type(filename) == int:
            filename = list(EXOTIC_IDS[name].keys())[filename] + '.txt'
        source = _data.get_xsc_source()
        table = source.processXscFile(name, filename)
        props = source.parseXscFileName(filename)
        rangeMin, rangeMax = (float(v) for v in props['RANGE'].split('-')[:2])
        temp = int(float(props['TEMP']))
        pressure = float(props['PRESSURE']) / _data.TORR_PER_MBAR
        self.name = name
        self._xsc_spec = dict(spec)
        self.exotic = True
        self._xsc_member = Isotope(name, self)      # the reference's dummyIso: holds the device copy here
        if temp != self.layer.T:
            self.layer.changeTemperature(temp)
        if pressure != self.layer.P:
            self.layer.changePressure(pressure)
        xAxis = np.arange(rangeMin, rangeMax, .01)
        if float(props['RES']) > .01:
            measured = interpolateArray(xAxis, table['wavenumber'], table['intensity'])
        else:
            measured = table['intensity']
        self.crossSection = mergeArray(self.layer.xAxis, xAxis, measured)
        self.progressCrossSection = True
        self._xsc_member.crossSection = self.crossSection
        self._xsc_member.progressCrossSection = True

    def __str__(self):
        return '%s: %s' % (self.name, self.concText)

    def __bool__(self):
        return True

    def _layer(self):
        return self.layer

    def _members(self):
        """What the device sweep reads for this molecule: its isotopologues, or the holder of a
        measured cross section (kept in step with self.crossSection)."""
        if not self.exotic:
            return list(self)
        if self._xsc_member.crossSection is not self.crossSection:
            self._xsc_member.crossSection = self.crossSection
            self._xsc_member._dev_xsec_valid = False
        return [self._xsc_member]

    def _sweep_members(self):
        return [self._members()], [self.concentration]

    def returnCopy(self, layer=None):
        valueUnit = self.concText.split()
        tempDict = {valueUnit[1]: float(valueUnit[0])}
        if self.exotic:         # the reference's copy fails on these (no isotopeDepth, cls:539): re-read the file
            return Molecule(dict(self._xsc_spec), layer if layer is not None else self.layer, **tempDict)
        # a molecule made from its HITRAN number carries the upper-case short name, which is not
        # a MOLECULE_ID key (the reference's copy raises KeyError there): copy by number instead
        newMolecule = Molecule(self.ID if self._by_number else self.name, layer if layer is not None else self.layer,
                               isotopeDepth=int(self.isotopeDepth), **tempDict)
        newMolecule.getData()
        return newMolecule

    def setPercentage(self, percentage):
        self.concentration = percentage / 100
        self.concText = '%s %%' % percentage
        resetCrossSection(self)

    def setPPM(self, ppm):
        self.concentration = ppm * 10**-6
        self.concText = '%s ppm' % ppm
        resetCrossSection(self)

    def setPPB(self, ppb):
        self.concentration = ppb * 10**-8          # sic (cls:554)
        self.concText = '%s ppb' % ppb
        resetCrossSection(self)

    def setConcentration(self, concentration):
        self.setPPM(concentration * 1E6)
        resetCrossSection(self)

    def getData(self):
        for isotope in self:
            isotope.getData()

    def createCrossSection(self):
        """cls:566-571: sum of the isotopologue cross sections (no abundance weighting).  The
        isotopologues are accumulated (with this molecule's sweep folded in when all of them are
        due); the sum itself is formed on the device when ``crossSection`` is read."""
        if self.exotic:
            return
        self._ensure_swept()
        self._mark_sum_ready(force=True)          # the reference re-sums on every call (cls:566-571)

    def _mark_sum_ready(self, force=False):
        """Defer ``crossSection`` = zeros + sum of the isotopologue cross sections to the first read.  A sum that
        is already deferred or loaded is kept only while the isotopologue cross sections it was made from are
        still the current ones (``_xs_version``: bumped by every recomputation and by an assigned host array);
        the loader always adds the device copies that are current when it runs."""
        if self.exotic:
            return
        isos = list(self)
        versions = [i._xs_version for i in isos]
        if self.progressCrossSection and not force and self.__dict__.get("_sum_versions") == versions:
            return
        n = int((self.rangeMax - self.rangeMin) / utils.BASE_RESOLUTION)

        def load():
            ctx = _ctx()
            return _sum_on_device(ctx, [i._device_xsec_current(ctx, n) for i in isos], n)
        Molecule.crossSection.defer(self, load)
        self.__dict__["_sum_versions"] = versions
        self.progressCrossSection = True

    def _members_ready(self):
        self._mark_sum_ready()

    @property
    def lineSurvey(self):
        """cls:589-594: sum of the isotopologue surveys (device sum, list order)."""
        return _sum_host_arrays([isotope.lineSurvey for isotope in self],
                                int((self.rangeMax - self.rangeMin) / utils.BASE_RESOLUTION))

    P = property(lambda self: self.layer.P)
    T = property(lambda self: self.layer.T)
    depth = property(lambda self: self.layer.depth)
    rangeMin = property(lambda self: self.layer.rangeMin)
    rangeMax = property(lambda self: self.layer.rangeMax)
    resolution = property(lambda self: self.layer.resolution)
    distanceFromCenter = property(lambda self: self.layer.distanceFromCenter)
    yAxis = property(lambda self: np.copy(self.layer.yAxis))
    xAxis = property(lambda self: np.copy(self.layer.xAxis))


def _sum_host_arrays(arrays, n):
    """zeros(n) + a0 + a1 + ... for host arrays, summed by the device kernel."""
    ctx = _ctx()
    tmp = []
    try:
        for a in arrays:
            tmp.append(ctx.buffer(max(n, 1)).upload(np.ascontiguousarray(a, dtype=np.float64)))
        return _sum_on_device(ctx, tmp, n)
    finally:
        for b in tmp:
            b.free()


def _sum_on_device(ctx, bufs, n):
    """zeros + b0 + b1 + ... in list order (cls:567-569, 685-687), on the device."""
    out = ctx.buffer(max(n, 1))
    try:
        ctx.sum_dev(bufs, n, out)
        return out.download(n)
    finally:
        out.free()


# ----------------------------------------------------------------------------------------
# Layer (cls:645-787)
# ----------------------------------------------------------------------------------------
class Layer(_OpticalMixin, list):
    hasAtmosphere = False
    crossSection = _LazyArray("crossSection")      # sum of the molecule cross sections, formed on read

    def __init__(self, depth, T, P, rangeMin, rangeMax, atmosphere=None, name='', dynamicResolution=True):
        super().__init__()
        self.rangeMin = rangeMin
        self.rangeMax = rangeMax
        self.T = T
        self.P = P
        self.depth = depth
        self.distanceFromCenter = self.P / 1013.25 * 5
        self.effectiveRangeMin = max(self.rangeMin - self.distanceFromCenter, 0)
        self.effectiveRangeMax = self.rangeMax + self.distanceFromCenter
        self.dynamicResolution = dynamicResolution
        self._set_resolution()
        if not atmosphere:
            if not Layer.hasAtmosphere:
                self.atmosphere = Atmosphere('generic')
                Layer.hasAtmosphere = self.atmosphere
            else:
                self.atmosphere = Layer.hasAtmosphere
        else:
            self.atmosphere = atmosphere
            self.hasAtmosphere = atmosphere
        _zeros_later(Layer.crossSection, self, int((rangeMax - rangeMin) / utils.BASE_RESOLUTION))
        self.progressCrossSection = False
        _live_layers[:] = [r for r in _live_layers if r() is not None] + [weakref.ref(self)]
        if not name:
            name = 'layer %s' % self.atmosphere.nextLayerName()
        self.name = name
        self.exotic = False

    def _set_resolution(self):
        if not self.dynamicResolution:
            self.resolution = utils.BASE_RESOLUTION
        else:
            self.resolution = max(10**int(np.log10((self.P / 1013.25))) * .01, utils.BASE_RESOLUTION)

    def _grid(self):
        """Grid scalars for the C ABI from the layer's CURRENT attributes (cls:672, 700, 377).  (Remembered by the attributes
        they are computed from: len(np.arange(...)) alone is 1 us, and the getters and the column ask for the grid of every
        layer on every call.)"""
        base = utils.BASE_RESOLUTION
        key = (self.distanceFromCenter, self.effectiveRangeMin, self.effectiveRangeMax, self.resolution, base, self.rangeMin, self.rangeMax)
        hit = self.__dict__.get("_grid_cache")
        if hit is not None and hit[0] == key:
            return hit[1]
        g = dict(dfc=self.distanceFromCenter, eff_min=self.effectiveRangeMin, eff_max=self.effectiveRangeMax,
                 resolution=self.resolution, base_resolution=base,
                 n_base=int((self.rangeMax - self.rangeMin) / base),
                 n_work=int((self.rangeMax - self.rangeMin) / self.resolution),
                 W=len(np.arange(0, self.distanceFromCenter, self.resolution)),
                 range_min=self.rangeMin, range_max=self.rangeMax)
        self.__dict__["_grid_cache"] = (key, g)
        return g

    def __str__(self):
        return '%s; %s' % (self.name, '; '.join(str(m) for m in self))

    def __bool__(self):
        return True

    def _layer(self):
        return self

    def _sweep_members(self):
        # Layer.absCoef (cls:707-712) walks the molecules through getAbsCoef; dirty ones are recomputed
        return [m._members() for m in self], [m.concentration for m in self]

    def _members_ready(self):
        for m in self:
            m._mark_sum_ready()

    def _column_stamp(self):
        """(values, versions) for Atmosphere's resident column: ``values`` changes when the layer's blocks on the C side must be
        re-read (a mutator changed T, P, the range, a concentration, the depth, the line lists, or somebody installed a cross
        section), ``versions`` when any of its line lists is due (resetCrossSection, cls:38-45).  A handful of attribute
        reads: this runs for every layer on every Atmosphere.transmission before the first kernel is enqueued."""
        ver = struct = 0
        conc = []
        for m in self:
            conc.append(m.concentration)
            for iso in m:
                ver += iso._inputs_version
                struct += iso._struct_version + id(iso)          # (WHICH isotopologues: a molecule swapped for another re-reads the layer)
        return (self.T, self.P, self.rangeMin, self.rangeMax, self.resolution, len(self), struct, tuple(conc), self.depth), ver

    def _merged_step_applies(self, flat, lbl):
        """settings.LAYER_STEP "merged" (default): the layer's property chain comes from one merged accumulate job when
        any of its line lists is due (all of them line-by-line: a measured cross-section table has no lines to merge).
        With every cross section current (somebody asked for each of them) the sweep kernel over those arrays is cheaper."""
        return (_merged_route(_ctx()) and bool(lbl) and len(lbl) == len(flat)      # (the reference's rounding chain, the Voigt shape: per-line-list entry points only)
                and len(flat) <= nat.limit("merged_lists_per_job")      # (more line lists: the per-line-list step, up to "arrays_per_layer")
                and not any(i._xs_installed and i.progressCrossSection for i in lbl)     # an installed array is not the lines' (advisor, round 5)
                and any(not i.progressCrossSection or i._xs_deferred for i in lbl))

    def _check_abs_coef_dT(self):
        """What Layer.absCoefDT refuses, before the device is touched."""
        if settings.LINE_SHAPE != "voigt":
            raise ValueError("dk/dT needs settings.set_line_shape(\"voigt\"): the reference line shape switches between Gaussian, "
                             "pseudo-Voigt and Lorentzian at lhw / ghw = 0.01 and 100, which makes k discontinuous in T")
        for m in self:
            if m.exotic:
                raise ValueError("dk/dT: %s is a measured cross-section table, which has no temperature model" % m.name)

    def _abs_coef_dT(self):
        """(device buffer, n) of dk/dT = sum_m f_m sum_iso d(sigma_iso)/dT - k / T, f_m = conc_m P / 1E4 / k_B / T as in absCoef:
        one lbl_xsec_voigt_dt_dev job per line list with dlnw_dT = -d ln Q / dT - 1 / T (the number density's 1 / T rides on
        every line), summed by the layer sweep, which is linear in its cross-section inputs.  Kept until an input changes
        (every mutator and settings.set_line_shape bump the isotopologues' input versions)."""
        self._check_abs_coef_dT()
        ctx = _ctx()
        g = self._grid()
        n = g["n_base"]
        members, conc = self._sweep_members()
        flat = [iso for isos in members for iso in isos]
        if len(flat) > nat.limit("arrays_per_layer"):
            raise ValueError("dk/dT: %d line lists in one layer, at most %d" % (len(flat), nat.limit("arrays_per_layer")))
        st = _kept_state(self, "_dT_state").reserve(ctx, n)
        key = (tuple((id(i), i._inputs_version) for i in flat), tuple(float(c) for c in conc), self.P, self.T, self.rangeMin,
               self.rangeMax, n, g["resolution"], settings.LINE_SHAPE)
        if st.key != key:
            out = st.buf(ctx, "abs_coef_dT")
            if not flat:
                out.fill(0.0)
            else:
                _check_window(g)
                jobs = [(iso._device_lines(ctx), _iso_params(iso), _engine.native_grid(g), st.buf(ctx, "dxs%d" % i))
                        for i, iso in enumerate(flat)]
                ctx.xsec_voigt_dT_dev(jobs, [-_dlnq_dT(iso) - 1.0 / float(self.T) for iso in flat])
                iso_mol = [m for m, isos in enumerate(members) for _ in isos]
                ctx.layer_sweep_dev([j[3] for j in jobs], iso_mol, conc, self.P, self.T, self.depth, self.rangeMin, self.rangeMax, n,
                                    abs_coef=out)
            st.key = key
        return st.bufs["abs_coef_dT"], n

    @property
    def absCoefDT(self):
        """dk/dT (per cm per K) on the layer's grid, analytic, under settings.set_line_shape("voigt") only (beyond the
        reference): line intensities (partition sum from the table's central difference, Boltzmann factor, stimulated
        emission), Doppler and Lorentz widths and the number density.  ValueError under the reference line shape (its regime
        switches make k discontinuous in T) and for a layer holding a measured cross-section table."""
        buf, n = self._abs_coef_dT()
        return buf.download(n, pinned=True)

    def createCrossSection(self):
        """cls:684-689: sum of the molecule cross sections.  One fused layer step brings every dirty
        line list up to date (and leaves absorption coefficient and transmittance resident for the
        getters that follow); the sum is formed on the device when ``crossSection`` is read."""
        self._ensure_swept()
        n = int((self.rangeMax - self.rangeMin) / utils.BASE_RESOLUTION)
        molecules = list(self)

        def load():
            ctx = _ctx()
            tmp = []
            try:
                for molecule in molecules:
                    xs = np.ascontiguousarray(getCrossSection(molecule), dtype=np.float64)
                    if xs.shape != (n,):        # e.g. a partially overlapping xsc table (mergeArray, cls:216-219)
                        raise ValueError("operands could not be broadcast together with shapes (%d,) %s" % (n, xs.shape))
                    tmp.append(ctx.buffer(max(n, 1)).upload(xs))
                return _sum_on_device(ctx, tmp, n)
            finally:
                for b in tmp:
                    b.free()
        Layer.crossSection.defer(self, load)
        self.progressCrossSection = True

    @property
    def lineSurvey(self):
        """cls:691-696: sum of the molecule surveys (device sum, list order)."""
        return _sum_host_arrays([molecule.lineSurvey for molecule in self],
                                int((self.rangeMax - self.rangeMin) / utils.BASE_RESOLUTION))

    @property
    def yAxis(self):
        return np.zeros(int((self.rangeMax - self.rangeMin) / self.resolution))

    @property
    def xAxis(self):
        return np.linspace(self.rangeMin, self.rangeMax, int((self.rangeMax - self.rangeMin) / utils.BASE_RESOLUTION),
                           endpoint=True)

    @property
    def title(self):
        return '%s\nP: %smBars; T: %sK; depth: %scm' % (str(self), self.P, self.T, self.depth)

    def changeRange(self, rangeMin, rangeMax):
        self.rangeMin = rangeMin
        self.rangeMax = rangeMax
        self.effectiveRangeMax = self.rangeMax + self.distanceFromCenter
        self.effectiveRangeMin = max(self.rangeMin - self.distanceFromCenter, 0)
        resetData(self)

    def changeTemperature(self, temperature):
        self.T = temperature
        resetCrossSection(self)

    def changePressure(self, pressure):
        self.P = pressure
        self.distanceFromCenter = self.P / 1013.25 * 5
        self._set_resolution()
        resetData(self)

    def changeDepth(self, depth):
        self.depth = depth

    def addMolecule(self, name, isotopeDepth=1, **abundance):
        molecule = Molecule(name, self, isotopeDepth, **abundance)
        self.append(molecule)
        if totalConcentration(self) > 1:
            print('**Warning : Concentrations exceed 1.')
        if not molecule.exotic:
            molecule.getData()
        return molecule

    def returnCopy(self):
        newCopy = Layer(self.depth, self.T, self.P, self.rangeMin, self.rangeMax,
                        self.atmosphere, name=self.atmosphere.nextLayerName(), dynamicResolution=self.dynamicResolution)
        for molecule in self:
            newCopy.append(molecule.returnCopy(newCopy))      # bound to the NEW layer (the reference binds to the old one)
        return newCopy

    def returnMoleculeObjects(self):
        return list(self)

    def planck(self, temperature):
        """pyradPlanck.planckWavenumber(self.xAxis, temperature) (cls:781-782, pl:38-44), on the device."""
        ctx = _ctx()
        n = int((self.rangeMax - self.rangeMin) / utils.BASE_RESOLUTION)
        st = _kept_state(self, "_planck_state")
        out = st.reserve(ctx, n).buf(ctx, "planck")
        ctx.planck_dev(self.rangeMin, self.rangeMax, n, float(temperature), out)
        return out.download(n, pinned=True)


# ----------------------------------------------------------------------------------------
# Level fluxes of a column (Atmosphere.fluxes; beyond the reference)
# ----------------------------------------------------------------------------------------
FLUX_DIFFUSIVITY = 1.66       # the "diffusivity" angle set: one angle, mu = 1 / 1.66, weight pi


def fluxAngles(angles=3):
    """The angle set of Atmosphere.fluxes as two float64 arrays (mu, weight), mu in (0, 1].
    - an integer N in 1..8: Gauss-Legendre on mu in [0, 1]: with x, w = numpy.polynomial.legendre.leggauss(N),
      mu_k = (x_k + 1) / 2 and W_k = pi w_k mu_k, so that sum W_k = pi and sum_k W_k I(mu_k) = 2 pi int_0^1 I(mu) mu dmu
      exactly for every polynomial I of degree <= 2N - 2;
    - "diffusivity": mu = 1 / 1.66, W = pi;
    - an explicit list of (mu, W) pairs.
    ValueError for anything else, N outside 1..8, more than 8 pairs or a mu outside (0, 1]."""
    nmax = 8
    if isinstance(angles, str):
        if angles != "diffusivity":
            raise ValueError("angles: an integer 1..%d, \"diffusivity\" or a list of (mu, weight) pairs, not %r" % (nmax, angles))
        return np.array([1.0 / FLUX_DIFFUSIVITY]), np.array([pi])
    if isinstance(angles, (int, np.integer)) and not isinstance(angles, bool):
        if not 1 <= int(angles) <= nmax:
            raise ValueError("angles: %d Gauss-Legendre angles, at most %d" % (int(angles), nmax))
        x, w = np.polynomial.legendre.leggauss(int(angles))
        mu = (x + 1.0) / 2.0
        return mu, pi * w * mu
    try:
        pairs = [(float(m), float(wt)) for m, wt in angles]
    except (TypeError, ValueError):
        raise ValueError("angles: an integer 1..%d, \"diffusivity\" or a list of (mu, weight) pairs, not %r" % (nmax, angles))
    if not 1 <= len(pairs) <= nmax:
        raise ValueError("angles: 1..%d (mu, weight) pairs, not %d" % (nmax, len(pairs)))
    mu = np.array([m for m, _ in pairs])
    weight = np.array([wt for _, wt in pairs])
    if not np.all((mu > 0.0) & (mu <= 1.0)):
        raise ValueError("angles: every mu must lie in (0, 1]")
    if not np.all(np.isfinite(weight)):
        raise ValueError("angles: every weight must be finite")
    return mu, weight


def heatingRates(net, P, T, depth):
    """Heating rate of every layer in K/day from the net flux (W m^-2) at its levels: H_l = -(F_(l+1) - F_l) / (c_p m_l) *
    86400 with the layer's mass per unit area m_l = (100 P_l / (R_d T_l)) (depth_l / 100) kg m^-2 (P in mbar, depth in cm,
    c_p = CP_AIR, R_d = R_DRY_AIR).  ``net``: (..., L + 1); P, T, depth: L values each; returns (..., L)."""
    net = np.asarray(net, dtype=np.float64)
    P, T, depth = (np.asarray(v, dtype=np.float64) for v in (P, T, depth))
    mass = (100.0 * P / (R_DRY_AIR * T)) * (depth / 100.0)
    return -(net[..., 1:] - net[..., :-1]) / (CP_AIR * mass) * 86400.0


def _flux_bands(rangeMin, rangeMax, n, bands):
    """(first, count) grid-index ranges of the bands: band (lo, hi) holds the points of linspace(rangeMin, rangeMax, n) with
    lo <= nu < hi (hi may lie beyond rangeMax, so that a band can end with the last point)."""
    if bands is None:
        if n < 1:
            raise ValueError("the wavenumber range holds no grid point")
        return [0], [n]
    bands = list(bands)
    nmax = 64
    if not bands:
        raise ValueError("bands: give at least one (lo, hi) band, or None for the whole range")
    if len(bands) > nmax:
        raise ValueError("bands: at most %d bands, not %d" % (nmax, len(bands)))
    x = np.linspace(rangeMin, rangeMax, n)
    first, count = [], []
    for b, band in enumerate(bands):
        try:
            lo, hi = (float(v) for v in band)
        except (TypeError, ValueError):
            raise ValueError("bands: band %d is not a (lo, hi) pair: %r" % (b, band))
        if not (lo >= rangeMin and lo <= rangeMax):
            raise ValueError("bands: band %d (%g, %g) starts outside the range [%g, %g]" % (b, lo, hi, rangeMin, rangeMax))
        i0, i1 = int(np.searchsorted(x, lo, "left")), int(np.searchsorted(x, hi, "left"))
        if i1 <= i0:
            raise ValueError("bands: band %d (%g, %g) holds no grid point" % (b, lo, hi))
        first.append(i0)
        count.append(i1 - i0)
    return first, count


def _grid_spectrum(name, spec, n):
    """``spec`` as n contiguous float64 values (ValueError for another shape), or None."""
    if spec is None:
        return None
    spec = np.ascontiguousarray(spec, dtype=np.float64)
    if spec.shape != (n,):
        raise ValueError("%s: %d grid points expected, got shape %s" % (name, n, spec.shape))
    return spec


REFLECTIONS = ("lambertian", "specular")        # the C ABI's ``reflection`` is the index


def _surface_emissivity(emissivity, x):
    """The ``emissivity`` of fluxes() and radiance() on the grid ``x``: a float for a number, else len(x) contiguous float64
    values - an array of that many values, or a pair (wavenumbers, values) interpolated with np.interp onto x (the end
    values held beyond the table).  ValueError for anything else, a value outside [0, 1] or a NaN."""
    n = len(x)
    bad = "emissivity: a number in [0, 1], %d values on xAxis or a pair (wavenumbers, values), not %r"
    if isinstance(emissivity, (bool, str)):
        raise ValueError(bad % (n, emissivity))
    if isinstance(emissivity, (int, float, np.integer, np.floating)):
        e = float(emissivity)
        if not 0.0 <= e <= 1.0:
            raise ValueError("emissivity: %r is outside [0, 1]" % (emissivity,))
        return e
    table = isinstance(emissivity, (tuple, list)) and len(emissivity) == 2 and all(np.ndim(v) == 1 for v in emissivity)
    try:
        if table:
            nu, val = (np.asarray(v, dtype=np.float64) for v in emissivity)
        else:
            e = np.ascontiguousarray(emissivity, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(bad % (n, emissivity))
    if table:
        if nu.size < 1 or nu.shape != val.shape or not np.all(np.isfinite(nu)) or np.any(np.diff(nu) <= 0):
            raise ValueError("emissivity: a table needs as many values as wavenumbers, the wavenumbers finite and increasing")
        e = np.ascontiguousarray(np.interp(x, nu, val))
    elif e.shape != (n,):
        raise ValueError("emissivity: %d grid points expected, got shape %s" % (n, e.shape))
    if not np.all((e >= 0.0) & (e <= 1.0)):             # (a NaN fails both comparisons)
        raise ValueError("emissivity: every value must lie in [0, 1]")
    return e


def _weight_sum(weight):
    """W_0 + W_1 + ... added in angle order, as lbl_column_flux_surface_dev adds them; ValueError unless it is > 0"""
    total = 0.0
    for w in weight:
        total += float(w)
    if not (total > 0.0 and total != float("inf")):
        raise ValueError("angles: over a reflecting surface the weights must add up to a finite sum > 0, not %r" % (total,))
    return total


def _surface_reflection(reflection):
    if not isinstance(reflection, str) or reflection not in REFLECTIONS:
        raise ValueError("reflection: \"lambertian\" or \"specular\", not %r" % (reflection,))
    return REFLECTIONS.index(reflection)


PLANCK_SOURCES = ("layer", "linear")


def _planck_source(planck, levelTemperatures):
    """True for the source linear in optical depth; ValueError for anything but "layer" and "linear", and for level
    temperatures that the layer source would ignore"""
    if not isinstance(planck, str) or planck not in PLANCK_SOURCES:
        raise ValueError("planck is \"layer\" or \"linear\", not %r" % (planck,))
    if planck == "layer" and levelTemperatures is not None:
        raise ValueError("levelTemperatures belong to planck=\"linear\"; planck=\"layer\" uses the layers' temperatures")
    return planck == "linear"


def _band_values(bands, values):
    """Copies of per-band results (leading band axis): without ``bands`` each one's single band alone."""
    return [(v[0] if bands is None else v).copy() for v in values]


class Fluxes:
    """What Atmosphere.fluxes returns.  ``up``, ``down``, ``net``: W m^-2 at the levels 0 (surface) .. L (top), shape (L + 1,)
    or (n_bands, L + 1); ``heatingRate``: K/day per layer, (L,) or (n_bands, L); ``mu``, ``weight``: the angle set used;
    ``upSpectrum`` / ``downSpectrum``: the spectral upward flux at the top and downward flux at the surface (W m^-2 per
    cm^-1, n points; 0 at points outside every band) when asked for, else None; ``upSurfaceSpectrum``: likewise the
    spectral upward flux at the surface, over a surface with an emissivity only."""

    def __init__(self, up, down, heatingRate, mu, weight, upSpectrum=None, downSpectrum=None, upSurfaceSpectrum=None):
        self.up = up
        self.down = down
        self.net = up - down
        self.heatingRate = heatingRate
        self.mu = mu
        self.weight = weight
        self.upSpectrum = upSpectrum
        self.downSpectrum = downSpectrum
        self.upSurfaceSpectrum = upSurfaceSpectrum

    def __repr__(self):
        return "Fluxes(levels=%d, angles=%d, up[top]=%s, down[surface]=%s)" % (
            self.up.shape[-1], len(self.mu), self.up[..., -1], self.down[..., 0])


# ----------------------------------------------------------------------------------------
# The direct solar beam (Atmosphere.solarFluxes; beyond the reference)
# ----------------------------------------------------------------------------------------
R_SUN = 6.957e8               # m, the nominal solar radius
AU = 1.495978707e11           # m
SOLAR_GEOMETRIES = ("plane", "spherical")


def solarIrradiance(xAxis, temperature=5772.0, distanceAU=1.0):
    """The irradiance of a black-body sun on a plane normal to its beam, W m^-2 per cm^-1 at the wavenumbers ``xAxis``:
    planckWavenumber(x, temperature) * pi * (R_SUN / (AU * distanceAU))**2 (0 at a wavenumber of 0).  Summed over all
    wavenumbers at 5772 K and 1 AU it is sigma T^4 (R_SUN / AU)^2 = 1361 W m^-2.  ValueError unless temperature and
    distanceAU are finite and > 0."""
    try:
        T, d = float(temperature), float(distanceAU)
    except (TypeError, ValueError):
        raise ValueError("solarTemperature and distanceAU: two numbers > 0, not %r and %r" % (temperature, distanceAU))
    if not (T > 0.0 and math.isfinite(T)):
        raise ValueError("solarTemperature must be finite and > 0, not %r" % (temperature,))
    if not (d > 0.0 and math.isfinite(d)):
        raise ValueError("distanceAU must be finite and > 0, not %r" % (distanceAU,))
    x = np.asarray(xAxis, dtype=np.float64)
    return np.where(x > 0.0, planckWavenumber(x, T), 0.0) * pi * (R_SUN / (AU * d)) ** 2


def _solar_beams(mu0):
    """``mu0`` of solarFluxes as two float64 arrays (cosine, weight): a number (weight 1) or a list of up to 8 (mu0, weight)
    pairs; every cosine in (0, 1], every weight finite and >= 0."""
    nmax = 8
    bad = "mu0: a cosine in (0, 1] or a list of up to %d (mu0, weight) pairs, not %r"
    if isinstance(mu0, (bool, str)):
        raise ValueError(bad % (nmax, mu0))
    if isinstance(mu0, (int, float, np.integer, np.floating)):
        pairs = [(float(mu0), 1.0)]
    else:
        try:
            pairs = [(float(m), float(wt)) for m, wt in mu0]
        except (TypeError, ValueError):
            raise ValueError(bad % (nmax, mu0))
    if not 1 <= len(pairs) <= nmax:
        raise ValueError("mu0: 1..%d beams, not %d" % (nmax, len(pairs)))
    mu = np.array([m for m, _ in pairs])
    weight = np.array([wt for _, wt in pairs])
    if not np.all((mu > 0.0) & (mu <= 1.0)):                # (a NaN fails both comparisons)
        raise ValueError("mu0: every cosine must lie in (0, 1]")
    if not np.all(np.isfinite(weight) & (weight >= 0.0)):
        raise ValueError("mu0: every weight must be finite and >= 0")
    return mu, weight


def solarSlants(depths, mu0, geometry="plane", planetRadius=6.371e8):
    """The path length of a solar beam through every layer per unit depth: (L,) for a number ``mu0``, (beams, L) for a list
    of (mu0, weight) pairs.  ``depths``: the layers' depths bottom to top, cm, each > 0.
    - "plane": 1 / mu0 in every layer.
    - "spherical": the straight ray, WITHOUT REFRACTION, that meets the surface at zenith cosine mu0, through the shells of
      Atmosphere.limbPath around a planet of radius ``planetRadius`` (cm).  With z_l the level heights (z_0 = 0) and
      q(z) = sqrt(z (2 R + z) + R^2 mu0^2), the distance along the ray from its point nearest the planet's centre,
          slant_l = (q(z_(l+1)) - q(z_l)) / depth_l
      evaluated in the factored form (a_(l+1) + a_l) / (q(z_(l+1)) + q(z_l)) with a = R + z, q = sqrt((a - b) (a + b)) and
      b = R sqrt((1 - mu0) (1 + mu0)), which keeps its digits (no difference of two long distances) and is exactly 1 for
      mu0 = 1.  Every slant is <= 1 / mu0 and tends to it as the radius grows.
    Only the path length is spherical: the projection of the beam's irradiance onto the horizontal stays mu0 at every
    level (solarFluxes' beam weight), as in the plane-parallel case.
    ValueError for another geometry, a radius that is not finite and > 0, or a depth that is not finite and > 0."""
    if not isinstance(geometry, str) or geometry not in SOLAR_GEOMETRIES:
        raise ValueError("geometry: \"plane\" or \"spherical\", not %r" % (geometry,))
    try:
        R = float(planetRadius)
    except (TypeError, ValueError):
        raise ValueError("planetRadius must be finite and > 0, not %r" % (planetRadius,))
    if not (R > 0.0 and math.isfinite(R)):
        raise ValueError("planetRadius must be finite and > 0, not %r" % (planetRadius,))
    single = isinstance(mu0, (int, float, np.integer, np.floating)) and not isinstance(mu0, bool)
    mu, _ = _solar_beams(mu0)
    try:
        depth = np.asarray([float(d) for d in depths], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("depths: the layers' depths in cm, not %r" % (depths,))
    if not np.all(np.isfinite(depth) & (depth > 0.0)):
        raise ValueError("depths: every depth must be finite and > 0")
    table = np.empty((len(mu), len(depth)))
    if geometry == "plane":
        table[:] = (1.0 / mu)[:, None]
    else:
        a = R + np.concatenate([[0.0], np.cumsum(depth)])
        for s, m in enumerate(mu):
            b = R * math.sqrt((1.0 - m) * (1.0 + m))
            q = np.sqrt((a - b) * (a + b))
            table[s] = (a[1:] + a[:-1]) / (q[1:] + q[:-1])
    return table[0] if single else table


def _solar_spectrum(solarSpectrum, solarTemperature, distanceAU, x):
    """The beam's irradiance at the top on the grid ``x`` as len(x) contiguous float64 values, finite and >= 0: from exactly
    one of ``solarSpectrum`` (a number, len(x) values, or a pair (wavenumbers, values) interpolated as _surface_emissivity
    does) and ``solarTemperature`` (solarIrradiance)."""
    n = len(x)
    if (solarSpectrum is None) == (solarTemperature is None):
        raise ValueError("give exactly one of solarSpectrum and solarTemperature")
    if solarSpectrum is None:
        S = solarIrradiance(x, solarTemperature, distanceAU)
    else:
        bad = "solarSpectrum: a number >= 0, %d values on xAxis or a pair (wavenumbers, values), not %r"
        if isinstance(solarSpectrum, (bool, str)):
            raise ValueError(bad % (n, solarSpectrum))
        table = (isinstance(solarSpectrum, (tuple, list)) and len(solarSpectrum) == 2
                 and all(np.ndim(v) == 1 for v in solarSpectrum))
        try:
            if isinstance(solarSpectrum, (int, float, np.integer, np.floating)):
                S = np.full(n, float(solarSpectrum))
            elif table:
                nu, val = (np.asarray(v, dtype=np.float64) for v in solarSpectrum)
            else:
                S = np.asarray(solarSpectrum, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(bad % (n, solarSpectrum))
        if table:
            if nu.size < 1 or nu.shape != val.shape or not np.all(np.isfinite(nu)) or np.any(np.diff(nu) <= 0):
                raise ValueError("solarSpectrum: a table needs as many values as wavenumbers, the wavenumbers finite and increasing")
            S = np.interp(x, nu, val)
        elif S.shape != (n,):
            raise ValueError("solarSpectrum: %d grid points expected, got shape %s" % (n, S.shape))
    S = np.ascontiguousarray(S, dtype=np.float64)
    if not np.all(np.isfinite(S) & (S >= 0.0)):
        raise ValueError("solarSpectrum: every value must be finite and >= 0")
    return S


def _solar_source_key(solarSpectrum, solarTemperature, distanceAU):
    """What names a source that is made from numbers alone - a black body or one value at every point - else None (also
    for numbers that _solar_spectrum will refuse)"""
    try:
        if solarSpectrum is None and solarTemperature is not None:
            return ("black body", float(solarTemperature), float(distanceAU))
        if isinstance(solarSpectrum, (int, float, np.integer, np.floating)) and not isinstance(solarSpectrum, bool):
            return ("constant", float(solarSpectrum)) if solarTemperature is None else None
    except (TypeError, ValueError):
        pass
    return None


class SolarFluxes:
    """What Atmosphere.solarFluxes returns.  ``up``, ``down``, ``net`` (= up - down, Fluxes' sign): W m^-2 at the levels 0
    (surface) .. L (top), shape (L + 1,) or (n_bands, L + 1); ``heatingRate``: K/day per layer, (L,) or (n_bands, L);
    ``absorbedSurface`` = down[0] - up[0], what the surface takes up, per band; ``mu0``, ``beamWeight`` (= weight mu0, what
    multiplies a beam in a level's flux) and ``slant`` (beams, L): the beams used; ``mu``, ``weight``: the diffuse angles
    of a Lambertian surface; ``upSpectrum`` / ``downSpectrum`` / ``upSurfaceSpectrum``: the spectral upward flux at the top,
    downward flux at the surface and upward flux at the surface (W m^-2 per cm^-1, n points; 0 outside every band) when
    asked for, else None."""

    def __init__(self, up, down, heatingRate, mu0, beamWeight, slant, mu, weight, upSpectrum=None, downSpectrum=None,
                 upSurfaceSpectrum=None):
        self.up = up
        self.down = down
        self.net = up - down
        self.heatingRate = heatingRate
        self.absorbedSurface = down[..., 0] - up[..., 0]
        self.mu0 = mu0
        self.beamWeight = beamWeight
        self.slant = slant
        self.mu = mu
        self.weight = weight
        self.upSpectrum = upSpectrum
        self.downSpectrum = downSpectrum
        self.upSurfaceSpectrum = upSurfaceSpectrum

    def __repr__(self):
        return "SolarFluxes(levels=%d, beams=%d, down[top]=%s, down[surface]=%s, up[top]=%s)" % (
            self.up.shape[-1], len(self.mu0), self.down[..., -1], self.down[..., 0], self.up[..., -1])


# ----------------------------------------------------------------------------------------
# Two-stream multiple scattering of the solar beam (Atmosphere.solarFluxesTwoStream; beyond the reference)
# ----------------------------------------------------------------------------------------
MAX_SCATTERERS = 4
TWOSTREAM_WORKSPACE_BYTES = 256 << 20      # the most solarFluxesTwoStream keeps for its workspace


def _spectral_quantity(name, value, x, lo, hi, open_ends=False):
    """A scatterer's ``name`` on the grid ``x``: a float for a number, else len(x) contiguous float64 values - that many
    values, or a pair (wavenumbers, values) interpolated with np.interp as _surface_emissivity does.  ValueError (it names
    ``name``) for anything else and for a value that is not finite or lies outside [lo, hi] ((lo, hi) with open_ends)."""
    n = len(x)
    bad = name + ": a number, %d values on xAxis or a pair (wavenumbers, values), not %r"
    if isinstance(value, (bool, str)) or value is None:
        raise ValueError(bad % (n, value))
    table = isinstance(value, (tuple, list)) and len(value) == 2 and all(np.ndim(v) == 1 for v in value)
    try:
        if isinstance(value, (int, float, np.integer, np.floating)):
            v = np.float64(value)
        elif table:
            nu, val = (np.asarray(t, dtype=np.float64) for t in value)
        else:
            v = np.ascontiguousarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(bad % (n, value))
    if table:
        if nu.size < 1 or nu.shape != val.shape or not np.all(np.isfinite(nu)) or np.any(np.diff(nu) <= 0):
            raise ValueError(name + ": a table needs as many values as wavenumbers, the wavenumbers finite and increasing")
        v = np.ascontiguousarray(np.interp(x, nu, val))
    elif v.ndim and v.shape != (n,):
        raise ValueError("%s: %d grid points expected, got shape %s" % (name, n, v.shape))
    inside = (v > lo) & (v < hi) if open_ends else (v >= lo) & (v <= hi)
    if not np.all(inside & np.isfinite(v)):
        raise ValueError("%s: every value must be finite and lie in %s%g, %g%s" % (name, "([" [not open_ends], lo, hi,
                                                                                   ")]"[not open_ends]))
    return v if v.ndim else float(v)


class Scatterer:
    """Something that scatters sunlight in Atmosphere.solarFluxesTwoStream: ``amounts``, one per layer bottom to top, finite
    and >= 0, in the unit the extinction is per (molecules cm^-2 for a cross section in cm^2; 1 where ``extinction`` is the
    layer's optical depth itself); ``extinction`` >= 0, ``singleScatteringAlbedo`` in [0, 1] and ``asymmetry`` in (-1, 1),
    each a number, n values on the column's xAxis or a pair (wavenumbers, values) interpolated onto it.  The spectral
    quantities are checked against the grid by the call that uses them.  Atmosphere.fluxesTwoStream takes the same objects
    for the thermal fluxes."""

    def __init__(self, amounts, extinction=1.0, singleScatteringAlbedo=1.0, asymmetry=0.0, name=None):
        try:
            self.amounts = np.array([float(a) for a in amounts], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("amounts: one number per layer, not %r" % (amounts,))
        if not np.all(np.isfinite(self.amounts) & (self.amounts >= 0.0)):
            raise ValueError("amounts: every amount must be finite and >= 0")
        self.extinction = extinction
        self.singleScatteringAlbedo = singleScatteringAlbedo
        self.asymmetry = asymmetry
        self.name = name

    def _on_grid(self, x):
        """(extinction, albedo, asymmetry) on the grid x, each a float or len(x) values"""
        return (_spectral_quantity("extinction", self.extinction, x, 0.0, float("inf")),
                _spectral_quantity("singleScatteringAlbedo", self.singleScatteringAlbedo, x, 0.0, 1.0),
                _spectral_quantity("asymmetry", self.asymmetry, x, -1.0, 1.0, open_ends=True))

    def __repr__(self):
        return "Scatterer(%s%d layers)" % ("%r, " % self.name if self.name else "", len(self.amounts))


def rayleighCrossSection(xAxis):
    """The Rayleigh scattering cross section of air, cm^2 per molecule, at the wavenumbers ``xAxis`` (cm^-1): Bucholtz
    (1995), sigma = A lam^-(B + C lam + D / lam) with lam = 1e4 / nu in micrometres and (A, B, C, D) =
    (4.01061e-28, 3.99668, 1.10298e-3, 2.71393e-2) for lam > 0.5, (3.01577e-28, 3.55212, 1.35579, 0.11563) for lam <= 0.5;
    0 at a wavenumber of 0."""
    nu = np.asarray(xAxis, dtype=np.float64)
    lam = 1e4 / np.where(nu > 0.0, nu, 1.0)
    long_ = lam > 0.5
    A = np.where(long_, 4.01061e-28, 3.01577e-28)
    B = np.where(long_, 3.99668, 3.55212)
    C = np.where(long_, 1.10298e-3, 1.35579)
    D = np.where(long_, 2.71393e-2, 0.11563)
    return np.where(nu > 0.0, A * lam ** -(B + C * lam + D / lam), 0.0)


def rayleighScatterer(atmosphere):
    """The air of ``atmosphere`` as a Scatterer: per layer 100 P / (k T) * 1e-6 * depth molecules cm^-2 (P in mbar, depth in
    cm), rayleighCrossSection on the layers' xAxis, albedo 1, asymmetry 0."""
    layers, _ = atmosphere._column_layers()
    amounts = [100.0 * L.P / (k * L.T) * 1e-6 * L.depth for L in layers]
    return Scatterer(amounts, rayleighCrossSection(layers[0].xAxis), 1.0, 0.0, name="rayleigh")


def _scatterers(scatterers, n_layers):
    """``scatterers`` of solarFluxesTwoStream as a list of at most MAX_SCATTERERS Scatterers with n_layers amounts each"""
    if isinstance(scatterers, Scatterer):
        scatterers = [scatterers]
    try:
        scatterers = list(scatterers)
    except TypeError:
        raise ValueError("scatterers: a list of Scatterer objects, not %r" % (scatterers,))
    if len(scatterers) > MAX_SCATTERERS:
        raise ValueError("scatterers: at most %d, not %d" % (MAX_SCATTERERS, len(scatterers)))
    for c, sc in enumerate(scatterers):
        if not isinstance(sc, Scatterer):
            raise ValueError("scatterers: entry %d is not a Scatterer: %r" % (c, sc))
        if len(sc.amounts) != n_layers:
            raise ValueError("scatterers: entry %d has %d amounts for %d layers" % (c, len(sc.amounts), n_layers))
    return scatterers


class TwoStreamFluxes:
    """What Atmosphere.solarFluxesTwoStream returns.  ``up``, ``down`` (diffuse plus direct), ``direct`` and ``net``
    (= up - down): W m^-2 at the levels 0 (surface) .. L (top), shape (L + 1,) or (n_bands, L + 1); ``heatingRate``: K/day per
    layer; ``absorbedSurface`` = down[0] - up[0]; ``mu0``, ``beamWeight``, ``slant``: the beams used; ``upSpectrum`` (top),
    ``downSpectrum`` (surface, diffuse plus direct), ``directSpectrum`` (surface) and ``upSurfaceSpectrum``: W m^-2 per cm^-1,
    n points, 0 outside every band, when asked for, else None."""

    def __init__(self, up, down, direct, heatingRate, mu0, beamWeight, slant, upSpectrum=None, downSpectrum=None,
                 directSpectrum=None, upSurfaceSpectrum=None):
        self.up = up
        self.down = down
        self.direct = direct
        self.net = up - down
        self.heatingRate = heatingRate
        self.absorbedSurface = down[..., 0] - up[..., 0]
        self.mu0 = mu0
        self.beamWeight = beamWeight
        self.slant = slant
        self.upSpectrum = upSpectrum
        self.downSpectrum = downSpectrum
        self.directSpectrum = directSpectrum
        self.upSurfaceSpectrum = upSurfaceSpectrum

    def __repr__(self):
        return "TwoStreamFluxes(levels=%d, beams=%d, down[top]=%s, down[surface]=%s, direct[surface]=%s, up[top]=%s)" % (
            self.up.shape[-1], len(self.mu0), self.down[..., -1], self.down[..., 0], self.direct[..., 0], self.up[..., -1])


class Jacobians:
    """What Atmosphere.jacobians returns (a leading band axis on every band value when ``bands`` was given).
    ``olr``: upward flux at the top, W m^-2; ``surfaceTemperature``: dF/dT_s in W m^-2 K^-1, None when a surface spectrum was
    given; ``temperature``: (L,) dF/dT_l, Planck part; ``opticalDepth``: (L,) dF/d ln tau_l; ``molecules``: one array per
    layer, aligned with list(layer), dF/d ln n of every molecule (None when not asked for); ``moleculeNames``: their names;
    ``mu``, ``weight``: the angle set; ``temperatureSpectrum`` / ``opticalDepthSpectrum``: (L, n) spectral dF/dT_l and
    dF/d ln tau_l (W m^-2 per cm^-1, 0 outside every band) when asked for, else None (the temperature spectrum is the Planck
    part whatever ``temperature`` was).  ``temperatureAbsorption``: (L,) the absorption part of dF/dT_l, through dk_l/dT, and
    ``temperatureFull`` = temperature + temperatureAbsorption: both None unless temperature="full" was asked for.
    ``emissivity``: dF/de per band, W m^-2 per unit emissivity, over a surface with an emissivity (None over the black
    surface); ``emissivitySpectrum``: (n,) the spectral dF/de when spectra were asked for as well, else None.
    From Atmosphere.jacobiansLinear only (else None): ``edgeTemperature``: (L, 2) dF/dT of the bottom and the top edge of
    every layer; ``levelTemperature``: (L + 1,) dF/d(level temperature), level i the top edge of layer i - 1 plus the bottom
    edge of layer i; ``levelTemperatureSpectrum``: (L + 1, n) with spectra.  ``temperature`` is then the chain through the
    default level temperatures, or None when level temperatures were given, and temperatureSpectrum is None.
    From Atmosphere.jacobiansTwoStream only (else None): ``scatterers``: (C, L) dF/d ln amount of scatterer c in layer l."""

    def __init__(self, olr, surfaceTemperature, temperature, opticalDepth, molecules, moleculeNames, mu, weight,
                 temperatureSpectrum=None, opticalDepthSpectrum=None, temperatureAbsorption=None, emissivity=None,
                 emissivitySpectrum=None, edgeTemperature=None, levelTemperature=None, levelTemperatureSpectrum=None,
                 scatterers=None):
        self.olr = olr
        self.surfaceTemperature = surfaceTemperature
        self.temperature = temperature
        self.opticalDepth = opticalDepth
        self.molecules = molecules
        self.moleculeNames = moleculeNames
        self.mu = mu
        self.weight = weight
        self.temperatureSpectrum = temperatureSpectrum
        self.opticalDepthSpectrum = opticalDepthSpectrum
        self.temperatureAbsorption = temperatureAbsorption
        self.temperatureFull = (None if temperatureAbsorption is None or temperature is None
                                else temperature + temperatureAbsorption)
        self.emissivity = emissivity
        self.emissivitySpectrum = emissivitySpectrum
        self.edgeTemperature = edgeTemperature
        self.levelTemperature = levelTemperature
        self.levelTemperatureSpectrum = levelTemperatureSpectrum
        self.scatterers = scatterers

    def __repr__(self):
        return "Jacobians(layers=%d, angles=%d, olr=%s)" % (self.opticalDepth.shape[-1], len(self.mu), self.olr)


# ----------------------------------------------------------------------------------------
# Instrument channels (Instrument, convolve, Atmosphere.observe; beyond the reference)
# ----------------------------------------------------------------------------------------
def planckWavenumber(wavenumber, temp):
    """pyradPlanck.py:38-44 (wavenumber in cm^-1, Wm-2sr-1(cm-1)-1) in host NumPy, for channel centres; a spectrum on the
    grid comes from Layer.planck, on the device."""
    nu = np.asarray(wavenumber, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        a = 2E8 * h * c**2 * nu**3
        b = 100 * h * c * nu / k / temp
        return a / (np.exp(b) - 1)


def brightnessTemperature(wavenumber, radiance):
    """The temperature at which planckWavenumber(wavenumber, T) equals ``radiance`` (host NumPy): 100 h c nu / k /
    log1p(a / R) with a = 2E8 h c^2 nu^3.  NaN where the radiance is not > 0."""
    nu = np.asarray(wavenumber, dtype=np.float64)
    R = np.asarray(radiance, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        a = 2E8 * h * c**2 * nu**3
        T = 100 * h * c * nu / k / np.log1p(a / R)
    return np.where(R > 0, T, np.nan)


def _planck_dT(wavenumber, temp):
    """dB/dT of planckWavenumber: B b e^b / ((e^b - 1) T), b = 100 h c nu / k / T (the expression jacobians() documents)."""
    nu = np.asarray(wavenumber, dtype=np.float64)
    temp = np.asarray(temp, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        b = 100 * h * c * nu / k / temp
        return planckWavenumber(nu, temp) * b * np.exp(b) / ((np.exp(b) - 1) * temp)


class Instrument:
    """The channels of an instrument: centres in cm^-1 and one instrument line shape (host-only description).

    ``shape`` and the meaning of ``width`` (a scalar or one value per channel, cm^-1), with t = (nu - centre) / width:
        "gaussian"  exp(-4 ln2 t^2)                     width = FWHM
        "triangle"  max(0, 1 - |t|)                     width = FWHM, half the base
        "boxcar"    1 for |t| <= 0.5, else 0            width = full width
        "sinc"      sin(pi t) / (pi t)                  width = centre to first zero, 1 / (2 OPD)
        "table"     ``table`` = (offsets, values): values at uniformly spaced offsets (cm^-1) symmetric about 0, linear
                    in between, 0 outside; no width
    ``cutoff``: half support in cm^-1 (a scalar or per channel); default 3 width (gaussian), width (triangle), width / 2
    (boxcar), the table's half extent (table); a sinc needs one.  The centres need not be sorted or uniform.  A channel value
    is sum_j w_j S_j / sum_j w_j over the grid points within the cutoff: nothing is renormalised at the ends of a range, a
    channel that hangs over one is refused (support)."""

    def __init__(self, centres, shape="gaussian", width=None, cutoff=None, table=None):
        if shape not in nat.ILS_SHAPES:
            raise ValueError("shape: one of %s, not %r" % (", ".join(nat.ILS_SHAPES), shape))
        try:
            centres = np.array(centres, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("centres: a 1-D sequence of wavenumbers, not %r" % (centres,))
        if centres.ndim != 1 or centres.size < 1 or not np.all(np.isfinite(centres)):
            raise ValueError("centres: a non-empty 1-D sequence of finite wavenumbers")
        if centres.size > nat.limit("ils_channels"):
            raise ValueError("centres: %d channels, at most %d" % (centres.size, nat.limit("ils_channels")))
        self.centres = centres
        self.shape = shape
        self.table = None
        self.tableHalf = 0.0
        if shape == "table":
            if table is None:
                raise ValueError("table: shape \"table\" needs table=(offsets, values)")
            try:
                offsets, values = (np.array(v, dtype=np.float64) for v in table)
            except (TypeError, ValueError):
                raise ValueError("table: (offsets, values), two sequences of equal length")
            if offsets.ndim != 1 or offsets.shape != values.shape or offsets.size < 2:
                raise ValueError("table: (offsets, values), two 1-D sequences of equal length >= 2")
            if offsets.size > nat.limit("ils_table"):
                raise ValueError("table: %d values, at most %d" % (offsets.size, nat.limit("ils_table")))
            if not (np.all(np.isfinite(offsets)) and np.all(np.isfinite(values))):
                raise ValueError("table: offsets and values must be finite")
            half = float(offsets[-1])
            d = np.diff(offsets)
            tol = 1e-9 * max(half, 0.0)
            if not (half > 0 and np.all(d > 0) and np.all(np.abs(d - 2.0 * half / (offsets.size - 1)) <= tol)):
                raise ValueError("table: the offsets must be uniformly spaced and ascending")
            if abs(offsets[0] + half) > tol:
                raise ValueError("table: the offsets must be symmetric about 0")
            self.table = values
            self.tableHalf = half
            self.width = None
            default_cutoff = half
        else:
            if table is not None:
                raise ValueError("table: only shape \"table\" takes one")
            if width is None:
                raise ValueError("width: shape %r needs a width" % shape)
            self.width = self._per_channel("width", width)
            default_cutoff = {"gaussian": 3.0 * self.width, "triangle": self.width, "boxcar": self.width / 2.0}.get(shape)
        if cutoff is None:
            if default_cutoff is None:
                raise ValueError("cutoff: shape %r has no default cutoff, give one" % shape)
            cutoff = default_cutoff
        self.cutoff = self._per_channel("cutoff", cutoff)

    def _per_channel(self, name, value):
        try:
            v = np.array(value, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s: a number or one per channel, not %r" % (name, value))
        if v.ndim == 0:
            v = np.full(self.centres.shape, float(v))
        if v.shape != self.centres.shape:
            raise ValueError("%s: a number or one per channel (%d), got shape %s" % (name, self.centres.size, v.shape))
        if not np.all(np.isfinite(v) & (v > 0)):
            raise ValueError("%s must be finite and > 0" % name)
        return v

    def __len__(self):
        return self.centres.size

    def __repr__(self):
        return "Instrument(%d channels, %s)" % (self.centres.size, self.shape)

    def support(self, rangeMin, rangeMax, n):
        """(position, first, count) of every channel on linspace(rangeMin, rangeMax, n): position = (centre - rangeMin) /
        step in grid-index units, and [first, first + count) the grid points nu_j with |nu_j - centre| <= cutoff (on the
        axis _flux_bands searches).  ValueError, naming the channel, when [centre - cutoff, centre + cutoff] is not inside
        [rangeMin, rangeMax] or holds no grid point."""
        n = int(n)
        if n < 2 or not rangeMax > rangeMin:
            raise ValueError("the wavenumber range holds fewer than two grid points")
        step = (float(rangeMax) - float(rangeMin)) / (n - 1)
        lo, hi = self.centres - self.cutoff, self.centres + self.cutoff
        bad = np.flatnonzero(~((lo >= rangeMin) & (hi <= rangeMax)))
        if bad.size:
            i = int(bad[0])
            raise ValueError("channel %d (centre %.10g, cutoff %.10g) is not inside the range [%g, %g]"
                             % (i, self.centres[i], self.cutoff[i], rangeMin, rangeMax))
        x = np.linspace(rangeMin, rangeMax, n)
        inside = lambda j: np.abs(x[np.clip(j, 0, n - 1)] - self.centres) <= self.cutoff
        first = np.searchsorted(x, lo, "left").astype(np.int64)
        end = np.searchsorted(x, hi, "right").astype(np.int64)
        for _ in range(2):       # (the searched bounds are rounded sums: settle the end points on the criterion itself)
            first -= (first > 0) & inside(first - 1)
            first += (first < end) & ~inside(first)
            end += (end < n) & inside(end)
            end -= (end > first) & ~inside(end - 1)
        count = end - first
        bad = np.flatnonzero(count < 1)
        if bad.size:
            i = int(bad[0])
            raise ValueError("channel %d (centre %.10g, cutoff %.10g) holds no grid point" % (i, self.centres[i], self.cutoff[i]))
        return (self.centres - rangeMin) / step, first, count


def _ils_convolve(ctx, instrument, rangeMin, rangeMax, n, support, rows, out):
    """K8 over ``rows`` = [(Buffer, offset)] into ``out`` (len(rows) x channels), ``support`` from instrument.support."""
    position, first, count = support
    ctx.ils_convolve_dev(rangeMin, rangeMax, n, rows, position, instrument.width, first, count,
                         nat.ILS_SHAPES[instrument.shape], out, table=instrument.table, table_half=instrument.tableHalf)


def convolve(instrument, spectra, rangeMin, rangeMax):
    """Spectra on the base grid linspace(rangeMin, rangeMax, n) convolved onto the channels of ``instrument`` on the device:
    ``spectra`` of shape (n,) or (M, n) gives (C,) or (M, C).  Channel c of a row S is sum_j w_cj S_j / sum_j w_cj over the
    channel's support (Instrument.support) with w_cj = shape(((j - position_c) * step) / width_c); the same inputs give the
    same bits, a row's result does not depend on the rows beside it, and a constant row returns its constant."""
    if not isinstance(instrument, Instrument):
        raise ValueError("instrument: an Instrument, not %r" % (instrument,))
    spectra = np.ascontiguousarray(spectra, dtype=np.float64)
    if spectra.ndim not in (1, 2) or spectra.shape[-1] < 2:
        raise ValueError("spectra: shape (n,) or (M, n) on the base grid, got %s" % (spectra.shape,))
    rows2d = spectra.reshape(-1, spectra.shape[-1])
    M, n = rows2d.shape
    support = instrument.support(rangeMin, rangeMax, n)
    C = len(instrument)
    result = np.empty((M, C))
    if M == 0:
        return result
    ctx = _ctx()
    per_call = min(M, nat.limit("ils_rows"))
    tmp = []
    try:
        src = ctx.buffer(per_call * n); tmp.append(src)
        out = ctx.buffer(per_call * C); tmp.append(out)
        for r0 in range(0, M, per_call):
            m = min(per_call, M - r0)
            src.upload(rows2d[r0:r0 + m].reshape(-1))
            _ils_convolve(ctx, instrument, rangeMin, rangeMax, n, support, [(src, i * n) for i in range(m)], out)
            result[r0:r0 + m] = out.download(m * C).reshape(m, C)
    finally:
        for b in tmp:
            b.free()
    return result[0] if spectra.ndim == 1 else result


# ----------------------------------------------------------------------------------------
# k-distributions (kDistribution, Atmosphere.kDistribution; beyond the reference)
# ----------------------------------------------------------------------------------------
def gIntervals(g=16, count=None):
    """Rank edges e_0 = 0 < e_1 < ... < e_G = count of the g intervals of a band of ``count`` points, int64.
    - ``g`` an integer G in 1..256: the g edges are the cumulative Gauss-Legendre weights on [0, 1],
      numpy.r_[0, numpy.cumsum(leggauss(G)[1] / 2)] with the last one set to exactly 1;
    - ``g`` an explicit increasing sequence of g edges from 0 to 1 (at most 256 intervals).
    e_i = int(numpy.rint(g_i * count)).  ValueError for anything else, and when an interval comes out empty."""
    nmax = 256
    try:
        count = int(count)
    except (TypeError, ValueError):
        raise ValueError("count: the number of points of the band, not %r" % (count,))
    if count < 1:
        raise ValueError("count: the band holds no point")
    if isinstance(g, (int, np.integer)) and not isinstance(g, bool):
        if not 1 <= int(g) <= nmax:
            raise ValueError("g: %d intervals, 1..%d are possible" % (int(g), nmax))
        ge = np.r_[0.0, np.cumsum(np.polynomial.legendre.leggauss(int(g))[1] / 2.0)]
        ge[-1] = 1.0
    else:
        try:
            ge = np.array(g, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("g: an integer 1..%d or an increasing sequence of g edges from 0 to 1, not %r" % (nmax, g))
        if ge.ndim != 1 or not 2 <= ge.size <= nmax + 1:
            raise ValueError("g: 2..%d edges (1..%d intervals), got shape %s" % (nmax + 1, nmax, ge.shape))
        if not (np.all(np.isfinite(ge)) and ge[0] == 0.0 and ge[-1] == 1.0):
            raise ValueError("g: the edges must run from 0 to 1")
        if not np.all(np.diff(ge) > 0.0):
            raise ValueError("g: the edges must increase")
    edges = np.rint(ge * count).astype(np.int64)
    empty = np.flatnonzero(np.diff(edges) < 1)
    if empty.size:
        raise ValueError("g: interval %d of %d holds none of the band's %d points" % (int(empty[0]), edges.size - 1, count))
    return edges


class KDistribution:
    """What kDistribution and Atmosphere.kDistribution return.  Per band (a list with one entry per band, or the single
    band's arrays alone when ``bands`` was None): ``k`` (rows, G) mean of the row over every g interval; ``kLower`` (rows,
    G + 1) the row's value at every interval's first rank and, last, at the band's last rank; ``weight`` (G,) the intervals'
    share of the band's points; ``edges`` (G + 1,) their rank edges (gIntervals); ``planck`` (rows, G) the mean Planck
    function over the same points, or None.  With spectra=True also ``order`` (int64 grid indices) and ``sorted`` (the
    values in that order), (rows, count) each for reference=None and (count,) - the reference row's - otherwise; else None.
    ``reference``: the row whose order was used, or None."""

    def __init__(self, k, kLower, weight, edges, planck=None, order=None, sorted=None, reference=None):
        self.k = k
        self.kLower = kLower
        self.weight = weight
        self.edges = edges
        self.planck = planck
        self.order = order
        self.sorted = sorted
        self.reference = reference

    def __repr__(self):
        one = isinstance(self.k, np.ndarray)
        return "KDistribution(bands=%s, intervals=%s, reference=%r)" % (
            "None" if one else len(self.k), self.weight.size if one else [w.size for w in self.weight], self.reference)


class _KdistBuffers:
    """Device buffers of the k-distribution calls by name, each kept while it is large enough."""

    def __init__(self, owner=None):
        self.bufs = {}
        if owner is not None:
            import weakref
            weakref.finalize(owner, _free_buffers, self.bufs)

    def get(self, ctx, name, n):
        b = self.bufs.get(name)
        if b is not None and (b.h is None or b.ctx is not ctx or b.n < n):
            if b.h is not None and b.ctx.h:
                b.free()
            b = None
        if b is None:
            b = self.bufs[name] = ctx.buffer(max(int(n), 1))
        return b

    def free(self):
        _free_buffers(self.bufs)


def _kdist_checks(rangeMin, rangeMax, n, n_rows, bands, g, reference):
    """What both k-distribution calls check before the device is touched: (band_first, band_count, edges per band)."""
    if n_rows > nat.limit("kdist_rows"):
        raise ValueError("%d rows, at most %d" % (n_rows, nat.limit("kdist_rows")))
    if reference is not None:
        if isinstance(reference, bool) or not isinstance(reference, (int, np.integer)) or not 0 <= int(reference) < n_rows:
            raise ValueError("reference: None or the index of one of the %d rows, not %r" % (n_rows, reference))
    first, count = _flux_bands(rangeMin, rangeMax, n, bands)
    return first, count, [gIntervals(g, c) for c in count]


def _kdist_run(ctx, keep, n, rows, first, count, edges, reference, spectra, bands, planck=None):
    """K9 over ``rows`` = [(Buffer, offset)]: one ranking (of every row, or of the reference row), the means of all rows and,
    with ``planck`` = (rangeMin, rangeMax, [T of every row]), of every row's Planck function made into one kept buffer."""
    M, nb = len(rows), len(count)
    S, G = int(sum(count)), int(sum(e.size - 1 for e in edges))
    ranked = list(rows) if reference is None else [rows[int(reference)]]
    order = keep.get(ctx, "order", len(ranked) * S)
    srt = keep.get(ctx, "sorted", len(ranked) * S) if spectra else None
    need = ctx.rank_order_workspace(len(ranked), n, count)
    ctx.rank_order_dev(n, ranked, first, count, order, sorted=srt, work=keep.get(ctx, "rank_work", need) if need else None)
    orders = [(order, r * S if reference is None else 0) for r in range(M)]
    work = keep.get(ctx, "means_work", ctx.ranked_means_workspace(M, count, edges))
    mean = keep.get(ctx, "mean", (2 if planck else 1) * M * G)
    lower = keep.get(ctx, "lower", M * (G + nb))
    ctx.ranked_means_dev(n, rows, orders, first, count, edges, work, mean, lower=lower)
    if planck:
        lo, hi, temps = planck
        row = keep.get(ctx, "planck_row", n)
        for l, T in enumerate(temps):                     # in stream: the row is overwritten once its means are enqueued
            ctx.planck_dev(lo, hi, n, float(T), row)
            ctx.ranked_means_dev(n, [(row, 0)], [orders[l]], first, count, edges, work, mean, mean_offset=(M + l) * G)
    v = mean.download((2 if planck else 1) * M * G).reshape(-1, M, G)
    lw = lower.download(M * (G + nb)).reshape(M, G + nb)
    k, kl, pl, weight, od, sd = [], [], [], [], [], []
    if spectra:
        o = order.download(len(ranked) * S).reshape(len(ranked), S).astype(np.int64)
        sv = srt.download(len(ranked) * S).reshape(len(ranked), S)
    g0 = s0 = 0
    for b in range(nb):
        Gb = edges[b].size - 1
        k.append(v[0][:, g0:g0 + Gb].copy())
        kl.append(lw[:, g0 + b:g0 + b + Gb + 1].copy())
        if planck:
            pl.append(v[1][:, g0:g0 + Gb].copy())
        weight.append(np.diff(edges[b]) / float(count[b]))
        if spectra:
            sl = (slice(None) if reference is None else 0, slice(s0, s0 + count[b]))
            od.append(o[sl].copy())
            sd.append(sv[sl].copy())
        g0 += Gb
        s0 += count[b]
    pick = (lambda v: v[0]) if bands is None else (lambda v: v)
    return KDistribution(pick(k), pick(kl), pick(weight), pick([e.copy() for e in edges]), pick(pl) if planck else None,
                         pick(od) if spectra else None, pick(sd) if spectra else None,
                         None if reference is None else int(reference))


def kDistribution(rows, rangeMin, rangeMax, bands=None, g=16, reference=None, spectra=False):
    """k-distributions of host rows on the base grid linspace(rangeMin, rangeMax, n), ranked and averaged on the device:
    ``rows`` of shape (n,) or (M, n) - absorption coefficients, usually.  In every band (``bands`` as Atmosphere.fluxes takes
    them, at most 64; None: the whole range) a row's points are put in ascending order - exactly first +
    numpy.argsort(row[first:first + count], kind="stable"): -0.0 and 0.0 tie, NaN after +inf, ties in grid order - and the
    row is averaged over the intervals gIntervals(g, count) of that rank.  reference=None ranks every row by itself (the
    classical k-distribution); reference=r averages every row over the point sets of row r's order (one sort, M gathers),
    which keeps the spectral correlation between the rows.  Sums are taken in one fixed order: the same inputs give the same
    bits, and a row's result does not depend on the rows beside it.  Returns a KDistribution (for a 1-D input every
    per-row array holds one row); ``spectra``: also the order and the sorted values."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim not in (1, 2) or rows.shape[-1] < 2:
        raise ValueError("spectra: shape (n,) or (M, n) on the base grid, got %s" % (rows.shape,))
    rows2d = rows.reshape(-1, rows.shape[-1])
    M, n = rows2d.shape
    if M < 1:
        raise ValueError("spectra: no rows")
    first, count, edges = _kdist_checks(rangeMin, rangeMax, n, M, bands, g, reference)
    ctx = _ctx()
    keep = _KdistBuffers()
    try:
        src = keep.get(ctx, "rows", M * n).upload(rows2d.reshape(-1))
        return _kdist_run(ctx, keep, n, [(src, r * n) for r in range(M)], first, count, edges, reference, spectra, bands)
    finally:
        keep.free()


class Path:
    """One line of sight through a column, for Atmosphere.radiance: the segments the light crosses on its way to the
    observer, farthest first.  Segment i runs ``lengths[i]`` cm through layer ``layers[i]`` (index in the atmosphere, bottom
    layer 0); a layer may be missing or come more than once.  ``source``: what enters the first segment - "surface" (the
    surface source of the radiance() call) or "space" (nothing).  Immutable; len(path) is the number of segments, which
    may be 0 (the observer then sees the source).  ``bounce``: None, or an integer i in 0..len(path) - the light meets the
    surface after its first i segments and is reflected specularly there (Atmosphere.radiance with an emissivity;
    Atmosphere.reflectedPath builds the usual one).  ``temperatures``: None, or one pair (Ta, Tb) per segment, finite and
    > 0 - the temperature where the light enters the segment and where it leaves it, for radiance(planck="linear"); kept
    as a tuple of pairs.  ValueError for anything else.  Atmosphere.nadirPath, zenithPath and limbPath build the usual
    ones, with ``levelTemperatures`` also the temperatures."""
    __slots__ = ("layers", "lengths", "source", "name", "bounce", "temperatures")
    SOURCES = ("space", "surface")          # the C ABI's source_kind is the index
    SURFACE_MARKER = -1                     # ... and this segment layer (length 0) the place of a bounce

    def __init__(self, layers, lengths, source="surface", name="", bounce=None, temperatures=None):
        try:
            layers = list(layers)
            lay = tuple(int(l) for l in layers)
            ok = all(a == b for a, b in zip(lay, layers))
            lens = tuple(float(x) for x in lengths)
        except (TypeError, ValueError):
            raise ValueError("Path: layers are integers and lengths numbers, one per segment")
        if not ok or any(l < 0 for l in lay):
            raise ValueError("Path: layers are integers >= 0, not %r" % (list(layers),))
        if len(lay) != len(lens):
            raise ValueError("Path: %d layers but %d lengths" % (len(lay), len(lens)))
        if not all(x >= 0.0 and x != float("inf") for x in lens):
            raise ValueError("Path: lengths must be finite and >= 0")
        if source not in self.SOURCES:
            raise ValueError("Path: source is \"surface\" or \"space\", not %r" % (source,))
        if bounce is not None:
            if isinstance(bounce, bool) or not isinstance(bounce, (int, np.integer)) or not 0 <= bounce <= len(lay):
                raise ValueError("Path: bounce is None or an integer 0..%d (the segments before the surface), not %r"
                                 % (len(lay), bounce))
            bounce = int(bounce)
        if temperatures is not None:
            try:
                temperatures = tuple((float(a), float(b)) for a, b in temperatures)
            except (TypeError, ValueError):
                raise ValueError("Path: temperatures are pairs (Ta, Tb) of numbers, one per segment")
            if len(temperatures) != len(lay):
                raise ValueError("Path: %d layers but %d pairs of temperatures" % (len(lay), len(temperatures)))
            if not all(math.isfinite(t) and t > 0.0 for pair in temperatures for t in pair):
                raise ValueError("Path: temperatures must be finite and > 0")
        for k, v in zip(self.__slots__, (lay, lens, source, str(name), bounce, temperatures)):
            object.__setattr__(self, k, v)

    def __setattr__(self, key, value):
        raise AttributeError("a Path is immutable")

    __delattr__ = __setattr__

    def __len__(self):
        return len(self.layers)

    def __repr__(self):
        return "Path(%s%d segments, source=%s%s%s)" % (self.name + ": " if self.name else "", len(self), self.source,
                                                       "" if self.bounce is None else ", bounce=%d" % self.bounce,
                                                       "" if self.temperatures is None else ", temperatures")

    def _segments(self):
        """(layers, lengths) as the C call takes them: the bounce as a segment of SURFACE_MARKER and length 0"""
        if self.bounce is None:
            return self.layers, self.lengths
        i = self.bounce
        return self.layers[:i] + (self.SURFACE_MARKER,) + self.layers[i:], self.lengths[:i] + (0.0,) + self.lengths[i:]

    def _segment_temperatures(self):
        """the temperatures beside _segments(): a dummy pair at the bounce, which the C call ignores"""
        if self.bounce is None:
            return self.temperatures
        i = self.bounce
        return self.temperatures[:i] + ((0.0, 0.0),) + self.temperatures[i:]


class PathRadiance:
    """What Atmosphere.radiance returns.  ``paths``: the paths, in order.  Without an instrument ``wavenumber`` is the grid
    (n,) and ``radiance`` (R, n) the spectrum arriving along every path, in the units of transmission(); with one they are
    the channel centres (C,) and the channel radiances (R, C).  ``transmittance``: the path transmittances in the same
    shape when asked for, else None."""

    def __init__(self, wavenumber, radiance, transmittance, paths):
        self.wavenumber = wavenumber
        self.radiance = radiance
        self.transmittance = transmittance
        self.paths = paths

    def __repr__(self):
        return "PathRadiance(paths=%d, points=%d, transmittance=%s)" % (
            len(self.paths), self.wavenumber.size, self.transmittance is not None)


class ScatterRadiance:
    """What Atmosphere.radianceTwoStream returns, for V views.  Without an instrument ``wavenumber`` is the grid (n,) and
    ``radiance`` (V, n) the spectrum along every view, in the units of transmission(); with one they are the channel centres
    (C,) and the channel radiances (V, C).  ``mu``: (V,) the viewing cosines; ``direction``: V times "up" (leaving the top of
    the column) or "down" (arriving at the surface).  brightnessTemperature(wavenumber, radiance) applies."""

    def __init__(self, wavenumber, radiance, mu, direction):
        self.wavenumber = wavenumber
        self.radiance = radiance
        self.mu = mu
        self.direction = direction

    def __repr__(self):
        return "ScatterRadiance(views=%d, points=%d)" % (len(self.mu), self.wavenumber.size)


def _scatter_views(views):
    """``views`` of radianceTwoStream as (mu (V,), down (V,) of 0 / 1, the directions' names)"""
    if isinstance(views, (str, bytes)) or not hasattr(views, "__len__") or len(views) == 0:
        raise ValueError("views: a sequence of mu or (mu, \"up\" | \"down\"), at least one, not %r" % (views,))
    mu, down = [], []
    for v in views:
        direction = "up"
        if isinstance(v, (tuple, list)):
            if len(v) != 2:
                raise ValueError("views: (mu, \"up\" | \"down\"), not %r" % (v,))
            v, direction = v
        if direction not in ("up", "down"):
            raise ValueError("views: the direction is \"up\" or \"down\", not %r" % (direction,))
        try:
            m = float(v)
        except (TypeError, ValueError):
            raise ValueError("views: mu must be a number in (0, 1], not %r" % (v,))
        if not (m > 0 and m <= 1):
            raise ValueError("views: mu must lie in (0, 1], not %r" % (v,))
        mu.append(m)
        down.append(1 if direction == "down" else 0)
    return np.array(mu), down, ["down" if d else "up" for d in down]


_NO_VIEWS = object()         # _thermal_scatter_checks: the call has no views (None is a caller's mistake, and reported)


class PathJacobians:
    """What Atmosphere.pathJacobians returns, for R paths through L layers.  X is the grid (n points) or, with an instrument,
    its channels (C).  ``wavenumber``: (X,) the grid or the channel centres; ``radiance``: (R, X), Atmosphere.radiance's;
    ``opticalDepth``: (R, L, X) dI/d ln tau_l; ``temperature``: (R, L, X) dI/dT_l, Planck part; ``surfaceTemperature``: (R, X)
    dI/dT_s, 0 for paths from space, None when a surface spectrum was given; ``molecules``: one (R, M_l, X) array per layer,
    aligned with list(layer), dI/d ln n of every molecule at fixed line shapes (None when not asked for); ``moleculeNames``:
    their names; ``temperatureAbsorption``: (R, L, X) the absorption part of dI/dT_l through dk_l/dT and ``temperatureFull``
    = temperature + temperatureAbsorption, both None unless temperature="full" was asked for; ``paths``: the paths, in
    order.  Layers a path does not cross hold exact zeros.  With an instrument also ``brightnessTemperature`` (R, C), the
    inverse Planck of the channel radiance at the centre, and ``brightnessTemperatureJacobian`` (R, L, C) = temperature /
    (dB/dT at the centre and the channel's brightness temperature), as Observation forms it; else both None.
    ``emissivity``: (R, X) dI/de per unit emissivity over a surface with an emissivity, None over the black surface.
    From Atmosphere.pathJacobiansLinear only (else None): ``segmentTemperature``: per path an (s, 2, X) array, dI/dTa and
    dI/dTb of each of its s segments in order of travel; ``temperature``, temperatureFull and
    brightnessTemperatureJacobian are then None."""

    def __init__(self, wavenumber, radiance, temperature, opticalDepth, surfaceTemperature, molecules, moleculeNames, paths,
                 temperatureAbsorption=None, channels=False, emissivity=None, segmentTemperature=None):
        self.wavenumber = wavenumber
        self.radiance = radiance
        self.temperature = temperature
        self.opticalDepth = opticalDepth
        self.surfaceTemperature = surfaceTemperature
        self.molecules = molecules
        self.moleculeNames = moleculeNames
        self.temperatureAbsorption = temperatureAbsorption
        self.temperatureFull = (None if temperatureAbsorption is None or temperature is None
                                else temperature + temperatureAbsorption)
        self.paths = paths
        self.emissivity = emissivity
        self.segmentTemperature = segmentTemperature
        self.brightnessTemperature = self.brightnessTemperatureJacobian = None
        if channels:
            self.brightnessTemperature = brightnessTemperature(wavenumber, radiance)
            if temperature is not None:
                with np.errstate(divide='ignore', invalid='ignore'):
                    self.brightnessTemperatureJacobian = temperature / _planck_dT(wavenumber, self.brightnessTemperature)[:, None, :]

    def __repr__(self):
        return "PathJacobians(paths=%d, layers=%d, points=%d, molecules=%s, full=%s)" % (
            len(self.paths), self.opticalDepth.shape[1], self.wavenumber.size, self.molecules is not None,
            self.temperatureAbsorption is not None)


class Observation:
    """What Atmosphere.observe returns.  ``wavenumber``: the channel centres, (C,); ``radiance``: channel radiance in the
    units of transmission(); ``brightnessTemperature``: its inverse Planck at the centre, K; ``mu``: the viewing cosine.
    With jacobians=True (else None), (L, C) each: ``temperatureJacobian`` dR_c/dT_l (Planck part only, as jacobians()
    documents), ``opticalDepthJacobian`` dR_c/d ln tau_l and ``brightnessTemperatureJacobian`` = temperatureJacobian /
    (dB/dT at the centre and the channel's brightness temperature); over a surface with an emissivity also
    ``emissivityJacobian`` (C,) dR_c/de, else None.  From Atmosphere.observeLinear with jacobians=True (else None):
    ``levelTemperatureJacobian`` (L + 1, C) dR_c/d(level temperature); temperatureJacobian is then None."""

    def __init__(self, wavenumber, radiance, mu, temperatureJacobian=None, opticalDepthJacobian=None,
                 emissivityJacobian=None, levelTemperatureJacobian=None):
        self.wavenumber = wavenumber
        self.radiance = radiance
        self.brightnessTemperature = brightnessTemperature(wavenumber, radiance)
        self.mu = mu
        self.temperatureJacobian = temperatureJacobian
        self.opticalDepthJacobian = opticalDepthJacobian
        self.emissivityJacobian = emissivityJacobian
        self.levelTemperatureJacobian = levelTemperatureJacobian
        self.brightnessTemperatureJacobian = None
        if temperatureJacobian is not None:
            with np.errstate(divide='ignore', invalid='ignore'):
                self.brightnessTemperatureJacobian = temperatureJacobian / _planck_dT(wavenumber, self.brightnessTemperature)

    def __repr__(self):
        return "Observation(channels=%d, mu=%g, jacobians=%s)" % (
            self.wavenumber.size, self.mu, self.opticalDepthJacobian is not None)


# ----------------------------------------------------------------------------------------
# Atmosphere (cls:790-821) + the column fold this build defines on it
# ----------------------------------------------------------------------------------------
class Atmosphere(list):
    def __init__(self, name):
        super().__init__()
        self.name = name

    def __str__(self):
        return self.name

    def __bool__(self):
        return True

    def addLayer(self, depth, T, P, rangeMin, rangeMax, name=None, dynamicResolution=True):
        if not name:
            name = self.nextLayerName()
        newLayer = Layer(depth, T, P, rangeMin, rangeMax, atmosphere=self, name=name,
                         dynamicResolution=dynamicResolution)
        self.append(newLayer)
        return newLayer

    def nextLayerName(self):
        return 'Layer %s' % (len(self) + 1)

    def returnLayerNames(self):
        return [layer.name for layer in self]

    def returnLayerObjects(self):
        return list(self)

    def _column_layers(self):
        """The layers, bottom to top, and the number of grid points of the one range they share."""
        layers = list(self)
        if not layers:
            raise ValueError("atmosphere has no layers")
        first = layers[0]
        for L in layers[1:]:
            if (L.rangeMin, L.rangeMax) != (first.rangeMin, first.rangeMax):
                raise ValueError("all layers of a column must share one wavenumber range")
        return layers, int((first.rangeMax - first.rangeMin) / utils.BASE_RESOLUTION)

    def _column_checks(self, surfaceSpectrum, surfaceTemperature, angles, bands):
        """The checks fluxes() and jacobians() share, before the device is touched: (layers, n, mu, weight, band_first,
        band_count, surfaceSpectrum as n float64 values or None)."""
        layers, n = self._column_layers()
        if surfaceSpectrum is None and surfaceTemperature is None:
            raise ValueError("give surfaceSpectrum or surfaceTemperature")
        if surfaceSpectrum is None and not float(surfaceTemperature) > 0:
            raise ValueError("surfaceTemperature must be > 0")
        mu, weight = fluxAngles(angles)
        band_first, band_count = _flux_bands(layers[0].rangeMin, layers[0].rangeMax, n, bands)
        return layers, n, mu, weight, band_first, band_count, _grid_spectrum("surfaceSpectrum", surfaceSpectrum, n)

    def _column_abs_coef(self, ctx, layers, n):
        """Every layer's resident absorption coefficient buffer and the plan of _resident_abs_coef, which makes them in the
        merged layer step of the default arithmetic; otherwise every layer's own sweep does, and the plan is None."""
        if _merged_route(ctx):
            plan = self._resident_abs_coef(ctx, layers, n)
            return [p[1].bufs["abs_coef"] for p in plan], plan
        return [L._ensure_swept()[0].bufs["abs_coef"] for L in layers], None

    # The four call helpers below hold the one rule that picks a transport entry point: ``edges`` (or ``linear``: the paths'
    # segment temperatures) given - the linear one, with emissivity None passed as 1.0; otherwise emissivity None - the black
    # one; otherwise the surface one.  ``emissivity`` is None, a float or a Buffer.  A new source or surface variant goes here.

    @staticmethod
    def _flux_call(ctx, layers, n, kbufs, edges, emissivity, reflection, mu, weight, band_first, band_count, level,
                   up_surface=None, **kw):
        """lbl_column_flux_dev, _surface_dev or _linear_dev; ``kw``: I_surface, surface_T, I_top, up_top, down_surface"""
        first = layers[0]
        args = ([L.depth for L in layers], first.rangeMin, first.rangeMax, n, mu, weight, band_first, band_count, level)
        if edges is not None:
            ctx.column_flux_linear_dev(kbufs, edges, *args, 1.0 if emissivity is None else emissivity, reflection=reflection,
                                       up_surface=up_surface, **kw)
        elif emissivity is None:
            ctx.column_flux_dev(kbufs, [L.T for L in layers], *args, **kw)
        else:
            ctx.column_flux_surface_dev(kbufs, [L.T for L in layers], *args, emissivity, reflection=reflection,
                                        up_surface=up_surface, **kw)

    @staticmethod
    def _jacobian_call(ctx, layers, n, kbufs, edges, emissivity, reflection, mu, weight, band_first, band_count, jac,
                       T_spectra=None, I_top=None, e_spectrum=None, **kw):
        """lbl_column_jacobian_dev, _surface_dev or _linear_dev (``T_spectra`` is then the edges'); ``kw``: I_surface,
        surface_T, term_abs_coef, term_layer, ln_tau_spectra"""
        first = layers[0]
        args = ([L.depth for L in layers], first.rangeMin, first.rangeMax, n, mu, weight, band_first, band_count, jac)
        if edges is not None:
            ctx.column_jacobian_linear_dev(kbufs, edges, *args, 1.0 if emissivity is None else emissivity,
                                           reflection=reflection, I_top=I_top, T_edge_spectra=T_spectra, e_spectrum=e_spectrum,
                                           **kw)
        elif emissivity is None:
            ctx.column_jacobian_dev(kbufs, [L.T for L in layers], *args, T_spectra=T_spectra, **kw)
        else:
            ctx.column_jacobian_surface_dev(kbufs, [L.T for L in layers], *args, emissivity, reflection=reflection, I_top=I_top,
                                            T_spectra=T_spectra, e_spectrum=e_spectrum, **kw)

    @staticmethod
    def _flat_paths(layers, n, paths, linear, emissivity):
        """What the ray entry points take between the absorption coefficients and their output: the temperatures, the range
        and the paths flattened into ray_first, seg_layer, seg_length and source_kind.  The black entry point knows no
        bounce marker and gets the paths' own segments, the other two Path._segments()."""
        first = layers[0]
        segs = [(p.layers, p.lengths) if emissivity is None and not linear else p._segments() for p in paths]
        return ([t for p in paths for t in p._segment_temperatures()] if linear else [L.T for L in layers],
                first.rangeMin, first.rangeMax, n, np.cumsum([0] + [len(lay) for lay, _ in segs]),
                [l for lay, _ in segs for l in lay], [x for _, lens in segs for x in lens],
                [Path.SOURCES.index(p.source) for p in paths])

    @staticmethod
    def _ray_radiance_call(ctx, layers, n, kbufs, paths, linear, emissivity, radiance, surface_down=None,
                           surface_down_norm=0.0, **kw):
        """lbl_ray_radiance_dev, _surface_dev or _linear_dev; ``kw``: I_source, source_T, transmittance"""
        args = Atmosphere._flat_paths(layers, n, paths, linear, emissivity)
        if linear:
            ctx.ray_radiance_linear_dev(kbufs, *args, radiance, 1.0 if emissivity is None else emissivity,
                                        surface_down=surface_down, surface_down_norm=surface_down_norm, **kw)
        elif emissivity is None:
            ctx.ray_radiance_dev(kbufs, *args, radiance, **kw)
        else:
            ctx.ray_radiance_surface_dev(kbufs, *args, radiance, emissivity, surface_down=surface_down,
                                         surface_down_norm=surface_down_norm, **kw)

    @staticmethod
    def _ray_jacobian_call(ctx, layers, n, kbufs, paths, linear, emissivity, jac, **kw):
        """lbl_ray_jacobian_dev, _surface_dev or _linear_dev; ``kw``: I_source, source_T, term_abs_coef, term_layer, radiance"""
        args = Atmosphere._flat_paths(layers, n, paths, linear, emissivity)
        if linear:
            ctx.ray_jacobian_linear_dev(kbufs, *args, jac, 1.0 if emissivity is None else emissivity, **kw)
        elif emissivity is None:
            ctx.ray_jacobian_dev(kbufs, *args, jac, **kw)
        else:
            ctx.ray_jacobian_surface_dev(kbufs, *args, jac, emissivity, **kw)

    @staticmethod
    def _device_emissivity(ctx, state, emissivity):
        """None or a number as it is, n values as ``state``'s "emissivity" buffer"""
        if emissivity is None or isinstance(emissivity, float):
            return emissivity
        return state.buf(ctx, "emissivity").upload(emissivity)

    @staticmethod
    def _term_count(layers, molecules, full, name_dT):
        """The number of terms of a Jacobian call - the molecules' and, with ``full``, dk_l/dT per layer - checked against
        the limit (``name_dT``: the wording that names dk/dT) and, with ``full``, against what dk/dT needs"""
        n_terms = (sum(len(L) for L in layers) if molecules else 0) + (len(layers) if full else 0)
        if n_terms > nat.limit("jacobian_terms"):
            raise ValueError(("molecules: %d molecule and dk/dT terms, at most %d (molecules=False skips the molecule terms)"
                              if name_dT else "molecules: %d molecule terms, at most %d (molecules=False skips them)")
                             % (n_terms, nat.limit("jacobian_terms")))
        if full:
            for L in layers:
                L._check_abs_coef_dT()
        return n_terms

    def _term_buffers(self, ctx, layers, n, plan, molecules, full):
        """(the terms' buffers, the layer of each, the number of molecule terms): _jacobian_terms' with ``molecules``, then
        with ``full`` dk_l/dT as one more term of layer l - the term sums are linear in the term, whatever its sign"""
        bufs, where = self._jacobian_terms(ctx, layers, n, plan) if molecules else ([], [])
        n_mol_terms = len(bufs)
        if full:
            bufs = bufs + [L._abs_coef_dT()[0] for L in layers]
            where = where + list(range(len(layers)))
        return bufs, where, n_mol_terms

    def _jacobian_spectra(self, ctx, linear, nl, n):
        """The kept buffers of the spectral (dF/d ln tau, dF/dT) rows, L x n and L x n or, ``linear``, 2 L x n edge rows"""
        # behaviour, kept: each source keeps its own state, sized for its own rows (the buffers stand between calls)
        sp = _kept_state(self, "_jacobian_linear_spec" if linear else "_jacobian_spec").reserve(ctx, (2 if linear else 1) * nl * n)
        return sp.buf(ctx, "ln_tau"), sp.buf(ctx, "T_edge" if linear else "T")

    def transmission(self, surfaceSpectrum=None, surfaceTemperature=None):
        """Fold Layer.transmission bottom to top over the layers in list order:
        I <- T_i I + (1 - T_i) B(nu, T_i), I_0 = surfaceSpectrum or B(nu, surfaceTemperature).
        (The reference announces an atmosphere path but ships no driver; this is the fold of
        cls:784-787, computed by one column-sweep kernel.)
        The Planck source is the layer source: one temperature per layer (fluxes() and radiance() also take
        planck="linear"; its derivatives are not part of this method)."""
        layers, n = self._column_layers()
        first = layers[0]
        ctx = _ctx()
        if surfaceSpectrum is None and surfaceTemperature is None:
            raise ValueError("give surfaceSpectrum or surfaceTemperature")
        merged = self._transmission_merged(ctx, layers, n, surfaceSpectrum, surfaceTemperature)
        if merged is not None:
            return merged
        _compute_cross_sections([iso for L in layers for m in L for iso in m])
        for L in layers:
            L._members_ready()
        # one pass over every layer's device-resident cross sections (lbl_column_step_dev)
        desc = []
        for L in layers:
            xs, iso_mol = [], []
            for k, m in enumerate(L):
                for iso in m._members():
                    xs.append(iso._device_xsec_current(ctx, n))
                    iso_mol.append(k)
            desc.append(dict(xsec=xs, iso_mol=iso_mol, conc=[m.concentration for m in L], P=L.P, T=L.T, depth=L.depth))
        tmp = []
        try:
            out = ctx.buffer(max(n, 1)); tmp.append(out)
            I_in = None
            if surfaceSpectrum is not None:
                I_in = ctx.buffer(max(n, 1)).upload(np.ascontiguousarray(surfaceSpectrum, dtype=np.float64))
                tmp.append(I_in)
            ctx.column_step_dev(desc, first.rangeMin, first.rangeMax, n, out, I_in=I_in,
                                surface_T=float(surfaceTemperature or 0.0))
            return out.download(n, pinned=True)
        finally:
            for b in tmp:
                b.free()


    def fluxes(self, surfaceTemperature=None, surfaceSpectrum=None, topSpectrum=None, angles=3, bands=None, spectra=False,
               emissivity=None, reflection="lambertian", planck="layer", levelTemperatures=None):
        """Upward, downward and net fluxes at every level and the heating rate of every layer (beyond the reference).

        Layers l = 0 .. L-1 in list order, bottom to top, as transmission() takes them; level i is the lower boundary of
        layer i (level 0 the surface, level L the top).  All layers share one range and grid.  At every grid point nu_j
        (xAxis) and for every angle k (cosine mu_k in (0, 1], weight W_k; ``angles``: see fluxAngles, default 3 Gauss
        angles):
            t_lk = exp(-k_l(nu_j) depth_l / mu_k)      k_l = the layer's absorption coefficient (getAbsCoef)
            B_l  = planckWavenumber(nu_j, T_l)
            up:   I_0k = surfaceSpectrum[j] or B(nu_j, surfaceTemperature)    I_(l+1)k = t_lk I_lk + (1 - t_lk) B_l
            down: I_Lk = topSpectrum[j] or 0                                  I_lk     = t_lk I_(l+1)k + (1 - t_lk) B_l
            spectral flux F_i(nu_j) = sum_k W_k I_ik(nu_j)   (each direction)
            band flux     F_i = res * sum over the band's points of nan_to_num(F_i(nu_j)),  res = settings.BASE_RESOLUTION
            net           F_i = F_up_i - F_down_i;   heating rate: heatingRates(net, P, T, depth), K/day
        The surface is black (emissivity 1); both boundary sources are isotropic radiances in the units of transmission()'s
        surfaceSpectrum.  ``bands``: None (the whole range) or a list of (lo, hi) in cm^-1, band = the points lo <= nu_j < hi
        (at most 64).  ``spectra``: also return F_up at the top and F_down at the surface per grid point.
        With angles=[(1.0, pi)] the upward spectral flux at the top is pi * transmission(...) bit for bit wherever the fold
        takes its one-exp-per-thread Planck path (every range and temperature away from nu -> 0).
        The absorption coefficients come from the machinery transmission() uses and stay resident: after transmission()
        nothing is accumulated again.  Everything is validated (ValueError) before the device is touched.

        ``emissivity``: None, the black surface above, or the surface's emissivity e - a number in [0, 1], n values on xAxis,
        or a pair (wavenumbers, values) interpolated onto xAxis with np.interp (the end values held).  The surface then
        emits e Is (Is the surface source above) and reflects what comes down: the downward walk runs first, and with D_k the
        downward radiance of angle k at level 0 and F0 = sum_k W_k D_k,
            I_0k = e Is + (1 - e) R_k      R_k = F0 / sum_k W_k ("lambertian": diffuse)  or  D_k ("specular": a mirror)
        Dividing by the sum of the weights (pi for the Gauss angles) makes the reflected upward flux (1 - e) F0 under the
        quadrature itself, so the surface conserves energy whatever the angle set.  With ``spectra`` the result also carries
        upSurfaceSpectrum, F_up at level 0.  One pass over the absorption coefficients (lbl_column_flux_surface_dev), nothing
        comes down in between; with emissivity 1 every result is the black surface's bit for bit.

        ``planck``: "layer", the isothermal layers above, or "linear" - the Planck function runs linearly in optical depth
        through a layer, between the temperatures of its two levels (``levelTemperatures``: L + 1 numbers, level 0 the
        surface; None: levelTemperatures()).  With tau = k_l depth_l / mu_k, Ba the Planck function at the level where the
        light enters the layer (the lower one going up, the upper one going down) and Bb where it leaves,
            I <- t I + (1 - t) Ba + g(tau) (Bb - Ba)        g(tau) = 1 - (1 - t) / tau
        which removes the isothermal layer's first-order error on a column with a lapse rate.  The surface source stays
        surfaceTemperature or surfaceSpectrum (a skin temperature may differ from level 0), emissivity, reflection, bands
        and spectra work as above (lbl_column_flux_linear_dev), and the heating rates are heatingRates() with the layers'
        own T, P and depth.  With level temperatures equal to the layers' on both sides of every layer, every result is the
        layer source's bit for bit."""
        layers, n, mu, weight, band_first, band_count, surfaceSpectrum = self._column_checks(
            surfaceSpectrum, surfaceTemperature, angles, bands)
        topSpectrum = _grid_spectrum("topSpectrum", topSpectrum, n)
        first = layers[0]
        refl = _surface_reflection(reflection)
        edges = None
        if _planck_source(planck, levelTemperatures):
            lev = self._level_temperatures(levelTemperatures)
            edges = np.column_stack([lev[:-1], lev[1:]])
        if emissivity is not None:
            emissivity = _surface_emissivity(emissivity, first.xAxis)
            wsum = _weight_sum(weight)
        res = utils.BASE_RESOLUTION
        nl, nb = len(layers), len(band_first)
        ctx = _ctx()
        kbufs, _ = self._column_abs_coef(ctx, layers, n)
        fst = _kept_state(self, "_flux_state")
        fst.reserve(ctx, max(n, nb * 2 * (nl + 1)))
        I_surface = fst.buf(ctx, "I_surface").upload(surfaceSpectrum) if surfaceSpectrum is not None else None
        I_top = fst.buf(ctx, "I_top").upload(topSpectrum) if topSpectrum is not None else None
        level = fst.buf(ctx, "level")
        up_top = fst.buf(ctx, "up_top") if spectra else None
        down_surface = fst.buf(ctx, "down_surface") if spectra else None
        emissivity = self._device_emissivity(ctx, fst, emissivity)
        up_surface = fst.buf(ctx, "up_surface") if spectra and emissivity is not None else None
        self._flux_call(ctx, layers, n, kbufs, edges, emissivity, refl, mu, weight, band_first, band_count, level,
                        up_surface=up_surface, I_surface=I_surface, surface_T=float(surfaceTemperature or 0.0), I_top=I_top,
                        up_top=up_top, down_surface=down_surface)
        sums = level.download(nb * 2 * (nl + 1)).reshape(nb, 2, nl + 1) * res
        up, down = sums[:, 0, :], sums[:, 1, :]
        heat = heatingRates(up - down, [L.P for L in layers], [L.T for L in layers], [L.depth for L in layers])
        up, down, heat = _band_values(bands, [up, down, heat])
        return Fluxes(up, down, heat, mu, weight,
                      upSpectrum=up_top.download(n) if spectra else None,
                      downSpectrum=down_surface.download(n) if spectra else None,
                      upSurfaceSpectrum=up_surface.download(n) if up_surface is not None else None)

    def solarFluxes(self, solarSpectrum=None, solarTemperature=None, distanceAU=1.0, mu0=1.0, geometry="plane",
                    planetRadius=6.371e8, emissivity=1.0, reflection="lambertian", angles=3, bands=None, spectra=False):
        """The direct solar beam through the column and its heating: gas absorption of sunlight, without scattering and
        without thermal emission (beyond the reference).

        SUPERPOSITION: without scattering the transfer is linear, so the fluxes of a sunlit column are
        fluxes(...) (thermal, reflected thermal included) plus solarFluxes(...) (solar, reflected solar included), level by
        level; likewise the net fluxes and the heating rates.

        Layers, levels, grid, bands and band sums as in fluxes().  ``solarSpectrum``: the beam's irradiance S0 at the top on
        a plane normal to it, W m^-2 per cm^-1, finite and >= 0 - a number, n values on xAxis or a pair (wavenumbers,
        values) interpolated onto xAxis with np.interp (the end values held); or ``solarTemperature``: a black-body sun,
        solarIrradiance(xAxis, solarTemperature, distanceAU).  Exactly one of the two.
        ``mu0``: the cosine of the solar zenith angle in (0, 1], or a list of up to 8 (mu0, weight) pairs - several suns,
        for example a day's mean; a plain number means weight 1.  ``geometry``: "plane" or "spherical" with
        ``planetRadius`` in cm, see solarSlants for the path of a beam through a layer; the projection onto the horizontal
        stays mu0 at every level in both.  At every grid point nu_j, for every beam s:
            tau_l = k_l(nu_j) depth_l                      k_l = the layer's absorption coefficient (getAbsCoef)
            down: S_sL = S0[j]                             S_sl = exp(-tau_l slant_sl) S_s(l+1)
                  F_down_i = sum_s weight_s mu0_s S_si
        The surface (``emissivity`` e as fluxes() takes it - here 1 - e is its albedo - and ``reflection``) emits nothing:
            "lambertian": I_0k = (1 - e) F_down_0 / sum_k W_k    I_(l+1)k = exp(-tau_l / mu_k) I_lk    F_up_i = sum_k W_k I_ik
                          over the diffuse angles (mu_k, W_k) of ``angles`` (see fluxAngles)
            "specular":   U_s0 = (1 - e) S_s0                    U_s(l+1) = exp(-tau_l slant_sl) U_sl
                          F_up_i = sum_s weight_s mu0_s U_si       (the mirrored beam leaves along its own slant path)
        Band fluxes, net = up - down and heatingRates(net, P, T, depth) as in fluxes(); ``spectra``: also F_up at the top,
        F_down at the surface and F_up at the surface per grid point.  Returns a SolarFluxes.
        The absorption coefficients come from the machinery transmission() and fluxes() use and stay resident: after either
        nothing is accumulated again (lbl_column_solar_dev walks them).  A source made from numbers alone (solarTemperature,
        or one value) stays on the device while those numbers and the grid stay the same.  Everything is validated
        (ValueError) before the device is touched."""
        layers, n = self._column_layers()
        first = layers[0]
        x = first.xAxis
        # (a source made from numbers alone stays on the device from call to call: neither formed nor uploaded again)
        key = _solar_source_key(solarSpectrum, solarTemperature, distanceAU)
        if key is not None:
            _solar_spectrum(solarSpectrum, solarTemperature, distanceAU, x[:1])
            key += (first.rangeMin, first.rangeMax, n)
        kept = self.__dict__.get("_solar_state")
        S0 = None
        if key is None or kept is None or kept.key != key:
            S0 = _solar_spectrum(solarSpectrum, solarTemperature, distanceAU, x)
        mu_s, weight_s = _solar_beams(mu0)
        depth = [L.depth for L in layers]
        slant = solarSlants(depth, list(zip(mu_s, weight_s)), geometry, planetRadius)
        beam_weight = weight_s * mu_s
        emissivity = _surface_emissivity(emissivity, x)
        refl = _surface_reflection(reflection)
        mu, weight = fluxAngles(angles)
        if refl == 0:
            _weight_sum(weight)
        band_first, band_count = _flux_bands(first.rangeMin, first.rangeMax, n, bands)
        res = utils.BASE_RESOLUTION
        nl, nb = len(layers), len(band_first)
        ctx = _ctx()
        kbufs, _ = self._column_abs_coef(ctx, layers, n)
        sst = _kept_state(self, "_solar_state")
        sst.reserve(ctx, max(n, nb * 2 * (nl + 1)))
        if S0 is None and sst.key != key:                   # (the buffers were given up in between)
            S0 = _solar_spectrum(solarSpectrum, solarTemperature, distanceAU, x)
        source = sst.buf(ctx, "S0")
        if S0 is not None:
            sst.key = None
            source.upload(S0)
            sst.key = key
        level = sst.buf(ctx, "level")
        up_top = sst.buf(ctx, "up_top") if spectra else None
        down_surface = sst.buf(ctx, "down_surface") if spectra else None
        up_surface = sst.buf(ctx, "up_surface") if spectra else None
        if not isinstance(emissivity, float):
            emissivity = sst.buf(ctx, "emissivity").upload(emissivity)
        ctx.column_solar_dev(kbufs, depth, first.rangeMin, first.rangeMax, n, source, beam_weight, slant,
                             mu if refl == 0 else (), weight if refl == 0 else (), band_first, band_count, level,
                             emissivity=emissivity, reflection=refl, up_top=up_top, down_surface=down_surface,
                             up_surface=up_surface)
        sums = level.download(nb * 2 * (nl + 1)).reshape(nb, 2, nl + 1) * res
        up, down = sums[:, 0, :], sums[:, 1, :]
        heat = heatingRates(up - down, [L.P for L in layers], [L.T for L in layers], depth)
        up, down, heat = _band_values(bands, [up, down, heat])
        return SolarFluxes(up, down, heat, mu_s, beam_weight, slant, mu, weight,
                           upSpectrum=up_top.download(n) if spectra else None,
                           downSpectrum=down_surface.download(n) if spectra else None,
                           upSurfaceSpectrum=up_surface.download(n) if spectra else None)

    # What the three two-stream methods below share.  A new member of the family names these instead of copying a sibling.
    @staticmethod
    def _scatter_checks(scatterers, deltaScaling, x, n_layers):
        """(the Scatterers, each one's (extinction, albedo, asymmetry) on the grid x) behind the checks of ``scatterers``
        and ``deltaScaling``"""
        scat = _scatterers(scatterers, n_layers)
        numbers = [sc._on_grid(x) for sc in scat]
        if not isinstance(deltaScaling, (bool, np.bool_)):
            raise ValueError("deltaScaling: True or False, not %r" % (deltaScaling,))
        return scat, numbers

    @staticmethod
    def _scatter_columns(ctx, st, scat, numbers):
        """scat_amount, scat_ext, scat_ssa, scat_asym of the column_*_dev call: a number stays one, n values go into the
        kept state ``st``"""
        columns = []
        for c, triple in enumerate(numbers):
            columns.append([v if isinstance(v, float) else st.buf(ctx, "scat%d_%d" % (c, q)).upload(v)
                            for q, v in enumerate(triple)])
        return [sc.amounts for sc in scat], [t[0] for t in columns], [t[1] for t in columns], [t[2] for t in columns]

    def _scatter_workspace(self, ctx, sizing, key, n_layers, points):
        """The workspace buffer kept under ``key``: ``points`` points in one pass where 256 MiB hold them, else as many whole
        tiles as they hold (``sizing``: the entry point's column_*_workspace)"""
        tile = sizing(n_layers, 1)
        want = sizing(n_layers, points)
        wst = _kept_state(self, key)
        wst.reserve(ctx, min(want, max(TWOSTREAM_WORKSPACE_BYTES // 8 // tile, 1) * tile))
        return wst.buf(ctx, "workspace")

    def _thermal_scatter_checks(self, surfaceTemperature, surfaceSpectrum, topSpectrum, bands, scatterers, deltaScaling,
                                emissivity, planck, levelTemperatures, views=_NO_VIEWS):
        """What fluxesTwoStream() and radianceTwoStream() check and form before the device is touched, as a namespace:
        layers, n, mu, weight, band_first, band_count, surfaceSpectrum, topSpectrum, views (_scatter_views' triple, with
        ``views``), scat, numbers, linear, T (the layers' temperatures, or with ``linear`` their edge pairs), emissivity,
        depth, surface_T"""
        c = types.SimpleNamespace()
        c.layers, c.n, c.mu, c.weight, c.band_first, c.band_count, c.surfaceSpectrum = self._column_checks(
            surfaceSpectrum, surfaceTemperature, [(1.0 / math.sqrt(3.0), pi)], bands)
        c.views = _scatter_views(views) if views is not _NO_VIEWS else None
        c.topSpectrum = _grid_spectrum("topSpectrum", topSpectrum, c.n)
        x = c.layers[0].xAxis
        c.scat, c.numbers = self._scatter_checks(scatterers, deltaScaling, x, len(c.layers))
        c.linear = _planck_source(planck, levelTemperatures)
        if c.linear:
            lev = self._level_temperatures(levelTemperatures)
            c.T = np.column_stack([lev[:-1], lev[1:]])
        else:
            c.T = [L.T for L in c.layers]
        c.emissivity = _surface_emissivity(emissivity, x)
        c.depth = [L.depth for L in c.layers]
        c.surface_T = float(surfaceTemperature or 0.0)
        return c

    def _thermal_scatter_uploads(self, ctx, st, c, sizing, workspace_key, points):
        """The uploads of a checked column ``c`` into the kept state ``st`` and the workspace for ``points`` points: the
        arguments of column_flux_scatter_dev and column_radiance_scatter_dev that they share - positional from scat_amount
        to delta_scaling, then the workspace, and the keywords emissivity, I_surface, surface_T, I_top"""
        I_surface = st.buf(ctx, "I_surface").upload(c.surfaceSpectrum) if c.surfaceSpectrum is not None else None
        I_top = st.buf(ctx, "I_top").upload(c.topSpectrum) if c.topSpectrum is not None else None
        emissivity = self._device_emissivity(ctx, st, c.emissivity)
        columns = self._scatter_columns(ctx, st, c.scat, c.numbers)
        workspace = self._scatter_workspace(ctx, sizing, workspace_key, len(c.layers), points)
        return columns, workspace, dict(emissivity=emissivity, I_surface=I_surface, surface_T=c.surface_T, I_top=I_top)

    def solarFluxesTwoStream(self, scatterers=(), deltaScaling=True, solarSpectrum=None, solarTemperature=None, distanceAU=1.0,
                             mu0=1.0, geometry="plane", planetRadius=6.371e8, emissivity=1.0, bands=None, spectra=False):
        """solarFluxes() through a column that also scatters: Rayleigh air, clouds, aerosol (beyond the reference).  A
        delta-two-stream (quadrature) solution per layer and grid point, the layers joined by the adding method, over a
        Lambertian surface of albedo 1 - ``emissivity``; the gas absorbs with the layers' absorption coefficients and
        nothing emits.  With scattering the superposition of solarFluxes() ends for the scattered light only: thermal
        fluxes still add to these level by level - fluxesTwoStream()'s, which sees the same scatterers.

        ``scatterers``: up to 4 Scatterer objects (see there and rayleighScatterer), each with one amount per layer and an
        extinction, a single-scattering albedo and an asymmetry per grid point; ``deltaScaling``: scale the forward peak
        f = g^2 out of every scatterer (delta-Eddington's scaling; recommended for clouds).  Source, ``mu0``, ``geometry``,
        ``planetRadius``, ``emissivity``, ``bands`` and ``spectra`` as solarFluxes() takes them.  The formulas are those of
        lbl_column_twostream_dev (include/pyrad_hip.h): per layer t = k depth + sum_c amount_c ext_c (scaled), the
        two-stream reflectance and transmittance R, T of the layer to diffuse light and Rb, Tb, Td to each beam, and the
        level relations up_(l+1) = T up_l + R dn_(l+1) + P, dn_l = T dn_(l+1) + R up_l + Q solved exactly.
        Returns a TwoStreamFluxes: ``up``, ``down`` (diffuse plus direct), ``direct``, ``net``, ``heatingRate``,
        ``absorbedSurface``.  Without scatterers it is solarFluxes() over a Lambertian surface with the one diffuse angle
        mu = 1 / sqrt(3).
        The absorption coefficients are the resident ones of transmission() and fluxes(): nothing is accumulated again.
        The kernels keep five numbers per level and point in a workspace that stays with the atmosphere: sized for the
        widest band, but never above 256 MiB - a longer band is done in several passes, with the same bits.  Everything
        is validated (ValueError) before the device is touched."""
        layers, n = self._column_layers()
        first = layers[0]
        x = first.xAxis
        nl = len(layers)
        scat, numbers = self._scatter_checks(scatterers, deltaScaling, x, nl)
        S0 = _solar_spectrum(solarSpectrum, solarTemperature, distanceAU, x)
        mu_s, weight_s = _solar_beams(mu0)
        depth = [L.depth for L in layers]
        slant = solarSlants(depth, list(zip(mu_s, weight_s)), geometry, planetRadius)
        beam_weight = weight_s * mu_s
        emissivity = _surface_emissivity(emissivity, x)
        band_first, band_count = _flux_bands(first.rangeMin, first.rangeMax, n, bands)
        res = utils.BASE_RESOLUTION
        nb = len(band_first)
        ctx = _ctx()
        kbufs, _ = self._column_abs_coef(ctx, layers, n)
        st = _kept_state(self, "_twostream_state")
        st.reserve(ctx, max(n, nb * 3 * (nl + 1)))
        source = st.buf(ctx, "S0").upload(S0)
        if not isinstance(emissivity, float):
            emissivity = st.buf(ctx, "emissivity").upload(emissivity)
        columns = self._scatter_columns(ctx, st, scat, numbers)
        # (the widest band in one pass)
        workspace = self._scatter_workspace(ctx, ctx.column_twostream_workspace, "_twostream_workspace", nl, max(band_count))
        level = st.buf(ctx, "level")
        names = ("up_top", "down_surface", "direct_surface", "up_surface")
        spec = {name: st.buf(ctx, name) if spectra else None for name in names}
        ctx.column_twostream_dev(kbufs, depth, first.rangeMin, first.rangeMax, n, source, beam_weight, slant, *columns,
                                 int(bool(deltaScaling)), band_first, band_count, workspace, level, emissivity=emissivity,
                                 **spec)
        sums = level.download(nb * 3 * (nl + 1)).reshape(nb, 3, nl + 1) * res
        up, direct = sums[:, 0, :], sums[:, 2, :]
        down = sums[:, 1, :] + direct
        heat = heatingRates(up - down, [L.P for L in layers], [L.T for L in layers], depth)
        up, down, direct, heat = _band_values(bands, [up, down, direct, heat])
        got = {name: spec[name].download(n) if spectra else None for name in names}
        return TwoStreamFluxes(up, down, direct, heat, mu_s, beam_weight, slant, upSpectrum=got["up_top"],
                               downSpectrum=got["down_surface"] + got["direct_surface"] if spectra else None,
                               directSpectrum=got["direct_surface"], upSurfaceSpectrum=got["up_surface"])

    def fluxesTwoStream(self, scatterers=(), deltaScaling=True, surfaceTemperature=None, surfaceSpectrum=None, topSpectrum=None,
                        emissivity=1.0, planck="layer", levelTemperatures=None, bands=None, spectra=False):
        """fluxes() through a column that also scatters: the thermal fluxes under clouds and aerosol (beyond the
        reference).  solarFluxesTwoStream()'s layer solution and adding, with the layers' own emission as the source
        instead of a beam, over an emitting Lambertian surface; the sum of the two calls is a cloudy column's flux.

        ``scatterers`` and ``deltaScaling`` as solarFluxesTwoStream() takes them; ``surfaceTemperature`` /
        ``surfaceSpectrum``, ``topSpectrum``, ``emissivity`` (a number in [0, 1], n values or a table; 1: the black
        surface), ``planck``, ``levelTemperatures``, ``bands`` and ``spectra`` as fluxes() takes them.  Fluxes are
        hemispheric - an isotropic radiance I is the flux pi I - and the result corresponds to fluxes(angles=[(1 / sqrt(3),
        pi)]), which it equals to rounding without scatterers.  The formulas are those of lbl_column_flux_scatter_dev
        (include/pyrad_hip.h): with Bt = pi B at a layer's top level, Bb at its bottom level (both pi B(T_l) for
        planck="layer"), d = Bb - Bt, R, T the layer's two-stream reflectance and transmittance and Ab = 1 - R - T,
            h = (Ab + 2 R) / (sqrt(3) (t - tsg)) - T        P = Bt Ab + d h        Q = Bb Ab - d h
        are what the layer emits upward at its top and downward at its bottom - the source linear in optical depth of
        planck="linear", through a scattering layer - and the level relations up_(l+1) = T up_l + R dn_(l+1) + P,
        dn_l = T dn_(l+1) + R up_l + Q are solved exactly between dn_L = pi topSpectrum (or 0) and
        up_0 = e pi Is + (1 - e) dn_0.
        Returns a Fluxes with mu = [1 / sqrt(3)] and weight = [pi].  The absorption coefficients are the resident ones;
        the workspace (four numbers per level and point) stays with the atmosphere, at most 256 MiB - a longer band is
        done in several passes, with the same bits.  Everything is validated (ValueError) before the device is touched."""
        c = self._thermal_scatter_checks(surfaceTemperature, surfaceSpectrum, topSpectrum, bands, scatterers, deltaScaling,
                                         emissivity, planck, levelTemperatures)
        layers, n, first = c.layers, c.n, c.layers[0]
        nl, nb = len(layers), len(c.band_first)
        ctx = _ctx()
        kbufs, _ = self._column_abs_coef(ctx, layers, n)
        st = _kept_state(self, "_scatter_flux_state")
        st.reserve(ctx, max(n, nb * 2 * (nl + 1)))
        # (the widest band in one pass)
        columns, workspace, kw = self._thermal_scatter_uploads(ctx, st, c, ctx.column_flux_scatter_workspace,
                                                               "_scatter_flux_workspace", max(c.band_count))
        level = st.buf(ctx, "level")
        names = ("up_top", "down_surface", "up_surface")
        spec = {name: st.buf(ctx, name) if spectra else None for name in names}
        ctx.column_flux_scatter_dev(kbufs, c.T, int(c.linear), c.depth, first.rangeMin, first.rangeMax, n, *columns,
                                    int(bool(deltaScaling)), c.band_first, c.band_count, workspace, level, **kw, **spec)
        sums = level.download(nb * 2 * (nl + 1)).reshape(nb, 2, nl + 1) * utils.BASE_RESOLUTION
        up, down = sums[:, 0, :], sums[:, 1, :]
        heat = heatingRates(up - down, [L.P for L in layers], [L.T for L in layers], c.depth)
        up, down, heat = _band_values(bands, [up, down, heat])
        return Fluxes(up, down, heat, c.mu, c.weight,
                      upSpectrum=spec["up_top"].download(n) if spectra else None,
                      downSpectrum=spec["down_surface"].download(n) if spectra else None,
                      upSurfaceSpectrum=spec["up_surface"].download(n) if spectra else None)

    def radianceTwoStream(self, views, scatterers=(), deltaScaling=True, surfaceTemperature=None, surfaceSpectrum=None,
                          topSpectrum=None, emissivity=1.0, planck="layer", levelTemperatures=None, instrument=None):
        """What an instrument sees of fluxesTwoStream()'s column: the spectrum leaving the top of a cloudy column, or
        arriving under it at the surface, at any viewing cosine (beyond the reference).  The two-stream source function
        technique (Toon et al. 1989): fluxesTwoStream()'s solution gives the hemispheric fluxes F+ and F- inside every
        layer, they give the source function in the viewing direction
            S+-(s, mu) = (a B(s) + (w / 2) [(1 +- sqrt(3) g mu) F+(s) + (1 -+ sqrt(3) g mu) F-(s)]) / pi
        (w the layer's scaled single-scattering albedo, g its asymmetry, a = 1 - w), and the radiance is the formal
        solution along the view - in closed form per layer, smooth through lam mu = 1 (lbl_column_radiance_scatter_dev,
        include/pyrad_hip.h).

        ``views``: a sequence of mu (upward at the top) or (mu, "up" | "down"), mu in (0, 1]: "up" is the radiance leaving
        the top of the column, from the Lambertian surface's up_0 / pi; "down" the radiance arriving at the surface, from
        ``topSpectrum`` (or 0).  More than 16 views run in chunks of 16; a view's values do not depend on the others.
        Every other argument as fluxesTwoStream() takes it.  ``instrument``: an Instrument - the rows are convolved onto
        its channels on the device, as radiance() does.
        At mu = 1 / sqrt(3) pi times the radiance is fluxesTwoStream()'s flux, without scatterers the result is
        radiance()'s along the same slant to rounding, and a column at one temperature under a sky of the same shows
        B(T) in every view.  The two-term phase function's 1 - sqrt(3) g mu is negative for g mu > 1 / sqrt(3), which
        ``deltaScaling`` (g -> g / (1 + g)) avoids; nothing is clamped.
        Returns a ScatterRadiance.  The absorption coefficients are the resident ones; the workspace (four numbers per
        level and point) stays with the atmosphere, at most 256 MiB - a longer grid is done in several passes, with the same
        bits.  Everything is validated (ValueError) before the device is touched."""
        c = self._thermal_scatter_checks(surfaceTemperature, surfaceSpectrum, topSpectrum, None, scatterers, deltaScaling,
                                         emissivity, planck, levelTemperatures, views=views)
        layers, n, first = c.layers, c.n, c.layers[0]
        view_mu, view_down, direction = c.views
        support = None
        if instrument is not None:
            if not isinstance(instrument, Instrument):
                raise ValueError("instrument: an Instrument, not %r" % (instrument,))
            support = instrument.support(first.rangeMin, first.rangeMax, n)
        chunk = nat.limit("scatter_views")
        V = len(view_mu)
        ctx = _ctx()
        kbufs, _ = self._column_abs_coef(ctx, layers, n)
        st = _kept_state(self, "_scatter_radiance_state")
        st.reserve(ctx, n)
        # (the grid in one pass)
        columns, workspace, kw = self._thermal_scatter_uploads(ctx, st, c, ctx.column_radiance_scatter_workspace,
                                                               "_scatter_radiance_workspace", n)
        rad = _kept_state(self, "_scatter_radiance_rows").reserve(ctx, min(V, chunk) * n).buf(ctx, "radiance")
        X = n if instrument is None else len(instrument)
        out = None
        if instrument is not None:
            out = _kept_state(self, "_scatter_radiance_out").reserve(ctx, min(V, chunk) * X).buf(ctx, "out")
        values = np.empty((V, X))
        for lo in range(0, V, chunk):
            hi = min(lo + chunk, V)
            ctx.column_radiance_scatter_dev(kbufs, c.T, int(c.linear), c.depth, first.rangeMin, first.rangeMax, n, *columns,
                                            int(bool(deltaScaling)), view_mu[lo:hi], view_down[lo:hi], workspace, rad, **kw)
            if instrument is None:
                values[lo:hi] = rad.download((hi - lo) * n).reshape(hi - lo, n)
            else:
                _ils_convolve(ctx, instrument, first.rangeMin, first.rangeMax, n, support, [(rad, r * n) for r in range(hi - lo)],
                              out)
                values[lo:hi] = out.download((hi - lo) * X).reshape(hi - lo, X)
        return ScatterRadiance(first.xAxis if instrument is None else instrument.centres.copy(), values, view_mu, direction)

    def solarRadianceTwoStream(self, views, scatterers=(), deltaScaling=True, solarSpectrum=None, solarTemperature=None,
                               distanceAU=1.0, mu0=1.0, geometry="plane", planetRadius=6.371e8, emissivity=1.0,
                               instrument=None):
        """What an instrument sees of solarFluxesTwoStream()'s column in sunlight: the reflected spectrum leaving the top,
        or the diffuse sky arriving at the surface, at any viewing cosine (beyond the reference).  radianceTwoStream()'s
        source function technique with the beam in the source: solarFluxesTwoStream()'s solution gives the hemispheric
        fluxes F+ and F- inside every layer and the beam's flux Fd through the horizontal at its top, and
            pi S+-(s, mu) = (w / 2) [(1 +- sqrt(3) g mu) F+(s) + (1 -+ sqrt(3) g mu) F-(s)]
                            + (w / (2 sqrt(3) m)) (1 -+ 3 g mu m) Fd exp(-s / m)
        (w the layer's scaled single-scattering albedo, g its asymmetry, m = 1 / slant the beam's cosine in the layer) is
        integrated along the view in closed form per layer, smooth through mu = m and lam mu = 1
        (lbl_column_beam_radiance_dev, include/pyrad_hip.h).  The second line is the singly scattered beam.  The radiance
        is the AZIMUTHAL MEAN: the two-term phase function 1 + 3 g cos(Theta) is averaged over the azimuth between sun and
        view, which leaves 1 -+ 3 g mu m, and there is no azimuth argument.  Its normalisation w / (2 sqrt(3) m) is the
        quadrature scheme's, 2 / sqrt(3) times the w / (4 m) of an exact single-scattering calculation - a known property
        of the two-stream source function technique: with it pi times the radiance at mu = 1 / sqrt(3) is
        solarFluxesTwoStream()'s flux.

        ``views`` and ``instrument`` as radianceTwoStream() takes them: "up" starts from the Lambertian surface's
        up_0 / pi (diffuse and direct light reflected alike), "down" from 0 - the diffuse sky; the solar disc itself is
        not in it.  More than 16 views run in chunks of 16; a view's values do not depend on the others.  ``mu0``: ONE
        cosine in (0, 1] - an instrument sees one sun, and a day's mean of radiances along a fixed view means nothing, so
        a list of (mu0, weight) pairs is refused.  Every other argument as solarFluxesTwoStream() takes it.
        A daytime spectrum is this plus radianceTwoStream(...) for the same views and scatterers, view by view: the
        thermal and the solar radiances superpose.
        Without scatterers an "up" view is solarFluxes(angles=[(mu, pi)], spectra=True).upSpectrum / pi over the same
        Lambertian surface and a "down" view is exactly 0; a layer split in two gives the same radiances.  The two-term
        phase function's 1 - 3 g mu m is negative for g mu m > 1 / 3, which ``deltaScaling`` (g -> g / (1 + g)) eases;
        nothing is clamped, as in radianceTwoStream().
        Returns a ScatterRadiance.  The absorption coefficients are the resident ones; the workspace (five numbers per
        level and point) stays with the atmosphere, at most 256 MiB - a longer grid is done in several passes, with the same
        bits.  Everything is validated (ValueError) before the device is touched."""
        layers, n = self._column_layers()
        first = layers[0]
        x = first.xAxis
        nl = len(layers)
        view_mu, view_down, direction = _scatter_views(views)
        scat, numbers = self._scatter_checks(scatterers, deltaScaling, x, nl)
        S0 = _solar_spectrum(solarSpectrum, solarTemperature, distanceAU, x)
        if isinstance(mu0, (bool, str)) or not isinstance(mu0, (int, float, np.integer, np.floating)):
            raise ValueError("mu0: one cosine in (0, 1] - one sun per call - not %r" % (mu0,))
        mu_s, _ = _solar_beams(mu0)
        depth = [L.depth for L in layers]
        slant = solarSlants(depth, float(mu0), geometry, planetRadius)
        emissivity = _surface_emissivity(emissivity, x)
        support = None
        if instrument is not None:
            if not isinstance(instrument, Instrument):
                raise ValueError("instrument: an Instrument, not %r" % (instrument,))
            support = instrument.support(first.rangeMin, first.rangeMax, n)
        chunk = nat.limit("beam_views")
        V = len(view_mu)
        ctx = _ctx()
        kbufs, _ = self._column_abs_coef(ctx, layers, n)
        st = _kept_state(self, "_beam_view_state")
        st.reserve(ctx, n)
        source = st.buf(ctx, "S0").upload(S0)
        emissivity = self._device_emissivity(ctx, st, emissivity)
        columns = self._scatter_columns(ctx, st, scat, numbers)
        # (the grid in one pass)
        workspace = self._scatter_workspace(ctx, ctx.column_beam_radiance_workspace, "_beam_view_workspace", nl, n)
        rad = _kept_state(self, "_beam_view_rows").reserve(ctx, min(V, chunk) * n).buf(ctx, "radiance")
        X = n if instrument is None else len(instrument)
        out = None
        if instrument is not None:
            out = _kept_state(self, "_beam_view_out").reserve(ctx, min(V, chunk) * X).buf(ctx, "out")
        values = np.empty((V, X))
        for lo in range(0, V, chunk):
            hi = min(lo + chunk, V)
            ctx.column_beam_radiance_dev(kbufs, depth, first.rangeMin, first.rangeMax, n, source, float(mu_s[0]), slant,
                                         *columns, int(bool(deltaScaling)), view_mu[lo:hi], view_down[lo:hi], workspace, rad,
                                         emissivity=emissivity)
            if instrument is None:
                values[lo:hi] = rad.download((hi - lo) * n).reshape(hi - lo, n)
            else:
                _ils_convolve(ctx, instrument, first.rangeMin, first.rangeMax, n, support, [(rad, r * n) for r in range(hi - lo)],
                              out)
                values[lo:hi] = out.download((hi - lo) * X).reshape(hi - lo, X)
        return ScatterRadiance(first.xAxis if instrument is None else instrument.centres.copy(), values, view_mu, direction)

    def jacobians(self, surfaceTemperature=None, surfaceSpectrum=None, angles=3, bands=None, molecules=True, spectra=False,
                  temperature="planck", emissivity=None, reflection="lambertian", topSpectrum=None):
        """Analytic sensitivities of the upward flux at the top (beyond the reference), in one pass over the resident
        absorption coefficients.

        Column, layer order, grid, angle set (fluxAngles), bands (as fluxes()), nan_to_num and res factor of fluxes().  At
        every grid point nu_j and angle k (mu_k, W_k):
            tau_l = k_l(nu_j) depth_l      t_lk = exp(-tau_l / mu_k)      B_l = planckWavenumber(nu_j, T_l)
            I_0k  = surfaceSpectrum[j] or B(nu_j, T_s)      I_(l+1)k = t_lk I_lk + (1 - t_lk) B_l
            A_lk  = prod_{i>l} t_ik  (A_(L-1)k = 1)          A_(-1)k = prod_i t_ik
            F(nu_j)             = sum_k W_k I_Lk                                             upward spectral flux at the top
            dF/d ln tau_l       = sum_k W_k (tau_l / mu_k) A_lk t_lk (B_l - I_lk)            all absorbers of layer l scaled
            dF/d ln n_(m,l)     = sum_k W_k (k_(m,l) depth_l / mu_k) A_lk t_lk (B_l - I_lk)  molecule m of layer l
            dF/dT_l  (Planck)   = sum_k W_k A_lk (1 - t_lk) dB_l/dT                          absorption coefficients held fixed
            dF/dT_l  (absorption) = sum_k W_k (dk_l/dT depth_l / mu_k) A_lk t_lk (B_l - I_lk)  temperature="full" only
            dF/dT_s             = sum_k W_k A_(-1)k dB(nu_j, T_s)/dT                         only when the surface is T_s
            band value          = res * sum over the band's points of nan_to_num(spectral value)
        k_(m,l) is molecule m's own absorption coefficient in layer l (Molecule.absCoef); their sum over m is k_l up to
        rounding.  The molecule Jacobian is the sensitivity to absorber amount AT FIXED LINE SHAPES: the self-broadening
        fraction in the Lorentz width is not differentiated.  ``temperature``: "planck" (default) gives the Planck part only;
        "full" also the absorption part through dk_l/dT (Layer.absCoefDT: line intensity, widths, number density; the Voigt line
        shape only), one more term per layer in the same pass: Jacobians.temperatureAbsorption and .temperatureFull.  The
        spectral temperatureSpectrum stays the Planck part.
        ``molecules``: also the molecule terms (one merged accumulate job per layer and molecule, kept with the atmosphere
        and re-used while that molecule's inputs stand; False skips them).  ``spectra``: also the spectral dF/dT_l and
        dF/d ln tau_l, (L, n) each.  Returns a Jacobians.  The layers' absorption coefficients are the ones fluxes() and
        transmission() keep resident: after either nothing is accumulated again.  No other result of the model changes.
        Everything is validated (ValueError) before the device is touched.

        ``emissivity``: None, the black surface above, or the surface's emissivity e as fluxes() takes it, with ``reflection``
        and ``topSpectrum`` as there: the derivatives of fluxes(emissivity=..., reflection=..., topSpectrum=...).up at the top
        (lbl_column_jacobian_surface_dev).  With Id_(l+1)k the downward radiance entering layer l from above, D_k = Id_0k,
        R_k and Iu_0k = e Is + (1 - e) R_k as fluxes() defines them, Iu_lk the upward radiances from there, C_lk =
        prod_{i<l} t_ik, Ttot_k = prod_i t_ik and Q_k = (1 - e) W_k (sum_k' W_k' Ttot_k') / sum_k W_k ("lambertian") or
        (1 - e) W_k Ttot_k ("specular"):
            gu_lk = A_lk t_lk (B_l - Iu_lk)        gd_lk = C_lk t_lk (B_l - Id_(l+1)k)      (the leg seen through the surface)
            dF/d ln tau_l     = sum_k (tau_l / mu_k) (W_k gu_lk + Q_k gd_lk)                 molecules and dk/dT likewise
            dF/dT_l  (Planck) = sum_k (W_k A_lk + Q_k C_lk) (1 - t_lk) dB_l/dT
            dF/dT_s           = e sum_k W_k Ttot_k dB(nu_j, T_s)/dT
            dF/de             = sum_k W_k Ttot_k (Is - R_k)                                  Jacobians.emissivity
        (an emissivity given per grid point or as a table moves as a whole: dF/de is the derivative by one number added to
        it everywhere; Jacobians.emissivitySpectrum has it per grid point).  With emissivity 1 and one or two angles every
        value but dF/de is the black surface's bit for bit.  ``topSpectrum`` without an emissivity is a ValueError: the
        black surface's outgoing flux does not depend on it.
        The Planck source is the layer source: one temperature per layer (fluxes() and radiance() also take
        planck="linear"; its derivatives are jacobiansLinear()'s)."""
        return self._column_jacobians(False, surfaceTemperature, surfaceSpectrum, angles, bands, molecules, spectra, temperature,
                                      emissivity, reflection, topSpectrum)

    def observe(self, instrument, surfaceTemperature=None, surfaceSpectrum=None, mu=1.0, jacobians=False, emissivity=None):
        """What an instrument above the column sees at viewing cosine ``mu`` (beyond the reference): the upward radiance at
        the top (fluxes() with the angle set [(mu, 1.0)]: column, layer order, grid and surface source as there) convolved
        onto the channels of ``instrument`` on the device, beside the resident spectrum; only the channel values come down.
        ``jacobians``: also the channel weighting functions, jacobians() for the same angle (molecules=False, its spectral
        dI/dT_l and dI/d ln tau_l) convolved in the same call.  Returns an Observation.  With mu = 1 the radiance is
        convolve(instrument, transmission(...)) bit for bit wherever fluxes() documents that identity.  The absorption
        coefficients are the resident ones: after transmission() or fluxes() nothing is accumulated again.  Everything is
        validated (ValueError) before the device is touched.

        ``emissivity``: None, the black surface above, or the surface's emissivity e as fluxes() takes it.  The surface then
        emits e Is and reflects, specularly at ``mu``, the downward radiance of the column under cold space (with the single
        viewing angle the Lambertian and the specular reflection of fluxes() are one expression): the radiance is
        fluxes(emissivity=e, reflection="specular", angles=[(mu, 1.0)])'s upward spectrum at the top, the weighting functions
        jacobians(emissivity=e, ...)'s for that angle, and Observation.emissivityJacobian their dR_c/de.
        The Planck source is the layer source: one temperature per layer (fluxes() and radiance() also take
        planck="linear"; its derivatives are observeLinear()'s)."""
        return self._observe(False, instrument, surfaceTemperature, surfaceSpectrum, mu, jacobians, emissivity)

    def _level_chain(self):
        """The (L + 1) x L matrix M of levelTemperatures(): lev = M T for the layers' temperatures T (the map is linear, its
        coefficients depend on the layers' depths alone)."""
        layers, _ = self._column_layers()
        d = [float(L.depth) for L in layers]
        nl = len(layers)
        M = np.zeros((nl + 1, nl))
        if nl == 1:
            M[:, 0] = 1.0
            return M
        for i in range(1, nl):
            a = d[i - 1] / (d[i - 1] + d[i])
            M[i, i - 1], M[i, i] = 1.0 - a, a
        M[0] = -M[1]
        M[0, 0] += 2.0
        M[nl] = -M[nl - 1]
        M[nl, nl - 1] += 2.0
        return M

    def jacobiansLinear(self, surfaceTemperature=None, surfaceSpectrum=None, angles=3, bands=None, molecules=True,
                        spectra=False, temperature="planck", emissivity=None, reflection="lambertian", topSpectrum=None,
                        levelTemperatures=None):
        """jacobians() for fluxes(planck="linear"): analytic sensitivities of the upward flux at the top with the Planck
        function linear in optical depth through every layer, the temperatures of the levels among the variables
        (lbl_column_jacobian_linear_dev; beyond the reference).  Column, angles, bands, molecules, spectra, emissivity,
        reflection and topSpectrum as jacobians() takes them (``emissivity`` None is the black surface);
        ``levelTemperatures`` as fluxes(planck="linear") takes them (None: levelTemperatures()).  With x = k_l depth_l /
        mu_k, t = exp(-x), g as fluxes() has it, h = (1 - t) - g, g' = h / x, Bbot and Btop the Planck function at the
        layer's lower and upper level, and A, C, Q, Iu, Id as jacobians() defines them over the linear forward radiances:
            dF/d ln tau_l   = sum_k W_k A_lk [x t (Bbot - Iu_lk) + h (Btop - Bbot)] + Q_k C_lk [x t (Btop - Id_(l+1)k) + h (Bbot - Btop)]
            molecules, dk/dT: the same with (k_m depth_l / mu_k) [t (B - I) + g' (B' - B)] per leg
            dF/dT_bottom(l) = dB(lev_l)/dT     sum_k (W_k A_lk h + Q_k C_lk g)
            dF/dT_top(l)    = dB(lev_(l+1))/dT sum_k (W_k A_lk g + Q_k C_lk h)
            dF/dT_s, dF/de  : jacobians()'s
        Returns a Jacobians with ``edgeTemperature`` (L, 2), ``levelTemperature`` (L + 1,) - level i is the top edge of
        layer i - 1 plus the bottom edge of layer i - and with ``spectra`` ``levelTemperatureSpectrum`` (L + 1, n) and
        opticalDepthSpectrum.  ``temperature`` (L,) is the exact chain through levelTemperatures(), which is linear in the
        layers' temperatures, when the default level temperatures are in use, and None when level temperatures were given;
        it is the Planck part, the absorption coefficients held fixed.  temperature="full" adds temperatureAbsorption
        through dk_l/dT as jacobians() does.  olr is fluxes(planck="linear")'s upward flux at the top to rounding.
        Everything is validated (ValueError) before the device is touched."""
        return self._column_jacobians(True, surfaceTemperature, surfaceSpectrum, angles, bands, molecules, spectra, temperature,
                                      emissivity, reflection, topSpectrum, levelTemperatures)

    def _column_jacobians(self, linear, surfaceTemperature, surfaceSpectrum, angles, bands, molecules, spectra, temperature,
                          emissivity, reflection, topSpectrum, levelTemperatures=None):
        """jacobians() and, with ``linear``, jacobiansLinear()"""
        if temperature not in ("planck", "full"):
            raise ValueError("temperature: \"planck\" or \"full\", not %r" % (temperature,))
        layers, n, mu, weight, band_first, band_count, surfaceSpectrum = self._column_checks(
            surfaceSpectrum, surfaceTemperature, angles, bands)
        first = layers[0]
        refl = _surface_reflection(reflection)
        edges = chain = None
        if linear:
            lev = self._level_temperatures(levelTemperatures)
            chain = self._level_chain() if levelTemperatures is None or levelTemperatures is True else None
            edges = np.column_stack([lev[:-1], lev[1:]])
        black = emissivity is None
        if black:
            if topSpectrum is not None:
                raise ValueError("topSpectrum: the outgoing flux over a black surface does not depend on it (give emissivity)")
        else:
            topSpectrum = _grid_spectrum("topSpectrum", topSpectrum, n)
            emissivity = _surface_emissivity(emissivity, first.xAxis)
        if linear or not black:  # behaviour, kept: jacobians() looks at the weights' sum over a reflecting surface only
            _weight_sum(weight)
        names = [[m.name for m in L] for L in layers]
        full = temperature == "full"
        # behaviour, kept: jacobiansLinear() words the limit with dk/dT whatever ``temperature`` is
        self._term_count(layers, molecules, full, linear or full)
        res = utils.BASE_RESOLUTION
        nl, nb = len(layers), len(band_first)
        ctx = _ctx()
        if ctx.option("sweep_ieee_divisions"):
            raise ValueError("Jacobians exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)")
        kbufs, plan = self._column_abs_coef(ctx, layers, n)
        term_bufs, term_layer, n_mol_terms = self._term_buffers(ctx, layers, n, plan, molecules, full)
        h = 2 if black and not linear else 3         # the values of a band ahead of the layers': F, dF/dT_s and dF/de
        w = 3 if linear else 2                       # ... and per layer: d ln tau and T, or d ln tau and the two edges' T
        nv = h + w * nl + len(term_bufs)
        out = _kept_state(self, "_jacobian_out").reserve(ctx, max(n, nb * nv))
        I_surface = out.buf(ctx, "I_surface").upload(surfaceSpectrum) if surfaceSpectrum is not None else None
        jac = out.buf(ctx, "jac")
        ln_tau_spec = T_spec = e_spec = I_top = None
        if spectra:
            ln_tau_spec, T_spec = self._jacobian_spectra(ctx, linear, nl, n)
        if linear or not black:  # behaviour, kept: jacobiansLinear() reserves the surface's state over the black surface too
            sst = _kept_state(self, "_jacobian_surface").reserve(ctx, n)
            emissivity = self._device_emissivity(ctx, sst, emissivity)
            I_top = sst.buf(ctx, "I_top").upload(topSpectrum) if topSpectrum is not None else None
            e_spec = sst.buf(ctx, "e_spec") if spectra and not black else None
        self._jacobian_call(ctx, layers, n, kbufs, edges, emissivity, refl, mu, weight, band_first, band_count, jac,
                            T_spectra=T_spec, I_top=I_top, e_spectrum=e_spec, I_surface=I_surface,
                            surface_T=float(surfaceTemperature or 0.0), term_abs_coef=term_bufs, term_layer=term_layer,
                            ln_tau_spectra=ln_tau_spec)
        v = jac.download(nb * nv).reshape(nb, nv) * res
        mol, o = None, h + w * nl                    # (where the terms begin: the molecules' layer by layer, then dk/dT)
        if molecules:
            mol, at = [], o
            for L in layers:
                mol.append(v[:, at:at + len(L)])
                at += len(L)
            mol = _band_values(bands, mol)
        rows = [v[:, 0], v[:, 1], v[:, h:h + nl]]
        if linear:
            edge = v[:, 3 + nl:3 + 3 * nl].reshape(nb, nl, 2)
            dlev = self._levels_of_edges(edge)
            rows += [edge, dlev] + ([dlev @ chain] if chain is not None else [])
        else:
            rows.append(v[:, h + nl:h + 2 * nl])
        olr, dTs, dtau, *own = _band_values(bands, rows)
        if surfaceSpectrum is not None:
            dTs = None
        T_rows = T_spec.download((w - 1) * nl * n) if spectra else None          # (the downloads in this order: T, ln tau, e)
        tau_rows = ln_tau_spec.download(nl * n).reshape(nl, n) if spectra else None
        dT_abs = _band_values(bands, [v[:, o + n_mol_terms:]])[0] if full else None
        de = None if black else _band_values(bands, [v[:, 2]])[0]
        e_row = e_spec.download(n) if e_spec is not None else None
        if not linear:
            return Jacobians(olr, dTs, own[0], dtau, mol, names, mu, weight,
                             temperatureSpectrum=T_rows.reshape(nl, n) if spectra else None, opticalDepthSpectrum=tau_rows,
                             temperatureAbsorption=dT_abs, emissivity=de, emissivitySpectrum=e_row)
        lev_spec = self._levels_of_edges(T_rows.reshape(nl, 2, n).transpose(2, 0, 1)).T.copy() if spectra else None
        return Jacobians(olr, dTs, own[2] if chain is not None else None, dtau, mol, names, mu, weight,
                         opticalDepthSpectrum=tau_rows, temperatureAbsorption=dT_abs, emissivity=de, emissivitySpectrum=e_row,
                         edgeTemperature=own[0], levelTemperature=own[1], levelTemperatureSpectrum=lev_spec)

    def jacobiansTwoStream(self, scatterers=(), deltaScaling=True, surfaceTemperature=None, surfaceSpectrum=None,
                           topSpectrum=None, emissivity=1.0, planck="layer", levelTemperatures=None, bands=None, molecules=True,
                           spectra=False, temperature="planck"):
        """Analytic sensitivities of fluxesTwoStream()'s upward flux at the top: jacobians() / jacobiansLinear() through a
        column that also scatters, and the sensitivity to every scatterer's amount (beyond the reference).  One adjoint pass
        over the stacks that the forward solution builds (lbl_column_jacobian_scatter_dev, include/pyrad_hip.h): with the
        stack above level l + 1 reflecting Rs' and passing Tu' of an upward flux to the top, and the surface with the layers
        below level l reflecting A_l, a change of layer l alone moves the flux at the top by
            dF = w1 (dT up_l + dR dn_(l+1) + dP) + w2 (dT dn_(l+1) + dR up_l + dQ)
            w1 = Tu' / ((1 - R Rs') - T^2 A_l Rs' / (1 - R A_l))        w2 = w1 T A_l / (1 - R A_l)
        where R, T, P, Q are the layer's reflectance, transmittance and sources as fluxesTwoStream() defines them, and
        their derivatives to the layer's three depths are closed forms.

        Arguments as fluxesTwoStream() takes them; ``molecules``, ``spectra`` and ``temperature`` as jacobians() takes
        them.  Returns a Jacobians with mu = [1 / sqrt(3)] and weight = [pi]: ``olr`` (fluxesTwoStream()'s up at the top, bit
        for bit), ``surfaceTemperature`` (None with a surface spectrum), ``emissivity``, ``opticalDepth`` (the gas of a layer
        scaled), ``molecules``, and ``scatterers``, (C, L): dF/d ln amount of scatterer c in layer l, 0 where the amount is
        0.  planck="layer": ``temperature`` (L,), the Planck part; planck="linear": ``edgeTemperature``,
        ``levelTemperature`` and, over the default level temperatures, ``temperature`` as jacobiansLinear() gives them.
        temperature="full" adds temperatureAbsorption through dk_l/dT.  With ``spectra`` also opticalDepthSpectrum and
        temperatureSpectrum (planck="layer") or levelTemperatureSpectrum (planck="linear").  Without scatterers the result
        is jacobians(angles=[(1 / sqrt(3), pi)], emissivity=..., reflection="lambertian") (jacobiansLinear()) to rounding.
        Not differentiated: the scatterers' albedo and asymmetry, and the downward flux at the surface.  The workspace (five
        numbers per level and point) stays with the atmosphere, at most 256 MiB.  Everything is validated (ValueError)
        before the device is touched."""
        if temperature not in ("planck", "full"):
            raise ValueError("temperature: \"planck\" or \"full\", not %r" % (temperature,))
        c = self._thermal_scatter_checks(surfaceTemperature, surfaceSpectrum, topSpectrum, bands, scatterers, deltaScaling,
                                         emissivity, planck, levelTemperatures)
        layers, n, first, linear = c.layers, c.n, c.layers[0], c.linear
        chain = self._level_chain() if linear and (levelTemperatures is None or levelTemperatures is True) else None
        names = [[m.name for m in L] for L in layers]
        full = temperature == "full"
        self._term_count(layers, molecules, full, full)
        nl, nb, nc = len(layers), len(c.band_first), len(c.scat)
        ctx = _ctx()
        if ctx.option("sweep_ieee_divisions"):
            raise ValueError("Jacobians exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)")
        kbufs, plan = self._column_abs_coef(ctx, layers, n)
        term_bufs, term_layer, n_mol_terms = self._term_buffers(ctx, layers, n, plan, molecules, full)
        nt = 2 if linear else 1
        o = 3 + (1 + nt + nc) * nl                   # (where the terms begin)
        nv = o + len(term_bufs)
        st = _kept_state(self, "_scatter_jacobian_state")
        st.reserve(ctx, max(n, nb * nv))
        # (the widest band in one pass)
        columns, workspace, kw = self._thermal_scatter_uploads(ctx, st, c, ctx.column_jacobian_scatter_workspace,
                                                               "_scatter_jacobian_workspace", max(c.band_count))
        jac = st.buf(ctx, "jac")
        ln_tau_spec, T_spec = self._jacobian_spectra(ctx, linear, nl, n) if spectra else (None, None)
        ctx.column_jacobian_scatter_dev(kbufs, c.T, int(linear), c.depth, first.rangeMin, first.rangeMax, n, *columns,
                                        int(bool(deltaScaling)), c.band_first, c.band_count, workspace, jac,
                                        term_abs_coef=term_bufs, term_layer=term_layer, ln_tau_spectra=ln_tau_spec,
                                        T_spectra=T_spec, **kw)
        v = jac.download(nb * nv).reshape(nb, nv) * utils.BASE_RESOLUTION
        mol = None
        if molecules:
            mol, at = [], o
            for L in layers:
                mol.append(v[:, at:at + len(L)])
                at += len(L)
            mol = _band_values(bands, mol)
        at = 3 + (1 + nt) * nl
        rows = [v[:, 0], v[:, 1], v[:, 2], v[:, 3:3 + nl], v[:, at:at + nc * nl].reshape(nb, nc, nl)]
        if linear:
            edge = v[:, 3 + nl:at].reshape(nb, nl, 2)
            dlev = self._levels_of_edges(edge)
            rows += [edge, dlev] + ([dlev @ chain] if chain is not None else [])
        else:
            rows.append(v[:, 3 + nl:at])
        olr, dTs, de, dtau, dscat, *own = _band_values(bands, rows)
        if c.surfaceSpectrum is not None:
            dTs = None
        T_rows = T_spec.download(nt * nl * n) if spectra else None
        tau_rows = ln_tau_spec.download(nl * n).reshape(nl, n) if spectra else None
        dT_abs = _band_values(bands, [v[:, o + n_mol_terms:]])[0] if full else None
        if not linear:
            return Jacobians(olr, dTs, own[0], dtau, mol, names, c.mu, c.weight,
                             temperatureSpectrum=T_rows.reshape(nl, n) if spectra else None, opticalDepthSpectrum=tau_rows,
                             temperatureAbsorption=dT_abs, emissivity=de, scatterers=dscat)
        lev_spec = self._levels_of_edges(T_rows.reshape(nl, 2, n).transpose(2, 0, 1)).T.copy() if spectra else None
        return Jacobians(olr, dTs, own[2] if chain is not None else None, dtau, mol, names, c.mu, c.weight,
                         opticalDepthSpectrum=tau_rows, temperatureAbsorption=dT_abs, emissivity=de,
                         edgeTemperature=own[0], levelTemperature=own[1], levelTemperatureSpectrum=lev_spec, scatterers=dscat)

    @staticmethod
    def _levels_of_edges(edge):
        """(..., L, 2) edge values (bottom, top per layer) -> (..., L + 1) level values: level i is the top edge of layer
        i - 1 plus the bottom edge of layer i"""
        lev = np.zeros(edge.shape[:-2] + (edge.shape[-2] + 1,))
        lev[..., :-1] += edge[..., :, 0]
        lev[..., 1:] += edge[..., :, 1]
        return lev

    def observeLinear(self, instrument, surfaceTemperature=None, surfaceSpectrum=None, mu=1.0, jacobians=False,
                      emissivity=None, levelTemperatures=None):
        """observe() for fluxes(planck="linear"): what an instrument above the column sees at viewing cosine ``mu`` with the
        Planck function linear in optical depth through every layer (lbl_column_flux_linear_dev and
        lbl_column_jacobian_linear_dev at the angle set [(mu, 1.0)]; beyond the reference).  Arguments as observe() takes
        them (``emissivity`` None is the black surface; with an emissivity the reflection is specular at ``mu``);
        ``levelTemperatures`` as fluxes(planck="linear") takes them.  The radiance is convolve(instrument,
        fluxes(planck="linear", angles=[(mu, 1.0)], ...).upSpectrum).  ``jacobians``: also opticalDepthJacobian (L, C) and
        ``levelTemperatureJacobian`` (L + 1, C), jacobiansLinear()'s spectral dI/d ln tau_l and edge rows for that angle
        convolved in the same call, the 2 L edge rows summed to levels on the host (the convolution is linear), and over a
        surface with an emissivity emissivityJacobian.  Returns an Observation whose temperatureJacobian is None.
        Everything is validated (ValueError) before the device is touched."""
        return self._observe(True, instrument, surfaceTemperature, surfaceSpectrum, mu, jacobians, emissivity, levelTemperatures)

    def _observe(self, linear, instrument, surfaceTemperature, surfaceSpectrum, mu, jacobians, emissivity,
                 levelTemperatures=None):
        """observe() and, with ``linear``, observeLinear()"""
        if not isinstance(instrument, Instrument):
            raise ValueError("instrument: an Instrument, not %r" % (instrument,))
        try:
            angle = [(float(mu), 1.0)]
        except (TypeError, ValueError):
            angle = None
        if angle is None or not (angle[0][0] > 0.0 and angle[0][0] <= 1.0):
            raise ValueError("mu: a viewing cosine in (0, 1], not %r" % (mu,))
        layers, n, mu_k, weight, band_first, band_count, surfaceSpectrum = self._column_checks(
            surfaceSpectrum, surfaceTemperature, angle, None)
        first = layers[0]
        edges = None
        if linear:
            lev = self._level_temperatures(levelTemperatures)
            edges = np.column_stack([lev[:-1], lev[1:]])
        black = emissivity is None
        if not black:
            emissivity = _surface_emissivity(emissivity, first.xAxis)
        support = instrument.support(first.rangeMin, first.rangeMax, n)
        nl, C = len(layers), len(instrument)
        w = 3 if linear else 2                       # a layer's rows: d ln tau and T, or d ln tau and the two edges' T
        n_rows = (1 + w * nl + (not black)) if jacobians else 1
        if n_rows > nat.limit("ils_rows"):           # behaviour, kept: the two methods work out "at most" differently
            most = (nat.limit("ils_rows") - 2) // 3 if linear else (nat.limit("ils_rows") - 1 - (not black)) // 2
            raise ValueError("jacobians: %d layers, at most %d" % (nl, most))
        ctx = _ctx()
        if jacobians and ctx.option("sweep_ieee_divisions"):
            raise ValueError("Jacobians exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)")
        kbufs, _ = self._column_abs_coef(ctx, layers, n)
        specular = REFLECTIONS.index("specular")
        src = dict(surface_T=float(surfaceTemperature or 0.0))
        fst = _kept_state(self, "_flux_state")       # behaviour, kept: the emissivity stands in fluxes()'s state
        fst.reserve(ctx, max(n, 2 * (nl + 1)))
        src["I_surface"] = fst.buf(ctx, "I_surface").upload(surfaceSpectrum) if surfaceSpectrum is not None else None
        up_top = fst.buf(ctx, "up_top")
        emissivity = self._device_emissivity(ctx, fst, emissivity)
        self._flux_call(ctx, layers, n, kbufs, edges, emissivity, specular, mu_k, weight, band_first, band_count,
                        fst.buf(ctx, "level"), up_top=up_top, **src)
        rows = [(up_top, 0)]
        if jacobians:
            jst = _kept_state(self, "_jacobian_out").reserve(ctx, max(n, 3 + w * nl))
            ln_tau_spec, T_spec = self._jacobian_spectra(ctx, linear, nl, n)
            e_spec = None if black else _kept_state(self, "_jacobian_surface").reserve(ctx, n).buf(ctx, "e_spec")
            self._jacobian_call(ctx, layers, n, kbufs, edges, emissivity, specular, mu_k, weight, band_first, band_count,
                                jst.buf(ctx, "jac"), T_spectra=T_spec, e_spectrum=e_spec, ln_tau_spectra=ln_tau_spec, **src)
            tau_rows, T_rows = [(ln_tau_spec, l * n) for l in range(nl)], [(T_spec, i * n) for i in range((w - 1) * nl)]
            # behaviour, kept: observe() hands the temperature rows to the convolution first, observeLinear() the edge rows last
            rows += tau_rows + T_rows if linear else T_rows + tau_rows
            if e_spec is not None:
                rows.append((e_spec, 0))
        out = _kept_state(self, "_observe_out").reserve(ctx, n_rows * C).buf(ctx, "out")
        _ils_convolve(ctx, instrument, first.rangeMin, first.rangeMax, n, support, rows, out)
        v = out.download(n_rows * C).reshape(n_rows, C)
        e_row = v[1 + w * nl].copy() if jacobians and not black else None
        if not linear:
            return Observation(instrument.centres.copy(), v[0].copy(), float(mu_k[0]),
                               temperatureJacobian=v[1:1 + nl].copy() if jacobians else None,
                               opticalDepthJacobian=v[1 + nl:1 + 2 * nl].copy() if jacobians else None, emissivityJacobian=e_row)
        dlev = None
        if jacobians:
            dlev = self._levels_of_edges(v[1 + nl:1 + 3 * nl].reshape(nl, 2, C).transpose(2, 0, 1)).T.copy()
        return Observation(instrument.centres.copy(), v[0].copy(), float(mu_k[0]),
                           opticalDepthJacobian=v[1:1 + nl].copy() if jacobians else None, emissivityJacobian=e_row,
                           levelTemperatureJacobian=dlev)

    @staticmethod
    def _path_mu(mu):
        try:
            mu = float(mu)
        except (TypeError, ValueError):
            raise ValueError("mu: a cosine in (0, 1], not %r" % (mu,))
        if not (mu > 0.0 and mu <= 1.0):
            raise ValueError("mu: a cosine in (0, 1], not %r" % (mu,))
        return mu

    def _path_level(self, observerLevel, default):
        nl = len(self._column_layers()[0])
        if observerLevel is None:
            observerLevel = default if default is not None else nl
        if isinstance(observerLevel, bool) or not isinstance(observerLevel, (int, np.integer)) or not 0 <= observerLevel <= nl:
            raise ValueError("observerLevel: a level 0..%d (0 the surface), not %r" % (nl, observerLevel))
        return int(observerLevel), nl

    def levelTemperatures(self):
        """The default temperatures of the L + 1 levels for planck="linear": linear in height between the layers'
        midpoints, where a layer has its own temperature,
            lev_i = T_(i-1) + (T_i - T_(i-1)) depth_(i-1) / (depth_(i-1) + depth_i)        0 < i < L
        and at both ends such that the layer's temperature is the mean of its two levels: lev_0 = 2 T_0 - lev_1, lev_L =
        2 T_(L-1) - lev_(L-1).  One layer: both levels are T_0.  ValueError if a level comes out <= 0."""
        layers, _ = self._column_layers()
        T = [float(L.T) for L in layers]
        d = [float(L.depth) for L in layers]
        nl = len(layers)
        lev = np.empty(nl + 1)
        if nl == 1:
            lev[:] = T[0]
        else:
            for i in range(1, nl):
                lev[i] = T[i - 1] + (T[i] - T[i - 1]) * d[i - 1] / (d[i - 1] + d[i])
            lev[0] = 2.0 * T[0] - lev[1]
            lev[nl] = 2.0 * T[nl - 1] - lev[nl - 1]
        if not np.all(np.isfinite(lev) & (lev > 0.0)):
            raise ValueError("levelTemperatures: the default level temperatures %r are not all finite and > 0; give "
                             "levelTemperatures" % (lev.tolist(),))
        return lev

    def _level_temperatures(self, levelTemperatures):
        """``levelTemperatures`` as L + 1 float64 values: None or True the default ones, else L + 1 numbers, finite, > 0"""
        if levelTemperatures is None or levelTemperatures is True:
            return self.levelTemperatures()
        nl = len(self._column_layers()[0])
        try:
            lev = np.array(levelTemperatures, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("levelTemperatures: %d numbers, one per level" % (nl + 1))
        if isinstance(levelTemperatures, (bool, str)) or lev.shape != (nl + 1,):
            raise ValueError("levelTemperatures: %d numbers, one per level (level 0 the surface), not %r"
                             % (nl + 1, levelTemperatures))
        if not np.all(np.isfinite(lev) & (lev > 0.0)):
            raise ValueError("levelTemperatures must be finite and > 0")
        return lev

    def _path_temperatures(self, levelTemperatures, crossings):
        """None without level temperatures, else the (Ta, Tb) of every crossing (layer, upward?) of whole layers"""
        if levelTemperatures is None:
            return None
        lev = self._level_temperatures(levelTemperatures)
        return [(lev[l], lev[l + 1]) if up else (lev[l + 1], lev[l]) for l, up in crossings]

    def nadirPath(self, mu=1.0, observerLevel=None, levelTemperatures=None):
        """The Path of an observer at level ``observerLevel`` (None: the top, level L) looking down at cosine ``mu``: the
        surface source, then the layers 0 .. observerLevel-1 upward, each over depth_l / mu.  ``levelTemperatures``: None,
        or L + 1 level temperatures (True: levelTemperatures()) - the path then carries every segment's temperatures in the
        direction of travel, for radiance(planck="linear")."""
        mu = self._path_mu(mu)
        lev, _ = self._path_level(observerLevel, None)
        return Path(range(lev), [self[l].depth / mu for l in range(lev)], "surface", "nadir mu=%g level=%d" % (mu, lev),
                    temperatures=self._path_temperatures(levelTemperatures, [(l, True) for l in range(lev)]))

    def zenithPath(self, mu=1.0, observerLevel=0, levelTemperatures=None):
        """The Path of an upward-looking observer at level ``observerLevel`` (0: the surface) at cosine ``mu``: cold space,
        then the layers L-1 down to observerLevel, each over depth_l / mu - the downwelling radiance an instrument there
        measures.  ``levelTemperatures``: as nadirPath takes them (every segment enters at its layer's upper level)."""
        mu = self._path_mu(mu)
        lev, nl = self._path_level(observerLevel, 0)
        lay = range(nl - 1, lev - 1, -1)
        return Path(lay, [self[l].depth / mu for l in lay], "space", "zenith mu=%g level=%d" % (mu, lev),
                    temperatures=self._path_temperatures(levelTemperatures, [(l, False) for l in lay]))

    def reflectedPath(self, mu=1.0, observerLevel=None, levelTemperatures=None):
        """The Path of nadirPath's observer together with its mirror path: cold space, the layers L-1 .. 0 downward, the
        surface (bounce = L), then the layers 0 .. observerLevel-1 upward, each over depth_l / mu - what a surface that
        reflects specularly sends to the observer (radiance() with an emissivity).  ``levelTemperatures``: as nadirPath
        takes them (downward segments enter at the upper level, upward ones at the lower)."""
        mu = self._path_mu(mu)
        lev, nl = self._path_level(observerLevel, None)
        lay = list(range(nl - 1, -1, -1)) + list(range(lev))
        return Path(lay, [self[l].depth / mu for l in lay], "space", "reflected mu=%g level=%d" % (mu, lev), bounce=nl,
                    temperatures=self._path_temperatures(levelTemperatures, [(l, False) for l in range(nl - 1, -1, -1)]
                                                         + [(l, True) for l in range(lev)]))

    def limbPath(self, tangentHeight, planetRadius=6.371e8, levelTemperatures=None):
        """The Path of a limb ray through the column taken as spherical shells around a planet of radius ``planetRadius``
        (cm; level heights z_0 = 0, z_(l+1) = z_l + depth_l): it enters from space, comes down to ``tangentHeight`` (cm above
        the surface, 0 <= tangentHeight < z_L) and leaves again towards an observer outside the atmosphere.  NO REFRACTION:
        the ray is a straight line.  With zt the tangent height and m the tangent layer (z_m <= zt < z_(m+1)), the half
        chord inside layer l >= m is, with lo = max(z_l, zt) and hi = z_(l+1),
            sqrt((hi - zt) (2 R + hi + zt)) - sqrt((lo - zt) (2 R + lo + zt))
        (the factored form of sqrt((R + hi)^2 - (R + zt)^2) - ..., which keeps its digits near the top).  Segments: the
        layers L-1 .. m+1 with their half chords, layer m once with twice its half chord, then m+1 .. L-1.
        ``levelTemperatures``: as nadirPath takes them; the tangent layer is then crossed in two segments of one half chord
        each, which meet at T(zt) = lev_m + (lev_(m+1) - lev_m) (zt - z_m) / depth_m."""
        layers, _ = self._column_layers()
        try:
            zt, R = float(tangentHeight), float(planetRadius)
        except (TypeError, ValueError):
            raise ValueError("tangentHeight and planetRadius: heights in cm")
        if not R > 0.0 or R == float("inf"):
            raise ValueError("planetRadius must be finite and > 0, not %r" % (planetRadius,))
        z = [0.0]
        for L in layers:
            z.append(z[-1] + float(L.depth))
        if not (zt >= 0.0 and zt < z[-1]):
            raise ValueError("tangentHeight: %r is outside [0, %r), the column's heights (rays that meet the surface are "
                             "not limb paths)" % (tangentHeight, z[-1]))
        nl = len(layers)
        m = max(l for l in range(nl) if z[l] <= zt)        # (zt < z_L: the layer above level m is not empty)
        reach = lambda h: math.sqrt((h - zt) * (2.0 * R + h + zt))
        half = {l: reach(z[l + 1]) - reach(max(z[l], zt)) for l in range(m, nl)}
        above = list(range(nl - 1, m, -1))
        if levelTemperatures is not None:
            lev = self._level_temperatures(levelTemperatures)
            Tt = lev[m] + (lev[m + 1] - lev[m]) * (zt - z[m]) / float(layers[m].depth)
            lay = above + [m, m] + above[::-1]
            return Path(lay, [half[l] for l in lay], "space", "limb zt=%g" % zt,
                        temperatures=[(lev[l + 1], lev[l]) for l in above] + [(lev[m + 1], Tt), (Tt, lev[m + 1])]
                                     + [(lev[l], lev[l + 1]) for l in above[::-1]])
        lay = above + [m] + above[::-1]
        return Path(lay, [half[l] for l in above] + [2.0 * half[m]] + [half[l] for l in above[::-1]], "space",
                    "limb zt=%g" % zt)

    def _path_checks(self, paths, surfaceTemperature, surfaceSpectrum):
        """The checks radiance() and pathJacobians() share, before the device is touched: (the paths as a list, layers,
        n, surfaceSpectrum as n float64 values or None)."""
        plist = [paths] if isinstance(paths, Path) else list(paths) if isinstance(paths, (list, tuple)) else None
        if not plist or not all(isinstance(p, Path) for p in plist):
            raise ValueError("paths: a Path or a non-empty list of them, not %r" % (paths,))
        R = len(plist)
        if R > nat.limit("ray_paths"):
            raise ValueError("paths: %d paths, at most %d in one call" % (R, nat.limit("ray_paths")))
        layers, n = self._column_layers()
        nl = len(layers)
        for i, p in enumerate(plist):
            if any(l >= nl for l in p.layers):
                raise ValueError("paths: path %d names layer %d, the column has %d" % (i, max(p.layers), nl))
        if sum(len(p) for p in plist) > nat.limit("ray_segments"):
            raise ValueError("paths: %d segments, at most %d in one call" % (sum(len(p) for p in plist), nat.limit("ray_segments")))
        if any(p.source == "surface" or p.bounce is not None for p in plist):
            if surfaceSpectrum is None and surfaceTemperature is None:
                raise ValueError("a path starts at the surface or meets it: give surfaceSpectrum or surfaceTemperature")
            if surfaceSpectrum is None and not float(surfaceTemperature) > 0:
                raise ValueError("surfaceTemperature must be > 0")
        return plist, layers, n, _grid_spectrum("surfaceSpectrum", surfaceSpectrum, n)

    def radiance(self, paths, surfaceTemperature=None, surfaceSpectrum=None, instrument=None, transmittance=False,
                 emissivity=None, reflection="lambertian", angles=3, planck="layer", levelTemperatures=None):
        """The radiance arriving along ``paths`` - one Path or a list of up to 512 - through this column (beyond the
        reference).  Layers, grid and units as transmission() has them.  For every path and grid point nu_j:
            I = surfaceSpectrum[j] or B(nu_j, surfaceTemperature) for source "surface", 0 for "space";  Ttot = 1
            per segment (layer l, length s), in order:   t = exp(-k_l(nu_j) s)   I <- t I + (1 - t) B(nu_j, T_l)   Ttot <- Ttot t
        A surface source is needed only if some path starts at the surface.  ``transmittance``: also return Ttot.
        ``instrument``: an Instrument - the rows are convolved onto its channels on the device, as observe() does, and
        only channel values come down (with transmittance twice the paths must fit the 512 rows of one convolution).
        radiance(nadirPath()) is transmission() bit for bit wherever fluxes() documents that identity, and with an
        instrument observe(instrument).radiance.  One kernel call (lbl_ray_radiance_dev) for all paths; a path's result does
        not depend on the others.  The absorption coefficients are the resident ones: after transmission() nothing is
        accumulated again.  Returns a PathRadiance.  Everything is validated (ValueError) before the device is touched.

        ``emissivity``: None, the black surface above, or the surface's emissivity e as fluxes() takes it; the call then goes
        through lbl_ray_radiance_surface_dev.  With Is the surface source above:
          - a path with a bounce (reflectedPath) is reflected specularly where it meets the surface, whatever ``reflection``:
                I <- e Is + (1 - e) I        Ttot <- Ttot (1 - e)
          - a path that starts at the surface starts with I = e Is + (1 - e) Rd.  "lambertian": Rd = F_down / sum_k W_k, the
            diffuse reflection of the downward flux at the surface that one fluxes() pass with ``angles`` (see fluxAngles)
            and cold space above leaves on the device - nothing comes down in between.  "specular": Rd = 0, the path carries
            e Is alone and the reflected light belongs to the paths with a bounce.
        With emissivity 1 every result is the black surface's bit for bit.  A path with a bounce needs an emissivity.

        ``planck``: "layer", the isothermal segments above, or "linear" - every path must then carry ``temperatures``, one
        pair (Ta, Tb) per segment (the path builders fill them from ``levelTemperatures``), and per segment
            I <- t I + (1 - t) B(nu_j, Ta) + g(tau) (B(nu_j, Tb) - B(nu_j, Ta))      tau = k_l s, g(tau) = 1 - (1 - t) / tau
        as fluxes(planck="linear") steps through a layer (lbl_ray_radiance_linear_dev).  Instrument, transmittance,
        emissivity and bounces work as above; the Lambertian start term then comes from one linear-source flux pass with
        ``levelTemperatures`` (L + 1 numbers; None: levelTemperatures()), which stays on the device as well."""
        plist, layers, n, surfaceSpectrum = self._path_checks(paths, surfaceTemperature, surfaceSpectrum)
        R, nl = len(plist), len(layers)
        first = layers[0]
        refl = _surface_reflection(reflection)
        linear = _planck_source(planck, levelTemperatures)
        edges = None
        if linear:
            for i, p in enumerate(plist):
                if p.temperatures is None:
                    raise ValueError("planck=\"linear\": path %d (%r) carries no temperatures" % (i, p))
            if levelTemperatures is not None or (emissivity is not None and refl == 0
                                                 and any(p.source == "surface" for p in plist)):
                lev = self._level_temperatures(levelTemperatures)
                edges = np.column_stack([lev[:-1], lev[1:]])
        if emissivity is None:
            if any(p.bounce is not None for p in plist):
                raise ValueError("a path with a bounce needs a surface that reflects: give emissivity")
        else:
            emissivity = _surface_emissivity(emissivity, first.xAxis)
            mu, weight = fluxAngles(angles)
            wsum = _weight_sum(weight)
        n_rows = 2 * R if transmittance else R
        support = None
        if instrument is not None:
            if not isinstance(instrument, Instrument):
                raise ValueError("instrument: an Instrument, not %r" % (instrument,))
            if n_rows > nat.limit("ils_rows"):
                raise ValueError("instrument: %d paths with transmittance are %d rows, at most %d in one convolution"
                                 % (R, n_rows, nat.limit("ils_rows")))
            support = instrument.support(first.rangeMin, first.rangeMax, n)
        ctx = _ctx()
        if ctx.option("sweep_ieee_divisions"):
            raise ValueError("ray paths exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)")
        kbufs, _ = self._column_abs_coef(ctx, layers, n)
        I_source = None
        if surfaceSpectrum is not None:
            I_source = _kept_state(self, "_path_source").reserve(ctx, n).buf(ctx, "I_source").upload(surfaceSpectrum)
        pst = _kept_state(self, "_path_state").reserve(ctx, R * n)
        rad = pst.buf(ctx, "radiance")
        trn = pst.buf(ctx, "transmittance") if transmittance else None
        down, norm = None, 0.0
        if emissivity is not None:
            sst = _kept_state(self, "_path_surface").reserve(ctx, max(n, 2 * (nl + 1)))
            emissivity = self._device_emissivity(ctx, sst, emissivity)
            if refl == 0 and any(p.source == "surface" for p in plist):
                # the downward flux at the surface under cold space, left on the device for the ray call behind it
                down, norm = sst.buf(ctx, "down_surface"), wsum
                self._flux_call(ctx, layers, n, kbufs, edges, None, 0, mu, weight, [0], [n], sst.buf(ctx, "level"),
                                I_surface=I_source, surface_T=float(surfaceTemperature or 0.0), down_surface=down)
        self._ray_radiance_call(ctx, layers, n, kbufs, plist, linear, emissivity, rad, surface_down=down, surface_down_norm=norm,
                                I_source=I_source, source_T=float(surfaceTemperature or 0.0), transmittance=trn)
        if instrument is None:
            return PathRadiance(first.xAxis, rad.download(R * n).reshape(R, n),
                                trn.download(R * n).reshape(R, n) if transmittance else None, plist)
        C = len(instrument)
        out = _kept_state(self, "_path_out").reserve(ctx, n_rows * C).buf(ctx, "out")
        rows = [(rad, r * n) for r in range(R)] + ([(trn, r * n) for r in range(R)] if transmittance else [])
        _ils_convolve(ctx, instrument, first.rangeMin, first.rangeMax, n, support, rows, out)
        v = out.download(n_rows * C).reshape(n_rows, C)
        return PathRadiance(instrument.centres.copy(), v[:R].copy(), v[R:].copy() if transmittance else None, plist)

    def pathJacobians(self, paths, surfaceTemperature=None, surfaceSpectrum=None, instrument=None, molecules=False,
                      temperature="planck", emissivity=None, reflection="lambertian"):
        """The weighting functions of radiance(): analytic derivatives of the radiance arriving along ``paths`` - one Path or
        a list of up to 512 - per path and grid point (beyond the reference), in one pass over the resident absorption
        coefficients per chunk of paths.  Paths, sources, layers, grid and units as radiance() has them.  For a path with
        the segments s (layer l_s, length x_s), I_s the radiance entering segment s, t_s = exp(-k_l(nu_j) x_s) and A_s the
        product of t_i over the segments after s:
            dI/d ln tau_l       = sum over the path's segments in layer l of k_l x_s A_s t_s (B_l - I_s)
            dI/d ln n_(m,l)     = the same sum with k_(m,l), molecule m's own absorption coefficient (fixed line shapes)
            dI/dT_l (Planck)    = sum over the same segments of A_s (1 - t_s) dB_l/dT
            dI/dT_l (absorption)= the same sum as dI/d ln tau_l with dk_l/dT for k_l         temperature="full" only
            dI/dT_s             = (product of all t_s) dB(nu_j, T_s)/dT       paths from a surface at surfaceTemperature
        as jacobians() defines the same quantities for the flux.  ``molecules``: also the molecule terms (jacobians()'s,
        kept with the atmosphere).  ``temperature``: "planck" or "full", as in jacobians() (the Voigt line shape only).
        ``instrument``: an Instrument - every row is convolved onto its channels on the device, as observe() does, and only
        channel values come down.  Returns a PathJacobians; its radiance is radiance()'s bit for bit.  A path's result does
        not depend on the others.  Chunks: as many whole paths, in order, as keep the rows of one kernel call
        (lbl_ray_jacobian_dev: 1 + 2 crossed layers + terms in crossed layers, per path) at or below the 512 rows of one
        convolution, one path at least, so the device work space never exceeds max(512, one path's rows) x n doubles
        whatever the number of paths.  The absorption coefficients are the resident ones: after transmission() nothing is
        accumulated again.  No other result of the model changes.  Everything is validated (ValueError) before the device
        is touched.

        ``emissivity``: None, the black surface above, or the surface's emissivity e as radiance() takes it: the weighting
        functions of radiance(paths, emissivity=e, reflection=...), whose radiance comes back bit for bit
        (lbl_ray_jacobian_surface_dev, one more row per path).  Paths with a bounce are then accepted (without an
        emissivity they are refused).  With "element" for a segment or the bounce, and A the product over every element
        after one of t_s for segments and 1 - e for the bounce (A_0: over the whole path):
            dI/d ln tau_l, dI/dT_l, molecules: the sums above with that A
            dI/dT_s  = e dB(nu_j, T_s)/dT (A at the bounce + A_0 for a path from the surface)
            dI/de    = A at the bounce (Is - the radiance arriving there) + A_0 Is for a path from the surface
        PathJacobians.emissivity holds dI/de.  A path that STARTS at the surface carries, under reflection="lambertian", the
        diffusely reflected sky, which depends on every layer of the column; that derivative is not built, and holding the
        sky fixed would disagree with differences of radiance(): such a path is refused (ValueError) with an emissivity
        and "lambertian" - take reflection="specular", under which it starts with e Is alone.
        The Planck source is the layer source: one temperature per layer (fluxes() and radiance() also take
        planck="linear"; its derivatives are pathJacobiansLinear()'s)."""
        return self._path_jacobians(False, paths, surfaceTemperature, surfaceSpectrum, instrument, molecules, temperature,
                                    emissivity, reflection)

    def pathJacobiansLinear(self, paths, surfaceTemperature=None, surfaceSpectrum=None, instrument=None, molecules=False,
                            temperature="planck", emissivity=None, reflection="lambertian"):
        """pathJacobians() for radiance(planck="linear"): the weighting functions of the radiance along ``paths`` with the
        Planck function linear in optical depth through every segment (lbl_ray_jacobian_linear_dev; beyond the reference).
        Every path must carry ``temperatures`` (the path builders fill them from levelTemperatures=...).  Arguments, chunks,
        instrument and refusals are pathJacobians()'s; ``emissivity`` None is the black surface.  Per segment s (layer l,
        length x, tau = k_l x, t = exp(-tau), Ba = B(Ta_s) where the light enters, Bb = B(Tb_s) where it leaves, I_s the
        radiance entering, A_s the product over every element after s), with g as radiance() has it, h = (1 - t) - g and
        g' = h / tau:
            dI/d ln tau_l    = sum over the path's segments in layer l of A_s [tau t (Ba - I_s) + h (Bb - Ba)]
            molecules, dk/dT = the same sums with k_m x [t (Ba - I_s) + g' (Bb - Ba)]
            dI/dTa_s = A_s h dB(Ta_s)/dT        dI/dTb_s = A_s g dB(Tb_s)/dT           per segment, not per layer
            dI/dT_s, dI/de   : pathJacobians()'s
        Returns a PathJacobians whose ``segmentTemperature`` holds, per path, an (s, 2, X) array of (dI/dTa, dI/dTb) for
        its s segments in order of travel (the bounce is no segment); a path's rows in one kernel call are 2 + crossed
        layers + 2 s + terms.  The per-layer ``temperature`` is None: which level a segment end belongs to is known only to
        whoever built the path (for the built-in builders, a level's derivative is the sum of the rows of the segment ends
        that lie on it).  temperature="full" fills temperatureAbsorption.  The radiance is radiance(planck="linear")'s
        bit for bit."""
        return self._path_jacobians(True, paths, surfaceTemperature, surfaceSpectrum, instrument, molecules, temperature,
                                    emissivity, reflection)

    def _path_jacobians(self, linear, paths, surfaceTemperature, surfaceSpectrum, instrument, molecules, temperature,
                        emissivity, reflection):
        """pathJacobians() and, with ``linear``, pathJacobiansLinear()"""
        if temperature not in ("planck", "full"):
            raise ValueError("temperature: \"planck\" or \"full\", not %r" % (temperature,))
        plist, layers, n, surfaceSpectrum = self._path_checks(paths, surfaceTemperature, surfaceSpectrum)
        R, nl = len(plist), len(layers)
        first = layers[0]
        refl = _surface_reflection(reflection)
        if emissivity is None:
            if any(p.bounce is not None for p in plist):
                raise ValueError("paths: a path with a bounce needs a surface that reflects: give emissivity")
        else:
            emissivity = _surface_emissivity(emissivity, first.xAxis)
            if refl == 0 and any(p.source == "surface" for p in plist):
                raise ValueError("reflection: a path that starts at the surface has no weighting functions under \"lambertian\" "
                                 "(the diffusely reflected sky is not differentiated); take reflection=\"specular\"")
        if linear:
            for i, p in enumerate(plist):
                if p.temperatures is None:
                    raise ValueError("paths: path %d (%r) carries no temperatures (the linear source needs a pair per segment)"
                                     % (i, p))
        black = emissivity is None
        h = 1 if black and not linear else 2          # a path's rows ahead of its layers': dI/dT_s and (not the black call's) dI/de
        full = temperature == "full"
        names = [[m.name for m in L] for L in layers]
        n_terms = self._term_count(layers, molecules, full, full)
        n_mol_terms = n_terms - (nl if full else 0)
        support = None
        if instrument is not None:
            if not isinstance(instrument, Instrument):
                raise ValueError("instrument: an Instrument, not %r" % (instrument,))
            support = instrument.support(first.rangeMin, first.rangeMax, n)
        # the terms' layers (molecules layer by layer as _jacobian_terms lists them, then dk_l/dT), and every path's rows
        term_layer = ([l for l, L in enumerate(layers) for _ in L] if molecules else []) + (list(range(nl)) if full else [])
        crossed = [sorted(set(p.layers)) for p in plist]
        ray_terms = [[t for t, l in enumerate(term_layer) if l in set(c)] for c in crossed]
        ray_rows = [h + (len(c) + 2 * len(p) if linear else 2 * len(c)) + len(t) for p, c, t in zip(plist, crossed, ray_terms)]
        block = nat.limit("ils_rows")
        chunks, r = [], 0
        while r < R:
            e, rows = r + 1, ray_rows[r]
            while e < R and rows + ray_rows[e] <= block:
                rows += ray_rows[e]
                e += 1
            chunks.append((r, e, rows))
            r = e
        ctx = _ctx()
        if ctx.option("sweep_ieee_divisions"):
            raise ValueError("Jacobians exist in the sweeps' default arithmetic only (\"sweep_ieee_divisions\" 0)")
        kbufs, plan = self._column_abs_coef(ctx, layers, n)
        term_bufs = self._term_buffers(ctx, layers, n, plan, molecules, full)[0]
        I_source = None
        if surfaceSpectrum is not None:
            I_source = _kept_state(self, "_path_source").reserve(ctx, n).buf(ctx, "I_source").upload(surfaceSpectrum)
        if emissivity is not None and not isinstance(emissivity, float):
            emissivity = _kept_state(self, "_path_surface").reserve(ctx, max(n, 2 * (nl + 1))).buf(ctx, "emissivity").upload(emissivity)
        jac = _kept_state(self, "_path_jacobian_rows").reserve(ctx, max(c[2] for c in chunks) * n).buf(ctx, "jac")
        rad = _kept_state(self, "_path_jacobian_radiance").reserve(ctx, max(e - r for r, e, _ in chunks) * n).buf(ctx, "radiance")
        X = n if instrument is None else len(instrument)
        total = sum(ray_rows)
        if instrument is not None:
            cst = _kept_state(self, "_path_jacobian_block").reserve(ctx, block * X)
            out = _kept_state(self, "_path_jacobian_out").reserve(ctx, (R + total) * X).buf(ctx, "out")
        I = np.empty((R, X))
        J = np.empty((total, X))
        row0 = 0
        for r, e, rows in chunks:
            self._ray_jacobian_call(ctx, layers, n, kbufs, plist[r:e], linear, emissivity, jac, I_source=I_source,
                                    source_T=float(surfaceTemperature or 0.0), term_abs_coef=term_bufs, term_layer=term_layer,
                                    radiance=rad)
            if instrument is None:
                I[r:e] = rad.download((e - r) * n).reshape(e - r, n)
                J[row0:row0 + rows] = jac.download(rows * n).reshape(rows, n)
            else:          # the radiances, then the rows in blocks of one convolution, gathered behind one another in `out`
                todo = [(rad, i * n, r + i) for i in range(e - r)] + [(jac, i * n, R + row0 + i) for i in range(rows)]
                for b in range(0, len(todo), block):
                    part = todo[b:b + block]
                    _ils_convolve(ctx, instrument, first.rangeMin, first.rangeMax, n, support, [(buf, o) for buf, o, _ in part],
                                  cst.buf(ctx, "block"))
                    at = 0
                    while at < len(part):          # (runs of consecutive output rows: one copy each)
                        end = at + 1
                        while end < len(part) and part[end][2] == part[end - 1][2] + 1:
                            end += 1
                        out.stage_from_dev(cst.buf(ctx, "block"), at * X, (end - at) * X, dst_offset=part[at][2] * X)
                        at = end
            row0 += rows
        if instrument is not None:
            v = out.download((R + total) * X).reshape(R + total, X)
            I, J = v[:R].copy(), v[R:]
        # rows -> (R, L, X) arrays: zeros where a path does not cross a layer
        dtau, dT = np.zeros((R, nl, X)), None if linear else np.zeros((R, nl, X))
        dTs = np.zeros((R, X))
        de = None if black else np.zeros((R, X))
        terms = np.zeros((R, n_terms, X))
        seg_T = [] if linear else None
        row0 = 0
        for r in range(R):
            c = len(crossed[r])
            dTs[r] = J[row0]
            if de is not None:
                de[r] = J[row0 + 1]
            dtau[r, crossed[r]] = J[row0 + h:row0 + h + c]
            if linear:
                ns = len(plist[r])
                seg_T.append(J[row0 + h + c:row0 + h + c + 2 * ns].reshape(ns, 2, X).copy())
                terms[r, ray_terms[r]] = J[row0 + h + c + 2 * ns:row0 + ray_rows[r]]
            else:
                dT[r, crossed[r]] = J[row0 + h + c:row0 + h + 2 * c]
                terms[r, ray_terms[r]] = J[row0 + h + 2 * c:row0 + ray_rows[r]]
            row0 += ray_rows[r]
        mol = None
        if molecules:
            mol, o = [], 0
            for L in layers:
                mol.append(terms[:, o:o + len(L)].copy())
                o += len(L)
        return PathJacobians(first.xAxis if instrument is None else instrument.centres.copy(), I, dT, dtau,
                             dTs if surfaceSpectrum is None else None, mol, names, plist,
                             temperatureAbsorption=terms[:, n_mol_terms:].copy() if full else None,
                             channels=instrument is not None, emissivity=de, segmentTemperature=seg_T)

    def kDistribution(self, bands=None, g=16, reference=None, planck=False, spectra=False):
        """k-distributions of the column's bands (beyond the reference): every layer's absorption coefficient (getAbsCoef)
        ranked in every band and averaged over g intervals on the device, as kDistribution() defines it, with one row per
        layer in list order.  reference=None ranks every layer by itself; reference=r averages every layer over the point
        sets of layer r's order (the mapped distribution: one sort and L gathers).  ``planck``: also the mean of
        planckWavenumber(nu, T_l) over the same point sets, KDistribution.planck.  ``spectra``: also the order and the sorted
        coefficients.  The absorption coefficients are the resident ones: after transmission() or fluxes() nothing is
        accumulated again.  Everything is validated (ValueError) before the device is touched."""
        layers, n = self._column_layers()
        first_layer = layers[0]
        first, count, edges = _kdist_checks(first_layer.rangeMin, first_layer.rangeMax, n, len(layers), bands, g, reference)
        ctx = _ctx()
        kbufs, _ = self._column_abs_coef(ctx, layers, n)
        keep = self.__dict__.get("_kdist_state")
        if keep is None:
            keep = self.__dict__["_kdist_state"] = _KdistBuffers(self)
        return _kdist_run(ctx, keep, n, [(b, 0) for b in kbufs], first, count, edges, reference, bool(spectra), bands,
                          planck=(first_layer.rangeMin, first_layer.rangeMax, [L.T for L in layers]) if planck else None)

    def _jacobian_terms(self, ctx, layers, n, plan):
        """The molecule terms of jacobians(): every molecule's own absorption coefficient k_(m,l), as (buffers, layer index
        of each).  In a layer that is one merged job (``plan`` of _resident_abs_coef) a molecule gets ONE merged accumulate
        job over its own line lists (its volume fraction, iso_mol all 0) into a buffer of the atmosphere's Jacobian state,
        keyed like the layer's (_merged_key): it is recomputed only when that molecule's inputs change, and all due
        molecules go in one launch sequence.  Exotic molecules, molecules without line lists and layers that are no merged
        job use the molecule's own route (Molecule._ensure_swept)."""
        terms = self.__dict__.setdefault("_jacobian_term_states", {})
        bufs, where, todo, keys, keep = [], [], [], [], set()
        for l, L in enumerate(layers):
            members, conc = L._sweep_members()
            merged = plan is not None and plan[l][6] is not None
            g = L._grid() if merged else None
            for mi, m in enumerate(L):
                isos = members[mi]
                if not merged or not isos or m.exotic:
                    bufs.append(m._ensure_swept()[0].bufs["abs_coef"])
                    where.append(l)
                    continue
                tk = (id(L), id(m))
                keep.add(tk)
                st = terms.get(tk)
                if st is None:
                    st = terms[tk] = _SweepState(self)
                st.reserve(ctx, n)
                key = L._merged_key(isos, [conc[mi]], L, g)[:-1]          # (the depth does not enter k)
                if st.key != key:
                    todo.append(dict(lines=[i._device_lines(ctx) for i in isos], iso=[_iso_params(i) for i in isos],
                                     grid=_engine.native_grid(g), iso_mol=[0] * len(isos), conc=[conc[mi]],
                                     abs_coef=st.buf(ctx, "abs_coef")))
                    keys.append((st, key))
                bufs.append(st.buf(ctx, "abs_coef"))
                where.append(l)
        for tk in [t for t in terms if t not in keep]:
            _free_buffers(terms.pop(tk).bufs)
        if todo:
            ctx.layers_merged_accumulate_dev(todo)
            for st, key in keys:
                st.key = key
        return bufs, where

    def _transmission_merged(self, ctx, layers, n, surfaceSpectrum, surfaceTemperature):
        """settings.LAYER_STEP "merged": every layer whose inputs changed gets ONE accumulate job over its merged,
        factor-weighted line lists, all of them in one launch sequence (lbl_layers_merged_accumulate_dev: the layers'
        absorption coefficients, cls:707-712), then one pass folds transmittance and emission bottom to top over those
        arrays (lbl_column_fold_dev, cls:714-716, 784-787) and leaves every layer's transmittance resident for its own
        getters.  A layer that cannot be a merged job (no line list, a measured cross-section table among its molecules, more
        line lists than a job takes, an installed cross section) brings its absorption coefficient by its own route
        (_ensure_swept) and is folded with the others.  None only when settings.LAYER_STEP is not "merged": the caller then
        goes through the per-line-list cross sections of the whole column (lbl_column_step_dev)."""
        if not _merged_route(ctx):
            return None
        fast = self._transmission_resident(ctx, layers, n, surfaceSpectrum, surfaceTemperature)
        if fast is not None:
            return fast
        plan = self._resident_abs_coef(ctx, layers, n)
        # (the outgoing spectrum's buffer stays with the atmosphere: a hipMalloc + hipFree pair per call is 0.2 ms of a 5 ms call)
        ast = _kept_state(self, "_toa_state")
        out = ast.reserve(ctx, n).buf(ctx, "toa")
        I_in = None
        if surfaceSpectrum is not None:
            I_in = ast.buf(ctx, "I_in").upload(np.ascontiguousarray(surfaceSpectrum, dtype=np.float64))
        first = layers[0]
        # The fold in four pieces of the grid, each piece's part of the outgoing spectrum on its way to the host while the
        # next piece is folded (19 MB at the link's rate are 0.4 ms of a 5 ms call).  No layer's transmittance is written
        # (30 x 19 MB for arrays nobody has asked for): a layer's own getter makes it from the resident absorption
        # coefficient, as after changeDepth (_ensure_swept: key equal up to its last entry).
        host = ctx.host_array(n)
        pieces = 4 if n >= (1 << 16) else 1
        step = max(((n + pieces - 1) // pieces + 3) & ~3, 4)
        try:
            for lo in range(0, n, step):
                cnt = min(step, n - lo)
                ctx.column_fold_dev([p[1].bufs["abs_coef"] for p in plan], [p[0].T for p in plan], [p[0].depth for p in plan],
                                    first.rangeMin, first.rangeMax, n, out, I_in=I_in, surface_T=float(surfaceTemperature or 0.0),
                                    first=lo, count=cnt)
                out.download_async(host, cnt, lo, lo)
        finally:
            # (also when a piece raised: copies into `host` may be in flight, and its page-locked block must not go back to
            # the pool before they have landed - advisor, round 5)
            ctx.download_wait()
        self._column_remember(ctx, layers, n, plan)
        return host

    def _resident_abs_coef(self, ctx, layers, n):
        """settings.LAYER_STEP "merged": make every layer's absorption coefficient resident on the device
        (_SweepState.bufs["abs_coef"]) and return the plan [(layer, state, grid, members, flat, conc, merged key or None)].
        The layers whose inputs changed get ONE accumulate job each over their merged, factor-weighted line lists, all of
        them in one launch sequence (lbl_layers_merged_accumulate_dev: cls:707-712); a layer that cannot be a merged job
        (no line list, a measured cross-section table among its molecules, more line lists than a job takes, an installed
        cross section) brings its absorption coefficient by its own route (_ensure_swept).  Shared by transmission() and
        fluxes(): after either, the other enqueues no accumulate job for unchanged layers."""
        plan = []
        for L in layers:
            members, conc = L._sweep_members()
            flat = [iso for isos in members for iso in isos]
            g = L._grid()
            if (not flat or any(i.exotic for i in flat) or len(flat) > nat.limit("merged_lists_per_job")
                    or any(i._xs_installed and i.progressCrossSection for i in flat)):
                # a layer that cannot be one merged job (no line list, a measured cross-section table, more line lists than a
                # job takes, somebody's own array installed): its own route leaves the same resident absorption coefficient
                st, _ = L._ensure_swept()
                plan.append((L, st, g, members, flat, conc, None))
                continue
            _check_window(g)
            st = _kept_state(L, "_sweep_state")
            st.reserve(ctx, n)
            plan.append((L, st, g, members, flat, conc, L._merged_key(flat, conc, L, g)))
        # (a layer's absorption coefficient stands as long as everything but the depth is what it was computed from)
        todo = [p for p in plan if p[6] is not None and not (isinstance(p[1].key, tuple) and p[1].key[:-1] == p[6][:-1])]
        ctx.layers_merged_accumulate_dev(
            [dict(lines=[i._device_lines(ctx) for i in flat], iso=[_iso_params(i) for i in flat],
                  grid=_engine.native_grid(g), iso_mol=[m for m, isos in enumerate(members) for _ in isos], conc=conc,
                  abs_coef=st.buf(ctx, "abs_coef")) for (L, st, g, members, flat, conc, key) in todo])
        for (L, st, g, members, flat, conc, key) in plan:
            if key is not None and st.key != key:
                st.key = key[:-1] + ("absorption coefficient only",)
        for (L, st, g, members, flat, conc, key) in todo:
            for iso in flat:
                iso._defer_cross_section()
            L._members_ready()
        return plan

    # -- the resident column: the next call's argument blocks are already on the C side (lbl_column, ABI 5) --------------
    def _column_drop(self):
        fast = self.__dict__.pop("_column_fast", None)
        if fast is not None and fast["col"].h and fast["col"].ctx.h:
            fast["col"].free()

    def _column_remember(self, ctx, layers, n, plan):
        """After a call through the general route: if every layer was one merged job, keep the column's blocks in a C-side
        handle; the next call then only looks at every layer's stamp (Layer._column_stamp)."""
        self._column_drop()
        if not plan or any(p[6] is None for p in plan):
            return
        col = ctx.column([dict(lines=[i._device_lines(ctx) for i in flat], iso=[_iso_params(i) for i in flat],
                               grid=_engine.native_grid(g), iso_mol=[m for m, isos in enumerate(members) for _ in isos], conc=conc,
                               depth=L.depth, abs_coef=st.bufs["abs_coef"]) for (L, st, g, members, flat, conc, key) in plan])
        stamps = [L._column_stamp() for L in layers]
        self.__dict__["_column_fast"] = dict(
            col=col, glob=(id(ctx), n, utils.BASE_RESOLUTION, settings.ACCURACY), layers=list(layers),
            val=[s_[0] for s_ in stamps], done=[(s_[0][:-1], s_[1]) for s_ in stamps], kbuf=[p[1].bufs["abs_coef"] for p in plan],
            n_iso=[len(p[4]) for p in plan])
        import weakref
        weakref.finalize(self, lambda c=col: c.free() if (c.h and c.ctx.h) else None)

    def _transmission_resident(self, ctx, layers, n, surfaceSpectrum, surfaceTemperature):
        """The call through the resident column handle, or None (no handle yet, another context / grid / accuracy mode, the
        list of layers changed, a layer can no longer be one merged job: the general route then rebuilds the handle)."""
        fast = self.__dict__.get("_column_fast")
        if fast is None:
            return None
        col = fast["col"]
        if (fast["glob"] != (id(ctx), n, utils.BASE_RESOLUTION, settings.ACCURACY) or not col.h or len(layers) != len(fast["layers"])
                or any(a is not b for a, b in zip(layers, fast["layers"]))):
            return None
        due, redo = [], []
        for l, L in enumerate(layers):
            val, ver = L._column_stamp()
            st = L.__dict__.get("_sweep_state")
            if st is None or st.bufs.get("abs_coef") is not fast["kbuf"][l]:
                return None
            if val != fast["val"][l]:
                if val[-1:] != fast["val"][l][-1:] and val[:-1] == fast["val"][l][:-1]:
                    redo.append((l, L, val, True))              # only the depth (changeDepth resets nothing, cls:754-755)
                else:
                    redo.append((l, L, val, False))
            due.append((val[:-1], ver) != fast["done"][l])
        for l, L, val, depth_only in redo:
            members, conc = L._sweep_members()
            flat = [iso for isos in members for iso in isos]
            if (len(flat) != fast["n_iso"][l] or any(i.exotic for i in flat) or len(conc) != len(val[7])
                    or any(i._xs_installed and i.progressCrossSection for i in flat)):
                return None
            g = L._grid()
            if g["n_base"] != n:
                return None
            _check_window(g)
            col.set_layer(l, [i._device_lines(ctx) for i in flat], [_iso_params(i) for i in flat], _engine.native_grid(g), conc,
                          L.depth, fast["kbuf"][l])
            fast["val"][l] = val
        ast = _kept_state(self, "_toa_state")
        out = ast.reserve(ctx, n).buf(ctx, "toa")
        I_in = None
        if surfaceSpectrum is not None:
            I_in = ast.buf(ctx, "I_in").upload(np.ascontiguousarray(surfaceSpectrum, dtype=np.float64))
        host = ctx.host_array(n)
        try:
            # (four pieces: eight measured no faster, and every piece is one more argument block in the library's cache of eight)
            col.transmission(due, out, host=host, I_in=I_in, surface_T=float(surfaceTemperature or 0.0),
                             pieces=4 if n >= (1 << 16) else 1)
            # bookkeeping of the object model, while the device works: what the general route does for the layers it recomputed
            for l, L in enumerate(layers):
                if not due[l]:
                    continue
                members, conc = L._sweep_members()
                flat = [iso for isos in members for iso in isos]
                key = L._merged_key(flat, conc, L, L._grid())
                L.__dict__["_sweep_state"].key = key[:-1] + ("absorption coefficient only",)
                for iso in flat:
                    iso._defer_cross_section()
                L._members_ready()
                val, ver = L._column_stamp()                  # (_defer_cross_section bumps no input version)
                fast["done"][l] = (val[:-1], ver)
        except Exception:
            self._column_drop()
            raise
        finally:
            ctx.download_wait()
        return host


# ----------------------------------------------------------------------------------------
# plot-type dispatch (cls:824-839), plot (cls:849-873) and plotSpectrum (cls:876-944).  What the
# figures show is computed on the device path (getters, transmission, band integrals); drawing it is
# matplotlib's job, imported when a figure is asked for.
# ----------------------------------------------------------------------------------------
def returnPlot(obj, propertyToPlot):
    if propertyToPlot == "transmittance":
        return getTransmittance(obj), 1
    if propertyToPlot == 'absorption coefficient':
        return getAbsCoef(obj), 0
    if propertyToPlot == 'cross section':
        return getCrossSection(obj), 0
    if propertyToPlot == 'absorbance':
        return getAbsorbance(obj), 0
    if propertyToPlot == 'optical depth':
        return getOpticalDepth(obj), 0
    if propertyToPlot == 'line survey':
        return obj.lineSurvey, 0
    return False


def _pyplot():
    try:
        import matplotlib.pyplot as plt
    except ImportError as e:            # the numbers do not need it: returnPlot / spectrumCurves
        raise ImportError("pyrad_amd.plot / plotSpectrum draw with matplotlib, which is not installed; the curves and legend "
                          "texts themselves are available without it from returnPlot() and spectrumCurves()") from e
    return plt


def _dark_axes(plt, title):
    plt.figure(figsize=(10, 6), dpi=80)
    plt.subplot(111, facecolor='xkcd:dark grey')
    plt.margins(0.01)
    plt.subplots_adjust(left=.07, bottom=.08, right=.97, top=.90)
    plt.title('%s' % title)


def _white_legend(plt, handles):
    legend = plt.legend(handles=handles, frameon=False)
    plt.setp(legend.get_texts(), color='w')


def plot(propertyToPlot, title, plotList, fill=False):
    """cls:849-873: one curve per object of ``plotList`` for a plot-type string of returnPlot (ui:407-413)."""
    plt = _pyplot()
    _dark_axes(plt, title)
    plt.xlabel('wavenumber cm-1')
    plt.ylabel(propertyToPlot)
    if propertyToPlot == 'line survey':
        plt.yscale('log')
    plt.grid('grey', linewidth=.5, linestyle=':')
    handles = []
    style = dict(linewidth=1.2, alpha=.7)
    for singlePlot, color in zip(plotList, COLOR_LIST):
        yAxis, fillAxis = returnPlot(singlePlot, propertyToPlot)
        xAxis = singlePlot.xAxis
        curve, = plt.plot(xAxis, yAxis, color=color, label='%s' % singlePlot.name, **style)
        handles.append(curve)
        plt.fill_between(xAxis, fillAxis, yAxis, color=color, alpha=.3 * fill)
        style = dict(linewidth=.7, alpha=.5)
    _white_legend(plt, handles)
    plt.show()


def _planck_axis(planckType, rangeMin, rangeMax):
    """abscissa and Planck function of a plotSpectrum type (cls:888-903); None for an unknown type"""
    if planckType == 'wavenumber':
        n = int((rangeMax - rangeMin) / utils.BASE_RESOLUTION)
        return ('wavenumber cm-1', 'Radiance Wm-2sr-1(cm-1)-1',
                np.linspace(rangeMin, rangeMax, n), lambda T: _planck_wavenumber_axis(rangeMin, rangeMax, n, T))
    if planckType == 'Hz':
        x = np.linspace(rangeMin, rangeMax, 1000)
        return 'Hertz', 'Radiance Wm-2sr-1Hz-1', x, lambda T: planckHz(x, T)
    if planckType == 'wavelength':
        x = np.linspace(rangeMin, rangeMax, int((rangeMax - rangeMin) / utils.BASE_RESOLUTION))
        return 'wavelength um', 'Radiance Wm-2sr-1um-1', x, lambda T: planckWavelength(x, T)
    return None


def _planck_wavenumber_axis(rangeMin, rangeMax, n, temperature):
    """pyradPlanck.planckWavenumber on linspace(rangeMin, rangeMax, n) (pl:38-44), on the device (lbl_planck_dev)."""
    ctx = _ctx()
    out = ctx.buffer(max(n, 1))
    try:
        ctx.planck_dev(rangeMin, rangeMax, n, float(temperature), out)
        return out.download(n)
    finally:
        out.free()


def planckHz(Hz, temp):
    """pyradPlanck.py:18-26 (Wm-2sr-1Hz-1; plot-only, host NumPy)"""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        a = 2 * h * Hz**3 / c**2
        b = h * Hz / k / temp
        return a / (np.exp(b) - 1)


def planckWavelength(lam, temp):
    """pyradPlanck.py:29-35 (wavelength in um, Wm-2sr-1um-1; plot-only, host NumPy)"""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        a = 2.0E24 * h * c ** 2 / (lam ** 5)
        b = 10 ** 6 * h * c / lam / k / temp
        return a / (np.exp(b) - 1)


def spectrumCurves(layer=None, title=None, rangeMin=None, rangeMax=None, objList=None, surfaceSpectrum=None,
                   planckTemperatureList=None, planckType='wavenumber'):
    """Everything plotSpectrum draws (cls:876-944), without drawing it: axis labels, title, and the curves in
    the reference's order - one Planck curve per temperature, labelled '<T>K : <band integral>Wm-2' with
    integrateSpectrum(y, res=(rangeMax - rangeMin) / len(y)) (cls:914), then for every object of ``objList`` its
    ``transmission(surfaceSpectrum)`` labelled '<name> : <integrateSpectrum(y, pi)>Wm-2' (cls:933-937).  Transmission,
    Planck curves on the layer axis and the integrals run on the device."""
    if layer:
        rangeMin, rangeMax, title = layer.rangeMin, layer.rangeMax, layer.title
    axis = _planck_axis(planckType, rangeMin, rangeMax)
    if axis is None:
        raise UnboundLocalError("local variable 'xAxis' referenced before assignment")     # what cls:906-912 ends in
    xlabel, ylabel, xAxis, planckFunction = axis
    if not rangeMax:
        xAxis = layer.xAxis                                                                # cls:910-911
    curves = []
    for temperature in planckTemperatureList:
        yAxis = planckFunction(float(temperature))
        power = integrateSpectrum(yAxis, res=(rangeMax - rangeMin) / len(yAxis))
        curves.append(dict(kind='planck', x=xAxis, y=yAxis, power=power, label='%sK : %sWm-2' % (temperature, round(power, 2))))
    surfacePower = None
    if objList:
        surfacePower = integrateSpectrum(surfaceSpectrum, pi)                              # cls:933
        for obj in objList:
            yAxis = obj.transmission(surfaceSpectrum)
            power = integrateSpectrum(yAxis, pi)
            curves.append(dict(kind='object', x=layer.xAxis, y=yAxis, power=power, label='%s : %sWm-2' % (obj.name, round(power, 2))))
    return dict(title=title, xlabel=xlabel, ylabel=ylabel, curves=curves, surfacePower=surfacePower)


def plotSpectrum(layer=None, title=None, rangeMin=None, rangeMax=None, objList=None, surfaceSpectrum=None,
                 planckTemperatureList=None, planckType='wavenumber', fill=False):
    """cls:876-944 (ui:373 Planck curves, ui:399 transmission through a layer): the figure of spectrumCurves()."""
    plt = _pyplot()
    spec = spectrumCurves(layer, title, rangeMin, rangeMax, objList, surfaceSpectrum, planckTemperatureList, planckType)
    _dark_axes(plt, spec['title'])
    plt.xlabel(spec['xlabel'])
    plt.ylabel(spec['ylabel'])
    handles = []
    rgb = [1.0, .6, .3]                       # the Planck curves walk through the colours like cls:904-931
    step = [-.15, .15, .15]
    objects = iter(zip(COLOR_LIST, [dict(alpha=.7, linewidth=1.2)] + [dict(alpha=.5, linewidth=1)] * len(COLOR_LIST)))
    for c in spec['curves']:
        if c['kind'] == 'planck':
            curve, = plt.plot(c['x'], c['y'], linewidth=.75, color=tuple(rgb), linestyle=':', label=c['label'])
            for i in range(3):
                if not 0 <= rgb[i] + step[i] <= 1:
                    step[i] = -step[i]
                rgb[i] += step[i]
            if rgb[0] < .3 and rgb[1] < .3 and rgb[2] < .3:
                rgb[1] += .5
                rgb[2] += .2
            if rgb[0] < .3 and rgb[1] < .3:
                rgb[1] += .4
        else:
            color, style = next(objects)
            curve, = plt.plot(c['x'], c['y'], color=color, label=c['label'], **style)
        handles.append(curve)
    _white_legend(plt, handles)
    plt.show()
