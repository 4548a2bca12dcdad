#!/usr/bin/env python3
"""The model-level sibling of dump_transport.py: every Atmosphere method over the column transport entry points (fluxes,
jacobians, jacobiansLinear, observe, observeLinear, radiance, pathJacobians, pathJacobiansLinear, solarFluxesTwoStream,
fluxesTwoStream, radianceTwoStream, solarRadianceTwoStream, jacobiansTwoStream) over its option matrix on
a seeded synthetic column, every array of every result saved as .npy (one file per call, the arrays concatenated in the
order of their attribute names), and beside them calls.txt: every Context.column_* / ray_* / ils_convolve_dev call and every
Buffer upload, download and device copy, with its arguments by value (arrays of more than 32 values as length and SHA-1 of
their float64 / int64 bytes) and its buffers as b<k>:<n>, k the order of first appearance.  Run it once per commit of the
Python layer with one library (PYRAD_HIP_LIB) and compare: the same files, the same values bit for bit and the same call log
say that the Python above the C boundary hands the same work to the device.
usage: dump_model_transport.py <out dir> [--against <dir of an earlier dump>]
With --against the dump is compared with the earlier one; the exit status is 1 if a file, a value or a line of calls.txt
differs, or if less than 95 % of the values dumped are finite and not zero (a dump of zeros compares equal and says nothing)."""
import hashlib, inspect, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrad_amd import _native as nat, data, model, settings, synthetic

RNG = (600, 610.07)             # 1,007 points: no multiple of 4 (asserted below)
LAYERS = ((1e4, 288, 1013.25), (2e4, 270, 700.0), (5e4, 240, 300.0), (1e5, 220, 80.0))
LEVELS = [293.0, 279.0, 256.0, 229.0, 214.0]
VOIGT_RNG = (600.0, 605.0)
VOIGT_LAYERS = ((1e4, 288, 1013.25), (2e4, 250, 100.0), (5e4, 220, 10.0))
FINITE_SHARE = 0.95


# ---- the call log ----------------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.lines, self.count = [], 0

    def value(self, v):
        if isinstance(v, nat.Buffer):
            if "_dump_k" not in v.__dict__:          # (stamped on the object: an id() comes back once a buffer is gone)
                v._dump_k = self.count = self.count + 1
            return "b%d:%d" % (v._dump_k, v.n)
        if v is None or isinstance(v, str):
            return repr(v)
        if isinstance(v, (bool, int, np.integer)):
            return repr(int(v))
        if isinstance(v, (float, np.floating)):
            return repr(float(v))
        if isinstance(v, np.ndarray) and v.dtype.kind in "fiub":
            a = np.ascontiguousarray(v, dtype=np.float64 if v.dtype.kind == "f" else np.int64).reshape(-1)
            if a.size > 32:
                return "%s[%d]:%s" % (a.dtype.name, a.size, hashlib.sha1(a.tobytes()).hexdigest())
            return "[" + ", ".join(self.value(x) for x in a) + "]"
        if isinstance(v, (list, tuple, np.ndarray)):
            if len(v) > 32 and all(isinstance(x, (float, np.floating)) for x in v):
                return self.value(np.asarray(v, dtype=np.float64))
            return "[" + ", ".join(self.value(x) for x in v) + "]"
        return "<%s>" % type(v).__name__

    def wrap(self, cls, name):
        fn = getattr(cls, name)
        sig = inspect.signature(fn)
        rec = self

        def logged(obj, *a, **kw):
            bound = sig.bind(obj, *a, **kw)
            bound.apply_defaults()
            args = list(bound.arguments.items())
            head = rec.value(obj) + "." if isinstance(obj, nat.Buffer) else ""
            rec.lines.append("%s%s(%s)" % (head, name, ", ".join("%s=%s" % (k, rec.value(v)) for k, v in args[1:])))
            return fn(obj, *a, **kw)
        setattr(cls, name, logged)

    def install(self):
        for name in sorted(vars(nat.Context)):
            if name.startswith(("column_", "ray_")) or name == "ils_convolve_dev":
                if callable(getattr(nat.Context, name)):
                    self.wrap(nat.Context, name)
        for name in ("upload", "download", "stage_from_dev"):
            self.wrap(nat.Buffer, name)
        return self


# ---- what is saved ---------------------------------------------------------------------------------------------------------
def _arrays(v):
    if isinstance(v, np.ndarray):
        return [np.asarray(v, dtype=np.float64).reshape(-1)] if v.dtype.kind in "fiu" else []
    if isinstance(v, (list, tuple)):
        return [a for x in v for a in _arrays(x)]
    return []


class Dump:
    def __init__(self, out):
        self.out, self.names = out, set()
        self.tally = [0, 0, 0]            # files, values, values that are finite and not zero

    def __call__(self, name, result):
        """one file per call: every array attribute of the result, in the order of the attributes' names"""
        assert name not in self.names, name
        self.names.add(name)
        attrs = vars(result) if hasattr(result, "__dict__") else {k: getattr(result, k) for k in result.__slots__}
        values = np.concatenate([a for k in sorted(attrs) for a in _arrays(attrs[k])])
        np.save(os.path.join(self.out, name + ".npy"), values)
        self.tally[0] += 1
        self.tally[1] += values.size
        self.tally[2] += int(np.count_nonzero(np.isfinite(values) & (values != 0.0)))


# ---- the calls -------------------------------------------------------------------------------------------------------------
def column(rng, layers):
    atm = model.Atmosphere("col")
    for depth, T, P in layers:
        L = atm.addLayer(depth, T, P, *rng)
        L.addMolecule("co2", ppm=400)
        L.addMolecule("h2o", percentage=0.5)
    return atm


def tag(**kw):
    def one(v):
        return "arr" if isinstance(v, np.ndarray) else "x".join(one(x) for x in v) if isinstance(v, list) else str(v)
    return "_".join("%s-%s" % (k, one(v)) for k, v in kw.items())


def path_sets(atm, reflecting, lev):
    """tests/test_gpu_path_jacobian.py's all_paths and a second limb path, a mirror path where the surface reflects, and
    nadir views enough for more than one chunk of pathJacobians(); ``lev``: the level temperatures the paths carry, or None"""
    kw = {} if lev is None else dict(levelTemperatures=lev)
    hand = {} if lev is None else dict(temperatures=[(250.0, 262.0), (262.0, 270.0), (281.0, 290.0), (270.0, 255.0)])
    paths = [atm.nadirPath(**kw), atm.nadirPath(mu=0.4, **kw), atm.nadirPath(observerLevel=2, **kw), atm.zenithPath(**kw),
             atm.zenithPath(mu=0.3, **kw), atm.zenithPath(observerLevel=2, **kw), atm.limbPath(5e3, **kw),
             atm.limbPath(2.5e4, **kw), atm.limbPath(1.7e5, **kw),
             model.Path([], [], source="surface", **({} if lev is None else dict(temperatures=[]))),
             model.Path([1, 1, 0, 1], [3e4, 1e4, 2e4, 5e3], source="surface", **hand)]
    paths += [atm.nadirPath(mu=m, **kw) for m in (0.9, 0.7, 0.55, 0.3)]
    paths.append(atm.limbPath(1.2e4, **kw))
    if reflecting:
        paths.append(atm.reflectedPath(mu=0.8, **kw))
    return paths, paths + [atm.nadirPath(mu=0.25 + 0.0125 * i, **kw) for i in range(60)]


def transport_calls(save):
    atm = column(RNG, LAYERS)
    x = atm[0].xAxis
    n = len(x)
    assert n % 4 != 0 and 900 < n < 1100, n
    rng = np.random.default_rng(20241020)
    e_arr = rng.uniform(0.55, 0.98, n)
    surface = np.array(model.planckWavenumber(x, 300.0)) * rng.uniform(0.9, 1.0, n)
    top = 0.1 * np.array(model.planckWavenumber(x, 250.0))
    bands = [(600.0, 604.0), (604.0, 610.07)]
    ins = model.Instrument(np.linspace(601.5, 608.5, 5), width=0.5)
    emissivities = (None, 0.8, e_arr)
    reflections = ("lambertian", "specular")

    for e in emissivities:
        for planck in ("layer", "linear"):
            for refl in reflections:
                for spectra in (False, True):
                    save("fluxes_" + tag(e=e, planck=planck, refl=refl, spectra=spectra),
                         atm.fluxes(surfaceTemperature=290.0, bands=bands, emissivity=e, planck=planck, reflection=refl,
                                    spectra=spectra))
    save("fluxes_surfaceSpectrum", atm.fluxes(surfaceSpectrum=surface, bands=bands, emissivity=e_arr, spectra=True))
    save("fluxes_topSpectrum", atm.fluxes(surfaceTemperature=290.0, topSpectrum=top, bands=bands, emissivity=0.8,
                                          planck="linear", levelTemperatures=LEVELS, spectra=True))

    for name in ("jacobians", "jacobiansLinear"):
        method = getattr(atm, name)
        for e in emissivities:
            for refl in reflections:
                for molecules in (False, True):
                    for spectra in (False, True):
                        save(name + "_" + tag(e=e, refl=refl, molecules=molecules, spectra=spectra),
                             method(surfaceTemperature=290.0, bands=bands, emissivity=e, reflection=refl,
                                    molecules=molecules, spectra=spectra))
        save(name + "_topSpectrum", method(surfaceSpectrum=surface, topSpectrum=top, emissivity=e_arr, spectra=True))
    save("jacobiansLinear_levels", atm.jacobiansLinear(surfaceTemperature=290.0, bands=bands, emissivity=0.8,
                                                       levelTemperatures=LEVELS, spectra=True))

    for name in ("observe", "observeLinear"):
        method = getattr(atm, name)
        for jac in (False, True):
            for e in (None, 0.8):
                for mu in (1.0, 0.6):
                    save(name + "_" + tag(jacobians=jac, e=e, mu=mu),
                         method(ins, surfaceTemperature=290.0, mu=mu, jacobians=jac, emissivity=e))
    save("observe_earr", atm.observe(ins, surfaceSpectrum=surface, jacobians=True, emissivity=e_arr))
    save("observeLinear_earr", atm.observeLinear(ins, surfaceSpectrum=surface, jacobians=True, emissivity=e_arr,
                                                 levelTemperatures=LEVELS))

    for e in (None, e_arr):
        for planck in ("layer", "linear"):
            few, many = path_sets(atm, e is not None, LEVELS if planck == "linear" else None)
            for refl in reflections:
                for trn in (False, True):
                    for instrument in (None, ins):
                        save("radiance_" + tag(e=e, planck=planck, refl=refl, transmittance=trn, ins=instrument is not None),
                             atm.radiance(few, surfaceTemperature=290.0, instrument=instrument, transmittance=trn,
                                          emissivity=e, reflection=refl, planck=planck))
            method = atm.pathJacobiansLinear if planck == "linear" else atm.pathJacobians
            for molecules in (False, True):
                for instrument in (None, ins):
                    save("pathJacobians_" + tag(e=e, planck=planck, molecules=molecules, ins=instrument is not None),
                         method(many, surfaceTemperature=290.0, instrument=instrument, molecules=molecules, emissivity=e,
                                reflection="specular"))
    few, _ = path_sets(atm, True, LEVELS)
    save("radiance_surfaceSpectrum", atm.radiance(few, surfaceSpectrum=surface, emissivity=0.8, planck="linear",
                                                   levelTemperatures=LEVELS, transmittance=True))
    save("pathJacobiansLinear_surfaceSpectrum", atm.pathJacobiansLinear(few, surfaceSpectrum=surface, emissivity=0.8,
                                                                         reflection="specular", instrument=ins))


def scatter_calls(save):
    """solarFluxesTwoStream, fluxesTwoStream, jacobiansTwoStream, radianceTwoStream and solarRadianceTwoStream: no scatterers and two (numbers, n values and a table,
    mixed), deltaScaling, the emissivity forms, planck, bands, spectra, more views than one chunk, with and without instrument"""
    atm = column(RNG, LAYERS)
    x = atm[0].xAxis
    n = len(x)
    rng = np.random.default_rng(20241021)
    e_arr = rng.uniform(0.55, 0.98, n)
    surface = np.array(model.planckWavenumber(x, 300.0)) * rng.uniform(0.9, 1.0, n)
    top = 0.1 * np.array(model.planckWavenumber(x, 250.0))
    bands = [(600.0, 604.0), (604.0, 610.07)]
    ins = model.Instrument(np.linspace(601.5, 608.5, 5), width=0.5)
    cloud = model.Scatterer([0.0, 3.0, 0.5, 0.0], extinction=1.0, singleScatteringAlbedo=rng.uniform(0.6, 0.99, n),
                            asymmetry=0.8, name="cloud")
    haze = model.Scatterer([0.2, 0.1, 0.05, 0.02], extinction=rng.uniform(0.5, 1.5, n), singleScatteringAlbedo=0.9,
                           asymmetry=(np.array([590.0, 620.0]), np.array([0.3, 0.5])), name="haze")
    few = [1.0, (0.6, "down"), (0.35, "up")]
    many = few + [(0.2 + 0.04 * i, "down" if i % 3 == 0 else "up") for i in range(18)]
    for scat in ((), (cloud, haze)):
        for delta in (False, True):
            for e in (1.0, 0.8, e_arr):
                t = tag(scat=len(scat), delta=delta, e=e)
                for spectra in (False, True):
                    for b in (None, bands):
                        u = t + "_" + tag(spectra=spectra, bands=b is not None)
                        save("solarFluxesTwoStream_" + u,
                             atm.solarFluxesTwoStream(scat, delta, solarTemperature=5772.0, mu0=[(0.5, 0.7), (0.9, 0.3)],
                                                      emissivity=e, bands=b, spectra=spectra))
                        for planck in ("layer", "linear"):
                            save("fluxesTwoStream_" + u + "_" + tag(planck=planck),
                                 atm.fluxesTwoStream(scat, delta, surfaceTemperature=290.0, topSpectrum=top, emissivity=e,
                                                     planck=planck, bands=b, spectra=spectra))
                            save("jacobiansTwoStream_" + u + "_" + tag(planck=planck),
                                 atm.jacobiansTwoStream(scat, delta, surfaceTemperature=290.0, topSpectrum=top, emissivity=e,
                                                        planck=planck, bands=b, molecules=b is None, spectra=spectra))
                for planck in ("layer", "linear"):
                    for views in (few, many):
                        for instrument in (None, ins):
                            save("radianceTwoStream_" + t + "_" + tag(planck=planck, views=len(views), ins=instrument is not None),
                                 atm.radianceTwoStream(views, scat, delta, surfaceTemperature=290.0, topSpectrum=top,
                                                       emissivity=e, planck=planck, instrument=instrument))
                for views in (few, many) if scat else (few,):       # (without scatterers a down view is 0 throughout)
                    for instrument in (None, ins):
                        save("solarRadianceTwoStream_" + t + "_" + tag(views=len(views), ins=instrument is not None),
                             atm.solarRadianceTwoStream(views, scat, delta, solarTemperature=5772.0, mu0=0.5, emissivity=e,
                                                        instrument=instrument))
    kw = dict(surfaceSpectrum=surface, emissivity=e_arr, planck="linear", levelTemperatures=LEVELS)
    save("fluxesTwoStream_surfaceSpectrum", atm.fluxesTwoStream((cloud, haze), bands=bands, spectra=True, **kw))
    save("radianceTwoStream_surfaceSpectrum", atm.radianceTwoStream(many, (cloud, haze), instrument=ins, **kw))
    save("jacobiansTwoStream_surfaceSpectrum", atm.jacobiansTwoStream((cloud, haze), bands=bands, spectra=True, **kw))
    save("solarRadianceTwoStream_spectrum", atm.solarRadianceTwoStream(many, cloud, solarSpectrum=surface, mu0=0.4,
                                                                       geometry="spherical", instrument=ins))
    save("solarFluxesTwoStream_spectrum", atm.solarFluxesTwoStream(cloud, solarSpectrum=surface, mu0=0.4, geometry="spherical",
                                                                   spectra=True))


def voigt_calls(save):
    """temperature="full": dk/dT as terms, which exists under the Voigt line shape only"""
    settings.set_line_shape("voigt")
    data.set_source(data.synthetic_source(dict(co2=synthetic.make_lines(41, 150, 590, 615),
                                               h2o=synthetic.make_lines(42, 150, 590, 615))))
    atm = column(VOIGT_RNG, VOIGT_LAYERS)
    for name in ("jacobians", "jacobiansLinear"):
        save(name + "_full", getattr(atm, name)(surfaceTemperature=288.0, temperature="full", emissivity=0.8, spectra=True))
    for planck in ("layer", "linear"):
        save("jacobiansTwoStream_full_" + planck, atm.jacobiansTwoStream(surfaceTemperature=288.0, temperature="full",
                                                                         emissivity=0.8, planck=planck, spectra=True))


def run(out):
    model.Layer.hasAtmosphere = False
    settings.set_resolution_multiplier(1)
    settings.set_layer_step("merged")
    settings.set_line_shape("reference")
    data.set_source(data.synthetic_source(dict(co2=synthetic.make_lines(51, 800, 580, 720),
                                               h2o=synthetic.make_lines(52, 500, 580, 720))))
    rec = Recorder().install()
    save = Dump(out)
    transport_calls(save)
    scatter_calls(save)
    voigt_calls(save)
    with open(os.path.join(out, "calls.txt"), "w") as f:
        f.write("\n".join(rec.lines) + "\n")
    return save.tally, len(rec.lines)


def compare(a, b):
    """the verdict per file as scripts/bitcmp_libs.sh gives it; the number of differences"""
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb:
        print("the two dumps hold different files: %s" % sorted(set(fa) ^ set(fb)))
        return 1
    bad = 0
    for f in fa:
        if f == "calls.txt":
            la, lb = open(os.path.join(a, f)).read().split("\n"), open(os.path.join(b, f)).read().split("\n")
            diff = [i for i, (p, q) in enumerate(zip(la, lb)) if p != q]
            same = not diff and len(la) == len(lb)
            print(f, "identical (%d lines)" % (len(la) - 1) if same else "DIFFERENT: %d and %d lines, first at line %d"
                  % (len(la) - 1, len(lb) - 1, diff[0] + 1 if diff else min(len(la), len(lb))))
            if diff:
                print("  <", la[diff[0]][:400])
                print("  >", lb[diff[0]][:400])
        else:
            p, q = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
            same = p.shape == q.shape and np.array_equal(p, q, equal_nan=True)
            if not same:
                with np.errstate(all="ignore"):
                    print(f, "DIFFERENT: shapes %s and %s" % (p.shape, q.shape) if p.shape != q.shape else
                          "DIFFERENT: max rel %.3e at %d points" % (np.nanmax(np.abs(p - q) / np.maximum(np.abs(q), 1e-300)),
                                                                   np.count_nonzero(~((p == q) | ((p != p) & (q != q))))))
        bad += 0 if same else 1
    print("%d files, bit-identical" % len(fa) if bad == 0 else "%d of %d files differ" % (bad, len(fa)))
    return bad


def main(argv):
    if len(argv) not in (2, 4) or (len(argv) == 4 and argv[2] != "--against"):
        sys.exit(__doc__)
    out = argv[1]
    os.makedirs(out, exist_ok=True)
    if os.listdir(out):
        sys.exit("%s is not empty: files of an earlier dump would be compared with this one's" % out)
    (files, values, live), calls = run(out)
    from pyrad_amd import engine
    engine.shutdown()
    share = live / max(values, 1)
    print("dumped to %s: %d files, %d values, %d of them finite and not zero (%.2f %%), %d calls logged"
          % (out, files, values, live, 100.0 * share, calls))
    bad = 0
    if len(argv) == 4:
        bad = compare(argv[3], out)
        if share < FINITE_SHARE:
            print("only %.2f %% of the values are finite and not zero, %.0f %% are asked for" % (100.0 * share, 100.0 * FINITE_SHARE))
            bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main(sys.argv)
