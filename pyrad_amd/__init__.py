"""MI355X line-by-line engine.  The object model lives in pyrad_amd.model; the names below are reachable from the package
itself and are resolved on first use, so that importing the package stays free of side effects."""
_MODEL_EXPORTS = ("gIntervals", "kDistribution", "KDistribution", "ScatterRadiance")


def __getattr__(name):
    if name in _MODEL_EXPORTS:
        from . import model
        return getattr(model, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
