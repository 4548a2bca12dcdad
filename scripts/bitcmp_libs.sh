# bit-for-bit comparison of two library builds: usage bitcmp_libs.sh <lib a> <lib b> [dump script]
# (libraries: names under scripts/bin without the libpyrad_hip_ prefix, or 'prod'; dump script: a script under scripts/ that
# takes an output directory - dump_spectra.py, the default: C1, C2, C3 (merged and per-list) and the column;
# dump_transport.py: every column transport entry point on synthetic absorption coefficients; dump_model_transport.py: every
# Atmosphere method over them, with its call log, which is compared byte for byte).  Each dump runs under a time
# limit of its own (DUMP_TIMEOUT seconds, default 300), and nothing more is started after one that fails.
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
D=${3:-dump_spectra.py}
T=/tmp/$(basename "$D" .py)
for l in $1 $2; do
  if [ "$l" = prod ]; then unset PYRAD_HIP_LIB; else export PYRAD_HIP_LIB=$R/scripts/bin/libpyrad_hip_$l.so; fi
  timeout -k 10 ${DUMP_TIMEOUT:-300} python3 $R/scripts/$D ${T}_$l || exit 1
done
python3 - ${T}_$1 ${T}_$2 <<'PY'
import sys, os, numpy as np
a, b = sys.argv[1:3]
bad = 0
if sorted(os.listdir(a)) != sorted(os.listdir(b)):
    sys.exit("the two dumps hold different files")
for f in sorted(os.listdir(a)):
    if not f.endswith(".npy"):          # (dump_model_transport.py's calls.txt: compared as bytes)
        with open(os.path.join(a, f), "rb") as fa, open(os.path.join(b, f), "rb") as fb:
            same = fa.read() == fb.read()
        bad += 0 if same else 1
        if not same:
            print(f, "DIFFERENT")
        continue
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    same = x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    bad += 0 if same else 1
    if not same or len(os.listdir(a)) <= 40:
        with np.errstate(all="ignore"):
            print(f, "identical" if same else "DIFFERENT: max rel %.3e at %d points" % (np.nanmax(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)), np.count_nonzero(~((x == y) | ((x != x) & (y != y))))))
print("%d files, bit-identical" % len(os.listdir(a)) if bad == 0 else "%d of %d files differ" % (bad, len(os.listdir(a))))
sys.exit(1 if bad else 0)
PY
