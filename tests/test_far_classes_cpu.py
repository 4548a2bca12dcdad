"""CPU: the exact mode's distance classes are the minimal staircase of the far-field series' remainder bound.

tests/test_far_terms_cpu.py holds every {d, terms} pair of `kFarClassExact` to the bound at the class's own start.  This
file holds the TABLE to the bound at every whole distance: a chunk whose nearest line is d half-spans from the span centre
falls into the last class that starts at or below d, and for every d in 3 .. 40 (a one-atmosphere window ends at 39) that
class must carry exactly the smallest term count whose remainder

    rho^NT (NT (1 - rho) + 1) (1 + rho)^2 / (1 - rho)^2,   rho = 1 / d,

stays at or below 7.8e-17 - no d could take fewer terms than its class gives it, and no class carries more than its own
start needs.  The first two rows are the two builds' own thresholds and counts (the series from 3 half-spans on with 38
terms, from 4 on with 30).
"""
import os
import re

from pyrad_amd import _native

LIMIT_EXACT = 7.8e-17
D_MAX = 40


def remainder(d, nt):
    rho = 1.0 / d
    return rho ** nt * (nt * (1.0 - rho) + 1.0) * (1.0 + rho) ** 2 / (1.0 - rho) ** 2


def classes(name="kFarClassExact"):
    with open(os.path.join(_native.CSRC, "lbl_kernels.hip")) as fh:
        text = fh.read()
    m = re.search(r"constexpr int %s\[(\d+)\]\[2\] = \{(.*)\};" % name, text)
    assert m, name
    pairs = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", m.group(2))]
    assert len(pairs) == int(m.group(1)), pairs
    return pairs


def minimal_terms(d):
    nt = 2
    while remainder(d, nt) > LIMIT_EXACT:
        nt += 1
    return nt


def class_of(pairs, d):
    """the last class that starts at or below d: what far_chunk's descent and the edge series' count select"""
    hit = [p for p in pairs if p[0] <= d]
    assert hit, d
    return hit[-1]


def test_every_distance_takes_the_minimal_count():
    pairs = classes()
    for d in range(3, D_MAX + 1):
        start, nt = class_of(pairs, d)
        need = minimal_terms(d)
        print("d = %2d: class from %2d, %2d terms (remainder %.2e), minimal %2d" % (d, start, nt, remainder(d, nt), need))
        assert remainder(d, nt) <= LIMIT_EXACT, (d, nt)
        assert nt == need, (d, start, nt, need)


def test_one_class_per_distinct_count_starting_where_the_count_first_holds():
    pairs = classes()
    counts = [nt for _, nt in pairs]
    assert len(set(counts)) == len(counts), pairs                        # one row per distinct count
    assert counts == sorted(counts, reverse=True), pairs                 # nearest first
    for start, nt in pairs:
        assert nt == minimal_terms(start), (start, nt)                   # no more than the class's own start needs
        if start > 3:
            assert minimal_terms(start - 1) > nt, (start, nt)            # and the class starts no later than it could
    assert pairs[-1][1] == minimal_terms(D_MAX), pairs                   # no row missing at the far end


def test_first_rows_are_the_builds_thresholds():
    pairs = classes()
    assert pairs[0] == (3, 38) and pairs[1] == (4, 30), pairs[:2]


def stops():
    with open(os.path.join(_native.CSRC, "lbl_kernels.hip")) as fh:
        m = re.search(r"#define LBL_FAR_STOPS \{([\d, ]+)\}", fh.read())
    assert m
    return [int(x) for x in m.group(1).split(",")]


def test_the_descents_stops_take_counts_that_hold_for_every_distance():
    """far_chunk leaves its chain only at the stops: a chunk at d half-spans takes the count of the table class of the last
    stop at or below d - never fewer terms than d needs, and the stops begin with the builds' thresholds."""
    pairs, st = classes(), stops()
    assert st[:2] == [3, 4] and st == sorted(set(st)) and st[-1] <= D_MAX, st
    for d in range(3, D_MAX + 1):
        stop = [s for s in st if s <= d][-1]
        nt = class_of(pairs, stop)[1]
        assert remainder(d, nt) <= LIMIT_EXACT, (d, stop, nt)
        assert nt >= class_of(pairs, d)[1]
