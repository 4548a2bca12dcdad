"""CPU: the term counts of the far-field series' distance classes stay inside the remainder bound.

A chunk of far lines whose nearest line is d half-spans from the span centre has rho <= 1/d and takes NT terms; the
remainder of the series is then at most (lbl_kernels.hip, "Truncation after FF_NT terms", with the factor of the
amplitude's own expansion)

    rho^NT (NT (1 - rho) + 1) (1 + rho)^2 / (1 - rho)^2.

Exact mode holds every class to what the class from 3 half-spans on (38 terms) already meets, 7.8e-17: below half an ulp
of the line's own smallest term on the span.  Budget mode's classes stay below its 5.9e-10.  The pairs are read from the
two table lines of the kernel source, so a count lowered there without the bound behind it fails here.
"""
import os
import re

from pyrad_amd import _native

LIMIT_EXACT = 7.8e-17
LIMIT_BUDGET = 5.9e-10


def remainder(d, nt):
    rho = 1.0 / d
    return rho ** nt * (nt * (1.0 - rho) + 1.0) * (1.0 + rho) ** 2 / (1.0 - rho) ** 2


def classes(name):
    with open(os.path.join(_native.CSRC, "lbl_kernels.hip")) as fh:
        text = fh.read()
    m = re.search(r"constexpr int %s\[(\d+)\]\[2\] = \{(.*)\};" % name, text)
    assert m, name
    pairs = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", m.group(2))]
    assert len(pairs) == int(m.group(1)) >= 4, pairs
    return pairs


def test_exact_mode_classes_stay_below_half_an_ulp():
    pairs = classes("kFarClassExact")
    assert pairs[0] == (3, 38)
    for d, nt in pairs:
        r = remainder(d, nt)
        print("d >= %d: %d terms, remainder %.2e" % (d, nt, r))
        assert r <= LIMIT_EXACT, (d, nt, r)
        assert remainder(d, nt - 1) > LIMIT_EXACT * 0.2, (d, nt)       # (and no class carries terms it has no use for)


def test_budget_mode_classes_stay_below_the_budget():
    for d, nt in classes("kFarClassBudget"):
        assert remainder(d, nt) <= LIMIT_BUDGET, (d, nt, remainder(d, nt))


def test_counts_do_not_increase_with_distance():
    for name in ("kFarClassExact", "kFarClassBudget"):
        pairs = classes(name)
        assert all(a[0] < b[0] for a, b in zip(pairs, pairs[1:])), pairs          # nearest first
        assert all(a[1] >= b[1] for a, b in zip(pairs, pairs[1:])), pairs
