"""The inputs of the untangled calls' tests (tests/golden/gfa/untangle/vntr.gfa, expected lines in
tests/golden/untangle_records.json; looped sites built on povu_amd.workloads.vntr_haplotypes' graph): what
test_untangle_ref.py, test_untangle_core.py, test_untangle_writer.py and test_gpu_untangle.py share."""
import json
import os

import numpy as np

import cohort_cases as CC
import untangle_ref as U
from povu_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = "untangle/vntr"
GFA = os.path.join(GOLDEN, "gfa", "untangle", "vntr.gfa")
ALIGN_CASES = os.path.join(GOLDEN, "untangle_align_cases.json")
ALIGN_LENGTHS = (1, 2, 32, 33, 63, 64)
ALIGN_SEED = 20261020


def golden():
    return json.load(open(os.path.join(GOLDEN, "untangle_records.json")))


def looped_paths(names, units, reverse=()):
    """(graph, paths) of one loop site (vntr_haplotypes' shape: flank 1, entry 2, units 3 | 4, exit 5, flank 6): path k walks
    the site once per entry of units[k], through unit 3 + that entry; the paths whose index is in `reverse` walk backwards."""
    g, _ = W.vntr_haplotypes(1, 1, 1, 0)
    pieces = []
    for k, us in enumerate(units):
        ids = [1]
        for u in us:
            ids += [2, 3 + int(u), 5]
        ids.append(6)
        w = np.asarray(ids, dtype=np.uint32)
        if k in reverse:
            pieces.append((w[::-1].copy(), np.ones(w.size, dtype=np.uint8)))
        else:
            pieces.append((w, np.zeros(w.size, dtype=np.uint8)))
    return g, W._paths(list(names), pieces)


def two_paths(n, m, seed):
    """One site the reference laps n times and one haplotype m times, units drawn with `seed`."""
    rng = np.random.default_rng(seed)
    return looped_paths(["ref#1#c", "hap#1#c"], [rng.integers(0, 2, size=n).tolist(), rng.integers(0, 2, size=m).tolist()])


def wide_site(seed=7):
    """One loop site walked by the 263 paths of the wide cohort's names (131 samples, 261 slots, two slots of two contigs),
    1 .. 5 laps each, every fifth path backwards."""
    names = CC.wide_names()
    rng = np.random.default_rng(seed)
    units = [rng.integers(0, 2, size=int(rng.integers(1, 6))).tolist() for _ in names]
    return looped_paths(names, units, reverse={k for k in range(len(names)) if k % 5 == 4 and not names[k].startswith(CC.REF_LOW)})


def sequences(g, seed=3):
    return W.random_sequences(g, seed, max_len=4, empty=0.0)


def align_cases():
    """The cases of tests/golden/untangle_align_cases.json, regenerated: every pair of ALIGN_LENGTHS with symbols drawn from
    three, then per pair of lengths the all-equal and the all-different extremes, each with the restatement's partners."""
    rng = np.random.default_rng(ALIGN_SEED)
    cases = []
    for n in ALIGN_LENGTHS:
        for m in ALIGN_LENGTHS:
            cases.append(([int(x) for x in rng.integers(0, 3, size=n)], [int(x) for x in rng.integers(0, 3, size=m)]))
    for n in ALIGN_LENGTHS:
        for m in ALIGN_LENGTHS:
            cases.append(([7] * n, [7] * m))
            cases.append((list(range(n)), list(range(100, 100 + m))))
    out = []
    for a, b in cases:
        partner, extra, cost = U.align(a, b)
        out.append(dict(a=a, b=b, partner=[-1 if x is None else x for x in partner], extra=extra, cost=cost))
    return out
