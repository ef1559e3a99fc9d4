"""The inputs and the cases of the region calls' tests (tests/test_region_ref.py on the CPU, tests/test_gpu_region.py on the
GPU): small workloads, the regions stated on them in bases of a path, and per case the mode of the call.  A case is
(workload, mode, regions, options); the regions are (name, start, end) tuples, [start, end) 1-based.  test_region_ref.py asserts
for every case of CASES that it is not vacuous: some records stay and some go."""
import functools
import os

import edge_cases as EC
import vcf_ref as V
from povu_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "downstream_repetitive/popped-parent-child-rescue"
GFA = os.path.join(ROOT, "tests", "golden", "gfa", FIXTURE + ".gfa")
GOLDEN = os.path.join(ROOT, "tests", "golden", "region_records.json")
HG1, HG2, HG3 = "HG1#1#chr1", "HG2#1#chr1", "HG3#1#chr1"
# the fixture: HG1 = 0,1,2,3,4,5, HG2 = 0,5, HG3 = 0,1,2,6,4,5, one base a segment; sites >0>5 and >2>4.  Region(s) -> the
# sites whose records remain (INTEGRATION.md "Region calls")
FIXTURE_ROWS = {
    "second-boundary-of-the-child": ([(HG1, 3, 4)], [">2>4"]),
    "first-base": ([(HG1, 1, 2)], [">0>5"]),
    "an-inner-segment": ([(HG1, 2, 3)], []),
    "both-right-ends": ([(HG1, 5, 7)], [">0>5", ">2>4"]),
    "on-a-haplotype": ([(HG2, 2, 3)], [">0>5"]),
    "segment-6-is-no-boundary": ([(HG3, 4, 5)], []),
    "beyond-the-end": ([(HG1, 7, 9)], []),
    "two-regions": ([(HG1, 1, 2), (HG1, 3, 4)], [">0>5", ">2>4"]),
}


@functools.lru_cache(maxsize=None)
def workload(name):
    """(graph, sequences by vertex, Paths, reference prefixes)"""
    if name == "chain":  # 181 segments: the marks span six words
        g = W.chain_of_bubbles(60)
        return g, W.random_sequences(g, 4, max_len=5), W.pansn(W.chain_haplotypes(60, 9, seed=3), samples=5), ("sample0#1",)
    if name == "backwards":  # every second haplotype walks backwards, the reference among them
        g = W.chain_of_bubbles(60)
        return g, W.random_sequences(g, 6, max_len=5), W.pansn(W.chain_haplotypes(60, 9, seed=5, reverse_every=2), samples=5), ("sample0#2",)
    if name == "vntr":  # loop sites: a segment occurs several times on a path
        g, p = W.vntr_haplotypes(12, 6, 4, 7, reverse_every=3)
        return g, W.random_sequences(g, 5, max_len=4, empty=0.0), p, ("hap0#",)
    if name == "wide":  # segment ids of one to ten digits: a vertex index is not its id
        c = EC.wide_cases()["chain"][1]
        return c.g, c.seqs, c.paths, tuple(c.refs[0])
    if name == "inverted":
        g = W.chain_of_bubbles(40)
        base = W.chain_haplotypes(40, 6, seed=2, reverse_every=0)
        return g, W.random_sequences(g, 3, max_len=5), W.pansn(W.inverted_haplotypes(base, 14, 2, 6, seed=4, keep=(0,)), samples=3), ("sample0#1",)
    if name == "skip":
        g = W.skip_nested(6, 2)
        return g, W.random_sequences(g, 1, max_len=4), W.skip_haplotypes(6, 2, 8, seed=1), ("hap0#",)
    if name == "tandem":
        g, seqs = W.tandem_indels(12, 1, max_copies=8, max_seg=10)
        return g, seqs, W.tandem_haplotypes(12, 1, 6, max_copies=8, max_seg=10), ("hap0#",)
    if name == "complex":
        g, seqs = W.complex_alleles(16, 1)
        return g, seqs, W.complex_haplotypes(16, 1, 6), ("hap0#",)
    raise KeyError(name)


def tables(name):
    """(names, step lists, {segment id: sequence}) of a workload, as the restatements take them."""
    g, seqs, p, _ = workload(name)
    return list(p.names), [p.steps(k) for k in range(len(p))], dict(zip(g.vid.tolist(), seqs))


def layout(name, k):
    """Per step of path k: (segment id, its first position, the position behind its last), a segment without bases one position."""
    _, paths, sq = tables(name)
    out, off = [], 0
    for seg, _rev in paths[k]:
        ln = len(sq[seg])
        out.append((int(seg), off + 1, off + 1 + max(ln, 1)))
        off += ln
    return out


def part(name, k, lo, hi):
    """The region [lo, hi) of path k's bases, as fractions."""
    names = tables(name)[0]
    total = layout(name, k)[-1][2] - 1
    return names[k], 1 + int(total * lo), max(2 + int(total * lo), 1 + int(total * hi))


def _chain_boundary():
    """A boundary segment (3 i + 1) of the chain's reference path with three bases or more, near the middle: (first, behind)."""
    return next((a, b) for seg, a, b in layout("chain", 0) if seg % 3 == 1 and seg > 80 and b - a >= 3)


def _edge_regions():
    """Regions whose start or end sits on, one before and one behind the first and the last base of a boundary segment."""
    name = tables("chain")[0][0]
    first, behind = _chain_boundary()
    last = behind - 1
    far_left, far_right = layout("chain", 0)[20][1], layout("chain", 0)[-20][1]
    out = {}
    for what, at in (("first", first), ("last", last)):
        for d in (-1, 0, 1):
            out[f"start-{what}{d:+d}"] = [(name, at + d, far_right)]
            out[f"end-{what}{d:+d}"] = [(name, far_left, at + d)]  # (exclusive: at + 1 is the first end that holds `at`)
    out["strictly-inside-a-boundary"] = [(name, first + 1, first + 2)]
    return out


def _second_lap():
    """The vntr reference's second walk of a site's entry segment alone: the other occurrences lie outside."""
    lay = layout("vntr", 0)
    for site in range(12):
        hits = [(a, b) for seg, a, b in lay if seg == 5 * site + 2]
        if len(hits) >= 3:
            return [(tables("vntr")[0][0], hits[1][0], hits[1][1])]
    raise AssertionError("no site is walked three times")


def _cases():
    n = tables("chain")[0]
    c = {"chain-middle": ("chain", "plain", [part("chain", 0, 0.4, 0.6)], {})}
    for k, r in _edge_regions().items():
        c["chain-" + k] = ("chain", "plain", r, {})
    c["chain-overlapping"] = ("chain", "plain", [part("chain", 0, 0.2, 0.4), part("chain", 0, 0.3, 0.5)], {})
    c["chain-two-paths"] = ("chain", "plain", [part("chain", 0, 0.1, 0.2), part("chain", 4, 0.7, 0.8)], {})
    c["chain-70-regions"] = ("chain", "plain", [(n[0], 2 + 2 * j, 3 + 2 * j) for j in range(70)], {})
    c["chain-on-a-haplotype"] = ("chain", "plain", [part("chain", 5, 0.45, 0.6)], {})
    c["chain-on-a-backward-haplotype"] = ("chain", "plain", [part("chain", 3, 0.1, 0.3)], {})
    c["chain-tier2"] = ("chain", "plain", [part("chain", 0, 0.4, 0.6)], dict(tier2=True))
    c["backwards-reference"] = ("backwards", "plain", [part("backwards", 1, 0.3, 0.5)], {})
    c["backwards-from-a-forward-path"] = ("backwards", "plain", [part("backwards", 0, 0.3, 0.5)], {})
    c["vntr-second-lap"] = ("vntr", "plain", _second_lap(), {})
    c["vntr-untangle"] = ("vntr", "untangle", [part("vntr", 0, 0.3, 0.6)], {})
    c["vntr-untangle-backward-path"] = ("vntr", "untangle", [part("vntr", 2, 0.3, 0.6)], {})
    c["wide-ids"] = ("wide", "plain", [part("wide", 0, 0.4, 0.6)], {})
    c["inversions"] = ("inverted", "inversions", [part("inverted", 0, 0.3, 0.6)], {})
    c["nested"] = ("skip", "nested", [part("skip", 0, 0.3, 0.6)], {})
    c["top-level-only"] = ("skip", "top-level-only", [part("skip", 0, 0.3, 0.6)], {})
    c["popped"] = ("skip", "popped", [part("skip", 0, 0.3, 0.6)], dict(max_level=0, max_ref_length=6, max_allele_length=6))
    c["left-normalized"] = ("tandem", "left-normalized", [part("tandem", 0, 0.3, 0.6)], {})
    c["decomposed"] = ("complex", "decomposed", [part("complex", 0, 0.3, 0.6)], {})
    c["merged"] = ("complex", "merged", [part("complex", 0, 0.3, 0.6)], {})
    return c


CASES = _cases()


def fixture_tables():
    return V.read_gfa(GFA)
