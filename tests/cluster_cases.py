"""The inputs and the cases of the clustered calls' tests (tests/test_cluster_ref.py on the CPU, tests/test_gpu_cluster.py on the
GPU).  A case is (graph, sequences by vertex, Paths, reference prefixes, threshold in ppm).  The hand-made ones are chains of
layered sites (`chain`): a site lies between two boundary segments, its inner segments stand in layers, consecutive layers are
linked completely, so that the PVST does not split it further; a haplotype walks one segment of every layer (a looped segment
several times), or the deletion link.  test_cluster_ref.py asserts for every case that it is not vacuous: some site has fewer
clusters than exact alleles and some record is written."""
import functools
import os

import numpy as np

import vcf_ref as V
from povu_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "downstream_repetitive/popped-parent-child-rescue"
GFA = os.path.join(ROOT, "tests", "golden", "gfa", FIXTURE + ".gfa")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster_records.json")
HG1 = "HG1#1#chr1"


def _text(n, salt):
    return "".join("ACGT"[(salt * 7 + k * (salt % 3 + 1)) % 4] for k in range(n))


def chain(sites, walks, reverse=()):
    """(Links, sequences by vertex, Paths) of a chain of layered sites.  sites: dicts with `layers` (lists of names), `lens`
    (name -> bases, 1 when left out), `deletion` (a link entry > exit) and `loops` (names with a link to themselves).  walks: per
    haplotype and site the names it walks, in order, or None for the deletion.  Boundaries are one base long.  The haplotypes
    in `reverse` are written walking backwards."""
    ids, lens, links = {}, {}, set()

    def seg(key, ln=1):
        if key not in ids:
            ids[key] = len(ids) + 1
            lens[ids[key]] = ln
        return ids[key]
    for k, st in enumerate(sites):
        e = seg(("b", k))
        inner = [[seg((k, nm), st.get("lens", {}).get(nm, 1)) for nm in layer] for layer in st["layers"]]
        z = seg(("b", k + 1))
        for a, b in zip([[e]] + inner, inner + [[z]]):
            links |= {(x, y) for x in a for y in b}
        if st.get("deletion"):
            links.add((e, z))
        links |= {(ids[(k, nm)], ids[(k, nm)]) for nm in st.get("loops", ())}
    pieces = []
    for h, w in enumerate(walks):
        steps = [ids[("b", 0)]]
        for k, names in enumerate(w):
            steps += [ids[(k, nm)] for nm in (names or [])] + [ids[("b", k + 1)]]
        assert all((a, b) in links for a, b in zip(steps, steps[1:])), (h, steps)
        arr = np.array(steps, dtype=np.uint32)
        pieces.append((arr[::-1].copy(), np.ones(arr.size, np.uint8)) if h in reverse else (arr, np.zeros(arr.size, np.uint8)))
    vid = np.arange(1, len(ids) + 1, dtype=np.uint32)
    pairs = sorted(links)
    g = W.from_plus_links(vid, np.array([a - 1 for a, _ in pairs]), np.array([b - 1 for _, b in pairs]))
    return g, [_text(lens[v], v) for v in vid.tolist()], W._paths([f"hap{h}#1#chr1" for h in range(len(walks))], pieces)


# ---- the sites of the hand-made cases (every similarity below is I / U in bases)
# x three times against x twice: I = 2 * 2, U = 6 + 4 - 4: 2/3; y apart
MULTISET = dict(layers=[["x", "y"]], loops=["x"], lens=dict(x=2, y=5))
MULTISET_WALKS = [["x", "x", "x"], ["x", "x"], ["y"], ["x", "x", "x"]]
# bags of no key and of one key; x and w are empty segments: {} ~ {x} ~ {w} with U == 0, {y} apart
EMPTY = dict(layers=[["x", "w", "y"]], deletion=True, lens=dict(x=0, w=0, y=3))
EMPTY_WALKS = [None, ["x"], ["y"], ["w"]]
# two exact alleles, 8 / 10 similar: one cluster at 0.7, the site vanishes
VANISH = dict(layers=[["a", "a2"], ["b", "c"]], lens=dict(a=8))
VANISH_WALKS = [["a", "b"], ["a", "c"], ["a", "b"], ["a", "c"]]
# r0 = x m, r1 = y m (10 / 16 apart), u m is 10 / 14 to both: the tie goes to cluster 0
TIE = dict(layers=[["x", "y", "u"], ["m", "m2"]], lens=dict(x=3, y=3, u=1, m=10))
TIE_WALKS = [["x", "m"], ["y", "m"], ["u", "m"], ["y", "m"]]
# r0 = x m s, r1 = y m t (10 / 16 apart); y m s is 11 / 15 to r0 and 12 / 14 to r1: best fit is cluster 1, first fit 0
BEST = dict(layers=[["x", "y"], ["m", "m2"], ["s", "t"]], lens=dict(x=2, y=2, m=10))
BEST_WALKS = [["x", "m", "s"], ["y", "m", "t"], ["y", "m", "s"], ["x", "m", "s"]]


def _star():
    """130 parallel long segments behind one of two short ones: 130 clusters, and five haplotypes that join one through p2."""
    xs = [f"x{i}" for i in range(130)]
    st = dict(layers=[["p", "p2"], xs], lens=dict({x: 20 for x in xs}, p=1, p2=1))
    return [st], [[["p", x]] for x in xs] + [[["p2", xs[7 * j]]] for j in range(5)]


def _several(*pairs):
    sites = [s for s, _ in pairs]
    n = len(pairs[0][1])
    return sites, [[w[h] for _, w in pairs] for h in range(n)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(graph, sequences by vertex, Paths, reference prefixes, T)"""
    if name == "braid-chain":  # several sites, a haplotype walking backwards
        g = W.braid(5, 6, 3, seed=2)
        return g, W.random_sequences(g, 2, max_len=9), W.braid_haplotypes(5, 6, 3, 10, seed=2, mutate=0.1, skip=0.1, reverse_every=3), ("hap0#",), 800000
    if name.startswith("braid-"):  # one braid site of that many layers: bags of 0 (the deletion) and of `layers` keys
        layers = int(name[6:])
        g = W.braid(1, layers, 2, seed=layers)
        return g, W.random_sequences(g, layers, max_len=6), W.braid_haplotypes(1, layers, 2, 9, seed=layers, mutate=0.03, skip=0.15), ("hap0#",), 900000
    hand = {
        "multiset": (_several((MULTISET, MULTISET_WALKS)), {}, ("hap0#",), 600000),
        "empty-segments": (_several((EMPTY, EMPTY_WALKS)), {}, ("hap0#",), 1000000),
        "vanish": (_several((VANISH, VANISH_WALKS), (TIE, TIE_WALKS)), {}, ("hap0#",), 700000),
        "tie": (_several((TIE, TIE_WALKS)), {}, ("hap0#",), 700000),
        "best-fit": (_several((BEST, BEST_WALKS)), {}, ("hap0#",), 700000),
        "star": (_star(), {}, ("hap0#",), 900000),
        "backward-reference": (_several((BEST, BEST_WALKS), (EMPTY, EMPTY_WALKS)), dict(reverse=(0, 2)), ("hap0#",), 700000),
        "own-ref": (_several((BEST, BEST_WALKS), (TIE, TIE_WALKS)), {}, ("hap2#",), 700000),  # hap2's allele joins, never founds
        "own-ref-backwards": (_several((BEST, BEST_WALKS), (TIE, TIE_WALKS)), dict(reverse=(2,)), ("hap2#",), 700000),
        "two-references": (_several((BEST, BEST_WALKS), (MULTISET, MULTISET_WALKS)), {}, ("hap0#", "hap1#", "hap2#"), 700000),
    }
    (sites, walks), kw, refs, t = hand[name]
    g, seqs, p = chain(sites, walks, **kw)
    return g, seqs, p, refs, t


CASES = ("braid-64", "braid-65", "braid-129", "braid-chain", "multiset", "empty-segments", "vanish", "tie", "best-fit", "star",
         "backward-reference", "own-ref", "own-ref-backwards", "two-references")
PRUNE_CASE = "braid-chain"  # a haplotype on the deletion link has a bag of no weight: the weights alone rule its pairs out


def tables(name):
    """(names, step lists, {segment id: sequence}) of a case, as the restatements take them."""
    g, seqs, p, _, _ = case(name)
    return list(p.names), [p.steps(k) for k in range(len(p))], dict(zip(g.vid.tolist(), seqs))


def fixture_tables():
    return V.read_gfa(GFA)
