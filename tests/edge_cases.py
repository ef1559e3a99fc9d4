"""The lower edge and the id range of the query and call family's tests: calls that end with no query, no traversal, no
record, no kept site, one slot, one vertex, inversion heads without a run, runs without a base, paths without a step -- and
graphs whose segment ids take every decimal width from 1 to 10 digits, on both sides of 2^31.  What each case must reach is
stated on the restatements and the CPU oracle alone (tests/test_edge_inputs.py, no GPU); the GPU tests
(tests/test_gpu_edges.py) put every case through their files' own comparisons."""
import functools

import numpy as np

import prim_cases as PC
import test_gpu_inversions as TI
from povu_amd import workloads as W
from test_gpu_norm import chain

WIDE_TOP = 4294967294  # the largest legal segment id
LONG = 66              # steps of the long allele and of the long inversion run of long_wide_case


class Case:
    """(graph, sequences, paths) with the reference prefixes of its calls: `refs` is a list of prefix lists, one call each."""

    def __init__(self, g, seqs, paths, refs, max_steps=65536, popped=None):
        self.g, self.seqs, self.paths, self.refs, self.max_steps = g, list(seqs), paths, refs, max_steps
        self.popped = popped or dict(max_level=0, max_ref_length=0, max_allele_length=0)

    @property
    def names(self):
        return list(self.paths.names)

    @property
    def steps(self):
        return [self.paths.steps(k) for k in range(len(self.paths))]

    @property
    def sq(self):
        return dict(zip(self.g.vid.tolist(), self.seqs))

    def triple(self):
        return self.g, self.seqs, self.paths


def hap_names(n):
    return [f"hap{k}#1#chr1" for k in range(n)]


def paths_of_walks(names, walks):
    return W._paths(names, [([i for i, _ in st], [r for _, r in st]) for st in walks])


def from_walks(n_seg, walks, names=None, more=()):
    """(graph, paths): segments 1 .. n_seg, one link for every pair of consecutive steps of `walks` (and of `more`, walks that
    are no path)."""
    seen, v1, s1, v2, s2 = set(), [], [], [], []
    for st in list(walks) + list(more):
        for a, b in zip(st, st[1:]):
            key = (a, b)
            back = ((b[0], 1 - b[1]), (a[0], 1 - a[1]))  # the same link read from its other end
            if key not in seen and back not in seen:
                seen.add(key)
                v1.append(a[0] - 1), s1.append(W.L if a[1] else W.R), v2.append(b[0] - 1), s2.append(W.R if b[1] else W.L)
    g = W._mk(np.arange(1, n_seg + 1), v1, s1, v2, s2)
    return g, paths_of_walks(names or hap_names(len(walks)), walks)


def fwd(ids):
    return [(int(i), 0) for i in ids]


def back(walk):
    """The walk the other way round."""
    return [(i, 1 - r) for i, r in reversed(walk)]


def beside(g, n_more):
    """`g` and a linear chain of n_more further segments as a second component: (graph, ids of the chain)."""
    v = g.n_vtx
    ids = np.arange(v + 1, v + n_more + 1)
    a = np.arange(v, v + n_more - 1)
    return W._mk(np.concatenate([g.vid, ids]), np.concatenate([g.v1, a]), np.concatenate([g.s1, np.full(n_more - 1, W.R)]),
                 np.concatenate([g.v2, a + 1]), np.concatenate([g.s2, np.full(n_more - 1, W.L)])), ids.tolist()


def bases(g, seed):
    """Short sequences, none empty."""
    return W.random_sequences(g, seed, max_len=5, empty=0.0)


# ---- zero and one

def no_sites():
    g, seqs, p = chain([("s", t, 0) for t in ("AC", "G", "TTA", "C", "GA")], [[], []], reversed_copy=True)
    return Case(g, seqs, p, [["hap0"]])


def no_sites_wide():
    """... under ids of 1, 7, 8 and 10 digits, on both sides of 2^31."""
    case = no_sites()
    g, p = relabel(case.g, case.paths, [7, 1000000, 99999999, 2147483648, WIDE_TOP])
    return Case(g, case.seqs, p, case.refs)


def untouched_sites():
    g, line = beside(W.chain_of_bubbles(3), 5)
    walks = [fwd(line), fwd(line), back(fwd(line))]
    return Case(g, bases(g, 2), paths_of_walks(hap_names(3), walks), [["hap0"]])


def all_agree():
    g = W.chain_of_bubbles(3)
    walk = fwd([1, 2, 4, 5, 7, 8, 10])
    return Case(g, bases(g, 3), paths_of_walks(hap_names(3), [walk] * 3), [["hap0"]])


def uncallable():
    """The reference enters the first bubble and ends inside it; the others cross all three, each by another allele."""
    g = W.chain_of_bubbles(3)
    walks = [fwd([1, 2]), fwd([1, 2, 4, 5, 7, 8, 10]), fwd([1, 3, 4, 6, 7, 9, 10]), fwd([1, 4, 7, 10])]
    return Case(g, bases(g, 4), paths_of_walks(hap_names(4), walks), [["hap0"]])


def one_path():
    g = W.chain_of_bubbles(3)
    return Case(g, bases(g, 5), paths_of_walks(["only#1#chr1"], [fwd([1, 2, 4, 6, 7, 10])]), [["only"]])


def self_inverting():
    """One path: through a bubble, on to segment 7 and back over 6 and 5 the other way round."""
    walk = fwd([1, 2, 4, 5, 6, 7]) + [(6, 1), (5, 1)]
    g, p = from_walks(7, [walk], names=["only#1#chr1"], more=[fwd([1, 3, 4])])
    return Case(g, bases(g, 6), p, [["only"]])


def single_snp():
    g, seqs, p = chain([("s", "A", 0), ("b", ["C", "G"], False), ("s", "T", 0)], [[1], [2]])
    return Case(g, seqs, p, [["hap0"], ["hap0", "hap1"]])


def runs_of_one():
    """The second path walks segments 2, 5 and 7 of the reference the other way round, each between forward steps."""
    ref = fwd(range(1, 9))
    other = [(i, int(i in (2, 5, 7))) for i in range(1, 9)]
    g, p = from_walks(8, [ref, other])
    return Case(g, bases(g, 7), p, [["hap0"]])


def runs_too_long():
    """Two runs of three steps, under max_steps = 2."""
    ref = fwd(range(1, 10))
    other = fwd([1]) + back(fwd([2, 3, 4])) + fwd([5]) + back(fwd([6, 7, 8])) + fwd([9])
    g, p = from_walks(9, [ref, other])
    return Case(g, bases(g, 8), p, [["hap0"]], max_steps=2)


def baseless_runs():
    """Runs of three and of two steps over segments without a base."""
    ref = fwd(range(1, 10))
    other = fwd([1]) + back(fwd([2, 3, 4])) + fwd([5, 6]) + back(fwd([7, 8])) + fwd([9])
    g, p = from_walks(9, [ref, other])
    return Case(g, ["A", "", "", "", "CG", "T", "", "", "G"], p, [["hap0"]])


def all_empty_sequences():
    g, seqs, p = chain([("s", "", 0), ("b", ["", ""], False), ("s", "", 0)], [[1], [2]], reversed_copy=True)
    return Case(g, seqs, p, [["hap0"]])


def empty_allele_among_others():
    """A site behind a segment without a base that one haplotype skips: the record is anchored on nothing, so the skip's text
    is empty beside two texts that differ.  The left-normalisation leaves such a record as it is and compares nothing."""
    g, seqs, p = chain([("s", "GG", 0), ("s", "", 0), ("b", ["AC", "AG"], True), ("s", "T", 0)], [[1], [2], [0]])
    return Case(g, seqs, p, [["hap0"]])


def popped_drops_all():
    g, seqs, p = chain([("s", "A", 0), ("b", ["ACGTACGT", "C"], False), ("s", "T", 0)], [[1], [2]])
    return Case(g, seqs, p, [["hap0"]], popped=dict(max_level=0, max_ref_length=1, max_allele_length=0))


ZERO_STEP_NAMES = ["e0#1#chr1", "a#1#chr1", "b#1#chr1", "e1#1#chr1", "c#1#chr1", "e2#1#chr1"]


def zero_step_paths(second_reference=False):
    """Paths without a step first, in the middle and last among three haplotypes of a chain; with second_reference the one in
    the middle is a reference path as well."""
    g = W.chain_of_bubbles(3)
    walks = [[], fwd([1, 2, 4, 5, 7, 8, 10]), fwd([1, 3, 4, 6, 7, 10]), [], back(fwd([1, 4, 5, 7, 9, 10])), []]
    return Case(g, bases(g, 9), paths_of_walks(ZERO_STEP_NAMES, walks), [["a#", "e1#"] if second_reference else ["a#"]])


def one_step_paths():
    """Two haplotypes of a chain and six paths of one step: four the reverse of a step of the reference (its first, its last,
    two in between), two a forward step."""
    g = W.chain_of_bubbles(3)
    walks = [fwd([1, 2, 4, 5, 7, 8, 10]), fwd([1, 3, 4, 6, 7, 10])] + [[s] for s in ((1, 1), (10, 1), (4, 1), (5, 1), (2, 0), (6, 0))]
    return Case(g, bases(g, 10), paths_of_walks(hap_names(len(walks)), walks), [["hap0"]])


def one_vertex(ident=5):
    g = W._mk(np.array([ident]), [], [], [], [])
    return Case(g, ["ACG"], paths_of_walks(hap_names(2), [[(ident, 0)], [(ident, 1)]]), [["hap0"]])


MINIMAL = dict(no_sites=no_sites, no_sites_wide=no_sites_wide, untouched_sites=untouched_sites, all_agree=all_agree, uncallable=uncallable, one_path=one_path,
               self_inverting=self_inverting, single_snp=single_snp, runs_of_one=runs_of_one, runs_too_long=runs_too_long,
               baseless_runs=baseless_runs, all_empty_sequences=all_empty_sequences, empty_allele_among_others=empty_allele_among_others, popped_drops_all=popped_drops_all,
               zero_step_paths=zero_step_paths, one_step_paths=one_step_paths, one_vertex=one_vertex)


# ---- wide ids

def wide_ids(v):
    """`v` ascending segment ids that hold every decimal width from 1 to 10, among them 1, 2^31 - 1, 2^31 and 4294967294:
    at most v // 20 (at least one) of each width below 10, the rest of 10 digits on both sides of 2^31."""
    assert v >= 16
    out = []
    for w in range(1, 10):
        lo, room = 10 ** (w - 1), 9 * 10 ** (w - 1)
        n = min(room, max(1, v // 20))
        out += [lo + (k * room) // n for k in range(n)]
    n = v - len(out)
    ten = np.linspace(10 ** 9, WIDE_TOP, n).astype(np.int64)
    at = int(np.searchsorted(ten, 2 ** 31))  # 1 <= at < n - 1: both neighbours of 2^31 stay inside, the ends stay the ends
    ten[at - 1], ten[at] = 2 ** 31 - 1, 2 ** 31
    out += ten.tolist()
    assert len(set(out)) == v and out == sorted(out) and out[0] == 1 and out[-1] == WIDE_TOP
    return np.array(out, dtype=np.uint32)


def relabel(g, paths, ids):
    """The same graph and paths with the segment of vertex index k called ids[k] (ascending, as g.vid is)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    assert ids.size == g.n_vtx and np.all(np.diff(ids.astype(np.int64)) > 0)
    at = np.searchsorted(g.vid, paths.ids)
    assert np.array_equal(g.vid[at], paths.ids)
    return W._mk(ids, g.v1, g.s1, g.v2, g.s2), W.Paths(list(paths.names), paths.off.copy(), ids[at], paths.rev.copy())


def id_map(g, ids):
    """{old id: new id} of relabel(g, ., ids)."""
    return dict(zip(g.vid.tolist(), np.asarray(ids).tolist()))


def long_wide_case():
    """Twenty SNPs in a row (segments 1 .. 60, which take the ids of one to nine digits under wide_ids), then a bubble whose
    first allele is LONG one-base segments and whose second is one; hap0 takes the long allele, hap1 the short one, hap2 walks
    the long one the other way round: a third allele of LONG steps and an inversion run of LONG steps.  Under wide_ids every
    segment of the long allele has a 10-digit id."""
    x = [i for u in range(20) for i in (3 * u + 1, 3 * u + 2)]
    y = [i for u in range(20) for i in (3 * u + 1, 3 * u + 3)]
    f, first = 61, 62
    long = list(range(first, first + LONG))
    short, g_ = first + LONG, first + LONG + 1
    tail = [g_ + 1, g_ + 2]
    walks = [fwd(x + [f] + long + [g_] + tail), fwd(y + [f, short, g_] + tail), fwd(x + [f]) + back(fwd(long)) + fwd([g_] + tail)]
    g, p = from_walks(tail[-1], walks)
    rng = np.random.default_rng(12)
    seqs = ["ACGT"[int(x)] for x in rng.integers(0, 4, size=g.n_vtx)]
    return Case(g, seqs, p, [["hap0"]])


def _wide_bases():
    g, p = TI.chain_case()
    yield "chain", Case(g, W.random_sequences(g, 1, max_len=8), p, [["sample0#1"]])
    g, p = TI.inverted_case()
    yield "inverted", Case(g, W.random_sequences(g, 3, max_len=8), p, [["sample0#1"]])
    g, seqs, p = PC.chain_case()
    yield "prim_chain", Case(g, seqs, p, [list(PC.CHAIN_REFS)])
    g = W.bubble_zoo(6, 8, 2)
    # 120 short walks, 31 of them references (walk1, walk10 .. walk19, walk100 .. walk119): few paths cross a site of the zoo
    yield "zoo", Case(g, W.random_sequences(g, 7, max_len=8), W.random_walk_paths(g, 120, 30, seed=5), [["walk1"]])
    yield "long", long_wide_case()


@functools.lru_cache(maxsize=None)
def wide_cases():
    """{name: (the case as it is, the same case under wide_ids, the ids)}."""
    out = {}
    for name, case in _wide_bases():
        ids = wide_ids(case.g.n_vtx)
        g, p = relabel(case.g, case.paths, ids)
        out[name] = (case, Case(g, case.seqs, p, case.refs, case.max_steps, case.popped), ids)
    return out


WIDE = ("chain", "inverted", "prim_chain", "zoo", "long")


def ids_of_at(text):
    """The segment ids of an AT string."""
    return [int(x) for x in text.replace("<", ">").replace(",", ">").split(">") if x]
