"""Graphs and a model for the tests of the class sort's payload (the bracket-list size of a candidate-stack entry above its
stack index, saturating at LMAX = 2^w - 1) and of the children sweep of k_capping.  Everything here is
decided by the CPU oracle's dump of a component; nothing needs a GPU."""
import numpy as np

from povu_amd import workloads as W
from test_oracle import dump_component

NIL = 0xFFFFFFFF
FIELD_CAP = 8              # bits the field has at most (LSZ_FIELD_CAP, par_kernels.hpp)
WIDTHS = (1, 2, 3)         # the hook's widths of the tests: LMAX = 1, 3, 7
FINISH_GROUP = 1024        # sorted positions a workgroup of k_class_finish_black takes (256 lanes, four each)
TOP_GROUP = 256            # ... of k_top_bracket (one each)


def concat(graphs):
    """The components of several graphs side by side (ids shifted so that they stay ascending)."""
    vid, v1, s1, v2, s2 = [], [], [], [], []
    off, id_off = 0, 0
    for g in graphs:
        vid.append(g.vid.astype(np.uint64) + id_off)
        v1.append(g.v1.astype(np.uint64) + off)
        v2.append(g.v2.astype(np.uint64) + off)
        s1.append(g.s1)
        s2.append(g.s2)
        off += g.n_vtx
        id_off = int(vid[-1].max()) + 1
    return W._mk(np.concatenate(vid), np.concatenate(v1), np.concatenate(s1), np.concatenate(v2), np.concatenate(s2))


def sized_components(sizes):
    """One component per entry of `sizes`, with exactly that many segments (= candidate-stack entries when it is decomposed,
    none when it has fewer than three): a chain a > a+1 > ... with a skip link over every third segment (a bubble)."""
    src, dst, base = [], [], 0
    for n in sizes:
        for i in range(n - 1):
            src.append(base + i)
            dst.append(base + i + 1)
            if i % 3 == 0 and i + 2 < n:
                src.append(base + i)
                dst.append(base + i + 2)
        base += n
    return W.from_plus_links(np.arange(1, base + 1), np.array(src, dtype=np.uint32), np.array(dst, dtype=np.uint32))


def random_connected(seed):
    """The stream of small connected random graphs of which some take the black-only pass and some do not."""
    n = 25 + 3 * seed
    return W.random_bidirected(n, int(n * (1.2 + 0.1 * (seed % 8))), 4242 + seed, connected=True)


def lmax(w):
    return (1 << w) - 1


def field_width(n_stack, cap=FIELD_CAP):
    """lsz_field (par_kernels.hpp): the bits a stack index below n_stack leaves free in 32, at most cap."""
    b = 1
    while b < 32 and (1 << b) <= n_stack:
        b += 1
    return min(32 - b, cap)


def components(g):
    """The oracle's dump of every component that is decomposed (it has a candidate stack)."""
    out, c = [], 0
    while True:
        d = dump_component(g, c)
        if d is None:
            return out
        if len(d["s_st_idx"]):
            out.append(d)
        c += 1


def list_sizes(d):
    """The size of the bracket list at every candidate-stack entry of one dumped component, in stack order: the brackets
    (back edges, capping and simplifying ones included) with their source inside the subtree of the entry's tree vertex -- the
    child end of its black edge -- and their target a proper ancestor of it.  A bracket (s, t) is live at every vertex on the
    tree path from s up to the child of t."""
    par = d["par"].astype(np.int64)
    live = np.zeros(len(par), dtype=np.int64)
    for s, t in zip(d["be_src"].tolist(), d["be_tgt"].tolist()):
        v, steps = s, 0
        while v != t:
            live[v] += 1
            v = int(par[v])
            steps += 1
            assert 0 <= v < len(par) and steps <= len(par), "a bracket's target is no ancestor of its source"
    return live[d["s_st_idx"].astype(np.int64) + 1]


def all_list_sizes(g):
    cs = components(g)
    return np.concatenate([list_sizes(d) for d in cs]) if cs else np.zeros(0, dtype=np.int64)


def n_stack(g):
    return sum(len(d["s_st_idx"]) for d in components(g))


def saturated(g, w):
    """Entries whose size does not fit a field of w bits (>= LMAX); all of them at w = 0."""
    return int((all_list_sizes(g) >= lmax(w)).sum())


def children_counts(d):
    """Children of every tree vertex of one dumped component."""
    par = d["par"]
    ok = par != NIL
    return np.bincount(par[ok].astype(np.int64), minlength=len(par))


def subtree_sizes(d):
    """Vertices in the subtree of every tree vertex (itself included); a parent's index is below its children's."""
    par = d["par"]
    sz = np.ones(len(par), dtype=np.int64)
    for v in range(len(par) - 1, -1, -1):
        if par[v] != NIL:
            assert par[v] < v
            sz[par[v]] += sz[v]
    return sz


# ---- builders
def towers(depth, n=3):
    """Nested bubbles, `depth` deep, n towers in a chain: the list sizes run from 1 up to depth + 1 and back under the one
    bracket that spans a tower."""
    return W.nested_towers(depth, n)


def valid_then_invalid(n_valid, invalid=(1, 2, 1)):
    """n_valid candidate-stack entries in two decomposed components, then segments of components that are not decomposed
    (fewer than three segments): their sort entries carry the NIL key and sit behind every valid one."""
    first = max(3, n_valid // 3)
    return sized_components([first, n_valid - first] + list(invalid))


def star(n_children, first_subtree=1, tail=2):
    """One segment whose right side has links to n_children chains: a branching tree vertex with that many children.  The
    first chain has first_subtree segments, the others `tail`; all of them end in one sink segment, so every chain but
    the one the tree takes closes with a back edge."""
    src, dst = [], []
    nxt = 1
    ends = []
    for k in range(n_children):
        n = first_subtree if k == 0 else tail
        src.append(0)
        dst.append(nxt)
        for i in range(n - 1):
            src.append(nxt + i)
            dst.append(nxt + i + 1)
        ends.append(nxt + n - 1)
        nxt += n
    sink = nxt
    for e in ends:
        src.append(e)
        dst.append(sink)
    return W.from_plus_links(np.arange(1, sink + 2), np.array(src, dtype=np.uint32), np.array(dst, dtype=np.uint32))


def broom(handle, chains, back=()):
    """Segments 0 .. handle - 1 in a chain; the right side of the last one has a link to the first segment of every dead-end
    chain of `chains` (so many segments each): its tree vertex branches into len(chains) children, in that order, and the
    subtree of a child is two vertices a segment.  `back`: dead-end chains whose LAST link enters the left side of segment
    handle - 1 as the handle's does: then that side branches too, into its black child first -- 1 + 2 sum(chains) vertices --
    and the chains of `back`."""
    src, dst = list(range(handle - 1)), list(range(1, handle))
    nxt = handle
    for n in chains:
        src.append(handle - 1)
        dst.append(nxt)
        for i in range(n - 1):
            src.append(nxt + i)
            dst.append(nxt + i + 1)
        nxt += n
    for n in back:
        for i in range(n - 1):
            src.append(nxt + i + 1)
            dst.append(nxt + i)
        src.append(nxt)
        dst.append(handle - 1)
        nxt += n
    return W.from_plus_links(np.arange(1, nxt + 1), np.array(src, dtype=np.uint32), np.array(dst, dtype=np.uint32))


def branching_vertices(d):
    """[(tree vertex, [subtree sizes of its children, in index order])] of one dumped component, for every vertex with two
    children or more."""
    cc, sz, par = children_counts(d), subtree_sizes(d), d["par"]
    return [(int(b), sz[np.nonzero(par == b)[0]].tolist()) for b in np.nonzero(cc >= 2)[0]]


def branching_last(n_children=3):
    """A chain whose LAST segment branches into n_children single segments: nothing of the tree lies behind the children
    of the branching vertex."""
    return broom(5, [1] * n_children)


def empty_slot_next_to_valid():
    """Components that are not decomposed (their tree-vertex slots keep size 0) in front of, between and behind decomposed
    ones with branching vertices."""
    return concat([sized_components([1, 2]), star(3, 2), sized_components([2, 1, 1]), broom(2, [4, 1]), sized_components([1]),
                   branching_last(2), sized_components([2])])
