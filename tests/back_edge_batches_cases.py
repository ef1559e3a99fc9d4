"""Graphs for the tests of the batched count phase of k_back_edges (tree_kernels.hip): a lane takes BE_ITER = 8 sides, 256 apart,
BE_BATCH = 4 at a time, and a workgroup BE_SIDES = 2 048 consecutive sides.  The builders put ONE side with a chosen number of
slots and back edges on a chosen place of that grid; the CPU test (test_back_edge_batches_inputs.py) asks the oracle whether
every builder makes what its name says."""
import numpy as np

from povu_amd import workloads as W
from test_gpu_bridge_stretch import graph, star
from test_gpu_gather_batches import fan, loops_and_parallels, small_around
from test_gpu_root_bit import mixed, ring
from test_gpu_stack_lookups import concat, sized_components
from test_oracle import dump_component

l, r = W.L, W.R
LANE, BATCH, GROUP = 256, 4 * 256, 2048          # sides: one iteration of a workgroup's lanes, one batch, one workgroup
EDGE_SEGMENTS = [127, 128, 129, 511, 512, 513, 1023, 1024, 1025]  # 2 n sides: on either side of the three edges
SLOTS = [1, 2, 3, 4, 5, 6, 8, 9]                  # slots on the fat side; it has slots - 1 back edges (0, 1, 2, 3, 4, 5, 7, 8)


def tail_fan(n, slots, last_side=True, parallel=0):
    """A chain 0 > 1 > ... > n-1 whose LAST segment is entered through its r side (last_side: the last side of the graph) or
    its l side (the last but one: for n = 1 025 the first side of the second workgroup), and slots - 1 more links from the
    segments right in front of it into that side: the side has `slots` slots (+ `parallel`: the first extra link that many
    times more) and slots - 1 ordinary back edges, all of them leaving its tree vertex."""
    e = r if last_side else l
    links = [(i, r, i + 1, l) for i in range(n - 2)] + [(n - 2, r, n - 1, e)]
    extra = [(n - 3 - i, r, n - 1, e) for i in range(slots - 1)]
    links += extra + extra[:1] * parallel
    return graph(n, links)


def fat_side(g_n, last_side=True):
    """(segment, side) of the side tail_fan(n, ...) makes fat."""
    return g_n - 1, (r if last_side else l)


def side_links(g):
    """Slots per side, side = 2 * segment + (0 = l, 1 = r)."""
    s1 = np.where(g.s1 == l, 0, 1).astype(np.int64)
    s2 = np.where(g.s2 == l, 0, 1).astype(np.int64)
    return np.bincount(np.concatenate([2 * g.v1.astype(np.int64) + s1, 2 * g.v2.astype(np.int64) + s2]), minlength=2 * g.n_vtx)


def tree_vertex_of(d, g, seg, side):
    """Tree vertex of a side in the oracle's dump of the component that holds it (typ: 0 = l, 1 = r, 2 = dummy root)."""
    hit = np.flatnonzero((d["gid"] == g.vid[seg]) & (d["typ"] == (0 if side == l else 1)))
    assert hit.size == 1
    return int(hit[0])


def ordinary_back_edges_of(d, v):
    """Ordinary back edges (type 0: those of from_bd, what k_back_edges writes) that leave tree vertex v."""
    return int(((d["be_src"][: d["n_be0"]] == v)).sum())


def linkless_places(g, tips=None):
    """Where the sides without a link of the decomposed components of g sit in their trees: a set out of 'root',
    'child of the root', 'child of the dummy root', 'deeper'."""
    n_links = side_links(g)
    out, c = set(), 0
    while True:
        d = dump_component(g, c, tips=tips)
        if d is None:
            return out
        c += 1
        if not len(d["gid"]):
            continue
        seg_of = {int(v): k for k, v in enumerate(g.vid)}
        dummy = d["typ"][0] == 2
        for v in range(len(d["gid"])):
            if d["typ"][v] == 2:
                continue
            if n_links[2 * seg_of[int(d["gid"][v])] + int(d["typ"][v])]:
                continue
            par = int(d["par"][v])
            if par == 0xFFFFFFFF:
                out.add("root")
            elif par == 0:
                out.add("child of the dummy root" if dummy else "child of the root")
            else:
                out.add("deeper")


def linkless():
    """Sides without a link on every place of a tree: the tips of a chain (the first one hangs off the dummy root, the last
    one lies deep), a ring with a tail (no dummy root: the tail's tip lies deep), a star whose hub roots the tree at a side
    without a link, and the mixed components of test_gpu_root_bit."""
    ring_tail = graph(7, [(i, r, (i + 1) % 5, l) for i in range(5)] + [(2, r, 5, l), (5, r, 6, l)])
    hub_root = graph(4, [(0, r, 1, l), (0, r, 2, l), (0, r, 3, l), (1, r, 1, r), (2, r, 2, r), (3, r, 3, r)])
    return concat([sized_components([5]), ring_tail, hub_root, mixed()])


def linkless_no_tips():
    """... and where no segment is declared a tip (NO_TIPS: the caller hands an all-zero tip array to the upload and to the
    oracle): no dummy root, the tree starts at the l side of the first segment of a component.  First component: that side
    has no link (the root itself, with its back edge to itself); second: it has the links and the r side has none (the child
    of the root); both have a side without a link deep in the tree as well."""
    a = graph(4, [(0, r, 1, l), (1, r, 2, l), (0, r, 2, l), (2, r, 3, l)])
    b = graph(4, [(0, l, 1, l), (1, r, 2, l), (0, l, 2, l), (2, r, 3, l)])
    return concat([a, b, a])


NO_TIPS = {"sides without a link, no tips declared"}


def tips_of(name, g):
    """The tip array a case is uploaded and handed to the oracle with (None: the tips are the sides without a link)."""
    return np.zeros(g.n_vtx, dtype=np.uint8) if name in NO_TIPS else None


def small_run(n_small=400):
    """A run of two-segment components -- none is decomposed, their sides are in no tree -- long enough (2 * 2 * n_small >=
    BATCH + LANE sides) that all four sides of a batch of EVERY lane of a workgroup are such sides, between decomposed
    components."""
    return concat([tail_fan(40, 3), sized_components([2] * n_small), W.bubble_zoo(3, 3, 5, shuffle_ids=False), sized_components([1, 2, 1]),
                   tail_fan(9, 2, last_side=False)])


def renumbered(self_loops):
    """Components that come in another order than their smallest segments' ids (the re-index renumbers the segments: pos and
    sbase are in use), with and without self loops."""
    parts = [tail_fan(12, 4), ring(6), sized_components([2, 7, 1]), tail_fan(10, 6, last_side=False, parallel=2)]
    if self_loops:
        parts.append(loops_and_parallels())
    g = concat(parts)
    # interleave: segment k of the concatenation becomes segment perm[k], so that components no longer own contiguous ranges
    n = g.n_vtx
    perm = np.argsort(np.random.default_rng(7).permutation(n), kind="stable").astype(np.uint64)
    return W._mk(np.arange(1, n + 1), perm[g.v1.astype(np.int64)], g.s1, perm[g.v2.astype(np.int64)], g.s2)


def identity_order(self_loops):
    parts = [tail_fan(12, 4), ring(6), sized_components([2, 7, 1]), tail_fan(10, 6, last_side=False, parallel=2)]
    if self_loops:
        parts.append(loops_and_parallels())
    return concat(parts)


NIL_TAILS = [(valid, invalid) for valid in (8, 9, 11) for invalid in (4, 5, 7)]


def nil_tail(n_valid, n_invalid):
    """A pass whose sorted order of class entries (one per segment) ends in n_invalid invalid ones: a decomposed component of
    n_valid segments in front of components of two segments and one of one (none is decomposed: their n_invalid segments
    have no class entry and carry NIL).  k_class_finish_black takes four sorted positions a lane, so n_valid % 4 says where in
    a lane's four the tail begins (0: on its edge) and n_invalid = 4n, 4n + 1, 4n + 3 where it ends."""
    small = [2] * (n_invalid // 2) + [1] * (n_invalid % 2)
    return concat([tail_fan(n_valid, 3), sized_components(small)])


def component_labels(g):
    """Component of every segment, numbered by first appearance in segment order (union-find over the links)."""
    par = list(range(g.n_vtx))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    for a, b in zip(g.v1.tolist(), g.v2.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            par[max(ra, rb)] = min(ra, rb)
    roots = [find(v) for v in range(g.n_vtx)]
    ids = {}
    return np.array([ids.setdefault(x, len(ids)) for x in roots])


def segments_without_a_tree(g, tips=None):
    """Segments of the components the oracle does not decompose."""
    sizes, n, c = np.bincount(component_labels(g)), 0, 0
    while True:
        d = dump_component(g, c, tips=tips)
        if d is None:
            return n
        n += 0 if len(d["gid"]) else int(sizes[c])
        c += 1


def cases():
    out = {}
    for valid, invalid in NIL_TAILS:
        out[f"{valid} class entries and {invalid} invalid ones behind them"] = nil_tail(valid, invalid)
    for n in EDGE_SEGMENTS:
        out[f"{n} segments, three back edges out of the last side"] = tail_fan(n, 4)
        out[f"{n} segments, two back edges out of the last side but one"] = tail_fan(n, 3, last_side=False)
    out["2049 segments, five back edges out of the first side of the third workgroup"] = tail_fan(2049, 6, last_side=False)
    for s in SLOTS:
        out[f"{s} slots on the last side"] = tail_fan(s + 6, s)
        if s > 1:  # (a side with one slot has the tree parent's link only: nothing to repeat)
            out[f"{s} slots and a parallel link on the last side but one"] = tail_fan(s + 7, s, last_side=False, parallel=1)
    out["sides without a link"] = linkless()
    out["sides without a link, no tips declared"] = linkless_no_tips()
    out["self loops and parallel links"] = loops_and_parallels()
    out["l-r self loops in front of other links"] = star(2, 3, 2)
    out["l-r self loop, nothing is a tip"] = star(1, 2, 3, tipless=True)
    out["70 links on one side"] = fan(70, "last")
    out["254 links on one side"] = fan(254, "last")
    out["small components around"] = small_around()
    out["a run of small components"] = small_run()
    out["one segment"] = sized_components([1])
    out["two segments, one link"] = graph(2, [(0, r, 1, l)])
    out["five segments, no link"] = graph(5, [])
    for loops in (False, True):
        out[f"components interleaved{', self loops' if loops else ''}"] = renumbered(loops)
        out[f"components in order{', self loops' if loops else ''}"] = identity_order(loops)
    return out
