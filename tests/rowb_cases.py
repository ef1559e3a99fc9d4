"""Inputs of the direct tests of rows A and B (tests/test_gpu_rowb.py): graphs at the thresholds and alternative forms of
povu_amd/csrc/hip/graph_kernels.hip.  Every case exists for a property -- a path the upload, the labelling or the re-index
takes --, states it (Case.path, .builder, .cross, ...), and tests/test_rowb_inputs.py asserts those properties on the plain
restatement (tests/rowb_ref.py) alone, without a GPU: a case that no longer reaches its edge fails there.

No case exceeds three tiles plus one segment or about 7 * 10^4 links."""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional

import numpy as np

from povu_amd import workloads as W
from primitives_cases import rng_of

# ---- these MIRROR constants of povu_amd/csrc/hip/graph_kernels.hip (tests/test_rowb_inputs.py compares them with the
# source): when one changes there, change it here, and the sizes below move with it
UF_TILE = 8192  # segments a workgroup of k_uf_tiles unites in LDS; a link that leaves its tile goes onto the cross list
UF_TPB = 1024  # lanes of that workgroup
UF_GROUPS = 2  # groups of four sides a lane takes a round
UF_HEAVY = 128  # a side with MORE links than this is left to the whole workgroup ...
UF_HEAVY_CAP = 256  # ... unless the tile already has this many such sides
FILL_MAX_SIDE_DEGREE = 64  # no side has more links: slot fill + insertion sort; else the radix sort of (side, link) pairs
SORT_FREE_MAX_VDEG = 48  # no segment has more links: k_local_adj; else the builder that numbers the local links densely
LOCAL_ADJ_REGS = 4  # entries of a side k_local_adj keeps in registers; the next one flushes them

L, R = W.L, W.R
TIP_NONE, TIP_L, TIP_R = 0, 1, 2
# the path bits of povu_hip_debug_row_b (include/povu_hip.h), as a pass without flags takes them
IDENTITY, SORT_FREE, LEAN, LOOPS, DENSE, SPEC_KEPT = 1, 2, 4, 8, 16, 32


@dataclass
class Case:
    name: str
    links: W.Links
    path: int  # IDENTITY | SORT_FREE | LEAN | LOOPS | DENSE of a pass without flags
    slot_fill: bool = True  # the builder of the upload (False: radix sort)
    tips: Optional[np.ndarray] = None
    C: Optional[int] = None  # component count, where the case states one
    cross: Optional[int] = None  # links whose ends lie in different tiles, where stated
    info: dict = field(default_factory=dict)  # what else the case is there for (tests/test_rowb_inputs.py)


def path_under(path, sorted_adj):
    """The path bits of the same graph under POVU_HIP_F_SORTED_ADJ."""
    return (path & (IDENTITY | LOOPS)) | DENSE if sorted_adj else path


class _Builder:
    """Collects links (segment, side, segment, side); the graph comes out with its links shuffled and about half of them
    naming their larger end first, unless the case keeps its order."""

    def __init__(self, name, V):
        self.name, self.V, self.rows = name, V, []

    def add(self, a, sa, b, sb):
        a, sa, b, sb = np.broadcast_arrays(np.asarray(a, np.int64), sa, b, sb)
        self.rows.append(np.stack([a.ravel(), sa.ravel(), b.ravel(), sb.ravel()], axis=1).astype(np.int64))

    def chain(self, segs):
        """r side of each to the l side of the next."""
        segs = np.asarray(segs, np.int64)
        if segs.size > 1:
            self.add(segs[:-1], R, segs[1:], L)

    def links(self, shuffle_ids, keep_order=False):
        rng = rng_of("rowb_" + self.name, self.V)
        t = np.concatenate(self.rows) if self.rows else np.zeros((0, 4), np.int64)
        if not keep_order:
            t = t[rng.permutation(t.shape[0])]
            larger_first = (rng.random(t.shape[0]) < 0.5) == (t[:, 0] < t[:, 2])
            t[larger_first] = t[larger_first][:, [2, 3, 0, 1]]
        vid = np.arange(1, self.V + 1)
        if shuffle_ids:  # the start key then does not follow the index
            vid = rng.permutation(3 * self.V)[:self.V] + 1
        return W._mk(vid, t[:, 0], t[:, 1], t[:, 2], t[:, 3])


# ================================================================================================ row A
def _side_n(n):
    """Segment 0's r side holds exactly n links: a same-side self loop, a pair of parallel links and n - 3 more, given in
    descending order of the far end; the far ends form a chain."""
    V = n + 2
    b = _Builder(f"side_{n}", V)
    far = np.arange(n - 2, 0, -1)  # n - 2 far ends, descending; the first of them twice
    b.add(0, R, np.concatenate([[far[0]], far]), L)
    b.add(0, R, 0, R)
    b.chain(np.arange(V - 1, 0, -1))
    return Case(f"side_{n}", b.links(n % 2 == 1, keep_order=True), IDENTITY | LOOPS | DENSE, slot_fill=n <= FILL_MAX_SIDE_DEGREE,
                C=1, info=dict(max_side=n))


def _sides_of_2_and_3():
    """A thousand r sides of two links (even segments) and three (odd), far ends spread over a chain of a thousand more:
    the two-entry swap of k_side_sort and its general loop, on lists whose links arrive from several workgroups."""
    n = 1000
    b = _Builder("sides_of_2_and_3", 2 * n)
    for j in range(3):
        i = np.arange(n) if j < 2 else np.arange(1, n, 2)
        b.add(i, R, n + (3 * i + 7 * j) % n, L)
    b.chain(np.arange(n, 2 * n))
    return Case("sides_of_2_and_3", b.links(True), IDENTITY | SORT_FREE | LEAN, C=1)


def _no_links(V, name):
    return Case(name, _Builder(name, V).links(V > 1), IDENTITY | SORT_FREE | LEAN, C=V, cross=0)


def _tips_given():
    """A chain of six and a chain of three; the tips given are not the ones the upload would infer: none where the first
    chain begins, an l tip where it ends (inferred: r), an r tip on a segment with links on both sides, none at all in the
    second chain."""
    b = _Builder("tips_given", 9)
    b.chain(np.arange(6))
    b.chain(np.arange(6, 9))
    tips = np.array([TIP_NONE, TIP_NONE, TIP_R, TIP_NONE, TIP_NONE, TIP_L, TIP_NONE, TIP_NONE, TIP_NONE], dtype=np.uint8)
    return Case("tips_given", b.links(True), IDENTITY | SORT_FREE | LEAN, tips=tips, C=2, cross=0)


# ================================================================================================ labelling
def _chain(name, V, order=None, shuffle_ids=False, keep_order=True):
    b = _Builder(name, V)
    b.chain(np.arange(V) if order is None else order)
    return b.links(shuffle_ids, keep_order=keep_order)


def _one_tile_chain():
    """Links (i, i + 1) in ascending order over one whole tile: neighbouring lanes unite them at the same moment."""
    return Case("one_tile_chain", _chain("one_tile_chain", UF_TILE), IDENTITY | SORT_FREE | LEAN, C=1, cross=0)


def _tile_plus_one():
    return Case("tile_plus_one", _chain("tile_plus_one", UF_TILE + 1, shuffle_ids=True), IDENTITY | SORT_FREE | LEAN, C=1, cross=1)


def _permuted_chain():
    V = 2 * UF_TILE + 3
    order = rng_of("rowb_permuted_chain_order", V).permutation(V)
    return Case("permuted_chain", _chain("permuted_chain", V, order, shuffle_ids=True, keep_order=False), IDENTITY | SORT_FREE | LEAN, C=1,
                info=dict(cross_share=(0.45, 0.55)))


STRIPES_PAIR = (UF_TILE // 2 + 1, 2 * UF_TILE + UF_TILE // 2)  # one in the first tile, one in the third, joined to each other only
STRIPES_ISOLATED = (5, UF_TILE - 1, UF_TILE + 4097, 3 * UF_TILE)  # (the last of a tile and the last of the graph among them)


def _stripes():
    """An odd number of segments over three tiles and one more: every ordinary segment links to the seventh ordinary one
    after it -- seven interleaved components --, a pair joined across two tile borders, and isolated segments."""
    V = 3 * UF_TILE + 1
    b = _Builder("stripes", V)
    ordinary = np.setdiff1d(np.arange(V), STRIPES_PAIR + STRIPES_ISOLATED)
    b.add(ordinary[:-7], R, ordinary[7:], L)
    b.add(STRIPES_PAIR[0], R, STRIPES_PAIR[1], L)
    return Case("stripes", b.links(True), SORT_FREE, C=7 + 1 + len(STRIPES_ISOLATED))


GROUPED_BOUNDS = (0, 1001, UF_TILE, UF_TILE + 2503, UF_TILE + 4005, UF_TILE + 5006)  # only UF_TILE is a multiple of 4


def _grouped(name, loop=False, swap=None):
    """Five components one after the other in segment order: chains in which every third segment also links to the next
    but one (at most three links a side, no self loop)."""
    V = GROUPED_BOUNDS[-1]
    b = _Builder(name, V)
    for lo, hi in zip(GROUPED_BOUNDS[:-1], GROUPED_BOUNDS[1:]):
        b.chain(np.arange(lo, hi))
        i = np.arange(lo, hi - 2, 3)
        b.add(i, R, i + 2, L)
    if loop:
        b.add(V - 1, L, V - 1, R)
    if swap:  # two segments of different components change places
        x, y = swap
        ren = np.arange(V)
        ren[x], ren[y] = y, x
        for t in b.rows:
            t[:, 0], t[:, 2] = ren[t[:, 0]], ren[t[:, 2]]
    path = SORT_FREE if swap else IDENTITY | SORT_FREE | LEAN | (LOOPS if loop else 0)
    return Case(name, b.links(name != "grouped_one_swap"), path, C=5, cross=0 if not swap else None)


GROUPED_SWAP = (500, 1500)
HUB_128, HUB_129 = UF_TILE - 192, UF_TILE - 92  # even segments: their r side is the second side of a group of four sides


def _heavy_128_129():
    """Two hub sides, of UF_HEAVY links (the lane walks it) and of one more (the workgroup does); about half their far ends
    lie in the next tile.  Each is the second side of a group of four whose other sides hold 2, 1 and 5 links."""
    V = 2 * UF_TILE
    b = _Builder("heavy_128_129", V)
    for hub, n, base in ((HUB_128, UF_HEAVY, 0), (HUB_129, UF_HEAVY + 1, 300)):
        here = UF_TILE - 2000 + base + np.arange(n // 2)
        there = UF_TILE + 1000 + base + np.arange(n - n // 2)
        b.add(hub, R, np.concatenate([here, there]), L)
        b.add(hub, L, hub - 10 + np.arange(2), R)
        b.add(hub + 1, L, hub - 20, R)
        b.add(hub + 1, R, hub - 40 + np.arange(5), L)
    return Case("heavy_128_129", b.links(False), DENSE, slot_fill=False, cross=UF_HEAVY // 2 + (UF_HEAVY + 1 - (UF_HEAVY + 1) // 2),
                info=dict(heavy_per_tile=[1, 0], sides_at_least_heavy=2, max_side=UF_HEAVY + 1))


PARALLEL_ENDS = (100, UF_TILE + 3)


def _heavy_parallel():
    """UF_HEAVY + 1 parallel links between the l side of a segment of the first tile and the r side of one of the second:
    a hub side in either tile, every one of the links on the cross list, and exactly one of them may join the forest."""
    u, w = PARALLEL_ENDS
    b = _Builder("heavy_parallel", UF_TILE + 8)
    b.add(np.full(UF_HEAVY + 1, u), L, w, R)
    b.add(u, R, u + 1, L)
    b.add(w, L, w - 1, R)
    return Case("heavy_parallel", b.links(True), DENSE, slot_fill=False, C=UF_TILE + 8 - 3, cross=UF_HEAVY + 1,
                info=dict(heavy_per_tile=[1, 1], max_side=UF_HEAVY + 1))


def _heavy_257():
    """One tile with one hub side more than the workgroup takes: UF_HEAVY_CAP + 1 r sides of UF_HEAVY + 1 links each; the last
    of them to arrive is walked by its lane.  Whichever it is, one of its links is the only link of the segment behind the
    hub (a link is united from its smaller end: nothing else would join that segment); the other far ends are spread over
    both sides of the remaining segments, and neighbouring hubs share one of them: one component."""
    n_hubs, n = UF_HEAVY_CAP + 1, UF_HEAVY + 1
    b = _Builder("heavy_257", UF_TILE)
    hubs = 16 * np.arange(n_hubs)
    b.add(hubs, R, hubs + 1, L)
    rest = np.setdiff1d(np.arange(UF_TILE), np.concatenate([hubs, hubs + 1]))
    t = (np.arange(n_hubs)[:, None] * (n - 2) + np.arange(n - 1)[None, :]).ravel()
    b.add(np.repeat(hubs, n - 1), R, rest[t % rest.size], (t // rest.size) % 2)
    return Case("heavy_257", b.links(True), IDENTITY | DENSE, slot_fill=False, C=1, cross=0,
                info=dict(heavy_per_tile=[UF_HEAVY_CAP + 1], max_side=UF_HEAVY + 1, hubs=hubs))


def _heavy_last_side():
    """The hub side is the r side of the last segment of a graph with an odd number of segments: the second side of the last,
    incomplete group of four."""
    V = 301
    b = _Builder("heavy_last_side", V)
    b.add(V - 1, R, np.arange(UF_HEAVY + 1), L)
    b.chain(np.arange(V))
    return Case("heavy_last_side", b.links(False), IDENTITY | DENSE, slot_fill=False, C=1, cross=0,
                info=dict(heavy_per_tile=[1], max_side=UF_HEAVY + 1, hub_side=2 * V - 1))


# ================================================================================================ re-index
def _vdeg(n):
    """Segment 30 has n links over its two sides, each to a segment of its own."""
    V = n + 31
    b = _Builder(f"vdeg_{n}", V)
    far = np.setdiff1d(np.arange(V), [30])[:n]
    b.add(30, L, far[:n // 2], R)
    b.add(30, R, far[n // 2:], L)
    free = n <= SORT_FREE_MAX_VDEG
    return Case(f"vdeg_{n}", b.links(n % 2 == 0), IDENTITY | (SORT_FREE | LEAN if free else DENSE), C=V - n, info=dict(max_vdeg=n))


LISTS_CENTRES = (40, 41, 42, 43)  # their l sides hold 3, 4, 5 and 6 local entries


def _lists_4_5(loop):
    """One chain of 84 segments; the l sides of four segments in its middle hold 3, 4, 5 and 6 local entries.  `own`: all
    of them the side's own slots (the fifth flushes the registers inside the slot loop).  `loop`: one of them is an r-r self
    loop, which the opposite side contributes (the flush happens behind the slot loop).  The far ends alternate below and
    above the segment, so the ids a side takes from its twins and its own arrive in mixed order."""
    name = "lists_4_5_loop" if loop else "lists_4_5_own"
    V = 84
    b = _Builder(name, V)
    b.chain(np.arange(V))  # (gives every l side in the middle its first entry)
    for k, c in enumerate(LISTS_CENTRES):
        extra = 2 + k - (1 if loop else 0)  # besides the chain's link (and the loop)
        j = np.arange(extra)
        far = np.where(j % 2 == 0, 50 + 8 * k + j, 8 * k + j)  # (the chain's link comes from below)
        b.add(c, L, far, np.where(far < c, R, L))
        if loop:
            b.add(c, R, c, R)
    return Case(name, b.links(loop, keep_order=True), IDENTITY | SORT_FREE | LEAN | (LOOPS if loop else 0), C=1,
                info=dict(list_lengths={3, 4, 5, 6}))


def _loops_renumbered():
    """Two interleaved chains (even and odd segments), so that the sorted position is not the segment index; l-l, r-r and l-r
    self loops, each alone, twice in parallel, and all three on one segment; and one l side of six entries."""
    V = 40
    b = _Builder("loops_renumbered", V)
    b.chain(np.arange(0, V, 2))
    b.chain(np.arange(1, V, 2))
    for v, kinds in ((4, [(L, L)]), (7, [(R, R)]), (10, [(L, R)]), (13, [(L, L), (R, R), (R, L)]), (21, [(L, L)] * 2), (24, [(R, R)] * 2),
                     (27, [(L, R), (R, L)])):
        for sa, sb in kinds:
            b.add(v, sa, v, sb)
    b.add(16, L, [2, 30, 6, 36, 16], [R, L, R, L, R])  # (the last of them an l-r self loop)
    return Case("loops_renumbered", b.links(True), SORT_FREE | LOOPS, C=2, cross=0, info=dict(list_lengths={4, 6}))


@lru_cache(maxsize=None)
def cases():
    cs = [_side_n(FILL_MAX_SIDE_DEGREE), _side_n(FILL_MAX_SIDE_DEGREE + 1), _sides_of_2_and_3(), _no_links(5, "no_links"),
          _no_links(1, "one_segment"), _tips_given(),
          _one_tile_chain(), _tile_plus_one(), _permuted_chain(), _stripes(), _grouped("grouped"), _grouped("grouped_one_loop", loop=True),
          _grouped("grouped_one_swap", swap=GROUPED_SWAP), _heavy_128_129(), _heavy_parallel(), _heavy_257(), _heavy_last_side(),
          _vdeg(SORT_FREE_MAX_VDEG), _vdeg(SORT_FREE_MAX_VDEG + 1), _lists_4_5(False), _lists_4_5(True), _loops_renumbered()]
    return {c.name: c for c in cs}


NAMES = ["side_64", "side_65", "sides_of_2_and_3", "no_links", "one_segment", "tips_given", "one_tile_chain", "tile_plus_one",
         "permuted_chain", "stripes", "grouped", "grouped_one_loop", "grouped_one_swap", "heavy_128_129", "heavy_parallel", "heavy_257",
         "heavy_last_side", "vdeg_48", "vdeg_49", "lists_4_5_own", "lists_4_5_loop", "loops_renumbered"]
SHUFFLED_IDS = 14  # cases whose segment ids are shuffled (at least half)


@lru_cache(maxsize=None)
def reference(name):
    """The restatement of a case, computed once and shared (read-only)."""
    import rowb_ref
    c = cases()[name]
    return rowb_ref.build(c.links, c.tips)
