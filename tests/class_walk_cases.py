"""Directed inputs for the two class walks of the tree stage: small deterministic graphs, each built for named conditions
of tests/class_walk_model.py's telemetry (budget, LDS stack depth, scan batches, list lengths, stack ring and chunks, window
distances).  test_class_walk_inputs.py proves on the CPU that every case reaches what it names; test_gpu_class_walks.py runs
the kernels on them.  Every component starts and ends in a tip, so every tree has a dummy root.

A condition is a TAG, a short string worked out from the telemetry alone by reached(); THRESHOLDS lists, for every row of the
kernels' table of hand-made constants, the tags on either side of it."""
import functools

import numpy as np

from povu_amd import workloads as W

L, R = W.L, W.R


class Builder:
    """Segments by index in creation order, links in the order given (the scan order of a side is the link order)."""

    def __init__(self):
        self.n = 0
        self.links = []

    def seg(self):
        self.n += 1
        return self.n - 1

    def segs(self, k):
        return [self.seg() for _ in range(k)]

    def link(self, a, b, sa=R, sb=L):
        self.links.append((a, sa, b, sb))

    def build(self, perm=None):
        """perm[v]: the vertex index segment v gets (a permutation that keeps every component a contiguous block)."""
        p = list(range(self.n)) if perm is None else list(perm)
        assert sorted(p) == list(range(self.n))
        a = np.array(self.links, dtype=np.int64).reshape(-1, 4)
        pv = np.array(p, dtype=np.int64)
        return W._mk(np.arange(1, self.n + 1), pv[a[:, 0]], a[:, 1], pv[a[:, 2]], a[:, 3])


def component(b, make, tips_first=False):
    """one component: a tip, what make(b, tip) appends (it returns the segment to go on from), a tip.  tips_first: both tips
    are numbered in front, so the component's last segment, and the array's last adjacency list, belong to what make built."""
    t0 = b.seg()
    t1 = b.seg() if tips_first else None
    last = make(b, t0)
    if t1 is None:
        t1 = b.seg()
    b.link(last, t1)


# ---- pieces.  Each takes the builder and the segment it hangs on (linked from that segment's right side) and returns the
# segment the chain goes on from.
def star(b, prev, m, doubled=False, open_at=0):
    """a source, m one-segment arms and a sink: one class of 2 m + 2 sides, two lists of m candidates (source's right side,
    sink's left side).  The walk takes arm 0 to the sink and comes back to the sink's list for every other arm.
    doubled: every third link is there twice (parallel links: list lengths grow, a candidate stands twice).
    open_at = k > 1: the arms 1 .. k - 1 are wired to one another on alternating sides, so the first return to the sink's list
    (remembered at index 2) finds its first unvisited candidate at index k."""
    src = b.seg()
    b.link(prev, src)
    arms = b.segs(m)
    snk = b.seg()
    n = 0
    for x in arms:
        for _ in range(2 if doubled and n % 3 == 2 else 1):
            b.link(src, x)
        n += 1
    for x in arms:
        for _ in range(2 if doubled and n % 3 == 2 else 1):
            b.link(x, snk)
        n += 1
    for i in range(1, open_at - 1):  # (arm i is left by the side it was not entered through)
        side = L if i % 2 == 1 else R
        b.link(arms[i], arms[i + 1], side, side)
    return snk


def closed_arc(b, prev, sides, loops=0, flipped=False):
    """a chain whose first segment links on to its last: one class of `sides` sides (even: the link arrives at the last
    segment's entered side; odd: at its far side, and the black edge of the last segment closes the cycle).  loops: that many
    of the chain's segments, every eighth, carry a one-segment loop on their far side that is scanned first, so the walk
    branches and returns long before it ends; the loops' sides count in `sides`.  flipped: the inner segments are entered
    through their right sides.  Returns (last segment, the chain)."""
    sides -= 2 * loops
    k = (sides + 2) // 2 if sides % 2 == 0 else (sides + 1) // 2
    vs = b.segs(k)
    ent = lambda i: R if flipped and 0 < i < k - 1 else L  # noqa: E731
    ext = lambda i: L if flipped and 0 < i < k - 1 else R  # noqa: E731
    b.link(prev, vs[0])
    b.link(vs[0], vs[1], R, ent(1))
    b.link(vs[0], vs[-1], R, L if sides % 2 == 0 else R)
    for i in range(1, k - 1):
        if loops and i % 8 == 4:
            y = b.seg()
            b.link(vs[i], y, ext(i), L)
            b.link(y, vs[i], R, ext(i))
            loops -= 1
        b.link(vs[i], vs[i + 1], ext(i), ent(i + 1))
    assert loops == 0
    return vs[-1], vs


def tower(b, prev, d, hangers=(), stubs=(), mid=1, wrap=False):
    """workloads.nested_towers' tower (a_0 .. a_{d-1}, c, b_{d-1} .. b_0; same link order), which remembers about three
    sides a level, plus
      hangers (r, n): a chain of n segments a_r > x .. > a_{r+1}, reached only on the way back, from a_{r+1}'s left side;
      stubs r:        two segments that hang on a_r's right side by doubled links: the walk returns from the first straight
                      to the entry it has just pushed;
      mid:            c is a chain of that many segments;
      wrap:           b_0 links back to a_0, so a_0's black edge is inside the class and every level lies one deeper.
    Returns (b_0, a, b)."""
    a = b.segs(d)
    c = b.segs(mid)
    bb = b.segs(d)[::-1]
    b.link(prev, a[0])
    for i in range(d - 1):
        b.link(a[i], a[i + 1])
        b.link(bb[i + 1], bb[i])
    b.link(a[d - 1], c[0])
    for x, y in zip(c, c[1:]):
        b.link(x, y)
    b.link(c[-1], bb[d - 1])
    for j in range(d):
        b.link(a[j], bb[j])
    for r, n in hangers:
        xs = b.segs(n)
        b.link(a[r], xs[0])
        for x, y in zip(xs, xs[1:]):
            b.link(x, y)
        b.link(xs[-1], a[r + 1])
    for r in stubs:
        for z in b.segs(2):
            b.link(a[r], z)
            b.link(a[r], z)  # (the stub's far side is one more tip of the component)
    if wrap:
        b.link(bb[0], a[0])
    return bb[0], a, bb


def place(b, perm, vs, pos):
    """number the segments vs (a contiguous block of the builder) in the order pos (a permutation of range(len(vs)))"""
    base = min(vs)
    assert sorted(vs) == list(range(base, base + len(vs))) and sorted(pos) == list(range(len(vs)))
    for v, p in zip(vs, pos):
        perm[v] = base + p


def stride_order(n, k):
    """0, k, 2 k, .. mod n: every step is k or k - n places"""
    assert np.gcd(n, k) == 1
    return [(i * k) % n for i in range(n)]


# ---- the cases
def case_budget():
    """Closed arcs with 255 .. 258 and 15 .. 18 steps (the count k_class_dfs_small tests against its budget) among bubbles of
    4 to 10 sides, and one arc just over either budget whose walk has branched and returned before the lane gives up."""
    b = Builder()

    def make(b, x):
        for i, s in enumerate((256, 257, 258, 259, 16, 17, 18, 19)):
            for j in range(3):
                x = star(b, x, 1 + (i + j) % 4) if (i + j) % 4 else closed_arc(b, x, 4)[0]
            x = closed_arc(b, x, s)[0]
        x = closed_arc(b, x, 263, loops=3)[0]
        x = star(b, x, 3)
        return closed_arc(b, x, 21, loops=1)[0]
    component(b, make)
    return b.build()


def case_small_depth():
    """Classes of at most 200 sides for the one-lane walk: returns that go on at path depths 5, 7, 9 (tower) and 6, 8, 10
    (wrapped tower: one of them behind a follow-through pair pushed at depths 7 and 8), lists of 1 to 9 links for the
    batches of four; the last component ends in a class, so its last list ends the adjacency array."""
    b = Builder()
    hang = [(2, 1), (3, 1), (4, 2)]
    component(b, lambda b, x: tower(b, x, 6, hangers=hang, stubs=[1])[0])
    component(b, lambda b, x: tower(b, x, 6, hangers=hang, stubs=[1], wrap=True)[0])

    def stars(b, x):
        for m in range(2, 10):
            x = star(b, x, m, doubled=m % 2 == 1)
            x = star(b, x, m, open_at=max(0, m - 2))
        return star(b, x, 5, open_at=4)  # (a batch of the last three slots whose third is the first open one)
    component(b, stars)
    component(b, lambda b, x: star(b, tower(b, x, 5, hangers=[(3, 1)], wrap=True)[0], 6), tips_first=True)
    return b.build()


LIST_M = (5, 6, 7, 8, 63, 64, 65, 66, 127, 128, 129, 130)


def case_lists():
    """A source, m arms and a sink for every m around W_INLINE 6 and around 64 and 128 candidates: two lists of m."""
    b = Builder()

    def make(b, x):
        for m in LIST_M:
            x = star(b, x, m)
        return x
    component(b, make)
    return b.build()


def case_lists_doubled():
    """The same with every third link doubled: list lengths 7, 8, 9 (past the record), 86 and 170 (past one and two looks)."""
    b = Builder()

    def make(b, x):
        for m in (5, 6, 7, 64, 128):
            x = star(b, x, m, doubled=True)
        return x
    component(b, make)
    return b.build()


WIRED_OPEN = (5, 6, 63, 64, 65, 127, 128)


def case_lists_wired():
    """Long lists whose first return finds the first unvisited candidate at index 5, 6, 63, 64, 65, 127, 128 (130 arms: wave
    walk by default) and at 5, 64, 126 in classes the one-lane walk keeps (127 arms); one list of 140 whose scan moves on twice."""
    b = Builder()

    def make(b, x):
        for k in WIRED_OPEN:
            x = star(b, x, 130, open_at=k)
        for k in (5, 64, 126):
            x = star(b, x, 127, open_at=k)
        return star(b, x, 140, open_at=135)  # (two looks of 64 without an unvisited candidate, the third has it)
    component(b, make)
    return b.build()


STACK_MAX = (63, 64, 65, 96, 97, 128, 129, 192, 193)


def case_stack():
    """Towers whose walks remember 63 .. 193 and 323 sides (3 d - 1 + (mid - 1) for a tower of depth d), with hangers that
    make the walk resume at stack indices 31 .. 33, 63 .. 65, 95 .. 97 and 127 .. 129, dropping 1, 32, 63, 64 and more than
    64 entries, out of the ring, out of chunk 0 and chunk 1, and a long hanger whose pushes evict ring slots a second time."""
    b = Builder()
    odd = [(15, 1), (16, 1), (31, 2), (32, 1), (47, 2), (48, 1), (63, 2), (64, 1), (95, 1)]
    component(b, lambda b, x: tower(b, x, 108, hangers=odd, stubs=[20])[0])
    even = [(15, 1), (31, 1), (47, 1), (63, 1)]
    component(b, lambda b, x: tower(b, x, 70, hangers=even, wrap=True)[0])
    component(b, lambda b, x: tower(b, x, 60, hangers=[(9, 1), (40, 2)])[0])
    component(b, lambda b, x: tower(b, x, 80, hangers=[(40, 90)])[0])

    def plain(b, x):
        for d, mid in ((21, 2), (21, 3), (22, 1), (32, 2), (32, 3), (43, 1), (43, 2), (64, 2), (64, 3)):
            x = tower(b, x, d, mid=mid)[0]
        return x
    component(b, plain)
    return b.build()


def case_hot_ladder():
    """A tower of depth 30 numbered along its rails (a_i next to b_i): every step is near, the probe chooses the hot loop,
    and the stack passes the 62 entries at which the hot loop hands over to the general step; four rings in index order
    stop at 61, 62, 63 and 64 entries."""
    b = Builder()
    got = {}

    def make(b, x):
        last, a, bb = tower(b, x, 30)
        got["a"], got["b"] = a, bb
        return last
    component(b, make)

    def arcs(b, x):  # rings in index order whose walks remember 61 .. 64 sides
        for sides in (122, 124, 126, 128):
            x = closed_arc(b, x, sides)[0]
        return x
    component(b, arcs)
    perm = list(range(b.n))
    vs = list(range(min(got["a"]), max(got["b"]) + 1))  # a_0 .. a_29, c, b_29 .. b_0
    d = 30
    pos = [2 * i for i in range(d)] + [2 * d] + [2 * j + 1 for j in range(d - 1, -1, -1)]
    place(b, perm, vs, pos)
    return b.build(perm)


WIN_OFFSETS = (-18, -16, -14, 110, 112, 126, 128, 130)  # sides from the side a far jump lands on


def _window_positions():
    """order (in segments) in which a ring visits its block: after every far jump (200 segments) five near steps, then a
    jump by the wanted offset from the landing place, three near steps; one region moves forward by less than a window,
    back inside the old window, then in front of it.  The slots left over are visited last, ascending."""
    pos = list(range(6))
    region = 1
    for off in WIN_OFFSETS:
        c = 200 * region + 20
        region += 1
        pos += [c + i for i in range(6)]
        t = c + off // 2
        pos += [t + i for i in range(4) if not c <= t + i < c + 6]
    c = 200 * region + 20
    pos += [c + i for i in range(6)] + [c + 60 + i for i in range(6)] + [c + 55, c + 56, c + 57] + [c + 45, c + 46, c + 47, c + 48]
    n = c + 130
    assert len(set(pos)) == len(pos)
    used = set(pos)
    return pos + [p for p in range(n) if p not in used]


def case_window(flipped=False):
    """A ring whose numbering makes the walk land, after a jump that moves the window, 18, 16, 14 sides behind the landing
    side and 110, 112, 126, 128, 130 in front of it (the window keeps 16 sides behind and holds 128); flipped: the ring's
    segments are entered through their right sides, so the landing sides are odd."""
    b = Builder()
    pos = _window_positions()
    got = {}

    def make(b, x):
        last, got["vs"] = closed_arc(b, x, 2 * len(pos) - 2, flipped=flipped)
        return last
    component(b, make)
    perm = list(range(b.n))
    place(b, perm, got["vs"], pos)
    return b.build(perm)


def case_window_edges():
    """One class inside the first 16 sides of the array (the window's low end is clamped to 0) and one on its last sides
    (the window reaches past the array)."""
    b = Builder()
    component(b, lambda b, x: closed_arc(b, x, 12)[0])
    component(b, lambda b, x: star(b, x, 3))
    component(b, lambda b, x: closed_arc(b, x, 40)[0], tips_first=True)
    return b.build()


def _probe_case(near, n_far, stride, far_first):
    b = Builder()
    got = {}

    def make(b, x):
        last, got["vs"] = closed_arc(b, x, 2 * (near + n_far) - 2)
        return last
    component(b, make)
    far = stride_order(n_far, stride)
    pos = far + [n_far + i for i in range(near)] if far_first else list(range(near)) + [near + p for p in far]
    perm = list(range(b.n))
    place(b, perm, got["vs"], pos)
    return b.build(perm)


def case_near_then_scattered():
    """757 steps: 50 segments in index order (the probe's 48 hops are near: the form with the hot loop), then 330 segments
    in steps of 127 and -203 places: the hot form's trial of 512 general steps gives up."""
    return _probe_case(50, 330, 127, False)


def case_scattered_then_near():
    """797 steps, scattered first (the probe says plain), the last 200 segments in index order."""
    return _probe_case(200, 200, 77, True)


def case_scattered_long():
    """2 597 scattered steps: the window's refill back-off doubles up to its cap of 1024 steps."""
    return _probe_case(0, 1300, 487, True)


CASES = {
    "budget": case_budget,
    "small_depth": case_small_depth,
    "lists": case_lists,
    "lists_doubled": case_lists_doubled,
    "lists_wired": case_lists_wired,
    "stack": case_stack,
    "hot_ladder": case_hot_ladder,
    "window": case_window,
    "window_flipped": lambda: case_window(True),
    "window_edges": case_window_edges,
    "near_then_scattered": case_near_then_scattered,
    "scattered_then_near": case_scattered_then_near,
    "scattered_long": case_scattered_long,
}


# ---- tags: what a graph reaches, from the model's telemetry alone
def reached(classes, n_sides):
    """the set of tags the classes (class_walk_model.model_graph) reach; n_sides: sides of the whole graph"""
    tags = set()
    last_comp = max((c["comp"] for c in classes), default=0)
    for c in classes:
        sm, wv = c["small"], c["wave"]
        # budget
        if c["steps"] in (15, 16, 17, 18, 255, 256, 257, 258):
            tags.add(f"steps={c['steps']}:{'go' if c['over'][256] else 'stay'}@256")
            tags.add(f"steps={c['steps']}:{'go' if c['over'][16] else 'stay'}@16")
        for bud, (_, n_ret) in c["abandoned_at"].items():
            if n_ret:
                tags.add(f"abandoned-after-returns@{bud}")
        # the one-lane walk's stack and batches
        if c["sides"] <= 200:
            for r in sm["returns"]:
                if r["scans"] and r["advances"]:
                    tags.add(f"ret-depth={r['depth']}:{'lds' if r['lds'] else 'dps'}")
                    if r["depth"] == 8 and r["pair_first"] == 7:
                        tags.add("ret-behind-pair-7-8")
            for p in sm["pairs"]:
                if p == 7:
                    tags.add("pair-pushed-at-7-8")
            for rem, j in sm["batches"]:
                tags.add(f"batch=rem{rem},open{j if j < 4 else '-'}")
            if sm["adj_end"] and c["comp"] == last_comp:
                tags.add("batch-reads-past-last-list")
        # list lengths
        for n in set(c["lists"].values()):
            tags.add(f"list={n}")
            if not c["over"][256]:
                tags.add(f"list={n}:small-walk")
        for k in wv["look_moves"]:
            tags.add(f"look-moved-on={k}")
        if wv["beyond_only_pushes"]:
            tags.add("pushed-for-next-look-only")
        # the wave walk's stack
        if wv["max_entries"] >= 60:
            tags.add(f"max-entries={wv['max_entries']}")
        if wv["max_entries"] > 256:
            tags.add(f"max-entries>256:pool={wv['pool']}")
        tags.add(f"pool={wv['pool']}")
        if wv["re_evictions"]:
            tags.add("ring-slots-evicted-again")
        for r in wv["resumes"]:
            if r["first_open"] is None:
                tags.add("long-list-entry-nothing-open")
                continue
            tags.add(f"resume-index={r['index']}")
            tags.add(f"drop={r['dropped']}" if r["dropped"] <= 64 else f"drop>64:fetches={r['fetches']}")
            tags.add(f"resumed-from={'chunk%d' % r['chunk'] if r['from_hbm'] else 'ring'}")
            if r["span"]:
                tags.add("fetch-spans-chunks")
            tags.add("resume-list<=6" if r["list_len"] <= 6 else "resume-list>6")
            if r["first_open"] > r["j"] and r["first_open"] in WIRED_OPEN:
                tags.add(f"first-open={r['first_open']}:behind-visited")
        # numbering: the hot loop, the window, the form choice
        dist = c["dist"]
        near_all = all(abs(d) <= 64 for d in dist)
        if c["probe_hot"] and near_all and wv["max_entries"] >= 60:
            tags.add(f"hot:near-steps:max-entries={wv['max_entries']}")
        if c["hi"] < 16:
            tags.add("class-inside-first-16-sides")
        if c["hi"] >= n_sides - 2 and c["sides"] > 16:
            tags.add("class-on-last-sides")
        land, seq = None, []
        for p, ch in c["tree_steps"]:
            if abs(ch - p) > 128:
                land, seq = ch, []
                continue
            if land is not None:
                off = ch - land
                if off in WIN_OFFSETS:
                    tags.add(f"win-offset={off}:{'odd' if land & 1 else 'even'}-landing")
                if abs(ch - p) > 1:
                    seq.append(off)
                    if [o for o in seq if o in (120, 110, 90)] == [120, 110, 90]:
                        tags.add("win-forward-back-inside-back-before")
        link_steps = [d for d in dist if abs(d) != 1]
        far = lambda ds: sum(1 for d in ds if abs(d) > 128)  # noqa: E731
        if c["steps"] > 600 and c["probe_hot"] and all(abs(d) <= 64 for d in dist[:96]) and far(dist[96:]) * 5 >= 2 * len(dist[96:]):
            tags.add("probe-near-body-scattered>600")
        if c["steps"] > 600 and not c["probe_hot"] and c["probe"][1] == 48 and all(abs(d) <= 64 for d in dist[-300:]) and far(dist[:300]) >= 120:
            tags.add("probe-scattered-tail-near>600")
        if c["steps"] > 2500 and far(link_steps) * 10 >= 9 * len(link_steps):
            tags.add("scattered>2500")
    return tags


# ---- the kernels' hand-made constants: for every row, the tags on either side of the threshold.  Every tag is named by a case
# (CASE_TAGS) and shown there by the model; nothing is left to a graph whose telemetry does not show it.
_BATCHES = tuple(f"batch=rem{r},open{j}" for r in (1, 2, 3, 4) for j in list(range(r)) + ["-"])
THRESHOLDS = {
    "CLASS_BUDGET 256": ("steps=255:stay@256", "steps=256:stay@256", "steps=257:go@256", "steps=258:go@256", "abandoned-after-returns@256"),
    "POVU_HIP_CLASS_BUDGET=16": ("steps=15:stay@16", "steps=16:stay@16", "steps=17:go@16", "steps=18:go@16", "abandoned-after-returns@16"),
    "DFS_STK 8": ("ret-depth=6:lds", "ret-depth=7:lds", "ret-depth=8:dps", "ret-depth=9:dps", "ret-depth=10:dps", "pair-pushed-at-7-8",
                  "ret-behind-pair-7-8"),
    "batches of 4": _BATCHES + ("batch-reads-past-last-list",),
    "W_INLINE 6": ("list=5", "list=6", "list=7", "list=8", "resume-list<=6", "resume-list>6", "long-list-entry-nothing-open"),
    "64 lanes a look": tuple(f"list={m}" for m in LIST_M[4:]) + tuple(f"list={m}:small-walk" for m in (63, 64, 65, 66, 127))
    + tuple(f"first-open={k}:behind-visited" for k in WIRED_OPEN) + ("look-moved-on=1", "look-moved-on=2", "pushed-for-next-look-only"),
    "ring 64, eviction 32, chunks": tuple(f"max-entries={n}" for n in STACK_MAX) + ("max-entries>256:pool=512", "pool=0", "pool=64", "pool=128", "pool=256")
    + tuple(f"resume-index={i}" for i in (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129))
    + ("drop=1", "drop=32", "drop=63", "drop=64", "drop>64:fetches=2", "resumed-from=ring", "resumed-from=chunk0", "resumed-from=chunk1",
       "fetch-spans-chunks", "ring-slots-evicted-again"),
    "hot loop leaves at 62 entries": tuple(f"hot:near-steps:max-entries={n}" for n in (61, 62, 63, 64, 89)),
    "W_WIN 128, W_WIN_BACK 16": tuple(f"win-offset={o}:{p}-landing" for o in WIN_OFFSETS for p in ("even", "odd"))
    + ("class-inside-first-16-sides", "class-on-last-sides", "win-forward-back-inside-back-before"),
    "W_PROBE 48, W_TRIAL 512, penalty 1024": ("probe-near-body-scattered>600", "probe-scattered-tail-near>600", "scattered>2500"),
}
_WIN = THRESHOLDS["W_WIN 128, W_WIN_BACK 16"]
CASE_TAGS = {
    "budget": THRESHOLDS["CLASS_BUDGET 256"] + THRESHOLDS["POVU_HIP_CLASS_BUDGET=16"],
    "small_depth": THRESHOLDS["DFS_STK 8"] + THRESHOLDS["batches of 4"],
    "lists": tuple(f"list={m}" for m in LIST_M) + tuple(f"list={m}:small-walk" for m in (63, 64, 65, 66, 127))
    + ("resume-list<=6", "resume-list>6", "long-list-entry-nothing-open"),
    "lists_doubled": ("list=7", "list=8", "list=9", "list=85", "list=170", "look-moved-on=1"),
    "lists_wired": tuple(f"first-open={k}:behind-visited" for k in WIRED_OPEN) + ("look-moved-on=1", "look-moved-on=2", "pushed-for-next-look-only"),
    "stack": THRESHOLDS["ring 64, eviction 32, chunks"],
    "hot_ladder": THRESHOLDS["hot loop leaves at 62 entries"],
    "window": tuple(t for t in _WIN if "even" in t) + ("win-forward-back-inside-back-before",),
    "window_flipped": tuple(t for t in _WIN if "odd" in t) + ("win-forward-back-inside-back-before",),
    "window_edges": ("class-inside-first-16-sides", "class-on-last-sides"),
    "near_then_scattered": ("probe-near-body-scattered>600",),
    "scattered_then_near": ("probe-scattered-tail-near>600",),
    "scattered_long": ("scattered>2500",),
}


@functools.lru_cache(maxsize=None)
def modelled(name):
    """(graph, [(component rank, oracle dump, model tree or None)], classes) of a case: built and modelled once a process"""
    import class_walk_model as M
    g = CASES[name]()
    comps, classes = M.model_graph(g)
    return g, comps, classes
