"""Rows A and B restated in numpy and plain Python: what oracle/povu_oracle.c does in orc_graph_build_csr,
orc_graph_infer_tips, orc_comp_map_of and orc_componetize, for a workloads.Links and optional tips.

Everything is in one of two index spaces.  GLOBAL: segment idx v, side 2 v + end (0 = l, 1 = r), link idx e, adjacency slot k.
SORTED: the segments ordered by (component, idx); position i, sorted side 2 i + end.  Components are ranked by their smallest
segment idx, component c owns positions [voff[c], voff[c + 1]) and local idx = i - voff[c]."""
from types import SimpleNamespace

import numpy as np

TIP_NONE, TIP_L, TIP_R = 0, 1, 2
NO_KEY = (1 << 64) - 1


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def build(links, tips=None):
    V, E = links.n_vtx, links.n_links
    v1, v2 = links.v1.astype(np.int64), links.v2.astype(np.int64)
    a, b = 2 * v1 + links.s1, 2 * v2 + links.s2
    r = SimpleNamespace(V=V, E=E)

    # ---- row A.  Per-side lists of link ids, ascending; a same-side self loop sits once in its side's list
    two = np.flatnonzero(b != a)
    side = np.concatenate([a, b[two]])
    link = np.concatenate([np.arange(E, dtype=np.int64), two])
    order = np.lexsort((link, side))
    side, r.adj = side[order], link[order]
    r.deg = np.bincount(side, minlength=2 * V)[:2 * V] if E else np.zeros(2 * V, np.int64)
    r.off = np.concatenate([[0], np.cumsum(r.deg)])
    r.slot_side = side
    # other side of every slot (a same-side self loop: its own side) and the slot of the same link in that side's list
    r.aoth = np.where(a[r.adj] == side, b[r.adj], a[r.adj])
    key = side * max(E, 1) + r.adj  # (ascending: the slots are in (side, link) order)
    r.atwin = np.searchsorted(key, r.aoth * max(E, 1) + r.adj)
    if tips is None:
        le, re = r.deg[0::2] == 0, r.deg[1::2] == 0
        r.tip = np.where(le, TIP_L, np.where(re, TIP_R, TIP_NONE)).astype(np.uint8)
    else:
        r.tip = np.asarray(tips, dtype=np.uint8)
    r.max_side = int(r.deg.max()) if V else 0
    r.max_vdeg = int((r.deg[0::2] + r.deg[1::2]).max()) if V else 0
    r.n_empty_sides = int((r.deg == 0).sum())

    # ---- row B.  Components by plain connectivity, ranked by their smallest segment
    parent = list(range(V))
    for x, y in zip(v1.tolist(), v2.tolist()):
        rx, ry = _find(parent, x), _find(parent, y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    root = np.array([_find(parent, v) for v in range(V)], dtype=np.int64)
    roots = np.unique(root)
    r.C = int(roots.size)
    r.comp = np.searchsorted(roots, root)
    r.perm = np.argsort(r.comp, kind="stable")  # sorted position -> segment
    r.pos = np.empty(V, np.int64)
    r.pos[r.perm] = np.arange(V)
    r.voff = np.concatenate([[0], np.cumsum(np.bincount(r.comp, minlength=r.C))])
    r.local_idx = r.pos - r.voff[r.comp]
    r.labels_sorted = bool((np.diff(r.comp) >= 0).all())
    r.has_self_loops = bool((v1 == v2).any())

    # the local links in first-encounter order: segments ascend (inside their component), l side before r side, slots
    # ascend; each link is stored from the side that met it first, a self loop as (side, opposite side)
    vdeg = r.deg[0::2] + r.deg[1::2]
    sbase = np.concatenate([[0], np.cumsum(vdeg[r.perm])])  # slots in front of sorted position i
    sv = side >> 1
    P = sbase[r.pos[sv]] + (np.arange(side.size) - r.off[2 * sv])  # place of every slot in the walk
    first = np.full(E, np.iinfo(np.int64).max)
    np.minimum.at(first, r.adj, P)
    meets = np.flatnonzero(P == first[r.adj])
    meets = meets[np.argsort(P[meets])]  # one slot a link, in walk order
    e = r.adj[meets]
    r.la = 2 * r.pos[sv[meets]] + (side[meets] & 1)
    o = r.aoth[meets]
    r.lb = np.where(v1[e] == v2[e], r.la ^ 1, 2 * r.pos[o >> 1] + (o & 1))
    r.link_of_local = e  # global link of every local link
    link_comp = r.comp[r.perm[r.la >> 1]] if E else np.zeros(0, np.int64)
    r.eoff = np.concatenate([[0], np.cumsum(np.bincount(link_comp, minlength=r.C))])

    # the per-side local lists that follow: a local link sits in the lists of both its sides, ascending by local link index
    le = np.arange(E, dtype=np.int64)
    ls, lo, ll = np.concatenate([r.la, r.lb]), np.concatenate([r.lb, r.la]), np.concatenate([le, le])
    order = np.lexsort((ll, ls))
    r.ldeg = np.bincount(ls, minlength=2 * V)[:2 * V] if E else np.zeros(2 * V, np.int64)
    r.loff = np.concatenate([[0], np.cumsum(r.ldeg)])
    r.ladj, r.lle = lo[order], ll[order]  # other sorted side; local link index + the component's link offset
    r.max_local_side = int(r.ldeg.max()) if V else 0

    # start key of every component: the smallest (segment id, sorted side) among its tips
    r.start_key = np.full(r.C, NO_KEY, dtype=np.uint64)
    vid = links.vid.astype(np.uint64)
    for v in np.flatnonzero(r.tip).tolist():
        k = (int(vid[v]) << 32) | (2 * int(r.pos[v]) + (0 if r.tip[v] == TIP_L else 1))
        c = r.comp[v]
        if k < int(r.start_key[c]):
            r.start_key[c] = k
    return r


def component(r, c):
    """Component c the way orc_dump_component shows it: gidx, and the local links with local segment indices."""
    lo, hi = int(r.eoff[c]), int(r.eoff[c + 1])
    vo = int(r.voff[c])
    return dict(gidx=r.perm[vo:int(r.voff[c + 1])], ev1=(r.la[lo:hi] >> 1) - vo, es1=r.la[lo:hi] & 1,
                ev2=(r.lb[lo:hi] >> 1) - vo, es2=r.lb[lo:hi] & 1)


def componetized(r, links):
    """The arrays of povu_hip_components."""
    c = np.searchsorted(r.eoff, np.arange(r.E), side="right") - 1  # component of every local link
    vo = r.voff[c] if r.E else np.zeros(0, np.int64)
    return dict(n_components=r.C, vtx_off=r.voff, link_off=r.eoff, vtx_id=links.vid[r.perm], vtx_tip=r.tip[r.perm],
                v1=(r.la >> 1) - vo, s1=r.la & 1, v2=(r.lb >> 1) - vo, s2=r.lb & 1)


def cross_links(links, tile):
    """Links whose two ends lie in different tiles of `tile` consecutive segments."""
    return int((links.v1 // tile != links.v2 // tile).sum())


def sides_over(r, limit, tile):
    """Per tile: the number of sides with more than `limit` links."""
    n_tiles = -(-r.V // tile)
    heavy = np.flatnonzero(r.deg > limit) >> 1
    return np.bincount(heavy // tile, minlength=n_tiles).tolist()
