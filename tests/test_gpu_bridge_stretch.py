"""GPU tests of the far side's tour stretch that k_t0_parents hands to k_bridges (one 8-byte record per segment: where the
subtrees hanging off the far side begin and end in the tour, "the far side has no arc" and the hash bits of both sides).

Every graph is the smallest shape that drives one branch of the record.  The shapes are trees of segments whose only
non-tree links are self loops, so the spanning forest is forced (every other link is a bridge and therefore an arc) and
the slot geometry a name claims -- which side a segment is entered through, where the first forest slot of a side sits in
the segment's slot range -- is worked out on the CPU from the oracle's component dump and asserted before any GPU pass.
The forests of a plain pass are compared with the CPU oracle's texts and, array by array, with those of a pass whose tree
stage is the sequential one (POVU_HIP_F_SEQ_TREE), an independent implementation."""
import numpy as np
import pytest

import oracle_lib as O
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_NO_STAGE_TIMES, F_SEQ_TREE
from test_oracle import dump_component

pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
l, r = W.L, W.R


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


# ------------------------------------------------------------------ graphs
def graph(n, links):
    """n segments (ids 1..n) and links (a, side of a, b, side of b) by vertex idx."""
    a = np.array(links, dtype=np.int64).reshape(-1, 4)
    return W._mk(np.arange(1, n + 1), a[:, 0], a[:, 1], a[:, 2], a[:, 3])


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


def star(n_lr_loops, n_l, n_r, hang_root_on=l, tipless=False, x_first=True):
    """Segment X with `n_lr_loops` l-r self loops in front of n_l links out of its l side and n_r out of its r side, each to
    the l side of a leaf of its own.  The leaves' r sides are tips (the smallest leaf roots the tree, so X is entered through
    the side `hang_root_on` over the first link of that side) unless `tipless`: then every leaf carries a same-side self
    loop there, nothing is a tip and X = vertex 0 roots the tree at its l side."""
    n = 1 + n_l + n_r
    x = 0 if x_first else n - 1
    leaves = [v for v in range(n) if v != x]
    on_l, on_r = (leaves[:n_l], leaves[n_l:]) if hang_root_on == l else (leaves[n_r:], leaves[:n_r])
    links = [(x, l, x, r)] * n_lr_loops
    links += [(x, l, v, l) for v in on_l] + [(x, r, v, l) for v in on_r]
    if tipless:
        links += [(v, r, v, r) for v in leaves]
    return graph(n, links)


def chain(links_sides, tail=()):
    """Segments 0, 1, 2, ... joined one after the other: links_sides[k] = (side of segment k, side of segment k + 1);
    `tail` = more links."""
    return graph(len(links_sides) + 1, [(k, a, k + 1, b) for k, (a, b) in enumerate(links_sides)] + list(tail))


def child_in_front(e):
    """Segment 3 is entered through side e from segment 2 and has a child (segment 1) over a link of the same side with a
    smaller link id: the first forest slot of the entered side is not the entering one.  Segment 0 (its l side is the
    smallest tip) roots the tree."""
    return graph(5, [(0, r, 2, l), (1, r, 3, e), (2, r, 3, e), (3, 1 - e, 4, l)])


# ------------------------------------------------------------------ what a graph really looks like (CPU)
def component_geometry(g, comp):
    """Per segment of component `comp` (None: no such component), from the oracle's dump: the slots of its l and r side in
    link-id order as (link, is_arc), the side it is entered through, the entering link (None for the root) -- or
    {"forced": False} when the component has a cycle besides self loops (then its spanning forest is the GPU's choice)."""
    d = dump_component(g, comp)
    if d is None:
        return None
    nv = len(d["gidx"])
    sides = [[] for _ in range(2 * nv)]
    arcs = 0
    for k, (a, sa, b, sb) in enumerate(zip(d["ev1"].tolist(), d["es1"].tolist(), d["ev2"].tolist(), d["es2"].tolist())):
        arc = a != b
        arcs += arc
        sides[2 * a + sa].append((k, arc))
        sides[2 * b + sb].append((k, arc))  # (the component's graph holds every self loop as an l-r one: a slot on either side)
    out = {"nv": nv, "forced": arcs == nv - 1, "sides": sides, "gidx": d["gidx"]}
    # tips are sides without a link in the graph as given (there a same-side self loop is a link of its side alone)
    linked = set(zip(g.v1.tolist(), g.s1.tolist())) | set(zip(g.v2.tolist(), g.s2.tolist()))
    tips = [v for v in range(nv) if (d["gidx"][v], l) not in linked or (d["gidx"][v], r) not in linked]
    if tips:
        v = min(tips, key=lambda v: g.vid[d["gidx"][v]])
        root = 2 * v + (l if (d["gidx"][v], l) not in linked else r)
    else:
        root = 0
    out["root"], out["tipless"] = root, not tips
    if len(d["gid"]):  # (a decomposed component: the oracle's DFS starts there too)
        t0 = 1 if d["gid"][0] == NIL else 0
        assert d["gid"][t0] == g.vid[d["gidx"][root >> 1]] and d["typ"][t0] == (root & 1)
    if not out["forced"]:
        return out
    entered, enter_link = {root >> 1: root & 1}, {root >> 1: None}
    far_end = {}
    for k, (a, sa, b, sb) in enumerate(zip(d["ev1"].tolist(), d["es1"].tolist(), d["ev2"].tolist(), d["es2"].tolist())):
        if a != b:
            far_end[(2 * a + sa, k)] = 2 * b + sb
            far_end[(2 * b + sb, k)] = 2 * a + sa
    todo = [root >> 1]
    while todo:
        v = todo.pop()
        for s in (2 * v, 2 * v + 1):
            for k, arc in sides[s]:
                if arc and k != enter_link[v]:
                    w = far_end[(s, k)]
                    entered[w >> 1], enter_link[w >> 1] = w & 1, k
                    todo.append(w >> 1)
    assert len(entered) == nv
    out["entered"], out["enter_link"] = entered, enter_link
    return out


def properties(g):
    """The set of properties the segments of g have (names as in the cases below)."""
    props = set()
    loops = g.v1 == g.v2
    if np.any(loops & (g.s1 == g.s2)):
        props.add("same_side_self_loop")
    if np.any(loops & (g.s1 != g.s2)):
        props.add("lr_self_loop")
    c = 0
    while True:
        geo = component_geometry(g, c)
        if geo is None:
            break
        c += 1
        props.add(f"component_of_{geo['nv']}" if geo["nv"] <= 2 else "component_of_3_or_more")
        if geo["tipless"]:
            props.add("tipless_root_l0")
            assert geo["root"] == 0
        if not geo["forced"]:
            props.add("cycles")
            continue
        sides = geo["sides"]
        for v in range(geo["nv"]):
            e = geo["entered"][v]
            se, sf = sides[2 * v + e], sides[2 * v + (1 - e)]
            is_root = geo["enter_link"][v] is None
            side_name = "lr"[e]
            n_l = len(sides[2 * v])
            for s in (l, r):
                first = next((i for i, (_, arc) in enumerate(sides[2 * v + s]) if arc), None)
                if first is not None:
                    role = "entered" if s == e else "far"
                    props.add(f"first_arc_of_{'lr'[s]}_in_round_position_{((n_l if s == r else 0) + first) % 4}")
                    props.add(f"first_arc_of_{role}_side_in_round_position_{((n_l if s == r else 0) + first) % 4}")
                props.add(f"side_of_{len(sides[2 * v + s])}_slots")
            if len(se) + len(sf) > 8:
                props.add("segment_of_more_than_8_slots")
            arcs_e, arcs_f = [k for k, arc in se if arc], [k for k, arc in sf if arc]
            loops_f = [k for k, arc in sf if not arc]
            if is_root and geo["nv"] > 1:
                if arcs_e and arcs_f:
                    props.add("root_with_arcs_on_both_sides")
                    if len(arcs_e) < len(arcs_f):
                        props.add("root_start_side_few_far_side_many")
                if arcs_e and not arcs_f:
                    props.add("root_far_side_without_arc")
            if not arcs_f and geo["nv"] > 1:
                props.add("far_side_without_arc_" + ("with_nontree_links" if loops_f else "and_without_links"))
            if not is_root:
                if arcs_e[0] == geo["enter_link"][v]:
                    props.add(f"entered_{side_name}_first_arc_is_entering")
                else:
                    props.add(f"entered_{side_name}_child_arc_in_front")
                    if arcs_f:
                        props.add(f"entered_{side_name}_child_arc_in_front_and_far_side_arcs")
            if geo["nv"] == 1:
                props.add("component_of_1_" + ("with_loops" if se or sf else "bare"))
    return props


ONE, ONE_LR, ONE_SAME = graph(1, []), graph(1, [(0, l, 0, r)]), graph(1, [(0, r, 0, r), (0, l, 0, r)])
TWO, TWO_LOOPS = graph(2, [(0, r, 1, l)]), graph(2, [(0, r, 1, r), (1, l, 1, r), (0, l, 0, l)])
# no tip: vertex 0 roots the tree at its l side, where all its arcs are; its r side holds a self loop only
TIPLESS_ROOT_ONE_SIDED = graph(3, [(0, l, 1, l), (0, l, 2, l), (0, r, 0, r), (1, r, 1, r), (2, r, 2, r)])
ROUNDS = [star(k, a, b, hang_root_on=h, x_first=xf) for k in range(4) for a, b in ((1, 2), (2, 5), (5, 6), (4, 9 - k), (8 - k, 9 - k))
          for h in (l, r) for xf in (True, False)]

CASES = {
    # a tip-less tree: vertex 0 roots it at its l side and has arcs on both sides, 1 / 2 on the start side, 5 / 7 on the far side
    "root_both_sides": (concat([star(0, 1, 5, tipless=True), star(1, 2, 7, tipless=True), star(3, 1, 1, tipless=True)]),
                        {"root_with_arcs_on_both_sides", "root_start_side_few_far_side_many", "tipless_root_l0", "same_side_self_loop"}),
    # tips behind black edges: the far side bare, with a same-side self loop, and under an l-r self loop
    "far_side_without_arc": (concat([chain([(r, l), (r, l)]), chain([(r, l), (r, l)], [(2, r, 2, r)]), chain([(r, l), (r, l)], [(2, l, 2, r)]),
                                     chain([(r, r), (l, l), (r, r)], [(3, l, 3, l), (1, l, 1, r)]), star(0, 3, 0), star(2, 0, 3, hang_root_on=r), TIPLESS_ROOT_ONE_SIDED]),
                             {"far_side_without_arc_and_without_links", "far_side_without_arc_with_nontree_links", "lr_self_loop",
                              "same_side_self_loop", "root_far_side_without_arc"}),
    "entered_first_arc_is_entering": (concat([chain([(r, l), (r, r), (l, l), (r, l)]), star(0, 3, 4), star(1, 4, 3, hang_root_on=r)]),
                                      {"entered_l_first_arc_is_entering", "entered_r_first_arc_is_entering"}),
    "entered_child_arc_in_front": (concat([child_in_front(l), child_in_front(r), child_in_front(r), child_in_front(l)]),
                                   {"entered_l_child_arc_in_front", "entered_r_child_arc_in_front",
                                    "entered_l_child_arc_in_front_and_far_side_arcs", "entered_r_child_arc_in_front_and_far_side_arcs"}),
    "rounds_of_four_slots": (concat(ROUNDS),
                             {"side_of_5_slots", "side_of_8_slots", "side_of_9_slots", "segment_of_more_than_8_slots", "lr_self_loop"}
                             | {f"first_arc_of_{s}_in_round_position_{p}" for s in "lr" for p in range(4)}
                             | {f"first_arc_of_{s}_side_in_round_position_{p}" for s in ("far", "entered") for p in range(4)}),
    "self_loops": (concat([chain([(r, l), (r, l), (r, l)], [(1, l, 1, r)]), chain([(r, l), (r, l), (r, l)], [(1, r, 1, r), (2, l, 2, l)]),
                           chain([(r, r), (l, r)], [(1, l, 1, r), (1, r, 1, r), (1, l, 1, l)])]),
                   {"lr_self_loop", "same_side_self_loop"}),
    # voff / abase differ per component: components of one and of two segments in front of, between and behind larger ones
    "tiny_components": (concat([ONE, TWO, star(1, 2, 3), ONE_LR, child_in_front(l), TWO_LOOPS, ONE_SAME, TWO, star(0, 5, 1, tipless=True), ONE,
                                chain([(r, l)] * 6), TWO, ONE_LR]),
                        {"component_of_1", "component_of_2", "component_of_3_or_more", "component_of_1_bare", "component_of_1_with_loops",
                         "lr_self_loop", "same_side_self_loop"}),
    "tipless_ring": (W.hprc_circular(8), {"tipless_root_l0", "cycles"}),
    # 2101 segments: nine workgroups of k_t0_parents and of k_bridges
    "bubble_chain": (W.chain_of_bubbles(700), {"cycles", "component_of_3_or_more"}),
}


def forest_arrays(f):
    """Every array of every PVST of a forest, keyed by component id."""
    out = {}
    for i in range(len(f)):
        t = f.tree(i)
        out[t.component_id] = (t.n_vtx, t.n_links, t.a_id, t.z_id, t.a_or, t.z_or, t.parent, t.hairpins)
    return out


def same_arrays(a, b):
    if a.keys() != b.keys():
        return False
    return all(x[:2] == y[:2] and all(np.array_equal(p, q) for p, q in zip(x[2:], y[2:])) for x, y in ((a[k], b[k]) for k in a))


@pytest.mark.parametrize("name", list(CASES))
def test_far_side_stretch(hip, name):
    """The graph has the properties its case claims (CPU), and the plain pass's forest is the oracle's and, array by array,
    the sequential-tree pass's."""
    g, claims = CASES[name]
    missing = claims - properties(g)
    assert not missing, missing
    want = O.decompose(g)
    hip.upload(g)
    plain = hip.decompose()
    assert plain.texts() == want
    seq = hip.decompose(flags=F_SEQ_TREE)
    assert seq.texts() == want
    ref = forest_arrays(seq)
    assert same_arrays(forest_arrays(plain), ref)
    lean = hip.decompose(flags=F_NO_STAGE_TIMES)  # (the pass bench.py times)
    assert lean.texts() == want and same_arrays(forest_arrays(lean), ref)
    assert hip.seq_redo_count() == 0


def test_records_of_a_larger_pass_left_behind(hip):
    """The records live in the tour's list words: a small pass behind a large one, and a large one behind a small one, must
    see only their own."""
    big, small = CASES["bubble_chain"][0], CASES["tiny_components"][0]
    want_big, want_small = O.decompose(big), O.decompose(small)
    for g, want in ((big, want_big), (small, want_small), (big, want_big), (small, want_small)):
        hip.upload(g)
        assert hip.decompose().texts() == want
        assert hip.decompose(flags=F_NO_STAGE_TIMES).texts() == want
