"""GPU tests of the batched gathers of the tree stage (common.hpp: gather_if / landed).  The kernels that take four adjacency
slots a round load the words those slots lead to UNCONDITIONALLY, from a clamped index where a slot does not ask for one
(behind the end of a side's list, no forest slot, no parent): every shape here puts such a clamp, or the 16-byte load in front
of it, on a boundary -- the last slots of the LAST side of the graph, the `rem` boundaries of a round (1, 2, 3, 4, 5, 8, 9 and
12 links on a side), a far segment with exactly 8 and with 9 slots (the in-register search of k_tour_words), no link at all
(the first ranking never runs and its ranks stay null), roots and components too small to be decomposed on every side of
decomposed ones -- and runs it again behind a larger graph, so that slack and dead workspace hold old data.

Every case compares the forests with the CPU oracle's texts; where a component is decomposed its tree (parents, root bits,
types, colours) is compared with the oracle's dump as well."""
import numpy as np
import pytest

import oracle_lib as O
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_ALL_VERTEX_CLASSES, F_NO_STAGE_TIMES
from test_gpu_bridge_stretch import graph, star
from test_gpu_root_bit import check_roots, check_roots_all, mixed, ring
from test_gpu_stack_lookups import concat, sized_components

pytestmark = pytest.mark.gpu

l, r = W.L, W.R
FLAGS = [0, F_NO_STAGE_TIMES, F_ALL_VERTEX_CLASSES]  # (F_NO_STAGE_TIMES: the speculative re-index and the early k_events)


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


# ------------------------------------------------------------------ graphs
def fan(d, where):
    """A hub segment one side of which carries d links, each to a leaf of its own; the leaves meet again in a sink, so all
    but one of the hub's links and of the sink's close a cycle, and a tail of two segments hangs off the hub's other side.
    `where`: the hub's full side is the FIRST side of the graph (l of segment 0), the LAST one (r of the last segment) or one
    in the MIDDLE (r of a segment with leaves on both sides of it)."""
    n = d + 4
    if where == "first":
        hub, hs, rest = 0, l, list(range(1, n))
    elif where == "last":
        hub, hs, rest = n - 1, r, list(range(n - 1))
    else:
        hub, hs = n // 2, r
        rest = [v for v in range(n) if v != hub]
    leaves, sink, t1, t2 = rest[:d], rest[d], rest[d + 1], rest[d + 2]
    links = [(hub, hs, v, l) for v in leaves] + [(v, r, sink, l) for v in leaves]
    links += [(hub, 1 - hs, t1, l), (t1, r, t2, l)]
    return graph(n, links)


def loops_and_parallels():
    """Same-side self loops, l-r self loops and parallel links, on sides with other links in front of and behind them."""
    return graph(6, [(0, r, 1, l), (1, r, 1, r), (1, r, 2, l), (1, r, 2, l), (2, r, 2, l), (2, r, 3, l), (2, r, 3, l), (2, r, 3, l),
                     (3, r, 3, l), (3, l, 3, l), (3, r, 4, l), (4, r, 5, l), (4, r, 5, l), (5, r, 5, r), (5, r, 5, l)])


def far_slots(n_l, n_r):
    """A chain 0 > 1 > 2 whose last segment leads into segment X (3), n_l slots on its l side and n_r on its r side in all:
    the look-up of X from segment 2 goes over a forest link, and so do those from X's leaves."""
    links = [(0, r, 1, l), (1, r, 2, l), (2, r, 3, l)]
    v = 4
    for side, cnt in ((l, n_l - 1), (r, n_r)):
        for _ in range(cnt):
            links.append((3, side, v, l))
            v += 1
    links += [(4, r, 5, r)] if v > 5 else []  # one cycle through X
    return graph(v, links)


def small_around():
    """Components of one and two segments in front of, between and behind decomposed ones."""
    return concat([sized_components([1, 2]), fan(3, "middle"), sized_components([2, 1, 1]), W.bubble_zoo(3, 3, 5, shuffle_ids=False),
                   sized_components([1]), ring(4), sized_components([2])])


def cases():
    out = {"one segment": sized_components([1]), "five segments, no link": graph(5, []),
           "two segments, one link": graph(2, [(0, r, 1, l)])}
    for d in (1, 2, 3, 4, 5, 8, 9, 12):
        for where in ("first", "middle", "last"):
            out[f"{d} links on the {where} side"] = fan(d, where)
    out["far segment with 8 slots"] = far_slots(3, 5)
    out["far segment with 9 slots"] = far_slots(3, 6)
    out["far segment with 8 slots, all on r"] = far_slots(1, 7)
    out["far star with 8 slots, last"] = star(0, 3, 5, x_first=False)
    out["far star with 9 slots, l-r loop"] = star(1, 3, 4, tipless=True)
    out["70 links on one side"] = fan(70, "last")
    out["self loops and parallel links"] = loops_and_parallels()
    out["rings"] = concat([ring(3), ring(4), ring(9)])
    out["small components around"] = small_around()
    out["mixed"] = mixed()
    return out


CASES = cases()
_WANT = {}


def want(name):
    if name not in _WANT:
        _WANT[name] = O.decompose(CASES[name])
    return _WANT[name]


# ------------------------------------------------------------------ tests
def test_shapes_are_what_their_names_say():
    """(no GPU work) the side that carries d links is the first / the last side of the graph, X has 8 / 9 slots."""
    def side_links(g):
        return np.bincount(np.concatenate([2 * g.v1.astype(np.int64) + g.s1, 2 * g.v2.astype(np.int64) + g.s2]), minlength=2 * g.n_vtx)
    for d in (1, 2, 3, 4, 5, 8, 9, 12, 70):
        assert side_links(fan(d, "first"))[0] == d and side_links(fan(d, "last"))[-1] == d
        m = fan(d, "middle")
        assert side_links(m)[2 * (m.n_vtx // 2) + 1] == d
    for g, n in ((far_slots(3, 5), 8), (far_slots(3, 6), 9), (far_slots(1, 7), 8)):
        s = side_links(g)
        assert s[6] + s[7] == n
    assert CASES["five segments, no link"].n_links == 0 and CASES["one segment"].n_links == 0


@pytest.mark.parametrize("name", list(CASES))
def test_forests_equal_the_oracle(hip, name):
    g = CASES[name]
    hip.upload(g)
    for flags in FLAGS:
        assert hip.decompose(flags=flags).texts() == want(name), flags
    hip.decompose()
    check_roots(hip, g)


def test_again_behind_a_larger_graph(hip):
    """Every graph right behind a larger one on the same context: the slack behind the arrays and the workspace a small graph
    does not write hold the larger graph's data."""
    big = W.hprc_shaped([400, 150], seed=3, tiny=5)
    want_big = O.decompose(big)
    for k, name in enumerate(CASES):
        if k % 6 == 0:
            hip.upload(big)
            assert hip.decompose(flags=FLAGS[(k // 6) % 3]).texts() == want_big
        hip.upload(CASES[name])
        for flags in FLAGS:
            assert hip.decompose(flags=flags).texts() == want(name), (name, flags)


@pytest.mark.parametrize("name", ["mixed", "small components around"])
def test_as_shard_one_of_two(hip, name):
    """The components of the other shard get inert words (no tree); those of this one have the oracle's trees, and the two
    shards together hold every decomposed component once.  A whole pass behind them equals the oracle."""
    g = CASES[name]
    hip.upload(g)
    seen = 0
    for rank in (0, 1):
        hip.decompose(rank=rank, world=2)
        seen += check_roots(hip, g, shard=rank)[0]
    assert seen == check_roots_all(g)
    assert hip.decompose().texts() == want(name)
