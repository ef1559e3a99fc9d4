"""CPU checks of back_edge_batches_cases: the oracle says whether every builder makes the shape its name claims -- that many
slots and that many back edges on that side, that side on that place of the kernel's grid, sides without a link on every
place of a tree, components that are not decomposed where they should be, components in and out of order."""
import numpy as np
import pytest

import back_edge_batches_cases as B
from povu_amd import workloads as W
from test_oracle import dump_component

l, r = W.L, W.R


def fat(g, last_side, tips=None):
    """(side index, slots, ordinary back edges out of it) of the side tail_fan makes fat."""
    seg, side = B.fat_side(g.n_vtx, last_side)
    d = dump_component(g, 0, tips=tips)
    S = 2 * seg + (0 if side == l else 1)
    return S, int(B.side_links(g)[S]), B.ordinary_back_edges_of(d, B.tree_vertex_of(d, g, seg, side))


@pytest.mark.parametrize("n", B.EDGE_SEGMENTS)
def test_segment_counts_on_the_edges(n):
    """2 n sides lie one segment in front of, on and behind a lane's iteration, a batch or a workgroup; the fat side is the
    last side of the graph, or the last but one."""
    assert min(abs(2 * n - e) for e in (B.LANE, B.BATCH, B.GROUP)) <= 2
    g = B.tail_fan(n, 4)
    assert g.n_vtx == n and fat(g, True) == (2 * n - 1, 4, 3)
    g = B.tail_fan(n, 3, last_side=False)
    assert g.n_vtx == n and fat(g, False) == (2 * n - 2, 3, 2)


def test_the_three_edges_are_all_there():
    sides = {2 * n for n in B.EDGE_SEGMENTS}
    for e in (B.LANE, B.BATCH, B.GROUP):
        assert {e - 2, e, e + 2} <= sides


def test_fat_sides_that_are_first_in_their_workgroup():
    S, slots, k = fat(B.tail_fan(1025, 3, last_side=False), False)
    assert S == B.GROUP and (slots, k) == (3, 2)
    S, slots, k = fat(B.tail_fan(2049, 6, last_side=False), False)
    assert S == 2 * B.GROUP and (slots, k) == (6, 5)


@pytest.mark.parametrize("slots", B.SLOTS)
def test_slots_and_back_edges_per_side(slots):
    assert fat(B.tail_fan(slots + 6, slots), True)[1:] == (slots, slots - 1)
    if slots > 1:  # a parallel link: one more slot, no more back edges
        assert fat(B.tail_fan(slots + 7, slots, last_side=False, parallel=1), False)[1:] == (slots + 1, slots - 1)


def test_the_listed_counts_are_covered():
    assert {1, 2, 3, 4, 5, 8, 9} <= set(B.SLOTS)                    # the `rem` edges of a round of four
    assert {0, 1, 2, 3, 5} <= {s - 1 for s in B.SLOTS}              # back edges per side; two is the LDS path's edge


def test_sides_without_a_link_on_every_place():
    assert B.linkless_places(B.linkless()) == {"child of the dummy root", "deeper"}
    g = B.linkless_no_tips()
    assert B.linkless_places(g, tips=np.zeros(g.n_vtx, dtype=np.uint8)) == {"root", "child of the root", "deeper"}
    # the root without a link has its back edge to itself (the target is the root: the remembered bit)
    d = dump_component(g, 0, tips=np.zeros(g.n_vtx, dtype=np.uint8))
    be = list(zip(d["be_src"][: d["n_be0"]].tolist(), d["be_tgt"][: d["n_be0"]].tolist()))
    assert (0, 0) in be


def decomposed(g, tips=None):
    """Per component: does it have a tree."""
    out, c = [], 0
    while True:
        d = dump_component(g, c, tips=tips)
        if d is None:
            return out
        out.append(len(d["gid"]) > 0)
        c += 1


def test_small_components_on_every_side_of_decomposed_ones():
    dec = decomposed(B.small_around())
    assert not dec[0] and not dec[-1] and any(dec)
    first, last = dec.index(True), len(dec) - 1 - dec[::-1].index(True)
    assert not all(dec[first:last + 1])                             # ... and between them


def test_the_run_of_small_components_fills_whole_batches():
    g = B.small_run()
    dec = decomposed(g)
    # the longest run of sides that are in no tree covers a batch of some lane (its four sides lie 256 apart): BATCH sides
    comp_sizes = np.bincount(component_labels(g))
    run = best = 0
    for has_tree, size in zip(dec, comp_sizes):
        run = 0 if has_tree else run + 2 * int(size)
        best = max(best, run)
    assert best >= B.BATCH + B.LANE and dec[0] and dec[-1]


component_labels = B.component_labels


@pytest.mark.parametrize("valid,invalid", B.NIL_TAILS)
def test_invalid_tail_entries(valid, invalid):
    """That many segments without a class entry behind that many with one (the class pass of the black tree edges has one
    entry per segment); the decomposed component comes first."""
    g = B.nil_tail(valid, invalid)
    assert g.n_vtx == valid + invalid and B.segments_without_a_tree(g) == invalid
    assert decomposed(g)[0] and not any(decomposed(g)[1:])


def test_the_tails_end_inside_a_lane_and_on_its_edge():
    assert {i % 4 for _, i in B.NIL_TAILS} == {0, 1, 3} and {v % 4 for v, _ in B.NIL_TAILS} == {0, 1, 3}


@pytest.mark.parametrize("loops", [False, True])
def test_components_in_and_out_of_order(loops):
    a, b = B.identity_order(loops), B.renumbered(loops)
    la, lb = component_labels(a), component_labels(b)
    assert (np.diff(la) >= 0).all()                                  # in order: every component owns a range of segments
    assert (np.diff(lb) < 0).any()                                   # interleaved: the re-index has to renumber
    assert np.array_equal(np.sort(np.bincount(la)), np.sort(np.bincount(lb))) and a.n_links == b.n_links
    self_loops = int((b.v1 == b.v2).sum())
    assert (self_loops > 0) == loops and int((a.v1 == a.v2).sum()) == self_loops


def test_fat_sides_of_the_dupflag_and_word_form_cases():
    cases = B.cases()
    assert int(B.side_links(cases["70 links on one side"]).max()) == 70      # more than 64: dupflag
    assert int(B.side_links(cases["254 links on one side"]).max()) == 254    # 254 + 2 does not fit a byte
    assert cases["five segments, no link"].n_links == 0 and cases["one segment"].n_vtx == 1
    assert cases["two segments, one link"].n_vtx == 2
    for name in B.NO_TIPS:
        assert name in cases
