"""Rows A and B of the scope table (graph_kernels.hip) directly: the per-side CSR of the upload, the union-find labelling
and the re-index, against a plain restatement (tests/rowb_ref.py) at their thresholds; every comparison is exact.

povu_hip_debug_csr reads what the last upload left; povu_hip_debug_row_b runs the row-B step of a pass -- the pass's own
function behind the pass's own set-up -- under the pass flags given and exports its arrays, the path it took (ROWB_* bits)
and the length of the union-find's cross list.  The bits are asserted, so a case cannot pass on another path than the one it is
there for.  Inputs come from tests/rowb_cases.py, whose conditions tests/test_rowb_inputs.py checks without a GPU.  Which
spanning forest the labelling marks is its own choice: the flags must be consistent, V - C in number and acyclic, no more.

A link is united from its smaller end, so a hub side only matters to the labelling through the far ends above it: the hubs
of heavy_128_129, heavy_parallel and heavy_257 have far ends above them that nothing else joins, the hub of heavy_last_side
(the last segment of its graph) has none, and is there for the offsets of the last, incomplete group of four sides alone.

    kernel                                         test function (cases)
    ---------------------------------------------  ------------------------------------------------------------
    k_side_degree                                  test_csr (all; a same-side loop counted once: side_64, loops_renumbered)
    k_slot_fill, k_side_sort                       test_csr (side_64 at the limit; the swap and the loop: sides_of_2_and_3)
    k_side_pairs + the radix sort                  test_csr (side_65, heavy_*)
    k_slot_other, k_slot_twin                      test_csr (all; loops: side_64, loops_renumbered; parallel links: heavy_parallel)
    k_infer_tips                                   test_csr (all but tips_given, which uploads its own)
    k_uf_tiles, lane path                          test_row_b (one_tile_chain, grouped; a side of UF_HEAVY links: heavy_128_129)
    k_uf_tiles, workgroup path                     test_row_b (heavy_257: unions in LDS; heavy_128_129, heavy_parallel: onto the cross list)
    k_uf_tiles, beyond the cap                     test_row_b (heavy_257: the segment behind every hub hangs on the hub side alone)
    k_uf_tiles, last group                         test_row_b (heavy_last_side: a hub side found in it; stripes: odd segment counts)
    k_uf_cross                                     test_row_b (tile_plus_one, permuted_chain, stripes, heavy_parallel: n_cross too)
    k_uf_flatten, k_labels_sorted, k_comp_of       test_row_b (grouped / grouped_one_swap; all), test_speculation_sequence
    k_sorted_vertices without a permutation        test_row_b (grouped: boundaries inside groups of four; tips_given; no_links)
    k_sorted_vertices with a permutation           test_row_b (stripes, grouped_one_swap, loops_renumbered; all under F_SORTED_ADJ)
    k_local_degree                                 test_row_b (grouped_one_loop, lists_4_5_loop: no permutation; stripes,
                                                   loops_renumbered: with one)
    k_local_adj, registers only                    test_row_b (one_tile_chain, grouped, stripes)
    k_local_adj, flushed                           test_row_b (lists_4_5_own, vdeg_48, loops_renumbered)
    k_local_adj, with loops                        test_row_b (lists_4_5_loop, grouped_one_loop, loops_renumbered)
    k_local_adj, speculative                       test_speculation_sequence (kept, overwritten, not started)
    k_first_slot, k_mark_first, k_local_edges,     test_row_b (side_64 / 65, heavy_*, vdeg_49; every case under F_SORTED_ADJ),
    k_local_slots                                  test_componetize (all)
    k_comp_edge_offsets                            test_row_b (all: voff / eoff / stats[0] as published to the host)
    the whole pass on top of these                 test_decompose_equals_the_oracle"""
import numpy as np
import pytest

import oracle_lib as O
import rowb_cases as RC
import rowb_ref
from povu_amd import HipDecomposer
from povu_amd.hip import F_NO_STAGE_TIMES, F_SORTED_ADJ, LLE_ID, LLE_TREE

pytestmark = pytest.mark.gpu

CASES = RC.cases()
FLAGS = [0, F_NO_STAGE_TIMES, F_SORTED_ADJ]


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def upload(hip, name):
    c = CASES[name]
    hip.upload(c.links, c.tips)
    return c, RC.reference(name)


def same(got, want, what):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ; first at {int(bad[0])}: {int(got[bad[0]])}, expected {int(want[bad[0]])}"


# ---------------------------------------------------------------------------------------------- row A
@pytest.mark.parametrize("name", RC.NAMES)
def test_csr(hip, name):
    c, r = upload(hip, name)
    got = hip.debug_csr(r.V, r.E)
    assert got["slot_fill"] == (c.slot_fill and r.E > 0)  # (a graph without links builds nothing)
    same(got["off"], r.off, "off")
    same(got["adj"], r.adj, "adj")
    same(got["aoth"], r.aoth, "aoth")
    same(got["tip"], r.tip, "tip")
    assert (got["max_vdeg"], got["n_empty_sides"]) == (r.max_vdeg, r.n_empty_sides)
    # the twin slots: an involution that stays on its link and points into the list of the other end
    tw, n = got["atwin"].astype(np.int64), r.adj.size
    assert ((tw >= 0) & (tw < n)).all()
    same(tw[tw], np.arange(n), "atwin[atwin]")
    same(r.adj[tw], r.adj, "adj[atwin]")
    assert ((r.off[r.aoth] <= tw) & (tw < r.off[r.aoth + 1])).all()
    same(tw, r.atwin, "atwin")


# ---------------------------------------------------------------------------------------------- row B
def check_row_b(c, r, got, flags):
    """Everything povu_hip_debug_row_b exports, but the `speculative kept` bit (only an implication here)."""
    want_path = RC.path_under(c.path, bool(flags & F_SORTED_ADJ))
    assert got["bits"] & ~RC.SPEC_KEPT == want_path, (got["bits"], want_path)
    if got["bits"] & RC.SPEC_KEPT:
        assert flags & F_NO_STAGE_TIMES and want_path == RC.IDENTITY | RC.SORT_FREE | RC.LEAN and r.E
    assert got["C"] == r.C
    same(got["voff"], r.voff, "voff")
    same(got["eoff"], r.eoff, "eoff")
    same(got["comp"], r.comp, "component")
    same(got["pos"], r.pos, "sorted position")
    assert got["n_cross"] == rowb_ref.cross_links(c.links, RC.UF_TILE)
    # the local lists: offsets, and the order of the far sides within every side
    same(got["loff"], r.loff, "loff")
    same(got["ladj"], r.ladj, "ladj")
    lle = got["lle"].astype(np.int64)
    assert (lle & ~(LLE_ID | LLE_TREE) == 0).all()
    # the ids, replaced by their dense rank over the whole graph, are the local link index + the component's link offset;
    # each occurs twice (at each end, or at the two sides of a self loop) and a side's ids ascend
    ids, rank, times = np.unique(lle & LLE_ID, return_inverse=True, return_counts=True)
    assert ids.size == r.E and (times == 2).all()
    same(rank, r.lle, "rank of the link ids")
    inside = np.ones(max(lle.size - 1, 0), dtype=bool)
    ends = r.loff[1:-1]
    inside[ends[(ends > 0) & (ends < lle.size)] - 1] = False
    assert (np.diff(lle & LLE_ID)[inside] > 0).all()
    # the forest flag: the same at both slots of a link, never on a self loop, V - C links without a cycle
    marks = np.bincount(rank, weights=(lle & LLE_TREE) != 0, minlength=r.E).astype(np.int64)
    assert np.isin(marks, (0, 2)).all(), np.flatnonzero(marks == 1)[:8]
    forest = marks == 2
    a, b = r.la >> 1, r.lb >> 1
    assert not forest[a == b].any()
    assert int(forest.sum()) == r.V - r.C
    parent = list(range(r.V))
    for x, y in zip(a[forest].tolist(), b[forest].tolist()):
        rx, ry = rowb_ref._find(parent, x), rowb_ref._find(parent, y)
        assert rx != ry, "the flagged links hold a cycle"
        parent[rx] = ry
    same(got["start_key"].astype(np.uint64).view(np.int64), r.start_key.view(np.int64), "start keys")
    assert got["stats0"] >= r.max_local_side
    if want_path & (RC.LEAN | RC.LOOPS) != RC.LEAN:  # (lean without loops: an upper bound, the most links on one segment)
        assert got["stats0"] == r.max_local_side


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", RC.NAMES)
def test_row_b(hip, name, flags):
    c, r = upload(hip, name)
    check_row_b(c, r, hip.debug_row_b(r.V, r.E, flags), flags)


@pytest.mark.parametrize("name", RC.NAMES)
def test_componetize(hip, name):
    c, r = upload(hip, name)
    got, want = hip.componetize(), rowb_ref.componetized(r, c.links)
    assert got["n_components"] == want["n_components"]
    for k in ("vtx_off", "link_off", "vtx_id", "vtx_tip", "v1", "s1", "v2", "s2"):
        same(got[k], want[k], k)


# the adjacency written ahead of the component count: kept, overwritten, not started
SEQUENCE = [("grouped", False), ("grouped", True), ("grouped_one_loop", False), ("grouped_one_swap", False), ("vdeg_49", False),
            ("grouped", True)]


def test_speculation_sequence():
    """On a context of its own, under F_NO_STAGE_TIMES.  The first pass of a context (and the first after release_workspace)
    has no arena to write ahead into; from then on a pass speculates whenever the sort-free builder is due, and keeps what
    it wrote only on a graph grouped by component without self loops.  Every step's arrays are checked in full: what a
    failed speculation wrote must be gone."""
    hip = HipDecomposer(0)
    try:
        for again in (False, True):
            if again:
                hip.release_workspace()
            for step, (name, kept) in enumerate(SEQUENCE):
                c, r = upload(hip, name)
                got = hip.debug_row_b(r.V, r.E, F_NO_STAGE_TIMES)
                assert bool(got["bits"] & RC.SPEC_KEPT) == kept, (again, step, name)
                check_row_b(c, r, got, F_NO_STAGE_TIMES)
    finally:
        hip.close()


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", [n for n in RC.NAMES if np.diff(RC.reference(n).voff).max() >= 3])
def test_decompose_equals_the_oracle(hip, name):
    c, _ = upload(hip, name)
    assert hip.decompose().texts() == O.decompose(c.links, c.tips)
