"""The inputs of tests/test_gpu_rowb.py have the properties they are there for (tests/rowb_cases.py), the plain restatement
of rows A and B (tests/rowb_ref.py) agrees with the oracle's componetize, and the constants stated with the cases are the
ones of the sources.  numpy alone, no GPU."""
import os
import re

import numpy as np
import pytest

import rowb_cases as RC
import rowb_ref
from povu_amd import workloads as W
from test_oracle import dump_component

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "povu_amd", "csrc", "hip")
CASES = RC.cases()


def test_constants_mirror_the_sources():
    g = open(os.path.join(HIP, "graph_kernels.hip")).read()
    assert re.search(r"#define POVU_UF_TILE (\d+)", g).group(1) == str(RC.UF_TILE)
    assert re.search(r"#define POVU_UF_TPB (\d+)", g).group(1) == str(RC.UF_TPB)
    heavy, cap = re.search(r"UF_TILE = POVU_UF_TILE, UF_TPB = POVU_UF_TPB, UF_HEAVY = (\d+), UF_HEAVY_CAP = (\d+);", g).groups()
    assert (int(heavy), int(cap)) == (RC.UF_HEAVY, RC.UF_HEAVY_CAP)
    assert re.search(r"constexpr uint32_t UF_GROUPS = (\d+);", g).group(1) == str(RC.UF_GROUPS)
    assert "b[gq][j + 1] - b[gq][j] > UF_HEAVY" in g and "if (q < UF_HEAVY_CAP)" in g  # MORE than UF_HEAVY links; the cap
    assert re.search(r"static constexpr uint32_t FILL_MAX_SIDE_DEGREE = (\d+);", g).group(1) == str(RC.FILL_MAX_SIDE_DEGREE)
    assert "hw[3] <= FILL_MAX_SIDE_DEGREE" in g
    assert re.search(r"static constexpr uint32_t SORT_FREE_MAX_VDEG = (\d+);", g).group(1) == str(RC.SORT_FREE_MAX_VDEG)
    assert "g.max_vdeg <= SORT_FREE_MAX_VDEG" in g
    # k_local_adj: four entries in registers, the fifth flushes them
    assert f"if (n < {RC.LOCAL_ADJ_REGS}) {{" in g and f"if (n == {RC.LOCAL_ADJ_REGS}) {{" in g and f"if (n <= {RC.LOCAL_ADJ_REGS}) {{" in g
    assert len(re.findall(r"l(\d) = NIL32", g)) == RC.LOCAL_ADJ_REGS
    head = open(os.path.join(ROOT, "include", "povu_hip.h")).read()
    bits = {k: int(v) for k, v in re.findall(r"#define POVU_HIP_ROWB_(\w+) (\d+)u", head)}
    assert bits == dict(IDENTITY=RC.IDENTITY, SORT_FREE=RC.SORT_FREE, LEAN_IDENTITY=RC.LEAN, SELF_LOOPS=RC.LOOPS,
                        DENSE_EDGES=RC.DENSE, SPEC_KEPT=RC.SPEC_KEPT)
    from povu_amd import hip
    assert (hip.ROWB_IDENTITY, hip.ROWB_SORT_FREE, hip.ROWB_LEAN_IDENTITY, hip.ROWB_SELF_LOOPS, hip.ROWB_DENSE_EDGES,
            hip.ROWB_SPEC_KEPT) == (RC.IDENTITY, RC.SORT_FREE, RC.LEAN, RC.LOOPS, RC.DENSE, RC.SPEC_KEPT)
    lle_id, lle_tree = re.search(r"LLE_ID = (0x[0-9A-F]+)u, LLE_TREE = (0x[0-9A-F]+)u;", open(os.path.join(HIP, "graph_kernels.hpp")).read()).groups()
    assert (int(lle_id, 16), int(lle_tree, 16)) == (hip.LLE_ID, hip.LLE_TREE)


def test_the_cases_are_the_ones_listed():
    assert list(CASES) == RC.NAMES
    shuffled = sum(bool((np.diff(c.links.vid.astype(np.int64)) < 0).any()) for c in CASES.values())
    assert shuffled == RC.SHUFFLED_IDS and 2 * shuffled >= len(CASES)
    for c in CASES.values():
        assert c.links.n_vtx <= 3 * RC.UF_TILE + 1 and c.links.n_links <= 70000, c.name
        assert np.unique(c.links.vid).size == c.links.n_vtx, c.name
    # link order is shuffled, and about half the links name their larger end first, unless the case keeps its order
    for name in ("sides_of_2_and_3", "permuted_chain", "stripes", "grouped", "heavy_257"):
        g = CASES[name].links
        two = g.v1 != g.v2
        assert 0.4 < (g.v1[two] > g.v2[two]).mean() < 0.6, name
    g = CASES["one_tile_chain"].links
    assert np.array_equal(g.v1, np.arange(RC.UF_TILE - 1)) and np.array_equal(g.v2, g.v1 + 1)
    for n in (64, 65):  # given in descending order of the far end
        g = CASES[f"side_{n}"].links
        hub = np.flatnonzero((g.v1 == 0) & (g.v2 != 0))
        assert hub.size == n - 1 and (np.diff(g.v2[hub].astype(np.int64)) <= 0).all() and (np.diff(hub) == 1).all()


def compare_with_dump(g, tips, r):
    for c in range(r.C):
        d = dump_component(g, c, tips)
        want = rowb_ref.component(r, c)
        for k in ("gidx", "ev1", "es1", "ev2", "es2"):
            assert np.array_equal(d[k], want[k]), (c, k)
    assert dump_component(g, r.C, tips) is None


@pytest.mark.parametrize("name", [n for n in RC.NAMES if CASES[n].links.n_vtx <= 2000])
def test_restatement_equals_the_oracle_on_the_small_cases(name):
    c = CASES[name]
    compare_with_dump(c.links, c.tips, RC.reference(name))


@pytest.mark.parametrize("shape, loops", [((300, 520, 11), 0), ((64, 400, 5), 1), ((40, 300, 23), 2)])
def test_restatement_equals_the_oracle_on_random_graphs(shape, loops):
    g = W.random_bidirected(*shape, self_loops=True)
    r = rowb_ref.build(g)
    assert r.has_self_loops == (loops > 0) and ((g.v1 == g.v2) & (g.s1 == g.s2)).any() == (loops > 1)  # (2: same-side loops among them)
    compare_with_dump(g, None, r)


def test_restatement_of_a_graph_small_enough_to_check_by_hand():
    # 0 -r l- 2, 2 -r r- 2 (same-side loop), 1 alone, 3 -l r- 3 (l-r loop), links given out of order
    g = W._mk([10, 20, 30, 40], [2, 3, 2], [W.R, W.L, W.L], [2, 3, 0], [W.R, W.R, W.R])
    r = rowb_ref.build(g)
    assert r.off.tolist() == [0, 0, 1, 1, 1, 2, 3, 4, 5] and r.adj.tolist() == [2, 2, 0, 1, 1]
    assert r.aoth.tolist() == [4, 1, 5, 7, 6] and r.atwin.tolist() == [1, 0, 2, 4, 3]
    assert r.tip.tolist() == [1, 1, 0, 0] and (r.max_side, r.max_vdeg, r.n_empty_sides) == (1, 2, 3)
    assert r.C == 3 and r.comp.tolist() == [0, 1, 0, 2] and r.pos.tolist() == [0, 2, 1, 3] and r.voff.tolist() == [0, 2, 3, 4]
    assert r.la.tolist() == [1, 3, 6] and r.lb.tolist() == [2, 2, 7] and r.eoff.tolist() == [0, 2, 2, 3]
    assert r.loff.tolist() == [0, 0, 1, 3, 4, 4, 4, 5, 6] and r.ladj.tolist() == [2, 1, 3, 2, 7, 6] and r.lle.tolist() == [0, 0, 1, 1, 2, 2]
    assert r.start_key.tolist() == [(10 << 32) | 0, (20 << 32) | 4, rowb_ref.NO_KEY]


# ---------------------------------------------------------------------------------------------- what each case is there for
@pytest.mark.parametrize("name", RC.NAMES)
def test_case_takes_the_path_it_states(name):
    c, r = CASES[name], RC.reference(name)
    identity = r.C == 1 or r.labels_sorted
    free = r.max_vdeg <= RC.SORT_FREE_MAX_VDEG
    path = (RC.IDENTITY if identity else 0) | (RC.SORT_FREE if free else 0) | (RC.LEAN if identity and free else 0) | \
           (RC.LOOPS if r.has_self_loops else 0) | (0 if free else RC.DENSE)
    assert path == c.path
    assert RC.path_under(c.path, True) == (path & (RC.IDENTITY | RC.LOOPS)) | RC.DENSE and RC.path_under(c.path, False) == path
    assert c.slot_fill == (r.max_side <= RC.FILL_MAX_SIDE_DEGREE)
    if c.C is not None:
        assert r.C == c.C
    if c.cross is not None:
        assert rowb_ref.cross_links(c.links, RC.UF_TILE) == c.cross
    for k in ("max_side", "max_vdeg"):
        if k in c.info:
            assert getattr(r, k) == c.info[k]
    if "heavy_per_tile" in c.info:
        assert rowb_ref.sides_over(r, RC.UF_HEAVY, RC.UF_TILE) == c.info["heavy_per_tile"]
    if "list_lengths" in c.info:
        assert c.info["list_lengths"] <= set(r.ldeg.tolist())
    # every link sits once at either end, the twins point at each other
    assert r.loff[-1] == 2 * r.E and np.array_equal(r.atwin[r.atwin], np.arange(r.adj.size))


def test_row_a_cases():
    for n in (RC.FILL_MAX_SIDE_DEGREE, RC.FILL_MAX_SIDE_DEGREE + 1):
        c, r = CASES[f"side_{n}"], RC.reference(f"side_{n}")
        g = c.links
        assert r.deg[1] == n == r.max_side and np.sort(r.deg)[-2] < 4
        loops = (g.v1 == 0) & (g.v2 == 0) & (g.s1 == g.s2)
        assert loops.sum() == 1
        far, times = np.unique(g.v2[(g.v1 == 0) & ~loops], return_counts=True)
        assert sorted(times.tolist())[-2:] == [1, 2]  # one pair of parallel links
    r = RC.reference("sides_of_2_and_3")
    assert (r.deg[1:2000:4] == 2).all() and (r.deg[3:2000:4] == 3).all() and r.max_vdeg <= RC.SORT_FREE_MAX_VDEG
    adj2 = CASES["sides_of_2_and_3"].links  # the two links of a side are given in either order of their far ends
    assert CASES["no_links"].links.n_vtx == 5 and CASES["no_links"].links.n_links == 0 and adj2.n_links == 2500 + 999
    assert CASES["one_segment"].links.n_vtx == 1 and CASES["one_segment"].links.n_links == 0
    c, r = CASES["tips_given"], RC.reference("tips_given")
    inferred = rowb_ref.build(c.links).tip
    assert (inferred != c.tips).sum() == 5 and np.array_equal(r.tip, c.tips)
    marked = np.flatnonzero(c.tips)
    assert any(r.deg[2 * v] and r.deg[2 * v + 1] for v in marked)  # a tip mark on a segment with links on both sides
    assert r.start_key[0] != rowb_ref.NO_KEY and r.start_key[1] == rowb_ref.NO_KEY  # a component without a tip has no key


def test_labelling_cases():
    T = RC.UF_TILE
    assert CASES["one_tile_chain"].links.n_vtx == T and CASES["tile_plus_one"].links.n_vtx == T + 1
    c = CASES["permuted_chain"]
    lo, hi = c.info["cross_share"]
    assert c.links.n_vtx == 2 * T + 3 and lo < rowb_ref.cross_links(c.links, T) / c.links.n_links < hi
    # stripes: an odd count over three tiles and a segment; seven interleaved components, the pair, the isolated segments
    c, r = CASES["stripes"], RC.reference("stripes")
    assert c.links.n_vtx == 3 * T + 1 and c.links.n_vtx % 2 == 1 and not r.labels_sorted
    sizes = np.sort(np.diff(r.voff))
    assert sizes[:len(RC.STRIPES_ISOLATED)].tolist() == [1] * len(RC.STRIPES_ISOLATED) and sizes[len(RC.STRIPES_ISOLATED)] == 2 and (sizes[-7:] > 3000).all()
    p, q = RC.STRIPES_PAIR
    assert p // T == 0 and q // T == 2 and r.comp[p] == r.comp[q] and (r.comp == r.comp[p]).sum() == 2
    assert T - 1 in RC.STRIPES_ISOLATED and all(r.deg[2 * v] + r.deg[2 * v + 1] == 0 for v in RC.STRIPES_ISOLATED)
    assert rowb_ref.cross_links(c.links, T) == 2 * 7 + 1
    # grouped: no boundary a multiple of 4 but the one at the tile's edge
    assert [b % 4 == 0 for b in RC.GROUPED_BOUNDS[1:-1]] == [False, True, False, False] and RC.GROUPED_BOUNDS[2] == T
    r = RC.reference("grouped")
    assert r.voff.tolist() == list(RC.GROUPED_BOUNDS) and r.labels_sorted and not r.has_self_loops and r.max_side <= 3
    g, g1 = CASES["grouped"].links, CASES["grouped_one_loop"].links
    r1 = RC.reference("grouped_one_loop")
    assert g1.n_links == g.n_links + 1 and r1.has_self_loops and r1.labels_sorted and r1.max_side <= 3
    loop = np.flatnonzero(g1.v1 == g1.v2)
    assert loop.size == 1 and g1.v1[loop[0]] == g1.n_vtx - 1 and g1.s1[loop[0]] != g1.s2[loop[0]]
    r2 = RC.reference("grouped_one_swap")
    x, y = RC.GROUPED_SWAP
    assert not r2.labels_sorted and r2.C == 5 and r.comp[x] != r.comp[y]
    assert np.flatnonzero(r2.comp != r.comp).tolist() == [x, y] and r2.comp[x] == r.comp[y] and r2.comp[y] == r.comp[x]
    # the hub sides.  Sides with MORE than UF_HEAVY links per tile (test_case_takes_the_path_it_states): heavy_128_129 has one
    # (its side of exactly UF_HEAVY links stays with its lane: two sides of at least UF_HEAVY), heavy_parallel one in either of
    # its two tiles (the ends of the bundle), heavy_257 UF_HEAVY_CAP + 1, heavy_last_side one
    c, r = CASES["heavy_128_129"], RC.reference("heavy_128_129")
    for hub, n in ((RC.HUB_128, RC.UF_HEAVY), (RC.HUB_129, RC.UF_HEAVY + 1)):
        assert hub // T == 0 and (2 * hub + 1) % 4 == 1 and r.deg[2 * hub + 1] == n  # the second side of its group of four
        assert sorted(r.deg[[2 * hub, 2 * hub + 2, 2 * hub + 3]].tolist()) == [1, 2, 5]
        far = r.aoth[r.off[2 * hub + 1]:r.off[2 * hub + 2]] >> 1
        assert abs(int((far >= T).sum()) - n / 2) <= 1
    assert int((r.deg >= RC.UF_HEAVY).sum()) == c.info["sides_at_least_heavy"]
    c, r = CASES["heavy_parallel"], RC.reference("heavy_parallel")
    u, w = RC.PARALLEL_ENDS
    par = (np.minimum(c.links.v1, c.links.v2) == u) & (np.maximum(c.links.v1, c.links.v2) == w)
    assert par.sum() == RC.UF_HEAVY + 1 and r.deg[2 * u] == r.deg[2 * w + 1] == RC.UF_HEAVY + 1 and u // T != w // T
    c, r = CASES["heavy_257"], RC.reference("heavy_257")
    assert c.links.n_vtx == T and sorted(set(r.deg[r.deg > RC.UF_HEAVY].tolist())) == [RC.UF_HEAVY + 1] and np.sort(r.deg)[-RC.UF_HEAVY_CAP - 2] <= 5
    for h in c.info["hubs"].tolist():  # the segment behind every hub hangs on the hub's r side alone
        assert r.deg[2 * h + 1] == RC.UF_HEAVY + 1 and r.deg[2 * h + 2] + r.deg[2 * h + 3] == 1 and r.aoth[r.off[2 * h + 2]] == 2 * h + 1
    c, r = CASES["heavy_last_side"], RC.reference("heavy_last_side")
    V = c.links.n_vtx
    assert V % 2 == 1 and (2 * V) % 4 == 2 and c.info["hub_side"] == 2 * V - 1 and r.deg[2 * V - 1] == RC.UF_HEAVY + 1
    assert (2 * V - 1) % 4 == 1  # the second side of the last group of four, whose last two sides do not exist


def test_reindex_cases():
    for n in (RC.SORT_FREE_MAX_VDEG, RC.SORT_FREE_MAX_VDEG + 1):
        r = RC.reference(f"vdeg_{n}")
        assert r.max_vdeg == n == r.deg[60] + r.deg[61] and min(r.deg[60], r.deg[61]) == n // 2 and np.sort(r.deg[0::2] + r.deg[1::2])[-2] == 1
    for name, loop in (("lists_4_5_own", False), ("lists_4_5_loop", True)):
        c, r = CASES[name], RC.reference(name)
        assert r.C == 1 and r.has_self_loops == loop
        for want, v in zip((3, 4, 5, 6), RC.LISTS_CENTRES):
            S = 2 * v  # (one component: sorted side = global side)
            assert r.ldeg[S] == want and r.deg[S] == want - (1 if loop else 0)
            ids, other = r.lle[r.loff[S]:r.loff[S + 1]], r.ladj[r.loff[S]:r.loff[S + 1]]
            assert (np.diff(ids) > 0).all()
            # the order the entries ARRIVE in (own slots ascend by link, the loop of the opposite side last): ids from
            # twins (far end below) and own ids (far end above) alternate
            slots = np.arange(r.off[S], r.off[S + 1])
            below = (r.aoth[slots] >> 1) < v
            assert below.tolist() == [k % 2 == 0 for k in range(slots.size)]
            if loop:
                assert (other == S + 1).sum() == 1 and r.deg[S + 1] == 2
    c, r = CASES["loops_renumbered"], RC.reference("loops_renumbered")
    g = c.links
    same = g.v1 == g.v2
    kinds = {(int(v), int(a), int(b)) for v, a, b in zip(g.v1[same], g.s1[same], g.s2[same])}
    assert {(4, 0, 0), (7, 1, 1), (13, 0, 0), (13, 1, 1)} <= kinds and any(v == 10 and a != b for v, a, b in kinds)
    assert sum(same & (g.v1 == 21)) == 2 and sum(same & (g.v1 == 24)) == 2 and sum(same & (g.v1 == 27)) == 2  # parallel copies
    assert not r.labels_sorted and (r.pos != np.arange(r.V)).any() and r.C == 2
