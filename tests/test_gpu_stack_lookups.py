"""GPU tests of what row G looks up instead of storing: the component of a candidate-stack entry (a bit-rank directory over
"a non-empty component starts here" + the list of those components), the number of flubbles opened in front of an entry (a
bit-rank directory over the flag bytes) and "the class occurred before" (bit 1 of the flag byte; the word array `prev` only
exists when the laminarity check runs).  Every case is decided by the CPU oracle."""
import os

import numpy as np
import pytest

import oracle_lib as O
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_ALL_VERTEX_CLASSES, F_CHECK_LAMINAR, F_NO_STAGE_TIMES, F_SUBFLUBBLES
from test_oracle import dump_component

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


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


def check_hooks(hip, g):
    """debug_tree / debug_stack / debug_edge_ids of every decomposed component against the oracle's dump."""
    c = checked = 0
    while True:
        d = dump_component(g, c)
        if d is None:
            break
        if len(d["gid"]):
            t = hip.debug_tree(c)
            assert np.array_equal(t["gid"], d["gid"]) and np.array_equal(t["par"], d["par"]), c
            assert np.array_equal(t["typ"], d["typ"]) and np.array_equal(t["black"], d["pe_black"]), c
            s = hip.debug_stack(c)
            assert np.array_equal(s["tree_vtx"], d["s_st_idx"] + 1), c
            assert np.array_equal(s["next_seen"], d["next_seen"]), c

            def canon(x):
                m = {}
                return [m.setdefault(v, len(m)) for v in x.tolist()]
            assert canon(s["cls"]) == canon(d["s_cls"]), c
            assert np.array_equal(hip.debug_edge_ids(c), d["pe_id"]), c
            checked += 1
        c += 1
    return checked


BOUNDARY_SIZES = [
    [64, 64, 128, 256, 5],                   # components start at 64, 128, 256, 512
    [3, 61, 1, 2, 64, 1, 127, 1, 257, 2],    # starts at 3, 64, 128, 255; ends at 64, 128, 255, 512; empty ranges in between
    [1, 2, 1, 256, 2, 2, 256, 1, 512, 3, 1], # undecomposed components first, last and between tile boundaries
    [255, 3, 4, 250, 3, 3, 3, 3, 1, 700],    # a component across a tile boundary, tiny ones right behind it
    [63, 3, 62, 3, 3, 3, 3, 3, 3, 3, 3, 3],  # one start on the last bit of a record, several starts in one record
    [1, 1, 2],                               # nothing is decomposed: an empty candidate stack
    [3],
    [4, 1],
]


@pytest.mark.parametrize("k", range(len(BOUNDARY_SIZES)))
def test_component_boundaries_on_record_and_tile_edges(hip, k):
    """First / last entries of components at multiples of 64 and 256 (records and tiles of the directories), with components
    that are not decomposed (fewer than three segments: empty ranges in the table of stack offsets) in every position."""
    g = sized_components(BOUNDARY_SIZES[k])
    want = O.decompose(g)
    hip.upload(g)
    for fl in (0, F_NO_STAGE_TIMES, F_CHECK_LAMINAR, F_ALL_VERTEX_CLASSES):
        assert hip.decompose(flags=fl).texts() == want, fl
    hip.decompose()
    assert check_hooks(hip, g) == sum(1 for n in BOUNDARY_SIZES[k] if n >= 3)


@pytest.mark.parametrize("seed", range(6))
def test_many_tiny_components_mixed_with_large_ones(hip, seed):
    """Components of one or two segments, small sites of every kind and chromosome-like components in one graph, in an order
    that puts the tiny ones in front of, between and behind the large ones."""
    parts = [sized_components([1, 2, 1, 1, 2] * (3 + seed)), W.bubble_zoo(40 + 25 * seed, 3 + seed % 3, 70 + seed, shuffle_ids=False),
             W.hprc_shaped([700 + 331 * seed, 64 * (3 + seed)], seed=seed, tiny=30 + 10 * seed), sized_components([2, 1] * 20 + [256 - seed, 3, 1]),
             W.bubble_zoo(200, 1, 90 + seed, shuffle_ids=False), W.chain_of_bubbles(85 + seed), sized_components([1] * 70)]
    if seed % 2:
        parts.reverse()
    g = concat(parts)
    want = O.decompose(g)
    hip.upload(g)
    assert hip.decompose().texts() == want
    assert hip.decompose(flags=F_NO_STAGE_TIMES).texts() == want
    assert hip.seq_redo_count() == 0
    assert hip.decompose(flags=F_SUBFLUBBLES).texts() == O.decompose(g, leaf=2)


def test_both_forms_of_has_a_previous_occurrence(hip, golden_dir):
    """With exact classes the walk reads "the class occurred before" from the flag byte and `prev` is not written; with
    POVU_HIP_F_CHECK_LAMINAR (or when the literal hi_2 rule fired) `prev` is written and checked; the all-vertex class pass
    fills the bit from `prev`.  Same forests every way, and the context reports the path taken."""
    graphs = [W.chain_of_bubbles(700), sized_components([64, 3, 190, 1, 255]), W.hprc_shaped([3000, 500, 64], seed=21, tiny=40),
              W.nested_towers(30, 9), concat([W.bubble_zoo(120, 4, 5, shuffle_ids=False), W.hprc_shaped([900], seed=2)]),
              W.random_bidirected(900, 1300, 77), W.hprc_tangled(5000, seed=3, tangle_every=900, max_tangle=400)]
    for n, g in enumerate(graphs):
        want = O.decompose(g)
        hip.upload(g)
        assert hip.decompose().texts() == want, n
        exact = hip.last_black_only_classes()  # (false iff the literal hi_2 rule fired: then the check runs by itself)
        assert hip.last_laminar_check_ran() == (not exact), n
        if n < 5:
            assert exact, n  # chains, towers, simple sites: the capping rule has nothing to deviate on
        assert hip.decompose(flags=F_CHECK_LAMINAR).texts() == want, n
        assert hip.last_laminar_check_ran() and hip.last_black_only_classes() == exact and hip.seq_redo_count() == 0, n
        assert hip.decompose(flags=F_ALL_VERTEX_CLASSES).texts() == want, n
        assert not hip.last_black_only_classes() and hip.last_laminar_check_ran() == (not exact), n
        assert hip.decompose(flags=F_ALL_VERTEX_CLASSES | F_CHECK_LAMINAR).texts() == want, n
        assert hip.last_laminar_check_ran(), n
        assert hip.decompose().texts() == want, n  # and back: no state of the checked pass leaks into a plain one
        assert hip.last_laminar_check_ran() == (not exact), n
    # a real crossing pair: the check runs whatever the flags say, and resolves it
    d = np.load(os.path.join(golden_dir, "literal_hi2_crossing_stack.npz"))
    g = W._mk(d["vid"], d["v1"], d["s1"], d["v2"], d["s2"])
    want = O.decompose(g)
    hip.upload(g)
    for fl in (0, F_CHECK_LAMINAR, F_ALL_VERTEX_CLASSES):
        assert hip.decompose(flags=fl).texts() == want
        assert hip.last_laminar_check_ran() and not hip.last_black_only_classes() and hip.last_crossings() == (1, 1)


@pytest.mark.parametrize("seed", range(4))
def test_debug_hooks_and_sub_pass_behind_a_plain_pass(hip, seed):
    """The debug hooks read the tree's parents and the components of the stack entries AFTER an ordinary pass, and a -s pass
    on the same context needs the parents again: neither may see what a plain pass no longer keeps."""
    g = concat([sized_components([2, 64, 1, 3, 125]), W.random_bidirected(150 + 40 * seed, 240 + 60 * seed, 400 + seed, connected=True),
                W.hprc_shaped([300 + 64 * seed], seed=seed, tiny=6), W.random_bidirected(90, 120, 500 + seed)])
    want, want_sub = O.decompose(g), O.decompose(g, leaf=2)
    hip.upload(g)
    assert hip.decompose(flags=F_NO_STAGE_TIMES).texts() == want
    assert check_hooks(hip, g) >= 4
    assert hip.decompose(flags=F_SUBFLUBBLES).texts() == want_sub
    assert hip.decompose().texts() == want
    assert hip.decompose(flags=F_SUBFLUBBLES | F_NO_STAGE_TIMES).texts() == want_sub
    assert hip.decompose(flags=F_CHECK_LAMINAR).texts() == want
    assert check_hooks(hip, g) >= 4


def test_small_pass_behind_a_large_one_on_the_same_context(hip):
    """Stale workspace: records of the directories and flag bytes beyond the new stack's end are those of the larger pass
    before; none of them may reach a rank."""
    big = W.hprc_shaped([60000, 9000, 700], seed=8, tiny=100)
    want_big = O.decompose(big)
    smalls = [sized_components([70, 3, 130]), sized_components([1, 2, 1]), W.chain_of_bubbles(21), sized_components([64]),
              W.bubble_zoo(9, 2, 3), sized_components([3, 1, 60])]
    for n, g in enumerate(smalls):
        hip.upload(big)
        assert hip.decompose(flags=F_CHECK_LAMINAR if n % 2 else 0).texts() == want_big
        hip.upload(g)
        want = O.decompose(g)
        assert hip.decompose().texts() == want, n
        assert hip.decompose(flags=F_CHECK_LAMINAR).texts() == want, n
        assert hip.decompose(flags=F_ALL_VERTEX_CLASSES).texts() == want, n
        assert hip.decompose(flags=F_SUBFLUBBLES).texts() == O.decompose(g, leaf=2), n
        hip.decompose()
        check_hooks(hip, g)
