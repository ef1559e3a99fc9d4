"""GPU tests of the root bit of the tree vertex flags: the tree stage marks every tree vertex without a parent (a dummy
root, or the side a tip-less component is entered by), and the class stage's bridge kernel reads that bit, four flag bytes
to a word, instead of streaming the parent array.  debug_tree exports the flags: the bit must be set exactly where the
parent is NIL, with the parents themselves equal to the CPU oracle's."""
import numpy as np
import pytest

import oracle_lib as O
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_ALL_VERTEX_CLASSES, F_HAIRPINS, F_NO_STAGE_TIMES, F_SEQ_TREE, F_SUBFLUBBLES
from test_gpu_narrow_counts import comb, fan_in
from test_gpu_stack_lookups import concat, sized_components
from test_oracle import dump_component

pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def ring(n):
    return W.from_plus_links(np.arange(1, n + 1), np.arange(n, dtype=np.uint32), (np.arange(n, dtype=np.uint32) + 1) % n)


def mixed():
    """Components with a dummy root (tips), without one (rings, a circular backbone) and too small to be decomposed, in
    front of, between and behind each other, so that roots fall on every position of a four-byte word of flags."""
    return concat([sized_components([1, 2, 7]), ring(5), W.bubble_zoo(6, 3, 11, shuffle_ids=False), ring(3), sized_components([2, 4, 1]),
                   W.hprc_circular(300), fan_in(5), sized_components([1]), ring(9), comb(4), W.nested_towers(4, 3), sized_components([1, 1])])


def check_roots(hip, g, shard=None):
    """Parents and root bits of every component the pass processed against the oracle's dump; returns how many were checked,
    how many of those have a dummy root and how many a real one."""
    c = checked = dummy = real = 0
    while True:
        d = dump_component(g, c)
        if d is None:
            break
        t = hip.debug_tree(c)
        if shard is not None and len(t["par"]) == 0:  # (another shard's component: no tree, nothing marked)
            c += 1
            continue
        assert np.array_equal(t["par"], d["par"]), c
        assert np.array_equal(t["root"] != 0, t["par"] == NIL), c
        if len(d["par"]):
            assert np.array_equal(t["typ"], d["typ"]) and np.array_equal(t["black"], d["pe_black"]), c
            assert int((t["par"] == NIL).sum()) == 1 and t["par"][0] == NIL, c
            checked += 1
            dummy += int(d["typ"][0] == 2)
            real += int(d["typ"][0] != 2)
        c += 1
    return checked, dummy, real


@pytest.mark.parametrize("flags", [0, F_NO_STAGE_TIMES, F_ALL_VERTEX_CLASSES, F_HAIRPINS, F_SEQ_TREE])
def test_root_bit_is_set_exactly_where_the_parent_is_nil(hip, flags):
    """A plain pass (lean: the bridge kernel reads the tree stage's flags in place), one with every vertex's class, one with
    the hairpin report (the per-vertex tables are built, k_globalize marks the roots again) and one whose tree comes from the
    one-lane kernels (k_globalize is the only one that marks them): forests equal to the oracle's, the bit where the parent
    is NIL."""
    g = mixed()
    hip.upload(g)
    want = O.decompose(g)
    f = hip.decompose(flags=flags)
    assert f.texts() == want
    checked, dummy, real = check_roots(hip, g)
    assert checked >= 15 and dummy >= 5 and real >= 4


def test_root_bit_with_components_of_another_shard(hip):
    """Shard 1 of 2: the components the pass does not process have no tree (and no root bit to read); the others match."""
    g = mixed()
    hip.upload(g)
    seen = 0
    for rank in (0, 1):
        hip.decompose(rank=rank, world=2)
        checked, _, _ = check_roots(hip, g, shard=rank)
        assert checked >= 1  # (the shards are balanced by weight: one of them may hold the large component alone)
        seen += checked
    assert seen == check_roots_all(g)


def check_roots_all(g):
    c = n = 0
    while True:
        d = dump_component(g, c)
        if d is None:
            return n
        n += int(len(d["par"]) > 0)
        c += 1


def test_sub_pass_behind_a_plain_pass(hip):
    """A -s pass right behind a plain pass on the same context (the leaf and inserting passes read the flags' type and colour
    bits beside the new one) equals the oracle's, and the plain pass behind it still does."""
    g = mixed()
    hip.upload(g)
    want, want_sub = O.decompose(g), O.decompose(g, leaf=2)
    assert hip.decompose().texts() == want
    assert hip.decompose(flags=F_SUBFLUBBLES).texts() == want_sub
    assert hip.decompose().texts() == want
    check_roots(hip, g)
