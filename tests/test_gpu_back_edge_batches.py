"""GPU tests of the batched count phase of k_back_edges (tree_kernels.hip): a lane loads the words of BE_BATCH = 4 of its eight
sides together -- the sides' own words, their first four slot words, the tree vertices behind the slots that can be back edges
-- unconditionally, a lane behind the last side from the last side's words.  The shapes (back_edge_batches_cases.py) put a side
with a known number of slots and back edges last in the graph and first in a workgroup, with 2 n sides on either side of a
lane's iteration (256 sides), a batch (1 024) and a workgroup (2 048); sides with 1 ... 9 slots (the edges of a round of four:
from five slots on the side goes the plain way behind its batch) and 0 ... 8 back edges (two: the edge between the LDS path
and the second walk of the emit phase); sides without a link on every place of a tree (the remembered "the target is the root"
bit); self loops and parallel links; 70 links on a side (the pass takes dupflag, and no batch) and 254 (the word forms);
components that are not decomposed around and between decomposed ones, a run of them that fills whole batches; graphs of one
and two segments and without a link; components in and out of order, with and without self loops (the two forms of the
re-index in front of the tree stage).

Every case compares the forests with the CPU oracle's texts under three flag sets, and the trees, candidate stacks and edge ids
of the decomposed components with the oracle's dumps; then all of it again behind a larger graph, so that slack and dead
workspace hold old data.

For k_class_finish_black (par_kernels.hip, four sorted positions a lane; its code is unchanged): passes whose sorted order of
class entries ends in 4n, 4n + 1 and 4n + 3 invalid ones, behind 4m, 4m + 1 and 4m + 3 valid ones, so that the tail begins and
ends inside a lane's four and on its edge."""
import numpy as np
import pytest

import back_edge_batches_cases as B
import oracle_lib as O
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_ALL_VERTEX_CLASSES, F_NO_STAGE_TIMES
from test_oracle import dump_component

pytestmark = pytest.mark.gpu

FLAGS = [0, F_NO_STAGE_TIMES, F_ALL_VERTEX_CLASSES]
CASES = B.cases()
_WANT = {}


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def want(name):
    """The oracle's texts and dumps of a case, worked out once."""
    if name not in _WANT:
        g, tips = CASES[name], B.tips_of(name, CASES[name])
        dumps, c = [], 0
        while True:
            d = dump_component(g, c, tips=tips)
            if d is None:
                break
            dumps.append(d)
            c += 1
        _WANT[name] = (O.decompose(g, tips=tips), dumps)
    return _WANT[name]


def check_hooks(hip, dumps):
    """debug_tree / debug_stack / debug_edge_ids of every decomposed component against the oracle's dump (check_hooks of
    test_gpu_stack_lookups, with the dumps shared between the runs of a case)."""
    for c, d in enumerate(dumps):
        if not len(d["gid"]):
            continue
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


def run_case(hip, name):
    g = CASES[name]
    texts, dumps = want(name)
    hip.upload(g, tips=B.tips_of(name, g))
    for flags in FLAGS:
        assert hip.decompose(flags=flags).texts() == texts, (name, flags)
    hip.decompose()
    check_hooks(hip, dumps)


@pytest.mark.parametrize("name", list(CASES))
def test_forests_and_hooks_equal_the_oracle(hip, name):
    run_case(hip, name)


def test_the_fat_sides_take_the_word_forms(hip):
    """254 links on a side: every count of the pass is a word (k_back_edges<u32, u32>); 70: bytes."""
    hip.upload(CASES["254 links on one side"])
    hip.decompose()
    assert hip.last_narrow_forms() == (False, False, False)
    hip.upload(CASES["70 links on one side"])
    hip.decompose()
    assert hip.last_narrow_forms()[0]


def test_again_behind_a_larger_graph(hip):
    """Every case right behind a larger graph on the same context: the slack behind the arrays and the workspace a small graph
    does not write hold the larger graph's data."""
    big = W.hprc_shaped([4000, 1500], seed=3, tiny=5)
    want_big = O.decompose(big)
    for k, name in enumerate(CASES):
        if k % 8 == 0:
            hip.upload(big)
            assert hip.decompose(flags=FLAGS[(k // 8) % 3]).texts() == want_big
        run_case(hip, name)
