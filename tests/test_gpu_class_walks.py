"""The two class walks of the tree stage (k_class_dfs_small, k_class_walk_wave with and without the hot loop) on the directed
inputs of tests/class_walk_cases.py, whose thresholds tests/test_class_walk_inputs.py shows reached on the CPU model.  Every
case in every mode: PVST text, tree and tree-edge ids equal the oracle's, and the walks' three counter words
(povu_hip_debug_walk_words) equal what the model says -- which walk a class got, how many chunks the stacks took."""
import numpy as np
import pytest

import class_walk_cases as K
import class_walk_model as M
import oracle_lib as O
from povu_amd import HipDecomposer
from povu_amd.hip import F_BIG_CLASS_DFS, F_NO_STAGE_TIMES, F_SEQ_TREE

pytestmark = pytest.mark.gpu

# (name, flags, POVU_HIP_WALK_ROUTE, POVU_HIP_CLASS_BUDGET)
MODES = [
    ("default", 0, None, None),
    ("big-route0", F_BIG_CLASS_DFS, "0", None),
    ("big-route1", F_BIG_CLASS_DFS, "1", None),
    ("big-route2", F_BIG_CLASS_DFS, "2", None),
    ("budget16-route0", 0, "0", "16"),
    ("budget16-route2", 0, "2", "16"),
    ("default-no-stage-times", F_NO_STAGE_TIMES, None, None),
]


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


_want = {}


def expected(name):
    """the oracle's texts and the model's figures of a case, worked out once"""
    if name not in _want:
        g, comps, classes = K.modelled(name)
        _want[name] = dict(g=g, texts=O.decompose(g), comps=comps, classes=classes)
    return _want[name]


def set_mode(monkeypatch, route, budget):
    for var, val in (("POVU_HIP_WALK_ROUTE", route), ("POVU_HIP_CLASS_BUDGET", budget)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


def check_words(hip, w, flags, route, budget):
    """the walks' counter words against the model"""
    classes, n_sides = w["classes"], 2 * w["g"].n_vtx
    words = hip.debug_walk_words()
    assert words["n_entry"] == len(classes)
    small_ran = not flags & F_BIG_CLASS_DFS
    bud = M.CLASS_BUDGET if budget is None else max(int(budget), M.BUDGET_FLOOR)
    if small_ran:
        assert words["n_over"] == M.n_over(classes, bud)
    else:
        assert words["n_over"] == 0
    if route == "2":
        assert words["pool_top"] == M.pool_sum(classes, bud if small_ran else None)
    else:  # the pushes of the forms with a window depend on where the window lies
        assert words["pool_top"] <= 3 * n_sides
        if small_ran and M.n_over(classes, bud) == 0:
            assert words["pool_top"] == 0
    return words


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case(hip, monkeypatch, name, mode):
    _, flags, route, budget = mode
    w = expected(name)
    set_mode(monkeypatch, route, budget)
    hip.upload(w["g"])
    assert hip.decompose(flags=flags).texts() == w["texts"]
    for rank, d, tree in w["comps"]:
        if tree is None:
            continue
        t = hip.debug_tree(rank)
        assert np.array_equal(t["gid"], d["gid"]) and np.array_equal(t["par"], d["par"]), rank
        assert np.array_equal(t["typ"], d["typ"]) and np.array_equal(t["black"], d["pe_black"]), rank
        assert np.array_equal(hip.debug_edge_ids(rank), d["pe_id"]), rank
    check_words(hip, w, flags, route, budget)


def test_numbering_is_the_models(hip):
    """the window cases rest on the device numbering the sides as the model does: components in rank order, vertices in
    index order inside them"""
    for name in ("window_edges", "small_depth", "stack"):
        w = expected(name)
        hip.upload(w["g"])
        hip.decompose()
        comp, loc = hip.debug_components(w["g"].n_vtx)
        for rank, d, _ in w["comps"]:
            gl = d["gidx"]
            assert np.all(comp[gl] == rank) and np.array_equal(loc[gl], np.arange(len(gl)))


def test_walk_words_guards(hip):
    """the hook refuses a pass that walked no classes on the parallel tree stage"""
    w = expected("window_edges")
    hip.upload(w["g"])
    assert hip.decompose(flags=F_SEQ_TREE).texts() == w["texts"]
    with pytest.raises(RuntimeError):
        hip.debug_walk_words()
    fresh = HipDecomposer(0)
    try:
        with pytest.raises(RuntimeError):
            fresh.debug_walk_words()
    finally:
        fresh.close()


def test_stale_workspace(hip, monkeypatch):
    """One warm context, every case right after the largest one (the wave walk's records, stacks and parent words keep the
    bigger pass's contents behind the smaller graph's sides), then the same sequence backwards."""
    names = sorted(K.CASES, key=lambda n: expected(n)["g"].n_vtx)
    big, rest = names[-1], names[:-1]
    seq = [x for n in rest for x in (big, n)]
    for order, route in ((seq, "0"), (seq[::-1], "2")):
        set_mode(monkeypatch, route, None)
        for n in order:
            w = expected(n)
            hip.upload(w["g"])
            assert hip.decompose(flags=F_BIG_CLASS_DFS).texts() == w["texts"], (n, route)
            check_words(hip, w, F_BIG_CLASS_DFS, route, None)
