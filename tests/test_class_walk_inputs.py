"""The inputs of tests/test_gpu_class_walks.py reach what they are there for (tests/class_walk_cases.py), shown on the
restatement of the two class walks with telemetry (tests/class_walk_model.py): its tree equals the oracle's on every case, and
every hand-made threshold of the walks is reached on both sides by a case that names it.  Plain Python, no GPU."""
import os
import re

import numpy as np
import pytest

import class_walk_cases as K
import class_walk_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "povu_amd", "csrc", "hip")


def test_constants_mirror_the_sources():
    tree = open(os.path.join(HIP, "tree_kernels.hip")).read()
    step = open(os.path.join(HIP, "walk_step.inc")).read()
    hooks = open(os.path.join(HIP, "pass_hooks.hpp")).read()  # (the budget and its floor: with the hooks of a pass)

    def const(name, text=tree):
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))
    assert const("CLASS_BUDGET", hooks) == M.CLASS_BUDGET and "std::max(16, atoi(ev))" in hooks and M.BUDGET_FLOOR == 16
    assert "uint32_t class_budget = CLASS_BUDGET;" in hooks and "budget = P.hooks.class_budget;" in tree
    assert "if (sides > budget)" in tree  # (tested after each advance; a follow-through pair counts two)
    assert const("DFS_STK") == M.DFS_STK and "k = up.y + 1;" in tree
    assert const("W_INLINE") == M.W_INLINE and "if (e0.x > W_INLINE)" in step
    assert const("W_CHUNK0") == M.W_CHUNK0 and const("W_WIN") == M.W_WIN and const("W_WIN_BACK") == M.W_WIN_BACK
    assert const("W_PROBE") == M.W_PROBE and const("W_TRIAL") == M.W_TRIAL
    assert "(y - x + 64u) <= 128u" in tree and "tot == W_PROBE && 4 * near >= 3 * tot" in tree
    # the ring of 64, the eviction of 32, the growth rule, the looks of 64 lanes, the push rule of the form without window
    assert "if (d - lds_lo == 64)" in tree and "lds_lo = ev + 32;" in tree
    assert "if (ev + 32 > (n_chunks ? (W_CHUNK0 << (n_chunks - 1)) : 0u))" in tree
    assert "const bool beyond = j0 + 64 < r.n;" in step and "j0 += 64;" in step
    assert "if ((m & (m - 1)) || beyond || (fast && (miss >> f)))" in step
    assert "depth - lds_lo < 62u" in step and "min(win_penalty ? 2 * win_penalty : 8u, 1024u)" in step
    assert [M.chunk_of(d) for d in (0, 63, 64, 127, 128, 255, 256, 511, 512)] == [0, 0, 1, 1, 2, 2, 3, 3, 4]
    assert [M.chunk_size(c) for c in range(5)] == [64, 64, 128, 256, 512]


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_model_tree_equals_the_oracle(name):
    """Both simulated walks leave the parents of the lexicographic DFS (asserted inside the model), and the tree built from
    them is the oracle's, component by component."""
    g, comps, classes = K.modelled(name)
    checked = 0
    first = 0
    for rank, d, tree in comps:
        # the device numbers the sides as the model does: components in rank order, their vertices in index order
        assert d["gidx"].tolist() == list(range(first, first + len(d["gidx"])))
        first += len(d["gidx"])
        if tree is None:
            continue
        assert tree["gid"] == d["gid"].tolist() and tree["par"] == d["par"].tolist()
        assert tree["typ"] == d["typ"].tolist() and tree["black"] == d["pe_black"].tolist()
        checked += 1
    assert checked and first == g.n_vtx and g.n_vtx <= 4000
    assert classes and all(c["wave"]["steps"] == c["steps"] == c["sides"] - 1 for c in classes)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case_reaches_what_it_names(name):
    g, comps, classes = K.modelled(name)
    tags = K.reached(classes, 2 * g.n_vtx)
    missing = [t for t in K.CASE_TAGS[name] if t not in tags]
    assert not missing, missing


def test_every_threshold_is_reached_on_both_sides():
    """Over all cases together: every tag of every row of THRESHOLDS is named by a case (and test_case_reaches_what_it_names
    shows that the case reaches it).  A cap, not a measurement: no threshold is left to a graph whose telemetry does not show it."""
    named = {t for tags in K.CASE_TAGS.values() for t in tags}
    for row, tags in K.THRESHOLDS.items():
        assert not [t for t in tags if t not in named], row
    assert set(K.CASE_TAGS) == set(K.CASES)
    reached = set()
    for name in K.CASES:
        g, comps, classes = K.modelled(name)
        reached |= K.reached(classes, 2 * g.n_vtx)
    for row, tags in K.THRESHOLDS.items():
        assert not [t for t in tags if t not in reached], row


def test_star_lists():
    """a source, m arms and a sink: one class of 2 m + 2 sides with two lists of m candidates, all others of 2"""
    g, comps, classes = K.modelled("lists")
    assert sorted(c["sides"] for c in classes) == sorted(2 * m + 2 for m in K.LIST_M)
    for c in classes:
        m = (c["sides"] - 2) // 2
        lens = sorted(c["lists"].values())
        assert lens == [2] * (2 * m) + [m, m]
        # the one-lane walk keeps 257 sides: m = 127 is the longest list it scans
        assert c["over"][M.CLASS_BUDGET] == (m > 127)


def test_budget_rule():
    """sides reached except the entry, tested after each advance: 257 sides stay, 258 go; 17 and 18 under the floor of 16"""
    g, comps, classes = K.modelled("budget")
    by = {c["sides"]: c for c in classes}
    assert [by[s]["over"][256] for s in (256, 257, 258, 259)] == [False, False, True, True]
    assert [by[s]["over"][16] for s in (16, 17, 18, 19)] == [False, False, True, True]
    assert M.n_over(classes, 256) == 3 and M.n_over(classes, 16) == 8  # (256 .. 259, 263; those, 18, 19 and 21)
    # an abandoned lane had branched, returned and written parents before it gave up
    assert by[263]["abandoned_at"][256] == (258, 6) and by[21]["abandoned_at"][16] == (18, 2)
    small = [c["sides"] for c in classes if c["sides"] <= 10]
    assert len(small) >= 20 and set(small) == {4, 6, 8, 10}


def test_stack_case_pool_shares():
    """the share of the pool a class takes = the sum of its chunk sizes.  A stack that only grows takes a chunk when its 65th,
    129th, 193rd and 321st entry is pushed (the eviction of 32 that would pass the chunks' capacity); after a fetch the ring's
    low end is no multiple of 32 any more and a chunk may come a little earlier, always below 64 + 2 x entries."""
    g, comps, classes = K.modelled("stack")
    for c in classes:
        e = c["wave"]["max_entries"]
        if not c["wave"]["resumes"]:
            want = 0 if e <= 64 else 64 if e <= 128 else 128 if e <= 192 else 256 if e <= 320 else 512
            assert c["wave"]["pool"] == want, (e, c["wave"]["pool"])
        assert c["wave"]["pool"] == 0 if e <= 64 else c["wave"]["pool"] < 64 + 2 * e
    assert max(c["wave"]["max_entries"] for c in classes) == 323
    assert M.pool_sum(classes) == sum(c["wave"]["pool"] for c in classes) <= 3 * 2 * g.n_vtx


def test_numbering_cases_differ_only_in_numbering():
    """the window cases are rings: one path, list lengths 2, so only the numbering tells them from a plain closed arc"""
    for name in ("window", "window_flipped", "near_then_scattered", "scattered_then_near", "scattered_long"):
        g, comps, classes = K.modelled(name)
        assert len(classes) == 1 and classes[0]["max_list"] == 2 and not classes[0]["wave"]["resumes"]
    for name, hot in (("near_then_scattered", True), ("scattered_then_near", False), ("scattered_long", False), ("hot_ladder", True)):
        assert all(c["probe_hot"] == hot for c in K.modelled(name)[2] if c["sides"] > 100), name
    assert np.gcd(330, 127) == 1
