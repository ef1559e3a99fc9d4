"""The parallel splice of `-s` (k_sub_splice_cn .. k_sub_smothered, DESIGN.md §4 "splice") gives every flubble its own wave and
lets the waves run in any order.  The default schedule runs a parent's wave and its child's together on whatever the last
pass left in the workspace, so the suite's other `-s` tests pass whatever a turn reads of another's.  Here the order is
forced: POVU_HIP_SUB_SERIAL_SPLICE=forward|reverse fills X-space with a stale forest (every spare slot a flubble whose bounds
make the nestings take it) and runs each splice kernel on ONE wave, in list order or children before parents.  A turn that
reads a word another turn writes in the same launch -- the concealed vertex a parent's z-side trunk record pushes into a
child's vector -- then sees the stale flubble, and the PVST comes out wrong.  The oracle counts those flubbles
(nest_over_pinned) so every set below is known to contain them."""
import collections
import glob
import os

import numpy as np
import pytest

import oracle_lib as O
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_ASYNC, F_HAIRPINS, F_LEAF_SUBFLUBBLES, F_NO_STAGE_TIMES, F_SUBFLUBBLES
from test_oracle import _load_gfa_links
from test_oracle_subflubbles import (HAND_TRACED, PINNED_SEEDS, RULE_SEEDS, disjoint_union, hand_traced_graph, rule_graph,
                                     rule_tips, seed_graph, sub_stats)

pytestmark = pytest.mark.gpu
SCHEDULES = ("forward", "reverse")
ENV = "POVU_HIP_SUB_SERIAL_SPLICE"


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def pinned(copies):
    """every PINNED_SEEDS graph `copies` times side by side: copies * 11 flubbles that nest over a pinned vertex"""
    return disjoint_union([seed_graph(p) for p in PINNED_SEEDS] * copies)


def check(hip, g, tips=None, flags=F_SUBFLUBBLES, texts=None):
    """the device's texts against the oracle's, component by component; returns the line kinds and how often the oracle
    ran a nesting over a pinned concealed vertex (texts: a list that takes the device's texts)"""
    sub_stats()
    want = O.decompose(g, tips=tips, leaf=2 if flags & F_SUBFLUBBLES else bool(flags & F_LEAF_SUBFLUBBLES))
    seen = collections.Counter(pinned=sub_stats()["nest_over_pinned"])
    hip.upload(g, tips)
    f = hip.decompose(flags=flags)
    if flags & F_ASYNC:
        f.wait()
    got = f.texts()
    if texts is not None:
        texts.append(got)
    assert got.keys() == want.keys()
    for c in want:
        assert got[c] == want[c], f"component {c}:\n--- HIP\n{got[c]}\n--- oracle\n{want[c]}"
        seen.update(l[0] for l in want[c].splitlines())
    return seen


@pytest.mark.parametrize("sched", SCHEDULES)
def test_rule_seeds_hand_traced_and_golden_graphs(hip, monkeypatch, golden_dir, sched):
    monkeypatch.setenv(ENV, sched)
    seen = collections.Counter()
    for rule in sorted(RULE_SEEDS):
        g = rule_graph(rule)
        seen += check(hip, g, rule_tips(rule, g))
    for name in sorted(HAND_TRACED):
        seen += check(hip, hand_traced_graph(name))
    for path in sorted(glob.glob(os.path.join(golden_dir, "gfa", "**", "*.gfa"), recursive=True)):
        seen += check(hip, _load_gfa_links(path))
    assert seen["pinned"] >= 1 and seen["C"] >= 40 and seen["M"] >= 3 and seen["S"] >= 8, seen


@pytest.mark.parametrize("sched", SCHEDULES)
def test_small_random_graphs(hip, monkeypatch, sched):
    """240 random graphs, each next to one PINNED_SEEDS graph (one of them in its own component)"""
    monkeypatch.setenv(ENV, sched)
    rng = np.random.default_rng(4242)
    seen = collections.Counter()
    for it in range(240):
        nv = int(rng.integers(5, 30))
        g = W.random_bidirected(nv, int(rng.integers(nv, 3 * nv)), int(rng.integers(1 << 30)), self_loops=bool(it % 2))
        seen += check(hip, disjoint_union([g, seed_graph(PINNED_SEEDS[it % len(PINNED_SEEDS)])]))
    assert seen["pinned"] >= 240 and seen["C"] >= 400 and seen["M"] >= 50 and seen["S"] >= 20, seen


@pytest.mark.parametrize("sched", SCHEDULES)
def test_bubble_zoo_and_hprc_shapes(hip, monkeypatch, sched):
    monkeypatch.setenv(ENV, sched)
    seen = collections.Counter()
    for seed in range(2):
        seen += check(hip, disjoint_union([W.bubble_zoo(20, 8, seed), pinned(2)]))
        seen += check(hip, disjoint_union([W.hprc_shaped([3000, 1500], seed=seed), pinned(2)]))
    assert seen["pinned"] >= 4 * 2 * len(PINNED_SEEDS) and seen["C"] >= 100 and seen["M"] >= 10 and seen["S"] >= 4, seen


@pytest.mark.parametrize("sched", SCHEDULES)
def test_thousands_of_flubbles_that_nest_over_a_pinned_vertex(hip, monkeypatch, sched):
    monkeypatch.setenv(ENV, sched)
    seen = check(hip, pinned(200))
    assert seen["pinned"] == 200 * len(PINNED_SEEDS) and seen["C"] >= 3000 and seen["M"] >= 300 and seen["S"] >= 100, seen


def test_default_and_serial_schedules_give_the_same_bytes(hip, monkeypatch):
    for g in (pinned(100), disjoint_union([W.hprc_shaped([3000, 1500], seed=3), W.bubble_zoo(20, 8, 3), pinned(5)])):
        hip.upload(g)
        monkeypatch.delenv(ENV, raising=False)
        want = hip.decompose(flags=F_SUBFLUBBLES).texts()
        for sched in SCHEDULES:
            monkeypatch.setenv(ENV, sched)
            assert hip.decompose(flags=F_SUBFLUBBLES).texts() == want, sched
        monkeypatch.delenv(ENV)
        assert hip.decompose(flags=F_SUBFLUBBLES).texts() == want


def test_unknown_schedule_is_refused(hip, monkeypatch):
    hip.upload(seed_graph(PINNED_SEEDS[0]))
    monkeypatch.setenv(ENV, "sideways")
    with pytest.raises(RuntimeError, match=ENV):
        hip.decompose(flags=F_SUBFLUBBLES)


def test_a_context_reused_on_a_different_graph(monkeypatch):
    """The stale-workspace case, default schedule: `-s` on graph A, then on graph B in the same context.  A holds B's
    components, each behind a chain of bubbles of its own, so the workspace B reuses is full of A's flubbles where B's
    concealed vertices go.  B matches the oracle and B on a fresh context."""
    monkeypatch.delenv(ENV, raising=False)
    b = pinned(100)
    a = disjoint_union([x for p in PINNED_SEEDS for x in (W.chain_of_bubbles(6), seed_graph(p))] * 100)
    fresh = HipDecomposer(0)
    try:
        fresh.upload(b)
        want_fresh = fresh.decompose(flags=F_SUBFLUBBLES).texts()
    finally:
        fresh.close()
    d = HipDecomposer(0)
    try:
        check(d, a)
        assert check(d, b)["pinned"] == 100 * len(PINNED_SEEDS)
        assert d.decompose(flags=F_SUBFLUBBLES).texts() == want_fresh
        check(d, a)
        check(d, b)
    finally:
        d.close()


def test_phase_arenas_grow_shrink_and_stay_empty(monkeypatch):
    """The tables of `-s` lie in one arena per phase, carved when the phase's sizes are known and kept from pass to pass.  One
    fresh context, default schedule, through passes whose phases are empty (no concealed vertex: every later phase has
    nothing), tiny (one record, no smothered one), and full, so that each arena is carved empty, reused while too small and
    reused while full of a larger forest."""
    monkeypatch.delenv(ENV, raising=False)
    zi = rule_graph("zi_trunk")
    steps = [(W.chain_of_bubbles(50), None), (pinned(20), None), (zi, rule_tips("zi_trunk", zi)), (W.nested_towers(6, 3), None),
             (pinned(20), None), (W.chain_of_bubbles(6), None)]
    d = HipDecomposer(0)
    try:
        seen, texts = [], []
        for g, tips in steps:
            seen.append(check(d, g, tips, texts=texts))
    finally:
        d.close()
    for i in (0, 3, 5):
        assert seen[i]["C"] == 0 and seen[i]["M"] == 0 and seen[i]["S"] == 0, (i, seen[i])
    assert seen[2]["C"] == 1 and seen[2]["S"] == 0, seen[2]
    for i in (1, 4):
        assert seen[i]["C"] >= 400 and seen[i]["M"] >= 50 and seen[i]["S"] >= 20, (i, seen[i])
    assert texts[1] == texts[4]


def test_one_context_through_every_mode(monkeypatch):
    """One fresh context: -s -> plain (async) -> -s -> leaf passes -> hairpins -> -s with the async flag (which -s does not
    take) -> plain, on graphs that shrink and grow, two of them with a class large enough for the wave walk.  The arenas that keep their contents from one pass to the next
    (the -s workspace, the leaf passes', the wave walk's, the resident graph's with head room) must not leak into the next."""
    monkeypatch.delenv(ENV, raising=False)
    tangled = W.hprc_tangled(3000, seed=7, tangle_every=700, max_tangle=2500)
    steps = [(pinned(20), F_SUBFLUBBLES), (tangled, F_ASYNC | F_NO_STAGE_TIMES), (rule_graph("nest_over_pinned"), F_SUBFLUBBLES),
             (W.hprc_shaped([3000, 1500], seed=2), F_LEAF_SUBFLUBBLES), (W.bubble_zoo(20, 8, 3), F_HAIRPINS),
             (disjoint_union([tangled, pinned(5)]), F_SUBFLUBBLES | F_ASYNC), (W.chain_of_bubbles(50), 0)]
    d = HipDecomposer(0)
    try:
        for i, (g, flags) in enumerate(steps):
            seen = check(d, g, flags=flags)
            if flags & F_SUBFLUBBLES:
                assert seen["pinned"] >= 1 and seen["C"] >= 1, (i, seen)
    finally:
        d.close()
