"""The splice of `-s` on children vectors wider than a wave.  One wave works on a flubble, 64 children a round: the stable
filter's write cursor carried from round to round, a vector copied in more than one stride when it grows, find_midi's two
trunk children found in different ballots, a wave's second and third flubble -- none of it is reached by a graph with at
most 3 children under a flubble that has a concealed vertex, which is all the other `-s` tests build.  The cases of
tests/splice_width_cases.py reach each of them with figures pinned on the CPU (tests/test_splice_width_inputs.py); here the
device's text is compared with the oracle's, component by component, under the default schedule and both serial ones, alone
and next to the pinned seeds, and after every pass no component has taken more of the vector pool than the layout gave it
(povu_hip_debug_splice_pool)."""
import pytest

import oracle_lib as O
import splice_width_cases as S
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_SUBFLUBBLES
from test_oracle_subflubbles import PINNED_SEEDS, disjoint_union, rule_graph, rule_tips, seed_graph

pytestmark = pytest.mark.gpu
ENV = "POVU_HIP_SUB_SERIAL_SPLICE"
SCHEDULES = ("default", "forward", "reverse")
POOL = {"ratio": 0.0, "where": None, "passes": 0}  # the fullest stretch of the pool any pass of this file left


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()
    print(f"\nsplice pool: highest used / room = {POOL['ratio']:.4f} ({POOL['where']}) over {POOL['passes']} passes")


_inputs = {}


def inputs(name, with_pinned=False):
    """(graph, tips, the oracle's texts) of a case, alone or next to every PINNED_SEEDS graph: worked out once"""
    key = (name, with_pinned)
    if key not in _inputs:
        g, tips = S.case_graph(name) if name in S.CASES else NAMED[name]()
        if with_pinned:
            assert tips is None, name  # (no case of the table has explicit tips: the union would need them for every part)
            g = disjoint_union([g] + [seed_graph(p) for p in PINNED_SEEDS])
        _inputs[key] = (g, tips, O.decompose(g, tips=tips, leaf=2))
    return _inputs[key]


def _zi_trunk():
    g = rule_graph("zi_trunk")
    return g, rule_tips("zi_trunk", g)


NAMED = {"stride": lambda: (S.stride_graph(), None), "zi_trunk": _zi_trunk, "chain_50": lambda: (W.chain_of_bubbles(50), None)}


def set_schedule(monkeypatch, sched):
    if sched == "default":
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, sched)


def check(d, name, with_pinned=False):
    """one `-s` pass (a sizing error of the pool would throw here): texts against the oracle's, then the pool"""
    g, tips, want = inputs(name, with_pinned)
    d.upload(g, tips)
    f = d.decompose(flags=F_SUBFLUBBLES)
    got = f.texts()
    assert got.keys() == want.keys()
    for c in want:
        assert got[c] == want[c], f"{name}, component {c}:\n--- HIP\n{got[c]}\n--- oracle\n{want[c]}"
    POOL["passes"] += 1
    for c in range(f.total_components):
        used, room = d.debug_splice_pool(c)
        assert used <= room, (name, c, used, room)
        if room and used / room > POOL["ratio"]:
            POOL["ratio"], POOL["where"] = used / room, f"{name}{' + pinned seeds' if with_pinned else ''}, component {c + 1}: {used} of {room}"
    return got


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_case_alone(hip, monkeypatch, name, sched):
    set_schedule(monkeypatch, sched)
    check(hip, name)


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_case_next_to_the_pinned_seeds(hip, monkeypatch, name, sched):
    set_schedule(monkeypatch, sched)
    check(hip, name, with_pinned=True)


def test_more_listed_flubbles_than_waves(hip, monkeypatch):
    """k_sub_splice_cn's list is longer than 2 * 8192 entries and k_sub_smothered sees more than 8192 concealed vertices:
    a wave takes a second and a third flubble, wide ones among the first, the middle and the last entries"""
    set_schedule(monkeypatch, "default")
    check(hip, "stride")


def test_wide_then_small_on_one_context(monkeypatch):
    """The stale workspace: a wide case, a small one, the wide one again, then a graph without records, all on one context;
    each pass gives the oracle's text (check) and the bytes of the same pass on a fresh context."""
    set_schedule(monkeypatch, "default")
    steps = ("several_wide", "zi_trunk", "several_wide", "chain_50")
    d = HipDecomposer(0)
    try:
        reused = [check(d, n) for n in steps]
    finally:
        d.close()
    for n, got in zip(steps, reused):
        fresh = HipDecomposer(0)
        try:
            assert check(fresh, n) == got, n
        finally:
            fresh.close()
    assert reused[0] == reused[2]


def test_pool_figures_only_after_a_pass_with_s(hip, monkeypatch):
    set_schedule(monkeypatch, "default")
    g, tips, _ = inputs("several_wide")
    hip.upload(g, tips)
    hip.decompose(flags=F_SUBFLUBBLES)
    used, room = hip.debug_splice_pool(0)
    assert 0 < used <= room
    with pytest.raises(RuntimeError, match="no component 1"):
        hip.debug_splice_pool(1)  # (one component)
    hip.decompose()
    with pytest.raises(RuntimeError, match="no inserting passes"):
        hip.debug_splice_pool(0)
