"""The walks and the traversals on the MI355X at their tier hand-overs (tests/query_tier_cases.py): every case array for array
against walks_ref / traversals_ref through the checks of test_gpu_walks.py and test_gpu_traversals.py, n_tier2 against the
restatement of the tiering (tests/query_tier_model.py), the forced tier against the unforced run, tier-2 lanes that serve many
queries each (max_steps of 2^20, 2^22 and 2^24: 16, 4 and 1 lanes), more scan tasks than tier 2 has waves, and calls on a
context whose scratch an earlier call with other caps has used."""
import numpy as np
import pytest

import query_tier_cases as K
import query_tier_model as M
import test_gpu_traversals as TT
import test_gpu_walks as TW
import traversals_ref as TR
import walks_ref as WR
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W

pytestmark = pytest.mark.gpu

WALK_KEYS = ("walk_off", "step_off", "step_id", "step_or", "status")


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


# ---- walks

@pytest.mark.parametrize("name", sorted(K.walk_cases()))
def test_walk_case_both_tiers_and_the_predicted_hand_over(hip, name):
    g, caps, q = K.walk_cases()[name]
    f, w, qs = TW._check(hip, g, **caps)
    assert q in qs
    assert w.n_tier2 == M.walks_n_tier2(WR.successors(g), qs, **K.caps_of(caps))
    f2, w2, _ = TW._check(hip, g, force2=True, **caps)  # (n_tier2 == queries: asserted there)
    _same(w, w2, WALK_KEYS)


def test_union_hand_overs(hip):
    u = K.union()
    f, w, qs = TW._check(hip, u)
    assert len(qs) == 248 and w.n_tier2 == M.walks_n_tier2(WR.successors(u), qs, **WR.DEFAULTS) == 6


@pytest.mark.parametrize("max_steps", K.REUSE_MAX_STEPS)
def test_tier2_lanes_serve_many_queries(hip, max_steps):
    """fewer lanes than queries: every lane takes query after query, on the stack and the path set the one before left -- also
    after a search that MORE or BUDGET stopped with frames still on the path"""
    u = K.union()
    for caps in K.REUSE_CAPS:
        f, w, qs = TW._check(hip, u, force2=True, max_steps=max_steps, **caps)
        assert 1 <= M.t2_lanes(len(qs), max_steps) < w.n_tier2 == len(qs)
        if caps:  # (searches that stopped early: test_query_tier_inputs.py counts those that leave frames behind)
            assert int(np.count_nonzero(w.status & (WR.MORE | WR.BUDGET))) >= 100


def test_max_steps_above_the_cap_is_refused(hip):
    g, _, _ = K.walk_cases()["arm14"]
    hip.upload(g)
    f = hip.decompose()
    with pytest.raises(RuntimeError, match=r"max_steps above 2\^24"):
        hip.walks(f, max_steps=M.MAX_STEPS_CAP + 1)
    assert hip.walks(f, max_steps=M.MAX_STEPS_CAP).n_queries == 1


def _walks_on(d, g, force2=False, **caps):
    d.upload(g)
    return d.walks(d.decompose(), flags=H.W_FORCE_TIER2 if force2 else 0, **K.caps_of(caps))


def test_walks_on_scratch_an_earlier_call_used(hip):
    u = K.union()
    calls = (dict(max_steps=1000), dict(max_steps=8), dict(max_steps=1000), dict(max_steps=8, force2=True))
    got = [_walks_on(hip, u, **c) for c in calls]
    for c, w in zip(calls, got):
        fresh = HipDecomposer(0)
        try:
            w2 = _walks_on(fresh, u, **c)
            _same(w, w2, WALK_KEYS)
            assert w.n_tier2 == w2.n_tier2
        finally:
            fresh.close()
    assert got[0].n_tier2 == 6 and got[3].n_tier2 == got[3].n_queries


# ---- traversals

@pytest.mark.parametrize("max_steps", K.TRAV_MAX_STEPS)
def test_traversal_cases_both_tiers_and_the_predicted_hand_over(hip, max_steps):
    g, paths, cases = K.trav_inputs()
    f, t, qs = TT._check(hip, g, paths, max_steps=max_steps)
    tasks = M.trav_tasks(paths, qs, max_steps)
    assert t.n_tier2 == sum(x[4] for x in tasks)
    f2, t2, _ = TT._check(hip, g, paths, max_steps=max_steps, force2=True)
    assert t2.n_tier2 == len(tasks)
    _same(t, t2, TT.KEYS)
    if max_steps == TR.DEFAULT_MAX_STEPS:
        q = qs.index(K._unit(cases["dedup130"][0]))
        assert int(t.allele_off[q + 1] - t.allele_off[q]) == 2 and int(t.trav_off[q + 1] - t.trav_off[q]) == 3


def test_more_tasks_than_tier2_has_waves(hip):
    k, n = K.TASKS_CHAIN
    f, t, qs = TT._check(hip, W.chain_of_bubbles(k), W.chain_haplotypes(k, n, 4), force2=True)
    assert t.n_tier2 == k * n > 4 * 4096 and t.n_traversals == k * n


def _traversals_on(d, g, paths, max_steps):
    d.upload(g)
    f = d.decompose()
    d.upload_paths(paths)
    return d.traversals(f, max_steps=max_steps)


def test_traversals_on_scratch_an_earlier_call_used(hip):
    g, paths, _ = K.trav_inputs()
    calls = (65536, 65, 65536)
    got = [_traversals_on(hip, g, paths, ms) for ms in calls]
    for ms, t in zip(calls, got):
        fresh = HipDecomposer(0)
        try:
            t2 = _traversals_on(fresh, g, paths, ms)
            _same(t, t2, TT.KEYS)
            assert t.n_tier2 == t2.n_tier2
        finally:
            fresh.close()
    _same(got[0], got[2], TT.KEYS)
