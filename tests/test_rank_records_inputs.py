"""The hand-made lists of rank_records_cases.py reach the conditions they are named for (no GPU: the level-0 walk
restated in numpy).  A change of a field width, of the splitter hash or of a builder that empties one of them fails
here, not silently on the GPU."""
import numpy as np
import pytest

import rank_records_cases as RC

HALF = RC.HALF


def by_name(prefix):
    return [c for c in RC.EDGE_CASES if c.name.startswith(prefix)]


@pytest.mark.parametrize("case", by_name("delta_edges"), ids=lambda c: c.name)
def test_delta_edges_reach_both_ends_of_the_field(case):
    owner, pa, pd, esc = case.model()
    d = case.delta()[case.order]
    e = esc[case.order]
    for value, escapes in ((-HALF, False), (-HALF - 1, True), (HALF - 1, False), (HALF, True)):
        at = np.flatnonzero(d == value)
        assert at.size == 1, (case.name, value)
        assert bool(e[at[0]]) == escapes
    # the head-led first element aside, nothing else escapes; the partials stay far inside their fields
    assert esc.sum() == 3 and esc[case.order[0]]
    assert max(pa.max(), pd.max()) < 120


@pytest.mark.parametrize("case", by_name("partial_edges"), ids=lambda c: c.name)
def test_partial_edges_reach_the_maximum_and_one_past_it(case):
    owner, pa, pd, esc = case.model()
    assert np.all(np.abs(case.delta()[owner >= 0]) < HALF)  # the partials alone decide
    if case.events:
        pmax = (1 << RC.EVT_PBITS) - 1
        assert sorted(pa[esc].tolist()) == [2, pmax + 1] and (pa[~esc] <= pmax - 1).all() and (pa == pmax - 1).any()
        assert sorted(pd[esc].tolist()) == [1, pmax + 1] and (pd[~esc] <= pmax).all() and (pd == pmax).any()
    else:
        pmax = (1 << RC.TOUR_PBITS) - 1
        assert (pa == pmax).sum() == 2 and pa[esc].tolist() == [pmax + 1]


@pytest.mark.parametrize("case", by_name("side_by_side"), ids=lambda c: c.name)
def test_side_by_side_alternates_lane_by_lane(case):
    owner, pa, pd, esc = case.model()
    lanes = np.arange(2, 260)
    spl = RC.bucket_splitter(lanes, case.bits)
    assert (owner[spl] == lanes).all()
    per_lane = np.array([esc[owner == q].any() for q in lanes])
    assert not per_lane[0::2].any() and per_lane[1::2].all()  # even lanes narrow, odd lanes escaped: 32 of each in a wave
    assert esc.sum() == 3 * 129 + 1


@pytest.mark.parametrize("case", RC.HEAD_CASES, ids=lambda c: c.name)
def test_head_cases(case):
    owner, pa, pd, esc = case.model()
    nxt, heads, start = case.lists()
    m = (case.n + 7) >> 3
    led = owner >= m  # elements of head-led segments
    assert led[heads[heads != RC.NIL]].all()
    if case.n > 7:
        assert esc[led].sum() > led.sum() // 2 and (~esc[led]).sum() > 100  # most head-led elements escape, the early ones fit
        assert (owner[case.order] >= 0).all() and (~esc[~led & (owner >= 0)]).sum() > 1000
    else:
        assert not esc.any()


def test_three_modes():
    case = RC.three_modes()
    owner, pa, pd, esc = case.model()
    pmax = (1 << RC.EVT_PBITS) - 1
    assert pa.max() > RC.REC_MAX  # one segment outgrows the escaped record too
    far = np.abs(case.delta()) >= HALF
    assert far.sum() > 50 and (esc & ~far & (pa <= RC.REC_MAX)).sum() > 1000  # escaped by delta, escaped by partial
    assert ((owner >= 0) & ~esc).sum() > 100  # and narrow ones
    assert pa[~esc].max() <= pmax
