"""The level-0 records of the tree stage's list rankings in their two-plane form (list_rank.hip / list_rank.hpp: rec_store /
rec_decode): a narrow word where the owner's delta to the element's bucket and the partial sums fit their fields, an
escaped pair of words where they do not, final ranks over both planes where the events' 16-bit partials overflow.

Every hand-made list of rank_records_cases.py goes through povu_hip_debug_list_rank (ranks against numpy suffix sums,
resolved the way the readers resolve them) and povu_hip_debug_rank_escapes (exactly the elements the numpy walk names
carry the escape bit); test_rank_records_inputs.py shows on the CPU that each list reaches the condition it is named
for.  Whole passes against the oracle close the file: ids that run along the lists leave nearly all records narrow, ids
in random order inside two large components leave most of them escaped.

Head-led segments are not special: lane m + h escapes where m + h - (x >> b) leaves the field, which is most of them
once there are more than 2^15 lanes, and none on a small graph."""
import numpy as np
import pytest

import oracle_lib as O
import rank_records_cases as RC
from povu_amd import HipDecomposer, workloads as W
from test_gpu_list_rank import suffix_sums, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def run_case(hip, case):
    """Ranks of every list element against the suffix sums; returns the hook's report with the per-element flags."""
    nxt, heads, start = case.lists()
    wa, wb = weights(case.n, case.events, case.wbit)
    got = hip.debug_list_rank(nxt, case.wbit, heads, events=case.events, bits=case.bits)
    order = case.order
    if case.events:
        assert np.array_equal(got[0][order], suffix_sums(order, start, wa)[order])
        assert np.array_equal(got[1][order], suffix_sums(order, start, wb)[order])
    else:
        assert np.array_equal(got[order], suffix_sums(order, start, wa)[order])
    rep = hip.debug_rank_escapes("list_rank", flags=True)
    assert rep["bucket_bits"] == case.bits and rep["delta_bits"] == RC.DELTA_BITS
    assert rep["partial_bits"] == ((RC.EVT_PBITS, RC.EVT_PBITS) if case.events else (RC.TOUR_PBITS, 0))
    return rep


def check_escapes(case, rep):
    owner, pa, pd, esc = case.model()
    reached = owner >= 0
    assert not rep["final_ranks"]
    assert rep["live"] == reached.sum()
    assert np.array_equal(rep["esc"][reached] != 0, esc[reached])  # exactly the elements that must escape
    assert rep["escaped"] == esc.sum()
    # the histogram is of the walk, not of the fields: every reached element once, under the width of its delta
    assert rep["hist"].sum() == reached.sum()
    d = case.delta()[reached]
    zz = np.where(d < 0, -2 * d - 1, 2 * d)
    assert np.array_equal(rep["hist"].sum(axis=1), np.bincount([int(v).bit_length() for v in zz], minlength=33))


@pytest.mark.parametrize("case", RC.EDGE_CASES, ids=lambda c: c.name)
def test_field_edges_and_mixed_waves(hip, case):
    check_escapes(case, run_case(hip, case))


@pytest.mark.parametrize("case", RC.HEAD_CASES, ids=lambda c: c.name)
def test_heads(hip, case):
    check_escapes(case, run_case(hip, case))


def test_events_three_modes_together(hip):
    """Narrow segments, escaped ones and one that outgrows REC_MAX: the fallback writes final ranks over both planes, and
    every element resolves (run_case); the hook reports the overflow and counts every record as escaped."""
    case = RC.three_modes()
    rep = run_case(hip, case)
    assert rep["final_ranks"]
    assert rep["live"] == rep["escaped"] == (case.model()[0] >= 0).sum()
    assert rep["esc"][case.order].all()


@pytest.mark.parametrize("shuffle", [False, True])
def test_whole_pass_against_oracle(hip, monkeypatch, shuffle):
    """bubble_zoo, PVST text against the oracle as in test_gpu_parity.py, the records counted behind both rankings.  In id
    order (a few hundred segments) all but a handful of records are narrow.  Ids in random order must be many to leave the
    field -- the re-index keeps a component's segments together, so it takes two components of ~260 000 segments each: then
    an owner is anywhere among > 10^5 lanes and most deltas need more than 16 bits."""
    monkeypatch.setenv("POVU_HIP_RANK_STATS", "1")
    g = W.bubble_zoo(2, 220000, 7, shuffle_ids=True) if shuffle else W.bubble_zoo(40, 8, 7, shuffle_ids=False)
    hip.upload(g)
    assert hip.decompose().texts() == O.decompose(g)
    for which in ("tour", "events"):
        rep = hip.debug_rank_escapes(which)
        assert not rep["final_ranks"] and rep["live"] > g.n_vtx
        share = rep["escaped"] / rep["live"]
        print(f"shuffle={shuffle} {which}: live {rep['live']} escaped {rep['escaped']} ({share:.3f})")
        assert share > 0.5 if shuffle else share < 0.1


def test_pass_without_the_variable_collects_nothing(hip, monkeypatch):
    monkeypatch.delenv("POVU_HIP_RANK_STATS", raising=False)
    hip.upload(W.bubble_zoo(4, 8, 3))
    hip.decompose()
    with pytest.raises(RuntimeError):
        hip.debug_rank_escapes("tour")
