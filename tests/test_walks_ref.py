"""CPU tests of the walk restatement (tests/walks_ref.py): hand cases whose answers are written out here, every cap, and
the PVST text of golden files.  The GPU walks are compared with this restatement in test_gpu_walks.py."""
import os

import numpy as np
import pytest

import walks_ref as R
from povu_amd import workloads as W
from test_oracle import _load_gfa_links


def graph(ids, links):
    """links as GFA L-line pairs: ("1+", "2+") = out of 1's r side into 2's l side, ("1+", "2-") = into 2's r side."""
    ids = sorted(ids)
    pos = {v: i for i, v in enumerate(ids)}
    v1, s1, v2, s2 = [], [], [], []
    for a, b in links:
        v1.append(pos[int(a[:-1])])
        s1.append(W.R if a[-1] == "+" else W.L)
        v2.append(pos[int(b[:-1])])
        s2.append(W.L if b[-1] == "+" else W.R)
    return W._mk(np.array(ids), np.array(v1), np.array(s1), np.array(v2), np.array(s2))


def fw(i):
    return (i, 0)


def walks(g, s, z, **caps):
    ws, st = R.walks_of(R.successors(g), s, z, **dict(R.DEFAULTS, **caps))
    return [R.as_text(w) for w in ws], st


# every hand case: (graph, start, end) -- shared with the GPU tests
SNP = (graph([1, 2, 3, 4], [("1+", "2+"), ("1+", "3+"), ("2+", "4+"), ("3+", "4+")]), fw(1), fw(4))
INDEL = (graph([1, 2, 5], [("1+", "2+"), ("1+", "5+"), ("5+", "2+")]), fw(1), fw(2))
INDEL_LOW_ID = (graph([1, 2, 3], [("1+", "2+"), ("2+", "3+"), ("1+", "3+")]), fw(1), fw(3))
NESTED = (graph(range(1, 11), [("1+", "2+"), ("2+", "3+"), ("2+", "4+"), ("3+", "5+"), ("4+", "5+"), ("5+", "6+"), ("1+", "7+"),
                               ("7+", "8+"), ("7+", "9+"), ("8+", "10+"), ("9+", "10+"), ("10+", "6+")]), fw(1), fw(6))
INVERTED = (graph([1, 2, 3], [("1+", "2-"), ("2-", "3+"), ("1+", "3+")]), fw(1), fw(3))
CYCLE = (graph([1, 2, 3, 4], [("1+", "2+"), ("2+", "3+"), ("3+", "2+"), ("2+", "4+"), ("3+", "4+")]), fw(1), fw(4))
PARALLEL = (graph([1, 2, 3], [("1+", "2+"), ("1+", "2+"), ("2+", "3+"), ("1+", "3+"), ("1+", "3+")]), fw(1), fw(3))
HAND = dict(snp=SNP, indel=INDEL, indel_low_id=INDEL_LOW_ID, nested=NESTED, inverted=INVERTED, cycle=CYCLE, parallel=PARALLEL)


def test_snp_bubble_has_two_walks():
    assert walks(*SNP) == ([">1>2>4", ">1>3>4"], 0)


def test_indel_lists_the_two_step_walk_first():
    assert walks(*INDEL) == ([">1>2", ">1>5>2"], 0)
    # the order is by segment id, not by length: an inserted segment with the lower id comes first
    assert walks(*INDEL_LOW_ID) == ([">1>2>3", ">1>3"], 0)


def test_nested_bubbles_parent_has_four_walks_in_order():
    assert walks(*NESTED) == ([">1>2>3>5>6", ">1>2>4>5>6", ">1>7>8>10>6", ">1>7>9>10>6"], 0)
    assert walks(NESTED[0], fw(2), fw(5)) == ([">2>3>5", ">2>4>5"], 0)


def test_inverted_middle_segment_gives_a_reverse_step():
    assert walks(*INVERTED) == ([">1<2>3", ">1>3"], 0)
    # the same site read the other way round: segment 1 has the lowest id, so the direct walk comes first
    assert walks(INVERTED[0], (3, 1), (1, 1)) == (["<3<1", "<3>2<1"], 0)


def test_cycle_inside_a_flubble_repeats_no_segment():
    assert walks(*CYCLE) == ([">1>2>3>4", ">1>2>4"], 0)


def test_parallel_links_count_once():
    assert walks(*PARALLEL) == ([">1>2>3", ">1>3"], 0)


def test_same_segment_boundaries_have_no_walk():
    assert walks(SNP[0], (1, 0), (1, 1)) == ([], 0)


def test_z_segment_in_the_other_orientation_is_not_passed_through():
    # 1 -> 3- -> 2: the only way to 2 passes 3 the wrong way round, the query ends at >3
    g = graph([1, 2, 3], [("1+", "3-"), ("3-", "2+"), ("2+", "3+")])
    assert walks(g, fw(1), fw(3)) == ([], 0)
    assert walks(g, fw(1), fw(2)) == ([">1<3>2"], 0)


def test_caps_more_long_budget():
    assert walks(*SNP, max_walks=1) == ([">1>2>4"], R.MORE)
    assert walks(*SNP, max_walks=2) == ([">1>2>4", ">1>3>4"], 0)  # exactly K walks: no MORE
    assert walks(*INDEL, max_steps=2) == ([">1>2"], R.LONG)
    assert walks(*INDEL, max_steps=1) == ([], R.LONG)
    assert walks(*INDEL, max_steps=3) == ([">1>2", ">1>5>2"], 0)
    # expansions of NESTED: +2 +3 +5 +6(walk) +4 | the sixth (+5) is over a budget of 5
    assert walks(*NESTED, max_expansions=5) == ([">1>2>3>5>6"], R.BUDGET)
    # 14 expansions in all: +2 +3 +5 +6 +4 +5 +6 +7 +8 +10 +6 +9 +10 +6
    assert walks(*NESTED, max_expansions=14) == ([">1>2>3>5>6", ">1>2>4>5>6", ">1>7>8>10>6", ">1>7>9>10>6"], 0)
    assert walks(*NESTED, max_expansions=13) == ([">1>2>3>5>6", ">1>2>4>5>6", ">1>7>8>10>6"], R.BUDGET)
    # both MORE and LONG
    assert walks(*INDEL_LOW_ID, max_walks=1, max_steps=2) == ([">1>3"], R.LONG)
    assert walks(*NESTED, max_walks=1, max_steps=4) == ([], R.LONG)


def test_budget_counts_the_walk_end_and_stops_before_exceeding():
    # SNP: +2 +4(walk) +3 +4(walk): four expansions
    assert walks(*SNP, max_expansions=4) == ([">1>2>4", ">1>3>4"], 0)
    assert walks(*SNP, max_expansions=3) == ([">1>2>4"], R.BUDGET)


def test_flat_arrays_layout():
    g, s, z = NESTED
    f = R.flat(R.successors(g), [(s, z), (fw(1), fw(1)), (fw(2), fw(5))], max_walks=3)
    assert f["walk_off"].tolist() == [0, 3, 3, 5]
    assert f["step_off"].tolist() == [0, 5, 10, 15, 18, 21]
    assert f["status"].tolist() == [R.MORE, 0, 0]
    assert f["step_id"][:5].tolist() == [1, 2, 3, 5, 6] and f["step_or"].sum() == 0


@pytest.mark.parametrize("name", ["nested_deletion", "insertion_flubble", "deletion_flubble", "pvst_tests_graph"])
def test_golden_pvst_queries(golden_dir, name):
    g = _load_gfa_links(os.path.join(golden_dir, "gfa", name + ".gfa"))
    qs = R.queries_of_pvst_text(open(os.path.join(golden_dir, "pvst", name + ".pvst")).read())
    assert qs
    succ = R.successors(g)
    for s, z in qs:
        ws, st = R.walks_of(succ, s, z)
        for w in ws:  # every walk is a path of the graph from S to Z without a repeated segment
            assert w[0] == s and w[-1] == z and len({i for i, _ in w}) == len(w)
            for a, b in zip(w, w[1:]):
                assert b in succ[(a[0], 1 - a[1])]
        assert ws == sorted(ws)
    if name == "nested_deletion":
        got = [[R.as_text(w) for w in R.walks_of(succ, s, z)[0]] for s, z in qs]
        assert got == [[">0>1>3>4>5", ">0>1>4>5", ">0>2>5"], [">1>3>4", ">1>4"]]
