"""The plain-Python restatement of the region calls (tests/region_ref.py): the answers of INTEGRATION.md "Region calls" on the
popped-parent-child-rescue fixture, derivable by hand, and the lines pinned in tests/golden/region_records.json; the rules at
their edges; and for every case the GPU tests use (tests/region_cases.py) that it is not vacuous.  No GPU."""
import json

import pytest

import oracle_lib as O
import region_cases as RC
import region_ref as R
import vcf_ref as V


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    out = tmp_path_factory.mktemp("region_fx")
    n = O.decompose_gfa(RC.GFA, str(out))
    texts = [(out / f"{i}.pvst").read_text() for i in range(1, n + 1) if (out / f"{i}.pvst").exists()]
    names, paths, seqs = RC.fixture_tables()
    sites = V.sites_of_pvst(texts)
    assert sorted(V.label(s["s"], s["z"]) for s in sites) == [">0>5", ">2>4"]
    assert [names, [[s for s, _ in p] for p in paths]] == [[RC.HG1, RC.HG2, RC.HG3], [[0, 1, 2, 3, 4, 5], [0, 5], [0, 1, 2, 6, 4, 5]]]
    assert all(len(seqs[k]) == 1 for k in seqs)
    return sites, names, paths, seqs


def _lines(text):
    return [ln for ln in text.splitlines() if not ln.startswith("#")]


@pytest.mark.parametrize("row", sorted(RC.FIXTURE_ROWS))
def test_fixture_rows(fixture, row):
    sites, names, paths, seqs = fixture
    regions, want = RC.FIXTURE_ROWS[row]
    recs, text, full = R.call("plain", sites, names, paths, seqs, ["HG1"], regions)
    assert sorted(r["id"] for r in recs) == want and len(full) == 2
    assert [r["chrom"] for r in recs] == [RC.HG1] * len(want)  # (a region on HG2 or HG3 still selects records written on HG1)
    full_text = R.call("plain", sites, names, paths, seqs, ["HG1"], None)[1]
    head = [ln for ln in full_text.splitlines() if ln.startswith("#")]
    assert [ln for ln in text.splitlines() if ln.startswith("#")] == head  # header and contig lines are unchanged
    assert _lines(text) == [ln for ln in _lines(full_text) if ln.split("\t")[2] in want]  # byte for byte, in the same order
    golden = json.load(open(RC.GOLDEN))
    assert _lines(text) == golden["plain"][row]


def test_fixture_nested_child_keeps_its_parent_fields(fixture):
    sites, names, paths, seqs = fixture
    recs, text, full = R.call("nested", sites, names, paths, seqs, ["HG1"], [(RC.HG1, 3, 4)])
    assert [r["id"] for r in recs] == [">2>4"] and len(full) == 2
    (line,) = _lines(text)
    assert line.split("\t")[7].endswith(";ES=>2>4;LV=1;PS=>0>5")  # the parent is not written, the child still names it
    assert [line] == json.load(open(RC.GOLDEN))["nested"]["second-boundary-of-the-child"]
    popt = json.load(open(RC.GOLDEN.replace("region_records", "reference_nested_records")))["popped_options"]
    recs, text, full = R.call("popped", sites, names, paths, seqs, ["HG1"], [(RC.HG1, 3, 4)], **popt)
    assert [(r["id"], r.get("rescued")) for r in recs] == [(">2>4:rescued", True)] and "POPPED_PARENT=>0>5" in _lines(text)[0]
    assert R.call("popped", sites, names, paths, seqs, ["HG1"], [(RC.HG1, 1, 2)], **popt)[0] == []  # the parent passes, and is popped


def test_strings_and_tuples_are_one_region(fixture):
    sites, names, paths, seqs = fixture
    a = R.call("plain", sites, names, paths, seqs, ["HG1"], [f"{RC.HG1}:3-4"])[1]
    assert a == R.call("plain", sites, names, paths, seqs, ["HG1"], [(RC.HG1, 3, 4)])[1]
    assert R.call("plain", sites, names, paths, seqs, ["HG1"], [(RC.HG1, 1, 2 ** 62)])[1] == R.call("plain", sites, names, paths, seqs, ["HG1"], None)[1]


def test_step_predicate_at_every_off_by_one():
    for off in (0, 1, 7):
        for ln in (0, 1, 2, 5):
            first, behind = off + 1, off + 1 + max(ln, 1)
            assert not R.step_in_region(off, ln, max(first - 1, 0), first)  # e == off + 1
            assert R.step_in_region(off, ln, max(first - 1, 0), first + 1)
            assert not R.step_in_region(off, ln, behind, behind + 3)  # s == off + 1 + len
            assert R.step_in_region(off, ln, behind - 1, behind + 3)
    assert R.step_in_region(4, 0, 5, 6) and not R.step_in_region(4, 0, 6, 7) and not R.step_in_region(4, 0, 4, 5)


def test_marks_are_by_intersection_and_in_either_orientation():
    names, seqs = ["p", "q"], {1: "AAAA", 2: "C", 3: "", 4: "GG"}
    paths = [[(1, 0), (2, 0), (3, 0), (4, 0)], [(4, 1), (2, 1), (1, 1)]]  # q walks backwards and skips 3
    assert R.marked_segments(names, paths, seqs, [("p", 3, 4)]) == {1}  # strictly inside the first segment
    assert R.marked_segments(names, paths, seqs, [("p", 4, 6)]) == {1, 2}
    assert R.marked_segments(names, paths, seqs, [("p", 6, 7)]) == {3, 4}  # the segment without bases counts as position 6
    assert R.marked_segments(names, paths, seqs, [("q", 1, 3)]) == {4}
    assert R.marked_segments(names, paths, seqs, [("q", 3, 4), ("p", 1, 2)]) == {1, 2}
    assert R.marked_segments(names, paths, seqs, [("p", 8, 90)]) == set()  # beyond the path's end
    sites = [dict(s=(1, 0), z=(4, 0)), dict(s=(2, 0), z=(3, 0))]
    assert R.passing_sites(sites, names, paths, seqs, [("p", 5, 6)]) == [False, True]
    assert R.passing_sites(sites, names, paths, seqs, [("q", 1, 2)]) == [True, False]


def test_refusals():
    names = ["p"]
    for bad, word in ((("x", 1, 2), "no path is named x"), (("p", 5, 5), "start < end"), (("p", 9, 3), "start < end"),
                      (("p", 1, 2 ** 63), "2\\^63")):
        with pytest.raises(R.RegionError, match=word):
            R.regions_of([bad], names)
    with pytest.raises(R.RegionError, match="more than 65536"):
        R.regions_of([("p", 1, 2)] * 65537, names)
    assert len(R.regions_of([("p", 1, 2)] * 65536, names)) == 65536


_SITES = {}


def _sites(workload):
    if workload not in _SITES:
        _SITES[workload] = V.sites_of_pvst(list(O.decompose(RC.workload(workload)[0]).values()))
    return _SITES[workload]


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_no_case_of_the_gpu_tests_is_vacuous(case):
    workload, mode, regions, opts = RC.CASES[case]
    names, paths, seqs = RC.tables(workload)
    popt = {k: v for k, v in opts.items() if k != "tier2"}
    recs, text, full = R.call(mode, _sites(workload), names, paths, seqs, list(RC.workload(workload)[3]), regions, **popt)
    assert 0 < len(recs) < len(full), (len(recs), len(full))
    if mode == "inversions":  # inversion records on both sides
        kept = sum(r["q"] == R.NIL for r in recs)
        assert 0 < kept < sum(r["q"] == R.NIL for r in full)
    assert len(_lines(text)) > 0


def test_the_edge_cases_differ_where_the_rule_says():
    """One position more or less at a boundary segment's first and last base changes what passes exactly as the predicate says."""
    names, paths, seqs = RC.tables("chain")
    sites = _sites("chain")
    n = {k: sum(R.passing_sites(sites, names, paths, seqs, RC.CASES["chain-" + k][2])) for k in RC._edge_regions()}
    # the boundary segment is the Z of one site and the S of the next: the site on the far side of it comes and goes with its mark
    assert n["start-last-1"] == n["start-last+0"] == n["start-last+1"] + 1  # gone once the start is behind its last base
    assert n["start-first-1"] >= n["start-first+0"] == n["start-first+1"] == n["start-last+0"]
    assert n["end-first-1"] <= n["end-first+0"] == n["end-first+1"] - 1  # an exclusive end on the first base does not hold it
    assert n["end-first+1"] == n["end-last-1"] == n["end-last+0"] <= n["end-last+1"]
    assert n["strictly-inside-a-boundary"] == 2
