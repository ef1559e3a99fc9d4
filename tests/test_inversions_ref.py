"""The plain-Python restatement of the inversion calls (tests/inversions_ref.py) against the two records the reference
states (tests/golden/reference_subr_records.json) and hand-made cases, one per rule of INTEGRATION.md "Inversion calls"."""
import json
import os

import inversions_ref as I
import vcf_ref as V

BASE = "ACGT"


def _recs(paths, names=None, prefixes=("ref",), seqs=None, max_steps=65536):
    names = names or (["ref"] + [f"p{k}" for k in range(1, len(paths))])
    if seqs is None:
        seqs = {s: BASE[s % 4] for p in paths for s, _ in p}
    return I.records(names, paths, seqs, list(prefixes), max_steps)


def _fwd(ids):
    return [(i, 0) for i in ids]


def _inv(ids):
    """The steps of _fwd(ids) walked backwards."""
    return [(i, 1) for i in reversed(ids)]


def _keys(recs):
    return [(r["path"], r["first"], r["n_steps"]) for r in recs]


def test_the_two_pinned_records(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "reference_subr_records.json")))
    for name, rel in want["fixtures"].items():
        names, paths, seqs = V.read_gfa(os.path.join(golden_dir, rel))
        recs, stats = I.records(names, paths, seqs, [want["reference_prefix"]])
        assert len(recs) == 1 and stats["heads"] == 1, name
        r = recs[0]
        assert {k: r[k] for k in want["record"]} == want["record"], name
        assert I.record_line(r) == want["line"], name
        assert V.slots_of(names)[0] == want["samples"]
        # a call with no site: the record alone, and the VCF's last line
        merged = I.call([], names, paths, seqs, [want["reference_prefix"]])
        assert merged == recs
        assert I.vcf_text(names, paths, seqs, merged, ["ref"]).splitlines()[-1] == want["line"]


def test_no_record_on_the_ten_flubble_fixtures(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "reference_vcf_records.json")))
    assert len(want["fixtures"]) == 10
    for name in want["fixtures"]:
        names, paths, seqs = V.read_gfa(os.path.join(golden_dir, "gfa", name + ".gfa"))
        assert I.records(names, paths, seqs, [want["reference_prefix"]])[0] == [], name


def test_runs_cut_by_each_path_end():
    ref = _fwd([1, 2, 3, 4])
    recs, stats = _recs([ref, _inv([1, 2, 3]), _inv([3, 4])])
    # p1 walks 1..3 backwards: the run starts at ref's first step and ends with p1's first; p2: ends at ref's last step
    assert _keys(recs) == [(0, 0, 3), (0, 2, 2)] and stats["heads"] == 2
    assert [(r["pos"], r["ref"], r["alts"], r["id"]) for r in recs] == [(2, "CGT", ["ACG"], ">1>3"), (4, "TA", ["TA"], ">3>4")]
    assert recs[1]["ref"] == recs[1]["alts"][0]  # (a palindromic REF is written as is)
    assert [r["gt"] for r in recs] == [["0", "1", "."], ["0", ".", "1"]]
    assert recs[0]["at"] == [">1>2>3", "<3<2<1"]


def test_supporters_in_other_slots_and_in_the_reference_slot():
    ref = _fwd([1, 2, 3])
    recs, _ = _recs([ref, _inv([1, 2, 3]), _inv([1, 2, 3]) + _fwd([9])], names=["ref", "s#1#c", "s#2#c"])
    assert _keys(recs) == [(0, 0, 3)]
    assert (recs[0]["slots"], recs[0]["gt"], recs[0]["ac"], recs[0]["an"], recs[0]["ns"]) == ([0, 1, 1], ["0", "1|1"], [2], 3, 2)
    # a supporter that shares the reference's slot: the slot stays 0
    recs, _ = _recs([ref, _inv([1, 2, 3]), _fwd([1, 2, 3])], names=["x#1#c1", "x#1#c2", "y#1#c1"], prefixes=["x#1#c1"])
    assert _keys(recs) == [(0, 0, 3)]
    assert (recs[0]["slots"], recs[0]["gt"], recs[0]["ac"], recs[0]["an"], recs[0]["ns"]) == ([0, None], ["0", "."], [0], 1, 1)
    assert I.record_line(recs[0]).split("\t")[7].startswith("AC=0;AF=0.0;AN=1;NS=1;")


def test_groups_that_share_the_first_step_but_not_the_length():
    ref = _fwd([1, 2, 3, 4])
    recs, _ = _recs([ref, _inv([1, 2, 3]) + _fwd([4]), _inv([1, 2]) + _fwd([3, 4]), _inv([1, 2]) + _fwd([7])])
    assert _keys(recs) == [(0, 0, 2), (0, 0, 3)]
    assert [r["slots"] for r in recs] == [[0, None, 1, 1], [0, 1, None, None]]
    assert [r["pos"] for r in recs] == [2, 2]


def test_a_repeat_visited_three_times_by_the_reference_and_twice_by_the_other_path():
    ref = [(1, 0), (2, 0), (1, 0), (3, 0), (1, 0)]
    alt = [(1, 1), (2, 1), (1, 1)]
    found, stats = I.runs([ref, alt], [0])
    # the six matches of segment 1 and the one of segment 2: the anti-diagonal (0, 2), (1, 1), (2, 0) is one run, the
    # other four matches are runs of one step
    assert sorted((i, j, n) for _r, i, n, _a, j in found) == [(0, 0, 1), (0, 2, 3), (2, 2, 1), (4, 0, 1), (4, 2, 1)]
    assert stats["heads"] == 5 and stats["max_opposite"] == 2
    recs, _ = _recs([ref, alt])
    assert _keys(recs) == [(0, 0, 3)] and recs[0]["at"] == [">1>2>1", "<1<2<1"]


def test_one_step_runs_and_the_step_limit():
    ref = _fwd([1, 2, 3, 4, 5])
    assert _recs([ref, [(9, 0), (3, 1), (8, 0)]])[0] == []  # L == 1
    recs, stats = _recs([ref, _inv([1, 2, 3, 4, 5])], max_steps=5)
    assert _keys(recs) == [(0, 0, 5)] and stats["long"] == 0
    recs, stats = _recs([ref, _inv([1, 2, 3, 4, 5])], max_steps=4)
    assert recs == [] and stats["long"] == 1 and stats["heads"] == 1


def test_a_run_of_empty_segments_is_dropped():
    ref = _fwd([1, 2, 3])
    seqs = {1: "", 2: "", 3: "G", 9: "T"}
    assert _recs([ref, _inv([1, 2]) + _fwd([9])], seqs=seqs)[0] == []
    recs, _ = _recs([ref, _inv([1, 2, 3])], seqs=seqs)
    assert _keys(recs) == [(0, 0, 3)] and (recs[0]["ref"], recs[0]["alts"], recs[0]["pos"]) == ("G", ["C"], 1)


def test_both_backward_ids_are_written_forward():
    recs, _ = _recs([_inv([3, 4, 5]), _fwd([3, 4, 5])])
    assert _keys(recs) == [(0, 0, 3)]
    assert (recs[0]["id"], recs[0]["at"]) == (">5>3", ["<5<4<3", ">3>4>5"])
    recs, _ = _recs([[(5, 1), (4, 0)], [(4, 1), (5, 0)]])
    assert (recs[0]["id"], recs[0]["at"]) == ("<5>4", ["<5>4", "<4>5"])
    assert I.step_label((5, 0), (4, 1)) == ">5<4"


def test_two_reference_paths_that_invert_each_other():
    recs, _ = _recs([_fwd([1, 2, 3]), _inv([1, 2, 3])], names=["ref1", "ref2"], prefixes=["ref"])
    assert _keys(recs) == [(0, 0, 3), (1, 0, 3)]
    assert [(r["chrom"], r["id"], r["ref"], r["alts"], r["gt"]) for r in recs] == \
        [("ref1", ">1>3", "CGT", ["ACG"], ["0", "1"]), ("ref2", ">3>1", "ACG", ["CGT"], ["1", "0"])]


def test_merged_order_puts_flubble_records_first_at_one_pos():
    # the bubble 1 > (2 | 3) > 4 called by ref, and p2 walking 1 > 2 backwards: both records have POS 2
    pvst = ["H\t0.0.3\t.\t.\t.\nD\t0\t.\t1\t.\nF\t1\t>1>4\t.\tL\n"]
    names, paths = ["ref", "p1", "p2"], [_fwd([1, 2, 4]), _fwd([1, 3, 4]), _inv([1, 2])]
    seqs = {1: "A", 2: "C", 3: "G", 4: "T"}
    merged = I.call(V.sites_of_pvst(pvst), names, paths, seqs, ["ref"])
    assert [(r["pos"], r["vartype"], r["q"], r["n_steps"]) for r in merged] == [(2, "SUB", 0, 0), (2, "SUBR", I.NIL, 2)]
    text = I.vcf_text(names, paths, seqs, merged, ["ref"])
    assert [ln.split("\t")[7].split(";")[5:] for ln in text.splitlines()[-2:]] == \
        [["VARTYPE=SUB", "TANGLED=F", "ES=>1>4", "LV=0"], ["VARTYPE=SUBR", "TANGLED=F"]]
