"""The plain-Python restatement of the variant calls (tests/vcf_ref.py) on the ten flubble fixtures, against the records
the reference states for them (tests/golden/reference_vcf_records.json), and on hand cases for what the fixtures do not
reach: a reverse reference traversal, a diploid PanSN sample, an ambiguous slot, a multi-allelic record mixing DEL and
SUB alleles, and the presence reading across two reference contigs."""
import json
import os

import pytest

import oracle_lib as O
import vcf_ref as V

KEYS = ("chrom", "pos", "id", "ref", "alts", "at", "vartype", "lv", "gt", "ac", "an")


def _fixture(golden_dir, name, tmp_path):
    gfa = os.path.join(golden_dir, "gfa", name + ".gfa")
    out = tmp_path / name
    out.mkdir()
    n = O.decompose_gfa(gfa, str(out))
    texts = [(out / f"{i}.pvst").read_text() for i in range(1, n + 1) if (out / f"{i}.pvst").exists()]
    return V.read_gfa(gfa), V.sites_of_pvst(texts)


def test_fixtures_match_reference_records(golden_dir, tmp_path):
    want = json.load(open(os.path.join(golden_dir, "reference_vcf_records.json")))
    assert len(want["fixtures"]) == 10
    for name, fx in sorted(want["fixtures"].items()):
        (names, paths, seqs), sites = _fixture(golden_dir, name, tmp_path)
        recs = V.call(sites, names, paths, seqs, [want["reference_prefix"]])
        assert [{k: r[k] for k in KEYS} for r in recs] == fx["records"], name
        text = V.vcf_text(names, paths, seqs, recs, [want["reference_prefix"]])
        assert text.splitlines()[len(V.HEADER.splitlines()) + 1].split("\t")[9:] == fx["samples"], name
        for r in recs:
            assert not r["tangled"] and r["ns"] == 2


def test_nested_deletion_line(golden_dir, tmp_path):
    (names, paths, seqs), sites = _fixture(golden_dir, "nested_deletion", tmp_path)
    recs = V.call(sites, names, paths, seqs, ["HG1"])
    text = V.vcf_text(names, paths, seqs, recs, ["HG1"], date="20261016")
    lines = text.splitlines()
    assert lines[1] == "##fileDate=20261016"
    assert lines[3] == lines[12]  # the duplicated FORMAT line stays
    assert lines[13] == "##contig=<ID=HG1#1#chr1,length=5>"
    assert lines[-1] == ("HG1#1#chr1\t2\t>1>4\tCT\tC\t60\tPASS\tAC=1;AF=0.5;AN=2;NS=2;AT=>1>3,>1;VARTYPE=DEL;TANGLED=F;"
                         "ES=>1>4;LV=1\tGT\t0\t1\t.")


def _one(pvst, names, paths, seqs, prefixes):
    return V.call(V.sites_of_pvst(pvst), names, paths, seqs, prefixes)


PV1 = ["H\t0.0.3\t.\t.\t.\nD\t0\t.\t1\t.\nF\t1\t>1>4\t.\tL\n"]
SEQS = {1: "AC", 2: "GGT", 3: "T", 4: "CA", 5: "TTA"}


def test_reverse_reference_traversal():
    # the reference reads the bubble from 4 to 1 on its reverse strand; the alleles are flipped and reverse-complemented
    names = ["ref", "alt"]
    paths = [[(4, 1), (3, 1), (1, 1)], [(1, 0), (2, 0), (4, 0)]]
    recs = _one(PV1, names, paths, SEQS, ["ref"])
    assert len(recs) == 1
    r = recs[0]
    # flip(Z) = <4 spells TG, then <3 spells A: not anchored, REF = A at POS len(TG) + 1, ALT = revcomp(GGT) = ACC
    assert (r["pos"], r["ref"], r["alts"], r["at"], r["vartype"]) == (3, "A", ["ACC"], ["<3", "<2"], "SUB")
    assert r["gt"] == ["0", "1"]


def test_diploid_sample_and_ambiguous_slot():
    names = ["R#0#c", "S#1#c", "S#2#c", "T#1#c", "T#1#d"]
    paths = [[(1, 0), (3, 0), (4, 0)], [(1, 0), (2, 0), (4, 0)], [(1, 0), (3, 0), (4, 0)],
             [(1, 0), (2, 0), (4, 0)], [(1, 0), (3, 0), (4, 0)]]
    recs = _one(PV1, names, paths, SEQS, ["R#"])
    r = recs[0]
    # S is diploid (1|0); T's one slot holds two alleles over its two contigs: '.', and the record is tangled
    assert r["gt"] == ["0", "1|0", "."]
    assert (r["ac"], r["an"], r["ns"], r["tangled"]) == ([1], 3, 2, True)
    assert V.record_line(r).split("\t")[7].startswith("AC=1;AF=0.3;AN=3;NS=2;")


def test_multiallelic_del_and_sub():
    names = ["ref", "a", "b"]
    paths = [[(1, 0), (2, 0), (4, 0)], [(1, 0), (4, 0)], [(1, 0), (3, 0), (4, 0)]]
    recs = _one(PV1, names, paths, SEQS, ["ref"])
    r = recs[0]
    # one ALT is empty: the record is anchored on the last base of AC, and it is a DEL
    assert (r["pos"], r["ref"], r["alts"], r["at"], r["vartype"]) == (2, "CGGT", ["C", "CT"], [">1>2", ">1", ">1>3"], "DEL")
    assert r["gt"] == ["0", "1", "2"] and r["ac"] == [1, 1]
    assert "AF=0.3,0.3" in V.record_line(r)


def test_presence_across_two_reference_contigs():
    # two trees, one reference contig on each: every present reference path crosses each bubble, so both are called
    pv = PV1 + ["H\t0.0.3\t.\t.\t.\nD\t0\t.\t1\t.\nF\t1\t>11>14\t.\tL\n"]
    seqs = {**SEQS, **{k + 10: v for k, v in SEQS.items()}}
    names = ["G#1#chr1", "G#1#chr2", "H#1#chr1", "H#1#chr2"]
    paths = [[(1, 0), (2, 0), (4, 0)], [(11, 0), (12, 0), (14, 0)], [(1, 0), (3, 0), (4, 0)], [(11, 0), (13, 0), (14, 0)]]
    recs = _one(pv, names, paths, seqs, ["G#"])
    assert [(r["chrom"], r["id"]) for r in recs] == [("G#1#chr1", ">1>4"), ("G#1#chr2", ">11>14")]
    # a reference contig that misses one boundary makes the bubble uncallable
    paths[0] = [(1, 0), (2, 0)]
    assert [r["id"] for r in _one(pv, names, paths, seqs, ["G#"])] == [">11>14"]


def test_refusals():
    with pytest.raises(V.CallError, match="no path name"):
        _one(PV1, ["a"], [[(1, 0), (2, 0), (4, 0)]], SEQS, ["x"])
    with pytest.raises(V.CallError, match="segment 2"):
        _one(PV1, ["r", "a"], [[(1, 0), (2, 0), (4, 0)], [(1, 0), (3, 0), (4, 0)]], {**SEQS, 2: "GQ"}, ["r"])
