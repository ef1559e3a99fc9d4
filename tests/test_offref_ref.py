"""The plain-Python restatement of the off-reference calls (tests/offref_ref.py) on the graph the feature was stated on, on
the reference's nested-child-inside-insertion fixture, on hand cases whose lines are written out in
tests/golden/offref_records.json, and the refusals of `povu call --off-reference` that need no GPU.  No GPU."""
import os
import subprocess

import pytest

import offref_cases as OC
import offref_ref as F
import vcf_ref as V

ROOT = OC.ROOT
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"


def _case(name, tmp_path):
    return OC.load(OC.gfa_of(name), tmp_path / name)


def test_the_graph_of_the_issue(tmp_path):
    sites, names, paths, seqs, _ = _case(OC.ISSUE, tmp_path)
    assert [V.label(s["s"], s["z"]) for s in sites] == [">0>3", ">4>7"] and {s["parent"] for s in sites} == {V.NO_PARENT}
    recs, counts = F.call(sites, names, paths, seqs, ["HG1"])
    text = F.vcf_text(sites, names, paths, seqs, recs, ["HG1"], date=DATE)
    lines = OC.records_of(text)
    assert len(lines) == 2
    plain = V.call(sites, names, paths, seqs, ["HG1"])
    assert lines[0] == V.record_line(plain[0]) and len(plain) == 1 and plain[0]["id"] == ">0>3"
    assert (plain[0]["ref"], plain[0]["alts"]) == ("CG", ["CATT", "CGTT"])
    assert lines[1] == ("HG2#1#chr1\t3\t>4>7\tA\tG\t60\tPASS\tAC=2;AF=0.7;AN=3;NS=3;AT=>5,>6;VARTYPE=SUB;TANGLED=F;ES=>4>7;LV=0;"
                        "OFFREF=T;HOST=>0>3;HA=1\tGT\t.\t0\t1\t1")
    assert OC.contigs_of(text) == ["HG1#1#chr1,length=4", "HG2#1#chr1,length=6"]
    # without its three added keys the record is that of the call with HG2 as the only reference
    by_hg2 = [V.record_line(r) for r in V.call(sites, names, paths, seqs, ["HG2"]) if r["id"] == ">4>7"]
    assert by_hg2 == [lines[1].replace(";OFFREF=T;HOST=>0>3;HA=1", "")]
    assert counts == dict(n_offref_sites=1, n_offref_records=1, n_offref_hosted=1)
    # the header: the three INFO lines behind the verbatim header, in front of the contig lines
    head = text.splitlines()
    k = len(V.HEADER.splitlines())
    assert [ln.split(",")[0] for ln in head[k:k + 3]] == ["##INFO=<ID=OFFREF", "##INFO=<ID=HOST", "##INFO=<ID=HA"]
    assert "Number=0,Type=Flag" in head[k] and "Number=1,Type=String" in head[k + 1] and "Number=1,Type=Integer" in head[k + 2]
    assert head[k + 3].startswith("##contig")
    # -o DIR: the prefix's file and off-reference.vcf
    assert OC.records_of(F.vcf_text(sites, names, paths, seqs, recs, ["HG1"], only="HG1")) == lines[:1]
    rest = F.vcf_text(sites, names, paths, seqs, recs, ["HG1"], rest=True)
    assert OC.records_of(rest) == lines[1:] and OC.contigs_of(rest) == ["HG2#1#chr1,length=6"]


def test_nothing_is_fabricated_on_the_reference_fixture(tmp_path):
    sites, names, paths, seqs, _ = OC.load(OC.FIXTURE, tmp_path / "fx")
    assert [V.label(s["s"], s["z"]) for s in sites] == [">0>3"]  # (its inner child is no PVST site)
    recs, counts = F.call(sites, names, paths, seqs, ["HG1"])
    plain = V.call(sites, names, paths, seqs, ["HG1"])
    assert counts["n_offref_records"] == 0 and counts["n_offref_sites"] == 0
    assert [F.record_line(r, sites) for r in recs] == [V.record_line(r) for r in plain] and len(plain) == 1
    assert OC.contigs_of(F.vcf_text(sites, names, paths, seqs, recs, ["HG1"])) == OC.contigs_of(V.vcf_text(names, paths, seqs, plain, ["HG1"]))


@pytest.mark.parametrize("name", sorted(OC.golden()["cases"]))
def test_hand_cases(name, tmp_path):
    want = OC.golden()["cases"][name]
    sites, names, paths, seqs, _ = _case(name, tmp_path)
    assert len(seqs) <= 20
    recs, counts = F.call(sites, names, paths, seqs, [OC.golden()["reference_prefix"]])
    text = F.vcf_text(sites, names, paths, seqs, recs, [OC.golden()["reference_prefix"]], date=DATE)
    assert OC.records_of(text) == want["lines"]
    assert OC.contigs_of(text) == want["contigs"]
    assert counts == want["counts"]


def test_what_the_hand_cases_reach(tmp_path):
    got = {}
    for name in OC.golden()["cases"]:
        sites, names, paths, seqs, _ = _case(name, tmp_path)
        got[name] = (sites, names, F.call(sites, names, paths, seqs, ["HG1"])[0])
    off = {k: [r for r in v[2] if r["offref"]] for k, v in got.items()}
    # backwards: REF is the reverse complement of the forward allele, POS counts from the surrogate's start
    assert off["backwards"][0]["at"] == ["<5", "<6"] and (off["backwards"][0]["ref"], off["backwards"][0]["pos"]) == ("T", 4)
    # the outer bubble of the insertion writes nothing; the inner one is a level down
    sites = got["bubble-in-bubble"][0]
    assert [V.label(s["s"], s["z"]) for s in sites] == [">0>3", ">4>7", ">5>12"] and sites[2]["parent"] == 1
    assert [r["id"] for r in off["bubble-in-bubble"]] == [">5>12"] and off["bubble-in-bubble"][0]["lv"] == 1
    # two surrogates, the second behind the first in the concatenation
    assert [r["path"] for r in off["two-insertions"]] == [1, 2] and [r["host"] for r in off["two-insertions"]] == [0, 2]
    # a surrogate that is a reference path
    assert off["surrogate-is-reference"][0]["chrom"] == "HG1#2#chr1"
    assert F.off_contigs(got["surrogate-is-reference"][1], got["surrogate-is-reference"][2], ["HG1"]) == []
    assert off["no-host"][0]["host"] is None and off["one-allele"] == []


def test_enclosure():
    assert F.encloses(0, 4, 1, 3) and F.encloses(1, 4, 1, 3) and F.encloses(0, 3, 1, 3)
    assert not F.encloses(1, 3, 1, 3) and not F.encloses(2, 5, 1, 3) and not F.encloses(0, 2, 1, 3)


@pytest.mark.parametrize("extra,word", [(["--nested"], "--nested"), (["--profile", "decomposed", "--merge-primitives"], "--merge-primitives"),
                                        (["--profile", "popped"], "raw-graph"), (["--profile=left-normalized"], "raw-graph"),
                                        (["--profile", "decomposed"], "raw-graph"), (["--profile", "top-level-only"], "raw-graph")])
def test_the_cli_refuses_the_flag_with_what_it_cannot_join(extra, word):
    if not os.path.exists(POVU):
        import __graft_entry__ as G
        G.build()
    r = subprocess.run([POVU, "call", "-i", "x.gfa", "-P", "a", "--off-reference"] + extra, capture_output=True, text=True, timeout=120)
    out = r.stderr + r.stdout
    assert r.returncode != 0 and "--off-reference" in out and word in out, out
    # alone the flag is taken: the run gets as far as the graph it cannot read
    r = subprocess.run([POVU, "call", "-i", "/nonexistent/x.gfa", "-P", "a", "--off-reference"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--off-reference" not in r.stderr + r.stdout
    r = subprocess.run([POVU, "call", "--help"], capture_output=True, text=True, timeout=120)
    assert "--off-reference" in r.stderr + r.stdout
