"""The consensus haplotypes without a GPU (INTEGRATION.md "Consensus haplotypes"): the restatement (tests/vcfcons_ref.py) on the
two golden files pinned by hand and on the drop rule case by case; tests/golden/vcfcons_expected.json against the restatement;
the rules as the device runs them (hip/vcfcons_rules.hpp) on the CPU under the sanitizers (`make vcfcons_check`); the refusals
of `povu vcf --consensus` by name; the three text writers on a hand-made result through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import vcfcmp_ref as M
import vcfcons_cases as K
import vcfcons_ref as CR
from povu_amd import hip as H

ROOT = K.ROOT
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")


def _golden(fixture):
    names, ref = K.gfa_named(K.K.gfa_path(fixture))
    res, doc = K.ref_run(K.golden(fixture, "raw_graph"), names, ref)
    return res, doc, names


def _by_sample(res, doc):
    return {doc["samples"][h["col"]]: h for h in res["haps"]}


def test_the_tandem_file_pinned_by_hand():
    res, doc, _ = _golden("tandem-repeat-left-normalization")
    haps = _by_sample(res, doc)
    assert {s: h["text"] for s, h in haps.items()} == dict(HG1="AAAAAC", HG2="AAAAC", HG3="AAAAAAC")
    assert K.statuses(res) == ["equal"] * 3 and res["n_unplaced"] == 0
    assert [h["n_applied"] for h in res["haps"]] == [0, 1, 1] and all(h["n_nocall"] == 0 for h in res["haps"])


def test_the_popped_file_pinned_by_hand():
    res, doc, names = _golden("popped-parent-child-rescue")
    haps = _by_sample(res, doc)
    assert haps["HG1"]["rt_status"] == CR.RT_EQUAL and haps["HG1"]["text"] == "AAAAAC"
    assert haps["HG2"]["text"] == "AC" and haps["HG2"]["rt_status"] == CR.RT_EQUAL and haps["HG2"]["n_nocall"] == 1
    h3 = haps["HG3"]  # the second record sits at POS 3, the graph has that base at POS 4
    assert h3["text"] == "AAGAAC" and h3["rt_status"] == CR.RT_DIFFER and h3["rt_first_diff"] == 2 and (h3["len"], h3["rt_path_len"]) == (6, 6)
    assert names[h3["rt_path"]] == "HG3#1#chr1"
    assert CR.roundtrip_text(doc, res, names).split("\n")[1] == "HG1#1#chr1\tHG3\t0\tdiffer\t6\tHG3#1#chr1\t6\t2\t1\t0\t0\t0\t0\t0"
    assert CR.fasta_text(doc, res).startswith(">HG1#1#HG1#1#chr1\nAAAAAC\n>HG2#1#HG1#1#chr1\nAC\n")


def test_the_drop_rule_case_by_case():
    assert sorted(K.DROP_CASES) == sorted(K.DROP_PINS)
    for name, (counts, text) in K.DROP_PINS.items():
        vcf_text, named = K.drop_case(name)
        res, _ = K.ref_run(vcf_text, [n for n, _ in named], dict(named))
        (h,) = res["haps"]
        assert (h["n_applied"], h["n_duplicate"], h["n_enclosed"], h["n_overlap"]) == counts, name
        assert h["text"] == text and h["len"] == len(text), name


def test_the_expected_file_is_the_restatements():
    assert K.expected() == K.expected_now()  # (K.write_expected() writes it)


def test_order_selection_unspelled_and_no_path():
    named = [("s1#1#c", "ACGTACGT"), ("s1#2#c", "ACGTTCGT"), ("other", "GGGG")]
    names, ref = [n for n, _ in named], dict(named)
    rows = [("s1#1#c", 5, "r0", "A", "T,*", ["0|1", "2", "."]), ("s1#1#c", 2, "r1", "C", "G", ["0|0", "3", "1"]),
            ("nowhere", 1, "r2", "A", "C", ["1|1", "1", "1"]), ("other", 4, "r3", "G", "GA", ["1|0", "0", "1"])]
    text = K.vcf(["s1", "s2", "x"], rows)
    res, doc = K.ref_run(text, names, ref)
    assert [(h["chrom"], h["col"], h["phase"]) for h in res["haps"]] == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 2, 0), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 2, 0)]
    assert res["n_unplaced"] == 1
    by = {(h["chrom"], h["col"], h["phase"]): h for h in res["haps"]}
    assert by[(0, 0, 1)]["text"] == "ACGTTCGT" and by[(0, 0, 1)]["rt_status"] == CR.RT_EQUAL and by[(0, 0, 1)]["rt_path"] == 1
    assert by[(0, 1, 0)]["n_unspelled"] == 2 and by[(0, 1, 0)]["rt_status"] == CR.RT_NO_PATH  # `*`, an allele beyond the ALTs; no sample s2
    assert by[(0, 2, 0)]["n_nocall"] == 1 and by[(0, 2, 0)]["text"] == "AGGTACGT"
    # a CHROM without a third field takes the slot's paths as they are: s1's first slot holds s1#1#c alone
    assert by[(2, 0, 0)]["text"] == "GGGGA" and (by[(2, 0, 0)]["rt_status"], by[(2, 0, 0)]["rt_first_diff"]) == (CR.RT_DIFFER, 0)
    one, _ = K.ref_run(text, names, ref, samples=["s1"], chroms=["s1#1#c"])
    assert [h["text"] for h in one["haps"]] == [by[(0, 0, 0)]["text"], by[(0, 0, 1)]["text"]]


def test_vcfcons_check_builds_and_passes():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "vcfcons_check", "-s"])
    r = subprocess.run([os.path.join(ROOT, "build", "obj", "vcfcons_check")], capture_output=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    assert r.stdout.decode().split("\n")[-2] == "vcfcons_check: ok"


def _run(*args):
    return subprocess.run([POVU] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_flags_that_do_not_go_together_are_refused_by_name(tmp_path):
    vcf = tmp_path / "v.vcf"
    vcf.write_text(K.K.K.COLUMNS + "\n")
    gfa = tmp_path / "g.gfa"
    gfa.write_text("S\t1\tA\n")
    for flag in (["--roundtrip"], ["--no-fasta"], ["--sample", "x"], ["--chrom=c"], ["--line-width", "10"]):
        name = flag[0].split("=")[0]
        r = _run("vcf", "-i", gfa, "-c", vcf, "--report", *flag)
        assert r.returncode == 1 and f"{name} is read by --consensus only" in r.stderr, (flag, r.stderr)
    r = _run("vcf", "-i", gfa, "-c", vcf, "--consensus", "--report")
    assert r.returncode == 1 and "--consensus and --report exclude each other" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", vcf, "-d", vcf, "--consensus", "--compare")
    assert r.returncode == 1 and "--consensus and --compare exclude each other" in r.stderr
    for args in (["--consensus", "--tui"], ["--tui", "--consensus"]):
        r = _run("vcf", "-i", gfa, "-c", vcf, *args)
        assert r.returncode == 1 and "--consensus and --tui exclude each other" in r.stderr
    r = _run("vcf", "-c", vcf, "--consensus")
    assert r.returncode == 1 and "--consensus needs the graph" in r.stderr and "Flag 'gfa' is required" in r.stderr
    r = _run("vcf", "-i", gfa, "--consensus")
    assert r.returncode == 1 and "Flag 'vcf' is required" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", vcf, "--consensus", "--haplotypes")
    assert r.returncode == 1 and "--haplotypes is not read by --consensus" in r.stderr
    for bad in ("-1", "wide", ""):
        r = _run("vcf", "-i", gfa, "-c", vcf, "--consensus", "--line-width=" + bad)
        assert r.returncode == 1 and "'--line-width' expects a number of bases" in r.stderr, bad
    r = _run("vcf", "-i", gfa, "-c", vcf, "--tui")  # as before
    assert r.returncode == 1 and "the interactive --tui is not provided" in r.stderr and "--consensus" not in r.stderr
    help_text = _run("--help").stdout
    assert all(f in help_text for f in ("--consensus", "--roundtrip", "--no-fasta", "--sample", "--chrom", "--line-width"))


def _hand_made(res: dict):
    """A povu_hip_vcf_cons filled by hand from the restatement's result; returns (the struct, what keeps its arrays alive)."""
    c, keep = H._VcfCons(), []
    types = {name: t for name, t in H._VcfCons._fields_}
    for name in K.ARRAYS:
        t = types[name]
        arr = np.ascontiguousarray(np.array([h[K.KEY.get(name, name)] for h in res["haps"]], dtype=np.dtype(t._type_)))
        keep.append(arr)
        setattr(c, name, arr.ctypes.data_as(t) if arr.size else t())
    text = np.frombuffer("".join(h["text"] for h in res["haps"]).encode() + b"\0", dtype=np.uint8).copy()
    keep.append(text)
    c.text = text.ctypes.data_as(C.POINTER(C.c_uint8))
    c.n_haps, c.n_text_bytes, c.n_unplaced, c.roundtrip = res["n_haps"], res["n_text_bytes"], res["n_unplaced"], int(res["roundtrip"])
    return c, keep


def test_the_text_writers_on_a_hand_made_result():
    lib = H.load_lib()
    named = [("s1#1#c", "ACGTACGTAC" * 13), ("s1#2#c", "ACGTTCGT"), ("gone", "ACGT")]
    names, ref = [n for n, _ in named], dict(named)
    rows = [("s1#1#c", 5, "r0", "A", "T,*", ["0|1", "2"]), ("gone", 1, "whole", "ACGT", "<DEL>", ["0", "1"]), ("gone", 1, "all", "ACGT", "A", ["0", "0"]),
            ("nowhere", 1, "r2", "A", "C", ["1|1", "1"])]
    text = K.vcf(["s1", "x"], rows)
    res, doc = K.ref_run(text, names, ref)
    gone = [h for h in res["haps"] if doc["chroms"][h["chrom"]] == "gone"][0]
    res["n_text_bytes"] -= gone["len"]
    for h in res["haps"][res["haps"].index(gone) + 1:]:
        h["off"] -= gone["len"]
    gone.update(text="", len=0)  # an empty haplotype
    assert res["n_unplaced"] == 1 and {h["len"] for h in res["haps"]} >= {0, 130}
    d = H.parse_vcf(text)
    c, keep = _hand_made(res)
    for width in (0, 1, 60):
        got = H.cons_texts(lib, C.byref(c), d._p, names, width)
        assert got == (CR.fasta_text(doc, res, width), CR.roundtrip_text(doc, res, names), CR.summary_text(res)), width
    fa = H.cons_texts(lib, C.byref(c), d._p, names, 60)[0].split("\n")
    assert fa[0] == ">s1#1#s1#1#c" and [len(x) for x in fa[1:4]] == [60, 60, 10] and ">s1#1#gone\n>x#0#gone\n" in "\n".join(fa)
    assert len(H.cons_texts(lib, C.byref(c), d._p, names, 1)[0].split("\n")) > 130
    assert H.cons_texts(lib, C.byref(c), d._p, names)[2].endswith("Unplaced records: 1\n")
    # what does not belong together gives no text
    for name, value in (("rt_status", 5), ("hap_chrom", 9), ("hap_col", 2), ("rt_path", 3), ("hap_off", 10 ** 6)):
        broken, keep2 = _hand_made(res)
        getattr(broken, name)[0] = value
        try:
            H.cons_texts(lib, C.byref(broken), d._p, names)
            assert False, name
        except RuntimeError as e:
            assert "do not belong together" in str(e)
    c.text = None  # without the text: no FASTA, the other two as before
    got = H.cons_texts(lib, C.byref(c), d._p, names)
    assert got[0] == "" and got[1:] == (CR.roundtrip_text(doc, res, names), CR.summary_text(res))
    none, ndoc = K.ref_run(K.HEAD + "s\n", names, ref)
    c0, _ = _hand_made(none)
    assert H.cons_texts(lib, C.byref(c0), H.parse_vcf(K.HEAD + "s\n")._p, names) == ("", CR.roundtrip_text(ndoc, none, names), CR.summary_text(none))


def test_the_python_surface():
    assert (H.C_ROUNDTRIP, H.C_NO_TEXT, H.C_TIME_WRITE, H.C_TILE_BYTES) == (1, 2, 8, 4096) and H.C_RT_NAMES == tuple(CR.RT_NAME)
    header = open(os.path.join(ROOT, "include", "povu_hip.h")).read()
    for k, v in (("POVU_HIP_C_ROUNDTRIP", "1u"), ("POVU_HIP_C_NO_TEXT", "2u"), ("POVU_HIP_C_TIME_WRITE", "8u"), ("POVU_HIP_C_TILE_BYTES", "4096u")):
        assert f"#define {k} {v}" in header
    assert callable(H.HipDecomposer.consensus) and hasattr(H.load_lib(), "povu_hip_vcf_consensus")
