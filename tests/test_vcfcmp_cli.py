"""`povu vcf --compare` (INTEGRATION.md "VCF comparison"): compare.tsv and summary.txt equal the library's texts and the
restatement's (tests/vcfcmp_ref.py), the exit status is 0 whatever the comparison finds, -i is accepted and not read; the flags
that do not go together are refused by name."""
import os
import subprocess

import pytest

import vcfcmp_cases as K
import vcfcmp_ref as M

POVU = os.path.join(K.ROOT, "povu_amd", "bin", "povu")
FIXTURE = "vcfwave-complex-decomposition"


def _run(*args):
    return subprocess.run([POVU] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.gpu
def test_both_files_equal_the_librarys_texts(tmp_path):
    from povu_amd import HipDecomposer
    a, b = os.path.join(K.GOLDEN, FIXTURE, "raw_graph.vcf"), os.path.join(K.GOLDEN, FIXTURE, "decomposed.vcf")
    ta, tb = open(a).read(), open(b).read()
    da, db = M.parse(ta), M.parse(tb)
    want = M.compare(da, db)
    d = HipDecomposer(0)
    try:
        c = d.compare_vcfs(ta, tb)
        lib = c.compare_text(), c.summary_text()
    finally:
        d.close()
    assert lib == (M.compare_text(da, db, want), M.summary_text(want)) and want["n_only_b"] == 2
    out = tmp_path / "out"
    r = _run("-t", "4", "vcf", "-c", a, "-d", b, "--compare", "-o", out)  # differences found: still 0
    assert r.returncode == 0, r.stderr
    assert ((out / "compare.tsv").read_text(), (out / "summary.txt").read_text()) == lib
    # -i is accepted and not read; the long flags; a file against itself
    out2 = tmp_path / "out2"
    r = _run("vcf", "-i", tmp_path / "nothing.gfa", "--vcf=" + a, "--other-input-vcf=" + a, "--compare", "--output-dir=" + str(out2))
    assert r.returncode == 0, r.stderr
    assert (out2 / "compare.tsv").read_text() == "side\tCHROM\tPOS\tREF\tALT\trec_idx\tID\tn\n"
    assert (out2 / "summary.txt").read_text().startswith("Alleles: shared 2, only A 0, only B 0\nAlleles: precision 1.0000, recall 1.0000, F1 1.0000\n")
    # a VCF that cannot be read: the comparison did not run
    r = _run("vcf", "-c", a, "-d", tmp_path / "nothing.vcf", "--compare", "-o", tmp_path / "no")
    assert r.returncode == 1 and "cannot read the VCF" in r.stderr and not (tmp_path / "no").exists()
    broken = tmp_path / "broken.vcf"
    broken.write_text(tb.replace("\tGT\t", "\tGT\tx\t", 1))
    r = _run("vcf", "-c", a, "-d", broken, "--compare", "-o", tmp_path / "no")
    assert r.returncode == 1 and "broken.vcf: line " in r.stderr and not (tmp_path / "no").exists()


def test_flags_that_do_not_go_together_are_refused_by_name(tmp_path):
    vcf = tmp_path / "v.vcf"
    vcf.write_text(K.COLUMNS + "\n")
    gfa = tmp_path / "g.gfa"
    gfa.write_text("S\t1\tA\n")
    r = _run("vcf", "-i", gfa, "-c", vcf, "-d", vcf, "--compare", "--report")
    assert r.returncode == 1 and "--compare" in r.stderr and "--report" in r.stderr and "exclude" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", vcf, "-d", vcf, "--report")
    assert r.returncode == 1 and "'-d'" in r.stderr and "--compare" in r.stderr
    r = _run("vcf", "-c", vcf, "--compare")
    assert r.returncode == 1 and "--compare" in r.stderr and "-d <vcf>" in r.stderr
    r = _run("vcf", "-d", vcf, "--compare")
    assert r.returncode == 1 and "'vcf' is required" in r.stderr
    r = _run("vcf", "-c", vcf, "-d", vcf, "--compare", "--spelling")
    assert r.returncode == 1 and "--spelling" in r.stderr
    # with neither flag the message of before, word for word; without --compare -i is still asked for
    r = _run("vcf", "-i", gfa, "-c", vcf)
    assert r.returncode == 1 and "vcf needs --report (the interactive --tui is not provided by this build)" in r.stderr
    r = _run("vcf", "-c", vcf, "--report")
    assert r.returncode == 1 and "'gfa' is required" in r.stderr
    help_text = _run("--help").stdout
    assert "--compare" in help_text and "--other-input-vcf" in help_text
