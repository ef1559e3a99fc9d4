"""`povu vcf --report` (INTEGRATION.md "VCF checks"): a called VCF checks clean, a mutated one gives the report and the error
rate the restatement (tests/vcfcheck_ref.py) predicts; --tui and a missing -i or -c are refused."""
import os
import subprocess

import pytest

import vcfcheck_ref as R
from povu_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")


def _run(*args):
    return subprocess.run([POVU] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.gpu
def test_report_of_a_called_and_of_a_mutated_vcf(tmp_path):
    g = W.chain_of_bubbles(40)
    p = W.pansn(W.chain_haplotypes(40, 8, seed=9), samples=4)
    seqs = W.random_sequences(g, 9, max_len=12, empty=0.0)  # (a GFA S line needs a sequence)
    gfa = tmp_path / "g.gfa"
    gfa.write_text(g.to_gfa(seqs) + p.to_gfa())
    forest = tmp_path / "forest"
    forest.mkdir()
    assert _run("decompose", "-i", gfa, "-o", forest).returncode == 0
    r = _run("call", "-i", gfa, "-f", forest, "-P", "sample0#1", "--inversions")
    assert r.returncode == 0, r.stderr
    names, steps = list(p.names), [p.steps(k) for k in range(len(p))]
    sq = dict(zip(g.vid.tolist(), seqs))
    vcf = tmp_path / "calls.vcf"
    vcf.write_text(r.stdout)
    out = tmp_path / "clean"
    r = _run("-t", "4", "vcf", "-i", gfa, "-c", vcf, "--report", "--spelling", "-o", out)
    assert r.returncode == 0, r.stderr
    doc = R.parse(vcf.read_text())
    assert len(doc["records"]) > 10
    assert (out / "summary.txt").read_text() == "No errors\n"
    assert (out / "report.tsv").read_text() == "rec_idx\tID\tPOS\tAT\tHap ID\tsample\treason\n"
    # every third record loses a step of its REF walk, every seventh its last REF base; the exit status stays 0
    lines, k = vcf.read_text().split("\n"), 0
    for i, ln in enumerate(lines):
        if ln and not ln.startswith("#"):
            f = ln.split("\t")
            if k % 3 == 0:
                f[7] = f[7].replace("AT=>", "AT=>999999>", 1)
            if k % 7 == 0:
                f[3] = f[3][:-1] + ("A" if f[3][-1] != "A" else "C")
            lines[i] = "\t".join(f)
            k += 1
    bad = tmp_path / "bad.vcf"
    bad.write_text("\n".join(lines))
    for flags in ([], ["--spelling"], ["--forward-only"]):
        out = tmp_path / ("bad" + "".join(flags))
        r = _run("vcf", "-i", gfa, "--vcf=" + str(bad), "--report", "-o", out, *flags)
        assert r.returncode == 0, r.stderr
        doc = R.parse(bad.read_text())
        res = R.check(doc, names, steps, sq.keys(), sq, spelling="--spelling" in flags, forward_only="--forward-only" in flags)
        assert sum(res["rec_invalid"]) >= len(doc["records"]) // 3
        assert (out / "report.tsv").read_text() == R.report_text(doc, res, names)
        assert (out / "summary.txt").read_text() == R.summary_text(doc, res) != "No errors\n"
    # a VCF that cannot be read, a GFA that cannot be read: the check did not run
    broken = tmp_path / "broken.vcf"
    broken.write_text(vcf.read_text().replace("\tGT\t", "\tGT\tx\t", 1))
    r = _run("vcf", "-i", gfa, "-c", broken, "--report", "-o", tmp_path / "no")
    assert r.returncode == 1 and "line " in r.stderr and "sample columns" in r.stderr
    r = _run("vcf", "-i", tmp_path / "nothing.gfa", "-c", vcf, "--report", "-o", tmp_path / "no")
    assert r.returncode == 1 and not (tmp_path / "no").exists()


def test_tui_and_missing_files_are_refused(tmp_path):
    gfa = tmp_path / "g.gfa"
    gfa.write_text(W.chain_of_bubbles(2).to_gfa())
    vcf = tmp_path / "v.vcf"
    vcf.write_text("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    r = _run("vcf", "-i", gfa, "-c", vcf, "--tui")
    assert r.returncode == 1 and "--report" in r.stderr and "--tui" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", vcf)
    assert r.returncode == 1 and "--report" in r.stderr
    r = _run("vcf", "-c", vcf, "--report")
    assert r.returncode == 1 and "'gfa' is required" in r.stderr
    r = _run("vcf", "-i", gfa, "--report")
    assert r.returncode == 1 and "'vcf' is required" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", tmp_path / "nothing.vcf", "--report")
    assert r.returncode == 1 and "cannot read the VCF" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", vcf, "--report", "--fast")
    assert r.returncode == 1 and "--fast" in r.stderr
    assert "vcf" in _run("--help").stdout
