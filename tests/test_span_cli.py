"""`povu call --spanning-alleles` while the arguments are read (INTEGRATION.md "Spanning alleles"): refused by name without a
nested call and under the profiles that rewrite alleles, accepted with --nested, popped and top-level-only -- there the call
goes on to its inputs (a forest directory that does not exist ends it before any GPU is opened).  The VCF checks on a text
with a `*` ALT, through `vcfcheck_check` (the reader and the rules of `povu vcf --report` on the CPU, under the sanitizers):
clean when a sample carries the `*`, and a wrong walk on another ALT still fails for that ALT; the same program against the
Python restatement of the `*` rule (tests/span_vcfcheck_ref.py) on mutations of that text.  No GPU."""
import os
import subprocess

import pytest

import span_vcfcheck_ref as SR
import vcfcheck_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
FIXTURE = "downstream_repetitive/popped-parent-child-rescue"


def _call(golden_dir, tmp_path, *extra):
    gfa = os.path.join(golden_dir, "gfa", FIXTURE + ".gfa")
    return subprocess.run([POVU, "call", "-i", gfa, "-f", str(tmp_path / "no-such-forest"), "-P", "HG1", *extra], capture_output=True, text=True,
                          timeout=60)


@pytest.mark.parametrize("extra,word", [
    ((), "--nested"),
    (("--profile", "raw-graph"), "--nested"),
    (("--inversions",), "--nested"),
    (("--profile", "left-normalized"), "left-normalized"),
    (("--nested", "--profile", "left-normalized"), "left-normalized"),
    (("--profile=decomposed",), "decomposed"),
    (("--nested", "--profile", "decomposed"), "decomposed"),
])
def test_refused_by_name(golden_dir, tmp_path, extra, word):
    r = _call(golden_dir, tmp_path, "--spanning-alleles", *extra)
    assert r.returncode == 1 and "'--spanning-alleles'" in r.stderr and word in r.stderr, r.stderr
    assert "forest directory" not in r.stderr


@pytest.mark.parametrize("extra", [("--nested",), ("--profile", "popped", "--max-ref-length", "3"), ("--profile=top-level-only",),
                                   ("--nested", "--inversions"), ("--nested", "--region", "HG1#1#chr1:1-4")])
def test_gets_past_its_arguments(golden_dir, tmp_path, extra):
    r = _call(golden_dir, tmp_path, "--spanning-alleles", *extra)
    assert r.returncode == 1 and "cannot open the forest directory" in r.stderr and "--spanning-alleles" not in r.stderr, r.stderr


def test_what_nested_refuses_stays_refused_by_its_own_rule(golden_dir, tmp_path):
    for extra, word in ((("--nested", "--cluster", "0.9"), "--cluster"), (("--nested", "--off-reference"), "--off-reference"),
                        (("--nested", "--untangle"), "--untangle")):
        r = _call(golden_dir, tmp_path, "--spanning-alleles", *extra)
        assert r.returncode == 1 and word in r.stderr and "--spanning-alleles" not in r.stderr, r.stderr


def test_help_names_the_flag():
    r = subprocess.run([POVU, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert "--spanning-alleles" in r.stdout + r.stderr


# ---- `povu vcf --report` on a `*` ALT, on the CPU

HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tHG1\tHG2\tHG3\n"
# the fixture's paths as (sample column, phase, path words): word = id << 1 | '<'
PATHS = [(0, 0, [0, 2, 4, 6, 8, 10]), (1, 0, [0, 10]), (2, 0, [0, 2, 4, 12, 8, 10])]
# (HG3 walks >0>1>2>6>4: the plain call's third allele, left out here)
OUTER = "HG1#1#chr1\t1\t>0>5\tAAAAA\tA\t60\tPASS\tAC=1;AN=2;AT=>0>1>2>3>4,>0\tGT\t0\t1\t.\n"
INNER = "HG1#1#chr1\t4\t>2>4\tA\tG,*\t60\tPASS\tAC=1,1;AN=3;AT=>3,>6,*\tGT\t0\t2\t1\n"


@pytest.fixture(scope="module")
def vcfcheck_check():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "vcfcheck_check", "-s"])
    return os.path.join(ROOT, "build", "obj", "vcfcheck_check")


def _report(exe, text):
    block = f"report {len(PATHS)} {len(text.encode())}\n" + "".join(f"{c} {j} {' '.join(map(str, w))}\n" for c, j, w in PATHS) + text
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input=block.encode(), capture_output=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    lines = r.stdout.decode().split("\n")
    assert lines[-2:] == ["vcfcheck_check: ok", ""]
    return lines[:-2]


def test_report_is_clean_on_a_star_a_sample_carries(vcfcheck_check):
    assert _report(vcfcheck_check, HEAD + OUTER + INNER) == ["V 0 ok", "V 1 ok"]
    # the `*` entry of AT is no reason for no_at, neither where AT leaves it out; a sample on REF or on G is still searched
    assert _report(vcfcheck_check, HEAD + INNER.replace("AT=>3,>6,*", "AT=>3,>6")) == ["V 0 ok"]
    assert _report(vcfcheck_check, HEAD + INNER.replace("\t0\t2\t1\n", "\t2\t2\t2\n")) == ["V 0 ok"]


def test_a_wrong_walk_on_another_alt_still_fails_for_that_alt(vcfcheck_check):
    assert _report(vcfcheck_check, HEAD + OUTER + INNER.replace("AT=>3,>6,*", "AT=>3,>7,*")) == ["V 0 ok", "V 1 absent 1"]
    assert _report(vcfcheck_check, HEAD + INNER.replace("AT=>3,>6,*", "AT=>9,>6,*")) == ["V 0 absent 0"]
    # records without a `*` ALT check exactly as before: a missing walk is no_at, a `*` in AT alone stands for no walk
    assert _report(vcfcheck_check, HEAD + OUTER.replace("AT=>0>1>2>3>4,>0", "AT=>0>1>2>3>4")) == ["V 0 no_at 1"]
    assert _report(vcfcheck_check, HEAD + OUTER.replace("AT=>0>1>2>3>4,>0", "AT=>0>1>2>3>4,*")) == ["V 0 no_at 1"]
    # a bad step is still malformed
    assert _report(vcfcheck_check, HEAD + INNER.replace("AT=>3,>6,*", "AT=>3,>6,**"))[0].startswith("error ")


def test_report_equals_the_python_restatement(vcfcheck_check):
    names = ["HG1#1#chr1", "HG2#1#chr1", "HG3#1#chr1"]
    paths = [[(w >> 1, w & 1) for w in words] for _c, _j, words in PATHS]
    segments = set(range(16))  # (the program has no graph: every step it reads is a segment)
    texts = [HEAD + OUTER + INNER]
    for old, new in (("AT=>3,>6,*", "AT=>3,>6"), ("AT=>3,>6,*", "AT=>3,>7,*"), ("AT=>3,>6,*", "AT=>3,>6,>1"), ("AT=>3,>6,*", "AT=*,>6,*"),
                     ("\tG,*\t", "\tG,T\t"), ("\tG,*\t", "\t*,G\t"), ("\tA\tG,*\t", "\t*\tG,*\t"), ("\t0\t2\t1\n", "\t2|2\t2/0\t3\n"),
                     ("\t0\t2\t1\n", "\t.\t2\t2\n")):
        assert old in INNER
        texts.append(HEAD + OUTER + INNER.replace(old, new))
    for text in texts:
        doc = SR.parse(text)
        res = SR.check(doc, names, paths, segments)
        want = [f"V {r} ok" if not res["rec_invalid"][r] else f"V {r} {R.STATUS_NAME[res['rec_reason'][r]]} {res['rec_allele'][r]}"
                for r in range(len(doc["records"]))]
        assert _report(vcfcheck_check, text) == want, text
