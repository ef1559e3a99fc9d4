"""`povu call` argument handling, on the CPU: the reference options are exclusive (one of -r, -P, positional prefixes),
--restrict and --structure-export are refused, and `call` is this build's own (no outside provider).  On the GPU: one call over
the wide cohort (tests/cohort_cases.py) written as a GFA, for the host's names maker and the writer with 131 sample columns."""
import os
import subprocess

import pytest

import cohort_cases as CC
import vcf_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
XOR = "exactly one of the reference options"


def _run(*args):
    return subprocess.run([POVU, *args], capture_output=True, text=True, timeout=60)


def _fixture(golden_dir):
    return os.path.join(golden_dir, "gfa", "nested_deletion.gfa")


def test_reference_options_are_exclusive(golden_dir, tmp_path):
    gfa = _fixture(golden_dir)
    refs = tmp_path / "refs.txt"
    refs.write_text("HG1\n")
    for extra in ([], ["-P", "HG1", "-r", str(refs)], ["-P", "HG1", "HG2"], ["-r", str(refs), "HG1"]):
        r = _run("call", "-i", gfa, "-f", str(tmp_path), *extra)
        assert r.returncode == 1, extra
        assert XOR in r.stderr, (extra, r.stderr)
        assert "POVU_CALL_EXE" not in r.stderr and "not part of" not in r.stderr


def test_restrict_and_structure_export_refused(golden_dir, tmp_path):
    gfa = _fixture(golden_dir)
    for flag in (["--restrict", "HG1:1-10"], ["-g", "HG1:1-10"], ["--structure-export", str(tmp_path / "x.json")]):
        r = _run("call", "-i", gfa, "-f", str(tmp_path), "-P", "HG1", *flag)
        assert r.returncode == 1 and "not supported" in r.stderr, (flag, r.stderr)


def test_call_is_listed_in_help():
    r = _run("--help")
    assert r.returncode == 0
    assert "call OPTIONS" in r.stdout and "not part of the MI355X decompose build" not in r.stdout


@pytest.mark.gpu
def test_wide_cohort_through_the_cli(tmp_path):
    g, p = CC.wide_chain()
    seqs = CC.wide_gfa_sequences(g)
    gfa = tmp_path / "wide.gfa"
    gfa.write_text(g.to_gfa(seqs) + p.to_gfa())
    forest = tmp_path / "forest"
    forest.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", str(gfa), "-o", str(forest)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    refs = list(CC.REFS)
    r = subprocess.run([POVU, "call", "-i", str(gfa), "-f", str(forest), "-P", refs[0], "-P", refs[1]], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    names, steps = list(p.names), CC.steps_of(p)
    sq = dict(zip(g.vid.tolist(), seqs))
    pv = sorted(forest.glob("*.pvst"), key=lambda x: int(x.stem))
    recs = V.call(V.sites_of_pvst([x.read_text() for x in pv]), names, steps, sq, refs)
    assert len(recs) == 24 and len(V.slots_of(names)[0]) == 131
    header = next(ln for ln in r.stdout.splitlines() if ln.startswith("#CHROM")).split("\t")
    assert len(header) == 9 + 131 and [header[9 + s] for s in CC.BARE] == [f"bare{s}" for s in CC.BARE]
    assert r.stdout.split("\n", 2)[2] == V.vcf_text(names, steps, sq, recs, refs).split("\n", 2)[2]  # (behind the date line)
