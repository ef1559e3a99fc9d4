"""`povu call` argument handling, on the CPU: the reference options are exclusive (one of -r, -P, positional prefixes),
--restrict and --structure-export are refused, and `call` is this build's own (no outside provider)."""
import os
import subprocess

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
