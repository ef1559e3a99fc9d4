"""The clustered calls at the command line: `cluster_check` (the rules of povu_amd/csrc/hip/cluster_rules.hpp under AddressSanitizer
and UBSan: parser, 128-bit comparisons, weight bound, leader loop), povu_hip_cluster_parse through the library, the argument
handling of `povu call --cluster`, which fails before any GPU is opened, and -- on the GPU -- `povu call` and `povu gfa2vcf` end to
end on the worked example."""
import ctypes as C
import json
import os
import subprocess

import pytest

import cluster_cases as CC
import cluster_ref as CR
from povu_amd import hip as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
# refused text -> a word of its own message
REFUSED = {"0": "above 0", "1.0000001": "six decimals", "1.5": "at most 1", "-0.5": "decimal number", ".": "decimal number",
           "0.5x": "decimal number", "0.1234567": "six decimals"}
# what a clustered call is refused with -> the flag its message names beside --cluster
COMBINATIONS = {("--nested",): "--nested", ("--profile", "top-level-only"): "top-level-only", ("--profile=popped",): "popped",
                ("--profile", "left-normalized"): "left-normalized", ("--profile", "decomposed"): "decomposed",
                ("--profile", "decomposed", "--merge-primitives"): "decomposed", ("--off-reference",): "--off-reference",
                ("--untangle",): "--untangle", ("--gpus", "2"): "--gpus", ("--gpus=2",): "--gpus"}


def test_cluster_check_passes_under_the_sanitizers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "cluster_check", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(ROOT, "build", "obj", "cluster_check")], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout == "cluster_check: ok\n" and not p.stderr, p.stderr


def _run(*args, **kw):
    return subprocess.run([POVU, *args], capture_output=True, text=True, timeout=120, **kw)


@pytest.mark.parametrize("text", sorted(REFUSED))
def test_a_refused_threshold_has_a_message_of_its_own(tmp_path, text):
    for flag in (["--cluster", text], ["--cluster=" + text]):
        r = _run("call", "-i", CC.GFA, "-f", str(tmp_path), "-P", "HG1", *flag)
        assert r.returncode == 1 and "--cluster" in r.stderr and f"'{text}'" in r.stderr and REFUSED[text] in r.stderr, (flag, r.stderr)
    with pytest.raises(CR.ClusterError, match=REFUSED[text]):  # the restatement reads it the same way
        CR.parse(text)


@pytest.mark.parametrize("with_", sorted(COMBINATIONS))
def test_the_refused_combinations_name_the_flag(tmp_path, with_):
    for args in (["--cluster", "0.9", *with_], [*with_, "--cluster=0.9"]):
        r = _run("call", "-i", CC.GFA, "-f", str(tmp_path), "-P", "HG1", *args)
        assert r.returncode == 1 and "'--cluster'" in r.stderr and COMBINATIONS[with_] in r.stderr, (args, r.stderr)


def test_cluster_needs_its_argument_and_gpus_stays_unknown_without_it(tmp_path):
    r = _run("call", "-i", CC.GFA, "-f", str(tmp_path), "-P", "HG1", "--cluster")
    assert r.returncode == 1 and "requires an argument" in r.stderr
    r = _run("call", "-i", CC.GFA, "-f", str(tmp_path), "-P", "HG1", "--gpus", "2")
    assert r.returncode == 1 and "Flag could not be matched: --gpus" in r.stderr


def test_help_states_the_threshold():
    out = _run("--help").stdout.splitlines()
    line = next(k for k, ln in enumerate(out) if "--cluster=" in ln)
    text = " ".join(out[line:line + 4])
    assert "0 < F <= 1" in text and "six decimals" in text and "NX" in text and "MINSIM" in text and "Clustered" in text


def test_cluster_parse_through_the_library():
    lib = H.load_lib()

    def parse(text):
        ppm, err = C.c_uint32(7), C.create_string_buffer(512)
        rc = lib.povu_hip_cluster_parse(text.encode(), C.byref(ppm), err, 512)
        return (rc, ppm.value) if rc == 0 else (rc, err.value.decode())
    for text in ("1", "1.0", "0.6", "0.600001", "0.000001", ".5", "1.", "0.95"):
        assert parse(text) == (0, CR.parse(text)), text
    for text, word in REFUSED.items():
        rc, msg = parse(text)
        assert rc == 1 and word in msg and f"'{text}'" in msg, (text, msg)
    assert hasattr(H, "CLUSTER_COUNTERS") and H.CLUSTER_NO_BOUND == 1


@pytest.mark.gpu
def test_the_command_line_end_to_end(tmp_path):
    forest = tmp_path / "forest"
    forest.mkdir()
    r = _run("decompose", "-i", CC.GFA, "-o", str(forest))
    assert r.returncode == 0, r.stderr
    golden = json.load(open(CC.GOLDEN))
    env = dict(os.environ, POVU_CALL_EXE=POVU)
    plain = _run("call", "-i", CC.GFA, "-f", str(forest), "-P", "HG1", "--stdout").stdout.splitlines()
    for f in ("0.6", "0.600001"):
        for cmd in (["call", "-i", CC.GFA, "-f", str(forest), "-P", "HG1", "--stdout", "--cluster", f],
                    ["call", "-i", CC.GFA, "-f", str(forest), "-P", "HG1", "--stdout", "--cluster=" + f],
                    ["gfa2vcf", "-i", CC.GFA, "-P", "HG1", "--stdout", "--cluster", f]):
            r = _run(*cmd, env=env)
            assert r.returncode == 0, r.stderr
            out = r.stdout.splitlines()
            assert [ln for ln in out if not ln.startswith("#")] == golden[f]["records"], cmd
            assert [ln for ln in out if ln.startswith("#") and ln not in plain] == golden[f]["header"], cmd
            assert [ln for ln in out if ln.startswith("#") and ln not in golden[f]["header"]] == [ln for ln in plain if ln.startswith("#")]
    # with --inversions and --region it composes; the files of -o carry the lines too
    r = _run("call", "-i", CC.GFA, "-f", str(forest), "-P", "HG1", "--cluster", "0.6", "--inversions", "--region", "HG1#1#chr1:1-2")
    assert r.returncode == 0 and [ln for ln in r.stdout.splitlines() if not ln.startswith("#")] == golden["0.6"]["records"][:1], r.stderr
    out_dir = tmp_path / "vcf"
    r = _run("call", "-i", CC.GFA, "-f", str(forest), "-P", "HG1", "-o", str(out_dir), "--cluster", "0.6")
    assert r.returncode == 0, r.stderr
    text = (out_dir / "HG1.vcf").read_text().splitlines()
    assert "##povu_call_cluster=0.600000" in text and [ln for ln in text if not ln.startswith("#")] == golden["0.6"]["records"]
