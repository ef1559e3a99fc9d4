"""The region calls on the CPU: `region_check` (the rules of povu_amd/csrc/hip/region_rules.hpp under AddressSanitizer and
UBSan: parser, step predicate, merged intervals and their search), povu_hip_region_parse through the library, and the argument
handling of `povu call --region`, which fails before any GPU is opened.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

import region_ref as R
from povu_amd import hip as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
# malformed text -> a word of its own message
MALFORMED = {"HG1": "no ':'", ":1-10": "empty path name", "HG1:110": "no '-'", "HG1:1x-10": "start '1x'", "HG1:1-1o": "end '1o'",
             "HG1:5-5": "below the end", "HG1:9-3": "below the end", "HG1:1-1000000000000000000": "18 digits"}


def test_region_check_passes_under_the_sanitizers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "region_check", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(ROOT, "build", "obj", "region_check")], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout == "region_check: ok\n" and not p.stderr, p.stderr


def _run(*args):
    return subprocess.run([POVU, *args], capture_output=True, text=True, timeout=60)


def _gfa(golden_dir):
    return os.path.join(golden_dir, "gfa", "nested_deletion.gfa")


@pytest.mark.parametrize("text", sorted(MALFORMED))
def test_a_malformed_region_has_a_message_of_its_own(golden_dir, tmp_path, text):
    for flag in (["--region", text], ["--region=" + text]):
        r = _run("call", "-i", _gfa(golden_dir), "-f", str(tmp_path), "-P", "HG1", *flag)
        assert r.returncode == 1 and "--region" in r.stderr and f"'{text}'" in r.stderr and MALFORMED[text] in r.stderr, (flag, r.stderr)
    with pytest.raises(R.RegionError):  # the restatement reads it the same way
        R.parse(text)


def test_region_needs_its_argument_and_refuses_off_reference(golden_dir, tmp_path):
    r = _run("call", "-i", _gfa(golden_dir), "-f", str(tmp_path), "-P", "HG1", "--region")
    assert r.returncode == 1 and "requires an argument" in r.stderr
    r = _run("call", "-i", _gfa(golden_dir), "-f", str(tmp_path), "-P", "HG1", "--region", "HG1#1#chr1:1-10", "--off-reference")
    assert r.returncode == 1 and "--region" in r.stderr and "--off-reference" in r.stderr, r.stderr


def test_restrict_stays_refused_and_names_region(golden_dir, tmp_path):
    for flag in (["--restrict", "HG1:1-10"], ["-g", "HG1:1-10"], ["--restrict=HG1:1-10"]):
        r = _run("call", "-i", _gfa(golden_dir), "-f", str(tmp_path), "-P", "HG1", *flag)
        assert r.returncode == 1 and "not supported" in r.stderr and "--region" in r.stderr, (flag, r.stderr)


def test_help_states_the_half_open_interval():
    r = _run("--help")
    line = next(k for k, ln in enumerate(r.stdout.splitlines()) if "--region=" in ln)
    text = " ".join(r.stdout.splitlines()[line:line + 4])
    assert "1-based start" in text and "exclusive end" in text and "[start, end)" in text


def test_region_parse_through_the_library():
    lib = H.load_lib()
    names = ["HG1#1#chr1", "a:b", "HG1#1#chr1:x"]
    arr = (C.c_char_p * 3)(*[n.encode() for n in names])

    def parse(text):
        out, err = H._Region(), C.create_string_buffer(512)
        rc = lib.povu_hip_region_parse(text.encode(), 3, arr, C.byref(out), err, 512)
        return (rc, (out.path, out.start, out.end)) if rc == 0 else (rc, err.value.decode())
    assert parse("HG1#1#chr1:3-4") == (0, (0, 3, 4))
    assert parse("a:b:10-20") == (0, (1, 10, 20))  # the last ':'
    assert parse("HG1#1#chr1:x:1-999999999999999999") == (0, (2, 1, 999999999999999999))
    rc, msg = parse("HG1:3-4")  # exact names, no prefixes
    assert rc == 1 and "no path is named HG1" in msg and "'HG1:3-4'" in msg
    for text, word in MALFORMED.items():
        rc, msg = parse(text)
        assert rc == 1 and word in msg and f"'{text}'" in msg, (text, msg)
    assert [R.parse(t) for t in ("HG1#1#chr1:3-4", "a:b:10-20")] == [("HG1#1#chr1", 3, 4), ("a:b", 10, 20)]
