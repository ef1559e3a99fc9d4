"""Which modes of a call combine, on the CPU: `modes_check` (the table of povu_amd/csrc/hip/call_modes.hpp under AddressSanitizer and
UBSan: all 2^7 * 5 requests, every exclusion from either mode of its pair, the wording of every rule pinned to literal strings);
the first refusal of either side for every one of the 640 requests against the recorded answers of tests/golden/call_modes.json,
which pins the order of each side where several rules apply; and `povu call` for every pair of mode flags and every (mode flag,
--profile): it is refused with the recorded text, or gets past its arguments and fails on a forest directory that does not exist,
before any GPU is opened."""
import os
import subprocess

import pytest

import call_modes_cases as MC

SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def _modes_check(*args):
    subprocess.check_call(["make", "-C", os.path.join(MC.ROOT, "povu_amd", "csrc"), "modes_check", "-s"])
    return subprocess.run([os.path.join(MC.ROOT, "build", "obj", "modes_check"), *args], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV),
                          timeout=120)


def test_modes_check_passes_under_the_sanitizers():
    p = _modes_check()
    assert p.returncode == 0 and p.stdout == "modes_check: ok\n" and not p.stderr, p.stderr


def test_both_sides_refuse_the_same_requests():
    """... and each with the recorded first refusal, for every one of the 640 requests"""
    p = _modes_check("--table")
    assert p.returncode == 0 and not p.stderr, p.stderr
    got = {}
    for ln in p.stdout.splitlines():
        bits, profile, lib, cli = ln.split("\t")
        got[int(bits), int(profile)] = (lib, cli)
    assert got == MC.golden()
    # both sides refuse the same requests, and neither a profile nor inversions alone is ever refused
    assert all(bool(lib) == bool(cli) for lib, cli in got.values()) and not any(lib for (bits, _), (lib, _) in got.items() if bits <= 1)


@pytest.mark.parametrize("modes,profile", MC.REQUESTS, ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_povu_call_answers_as_the_table_says(modes, profile):
    want = MC.expected(modes, profile)[1]
    assert MC.cli_answer(modes, profile) == want
    assert MC.cli_answer(tuple(reversed(modes)), profile) == want  # (the order of the flags does not matter)
    if want:  # it names a flag of the request, as the messages always have
        assert any(f"Flag '{MC.CLI[m][0]}'" in want for m in modes), want
