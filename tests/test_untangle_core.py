"""The lap alignment of the untangled calls as the device runs it (povu_amd/csrc/hip/untangle_rules.hpp), on the CPU:
`untangle_check` (povu_amd/csrc/host/untangle_check.cpp, built with -fsanitize=address,undefined) steps 64 lane states in
lockstep over the cases of tests/golden/untangle_align_cases.json -- every pair of the lengths 1, 2, 32, 33, 63 and 64 with
seeded symbols, the all-equal and the all-different extremes -- and prints the partners the restatement gives.  No GPU."""
import json
import os
import subprocess

import pytest

import untangle_cases as UC
import untangle_ref as U


@pytest.fixture(scope="module")
def untangle_check():
    subprocess.check_call(["make", "-C", os.path.join(UC.ROOT, "povu_amd", "csrc"), "untangle_check", "-s"])
    return os.path.join(UC.ROOT, "build", "obj", "untangle_check")


def run(exe, cases, tmp_path):
    """The program's lines for (a, b) cases; it must end clean under the sanitizers."""
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{len(a)} {len(b)} {' '.join(map(str, list(a) + list(b)))}\n" for a, b in cases))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "untangle_check: ok" and len(lines) == len(cases) + 1
    return lines[:-1]


def line_of(partner, extra):
    return " ".join("-" if x in (None, -1) else str(x) for x in partner) + f" | {extra}"


def test_the_golden_file_is_what_the_restatement_generates():
    stored = json.load(open(UC.ALIGN_CASES))
    assert stored["seed"] == UC.ALIGN_SEED and tuple(stored["lengths"]) == UC.ALIGN_LENGTHS
    assert stored["cases"] == UC.align_cases() and len(stored["cases"]) == 3 * 36
    assert {(len(c["a"]), len(c["b"])) for c in stored["cases"]} == {(n, m) for n in UC.ALIGN_LENGTHS for m in UC.ALIGN_LENGTHS}


def test_lockstep_lanes_give_the_stored_partners(untangle_check, tmp_path):
    cases = json.load(open(UC.ALIGN_CASES))["cases"]
    got = run(untangle_check, [(c["a"], c["b"]) for c in cases], tmp_path)
    for c, ln in zip(cases, got):
        assert ln.strip() == line_of(c["partner"], c["extra"]), (len(c["a"]), len(c["b"]))
        assert sum(x < 0 for x in c["partner"]) + c["extra"] <= c["cost"]
    # the last lane and both code words are used: 64 x 64 with a partner in column 63 and in a row past 32
    full = next(c for c in cases if len(c["a"]) == 64 and len(c["b"]) == 64)
    assert 63 in full["partner"] and any(x >= 0 for x in full["partner"][32:])


def test_the_tie_cases_and_the_example(untangle_check, tmp_path):
    cases = [([0], [1, 2]), ([0], [0, 2]), ([0, 1, 0], [1]), ([0, 1, 0], [0, 0]), ([0, 1, 0], [1, 1, 0, 0]), ([65534], [65534]), ([5], [6])]
    got = run(untangle_check, cases, tmp_path)
    assert [ln.strip() for ln in got] == ["1 | 1", "0 | 1", "- 0 - | 0", "0 - 1 | 0", "0 1 3 | 1", "0 | 0", "0 | 0"]
    assert [ln.strip() for ln in got] == [line_of(*U.align(a, b)[:2]) for a, b in cases]
