"""The search of a walks query as the device runs it (povu_amd/csrc/hip/walk_rules.hpp), on the CPU: `walk_check` (under
AddressSanitizer and UBSan) holds the path set of tier 2 to std::set on tables of 16, 32 and 2048 slots -- probes and backward shifts
across the wrap, entries that must move and entries that must stay, a lane's own words of a strided scratch -- and dfs on both
stacks to a recursive enumeration on random bidirected multigraphs with caps around every branch, the hand-over flag of tier 1,
emit buffers of the exact size and a path set left empty after every search."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_walk_check_passes_under_the_sanitizers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "walk_check", "-s"])
    p = subprocess.run([os.path.join(ROOT, "build", "obj", "walk_check")], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV), timeout=120)
    assert p.returncode == 0 and p.stdout == "walk_check: ok\n" and not p.stderr, p.stderr
