"""The binary searches of the device code, on the CPU: `search_check` (povu_amd/csrc/hip/search_rules.hpp under AddressSanitizer and
UBSan) holds first_not and last_upto to std::partition_point on every 0/1-monotone predicate over ranges of length 0 to 65 with
both index types, lower_bound / upper_bound to the standard library's on arrays with runs of equal keys, the midpoint to ranges
that end at the top of the index type (where lo + hi wraps), and span_of and the keys of the component view to a linear scan over
offset tables with empty spans."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_search_check_passes_under_the_sanitizers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "search_check", "-s"])
    p = subprocess.run([os.path.join(ROOT, "build", "obj", "search_check")], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV), timeout=120)
    assert p.returncode == 0 and p.stdout == "search_check: ok\n" and not p.stderr, p.stderr
