"""The aligner of the `decomposed` profile as the device runs it (povu_amd/csrc/hip/prim_align.hpp), on the CPU: `prim_check`
emulates one wave as 64 lane states stepped in lockstep, both tiers, under AddressSanitizer and UBSan, and its rows and cell
counts are compared with prim_ref.pair_rows, exactly.  No GPU."""
import os
import random
import subprocess

import pytest

import prim_ref as PR
from prim_cases import edited
from test_prim_ref import random_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513)


@pytest.fixture(scope="module")
def prim_check():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "prim_check", "-s"])
    return os.path.join(ROOT, "build", "obj", "prim_check")


def case(ref, alt, pos=7, base="G", cap=PR.MAX_LENGTH, one_alt=False):
    return ref, alt, pos, base if pos > 1 else "", cap, one_alt


def expected(c, force_tier2):
    """(cells, tier, rows) of a case by the restatement; tier 0: not aligned."""
    ref, alt, pos, base, cap, one_alt = c
    rows, cells = PR.pair_rows(ref, alt, pos, "N" * (pos - 2) + base, cap)
    tier = 0 if not cells else 2 if force_tier2 or max(len(ref), len(alt)) > 64 else 1
    # the rule of prim_ref.decompose for a record with one ALT
    if one_alt and len(rows) == 1 and rows[0]["kind"] != PR.ROW_PASS and (rows[0]["pos"],) + PR.row_texts(rows[0], ref, alt) == (pos, ref, alt):
        rows = [dict(rows[0], kind=PR.ROW_RAW, index=0)]
    return cells, tier, [(r["kind"], r["reason"], r["index"], r["pos"], r["ref_start"], r["ref_len"], r["alt_start"], r["alt_len"], r["lead"])
                         for r in rows]


def run(exe, cases, force_tier2=False):
    """What prim_check prints for the cases, parsed; the program must end clean under the sanitizers."""
    text = "".join(f"{ref or '.'} {alt or '.'} {pos} {base or '.'} {cap} {int(one_alt)}\n" for ref, alt, pos, base, cap, one_alt in cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe] + (["--force-tier2"] if force_tier2 else []), input=text, capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    out, lines, at = [], p.stdout.splitlines(), 0
    while at < len(lines):
        head = lines[at].split()
        assert head[0] == "pair"
        cells, tier, n = int(head[1]), int(head[2]), int(head[3])
        rows = []
        for f in (x.split() for x in lines[at + 1:at + 1 + n]):
            rows.append(tuple(int(x) for x in f[:8]) + ("" if f[8] == "." else f[8],))
        out.append((cells, tier, rows))
        at += 1 + n
    assert len(out) == len(cases)
    return out


def check(exe, cases, force_tier2=False):
    cases = list(cases)
    got = run(exe, cases, force_tier2)
    for c, g in zip(cases, got):
        assert g == expected(c, force_tier2), (c[0][:80], c[1][:80], c[2:], force_tier2)
    return got


HAND = [("CGT", "TGA"), ("CGT", "CGTACGTACGTA"), ("GAA", "G"), ("GAA", "GA"), ("AA", "A"), ("AC", "CA"), ("acgt", "ACGT"), ("", "AC"), ("AC", "")]


def small_cases():
    yield from (case(a, b) for a, b in HAND)
    yield from (case(a, b, pos=2 + k % 5, base="ACGTn"[k % 5]) for k, (a, b) in enumerate(random_pairs(4000, 20261018)))
    yield from (case(a, b) for a, b in random_pairs(300, 11, max_len=80))


def test_hand_alignments_and_random_pairs(prim_check):
    got = check(prim_check, small_cases())
    tiers = [t for _c, t, _r in got]
    kinds = {k for _c, _t, rows in got for k, *_ in rows}
    assert tiers.count(1) > 3000 and tiers.count(2) > 50 and {PR.ROW_SNP, PR.ROW_INS, PR.ROW_DEL, PR.ROW_PASS} <= kinds
    assert any(r[0] != PR.ROW_SNP and r[4] == 0 and r[8] for _c, _t, rows in got for r in rows)  # an indel at offset 0, anchored on the context


def test_every_small_case_with_tier_2_forced(prim_check):
    got = check(prim_check, small_cases(), force_tier2=True)
    assert all(t in (0, 2) for _c, t, _r in got)


def related(rng, n, m):
    """A random text of n bases and one of m bases: a copy (cut, or continued with itself) with three edits (substitutions,
    insertions and deletions of one or two bases, prim_cases.edited), brought back to m bases at its end."""
    a = "".join(rng.choice("ACGT") for _ in range(n))
    b = ((a or "A") * (m // max(n, 1) + 2))[:m + 8]
    return a, edited(b, rng)[:m] if m else ""


def test_lengths_around_the_stripes_and_the_cap(prim_check):
    rng = random.Random(5)
    cases = [case(*related(rng, n, m)) for n in LENGTHS for m in LENGTHS]
    # all-A against all-A one shorter (and one longer): the leftmost gap, along a whole stripe boundary
    cases += [case("A" * n, "A" * (n - 1)) for n in LENGTHS if n] + [case("A" * (n - 1), "A" * n) for n in LENGTHS if n]
    cases += [case("A" * n, "A" * (n - 1), pos=1) for n in (2, 65, 512)]
    got = check(prim_check, cases)
    assert sum(rows[0][1] == PR.REASON_MAX_ALLELE_LENGTH for _c, _t, rows in got) >= 20
    assert max(c for c, _t, _r in got) == 513 * 513


def test_contig_start_lower_case_and_caps(prim_check):
    cases = [case("AA", "A", pos=1), case("A", "TTA", pos=1), case("A", "C", pos=1), case("AC", "A", pos=1), case("TA", "A", pos=1)]
    cases += [case(a.lower(), b) for a, b in random_pairs(300, 3)] + [case(a, b.lower(), pos=1) for a, b in random_pairs(300, 4)]
    for cap in (1, 8, 64, 512):
        cases += [case(a, b, cap=cap) for a, b in random_pairs(200, cap, max_len=70 if cap == 64 else 12)]
    got = check(prim_check, cases)
    reasons = {rows[0][1] for _c, _t, rows in got}
    assert {PR.REASON_CONTIG_START, PR.REASON_EQUALS_REF, PR.REASON_EMPTY_ALLELE, PR.REASON_MAX_ALLELE_LENGTH} <= reasons
    check(prim_check, cases, force_tier2=True)


def test_the_one_row_of_a_one_alt_record(prim_check):
    """The records of test_prim_ref.test_unchanged_record_is_the_raw_line, and what must not turn _ROW_RAW."""
    cases = [case("A", "C", 3, "C", one_alt=True), case("GAA", "G", 6, "A", one_alt=True), case("G", "GTT", 11, "C", one_alt=True),
             case("GA", "gT", 15, "C", one_alt=True), case("gA", "G", 20, "T", one_alt=True), case("AA", "A", 5, "C", one_alt=True),
             case("CGT", "TGA", 5, "C", one_alt=True), case("A", "C", 3, "C", one_alt=False)]
    got = check(prim_check, cases)
    assert [rows[0][0] for _c, _t, rows in got] == [PR.ROW_RAW, PR.ROW_RAW, PR.ROW_RAW, PR.ROW_SNP, PR.ROW_DEL, PR.ROW_DEL, PR.ROW_SNP, PR.ROW_SNP]
    check(prim_check, cases, force_tier2=True)
