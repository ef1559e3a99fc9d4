"""The votes of the merged primitives as the device casts them (povu_amd/csrc/hip/prim_merge.hpp), on the CPU: `merge_check`
runs the vote of one member over its slots under AddressSanitizer and UBSan, the bisection over another ALT's rows included, and
its answers are compared with merge_ref.member_vote, which looks at every row.  No GPU."""
import os
import random
import subprocess

import pytest

import merge_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = 0xFFFF


@pytest.fixture(scope="module")
def merge_check():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "merge_check", "-s"])
    return os.path.join(ROOT, "build", "obj", "merge_check")


def case(span, k, alts, slots, rule=True):
    """alts: per ALT None (kept whole) or its rows [(pos, ref_len, lead 0 / 1)], ascending; slots: the allele of every slot."""
    return span, k, alts, slots, rule


def expected(c):
    span, k, alts, slots, rule = c

    def pair_spans(other):
        rows = alts[other - 1] if other <= len(alts) else None  # (an allele the record does not have: no vote)
        return None if rows is None or not rule else [(p, p + n + ld - 1) for p, n, ld in rows]
    votes = [MR.member_vote(g, k, span, pair_spans) for g in slots]
    one = MR.VOTE_ALT in votes
    zero = MR.VOTE_REF in votes or MR.VOTE_REF_ELSEWHERE in votes
    return votes, (1 if one else 0 if zero else 255, int(one and zero),
                   int(not one and MR.VOTE_REF_ELSEWHERE in votes and MR.VOTE_REF not in votes))


def run(exe, cases):
    """What merge_check prints for the cases, parsed; the program must end clean under the sanitizers."""
    lines = []
    for (a, b), k, alts, slots, rule in cases:
        f = [a, b, k, int(rule), len(alts)]
        for rows in alts:
            f += ["P"] if rows is None else ["W", len(rows)] + [v for r in rows for v in r]
        f += [len(slots)] + [MISSING if g is None else g for g in slots]
        lines.append(" ".join(map(str, f)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    out = []
    for ln in p.stdout.splitlines():
        votes, tail = ln.split("|")
        out.append(([int(x) for x in votes.split()], tuple(int(x) for x in tail.split())))
    assert len(out) == len(cases)
    return out


def check(exe, cases):
    cases = list(cases)
    got = run(exe, cases)
    for c, g in zip(cases, got):
        assert g == expected(c), c
    return got


def test_hand_cases(merge_check):
    rows = [(5, 1, 0), (9, 3, 1)]  # an SNP at 5, a deletion with the span [9, 12]
    alts = [[(7, 1, 0)], rows, None]
    cases = [case((7, 7), 1, alts, [None, 0, 1, 2, 3]),  # '.', reference, this ALT, elsewhere, kept whole
             case((6, 8), 1, alts, [2]), case((6, 9), 1, alts, [2]), case((5, 5), 1, alts, [2]), case((4, 4), 1, alts, [2]),
             case((12, 12), 1, alts, [2]), case((13, 13), 1, alts, [2]), case((8, 8), 1, alts, [2]),  # one base short of the deletion
             case((7, 7), 1, alts, [0, 2, 2], rule=False),  # a row kept whole: the plain projection
             case((7, 7), 1, alts, [4, 65534]),  # no ALT of the record
             case((3, 3), 2, [[], [(3, 1, 0)]], [1, 0]),  # an ALT without rows touches nothing
             case((7, 7), 1, alts, [1, 0]), case((7, 7), 1, alts, [2, None]), case((7, 7), 1, alts, [2, 0])]
    got = check(merge_check, cases)
    assert got[0][0] == [0, 1, 2, 3, 0]
    assert [g[0][0] for g in got[1:8]] == [3, 0, 0, 3, 0, 3, 3]
    assert got[8][0] == [1, 0, 0] and got[9][0] == [0, 0] and got[10][0] == [3, 1]
    assert [g[1] for g in got[11:]] == [(1, 1, 0), (0, 0, 1), (0, 0, 0)]  # a conflict; 0 by the rule alone; 0 by a direct vote too


def random_cases(n, seed):
    rng = random.Random(seed)
    for _ in range(n):
        alts = []
        for _k in range(rng.randint(1, 5)):
            if rng.random() < .15:
                alts.append(None)
                continue
            rows, pos = [], rng.randint(1, 12)
            for _r in range(rng.choice((0, 1, 1, 2, 3, 8, 33))):
                lead = rng.randint(0, 1)
                length = rng.randint(1 - lead, 4)
                rows.append((pos, length, lead))
                pos += rng.randint(max(length + lead - 1, 0), length + lead + 3)  # the next row begins at this one's end or behind it
            alts.append(rows)
        a = rng.randint(1, 60)
        slots = [rng.choice([None, 0] + list(range(1, len(alts) + 2))) for _s in range(rng.randint(1, 9))]
        yield case((a, a + rng.choice((0, 0, 1, 3, 10))), rng.randint(1, len(alts)), alts, slots, rng.random() < .9)


def test_random_cases(merge_check):
    got = check(merge_check, random_cases(4000, 20261019))
    seen = {v for votes, _ in got for v in votes}
    assert seen == {0, 1, 2, 3}
    assert {t[0] for _, t in got} == {0, 1, 255} and any(t[1] for _, t in got) and any(t[2] for _, t in got)
