"""GPU haplotype comparison (povu_hip_vcf_haplotypes, HipDecomposer.compare_haplotypes) against the plain-Python restatement
(tests/vcfhap_ref.py), array for array and text for text, every case again with the forced second tier (equal but for n_tier2):
the golden pairs in both modes against tests/golden/vcfhap_expected.json; trims and haplotype lengths on the edges of a ballot's
64 bytes and of the tiers; 0 to 130 edits in a cell, conflicts, duplicates; reaches of every length around 64 and around the
cap, at both ends of a path; windows that touch, nest, chain, interleave; both window verdicts; unplaced records; ploidies,
phases, columns; unspelled entries; every run colliding (POVU_HIP_TRAV_HASH_BITS); empty inputs; a context without a graph; the
arenas; the refusals; this project's own calls, raw against the rewriting profiles."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import vcfhap_cases as K
import vcfhap_ref as HR
from povu_amd import HipDecomposer
from povu_amd import hip as H

pytestmark = pytest.mark.gpu
ROOT = K.ROOT
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
LENGTHS = (1, 31, 32, 33, 63, 64, 65, 128, 200)


@pytest.fixture(scope="module")
def hip():
    """A context that never sees a graph: the REF-field mode needs none."""
    d = HipDecomposer(0)
    yield d
    d.close()


@pytest.fixture()
def ctx():
    d = HipDecomposer(0)
    yield d
    d.close()


def statuses(c):
    return [HR.STATUS_NAME[s] for s in c.cell_status.tolist()]


# ---- the golden pairs

@pytest.mark.parametrize("fixture", sorted(K.K.GOLDEN_FILES))
def test_golden_pairs_in_both_modes(hip, ctx, fixture):
    want = K.expected()
    reference = K.upload_gfa(ctx, fixture)
    assert reference == K.gfa_reference(fixture)
    names = K.K.GOLDEN_FILES[fixture]
    for name in names[1:]:
        for ref in (False, True):
            a, b = K.golden(fixture, names[0]), K.golden(fixture, name)
            got, _ = K.both_tiers(ctx if ref else hip, a, b, reference if ref else None)
            assert json.loads(json.dumps(K.digest(got))) == want[K.pair_key(fixture, names[0], name, ref)]
    for name in names:  # a document against itself: every called cell is equal
        text = K.golden(fixture, name)
        got, _ = K.both_tiers(hip, text, text)
        assert set(got.cell_status.tolist()) <= {H.H_EQUAL_REF, H.H_EQUAL} and got.n_cells > 0


def test_the_pins_of_the_definition(hip, ctx):
    fx = "vcfwave-complex-decomposition"
    got, _ = K.both_tiers(hip, K.golden(fx, "raw_graph"), K.golden(fx, "decomposed"))
    assert (got.win_lo.tolist(), got.win_hi.tolist()) == ([9], [13]) and statuses(got) == ["equal_ref", "equal", "equal"]
    assert got.cell_len_a.tolist() == [4, 4, 16]
    fx = "popped-parent-child-rescue"
    reference = K.upload_gfa(ctx, fx)
    got, _ = K.both_tiers(ctx, K.golden(fx, "raw_graph"), K.golden(fx, "top_level_only"), reference)
    assert statuses(got) == ["equal_ref", "equal", "differ"] and got.cell_len_a.tolist() == [5, 1, 5] and int(got.cell_first_diff[2]) == 2


# ---- trims and haplotype lengths

def test_trims_and_haplotype_lengths_on_the_edges(hip):
    rng = np.random.default_rng(5)
    rows_a, rows_b, pos = [], [], 1
    for n in LENGTHS:
        core = K.bases(rng, n)
        flip = lambda t, k: t[:k] + K.other(t[k]) + t[k + 1:]  # noqa: E731
        cases = [(core, flip(core, 0), core, flip(core, 0).lower()),                 # the same SNV in the first byte
                 (core, flip(core, n - 1), core, flip(core, n - 1)),                # ... in the last
                 (core, flip(core, 0), core, flip(core, n - 1)),                    # different ones: a difference in the first byte
                 (core, core + core, core, core + core[:-1] + K.other(core[-1])),   # insertions that differ in the last byte
                 (core + "A", core, core + "A", core + "AC"),                       # a deletion against an insertion: a prefix of the other
                 ("G" + core, "G", "G" + core.lower(), "g"),                        # the whole core deleted, either case
                 (core, core, core, core)]                                          # REF == ALT: an edit of nothing
        for k in (63, 64, 65):
            if k < n:
                cases.append((core, core, core, flip(core, k)))                     # a difference in bytes 63, 64 and 65
        for ra, aa, rb, ab in cases:
            rows_a.append(("c", pos, f"a{len(rows_a)}", ra, aa, ["1"]))
            rows_b.append(("c", pos, f"b{len(rows_b)}", rb, ab, ["1"]))
            pos += 1000
    got, want = K.both_tiers(hip, K.vcf(["s"], rows_a), K.vcf(["s"], rows_b))
    assert {H.H_EQUAL, H.H_DIFFER} <= set(got.cell_status.tolist()) and 0 < want["n_tier2"] < got.n_items_a + got.n_items_b
    diffs = set(got.cell_first_diff[got.cell_status == H.H_DIFFER].tolist())
    assert {0, 63, 64, 65, 127, 255, 399} <= diffs, sorted(diffs)  # the first byte, bytes 63 to 65, the last byte of 2n
    lens = set(got.cell_len_a.tolist()) | set(got.cell_len_b.tolist())
    assert {1, 31, 32, 33, 63, 64, 65, 128, 200, 400} <= lens
    assert ((got.cell_status == H.H_DIFFER) & (got.cell_first_diff == np.minimum(got.cell_len_a, got.cell_len_b))).any()  # a prefix


# ---- edits per cell

def _snvs(rng, text, n, step=3):
    """n SNV rows over `text`, one every `step` bases from POS 2."""
    return [("c", 2 + step * k, f"v{k}", text[1 + step * k], K.other(text[1 + step * k]), ["1"]) for k in range(n)]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 130])
def test_n_edits_in_one_cell(hip, n):
    rng = np.random.default_rng(n)
    text = K.bases(rng, 3 * 130 + 5)
    whole = ("c", 1, "whole", text, text[:1] + K.other(text[1]) + text[2:], ["0"])  # one record spans the window; nobody carries it
    a = K.vcf(["s"], [whole] + _snvs(rng, text, n))
    alt = list(text)
    for k in range(n):
        alt[1 + 3 * k] = K.other(text[1 + 3 * k])
    b = K.vcf(["s"], [("c", 1, "joint", text, "".join(alt) if n else ".", ["1" if n else "0"])])  # the same haplotype as one edit
    got, _ = K.both_tiers(hip, a, b)
    assert got.n_windows == 1 and statuses(got) == ["equal" if n else "equal_ref"] and got.cell_edits_a.tolist() == [n]
    if n:  # one SNV less on B: the haplotypes differ in that base
        got, _ = K.both_tiers(hip, a, K.vcf(["s"], [whole] + _snvs(rng, text, n)[:-1]))
        assert statuses(got) == ["differ"] and int(got.cell_first_diff[0]) == 1 + 3 * (n - 1)


def test_conflicts_insertions_and_duplicates(hip):
    rng = np.random.default_rng(2)
    text = K.bases(rng, 3 * 70 + 5)
    whole = ("c", 1, "whole", text, ".", ["0"])
    snvs = _snvs(rng, text, 66)
    # edit 65 overlaps edit 64 (a two-base replacement that runs into the next SNV): the conflict lies across the chunk's edge
    p64 = 2 + 3 * 63
    overl = list(snvs)
    overl[63] = ("c", p64, "wide", text[p64 - 1:p64 + 3], K.other(text[p64 - 1]) + text[p64:p64 + 2] + K.other(text[p64 + 2]), ["1"])
    got, _ = K.both_tiers(hip, K.vcf(["s"], [whole] + overl), K.vcf(["s"], [whole] + snvs))
    assert statuses(got) == ["conflict_a"]
    got, _ = K.both_tiers(hip, K.vcf(["s"], [whole] + snvs), K.vcf(["s"], [whole] + overl))
    assert statuses(got) == ["conflict_b"]
    short = ("c", 1, "whole", "ACGTACGT", ".", ["0"])
    ins = lambda pos, t, i="i": ("c", pos, i, "ACGTACGT"[pos - 1], "ACGTACGT"[pos - 1] + t, ["1"])  # noqa: E731
    rep = ("c", 4, "rep", "TAC", "GGG", ["1"])  # replaces [3, 6)
    for rows, status in (([ins(3, "TT"), ins(3, "CC", "j")], "conflict_a"),       # two insertions at one point
                         ([ins(3, "TT"), rep], "differ"),                         # an insertion at the replaced span's start
                         ([ins(4, "AA"), rep], "conflict_a"),                     # ... inside it
                         ([ins(6, "TT"), rep], "differ"),                         # ... at its end
                         ([ins(3, "TT"), ins(3, "TT", "j")], "differ"),           # the same insertion from two records: once
                         ([("c", 3, "two", "G", "GTT,GTT", ["1"]), ("c", 3, "k", "G", "GTT", ["1"])], "differ")):  # ... and from one
        got, _ = K.both_tiers(hip, K.vcf(["s"], [short] + rows), K.vcf(["s"], [short]))
        assert statuses(got) == [status], rows
    got, _ = K.both_tiers(hip, K.vcf(["s"], [short, ins(3, "TT"), ins(3, "TT", "j")]), K.vcf(["s"], [short, ins(3, "TT")]))
    assert statuses(got) == ["equal"] and got.cell_edits_a.tolist() == [1]


# ---- reach

def test_reaches_of_every_length(ctx):
    rng = np.random.default_rng(8)
    named, rows = [], []
    for run in (0, 1, 63, 64, 65):
        for unit in ("A", "AC", "ACG", K.bases(rng, 64), K.bases(rng, 65)):
            m = len(unit)
            rep = (unit * (run // m + 2))[:run]                      # `run` bases of the repeat to the right of the unit
            lead = (unit * (run // m + 2))[-run:] if run else ""      # ... and to the left
            name = f"p{len(named)}"
            named.append((name, "G" + lead + unit + rep + "T"))
            at = 1 + len(lead)                                        # the unit's first base, 0-based
            rows.append((name, at, f"d{len(rows)}", ("G" + lead + unit)[at - 1] + unit, ("G" + lead + unit)[at - 1], ["1"]))  # the unit deleted
            named.append((name + "e", lead + unit + rep))             # the same at both ends of the path
            rows.append((name + "e", max(at - 1, 1), f"e{len(rows)}", (lead + unit + rep)[max(at - 2, 0)], (lead + unit + rep)[max(at - 2, 0)] + unit,
                         ["1"]))                                      # the unit inserted
    named.append(("mx", "GATTACA"))
    rows.append(("mx", 1, "mixed", "GA", "TAC", ["1"]))               # a mixed edit has no reach
    reference = K.upload_reference(ctx, named)
    a = K.vcf(["s"], rows)
    got, want = K.both_tiers(ctx, a, a, reference)
    reaches = set(got.item_left_a.tolist()) | set(got.item_right_a.tolist())
    print("reaches:", sorted(reaches))
    assert {0, 1, 63, 64, 65} <= reaches and got.n_reach_capped == 0
    assert set(got.cell_status.tolist()) <= {H.H_EQUAL} and got.n_unplaced_a == 0


def test_reach_at_the_cap_and_without_one(ctx):
    named = [("run", "G" + "A" * 300 + "T"), ("edge", "A" * 20)]
    reference = K.upload_reference(ctx, named)
    rows = [("run", 41, "x", "AA", "A", ["1"]), ("edge", 10, "y", "A", "AA", ["1"])]  # the edits [40, 41) -> nothing and "A" at 9
    a, b = K.vcf(["s"], rows), K.vcf(["s"], [("run", 1, "x", "GA", "G", ["1"]), ("edge", 1, "y", "A", "AA", ["1"])])
    # A's deletion has 39 more A to the left and 260 to the right, B's at [1, 2) none and 299; the insertions reach 9 and 11 (A's)
    # and 0 and 20 (B's)
    for cap in (260, 259, 39, 38, 0, 65536):
        got, want = K.both_tiers(ctx, a, b, reference, max_reach=cap)
        assert got.n_reach_capped == (cap < 260) + (cap < 299) + (cap < 11) + (cap < 20)  # exactly at the cap is not capped
        assert int(got.item_right_a[0]) == min(260, cap) and int(got.item_left_a[0]) == min(39, cap)
    got, _ = K.both_tiers(ctx, a, b, reference, max_reach=260)
    assert statuses(got) == ["equal", "equal"] and got.n_windows == 2  # A's and B's deletion share a window through the run
    got, _ = K.both_tiers(ctx, a, b, reference, max_reach=0)
    assert got.n_windows == 4 and got.item_left_a.tolist() == [0, 0] and got.n_reach_capped == 4


# ---- windows

def test_windows_touching_nested_chained_and_interleaved(hip):
    rng = np.random.default_rng(4)
    text = K.bases(rng, 400)
    row = lambda ch, pos, n, i, gt="0": (ch, pos, i, text[pos - 1:pos - 1 + n], ".", [gt])  # noqa: E731
    rows_a = [row("c", 1, 4, "t0"), row("c", 5, 4, "t1"),           # touching: one window
              row("c", 10, 4, "u0"), row("c", 15, 4, "u1"),         # one apart: two
              row("c", 30, 20, "n0"), row("c", 35, 3, "n1"),        # contained
              row("d", 1, 4, "d0"), row("c", 60, 2, "late"), row("d", 1, 2, "d1")]  # two CHROMs with equal positions, interleaved
    rows_a += [row("c", 100 + 2 * k, 3, f"ch{k}") for k in range(130)][::-1]  # a chain of 130 overlapping records, out of order
    rows_b = [row("c", 8, 2, "b0", "1"), row("e", 1, 3, "onlyb", "1"), row("d", 3, 3, "b1")]  # joins t0 / t1 and u0; a CHROM only in B
    got, want = K.both_tiers(hip, K.vcf(["s"], rows_a), K.vcf(["s"], rows_b))
    wins = list(zip([got.chroms[c] for c in got.win_chrom.tolist()], got.win_lo.tolist(), got.win_hi.tolist(), got.win_n_a.tolist(), got.win_n_b.tolist()))
    assert wins == [("c", 0, 13, 3, 1), ("c", 14, 18, 1, 0), ("c", 29, 49, 2, 0), ("c", 59, 61, 1, 0), ("c", 99, 360, 130, 0), ("d", 0, 5, 2, 1),
                    ("e", 0, 3, 0, 1)]
    assert got.n_inconsistent == 0


def test_both_window_verdicts(hip, ctx):
    a = K.vcf(["s"], [("c", 1, "x", "ACGT", "A", ["1"]), ("c", 3, "y", "GT", "G", ["0"]), ("c", 20, "ok", "AC", "A", ["1"])])
    b = K.vcf(["s"], [("c", 2, "z", "CTT", "C", ["1"]), ("c", 20, "ok", "ac", "a", ["1"])])  # B's REF says T where A's says G
    got, _ = K.both_tiers(hip, a, b)
    assert got.win_inconsistent.tolist() == [1, 0] and statuses(got) == ["inconsistent", "equal"]
    assert int(got.win_offender[0]) == 0 and int(got.win_offender[1]) == 0xFFFFFFFF  # the greater byte stands: A's records offend
    reference = K.upload_reference(ctx, [("c", "ACGTACGTACGTACGTACGTACGT")])
    got, _ = K.both_tiers(ctx, a, b, reference)
    assert got.win_inconsistent.tolist() == [1, 1] and int(got.win_offender[0]) == 3 and int(got.win_offender[1]) == 2
    assert statuses(got) == ["inconsistent", "inconsistent"] and "inconsistent 2" in got.summary_text()


def test_unplaced_records(ctx):
    reference = K.upload_reference(ctx, [("p", "ACGTACGT"), ("q", "TTTT")])
    rows = [("nopath", 1, "r0", "A", "C", ["1"]), ("p", 8, "r1", "TA", "T", ["1"]), ("p", 0, "r2", "A", "C", ["1"]), ("p", 8, "r3", "T", "C", ["1"]),
            ("q", 1, "r4", ".", "C", ["1"]), ("q", 4, "r5", "T", "<DEL>", ["1"])]
    a = K.vcf(["s"], rows)
    got, _ = K.both_tiers(ctx, a, a, reference)
    assert got.rec_placed_a.tolist() == [0, 0, 0, 1, 0, 1] and got.n_unplaced_a == got.n_unplaced_b == 4
    assert got.item_state_a.tolist() == [H.H_UNPLACED, H.H_UNPLACED, H.H_UNPLACED, H.H_EDIT, H.H_UNPLACED, H.H_UNSPELLED]
    assert "Unplaced records: A 4, B 4\n" in got.summary_text()
    got, _ = K.both_tiers(ctx, a, a)  # by the REF fields all but `.` are placed, POS 0 among them: its window begins at -1
    assert got.rec_placed_a.tolist() == [1, 1, 1, 1, 0, 1] and -1 in got.win_lo.tolist()


# ---- cells

def test_ploidies_phases_columns_and_unspelled_entries(hip):
    samples = ["s0", "s1", "s2", "s3", "s4"]
    rows_a = [("c", 10, "r0", "ACG", "A,ATT", ["1", "0|2", "1|0|2", ".|1", "."]),
              ("c", 11, "r1", "C", "T,*,<DEL>", ["1", "1|0", "0|1|0", "2|.", "3"]),       # entries naming `*` and <DEL>; s0 carries two overlapping edits
              ("c", 30, "r2", "G", "C", ["1", "1", "5", "1/1", "0"])]                       # an entry beyond the ALTs
    rows_b = [("c", 10, "q0", "ACG", "A,ATT", ["0|1", "1", "2", "2|0|1"]),                  # a phase only one side has
              ("c", 30, "q1", "G", "C", ["1", "1", "1", "1"])]
    a, b = K.vcf(samples, rows_a), K.vcf(["s3", "x", "s0", "s1"], rows_b)                   # permuted, renamed, dropped
    got, want = K.both_tiers(hip, a, b)
    assert got.n_common_samples == 3 and got.sample_col_b.tolist() == [2, 3, 0]
    seen = set(statuses(got))
    assert {"nocall_a", "nocall_b", "unspelled_a", "conflict_a", "equal", "differ"} <= seen, seen
    assert got.cell_phase.max() == 2
    got, _ = K.both_tiers(hip, b, a)
    assert {"unspelled_b", "conflict_b"} <= set(statuses(got))
    for sa, sb in ((samples, ["x", "y"]), (samples, []), ([], [])):  # no common sample; no sample columns
        ra = [(ch, p, i, r, alt, g[:len(sa)]) for ch, p, i, r, alt, g in rows_a]
        rb = [(ch, p, i, r, alt, (g + ["0"])[:len(sb)]) for ch, p, i, r, alt, g in rows_b]
        got, _ = K.both_tiers(hip, K.vcf(sa, ra), K.vcf(sb, rb))
        assert got.n_common_samples == 0 and got.n_cells == 0 and got.n_windows == 2 and "Concordance: nan\n" in got.summary_text()


def test_every_status_and_empty_documents(hip):
    full = K.vcf(["s"], [("c", 1, "x", "A", "C", ["1"]), ("c", 2, "y", "AT", "A,ATT", ["1/2"])])
    none, dots = K.HEAD + "s\n", K.vcf(["s"], [("c", 1, "x", ".", "A", ["1"])])
    for a, b in ((none, full), (full, none), (none, none), (dots, full), (dots, dots), (dots, none)):
        got, _ = K.both_tiers(hip, a, b)
        assert got.n_windows == (1 if full in (a, b) else 0)  # (its two records touch)
        assert set(statuses(got)) <= {"nocall_a", "nocall_b"}
    got = hip.compare_haplotypes(H.parse_vcf(full, threads=2), full)  # a VcfDoc for either side
    assert statuses(got) == ["equal", "equal"] and got.cell_phase.tolist() == [0, 1]


COLLIDE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import json
import vcfhap_cases as K
from povu_amd import HipDecomposer
a, b = open(sys.argv[2]).read(), open(sys.argv[3]).read()
d = HipDecomposer(0)
c, _ = K.both_tiers(d, a, b)
print(json.dumps(dict(digest=K.digest(c), n_splits=c.n_splits)))
d.close()
"""


def test_every_run_collides_with_one_hash_bit(hip, tmp_path):
    rng = np.random.default_rng(1)
    rows_a = [("c", 10 + 5 * (k % 40), f"a{k}", "A", "A" + K.bases(rng, 1 + k % 3), ["1"]) for k in range(150)]
    rows_a += [("c", 500, f"l{k}", "G", "G" + K.bases(rng, 70), ["1"]) for k in range(6)] + [("c", 9, "s", "A", "*", ["1"])] * 3
    rows_b = rows_a[::3] + [("c", 600 + k, f"b{k}", "AC", "A", ["1"]) for k in range(40)]
    a, b = K.vcf(["s"], rows_a), K.vcf(["s"], rows_b)
    (tmp_path / "a.vcf").write_text(a)
    (tmp_path / "b.vcf").write_text(b)
    c, _ = K.both_tiers(hip, a, b)
    r = subprocess.run([sys.executable, "-c", COLLIDE, os.path.join(ROOT, "tests"), str(tmp_path / "a.vcf"), str(tmp_path / "b.vcf")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, POVU_HIP_TRAV_HASH_BITS="1", PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.splitlines()[-1])
    assert out["digest"] == json.loads(json.dumps(K.digest(c))) and out["n_splits"] > 0 and c.n_splits == 0


# ---- contexts, arenas, refusals

def _vcs(d):
    return {a["name"]: a["bytes"] for a in d.arenas() if a["bytes"]}


def test_arena_bytes_only_in_the_two_vcf_arenas():
    d = HipDecomposer(0)
    try:
        assert len(d.arenas()) == 54 and _vcs(d) == {}
        a = K.vcf(["s"], [("c", 1, "x", "ACGT", "A", ["1"]), ("c", 20, "y", "A", "AT", ["1"])])
        first = K.digest(d.compare_haplotypes(a, a))  # a fresh context, no graph uploaded
        assert set(_vcs(d)) == {"vc_ws", "vc_hit"} and len(d.arenas()) == 54
        d.release_workspace()
        assert _vcs(d) == {}
        assert K.digest(d.compare_haplotypes(a, a)) == first
        assert K.K.digest(d.compare_vcfs(a, a))["n_shared"] == 2 and K.digest(d.compare_haplotypes(a, a)) == first
    finally:
        d.close()


def test_refusals(hip, ctx):
    lib = H.load_lib()
    err = C.create_string_buffer(512)
    doc = H.parse_vcf(K.vcf(["s"], [("c", 1, "x", "A", "C", ["1"])]))
    call = lambda c, a, b, names=None, n=0, opts=None: lib.povu_hip_vcf_haplotypes(c, a, b, names, n, opts, err, 512)  # noqa: E731
    assert not call(hip._ctx, None, doc._p) and "null" in err.value.decode()
    assert not call(hip._ctx, doc._p, None) and "null" in err.value.decode()
    assert not call(None, doc._p, doc._p) and "null" in err.value.decode()
    for field, what in (("n_tasks", "tasks"), ("n_text_bytes", "text bytes"), ("n_alleles", "alleles"), ("n_records", "records")):
        for n, together in ((2 ** 32, False), (2 ** 31, True)):
            big = H._VcfDoc()
            setattr(big, field, n)
            sides = (C.byref(big), C.byref(big)) if together else (doc._p, C.byref(big))
            assert not call(hip._ctx, sides[0], sides[1])
            msg = err.value.decode()
            assert what in msg and "2^32 or more are refused" in msg and (together or "of a document" in msg), msg
    bad = H._VcfDoc()
    C.memmove(C.byref(bad), doc._p, C.sizeof(H._VcfDoc))
    bad.n_chroms = 0
    assert not call(hip._ctx, doc._p, C.byref(bad)) and "document B" in err.value.decode()
    far = H.parse_vcf(K.vcf(["s"], [("c", 2 ** 40, "x", "A", "C", ["1"])]))
    assert not call(hip._ctx, doc._p, far._p) and "2^40 or more is refused" in err.value.decode()
    assert hip.compare_haplotypes(doc, H.parse_vcf(K.vcf(["s"], [("c", 2 ** 40 - 1, "x", "A", "C", ["1"])]))).n_windows == 2
    over = H._VcfHapOpts(0, 65537)
    assert not call(hip._ctx, doc._p, doc._p, None, 0, C.byref(over)) and "max_reach" in err.value.decode()
    # reference mode without resident paths and sequences, or with another number of names
    names = (C.c_char_p * 1)(b"c")
    assert not call(hip._ctx, doc._p, doc._p, names, 1) and "paths" in err.value.decode()
    links, paths, seqs = K.reference_graph([("c", "ACGT")])
    ctx.upload(links)
    ctx.upload_paths(paths)
    assert not call(ctx._ctx, doc._p, doc._p, names, 1) and "sequences" in err.value.decode()
    ctx.upload_sequences(seqs)
    assert not call(ctx._ctx, doc._p, doc._p, names, 2) and "2 path names for 1 resident paths" in err.value.decode()
    assert ctx.compare_haplotypes(doc, doc, reference=True).n_status[H.H_EQUAL] == 1
    assert hip.compare_haplotypes(doc, doc).n_status[H.H_EQUAL] == 1  # the context is as good as before


# ---- this project's own calls: raw-graph against the profiles that rewrite records, the GFA as reference

OWN = [(fx, options) for fx in ("tandem-repeat-left-normalization", "vcfwave-complex-decomposition")
       for options in (["--profile=left-normalized"], ["--profile=decomposed"], ["--profile=decomposed", "--merge-primitives"])]


@pytest.mark.parametrize("fixture, options", OWN)
def test_own_calls_raw_against_the_rewriting_profiles(ctx, fixture, options):
    gfa = K.gfa_path(fixture)
    call = lambda extra: subprocess.run([POVU, "gfa2vcf", "-i", gfa, "-P", "HG1", "--stdout"] + extra, capture_output=True, text=True,  # noqa: E731
                                        timeout=120, env=dict(os.environ, POVU_CALL_EXE=POVU))
    raw, other = call([]), call(options)
    assert raw.returncode == 0 and other.returncode == 0, raw.stderr + other.stderr
    reference = K.upload_gfa(ctx, fixture)
    got, want = K.both_tiers(ctx, raw.stdout, other.stdout, reference)
    print("own calls:", fixture, options, "\n" + got.summary_text() + got.haplotypes_text())
    assert got.n_cells > 0 and got.n_unplaced_a == got.n_unplaced_b == 0
    assert want["n_status"][HR.DIFFER] == 0 and want["n_status"][HR.INCONSISTENT] == 0
