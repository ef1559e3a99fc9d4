"""GPU consensus haplotypes (povu_hip_vcf_consensus, HipDecomposer.consensus) against the plain-Python restatement
(tests/vcfcons_ref.py), array for array and text for text, every case again with the forced second tier (equal but for n_tier2):
edits and haplotype ends on the edges of the materialiser's tile and of a lane's 16 bytes; 0 to 130 edits in a haplotype, at both
ends of the path; the drop rule's golden cases; ploidies, columns, unspelled and absent entries, unplaced records, two CHROMs;
the selection; every round-trip status; the golden files; this project's own calls, which must round-trip; empty inputs; the
output limit; the arenas; the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import vcfcons_cases as K
import vcfcons_ref as CR
from povu_amd import HipDecomposer
from povu_amd import hip as H

pytestmark = pytest.mark.gpu
ROOT = K.ROOT
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
T = H.C_TILE_BYTES
GFA = os.path.join(ROOT, "tests", "golden", "gfa")


@pytest.fixture()
def ctx():
    d = HipDecomposer(0)
    yield d
    d.close()


def _ins(path, s, t, rid, gt):
    """A row that inserts t in front of base s (s >= 1), anchored on the base before."""
    return ("p", s, rid, path[s - 1], path[s - 1] + t, gt)


def _del(path, s, e, rid, gt, chrom="p"):
    """A row that deletes [s, e) (s >= 1), anchored on the base before."""
    return (chrom, s, rid, path[s - 1:e], path[s - 1], gt)


# ---- tile edges

@pytest.mark.parametrize("k", [1, 15, 16, 17])
def test_an_insertion_across_a_tile_edge(ctx, k):
    rng = np.random.default_rng(k)
    path = K.bases(rng, 2 * T + 37)
    names, ref = K.upload_named(ctx, [("p", path), ("s#1#p", path)])
    t = K.bases(rng, 2 * k).lower()
    t = t[:-1] + K.other(path[T - k - 1]).lower()  # (its last byte is not the anchor's: the suffix trim takes nothing of it)
    gt = lambda *on: ["|".join("1" if j in on else "0" for j in range(6))]  # noqa: E731
    rows = [_ins(path, T - k, t, "ins", gt(0)),                 # T at the output offsets [T - k, T + k) of the first haplotype
            _del(path, T - 7, T, "del_to", gt(1)),              # a deletion that ends at base T
            _del(path, 160, 160 + 9, "del_lane", gt(2)),        # ... and ones whose output position is a lane's edge and one off it
            _del(path, 161, 161 + 9, "del_lane1", gt(3)), _del(path, 159, 159 + 9, "del_lane_1", gt(4)),
            ("p", 1 + 176, "snv", path[176], K.other(path[176]), gt(5))]
    got, want = K.both_tiers(ctx, K.vcf(["s"], rows), names, ref)
    assert got.n_haps == 6 and got.hap_len.tolist() == [len(path) + 2 * k, len(path) - 7] + [len(path) - 9] * 3 + [len(path)]
    assert got.sequence(0)[T - k:T + k] == t and got.n_text_bytes > 11 * T
    # the second haplotype begins inside a tile and a lane: at 2T + 37 + 2k
    assert int(got.hap_off[1]) % 16 != 0 and K.statuses(want) == ["differ", "no_path", "no_path", "no_path", "no_path", "no_path"]


def test_a_deletion_that_ends_at_a_tile_edge_of_the_output(ctx):
    rng = np.random.default_rng(3)
    path = K.bases(rng, 2 * T + 5)
    names, ref = K.upload_named(ctx, [("p", path)])
    rows = [_del(path, T, T + 11, "at_edge", ["1|0|0"]),        # the byte at output offset T comes from base T + 11
            _del(path, 2 * T - 20, 2 * T + 5, "tail", ["0|1|0"]),  # the path's tail deleted
            ("p", 1, "head", path[:T + 1], path[T], ["0|0|1"])]    # the first T bases deleted: REF[0 .. T] -> its last base
    got, want = K.both_tiers(ctx, K.vcf(["s"], rows), names, ref, roundtrip=False)
    assert got.hap_len.tolist() == [len(path) - 11, 2 * T - 20, T + 5] and got.sequence(0)[T] == path[T + 11]


def test_haplotype_lengths_around_a_lane_and_a_tile(ctx):
    rng = np.random.default_rng(9)
    path = K.bases(rng, T + 1)
    lengths = [0, 1, 15, 16, 17, T - 1, T, T + 1]
    names, ref = K.upload_named(ctx, [("q", path)])
    gt = lambda *on: ["|".join("1" if j in on else "0" for j in range(len(lengths)))]  # noqa: E731
    rows = [("q", 1, "first", path[:2], path[1], gt(0))]  # base 0 deleted: with `to1` the whole path
    for j, n in enumerate(lengths[:-1]):
        rows.append(_del(path, max(n, 1), T + 1, f"to{max(n, 1)}", gt(j), chrom="q"))
    got, want = K.both_tiers(ctx, K.vcf(["s"], rows), names, ref, roundtrip=False)
    assert got.hap_len.tolist() == lengths and got.sequence(0) == "" and got.sequence(1) == path[0]
    offs = got.hap_off.tolist()
    assert sum(1 for a, b in zip(offs[1:], offs[2:]) if a // T == b // T and a != b) >= 4  # haplotypes that end and begin in one tile
    assert got.n_applied.tolist() == [2, 1, 1, 1, 1, 1, 1, 0]


# ---- edits per haplotype

def test_0_to_130_edits_at_both_ends_of_the_path(ctx):
    rng = np.random.default_rng(11)
    path = K.bases(rng, 3 * 129 + 1)
    counts = [0, 1, 63, 64, 65, 130]
    names, ref = K.upload_named(ctx, [("p", path), ("s#1#p", path)])
    chosen = [set(range(n - 1)) | ({129} if n else set()) if n != 1 else {0} for n in counts]
    rows = []
    for k in range(130):
        rows.append(("p", 1 + 3 * k, f"v{k}", path[3 * k], K.other(path[3 * k]), ["|".join("1" if k in c else "0" for c in chosen) + "|0"]))
    lead, tail = "ttg", "gca"
    rows.append(("p", 1, "front", path[0], lead + path[0], ["0|" * 6 + "1"]))          # an insertion at offset 0
    rows.append(("p", len(path), "back", path[-1], path[-1] + tail, ["0|" * 6 + "1"]))  # ... and one behind the last base
    got, want = K.both_tiers(ctx, K.vcf(["s"], rows), names, ref)
    assert got.n_applied.tolist() == counts + [2] and got.sequence(6) == lead + path + tail
    assert got.sequence(5)[0] != path[0] and got.sequence(5)[-1] != path[-1] and got.hap_len.tolist() == [len(path)] * 6 + [len(path) + 6]
    assert K.statuses(want) == ["equal"] + ["no_path"] * 6  # (the sample has one slot: the phases behind it have no path)


# ---- drops

@pytest.mark.parametrize("name", sorted(K.DROP_CASES))
def test_the_drop_rule_golden_cases(ctx, name):
    text, named = K.drop_case(name)
    names, ref = K.upload_named(ctx, named)
    got, want = K.both_tiers(ctx, text, names, ref)
    assert json.loads(json.dumps(K.lib_digest(got))) == K.expected()[name]
    counts, hap = K.DROP_PINS[name]
    assert (int(got.n_applied[0]), int(got.n_duplicate[0]), int(got.n_enclosed[0]), int(got.n_overlap[0])) == counts and got.sequence(0) == hap


def test_drops_across_a_chunk_of_64_edits(ctx):
    rng = np.random.default_rng(5)
    path = K.bases(rng, 3 * 140 + 8)
    names, ref = K.upload_named(ctx, [("p", path)])
    rows = [("p", 2 + 3 * k, f"v{k}", path[1 + 3 * k], K.other(path[1 + 3 * k]), ["1"]) for k in range(132)]
    # a span over the SNVs 60 .. 69: they are enclosed, across the chunk's edge; one that ends behind it overlaps; a duplicate
    a, b = 1 + 3 * 60 - 1, 1 + 3 * 69 + 2
    rows.append(("p", a + 1, "span", path[a:b], K.other(path[a]) + "tt" + K.other(path[b - 1]), ["1"]))
    rows.append(("p", b - 1, "over", path[b - 2:b + 5], K.other(path[b - 2]) + K.other(path[b + 4]), ["1"]))
    rows.append(rows[5][:2] + ("dup",) + rows[5][3:])
    got, want = K.both_tiers(ctx, K.vcf(["s"], rows), names, ref, roundtrip=False)
    # (the SNVs 70 and 71 lie inside `over`, which is dropped itself: they are dropped too -- the rule is conservative)
    assert (int(got.n_enclosed[0]), int(got.n_overlap[0]), int(got.n_duplicate[0])) == (12, 1, 1), (got.n_enclosed, got.n_overlap)


def test_equal_starts_whose_ends_lie_in_different_words_of_the_sort(ctx):
    """A parent and a child that share a trimmed start: the parent sorts first (e descending) whatever bits their ends differ in
    -- ends on both sides of a multiple of 1024, ends more than 1024 apart."""
    rng = np.random.default_rng(13)
    path = K.bases(rng, 4000)
    names, ref = K.upload_named(ctx, [("p", path)])
    span = lambda s, e, rid, gt: ("p", s + 1, rid, path[s:e], K.other(path[s]) + K.other(path[e - 1]), [gt])  # noqa: E731
    rows = [span(1000, 1010, "kid", "1|0|0"), span(1000, 1030, "par", "1|0|0"),        # ends (one added) 1011 and 1031
            span(100, 150, "kid2", "0|1|0"), span(100, 2500, "par2", "0|1|0"),         # ... 151 and 2501
            span(2047, 2049, "kid3", "0|0|1"), span(2047, 3100, "par3", "0|0|1"), span(2047, 2048, "kid4", "0|0|1")]
    got, want = K.both_tiers(ctx, K.vcf(["s"], rows), names, ref, roundtrip=False)
    assert got.n_applied.tolist() == [1, 1, 1] and got.n_enclosed.tolist() == [1, 1, 2] and got.n_overlap.tolist() == [0, 0, 0]
    assert got.hap_len.tolist() == [4000 - 30 + 2, 4000 - 2400 + 2, 4000 - 1053 + 2]


# ---- tasks

def test_ploidies_columns_unspelled_entries_and_two_chroms(ctx):
    rng = np.random.default_rng(2)
    p1, p2 = K.bases(rng, 200), K.bases(rng, 90)
    names, ref = K.upload_named(ctx, [("c1", p1), ("c2", p2), ("s1#1#c1", p1), ("s1#2#c1", p1)])
    samples = ["s0", "s1", "s2", "s3"]
    rows = [("c1", 10, "r0", p1[9:12], p1[9] + "," + p1[9:12] + "tt", ["1", "0|2", "1|0|2", "."]),
            ("c1", 50, "r1", p1[49], K.other(p1[49]) + ",*,<DEL>", ["1", "1|0", "0|1|3", "2"]),    # entries naming `*` and <DEL>
            ("c1", 80, "r2", p1[79], K.other(p1[79]), ["1", "1", "5|0|0", "3"]),                    # entries beyond the ALTs
            ("c2", 5, "r3", p2[4:8], p2[4], ["0", "1|1", ".", "."]),                                # s2 and s3 have no task on c2
            ("c2", 0, "r4", "A", "C", ["1", "1", "1", "1"]), ("c2", 89, "r5", p2[88:] + "A", "A", ["1", "1", "1", "1"]),  # unplaced
            ("nopath", 3, "r6", "A", "C", ["1", "1", "1", "1"]), ("c1", 120, "r7", ".", "A", ["1", "1", "1", "1"])]
    got, want = K.both_tiers(ctx, K.vcf(samples, rows), names, ref)
    assert got.n_unplaced == 4 and got.n_haps == 1 + 2 + 3 + 1 + 1 + 2 and got.hap_phase.max() == 2
    assert got.n_unspelled.sum() >= 4 and got.n_nocall.sum() > 0 and "Unplaced records: 4\n" in got.summary_text()
    assert got.n_unspelled.tolist() == [0, 0, 0, 1, 0, 1, 2, 0, 0, 0] and set(K.statuses(want)) == {"differ", "no_path"}
    # one sample and one CHROM: the same haplotypes as in the whole run
    one, _ = K.both_tiers(ctx, K.vcf(samples, rows), names, ref, samples=["s1"], chroms=["c2"])
    at = [h for h in range(got.n_haps) if got.doc.chroms[got.hap_chrom[h]] == "c2" and got.hap_col[h] == 1]
    assert one.n_haps == 2 and [one.sequence(0), one.sequence(1)] == [got.sequence(h) for h in at]
    assert one.n_applied.tolist() == got.n_applied[at].tolist() and one.n_unplaced == 4
    cols, _ = K.both_tiers(ctx, K.vcf(samples, rows), names, ref, samples=["s2", "s0"])
    assert cols.hap_col.tolist() == [0, 2, 2, 2, 0]
    quiet = ctx.consensus(K.vcf(samples, rows), roundtrip=True, text=False)
    assert quiet.text is None and quiet.hap_len.tolist() == got.hap_len.tolist() and quiet.rt_status.tolist() == got.rt_status.tolist()
    assert quiet.fasta_text() == "" and quiet.roundtrip_text() == got.roundtrip_text()
    with pytest.raises(RuntimeError):
        quiet.sequence(0)


# ---- round trip

def test_every_round_trip_status(ctx):
    rng = np.random.default_rng(7)
    path = K.bases(rng, 150)
    flip = lambda t, k: t[:k] + K.other(t[k]) + t[k + 1:]  # noqa: E731
    named = [("ref", path), ("a#1#ref", path.lower()), ("b#1#ref", flip(path, 0)), ("c#1#ref", flip(path, 149)), ("d#1#ref", path + "A"),
             ("e#1#ref", path[:-1]), ("f#1#x", path), ("f#1#y", path), ("g#1#ref", path), ("g#2#ref", flip(path, 70))]
    names, ref = K.upload_named(ctx, named)  # (every third segment of a path is walked backwards)
    samples = ["a", "b", "c", "d", "e", "f", "nobody", "g"]
    rows = [("ref", 20, "r", path[19], path[19], ["0", "0", "0", "0", "0", "0", "0", "0|0|0"])]
    got, want = K.both_tiers(ctx, K.vcf(samples, rows), names, ref)
    assert K.statuses(want) == ["equal", "differ", "differ", "differ", "differ", "ambiguous", "no_path", "equal", "differ", "no_path"]
    assert got.rt_first_diff.tolist()[1:5] == [0, 149, 150, 149] and int(got.rt_first_diff[8]) == 70
    assert got.rt_path_len.tolist()[3:5] == [151, 149] and got.hap_len.tolist() == [150] * 10
    # a CHROM with a third field narrows the slot's paths to its contig
    named = [("f#1#x", path), ("f#1#y", flip(path, 3))]
    names, ref = K.upload_named(ctx, named)
    got, want = K.both_tiers(ctx, K.vcf(["f"], [("f#1#y", 20, "r", path[19], path[19], ["0"])]), names, ref)
    assert K.statuses(want) == ["equal"] and int(got.rt_path[0]) == 1


# ---- the golden files, and this project's own calls

@pytest.mark.parametrize("fixture", ["tandem-repeat-left-normalization", "popped-parent-child-rescue"])
def test_the_golden_files(ctx, fixture):
    names, ref = K.upload_gfa_file(ctx, K.K.gfa_path(fixture))
    got, want = K.both_tiers(ctx, K.golden(fixture, "raw_graph"), names, ref)
    by = {got.doc.samples[got.hap_col[h]]: h for h in range(got.n_haps)}
    if fixture.startswith("tandem"):
        assert {s: got.sequence(h) for s, h in by.items()} == dict(HG1="AAAAAC", HG2="AAAAC", HG3="AAAAAAC")
        assert got.rt_status.tolist() == [H.C_RT_EQUAL] * 3
    else:
        h3 = by["HG3"]
        assert got.sequence(by["HG2"]) == "AC" and got.sequence(h3) == "AAGAAC" and got.rt_status.tolist() == [H.C_RT_EQUAL, H.C_RT_EQUAL, H.C_RT_DIFFER]
        assert (int(got.rt_first_diff[h3]), int(got.hap_len[h3]), int(got.rt_path_len[h3])) == (2, 6, 6)


OWN = [(os.path.join(GFA, "downstream_repetitive", fx + ".gfa"), options)
       for fx in ("tandem-repeat-left-normalization", "popped-parent-child-rescue")
       for options in ([], ["--profile=left-normalized"], ["--profile=decomposed"])]
OWN += [(os.path.join(GFA, fx + ".gfa"), []) for fx in ("insertion_flubble", "deletion_flubble", "nested_deletion", "two_ordered_substitutions")]


@pytest.mark.parametrize("gfa, options", OWN, ids=[os.path.basename(g)[:-4] + "".join(o) for g, o in OWN])
def test_own_calls_round_trip(ctx, gfa, options):
    r = subprocess.run([POVU, "gfa2vcf", "-i", gfa, "-P", "HG1", "--stdout"] + options, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, POVU_CALL_EXE=POVU))
    assert r.returncode == 0, r.stderr
    names, ref = K.upload_gfa_file(ctx, gfa)
    got, want = K.both_tiers(ctx, r.stdout, names, ref)
    print("own calls:", os.path.basename(gfa), options, "\n" + got.summary_text() + got.roundtrip_text())
    # A finding, pinned: the raw-graph call of nested_deletion.gfa writes the inner site >1>4 alone, and HG3 (0+,2+,5+) leaves the
    # reference at the outer site, so its GT there is `.`: no task on any record, hence -- by the definition -- no haplotype of
    # HG3, and nothing to round-trip.  Every haplotype that exists is `equal`.
    absent = ["HG3#1#chr1"] if os.path.basename(gfa) == "nested_deletion.gfa" else []
    assert [got.doc.samples[c] + "#1#chr1" for c in got.hap_col.tolist()] == [n for n in names if n not in absent] and got.n_unplaced == 0
    assert K.statuses(want) == ["equal"] * got.n_haps


# ---- empty inputs, refusals, arenas

def test_empty_inputs(ctx):
    names, ref = K.upload_named(ctx, [("p", "ACGTACGT")])
    for text in (K.HEAD + "s\n", K.vcf(["s"], [("nopath", 1, "x", "A", "C", ["1"]), ("p", 8, "y", "TA", "T", ["1"])]), K.vcf([], [("p", 1, "x", "A", "C", [])])):
        got, want = K.both_tiers(ctx, text, names, ref)
        assert got.n_haps == 0 and got.n_text_bytes == 0 and got.fasta_text() == "" and got.summary_text().startswith("Haplotypes: 0, bases 0\n")


def test_refusals(ctx):
    lib = H.load_lib()
    err = C.create_string_buffer(512)
    doc = H.parse_vcf(K.vcf(["s"], [("p", 1, "x", "A", "C", ["1"])]))
    call = lambda c, d, names=None, n=0, opts=None: lib.povu_hip_vcf_consensus(c, d, names, n, opts, err, 512)  # noqa: E731
    assert not call(ctx._ctx, None) and "null" in err.value.decode()
    assert not call(None, doc._p) and "null" in err.value.decode()
    one = (C.c_char_p * 1)(b"p")
    assert not call(ctx._ctx, doc._p, one, 1) and "paths" in err.value.decode()
    links, paths, seqs = K.K.reference_graph([("p", "ACGT" * (2 ** 18))])  # 2^20 bases
    ctx.upload(links)
    ctx.upload_paths(paths)
    assert not call(ctx._ctx, doc._p, one, 1) and "sequences" in err.value.decode()
    ctx.upload_sequences(seqs)
    assert not call(ctx._ctx, doc._p, one, 2) and "2 path names for 1 resident paths" in err.value.decode()
    for field, what in (("n_tasks", "tasks"), ("n_text_bytes", "text bytes"), ("n_records", "records")):
        big = H._VcfDoc()
        setattr(big, field, 2 ** 32 - 64)
        assert not call(ctx._ctx, C.byref(big), one, 1) and what in err.value.decode() and "2^32 or more are refused" in err.value.decode()
    far = H.parse_vcf(K.vcf(["s"], [("p", 2 ** 40, "x", "A", "C", ["1"])]))
    assert not call(ctx._ctx, far._p, one, 1) and "2^40 or more is refused" in err.value.decode()
    sel = (C.c_uint32 * 1)(7)
    opts = H._VcfConsOpts(0, 1, sel, None)
    assert not call(ctx._ctx, doc._p, one, 1, C.byref(opts)) and "selected sample column 7" in err.value.decode()
    opts = H._VcfConsOpts(0, 1, None, sel)
    assert not call(ctx._ctx, doc._p, one, 1, C.byref(opts)) and "selected CHROM 7" in err.value.decode()
    # the output limit by arithmetic: 4096 phases of one column on a path of 2^20 bases are 2^32 bytes; nothing is written
    wide = H.parse_vcf(K.vcf(["s"], [("p", 1, "x", "A", "C", ["|".join(["0"] * 4096)])]))
    assert not call(ctx._ctx, wide._p, one, 1)
    msg = err.value.decode()
    assert str(2 ** 32) + " output bytes for 4096 haplotypes" in msg and "2^32 - 64 or more are refused" in msg and "povu_hip_vcf_cons_opts" in msg
    ok = ctx.consensus(doc)  # the context is as good as before
    assert ok.n_haps == 1 and ok.sequence(0)[:4] == "CCGT" and int(ok.hap_len[0]) == 2 ** 20


def test_the_arenas_hold_the_workspaces_and_release_frees_them():
    d = HipDecomposer(0)
    try:
        names, ref = K.upload_named(d, [("p", "ACGTACGT")])
        held = lambda: {a["name"]: a["bytes"] for a in d.arenas() if a["bytes"] and not a["resident"]}  # noqa: E731
        before = set(held())
        first = K.lib_digest(d.consensus(K.vcf(["s"], [("p", 2, "x", "C", "G", ["1"])])))
        assert {"vc_ws", "vc_hit"} <= set(held()) and set(held()) - before <= {"vc_ws", "vc_hit"}
        d.release_workspace()
        assert "vc_ws" not in held() and "vc_hit" not in held()
        assert K.lib_digest(d.consensus(K.vcf(["s"], [("p", 2, "x", "C", "G", ["1"])]))) == first and first["texts"] == ["AGGTACGT"]
    finally:
        d.close()


# ---- the CLI

def test_the_cli_writes_the_librarys_texts(ctx, tmp_path):
    fx = "tandem-repeat-left-normalization"
    vcf, gfa = os.path.join(K.GOLDEN, fx, "raw_graph.vcf"), K.K.gfa_path(fx)
    names, ref = K.upload_gfa_file(ctx, gfa)
    got = ctx.consensus(open(vcf).read(), roundtrip=True)
    r = subprocess.run([POVU, "vcf", "-i", gfa, "-c", vcf, "--consensus", "--roundtrip", "-o", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and sorted(os.listdir(tmp_path / "out")) == ["cons_summary.txt", "consensus.fa", "roundtrip.tsv"], r.stderr
    assert [(tmp_path / "out" / f).read_text() for f in ("consensus.fa", "roundtrip.tsv", "cons_summary.txt")] == [got.fasta_text(), got.roundtrip_text(),
                                                                                                                    got.summary_text()]
    fx = "popped-parent-child-rescue"  # a haplotype that differs: still exit status 0; a selection, a width, no FASTA
    vcf, gfa = os.path.join(K.GOLDEN, fx, "raw_graph.vcf"), K.K.gfa_path(fx)
    names, ref = K.upload_gfa_file(ctx, gfa)
    got = ctx.consensus(open(vcf).read(), roundtrip=True, samples=["HG3", "HG2"])
    r = subprocess.run([POVU, "vcf", "-i", gfa, "-c", vcf, "--consensus", "--roundtrip", "--sample", "HG3", "--sample=HG2", "--chrom", "HG1#1#chr1",
                        "--line-width=4", "-o", str(tmp_path / "sel")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [(tmp_path / "sel" / f).read_text() for f in ("consensus.fa", "roundtrip.tsv", "cons_summary.txt")] == [got.fasta_text(4), got.roundtrip_text(),
                                                                                                                    got.summary_text()]
    assert "differ" in got.roundtrip_text() and "AAGA\nAC\n" in got.fasta_text(4)
    r = subprocess.run([POVU, "vcf", "-i", gfa, "-c", vcf, "--consensus", "--no-fasta", "-o", str(tmp_path / "quiet")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and sorted(os.listdir(tmp_path / "quiet")) == ["cons_summary.txt", "roundtrip.tsv"], r.stderr
    r = subprocess.run([POVU, "vcf", "-i", gfa, "-c", vcf, "--consensus", "--sample", "nobody", "-o", str(tmp_path / "no")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--sample nobody" in r.stderr
