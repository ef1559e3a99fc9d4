"""The plain-Python restatement of the left-normalised calls (tests/norm_ref.py): its closed form against its literal loop
(hand cases, the reference's tandem-repeat-left-normalization fixture, random records over one or two letters), the
fixture's rows (tests/golden/reference_norm_records.json), a graph that must come out unchanged, the host writer
(povu_hip_calls_vcf_profile under POVU_HIP_PROFILE_LEFT_NORMALIZED) on hand-packed records against the restatement's text,
and the command line's reading of the profile.  No GPU."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

import norm_ref as NR
import oracle_lib as O
import vcf_ref as V
from povu_amd import hip as H
from test_nested_ref import _pack, _vcf
from test_vcf_writer import DATE, _names, _sites_of_texts, lib  # noqa: F401  (lib: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
FIXTURE = "downstream_repetitive/tandem-repeat-left-normalization"
VCFWAVE = "downstream_repetitive/vcfwave-complex-decomposition"

# (context, alleles) -> (r, s, u, alleles'); None: unchanged by definition
HAND = [
    (("CAAA", ["AA", "A"]), (4, 4, 0, ["CA", "C"])),            # a deletion in a homopolymer goes to its left end
    (("AAA", ["AA", "A"]), (3, 3, 0, ["AA", "A"])),             # the repeat begins the contig: the cap, no allele empty
    (("AAA", ["AA", "A", "AAA"]), (3, 3, 0, ["AA", "A", "AAA"])),  # the fixture's record
    (("G", ["TCA", "GA"]), (1, 0, 0, ["TC", "G"])),             # a common suffix only: POS stays
    (("G", ["ACT", "AG"]), (0, 0, 1, ["CT", "G"])),             # a common prefix only: POS grows
    (("G", ["ACTA", "ACGA"]), (1, 0, 2, ["T", "G"])),           # both
    (("caaa", ["AA", "A"]), (4, 4, 0, ["ca", "c"])),            # compared upper-cased, written as spelled
    (("CAAA", ["AA", "aa", "A"]), (4, 4, 0, ["CA", "CA", "C"])),  # an ALT that is REF's text takes no part
    (("TCACAC", ["ACA", "A"]), (6, 6, 0, ["TCA", "T"])),       # period 2, the anchor inside the repeat
    (("GG", ["CGT", "TGA", "CGTACGTACGTA"]), (0, 0, 0, ["CGT", "TGA", "CGTACGTACGTA"])),
    (("CAAA", ["AA", "AA"]), None),
    (("CAAA", ["AA", ""]), None),
]


def test_hand_cases_closed_form_and_loop():
    for (ctx, al), want in HAND:
        got = NR.closed_form(ctx, al)
        if want is None:
            assert got is None
            assert NR.literal_loop(ctx, al) == (0, 0, al)
            continue
        assert got[:4] == want, (ctx, al)
        assert NR.literal_loop(ctx, al) == (want[1], want[2], want[3]), (ctx, al)


def test_closed_form_is_the_loop_on_random_repeats():
    rng = random.Random(20260612)
    changed = shifted = trimmed = capped = 0
    for _ in range(6000):
        letters = rng.choice(["A", "AC", "AC", "Aa", "GT"])
        ctx = "".join(rng.choice(letters) for _ in range(rng.randint(0, 12)))
        al = ["".join(rng.choice(letters) for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(2, 4))]
        got = NR.closed_form(ctx, al)
        s, u, out = NR.literal_loop(ctx, al)
        if got is None:
            assert (s, u, out) == (0, 0, al)
            continue
        assert (got[1], got[2], got[3]) == (s, u, out), (ctx, al)
        assert all(out) and got[0] <= len(ctx) + min(map(len, al)) - 1
        changed += bool(got[0] or got[2])
        shifted += got[1] > 0
        trimmed += got[2] > 0
        capped += got[1] == len(ctx) and len(ctx) > 0
    assert min(changed, shifted, trimmed, capped) >= 100


def _pvst_texts(gfa, out):
    out.mkdir(exist_ok=True)
    n = O.decompose_gfa(gfa, str(out))
    return [(out / f"{i}.pvst").read_text() for i in range(1, n + 1) if (out / f"{i}.pvst").exists()]


def _graph(golden_dir, tmp_path, name):
    gfa = os.path.join(golden_dir, "gfa", name + ".gfa")
    return V.read_gfa(gfa), _pvst_texts(gfa, tmp_path / "fx")


def test_fixture_rows(golden_dir, tmp_path):
    """What the fixture pins and what it does not (INTEGRATION.md "Left-normalised calls"): this project's raw call gives one
    record at >3>5 with both ALTs; it goes from POS 4 to POS 1 as the fixture's rows do, and its REF, first ALT, ID and INFO
    keys are the fixture's first row's.  The fixture's second row (>3>4, no flubble of the plain PVST) states the same
    one-base insertion that is the second ALT here."""
    want = json.load(open(os.path.join(golden_dir, "reference_norm_records.json")))
    (names, paths, seqs), texts = _graph(golden_dir, tmp_path, FIXTURE)
    sites = V.sites_of_pvst(texts)
    assert [V.label(s["s"], s["z"]) for s in sites] == [">3>5"]
    raw = V.call(sites, names, paths, seqs, [want["reference_prefix"]])
    assert [(r["chrom"], r["pos"], r["id"], r["ref"], r["alts"], r["gt"]) for r in raw] == [
        ("HG1#1#chr1", 4, ">3>5", "AA", ["A", "AAA"], ["0", "1", "2"])]
    recs, counters = NR.normalise(raw, paths, seqs)
    (r,) = recs
    assert (r["r"], r["s"], r["u"]) == (3, 3, 0) and counters["n_normalized"] == 1 and counters["max_shift"] == 3
    w0, w1 = want["records"]
    assert (r["chrom"], r["pos"], r["id"], r["ref"], r["alts"][0]) == (w0["chrom"], w0["pos"], w0["id"], w0["ref"], w0["alts"][0])
    assert (r["at"][:2], r["vartype"], r["lv"], r["gt"][:2]) == (w0["at"], w0["vartype"], w0["lv"], w0["gt"][:2])
    assert r["pos"] == w1["pos"] and int(w1["info"]["RAW_POS"]) == r["raw_pos"] == int(w0["info"]["RAW_POS"])
    # the second row's insertion A -> AA is REF AA -> ALT AAA here, one record
    assert w1["ref"] + "A" == r["ref"] and w1["alts"][0] + "A" == r["alts"][1] and w1["gt"][2] == "1" and r["gt"][2] == "2"
    line = NR.record_line(r, V.record_line)
    info = dict(kv.split("=", 1) for kv in line.split("\t")[7].split(";"))
    keys = [kv.split("=", 1)[0] for kv in line.split("\t")[7].split(";")]
    assert keys[-7:] == want["info_keys_in_order"] and keys[-8] == "LV"
    assert {k: info[k] for k in want["info_keys_in_order"]} == dict(w0["info"], RAW_ALT_INDEX="1,2", RAW_ALT="A,AAA")
    assert info["ES"] == w0["es"]
    text = NR.vcf_text(names, paths, seqs, recs, ["HG1"])
    for k, d in want["info_descriptions"].items():
        n = "A" if k in ("RAW_ALT", "RAW_ALT_INDEX") else "1"
        t = "Integer" if k in ("RAW_POS", "RAW_ALT_INDEX") else "String"
        assert text.count(f'##INFO=<ID={k},Number={n},Type={t},Description="{d}">\n') == 1
    head = text.splitlines()
    assert head[len(V.HEADER.splitlines())].startswith("##INFO=<ID=ORIGIN,")  # where the other profiles' lines go
    assert [ln.split("\t")[9:] for ln in head if ln.startswith("#CHROM")] == [want["samples"]]


def test_vcfwave_graph_is_unchanged(golden_dir, tmp_path):
    (names, paths, seqs), texts = _graph(golden_dir, tmp_path, VCFWAVE)
    sites = V.sites_of_pvst(texts)
    raw = V.call(sites, names, paths, seqs, ["HG1"])
    assert [(r["ref"], r["alts"]) for r in raw] == [("CGT", ["TGA", "CGTACGTACGTA"])]
    recs, counters = NR.normalise(raw, paths, seqs)
    assert counters["n_normalized"] == 0 and [{k: r[k] for k in raw[0]} for r in recs] == raw
    assert NR.vcf_text(names, paths, seqs, recs, ["HG1"]) == V.vcf_text(names, paths, seqs, raw, ["HG1"]).replace(
        "##contig", NR.PROFILE_LINES + "##contig", 1)


# ---- the host writer on hand-packed records
# a homopolymer deletion at >3>5 (changed, shifted), a SNP at >5>8 (unchanged), a substitution with a common last base at
# >8>11 (changed, chopped only)
HAND_PVST = "H\t0.0.3\t.\t.\t.\nD\t0\t.\t1, 2, 3\t.\nF\t1\t>3>5\t.\tL\nF\t2\t>5>8\t.\tL\nF\t3\t>8>11\t.\tL\n"
HAND_NAMES = ["R#1#c", "A#1#c", "B#1#c"]
HAND_PATHS = [[(k, 0) for k in (0, 1, 2, 3, 4, 5, 6, 8, 9, 11)], [(k, 0) for k in (0, 1, 2, 3, 5, 7, 8, 10, 11)],
              [(k, 0) for k in (0, 1, 2, 3, 4, 5, 6, 8, 10, 11)]]
HAND_SEQS = dict(enumerate(["GT", "A", "A", "A", "A", "C", "G", "T", "C", "TA", "GA", "G"]))


def _pack_norm(recs, n_slots, contig_len):
    """povu_hip_calls of norm_ref records: the raw alleles packed as test_nested_ref packs a plain call's, a block of the
    normalised alleles (REF first, empty AT strings) behind them for every changed record, the per-record fields."""
    rawlike = [dict(r, ref=r["raw_ref"], alts=r["raw_alts"], ref_class=0, n_classes=1 + len(r["alts"]), ref_is_rep=True, collapsed=False,
                    rescued=False, parent=None) for r in recs]
    c, a = _pack(rawlike, n_slots, contig_len, nested=False)
    u32, u64 = (lambda x: np.ascontiguousarray(x, dtype=np.uint32)), (lambda x: np.ascontiguousarray(x, dtype=np.uint64))
    seq_off, at_off, block_off = a["seq_off"].tolist(), a["at_off"].tolist(), a["block_off"].tolist()
    seq = bytes(a["seq"][:-1]).decode()
    norm_block = []
    for r in recs:
        norm_block.append(len(block_off) - 1 if r["normalized"] else 0xFFFFFFFF)
        if r["normalized"]:
            for t in [r["ref"]] + r["alts"]:
                seq += t
                seq_off.append(len(seq))
                at_off.append(at_off[-1])
            block_off.append(len(seq_off) - 1)
    a.update(seq=np.frombuffer(seq.encode() + b"\0", np.uint8), seq_off=u64(seq_off), at_off=u64(at_off), block_off=u64(block_off),
             flags=a["flags"] | np.array([H.CALL_NORMALIZED if r["normalized"] else 0 for r in recs], np.uint8),
             raw_pos=u64([r["raw_pos"] for r in recs]), norm_block=u32(norm_block), norm_shift=u32([r["s"] for r in recs]),
             norm_chop=u32([r["r"] for r in recs]), norm_trim=u32([r["u"] for r in recs]))
    c.n_blocks, c.n_spelled, c.n_seq_bytes = len(block_off) - 1, len(seq_off) - 1, len(seq)
    c.n_normalized = sum(r["normalized"] for r in recs)
    for k in ("seq", "seq_off", "at_off", "block_off", "flags", "raw_pos", "norm_block", "norm_shift", "norm_chop", "norm_trim"):
        setattr(c, k, a[k].ctypes.data_as(dict(H._Calls._fields_ + H._CallsNested._fields_)[k]))
    return c, a


def test_writer_changed_unchanged_and_multi_alt(lib, golden_dir, tmp_path):
    vsites = V.sites_of_pvst([HAND_PVST])
    raw = V.call(vsites, HAND_NAMES, HAND_PATHS, HAND_SEQS, ["R#"])
    recs, counters = NR.normalise(raw, HAND_PATHS, HAND_SEQS)
    assert [(r["id"], r["raw_pos"], r["pos"], r["ref"], r["alts"], r["r"], r["s"], r["u"]) for r in recs] == [
        (">3>5:norm", 5, 2, "TA", ["T"], 3, 3, 0), (">5>8", 8, 8, "G", ["T"], 0, 0, 0), (">8>11:norm", 10, 10, "T", ["G"], 1, 0, 0)]
    assert counters == dict(n_normalized=2, max_shift=3, n_norm_compared=4 + 1 + 2)
    sites, nr = _sites_of_texts(lib, [HAND_PVST]), _names(lib, HAND_NAMES, ["R#"])
    calls, keep = _pack_norm(recs, 3, [12])
    want = NR.vcf_text(HAND_NAMES, HAND_PATHS, HAND_SEQS, recs, ["R#"], date=DATE)
    assert want.count(":norm\t") == 2 and want.count("LEFT_NORMALIZED=T") == 2
    for threads in (1, 4):
        assert _vcf(lib, calls, sites, nr, HAND_NAMES, NR.PROFILE, threads=threads) == want
    # the new arrays absent (a hand-made povu_hip_calls of before): the raw text under the profile's header lines
    rawrecs = [dict(r, pos=r["raw_pos"], id=r["id"].replace(":norm", ""), ref=r["raw_ref"], alts=r["raw_alts"], normalized=False) for r in recs]
    calls.raw_pos = None
    calls.norm_block = None
    calls.pos = np.ascontiguousarray([r["raw_pos"] for r in recs], np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))
    assert _vcf(lib, calls, sites, nr, HAND_NAMES, NR.PROFILE) == NR.vcf_text(HAND_NAMES, HAND_PATHS, HAND_SEQS, rawrecs, ["R#"], date=DATE)
    # ... and the other profiles do not read them
    assert _vcf(lib, calls, sites, nr, HAND_NAMES, "raw-graph") == V.vcf_text(HAND_NAMES, HAND_PATHS, HAND_SEQS, raw, ["R#"], date=DATE)
    # a block that is no block is refused
    calls2, keep2 = _pack_norm(recs, 3, [12])
    keep2["norm_block"][0] = 99
    ln = C.c_size_t(0)
    assert not lib.povu_hip_calls_vcf_profile(C.byref(calls2), sites._p, nr, (C.c_char_p * 3)(*[n.encode() for n in HAND_NAMES]), None, None, 1,
                                              H.PROFILES[NR.PROFILE], C.byref(ln))
    del keep, keep2
    lib.povu_hip_call_names_free(nr)
    # the fixture's multi-ALT record
    (names, paths, seqs), texts = _graph(golden_dir, tmp_path, FIXTURE)
    recs, _ = NR.normalise(V.call(V.sites_of_pvst(texts), names, paths, seqs, ["HG1"]), paths, seqs)
    sites, nr = _sites_of_texts(lib, texts), _names(lib, names, ["HG1"])
    calls, keep = _pack_norm(recs, 3, [6])
    got = _vcf(lib, calls, sites, nr, names, NR.PROFILE)
    assert got == NR.vcf_text(names, paths, seqs, recs, ["HG1"], date=DATE)
    assert "\t1\t>3>5:norm\tAA\tA,AAA\t" in got and ";RAW_ALT_INDEX=1,2;" in got and got.rstrip().endswith("RAW_REF=AA;RAW_ALT=A,AAA\tGT\t0\t1\t2")
    del keep
    lib.povu_hip_call_names_free(nr)


def test_cli_reads_the_profile(golden_dir):
    # (what is refused is refused while the arguments are read: no GPU is asked for)
    gfa = os.path.join(golden_dir, "gfa", FIXTURE + ".gfa")
    r = subprocess.run([POVU, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--profile=[raw-graph|top-level-only|popped|left-normalized]" in r.stdout
    # the profile is accepted: the next bad flag is the one named
    for extra in (["--profile", "left-normalized", "--max-level", "x"], ["--profile=left-normalized", "--max-level", "x"]):
        r = subprocess.run([POVU, "call", "-i", gfa, "-P", "HG1"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--max-level" in r.stderr and "--profile" not in r.stderr, extra
    r = subprocess.run([POVU, "call", "-i", gfa, "-P", "HG1", "--profile", "left-normalised"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--profile" in r.stderr and "left-normalized" in r.stderr
    assert H.PROFILES["left-normalized"] == 3 and H.CALL_NORMALIZED == 128
