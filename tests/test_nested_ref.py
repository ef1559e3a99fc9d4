"""The plain-Python restatement of the nested calls (tests/nested_ref.py) against the records the reference's
popped-parent-child-rescue fixture states for its three profiles (tests/golden/reference_nested_records.json), on hand
cases for what the fixture does not reach, and the host writer (povu_hip_calls_vcf_profile) on hand-packed records of
each profile against the restatement's text.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nested_ref as N
import oracle_lib as O
import vcf_ref as V
from povu_amd import hip as H
from povu_amd import workloads as W
from test_vcf_writer import DATE, _names, _sites_of_texts, _strings, lib  # noqa: F401  (lib: the fixture)

FIXTURE = "downstream_repetitive/popped-parent-child-rescue"
PLAIN_KEYS = ("path", "q", "first", "chrom", "pos", "id", "ref", "alts", "at", "vartype", "tangled", "lv", "gt", "slots", "ac", "an",
              "ns")


def _pvst_texts(gfa, out):
    out.mkdir(exist_ok=True)
    n = O.decompose_gfa(gfa, str(out))
    return [(out / f"{i}.pvst").read_text() for i in range(1, n + 1) if (out / f"{i}.pvst").exists()]


def _fixture(golden_dir, tmp_path):
    gfa = os.path.join(golden_dir, "gfa", FIXTURE + ".gfa")
    texts = _pvst_texts(gfa, tmp_path / "fx")
    return V.read_gfa(gfa), texts


def _golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "reference_nested_records.json")))


def test_fixture_records_of_the_three_profiles(golden_dir, tmp_path):
    want = _golden(golden_dir)
    (names, paths, seqs), texts = _fixture(golden_dir, tmp_path)
    sites = V.sites_of_pvst(texts)
    # the oracle's PVST is flat here: both sites are children of the root, nesting comes from the traversals alone
    assert sorted(V.label(s["s"], s["z"]) for s in sites) == [">0>5", ">2>4"] and {s["height"] for s in sites} == {1}
    assert set(want["profiles"]) == set(N.PROFILES)
    for profile, rows in sorted(want["profiles"].items()):
        opts = want["popped_options"] if profile == "popped" else {}
        recs = N.call(sites, names, paths, seqs, [want["reference_prefix"]], profile=profile, **opts)
        assert len(recs) == len(rows), profile
        for r, w in zip(recs, rows):
            got = dict(chrom=r["chrom"], id=r["id"], ref=r["ref"], alts=r["alts"], ac=r["ac"], an=r["an"], ns=r["ns"], at=r["at"],
                       vartype=r["vartype"], tangled="T" if r["tangled"] else "F", es=r["es"], lv=r["lv"], gt=r["gt"],
                       info=dict(r["info"]))
            assert got == {k: w[k] for k in got}, (profile, w["source"])
            for c, f in zip(r["ac"], w["af"]):  # this project writes %.1f
                assert abs(float("%.1f" % (c / r["an"])) - f) <= 0.05
            if w["es"] == ">0>5":
                assert r["pos"] == w["pos"] == 1
            else:
                # The fixture's hand-written POS of >2>4 is 3.  REF there is segment 3 alone (not anchored), the fourth base
                # of HG1#1#chr1 (0+,1+,2+,3+, one base each), and the 1-based "first replaced base" that the reference's own
                # minimal-substitution and two-ordered-substitutions records use (reference_vcf_records.json, matched by
                # vcf_ref) makes that POS 4.
                assert w["pos"] == 3 and r["pos"] == 4
        text = N.vcf_text(names, paths, seqs, recs, [want["reference_prefix"]], profile=profile)
        assert text.count("##INFO=<ID=PS,") == 1
        for k, d in want["info_descriptions"].items():
            assert (f'##INFO=<ID={k},Number=1,Type=String,Description="{d}">' in text) == (k in N.PROFILE_KEYS.get(profile, ())), k
        head = text.splitlines()
        assert head[len(V.HEADER.splitlines())].startswith("##INFO=<ID=PS,")  # after the verbatim reference header
        assert [ln.split("\t")[9:] for ln in head if ln.startswith("#CHROM")] == [want["samples"]]
    raw, counters = N.call_full(sites, names, paths, seqs, ["HG1"])
    assert counters == dict(n_enclosed=1, n_collapsed_sites=1, n_popped=0, n_rescued=0)
    assert [(r["es"], r["ps"], r["collapsed"], r["n_classes"]) for r in raw] == [(">0>5", None, True, 2), (">2>4", ">0>5", False, 2)]
    assert N.record_line(raw[1]).split("\t")[7].endswith(";ES=>2>4;LV=1;PS=>0>5")
    _, counters = N.call_full(sites, names, paths, seqs, ["HG1"], profile="popped", **want["popped_options"])
    assert (counters["n_popped"], counters["n_rescued"]) == (1, 1)
    # the plain call makes the SNP haplotype an allele of its own at the outer site: what the nested call is for
    plain = V.call(sites, names, paths, seqs, ["HG1"])
    assert (plain[0]["ref"], plain[0]["alts"], plain[0]["gt"]) == ("AAAAA", ["A", "AAAGA"], ["0", "1", "2"])


def test_without_enclosure_the_records_are_the_plain_ones():
    k = 40
    g = W.chain_of_bubbles(k)
    p = W.pansn(W.chain_haplotypes(k, 6, seed=2), samples=3)
    names, paths = list(p.names), [p.steps(i) for i in range(len(p))]
    seqs = dict(zip(g.vid.tolist(), W.random_sequences(g, 2, max_len=6)))
    sites = V.sites_of_pvst(list(O.decompose(g).values()))
    plain = V.call(sites, names, paths, seqs, ["sample0#1"])
    recs, counters = N.call_full(sites, names, paths, seqs, ["sample0#1"])
    assert len(plain) > 10 and len(recs) == len(plain)
    for r, w in zip(recs, plain):
        assert {k: r[k] for k in PLAIN_KEYS} == w
        assert r["level"] == w["lv"] and r["parent"] is None and r["ps"] is None and not r["collapsed"] and r["ref_is_rep"]
    assert counters == dict(n_enclosed=0, n_collapsed_sites=0, n_popped=0, n_rescued=0)
    assert N.vcf_text(names, paths, seqs, recs, ["sample0#1"]) == V.vcf_text(names, paths, seqs, plain, ["sample0#1"]).replace(
        "##contig", N.PS_LINE + "##contig", 1)


def test_reversed_reference_path(golden_dir, tmp_path):
    (names, paths, seqs), texts = _fixture(golden_dir, tmp_path)
    sites = V.sites_of_pvst(texts)
    paths = [[N.TR.flip(x) for x in reversed(paths[0])]] + paths[1:]  # HG1 reads the graph from 5 to 0
    recs = N.call(sites, names, paths, seqs, ["HG1"])
    # reverse strand: <5 spells G; the deletion is anchored on it: REF = G + TTTT at POS 1; the SNP is revcomp(A) -> revcomp(G)
    assert [(r["es"], r["pos"], r["ref"], r["alts"], r["at"], r["gt"], r["lv"], r["ps"]) for r in recs] == [
        (">0>5", 1, "GTTTT", ["G"], ["<5<4<3<2<1", "<5"], ["0", "1", "0"], 0, None),
        (">2>4", 3, "T", ["C"], ["<3", "<6"], ["0", ".", "1"], 1, ">0>5")]
    assert recs[0]["tangled"] and recs[0]["collapsed"] and not recs[1]["tangled"]


def test_ref_is_not_the_representative_of_its_class(golden_dir, tmp_path):
    (names, paths, seqs), texts = _fixture(golden_dir, tmp_path)
    sites = V.sites_of_pvst(texts)
    recs = N.call(sites, names, paths, seqs, ["HG1", "HG3"])
    outer = [r for r in recs if r["es"] == ">0>5"]
    assert [r["chrom"] for r in outer] == ["HG1#1#chr1", "HG3#1#chr1"]
    # both references carry class 0 of >0>5; HG3's exact allele (through the SNP's ALT) is not its representative, and REF
    # must spell the reference
    assert [(r["ref"], r["alts"], r["at"], r["ref_class"], r["ref_is_rep"], r["gt"]) for r in outer] == [
        ("AAAAA", ["A"], [">0>1>2>3>4", ">0"], 0, True, ["0", "1", "0"]),
        ("AAAGA", ["A"], [">0>1>2>6>4", ">0"], 0, False, ["0", "1", "0"])]
    inner = [r for r in recs if r["es"] == ">2>4"]
    assert [(r["chrom"], r["ref"], r["alts"], r["gt"], r["lv"], r["ps"]) for r in inner] == [
        ("HG1#1#chr1", "A", ["G"], ["0", ".", "1"], 1, ">0>5"), ("HG3#1#chr1", "G", ["A"], ["1", ".", "0"], 1, ">0>5")]


# a deletion 0 -> 9 around a chain that holds a deletion 2 -> 7 around a chain that holds the SNP >4>6; one base a segment
DEPTH2_SITES = [V._site((0, 0), (9, 0), V.NO_PARENT, 1, "F", 0), V._site((2, 0), (7, 0), V.NO_PARENT, 1, "F", 0),
                V._site((4, 0), (6, 0), V.NO_PARENT, 1, "F", 0)]
DEPTH2_NAMES = ["R#1#c", "A#1#c", "B#1#c", "D#1#c"]
DEPTH2_PATHS = [[(k, 0) for k in range(10)], [(0, 0), (9, 0)], [(k, 0) for k in (0, 1, 2, 7, 8, 9)],
                [(k, 0) for k in (0, 1, 2, 3, 4, 10, 6, 7, 8, 9)]]
DEPTH2_SEQS = {k: "ACGTACGTACG"[k] for k in range(11)}


def test_depth_two_chain_levels_and_rescue():
    a = (DEPTH2_SITES, DEPTH2_NAMES, DEPTH2_PATHS, DEPTH2_SEQS, ["R#"])
    raw, counters = N.call_full(*a)
    assert [(r["es"], r["lv"], r["ps"], r["n_classes"], r["collapsed"]) for r in raw] == [
        (">0>9", 0, None, 2, True), (">2>7", 1, ">0>9", 2, True), (">4>6", 2, ">2>7", 2, False)]
    assert [r["gt"] for r in raw] == [["0", "1", "0", "0"], ["0", ".", "1", "0"], ["0", ".", ".", "1"]]
    assert counters == dict(n_enclosed=2, n_collapsed_sites=2, n_popped=0, n_rescued=0)
    # REF of >0>9 spells 9 bases, of >2>7 5, of >4>6 1.  Limit 4: both deletions are popped, the grandchild is rescued
    # through two popped ancestors; the child >2>7 is reached but big itself, so it is not rescued
    recs, counters = N.call_full(*a, profile="popped", max_level=0, max_ref_length=4, max_allele_length=4)
    assert [(r["id"], r["rescued"], dict(r["info"])["POPPED_PARENT"]) for r in recs] == [(">4>6:rescued", True, ">2>7")]
    assert (counters["n_popped"], counters["n_rescued"]) == (2, 1)
    # limit 6: only the outer deletion is popped; its child is rescued, and the grandchild's parent is kept, so it is not reached
    recs, counters = N.call_full(*a, profile="popped", max_level=0, max_ref_length=6)
    assert [(r["id"], r["rescued"]) for r in recs] == [(">2>7:rescued", True)]
    assert (counters["n_popped"], counters["n_rescued"]) == (1, 1)
    # no limit: nothing is big, only level 0 is reached and passes through; max_level 1 reaches one more
    recs = N.call(*a, profile="popped")
    assert [(r["id"], dict(r["info"])) for r in recs] == [(">0>9", dict(ORIGIN=">0>9", PROFILE="popped", PASSTHROUGH="T"))]
    assert [r["id"] for r in N.call(*a, profile="popped", max_level=1)] == [">0>9", ">2>7"]
    assert [r["id"] for r in N.call(*a, profile="top-level-only")] == [">0>9:top"]
    # the allele-length limit alone: the ALT of the SNP is short, REF of the deletions long
    recs = N.call(*a, profile="popped", max_allele_length=4)
    assert [r["id"] for r in recs] == [">4>6:rescued"]
    with pytest.raises(V.CallError):
        N.call(*a, profile="flat")


def test_skip_nested_reaches_collapsed_sites():
    for units, depth, haps in ((30, 1, 8), (10, 2, 12)):
        g = W.skip_nested(units, depth, seed=1)
        p = W.skip_haplotypes(units, depth, haps, seed=1)
        names, paths = list(p.names), [p.steps(i) for i in range(len(p))]
        seqs = dict(zip(g.vid.tolist(), W.random_sequences(g, 1, max_len=4)))
        sites = V.sites_of_pvst(list(O.decompose(g).values()))
        recs, counters = N.call_full(sites, names, paths, seqs, [names[0]])
        with_records = {r["q"] for r in recs}
        assert len(with_records) >= 10 and 5 * len({r["q"] for r in recs if r["collapsed"]}) >= len(with_records)
        assert max(r["lv"] for r in recs) >= depth


# ---- the host writer on hand-packed records

def _pack(recs, n_slots, contig_len, nested=True):
    """povu_hip_calls of nested_ref records: one block per record with a spelled allele per class in class order (the REF
    class holds 'N' when REF is not its representative: the writer must not read it), the REFs that are no representative
    spelled after all blocks; level, parent_query, ref_spelled as the device writes them."""
    n = len(recs)
    u32, u64 = (lambda x: np.ascontiguousarray(x, dtype=np.uint32)), (lambda x: np.ascontiguousarray(x, dtype=np.uint64))
    seq, at, gt, ac, flags, extra = [], [], [], [], [], []
    block_off = [0]
    for r in recs:
        rc, alts, alt_at = r["ref_class"], list(r["alts"]), list(r["at"][1:])
        for c in range(r["n_classes"]):
            own = c == rc and r["ref_is_rep"]
            seq.append("N" if c == rc and not own else r["ref"] if own else alts.pop(0))
            at.append(">0" if c == rc and not own else r["at"][0] if own else alt_at.pop(0))
        block_off.append(len(seq))
        flags.append((H.CALL_ANCHORED if r["vartype"] != "SUB" else 0) | (H.CALL_TANGLED if r["tangled"] else 0) |
                     (H.CALL_INS if r["vartype"] == "INS" else 0) | (H.CALL_DEL if r["vartype"] == "DEL" else 0) |
                     (H.CALL_COLLAPSED if r["collapsed"] else 0) | (H.CALL_RESCUED if r["rescued"] else 0))
        gt += [H.GT_MISSING if g is None else g for g in r["slots"]]
        ac += r["ac"]
    ref_spelled = []
    for i, r in enumerate(recs):
        if r["ref_is_rep"]:
            ref_spelled.append(block_off[i] + r["ref_class"])
        else:
            ref_spelled.append(len(seq))
            seq.append(r["ref"])
            at.append(r["at"][0])
    off = lambda xs: u64(np.concatenate([[0], np.cumsum([len(x) for x in xs])]))  # noqa: E731
    a = dict(query=u32([r["q"] for r in recs]), path=u32([r["path"] for r in recs]), first=u32([r["first"] for r in recs]),
             ref_allele=u32([r["ref_class"] for r in recs]), n_alleles=u32([r["n_classes"] for r in recs]),
             an=u32([r["an"] for r in recs]), ns=u32([r["ns"] for r in recs]), block=u32(np.arange(n)),
             pos=u64([r["pos"] for r in recs]), flags=np.ascontiguousarray(flags, dtype=np.uint8), ac_off=off([r["ac"] for r in recs]),
             ac=u32(ac), gt=np.ascontiguousarray(gt, dtype=np.uint16), block_off=u64(block_off), seq_off=off(seq), at_off=off(at),
             seq=np.frombuffer("".join(seq).encode() + b"\0", np.uint8), at=np.frombuffer("".join(at).encode() + b"\0", np.uint8),
             contig_len=u64(contig_len), level=u32([r["lv"] for r in recs]),
             parent_query=u32([0xFFFFFFFF if r["parent"] is None else r["parent"] for r in recs]), ref_spelled=u64(ref_spelled))
    c = H._CallsNested(n_records=n, n_slots=n_slots, n_blocks=n, n_spelled=len(seq), n_seq_bytes=len(a["seq"]) - 1,
                 n_at_bytes=len(a["at"]) - 1, n_refs=len(contig_len), device_ms=0.0, nested=1 if nested else 0)
    for k, v in a.items():
        setattr(c, k, v.ctypes.data_as(dict(H._Calls._fields_ + H._CallsNested._fields_)[k]))
    return c, a


def _vcf(lib, calls, sites, names_rec, names, profile, only=None, threads=1):
    ln = C.c_size_t(0)
    p = lib.povu_hip_calls_vcf_profile(C.byref(calls), sites._p, names_rec, _strings(names), DATE.encode(),
                                       only.encode() if only is not None else None, threads, H.PROFILES[profile], C.byref(ln))
    assert p
    s = C.string_at(p, ln.value).decode()
    lib.povu_hip_buffer_free(p)
    return s


def test_writer_on_each_profile(lib, golden_dir, tmp_path):
    (names, paths, seqs), texts = _fixture(golden_dir, tmp_path)
    vsites, sites = V.sites_of_pvst(texts), _sites_of_texts(lib, texts)
    for prefixes in (["HG1"], ["HG1", "HG3"]):
        nr = _names(lib, names, prefixes)
        contig = [sum(len(seqs[x[0]]) for x in paths[r]) for r in V.ref_paths(names, prefixes)]
        for profile in N.PROFILES:
            recs = N.call(vsites, names, paths, seqs, prefixes, profile=profile, max_ref_length=4, max_allele_length=4)
            assert recs
            calls, keep = _pack(recs, 3, contig)
            for only in [None] + prefixes:
                want = N.vcf_text(names, paths, seqs, recs, prefixes, date=DATE, only=only, profile=profile)
                for threads in (1, 4):
                    assert _vcf(lib, calls, sites, nr, names, profile, only, threads) == want, (profile, only)
            del keep
        lib.povu_hip_call_names_free(nr)
    # a plain call's records through the new entry: arrays absent (NULL), not nested -- today's text, byte for byte
    plain = V.call(vsites, names, paths, seqs, ["HG1"])
    for r in plain:
        r.update(ref_class=0, n_classes=1 + len(r["alts"]), ref_is_rep=True, collapsed=False, rescued=False, parent=None)
    calls, keep = _pack(plain, 3, [6], nested=False)
    calls.level = calls.parent_query = None
    calls.ref_spelled = None
    nr = _names(lib, names, ["HG1"])
    assert _vcf(lib, calls, sites, nr, names, "raw-graph") == V.vcf_text(names, paths, seqs, plain, ["HG1"], date=DATE)
    ln = C.c_size_t(0)
    assert not lib.povu_hip_calls_vcf_profile(C.byref(calls), sites._p, nr, _strings(names), None, None, 1, 7, C.byref(ln))
    del keep
    lib.povu_hip_call_names_free(nr)


def test_writer_on_the_depth_two_chain(lib):
    pvst = "H\t0.0.3\t.\t.\t.\nD\t0\t.\t1, 2, 3\t.\nF\t1\t>0>9\t.\tL\nF\t2\t>2>7\t.\tL\nF\t3\t>4>6\t.\tL\n"
    assert V.sites_of_pvst([pvst]) == DEPTH2_SITES
    sites, nr = _sites_of_texts(lib, [pvst]), _names(lib, DEPTH2_NAMES, ["R#"])
    for profile, kw in (("raw-graph", {}), ("top-level-only", {}), ("popped", dict(max_ref_length=4)), ("popped", dict(max_ref_length=6)),
                        ("popped", dict(max_level=1))):
        recs = N.call(DEPTH2_SITES, DEPTH2_NAMES, DEPTH2_PATHS, DEPTH2_SEQS, ["R#"], profile=profile, **kw)
        calls, keep = _pack(recs, 4, [10])
        assert _vcf(lib, calls, sites, nr, DEPTH2_NAMES, profile) == N.vcf_text(DEPTH2_NAMES, DEPTH2_PATHS, DEPTH2_SEQS, recs, ["R#"],
                                                                               date=DATE, profile=profile), (profile, kw)
        del keep
    lib.povu_hip_call_names_free(nr)


def test_cli_refuses_bad_profile_options(lib, golden_dir):
    # (refused while the arguments are read: no GPU is asked for)
    import subprocess
    povu = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "povu_amd", "bin", "povu")
    gfa = os.path.join(golden_dir, "gfa", FIXTURE + ".gfa")
    for extra, word in ((["--profile", "flat"], "--profile"), (["--profile=deep"], "--profile"), (["--max-level", "x"], "--max-level"),
                        (["--max-ref-length=-1"], "--max-ref-length"), (["--max-allele-length"], "--max-allele-length"),
                        (["--nested", "--gpus", "2"], "--gpus")):
        r = subprocess.run([povu, "call", "-i", gfa, "-P", "HG1"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr, extra
