"""The host half of a variant call without a GPU (povu_amd/csrc/host/vcf.cpp through libpovu_hip.so): reference paths and
PanSN slots from names, sites from parsed PVST documents, and the VCF text of records packed into the flat arrays of
povu_hip_calls -- each against the plain-Python restatement (tests/vcf_ref.py), PVST texts from the CPU oracle."""
import ctypes as C
import glob
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import vcf_ref as V
from povu_amd import hip as H
from povu_amd import workloads as W
from test_cabi_and_host import _Doc, _built
from test_oracle import _load_gfa_links
from test_oracle_subflubbles import HAND_TRACED, hand_traced_graph
from test_vcf_ref import PV1, SEQS

DATE = "20240229"
NIL = 0xFFFFFFFF
SITE_FIELDS = ("id1", "or1", "id2", "or2", "parent", "height", "family", "tree")


@pytest.fixture(scope="module")
def lib():
    _built()
    l = H.load_lib()
    l.povu_pvst_parse.restype = C.POINTER(_Doc)
    l.povu_pvst_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    l.povu_pvst_doc_free.argtypes = [C.POINTER(_Doc)]
    return l


def _strings(xs):
    return (C.c_char_p * max(len(xs), 1))(*[x.encode() for x in xs])


def _names(lib, names, prefixes):
    """The library's names record (freed by the caller) or RuntimeError with its message."""
    err = C.create_string_buffer(512)
    r = lib.povu_hip_call_names_make(len(names), _strings(names), len(prefixes), _strings(prefixes), err, 512)
    if not r:
        raise RuntimeError(err.value.decode())
    return r


def _names_tuple(lib, names, prefixes):
    r = _names(lib, names, prefixes)
    x = r.contents
    out = ([x.sample[k].decode() for k in range(x.refs.n_samples)], [x.slot_of_path[k] for k in range(x.n_paths)],
           [x.refs.sample_of_slot[k] for k in range(x.refs.n_slots)], [x.refs.ref_path[k] for k in range(x.refs.n_refs)])
    assert x.n_paths == len(names)
    lib.povu_hip_call_names_free(r)
    return out


def _sites_of_texts(lib, texts):
    """The library's sites (H.Sites) of PVST texts, None when one of them does not parse."""
    docs = []
    for t in texts:
        raw = t.encode() if isinstance(t, str) else t
        docs.append(lib.povu_pvst_parse(raw, len(raw), None, 0))
    try:
        if not all(docs):
            return None
        p = lib.povu_hip_sites_of_docs((C.POINTER(_Doc) * max(len(docs), 1))(*docs), len(docs))
        assert p
        return H.Sites(lib, p)
    finally:
        for d in docs:
            if d:
                lib.povu_pvst_doc_free(d)


def _same_sites(got, want):
    """The library's sites equal the yardstick's, field by field."""
    assert got.n == len(want)
    cols = dict(id1=[w["s"][0] for w in want], or1=[w["s"][1] for w in want], id2=[w["z"][0] for w in want],
                or2=[w["z"][1] for w in want], parent=[NIL if w["parent"] == V.NO_PARENT else w["parent"] for w in want],
                height=[w["height"] for w in want], family=[ord(w["fam"]) for w in want], tree=[w["tree"] for w in want])
    for k in SITE_FIELDS:
        assert getattr(got, k).tolist() == cols[k], k


# ---- names

NAME_SETS = [
    (["R#0#c", "S#1#c", "S#2#c", "T#1#c", "T#1#d"], ["R#"]),                 # the diploid / ambiguous set of test_vcf_ref
    (["G#1#chr1", "G#1#chr2", "H#1#chr1", "H#1#chr2"], ["G#"]),              # its two-contig set
    (["ref", "alt"], ["ref", "alt"]),
    (["one#1", "x#y#z", "x#1y#z", "x##z", "x#2#", "x", "x#0#c", "#3#c"], ["x"]),  # one '#', a non-digit second field, empty fields
    (["s#2#x", "s#1#x", "t#10#a", "t#9#a", "s#1#y", "t#009#b"], ["t#1", "s#1#y"]),  # haps out of order: slots ascend by hap
]


def test_names_match_the_restatement(lib):
    sets = list(NAME_SETS)
    p = W.pansn(W.chain_haplotypes(50, 9, seed=3), samples=4)
    sets.append((list(p.names), ["sample0#1", "sample3"]))
    sets.append((list(W.pansn(W.chain_haplotypes(50, 6, seed=3), samples=6).names), ["sample"]))
    for names, prefixes in sets:
        samples, slot, sample_of = V.slots_of(names)
        assert _names_tuple(lib, names, prefixes) == (samples, slot, sample_of, V.ref_paths(names, prefixes)), names
    # slots of one sample are consecutive and ascend by hap, a name without PanSN form first
    assert _names_tuple(lib, ["s#2#x", "s", "s#1#x"], ["s"])[1:3] == ([2, 0, 1], [0, 0, 0])
    with pytest.raises(RuntimeError, match="^no path name starts with any of the reference prefixes a, b$"):
        _names(lib, ["x#1#c", "y"], ["a", "b"])
    with pytest.raises(V.CallError, match="^no path name starts with any of the reference prefixes a, b$"):
        V.ref_paths(["x#1#c", "y"], ["a", "b"])


# ---- sites of parsed PVST documents

def _fixture_texts(golden_dir, name, tmp_path):
    out = tmp_path / name
    out.mkdir(exist_ok=True)
    n = O.decompose_gfa(os.path.join(golden_dir, "gfa", name + ".gfa"), str(out))
    return [(out / f"{i}.pvst").read_text() for i in range(1, n + 1) if (out / f"{i}.pvst").exists()]


def _golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "reference_vcf_records.json")))


def test_sites_of_docs_match_the_restatement(lib, golden_dir, tmp_path):
    fixtures = sorted(_golden(golden_dir)["fixtures"])
    assert len(fixtures) == 10
    for name in fixtures:
        texts = _fixture_texts(golden_dir, name, tmp_path)
        _same_sites(_sites_of_texts(lib, texts), V.sites_of_pvst(texts))
    parsed = 0
    for path in sorted(glob.glob(os.path.join(golden_dir, "pvst", "*.pvst"))):
        text = open(path).read()
        got = _sites_of_texts(lib, [text])
        if got is not None:
            _same_sites(got, V.sites_of_pvst([text]))
            parsed += 1
    assert parsed >= 10
    # several trees in one forest, and what -s writes: T / O lines, C / M / S lines, a concealed vertex listed under two
    # parents (the last lister is the parent) and a flubble listed under none (no parent, height 0)
    texts = list(O.decompose(W.hprc_shaped([200, 150], seed=21)).values())
    assert len(texts) == 2
    _same_sites(_sites_of_texts(lib, texts), V.sites_of_pvst(texts))
    sub = [O.decompose(hand_traced_graph(k), leaf=2)[1] for k in sorted(HAND_TRACED)]
    sub.append(O.decompose(_load_gfa_links(os.path.join(golden_dir, "gfa", "pvst_tests_graph.gfa")), leaf=2)[1])
    sub += list(O.decompose(W.bubble_zoo(6, 8, 2), leaf=2).values())
    assert set("DFTOCMS") == {ln[0] for t in sub for ln in t.splitlines()[1:]}
    got, want = _sites_of_texts(lib, sub), V.sites_of_pvst(sub)
    _same_sites(got, want)
    assert 0 in got.height.tolist()  # (the flubble under no parent)
    assert _sites_of_texts(lib, []).n == 0


def test_sites_of_a_tree_nested_deeper_than_the_recursion_limit(lib):
    depth = sys.getrecursionlimit() + 500
    rows = ["D\t0\t.\t1\t."] + [f"F\t{k}\t>{k}<{2 * depth - k}\t{k + 1 if k < depth else '.'}\tL" for k in range(1, depth + 1)]
    head = "H\t0.0.3\t.\t.\t.\n"
    # parents before their children: the order the project writes (the restatement's h() then never nests)
    text = head + "\n".join(rows) + "\n"
    got = _sites_of_texts(lib, [text])
    _same_sites(got, V.sites_of_pvst([text]))
    assert got.height.tolist() == list(range(1, depth + 1))
    # every child line before its parent's, the root last: povu_pvst_parse accepts it (children are file ids); the
    # restatement's h() would recurse to the depth, so the heights are counted here
    text = head + "\n".join(reversed(rows)) + "\n"
    got = _sites_of_texts(lib, [text])
    assert got is not None and got.n == depth
    assert got.id1.tolist() == list(range(depth, 0, -1)) and got.or2.tolist() == [1] * depth
    assert got.height.tolist() == list(range(depth, 0, -1))
    assert got.parent.tolist() == list(range(1, depth)) + [NIL]
    assert set(got.family.tolist()) == {ord("F")} and set(got.tree.tolist()) == {0}


# ---- the writer

def _pack(recs, n_slots, contig_len):
    """The flat arrays of povu_hip_calls for yardstick records: one block per record, holding the alleles with REF at a
    position that varies from record to record (ref_allele = k, never 0 for the first record), the others in record order
    around it."""
    n = len(recs)
    u32, u64 = (lambda x: np.ascontiguousarray(x, dtype=np.uint32)), (lambda x: np.ascontiguousarray(x, dtype=np.uint64))
    seq, at, ref_allele, flags, gt, ac = [], [], [], [], [], []
    for i, r in enumerate(recs):
        bases, ats = [r["ref"]] + r["alts"], r["at"]
        assert len(bases) == len(ats) and len(r["slots"]) == n_slots
        k = (i + 1) % len(bases)
        order = list(range(1, k + 1)) + [0] + list(range(k + 1, len(bases)))
        seq += [bases[a] for a in order]
        at += [ats[a] for a in order]
        ref_allele.append(k)
        flags.append((H.CALL_ANCHORED if r["vartype"] != "SUB" else 0) | (H.CALL_TANGLED if r["tangled"] else 0) |
                     (H.CALL_INS if r["vartype"] == "INS" else 0) | (H.CALL_DEL if r["vartype"] == "DEL" else 0))
        gt += [H.GT_MISSING if g is None else g for g in r["slots"]]
        ac += r["ac"]
    off = lambda xs: u64(np.concatenate([[0], np.cumsum([len(x) for x in xs])]))  # noqa: E731
    n_alleles = [1 + len(r["alts"]) for r in recs]
    a = dict(query=u32([r["q"] for r in recs]), path=u32([r["path"] for r in recs]), first=u32([r["first"] for r in recs]),
             ref_allele=u32(ref_allele), n_alleles=u32(n_alleles), an=u32([r["an"] for r in recs]),
             ns=u32([r["ns"] for r in recs]), block=u32(np.arange(n)), pos=u64([r["pos"] for r in recs]),
             flags=np.ascontiguousarray(flags, dtype=np.uint8), ac_off=off([r["ac"] for r in recs]), ac=u32(ac),
             gt=np.ascontiguousarray(gt, dtype=np.uint16), block_off=u64(np.concatenate([[0], np.cumsum(n_alleles)])),
             seq_off=off(seq), at_off=off(at), seq=np.frombuffer("".join(seq).encode() + b"\0", np.uint8),
             at=np.frombuffer("".join(at).encode() + b"\0", np.uint8), contig_len=u64(contig_len))
    c = H._Calls(n_records=n, n_slots=n_slots, n_blocks=n, n_spelled=len(seq), n_seq_bytes=len(a["seq"]) - 1,
                 n_at_bytes=len(a["at"]) - 1, n_refs=len(contig_len), device_ms=0.0)
    for k, v in a.items():
        setattr(c, k, v.ctypes.data_as(dict(H._Calls._fields_)[k]))
    return c, a


def _vcf(lib, calls, sites, names_rec, names, date, only, threads):
    ln = C.c_size_t(0)
    p = lib.povu_hip_calls_vcf(C.byref(calls), sites._p, names_rec, _strings(names), date.encode() if date else None,
                               only.encode() if only is not None else None, threads, C.byref(ln))
    assert p
    s = C.string_at(p, ln.value).decode()
    lib.povu_hip_buffer_free(p)
    return s


def _check_writer(lib, texts, names, paths, seqs, prefixes):
    """povu_hip_calls_vcf of the packed yardstick records == the yardstick's text, byte for byte: every reference and each
    prefix alone, on 1 and 4 threads.  Returns the records."""
    recs = V.call(V.sites_of_pvst(texts), names, paths, seqs, prefixes)
    sites = _sites_of_texts(lib, texts)
    nr = _names(lib, names, prefixes)
    refs = V.ref_paths(names, prefixes)
    calls, keep = _pack(recs, nr.contents.refs.n_slots, [sum(len(seqs[x[0]]) for x in paths[r]) for r in refs])
    for only in [None] + list(prefixes):
        want = V.vcf_text(names, paths, seqs, recs, prefixes, date=DATE, only=only)
        for threads in (1, 4):
            assert _vcf(lib, calls, sites, nr, names, DATE, only, threads) == want, (only, threads)
    today = _vcf(lib, calls, sites, nr, names, None, None, 1).split("\n", 2)  # (date NULL: today's, eight digits)
    assert today[1][:11] == "##fileDate=" and len(today[1]) == 19 and today[1][11:].isdigit()
    assert today[2] == V.vcf_text(names, paths, seqs, recs, prefixes).split("\n", 2)[2]
    del keep
    lib.povu_hip_call_names_free(nr)
    return recs


def test_writer_on_the_ten_fixtures(lib, golden_dir, tmp_path):
    want = _golden(golden_dir)
    assert len(want["fixtures"]) == 10
    total = 0
    for name in sorted(want["fixtures"]):
        names, paths, seqs = V.read_gfa(os.path.join(golden_dir, "gfa", name + ".gfa"))
        total += len(_check_writer(lib, _fixture_texts(golden_dir, name, tmp_path), names, paths, seqs, [want["reference_prefix"]]))
    assert total >= 10


PV2 = PV1 + ["H\t0.0.3\t.\t.\t.\nD\t0\t.\t1\t.\nF\t1\t>11>14\t.\tL\n"]
SEQS2 = {**SEQS, **{k + 10: v for k, v in SEQS.items()}}
HAND = [  # the four hand cases of test_vcf_ref.py
    (PV1, ["ref", "alt"], [[(4, 1), (3, 1), (1, 1)], [(1, 0), (2, 0), (4, 0)]], SEQS, ["ref"]),
    (PV1, ["R#0#c", "S#1#c", "S#2#c", "T#1#c", "T#1#d"],
     [[(1, 0), (3, 0), (4, 0)], [(1, 0), (2, 0), (4, 0)], [(1, 0), (3, 0), (4, 0)], [(1, 0), (2, 0), (4, 0)], [(1, 0), (3, 0), (4, 0)]],
     SEQS, ["R#"]),
    (PV1, ["ref", "a", "b"], [[(1, 0), (2, 0), (4, 0)], [(1, 0), (4, 0)], [(1, 0), (3, 0), (4, 0)]], SEQS, ["ref"]),
    (PV2, ["G#1#chr1", "G#1#chr2", "H#1#chr1", "H#1#chr2"],
     [[(1, 0), (2, 0), (4, 0)], [(11, 0), (12, 0), (14, 0)], [(1, 0), (3, 0), (4, 0)], [(11, 0), (13, 0), (14, 0)]], SEQS2,
     ["G#1#chr1", "G#1#chr2"]),
]


def test_writer_on_the_hand_cases(lib):
    for texts, names, paths, seqs, prefixes in HAND:
        assert _check_writer(lib, texts, names, paths, seqs, prefixes)
    # the two-contig case with one prefix for both contigs, as test_vcf_ref.py states it
    texts, names, paths, seqs, _ = HAND[3]
    assert len(_check_writer(lib, texts, names, paths, seqs, ["G#"])) == 2


def test_writer_on_several_thread_chunks(lib):
    k = 6000
    g = W.chain_of_bubbles(k)
    p = W.pansn(W.chain_haplotypes(k, 8, seed=5), samples=4)
    names, paths = list(p.names), [p.steps(i) for i in range(len(p))]
    seqs = dict(zip(g.vid.tolist(), W.random_sequences(g, 5, max_len=12)))
    texts = list(O.decompose(g).values())
    recs = _check_writer(lib, texts, names, paths, seqs, ["sample0#1"])
    assert len(recs) > 4096  # (at least 1024 records a thread: four threads get a chunk each)
    assert {"INS", "DEL"} <= {r["vartype"] for r in recs} and any(len(r["alts"]) > 1 for r in recs)


def test_writer_on_a_record_whose_called_slots_all_carry_ref(lib):
    texts, names, paths, seqs, prefixes = HAND[2]
    rec = dict(path=0, q=0, first=0, chrom="ref", pos=2, id=">1>4", ref="CGGT", alts=["C"], at=[">1>2", ">1"], vartype="DEL",
               tangled=False, lv=0, gt=["0", "0", "."], slots=[0, 0, None], ac=[0], an=2, ns=2)
    sites, nr = _sites_of_texts(lib, texts), _names(lib, names, prefixes)
    calls, keep = _pack([rec], 3, [7])
    got = _vcf(lib, calls, sites, nr, names, DATE, None, 1)
    assert got == V.vcf_text(names, paths, seqs, [rec], prefixes, date=DATE)
    assert got.splitlines()[-1] == ("ref\t2\t>1>4\tCGGT\tC\t60\tPASS\tAC=0;AF=0.0;AN=2;NS=2;AT=>1>2,>1;VARTYPE=DEL;TANGLED=F;"
                                    "ES=>1>4;LV=0\tGT\t0\t0\t.")
    # arguments that do not belong together are refused, not read out of bounds
    calls.query[0] = 5
    ln = C.c_size_t(0)
    assert not lib.povu_hip_calls_vcf(C.byref(calls), sites._p, nr, _strings(names), None, None, 1, C.byref(ln))
    del keep
    lib.povu_hip_call_names_free(nr)
