"""povu_hip_calls_vcf on inversion (POVU_HIP_CALL_SUBR) records without a GPU: hand-packed arrays with SUBR and flubble
records interleaved against the text of the restatement (tests/inversions_ref.py), and the two records the reference states."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import inversions_ref as I
import vcf_ref as V
from povu_amd import hip as H
from test_vcf_writer import _names, _sites_of_texts, _vcf, lib  # noqa: F401  (lib: the fixture)

DATE = "20240229"


def _pack(recs, n_slots, contig_len):
    """The flat arrays of povu_hip_calls for merged yardstick records, one block per record: a flubble record's alleles with
    REF at a position that varies, an inversion record's REF then ALT."""
    n = len(recs)
    u32, u64 = (lambda x: np.ascontiguousarray(x, dtype=np.uint32)), (lambda x: np.ascontiguousarray(x, dtype=np.uint64))
    seq, at, ref_allele, flags, gt, ac = [], [], [], [], [], []
    for i, r in enumerate(recs):
        bases, ats = [r["ref"]] + r["alts"], r["at"]
        subr = r["vartype"] == "SUBR"
        k = 0 if subr else (i + 1) % len(bases)
        order = list(range(1, k + 1)) + [0] + list(range(k + 1, len(bases)))
        seq += [bases[a] for a in order]
        at += [ats[a] for a in order]
        ref_allele.append(k)
        flags.append(H.CALL_SUBR if subr else
                     (H.CALL_ANCHORED if r["vartype"] != "SUB" else 0) | (H.CALL_TANGLED if r["tangled"] else 0) |
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
             at=np.frombuffer("".join(at).encode() + b"\0", np.uint8), contig_len=u64(contig_len),
             n_steps=u32([r["n_steps"] for r in recs]))
    c = H._Calls(n_records=n, n_slots=n_slots, n_blocks=n, n_spelled=len(seq), n_seq_bytes=len(a["seq"]) - 1,
                 n_at_bytes=len(a["at"]) - 1, n_refs=len(contig_len), device_ms=0.0,
                 n_inv_records=sum(1 for r in recs if r["vartype"] == "SUBR"))
    for k, v in a.items():
        setattr(c, k, v.ctypes.data_as(dict(H._Calls._fields_)[k]))
    return c, a


def _check(lib, texts, names, paths, seqs, prefixes):
    recs = I.call(V.sites_of_pvst(texts), names, paths, seqs, prefixes)
    sites = _sites_of_texts(lib, texts)
    nr = _names(lib, names, prefixes)
    refs = V.ref_paths(names, prefixes)
    calls, keep = _pack(recs, nr.contents.refs.n_slots, [sum(len(seqs[x[0]]) for x in paths[r]) for r in refs])
    for only in [None] + list(prefixes):
        want = I.vcf_text(names, paths, seqs, recs, prefixes, date=DATE, only=only)
        for threads in (1, 4):
            assert _vcf(lib, calls, sites, nr, names, DATE, only, threads) == want, (only, threads)
    del keep
    lib.povu_hip_call_names_free(nr)
    return recs


def test_the_flag_and_fields_exist():
    assert H.CALL_SUBR == 16 and H.T_INVERSIONS == 2
    fields = [k for k, _ in H._Calls._fields_]
    assert fields[-5:] == ["n_steps", "n_inv_records", "n_inv_heads", "n_inv_long", "n_inv_tier2"]
    assert fields[fields.index("device_ms") + 1] == "n_steps"  # (appended: the existing offsets stay)


def test_the_pinned_records_without_any_site(lib, golden_dir):
    want = json.load(open(os.path.join(golden_dir, "reference_subr_records.json")))
    for name, rel in want["fixtures"].items():
        names, paths, seqs = V.read_gfa(os.path.join(golden_dir, rel))
        recs = _check(lib, [], names, paths, seqs, [want["reference_prefix"]])  # (sites with n == 0)
        assert [I.record_line(r) for r in recs] == [want["line"]], name


PV = ["H\t0.0.3\t.\t.\t.\nD\t0\t.\t1, 2\t.\nF\t1\t>1>4\t.\tL\nF\t2\t>4>7\t.\tL\n"]
SEQS = {1: "A", 2: "CC", 3: "G", 4: "T", 5: "AAC", 6: "", 7: "G", 8: "TT", 9: "c"}


def _f(ids):
    return [(i, 0) for i in ids]


def _b(ids):
    return [(i, 1) for i in reversed(ids)]


def test_interleaved_subr_and_flubble_records(lib):
    # two bubbles 1 > (2 | 3) > 4 > (5 | 6) > 7 and a tail 8 > 9; the other paths walk stretches of ref backwards
    names = ["r#1#c", "s#1#c", "s#2#c", "t#1#c", "r#1#d"]
    paths = [_f([1, 2, 4, 5, 7, 8, 9]), _f([1, 3, 4, 6, 7]), _b([1, 2]) + _f([4]) + _b([5, 7, 8]) + _f([9]),
             _b([4, 5, 7]) + _b([1, 2]), _b([8, 9]) + _f([1, 2, 4, 6, 7])]
    recs = _check(lib, PV, names, paths, SEQS, ["r#1#c"])
    kinds = [(r["pos"], r["vartype"]) for r in recs]
    assert {"SUB", "SUBR"} <= {k for _, k in kinds} and "SUBR" in [k for _, k in kinds[:-1]] and len(recs) >= 5
    assert any(a[0] == b[0] and a[1] != "SUBR" and b[1] == "SUBR" for a, b in zip(kinds, kinds[1:]))  # one POS, flubble first
    # both references, each prefix alone: r#1#d is inverted by r#1#c in turn
    recs = _check(lib, PV, names, paths, SEQS, ["r#1#c", "r#1#d"])
    assert {r["path"] for r in recs if r["vartype"] == "SUBR"} == {0, 4}
    # a backward reference: the ID of its record is written forward
    recs = _check(lib, PV, names, paths, SEQS, ["t#"])
    assert [r["id"] for r in recs if r["vartype"] == "SUBR" and r["at"][0].startswith("<") and r["at"][0].rfind("<") > 0]


def test_a_subr_record_that_does_not_fit_is_refused(lib):
    names, paths = ["ref", "alt"], [_f([1, 2]), _b([1, 2])]
    recs = I.call([], names, paths, SEQS, ["ref"])
    sites, nr = _sites_of_texts(lib, []), _names(lib, names, ["ref"])
    calls, keep = _pack(recs, 2, [3])
    assert _vcf(lib, calls, sites, nr, names, DATE, None, 1).splitlines()[-1] == \
        "ref\t2\t>1>2\tACC\tGGT\t60\tPASS\tAC=1;AF=0.5;AN=2;NS=2;AT=>1>2,<2<1;VARTYPE=SUBR;TANGLED=F\tGT\t0\t1"
    ln = C.c_size_t(0)
    calls.n_alleles[0] = 3
    assert not lib.povu_hip_calls_vcf(C.byref(calls), sites._p, nr, (C.c_char_p * 2)(b"ref", b"alt"), None, None, 1, C.byref(ln))
    calls.n_alleles[0] = 2
    calls.flags[0] = 0  # a flubble record needs a site
    assert not lib.povu_hip_calls_vcf(C.byref(calls), sites._p, nr, (C.c_char_p * 2)(b"ref", b"alt"), None, None, 1, C.byref(ln))
    del keep
    lib.povu_hip_call_names_free(nr)
