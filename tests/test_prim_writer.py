"""The host writer under POVU_HIP_PROFILE_DECOMPOSED (povu_hip_calls_vcf_profile) on hand-packed records and rows against the
restatement's text (tests/prim_ref.py): primitives of every kind, ALTs kept whole, a record that stays the raw line, a SUBR
record, several threads, one prefix of two; without row arrays the raw records; rows that point outside their texts are
refused.  No GPU."""
import ctypes as C

import numpy as np

import inversions_ref as I
import prim_ref as PR
import vcf_ref as V
from povu_amd import hip as H
from test_nested_ref import _pack, _vcf
from test_norm_ref import HAND_NAMES, HAND_PATHS, HAND_PVST, HAND_SEQS, _graph
from test_vcf_writer import DATE, _names, _sites_of_texts, lib  # noqa: F401  (lib: the fixture)

VCFWAVE = "downstream_repetitive/vcfwave-complex-decomposition"
SUBR = "downstream_repetitive/subr-inversion-preservation"
_FIELDS = dict(H._Calls._fields_ + H._CallsNested._fields_)
_ROW_U32 = ("row_record", "row_alt", "row_index", "row_ref_start", "row_ref_len", "row_alt_start", "row_alt_len", "row_ac", "row_an", "row_ns")


def _pack_rows(recs, rows, counters, n_slots, contig_len):
    """povu_hip_calls of raw records (packed as test_nested_ref packs a plain call's) and the rows of prim_ref.decompose."""
    rawlike = [dict(r, ref_class=0, n_classes=1 + len(r["alts"]), ref_is_rep=True, collapsed=False, rescued=False, parent=None,
                    lv=r["lv"] or 0) for r in recs]
    c, a = _pack(rawlike, n_slots, contig_len, nested=False)
    a["flags"] = a["flags"] | np.array([H.CALL_SUBR if r["vartype"] == "SUBR" else 0 for r in recs], np.uint8)
    a["n_steps"] = np.zeros(len(recs), np.uint32)
    key = dict(row_record="rec", row_alt="alt", row_index="index", row_ref_start="ref_start", row_ref_len="ref_len", row_alt_start="alt_start",
               row_alt_len="alt_len", row_ac="ac", row_an="an", row_ns="ns")
    for k in _ROW_U32:
        a[k] = np.ascontiguousarray([r[key[k]] for r in rows], np.uint32)
    a["row_kind"] = np.ascontiguousarray([r["kind"] for r in rows], np.uint8)
    a["row_reason"] = np.ascontiguousarray([r["reason"] for r in rows], np.uint8)
    a["row_lead"] = np.ascontiguousarray([ord(r["lead"]) if r["lead"] else 0 for r in rows], np.uint8)
    a["row_pos"] = np.ascontiguousarray([r["pos"] for r in rows], np.uint64)
    for k in ("flags", "n_steps", "row_kind", "row_reason", "row_lead", "row_pos") + _ROW_U32:
        setattr(c, k, a[k].ctypes.data_as(_FIELDS[k]))
    c.n_rows = len(rows)
    c.n_decomposed_alts, c.n_passthrough_alts, c.n_prim_cells = counters["n_decomposed_alts"], counters["n_passthrough_alts"], counters["n_prim_cells"]
    return c, a


def test_writer_rows_of_every_kind(lib):
    vsites = V.sites_of_pvst([HAND_PVST])
    raw = V.call(vsites, HAND_NAMES, HAND_PATHS, HAND_SEQS, ["R#"])
    assert [(r["pos"], r["ref"], r["alts"]) for r in raw] == [(5, "AA", ["A"]), (8, "G", ["T"]), (10, "TA", ["GA"])]
    rows, counters = PR.decompose(raw, HAND_NAMES, HAND_PATHS, HAND_SEQS)
    # the deletion's gap goes to offset 0 (anchored on the base in front of POS), the SNP is its raw record, the substitution
    # with a common last base is one SNP (not the raw record: its texts are shorter)
    assert [(r["kind"], r["pos"], r["lead"]) for r in rows] == [(PR.ROW_DEL, 4, "A"), (PR.ROW_RAW, 8, ""), (PR.ROW_SNP, 10, "")]
    sites, nr = _sites_of_texts(lib, [HAND_PVST]), _names(lib, HAND_NAMES, ["R#"])
    calls, keep = _pack_rows(raw, rows, counters, 3, [12])
    want = PR.vcf_text(HAND_NAMES, HAND_PATHS, HAND_SEQS, raw, rows, ["R#"], date=DATE)
    assert "\t4\t>3>5:1:del1\tAA\tA\t" in want and "\t8\t>5>8\tG\tT\t" in want and "\t10\t>8>11:1:snp1\tT\tG\t" in want
    assert want.count("DECOMPOSED=T") == 2 and ";ES=>5>8;LV=0\t" in want and want.count(";ES=") == 1
    for threads in (1, 4):
        assert _vcf(lib, calls, sites, nr, HAND_NAMES, PR.PROFILE, threads=threads) == want
    # NULL row arrays (a hand-made povu_hip_calls of before): the raw records under the profile's header lines
    calls.row_record = None
    rawtext = V.vcf_text(HAND_NAMES, HAND_PATHS, HAND_SEQS, raw, ["R#"], date=DATE)
    assert _vcf(lib, calls, sites, nr, HAND_NAMES, PR.PROFILE) == rawtext.replace("##contig", PR.PROFILE_LINES + "##contig", 1)
    # ... and the other profiles do not read the rows
    calls2, keep2 = _pack_rows(raw, rows, counters, 3, [12])
    assert _vcf(lib, calls2, sites, nr, HAND_NAMES, "raw-graph") == rawtext
    # a row that reaches behind its text, an ALT the record does not have, a record that is none: refused
    ln = C.c_size_t(0)
    for k, v in (("row_ref_len", 3), ("row_alt", 2), ("row_alt", 0), ("row_record", 3), ("row_kind", 5)):
        calls3, keep3 = _pack_rows(raw, rows, counters, 3, [12])
        keep3[k][0] = v
        assert not lib.povu_hip_calls_vcf_profile(C.byref(calls3), sites._p, nr, (C.c_char_p * 3)(*[n.encode() for n in HAND_NAMES]), None, None, 1,
                                                  H.PROFILES[PR.PROFILE], C.byref(ln)), k
    del keep, keep2
    lib.povu_hip_call_names_free(nr)


def test_writer_on_the_fixtures(lib, golden_dir, tmp_path):
    (names, paths, seqs), texts = _graph(golden_dir, tmp_path, VCFWAVE)
    raw = V.call(V.sites_of_pvst(texts), names, paths, seqs, ["HG1"])
    sites, nr = _sites_of_texts(lib, texts), _names(lib, names, ["HG1"])
    for cap in (8, 0):
        rows, counters = PR.decompose(raw, names, paths, seqs, max_allele_length=cap)
        calls, keep = _pack_rows(raw, rows, counters, 3, [5])
        got = _vcf(lib, calls, sites, nr, names, PR.PROFILE)
        assert got == PR.vcf_text(names, paths, seqs, raw, rows, ["HG1"], date=DATE)
        if cap:
            assert "\t2\t>9>14:1:snp1\tC\tT\t" in got and "\t4\t>9>14:1:snp2\tT\tA\t" in got and got.count("\tGT\t0\t1\t.\n") == 2
            assert "\t2\t>9>14:2:passthrough\tCGT\tCGTACGTACGTA\t" in got and got.count("\tGT\t0\t.\t1\n") == 1
            assert "PASSTHROUGH=T;PASS_THROUGH_REASON=max_allele_length;RAW_POS=2;RAW_REF=CGT;RAW_ALT=CGTACGTACGTA\t" in got
        else:
            assert "\t1\t>9>14:2:ins1\tA\tACGTACGTA\t" in got and "\t4\t>9>14:2:ins2\tT\tTA\t" in got
        del keep
    lib.povu_hip_call_names_free(nr)
    # the SUBR record passes through whole
    (names, paths, seqs), texts = _graph(golden_dir, tmp_path, SUBR)
    raw = I.call(V.sites_of_pvst(texts), names, paths, seqs, ["ref"])
    rows, counters = PR.decompose(raw, names, paths, seqs)
    sites, nr = _sites_of_texts(lib, texts), _names(lib, names, ["ref"])
    calls, keep = _pack_rows(raw, rows, counters, 2, [sum(len(seqs[x[0]]) for x in paths[0])])
    got = _vcf(lib, calls, sites, nr, names, PR.PROFILE)
    assert got == PR.vcf_text(names, paths, seqs, raw, rows, ["ref"], raw_line=I.record_line, date=DATE)
    assert ":subr-passthrough\t" in got and got.splitlines()[-1].split("\t")[7].endswith("PASS_THROUGH_REASON=subr_inversion_preservation;SUBR_ORIGIN=T")
    del keep
    lib.povu_hip_call_names_free(nr)
