"""The host writer on merged rows (povu_hip_calls_vcf_profile under POVU_HIP_PROFILE_DECOMPOSED with mrow_* set) on hand-packed
records, rows and merged rows against the restatement's text (tests/merge_ref.py): groups of one and of many, a _ROW_RAW row
as a member and as the representative, a row kept whole, several threads, one prefix of two; with NULL merged arrays the rows
as before; member indices and offsets that point outside the rows are refused.  No GPU."""
import ctypes as C

import numpy as np

import merge_cases as MC
import merge_ref as MR
import oracle_lib as O
import prim_ref as PR
import vcf_ref as V
from povu_amd import hip as H
from test_nested_ref import _vcf
from test_norm_ref import _graph
from test_prim_writer import _FIELDS, _pack_rows
from test_vcf_writer import DATE, _names, _sites_of_texts, _strings, lib  # noqa: F401  (lib: the fixture)

POPPED = "downstream_repetitive/popped-parent-child-rescue"
VCFWAVE = "downstream_repetitive/vcfwave-complex-decomposition"


def _pack_merged(recs, rows, counters, merged, mcounters, n_slots, contig_len):
    """povu_hip_calls of test_prim_writer._pack_rows with the merged rows of merge_ref.merge behind them."""
    c, a = _pack_rows(recs, rows, counters, n_slots, contig_len)
    off = np.zeros(len(merged) + 1, np.uint64)
    off[1:] = np.cumsum([len(m["members"]) for m in merged])
    a["mrow_off"] = off
    a["mrow_member"] = np.ascontiguousarray([x for m in merged for x in m["members"]], np.uint32)
    a["mrow_gt"] = np.ascontiguousarray([0xFF if v is None else v for m in merged for v in m["slots"]], np.uint8)
    for k in ("ac", "an", "ns"):
        a["mrow_" + k] = np.ascontiguousarray([m[k] for m in merged], np.uint32)
    for k in ("mrow_off", "mrow_member", "mrow_gt", "mrow_ac", "mrow_an", "mrow_ns"):
        setattr(c, k, a[k].ctypes.data_as(_FIELDS[k]))
    c.merged, c.n_mrows = 1, len(merged)
    for k in H.MERGE_COUNTERS:
        setattr(c, k, mcounters[k])
    return c, a


def _case(lib, names, paths, seqs, texts, prefixes, cap=0):
    raw = V.call(V.sites_of_pvst(texts), names, paths, seqs, prefixes)
    rows, counters = PR.decompose(raw, names, paths, seqs, max_allele_length=cap)
    merged, mcounters = MR.merge(raw, rows, names)
    n_slots = len(V.slots_of(names)[2])
    contig = [sum(len(seqs[x[0]]) for x in paths[r]) for r in V.ref_paths(names, prefixes)]
    pack = lambda: _pack_merged(raw, rows, counters, merged, mcounters, n_slots, contig)  # noqa: E731
    return raw, rows, merged, pack, _sites_of_texts(lib, texts), _names(lib, names, prefixes)


def _workload(g, seqs, p):
    return list(p.names), [p.steps(i) for i in range(len(p))], dict(zip(g.vid.tolist(), seqs)), list(O.decompose(g).values())


def test_writer_on_the_fixtures(lib, golden_dir, tmp_path):
    for name, n_merged in ((POPPED, 1), (VCFWAVE, 0)):
        (names, paths, seqs), texts = _graph(golden_dir, tmp_path, name)
        raw, rows, merged, pack, sites, nr = _case(lib, names, paths, seqs, texts, ["HG1"])
        calls, keep = pack()
        got = _vcf(lib, calls, sites, nr, names, PR.PROFILE)
        assert got == MR.vcf_text(names, paths, seqs, raw, rows, merged, ["HG1"], date=DATE)
        assert got.count(";MERGED=") == n_merged and got.count("##INFO=<ID=MERGED") == 2
        if name == POPPED:  # a _ROW_RAW row as the second member
            assert "\t4\t>0>5:2:snp1\tA\tG\t" in got and ";MERGED=2;MERGED_FROM=>0>5:2:snp1,>2>4:1:snp1;RAW_POS=1;" in got
            assert got.splitlines()[-1].endswith("\tGT\t0\t.\t1")
        else:
            assert "\t2\t>9>14:1:snp1\tC\tT\t60\tPASS\tAC=1;AF=0.3;AN=3;NS=3;" in got and got.count("\tGT\t0\t1\t0\n") == 1
        # NULL merged arrays: the rows as the decomposed profile writes them
        calls.mrow_off = None
        assert _vcf(lib, calls, sites, nr, names, PR.PROFILE) == PR.vcf_text(names, paths, seqs, raw, rows, ["HG1"], date=DATE)
        del keep
        lib.povu_hip_call_names_free(nr)


def test_writer_on_the_chain_and_refusals(lib):
    names, paths, seqs, texts = _workload(*MC.chain_case())
    raw, rows, merged, pack, sites, nr = _case(lib, names, paths, seqs, texts, MC.CHAIN_REFS, cap=MC.CHAIN_CAP)
    want = MR.vcf_text(names, paths, seqs, raw, rows, merged, MC.CHAIN_REFS, date=DATE)
    calls, keep = pack()
    assert _vcf(lib, calls, sites, nr, names, PR.PROFILE) == want
    assert f";MERGED={MC.MANY};MERGED_FROM=" in want and ":passthrough\t" in want
    assert any(len(m["members"]) > 1 and rows[m["members"][0]]["kind"] == PR.ROW_RAW for m in merged)  # a _ROW_RAW row as the representative
    assert ":1:ins1\tA\tAT\t" in want and want.count(":1:ins1,") == 1
    # the other profiles read neither the rows nor the merged rows
    assert _vcf(lib, calls, sites, nr, names, "raw-graph") == V.vcf_text(names, paths, seqs, raw, MC.CHAIN_REFS, date=DATE)
    # a member that is no row, offsets that do not cover the rows, descend or leave a group empty, an array left out: refused
    ln = C.c_size_t(0)
    n, g = len(rows), len(merged)
    for k, at, v in (("mrow_member", 0, n), ("mrow_member", n - 1, 0xFFFFFFFF), ("mrow_off", 0, 1), ("mrow_off", g, n + 1), ("mrow_off", g, n - 1),
                     ("mrow_off", 1, 0), ("mrow_off", 2, n + 5), ("mrow_gt", None, None), ("mrow_ns", None, None)):
        calls2, keep2 = pack()
        if at is None:
            setattr(calls2, k, None)
        else:
            keep2[k][at] = v
        assert not lib.povu_hip_calls_vcf_profile(C.byref(calls2), sites._p, nr, _strings(names), None, None, 1, H.PROFILES[PR.PROFILE],
                                                  C.byref(ln)), (k, at, v)
    del keep
    lib.povu_hip_call_names_free(nr)


def test_writer_on_many_rows_and_threads(lib):
    """skip_nested: groups across records, more than 1024 merged rows a thread's chunk."""
    names, paths, seqs, texts = _workload(*MC.skip_case(units=160))
    prefixes = ["hap0", "hap3"]
    raw, rows, merged, pack, sites, nr = _case(lib, names, paths, seqs, texts, prefixes)
    assert len(merged) > 2048
    calls, keep = pack()
    want = MR.vcf_text(names, paths, seqs, raw, rows, merged, prefixes, date=DATE)
    for threads in (1, 3):
        assert _vcf(lib, calls, sites, nr, names, PR.PROFILE, threads=threads) == want
    assert _vcf(lib, calls, sites, nr, names, PR.PROFILE, only="hap3", threads=2) == \
        MR.vcf_text(names, paths, seqs, raw, rows, merged, prefixes, date=DATE, only="hap3")
    del keep
    lib.povu_hip_call_names_free(nr)
