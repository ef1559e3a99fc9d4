"""The host writer on hand-made povu_hip_calls of the off-reference calls (povu_hip_calls_vcf_profile and povu_hip_calls_vcf_rest,
povu_amd/csrc/host/vcf.cpp), against the restatement's text (tests/offref_ref.py): the header order, the split between the
files of the prefixes and the rest, NULL arrays giving the text of before, indices outside their ranges refused.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import offref_cases as OC
import offref_ref as F
import vcf_ref as V
from povu_amd import hip as H
from test_vcf_writer import DATE, _names, _pack, _sites_of_texts, _strings, lib  # noqa: F401  (lib: the fixture)

NIL = 0xFFFFFFFF
FIELDS = dict(H._Calls._fields_ + H._CallsNested._fields_)


def _pack_offref(recs, names, paths, seqs, prefixes, n_slots, with_arrays=True):
    """povu_hip_calls of the restatement's records: test_vcf_writer's arrays and, with_arrays, those of the flag."""
    refs = V.ref_paths(names, prefixes)
    length = lambda k: sum(len(seqs[x[0]]) for x in paths[k])  # noqa: E731
    base, keep = _pack(recs, n_slots, [length(r) for r in refs])
    c = H._CallsNested()
    for k, _ in H._Calls._fields_:
        setattr(c, k, getattr(base, k))
    if with_arrays:
        contigs = F.off_contigs(names, recs, prefixes)
        keep.update(rec_offref=np.ascontiguousarray([r["offref"] for r in recs], dtype=np.uint8),
                    host_query=np.ascontiguousarray([NIL if r["host"] is None else r["host"] for r in recs], dtype=np.uint32),
                    host_allele=np.ascontiguousarray([NIL if r["ha"] is None else r["ha"] for r in recs], dtype=np.uint32),
                    off_contig_path=np.ascontiguousarray(contigs + [0], dtype=np.uint32),
                    off_contig_len=np.ascontiguousarray([length(k) for k in contigs] + [0], dtype=np.uint64))
        for k in ("rec_offref", "host_query", "host_allele", "off_contig_path", "off_contig_len"):
            setattr(c, k, keep[k].ctypes.data_as(FIELDS[k]))
        c.offref, c.n_off_contigs = 1, len(contigs)
        c.n_offref_records = sum(r["offref"] for r in recs)
    return c, keep


def _text(lib, c, sites, nr, names, only=None, threads=1, ok=True):
    ln = C.c_size_t(0)
    p = lib.povu_hip_calls_vcf_profile(C.byref(c), sites._p, nr, _strings(names), DATE.encode(), only.encode() if only is not None else None,
                                       threads, 0, C.byref(ln))
    if not ok:
        assert not p
        return None
    assert p
    s = C.string_at(p, ln.value).decode()
    lib.povu_hip_buffer_free(p)
    return s


def _rest(lib, c, sites, nr, names, prefixes, threads=1):
    lib.povu_hip_calls_vcf_rest.argtypes = [C.POINTER(H._CallsNested), C.POINTER(H._Sites), C.POINTER(H._CallNames), C.POINTER(C.c_char_p),
                                            C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t)]
    lib.povu_hip_calls_vcf_rest.restype = C.c_void_p
    ln = C.c_size_t(0)
    p = lib.povu_hip_calls_vcf_rest(C.byref(c), sites._p, nr, _strings(names), DATE.encode(), _strings(prefixes), len(prefixes), threads, 0,
                                    C.byref(ln))
    assert p
    s = C.string_at(p, ln.value).decode()
    lib.povu_hip_buffer_free(p)
    return s


def _setup(lib, name, tmp_path, prefixes):
    sites, names, paths, seqs, texts = OC.load(OC.gfa_of(name), tmp_path / name)
    recs, _ = F.call(sites, names, paths, seqs, prefixes)
    return sites, names, paths, seqs, recs, _sites_of_texts(lib, texts), _names(lib, names, prefixes)


@pytest.mark.parametrize("name,prefixes", [("inner-snp", ["HG1"]), ("two-insertions", ["HG1"]), ("surrogate-is-reference", ["HG1"]),
                                           ("no-host", ["HG1"]), ("one-allele", ["HG1"]), ("two-insertions", ["HG1", "HG3"]),
                                           ("backwards", ["HG1"]), ("bubble-in-bubble", ["HG1"])])
def test_text_header_and_split(lib, tmp_path, name, prefixes):
    sites, names, paths, seqs, recs, lsites, nr = _setup(lib, name, tmp_path, prefixes)
    c, keep = _pack_offref(recs, names, paths, seqs, prefixes, nr.contents.refs.n_slots)
    for threads in (1, 4):
        assert _text(lib, c, lsites, nr, names, threads=threads) == F.vcf_text(sites, names, paths, seqs, recs, prefixes, date=DATE)
    for only in prefixes:
        assert _text(lib, c, lsites, nr, names, only=only) == F.vcf_text(sites, names, paths, seqs, recs, prefixes, date=DATE, only=only)
    rest = _rest(lib, c, lsites, nr, names, prefixes)
    assert rest == F.vcf_text(sites, names, paths, seqs, recs, prefixes, date=DATE, rest=True)
    # every record is in exactly one file of -o DIR
    files = [_text(lib, c, lsites, nr, names, only=p) for p in prefixes] + [rest]
    if len(prefixes) == 1 or not any(n.startswith(prefixes[0]) and n.startswith(prefixes[1]) for n in names):
        assert sorted(ln for t in files for ln in OC.records_of(t)) == sorted(F.record_line(r, sites) for r in recs)
    head = _text(lib, c, lsites, nr, names).splitlines()
    k = len(V.HEADER.splitlines())
    assert [ln[:ln.index(",")] for ln in head[k:k + 3]] == ["##INFO=<ID=OFFREF", "##INFO=<ID=HOST", "##INFO=<ID=HA"]
    assert head[k + 3].startswith("##contig=<ID=HG1#1#chr1,")
    del keep
    lib.povu_hip_call_names_free(nr)


def test_the_rest_of_the_issue_graph_is_its_inner_record(lib, tmp_path):
    sites, names, paths, seqs, recs, lsites, nr = _setup(lib, "inner-snp", tmp_path, ["HG1"])
    c, keep = _pack_offref(recs, names, paths, seqs, ["HG1"], nr.contents.refs.n_slots)
    want = OC.golden()["cases"]["inner-snp"]["lines"]
    assert OC.records_of(_text(lib, c, lsites, nr, names, only="HG1")) == want[:1]
    rest = _rest(lib, c, lsites, nr, names, ["HG1"])
    assert OC.records_of(rest) == want[1:] and OC.contigs_of(rest) == ["HG2#1#chr1,length=6"]
    del keep
    lib.povu_hip_call_names_free(nr)


def test_null_arrays_give_the_text_of_before(lib, tmp_path):
    sites, names, paths, seqs, _, lsites, nr = _setup(lib, "inner-snp", tmp_path, ["HG1"])
    plain = V.call(sites, names, paths, seqs, ["HG1"])
    for r in plain:
        r.update(offref=False, host=None, ha=None)
    c, keep = _pack_offref(plain, names, paths, seqs, ["HG1"], nr.contents.refs.n_slots, with_arrays=False)
    assert not c.rec_offref and not c.host_query
    assert _text(lib, c, lsites, nr, names) == V.vcf_text(names, paths, seqs, plain, ["HG1"], date=DATE)
    del keep
    lib.povu_hip_call_names_free(nr)


def test_indices_outside_their_ranges_are_refused(lib, tmp_path):
    sites, names, paths, seqs, recs, lsites, nr = _setup(lib, "inner-snp", tmp_path, ["HG1"])
    c, keep = _pack_offref(recs, names, paths, seqs, ["HG1"], nr.contents.refs.n_slots)
    assert _text(lib, c, lsites, nr, names)
    keep["host_query"][1] = len(sites)
    _text(lib, c, lsites, nr, names, ok=False)
    keep["host_query"][1] = 0
    keep["off_contig_path"][0] = len(names)
    _text(lib, c, lsites, nr, names, ok=False)
    keep["off_contig_path"][0] = 1
    assert _text(lib, c, lsites, nr, names)
    c.host_allele = None  # (half of the arrays)
    _text(lib, c, lsites, nr, names, ok=False)
    del keep
    lib.povu_hip_call_names_free(nr)


def test_a_call_with_the_flag_and_no_record_keeps_its_header(lib, tmp_path):
    sites, names, paths, seqs, _, lsites, nr = _setup(lib, "inner-snp", tmp_path, ["HG1"])
    c, keep = _pack_offref([], names, paths, seqs, ["HG1"], nr.contents.refs.n_slots, with_arrays=False)
    assert _text(lib, c, lsites, nr, names) == V.vcf_text(names, paths, seqs, [], ["HG1"], date=DATE)
    c.offref = 1  # (no record: no array says so)
    assert _text(lib, c, lsites, nr, names) == F.vcf_text(sites, names, paths, seqs, [], ["HG1"], date=DATE)
    del keep
    lib.povu_hip_call_names_free(nr)
