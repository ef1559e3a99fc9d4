"""The host writer on hand-made povu_hip_calls of the untangled calls (povu_hip_calls_vcf_profile, povu_amd/csrc/host/vcf.cpp),
against the restatement's text (tests/untangle_ref.py): the header order, LN / LC, the GT:CN columns of a diploid sample, NULL
arrays giving the text of before, half of the arrays refused.  No GPU."""
import ctypes as C

import numpy as np

import offref_cases as OC
import untangle_cases as UC
import untangle_ref as U
import vcf_ref as V
from povu_amd import hip as H
from test_offref_writer import _text
from test_vcf_writer import DATE, _names, _pack, _sites_of_texts, lib  # noqa: F401  (lib: the fixture)

FIELDS = dict(H._Calls._fields_ + H._CallsNested._fields_)
ARRAYS = ("rec_unt", "lap", "n_laps", "lap_count")


def _pack_untangled(recs, names, paths, seqs, prefixes, n_slots, with_arrays=True):
    refs = V.ref_paths(names, prefixes)
    base, keep = _pack(recs, n_slots, [sum(len(seqs[x[0]]) for x in paths[r]) for r in refs])
    c = H._CallsNested()
    for k, _ in H._Calls._fields_:
        setattr(c, k, getattr(base, k))
    if with_arrays:
        keep.update(rec_unt=np.ascontiguousarray([r["unt"] for r in recs] + [0], dtype=np.uint8),
                    lap=np.ascontiguousarray([r["lap"] for r in recs] + [0], dtype=np.uint32),
                    n_laps=np.ascontiguousarray([r["n_laps"] for r in recs] + [0], dtype=np.uint32),
                    lap_count=np.ascontiguousarray([x for r in recs for x in r["lap_count"]] + [0], dtype=np.uint16))
        for k in ARRAYS:
            setattr(c, k, keep[k].ctypes.data_as(FIELDS[k]))
        c.untangled = 1
    return c, keep


def _diploid(tmp_path):
    """One loop site; sample `d` is diploid (3 and 1 laps), sample `e` has one haplotype of one lap, which pairs with the reference's second."""
    names = ["ref#1#c", "d#1#c", "d#2#c", "e#1#c"]
    g, p = UC.looped_paths(names, [[0, 1], [1, 1, 0], [0], [1]])
    out = tmp_path / "d"
    out.mkdir()
    gfa = out / "g.gfa"
    gfa.write_text(g.to_gfa(UC.sequences(g)) + p.to_gfa())
    return OC.load(str(gfa), out / "pvst")


def test_header_order_ln_lc_and_diploid_columns(lib, tmp_path):
    sites, names, paths, seqs, texts = _diploid(tmp_path)
    recs, counts = U.call(sites, names, paths, seqs, ["ref#"])
    lsites, nr = _sites_of_texts(lib, texts), _names(lib, names, ["ref#"])
    c, keep = _pack_untangled(recs, names, paths, seqs, ["ref#"], nr.contents.refs.n_slots)
    want = U.vcf_text(names, paths, seqs, recs, ["ref#"], date=DATE)
    for threads in (1, 4):
        assert _text(lib, c, lsites, nr, names, threads=threads) == want
    head = want.splitlines()
    k = len(V.HEADER.splitlines())
    assert [ln[:ln.index(",")] for ln in head[k:k + 3]] == ["##INFO=<ID=LN", "##INFO=<ID=LC", "##FORMAT=<ID=CN"]
    assert head[k + 3].startswith("##contig=<ID=ref#1#c,")
    lines = [ln.split("\t") for ln in head if not ln.startswith("#")]
    assert len(lines) == 2 and all(f[8] == "GT:CN" for f in lines)
    assert [f[7].split(";")[-2:] for f in lines] == [["LN=1", "LC=2"], ["LN=2", "LC=2"]]
    assert [f[9:] for f in lines] == [["0:2", "1|0:3,1", ".:1"], ["0:2", "0|.:3,1", "0:1"]]
    del keep
    lib.povu_hip_call_names_free(nr)


def test_the_fixture_and_null_arrays(lib, tmp_path):
    sites, names, paths, seqs, texts = OC.load(UC.GFA, tmp_path)
    recs, _ = U.call(sites, names, paths, seqs, ["HG1"])
    lsites, nr = _sites_of_texts(lib, texts), _names(lib, names, ["HG1"])
    c, keep = _pack_untangled(recs, names, paths, seqs, ["HG1"], nr.contents.refs.n_slots)
    text = _text(lib, c, lsites, nr, names)
    assert [ln for ln in text.splitlines() if not ln.startswith("#")] == UC.golden()["lines"]
    c.n_laps = None  # (half of the arrays)
    _text(lib, c, lsites, nr, names, ok=False)
    plain = V.call(sites, names, paths, seqs, ["HG1"])
    c2, keep2 = _pack_untangled(plain, names, paths, seqs, ["HG1"], nr.contents.refs.n_slots, with_arrays=False)
    assert not c2.rec_unt and _text(lib, c2, lsites, nr, names) == V.vcf_text(names, paths, seqs, plain, ["HG1"], date=DATE)
    # a call with the flag and no record keeps its header lines
    c3, keep3 = _pack_untangled([], names, paths, seqs, ["HG1"], nr.contents.refs.n_slots, with_arrays=False)
    c3.untangled = 1
    assert _text(lib, c3, lsites, nr, names) == U.vcf_text(names, paths, seqs, [], ["HG1"], date=DATE)
    del keep, keep2, keep3
    lib.povu_hip_call_names_free(nr)
