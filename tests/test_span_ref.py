"""The plain-Python restatement of the spanning alleles (tests/span_ref.py; INTEGRATION.md "Spanning alleles") on the
popped-parent-child-rescue fixture against the stored record lines (tests/golden/span_records.json), on the depth-two chain
of tests/test_nested_ref.py (a chain walk past an ancestor the slot does not cross), with the option off against
nested_ref, the rules under the sanitizers (`make span_check`), and the host writer (povu_hip_calls_vcf_profile) on
hand-packed records with and without rec_star.  No GPU.

The fixture's pins: with the option >2>4 (LV=1, PS=>0>5) reads ALT=G,* with AC=1,1, AN=3, NS=3, and >0>5 is unchanged.  The
haplotype on the 0 -> 5 edge is HG2, the second sample column, so the GT columns are 0, 2, 1."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import nested_ref as N
import oracle_lib as O
import span_ref as S
import vcf_ref as V
from povu_amd import hip as H
from povu_amd import workloads as W
from test_nested_ref import DEPTH2_NAMES, DEPTH2_PATHS, DEPTH2_SEQS, DEPTH2_SITES, _fixture, _pack, _vcf
from test_vcf_writer import DATE, _names, _sites_of_texts, lib  # noqa: F401  (lib: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "span_records.json")))


def test_fixture_against_the_golden_lines(golden_dir, tmp_path):
    want = _golden(golden_dir)
    (names, paths, seqs), texts = _fixture(golden_dir, tmp_path)
    sites = V.sites_of_pvst(texts)
    for profile, lines in sorted(want["profiles"].items()):
        opts = want["popped_options"] if profile == "popped" else {}
        recs, counters = S.call_full(sites, names, paths, seqs, [want["reference_prefix"]], profile=profile, **opts)
        assert [S.record_line(r) for r in recs] == lines, profile
        assert {k: counters[k] for k in ("n_star_records", "n_star_entries")} == want["counters"][profile]
        text = S.vcf_text(names, paths, seqs, recs, [want["reference_prefix"]], profile=profile)
        assert text.splitlines()[-len(lines):] == lines and "##ALT" not in text
    # what the definition states of the fixture, field by field
    raw = S.call(sites, names, paths, seqs, ["HG1"])
    outer, inner = raw
    assert (inner["es"], inner["lv"], inner["ps"], inner["alts"], inner["at"]) == (">2>4", 1, ">0>5", ["G", "*"], [">3", ">6", "*"])
    assert (inner["ac"], inner["an"], inner["ns"], inner["gt"], inner["star"], inner["n_alleles"]) == ([1, 1], 3, 3, ["0", "2", "1"], True, 3)
    assert names[1].startswith("HG2") and paths[1] == [(0, 0), (5, 0)] and inner["spanned"] == [1]
    plain = N.call(sites, names, paths, seqs, ["HG1"])
    assert {k: outer[k] for k in plain[0]} == plain[0] and not outer["star"]
    # the rescued child of the popped parent keeps its `*`; top-level-only has no record with an ancestor
    popped = S.call(sites, names, paths, seqs, ["HG1"], profile="popped", **want["popped_options"])
    assert [(r["id"], r["alts"], r["gt"]) for r in popped] == [(">2>4:rescued", ["G", "*"], ["0", "2", "1"])]
    assert not any(r["star"] for r in S.call(sites, names, paths, seqs, ["HG1"], profile="top-level-only"))


def test_chain_walk_passes_an_ancestor_the_slot_does_not_cross():
    a = (DEPTH2_SITES, DEPTH2_NAMES, DEPTH2_PATHS, DEPTH2_SEQS, ["R#"])
    recs, counters = S.call_full(*a)
    # A takes the 0 -> 9 edge: it crosses neither >2>7 nor >4>6, and is spanned in both (for >4>6 by its grandparent alone);
    # B takes the 2 -> 7 edge: spanned in >4>6 by its parent
    assert [(r["es"], r["gt"], r["ac"], r["an"], r["ns"]) for r in recs] == [
        (">0>9", ["0", "1", "0", "0"], [1], 4, 4), (">2>7", ["0", "2", "1", "0"], [1, 1], 4, 4), (">4>6", ["0", "2", "2", "1"], [1, 2], 4, 4)]
    assert (counters["n_star_records"], counters["n_star_entries"]) == (2, 3)
    # the choice is made before the profile: the grandchild rescued through two popped ancestors keeps both entries
    recs, counters = S.call_full(*a, profile="popped", max_level=0, max_ref_length=4, max_allele_length=4)
    assert [(r["id"], r["alts"][-1], r["gt"]) for r in recs] == [(">4>6:rescued", "*", ["0", "2", "2", "1"])]
    assert (counters["n_star_records"], counters["n_star_entries"]) == (1, 2)
    # a search cut short is "unknown": with max_steps 4 the sites >0>9 and >2>7 are TRAV_LONG and give no `*`; >4>6 is whole,
    # but its ancestors' sites have lost the traversals that would span it
    cut, _ = S.call_full(*a, max_steps=4)
    assert not any(r["star"] for r in cut)


def test_option_off_is_the_nested_call():
    for units, depth, haps in ((12, 1, 8), (6, 2, 12)):
        g = W.skip_nested(units, depth, seed=3)
        p = W.pansn(W.skip_haplotypes(units, depth, haps, seed=3), samples=(haps + 1) // 2)
        names, paths = list(p.names), [p.steps(i) for i in range(len(p))]
        seqs = dict(zip(g.vid.tolist(), W.random_sequences(g, 3, max_len=4)))
        sites = V.sites_of_pvst(list(O.decompose(g).values()))
        for profile, opts in ((None, {}), ("popped", dict(max_level=0, max_ref_length=6, max_allele_length=6))):
            want, wc = N.call_full(sites, names, paths, seqs, ["sample0#1"], profile=profile, **opts)
            off, oc = S.call_full(sites, names, paths, seqs, ["sample0#1"], profile=profile, spanning=False, **opts)
            assert [{k: r[k] for k in w} for r, w in zip(off, want)] == want and len(off) == len(want)
            assert oc == dict(wc, n_star_records=0, n_star_entries=0)
            assert S.vcf_text(names, paths, seqs, off, ["sample0#1"], profile=profile) == N.vcf_text(names, paths, seqs, want, ["sample0#1"],
                                                                                                   profile=profile)
            on, onc = S.call_full(sites, names, paths, seqs, ["sample0#1"], profile=profile, **opts)
            # the option changes nothing but the spanned entries and what counts them
            for r, w in zip(on, want):
                assert [g for sl, g in enumerate(r["slots"]) if sl not in r["spanned"]] == \
                    [g for sl, g in enumerate(w["slots"]) if sl not in r["spanned"]]
                assert r["ac"][:len(w["ac"])] == w["ac"] and r["an"] == w["an"] + len(r["spanned"])
            if profile is None:
                assert onc["n_star_records"] >= 3  # (the skips delete whole units: the input reaches the option)


def test_span_check_passes_under_the_sanitizers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "span_check", "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([os.path.join(ROOT, "build", "obj", "span_check")], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "span_check: ok", p.stdout + p.stderr


# ---- the host writer on hand-packed records

def _pack_star(recs, n_slots, contig_len, with_star=True):
    """test_nested_ref._pack, then the arrays of the option: n_alleles counts the `*`, rec_star marks it (the blocks stay
    those of the classes: `*` has no spelled allele)."""
    calls, keep = _pack(recs, n_slots, contig_len)
    keep["n_alleles"][:] = [r["n_alleles"] for r in recs]
    if with_star:
        keep["rec_star"] = np.ascontiguousarray([1 if r["star"] else 0 for r in recs], dtype=np.uint8)
        calls.rec_star = keep["rec_star"].ctypes.data_as(C.POINTER(C.c_uint8))
        calls.spanning = 1
    return calls, keep


def test_writer_writes_the_star_last_and_never_reads_a_text_for_it(lib):
    pvst = "H\t0.0.3\t.\t.\t.\nD\t0\t.\t1, 2, 3\t.\nF\t1\t>0>9\t.\tL\nF\t2\t>2>7\t.\tL\nF\t3\t>4>6\t.\tL\n"
    sites, nr = _sites_of_texts(lib, [pvst]), _names(lib, DEPTH2_NAMES, ["R#"])
    a = (DEPTH2_SITES, DEPTH2_NAMES, DEPTH2_PATHS, DEPTH2_SEQS, ["R#"])
    for profile, kw in (("raw-graph", {}), ("popped", dict(max_ref_length=4)), ("popped", dict(max_ref_length=6)), ("top-level-only", {})):
        recs = S.call(*a, profile=profile, **kw)
        calls, keep = _pack_star(recs, 4, [10])
        want = S.vcf_text(DEPTH2_NAMES, DEPTH2_PATHS, DEPTH2_SEQS, recs, ["R#"], date=DATE, profile=profile)
        for threads in (1, 4):
            assert _vcf(lib, calls, sites, nr, DEPTH2_NAMES, profile, threads=threads) == want, (profile, kw)
        del keep
    # (the last record's block is the last block: an index one past its classes would leave `seq_off` / `at_off`)
    recs = S.call(*a)
    assert recs[-1]["star"] and recs[-1]["alts"][-1] == "*"
    # hand-made records without rec_star: a record whose n_alleles is its class count is written as before
    off = S.call(*a, spanning=False)
    calls, keep = _pack_star(off, 4, [10], with_star=False)
    assert _vcf(lib, calls, sites, nr, DEPTH2_NAMES, "raw-graph") == N.vcf_text(DEPTH2_NAMES, DEPTH2_PATHS, DEPTH2_SEQS, N.call(*a), ["R#"],
                                                                               date=DATE)
    del keep
    # rec_star against n_alleles: a `*` on a record of two alleles, or with one AC entry too few, is refused
    calls, keep = _pack_star(recs, 4, [10])
    keep["n_alleles"][1] = 2
    ln = C.c_size_t(0)
    assert not lib.povu_hip_calls_vcf_profile(C.byref(calls), sites._p, nr, (C.c_char_p * 4)(*[n.encode() for n in DEPTH2_NAMES]),
                                              DATE.encode(), None, 1, 0, C.byref(ln))
    del keep
    lib.povu_hip_call_names_free(nr)
