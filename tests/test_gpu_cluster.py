"""GPU clustered calls (povu_hip_call_clustered, HipDecomposer.call(cluster=...)) against the plain-Python restatement
(tests/cluster_ref.py): the VCF text and the Calls fields (keys, n_alleles, ref_allele, gt, ac, an, the provenance arrays, every
spelled allele, the counters).  The cases are those of tests/cluster_cases.py, none of them vacuous (tests/test_cluster_ref.py):
braid sites whose bags have 0, 64, 65 and 129 keys (both sides of the tier threshold), a segment three times in one bag and twice in
the other, bags of empty segments, a site that vanishes, 130 clusters in one site, a tie, best fit against first fit, a reference
that walks backwards, a REF that is not its cluster's representative, two references in different clusters.  Then the laws: the
weight bound and the forced device-wide sort change no byte, T = 10^6 on distinct bags is the plain call, regions select the
clustered call's lines, inversion records stay the plain call's, and neither a clustered call nor a nested call sees what the
other left in the arenas they share."""
import numpy as np
import pytest

import cluster_cases as CC
import cluster_ref as CR
import nested_ref as N
import region_cases as RC
import vcf_ref as V
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W
from test_gpu_norm import _fixture_setup, _setup

pytestmark = pytest.mark.gpu

DATE = "00000000"
ARRAYS = ("query", "path", "first", "ref_allele", "n_alleles", "an", "ns", "pos", "flags", "n_steps", "level", "parent_query", "block",
          "ref_spelled", "gt", "ac_off", "ac", "block_off", "seq_off", "at_off", "seq", "at", "contig_len", "rec_clustered", "cl_minsim", "cl_nx")


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _case_setup(d, name):
    g, seqs, p, refs, t = CC.case(name)
    return _setup(d, g, list(seqs), p), list(refs), t


def _text(c, k, which="seq"):
    off = c.seq_off if which == "seq" else c.at_off
    return bytes(getattr(c, which)[int(off[k]):int(off[k + 1])]).decode()


def _digest(c):
    return [np.ascontiguousarray(getattr(c, a)).tobytes() for a in ARRAYS] + [c.vcf_text(date=DATE), c.n_records, c.cluster_ppm]


def _lines(text):
    return [ln for ln in text.splitlines() if not ln.startswith("#")]


def _same(c, want, text, counters=None):
    """The call's text and fields are the restatement's."""
    assert c.vcf_text(date=DATE) == text
    assert c.n_records == len(want)
    for i, r in enumerate(want):
        if r["vartype"] == "SUBR":
            assert int(c.flags[i]) & H.CALL_SUBR and not c.rec_clustered[i] and c.nx(i) == [0, 0]
            continue
        assert (int(c.path[i]), int(c.pos[i]), int(c.query[i]), int(c.first[i])) == (r["path"], r["pos"], r["q"], r["first"])
        assert (int(c.n_alleles[i]), int(c.ref_allele[i]), int(c.an[i]), int(c.ns[i])) == (r["n_classes"], r["ref_class"], r["an"], r["ns"])
        assert [None if g == 0xFFFF else int(g) for g in c.gt[i]] == r["slots"]
        assert c.ac[int(c.ac_off[i]):int(c.ac_off[i + 1])].tolist() == r["ac"]
        assert (bool(c.rec_clustered[i]), int(c.cl_minsim[i]), c.nx(i)) == (r["clustered"], r["minsim"], r["nx"])
        assert bool(int(c.flags[i]) & H.CALL_TANGLED) == r["tangled"] and not int(c.flags[i]) & H.CALL_COLLAPSED
        b = int(c.block_off[c.block[i]])
        order = [int(c.ref_spelled[i])] + [b + a for a in range(r["n_classes"]) if a != r["ref_class"]]
        assert [_text(c, k) for k in order] == [r["ref"]] + r["alts"] and [_text(c, k, "at") for k in order] == r["at"]
        assert (int(c.ref_spelled[i]) == b + r["ref_class"]) == r["ref_is_rep"]  # an own REF is spelled behind the cluster blocks
    if counters is not None:
        assert {k: getattr(c, k) for k in CR.COUNTERS} == counters
    assert c.nested is False and c.n_collapsed_sites == 0


@pytest.mark.parametrize("name", CC.CASES)
def test_the_cases(hip, name):
    setup, refs, t = _case_setup(hip, name)
    f, sites, names, steps, sq = setup
    want, text, counters = CR.call(sites, names, steps, sq, refs, t, date=DATE)
    c = hip.call(f, refs, cluster=t)
    _same(c, want, text, counters)
    assert c.cluster_ppm == t and c.n_cluster_tier2 == sum(len(a) - 2 > 64 for fnd in CR.site_clusters(sites, names, steps, sq, refs, t).values()
                                                              for a in fnd[0])
    # the two laws that hold for every case: without the bound, and with every bag through the device-wide sort
    free = hip.call(f, refs, cluster=t, cluster_no_bound=True)
    assert _digest(free) == _digest(c) and free.n_cluster_pruned == 0 and free.n_cluster_pairs == c.n_cluster_pairs
    forced = hip.call(f, refs, cluster=t, flags=H.T_FORCE_TIER2)
    assert _digest(forced) == _digest(c) and forced.n_cluster_pruned == c.n_cluster_pruned
    assert forced.n_cluster_tier2 == sum(len(a) > 2 for fnd in CR.site_clusters(sites, names, steps, sq, refs, t).values() for a in fnd[0])
    if name == CC.PRUNE_CASE:
        assert c.n_cluster_pruned > 0
    if name == "star":
        assert int(c.n_alleles[0]) == 130
    assert hip.call(f, refs, cluster=f"{t // 10 ** 6}.{t % 10 ** 6:06d}").vcf_text(date=DATE) == text  # the threshold as text


def test_the_worked_example(hip, golden_dir):
    import json
    setup = _fixture_setup(hip, golden_dir, CC.FIXTURE)
    f, sites, names, steps, sq = setup
    golden = json.load(open(CC.GOLDEN))
    plain = hip.call(f, ["HG1"])
    for text_f in ("0.6", "0.600001"):
        want, text, counters = CR.call(sites, names, steps, sq, ["HG1"], CR.parse(text_f), date=DATE)
        c = hip.call(f, ["HG1"], cluster=text_f)
        _same(c, want, text, counters)
        assert _lines(c.vcf_text(date=DATE)) == golden[text_f]["records"]
        assert [ln for ln in c.vcf_text(date=DATE).splitlines() if ln.startswith("#") and ln not in plain.vcf_text(date=DATE).splitlines()] == \
            golden[text_f]["header"]
    assert _lines(hip.call(f, ["HG1"], cluster="0.600001").vcf_text(date=DATE)) == _lines(plain.vcf_text(date=DATE))
    # without a threshold: the call of before, byte for byte, and nothing of the clusters
    assert plain.cluster_ppm == 0 and plain.cl_nx.size == plain.rec_clustered.size == 0 and all(getattr(plain, k) == 0 for k in H.CLUSTER_COUNTERS)
    assert "povu_call_cluster" not in plain.vcf_text(date=DATE) and "ID=NX" not in plain.vcf_text(date=DATE)


def test_every_bag_distinct_at_one_is_the_plain_call(hip):
    g = W.chain_of_bubbles(60)  # (no empty segment: the bags {x}, {y} and {} of a unit share nothing, and none is without weight)
    setup = _setup(hip, g, W.random_sequences(g, 4, max_len=5, empty=0.0), W.pansn(W.chain_haplotypes(60, 9, seed=3), samples=5))
    f = setup[0]
    plain, c = hip.call(f, ["sample0#1"]), hip.call(f, ["sample0#1"], cluster="1")
    assert c.n_records == plain.n_records > 0 and _lines(c.vcf_text(date=DATE)) == _lines(plain.vcf_text(date=DATE))
    assert c.n_clustered_sites == c.n_cluster_vanished == 0 and c.n_cluster_sites > 0 and not c.rec_clustered.any()
    for a in ("query", "path", "first", "ref_allele", "n_alleles", "an", "ns", "pos", "flags", "gt", "ac", "seq", "at", "ref_spelled"):
        assert np.array_equal(getattr(c, a), getattr(plain, a)), a


def test_regions_select_the_clustered_calls_lines(hip):
    setup, refs, t = _case_setup(hip, "braid-chain")
    f, sites, names, steps, sq = setup
    g = CC.case("braid-chain")[0]
    per = (g.n_vtx - 1) // 5
    # the bases of the reference around the second site's entry segment
    off = 0
    for seg, _ in steps[0]:
        if seg == 1 + per:
            break
        off += len(sq[seg])
    regions = [(names[0], off + 1, off + 2)]
    want, text, _ = CR.call(sites, names, steps, sq, refs, t, regions=regions, date=DATE)
    full = CR.call(sites, names, steps, sq, refs, t, date=DATE)[0]
    assert 0 < len(want) < len(full)
    for no_mask in (False, True):
        c = hip.call(f, refs, cluster=t, regions=regions, region_no_mask=no_mask)
        _same(c, want, text)
        assert c.n_regions == 1 and (c.n_region_dropped > 0) == no_mask
    whole = _lines(hip.call(f, refs, cluster=t).vcf_text(date=DATE))
    assert [ln for ln in whole if ln in _lines(text)] == _lines(text)


def test_inversion_records_stay_the_plain_calls(hip):
    g, seqs, p, refs = RC.workload("inverted")
    setup = _setup(hip, g, list(seqs), p)
    f, sites, names, steps, sq = setup
    want, text, _ = CR.call(sites, names, steps, sq, list(refs), 500000, inversions=True, date=DATE)
    c = hip.call(f, list(refs), flags=H.T_INVERSIONS, cluster=500000)
    _same(c, want, text)
    plain = hip.call(f, list(refs), flags=H.T_INVERSIONS)
    subr = [ln for ln in _lines(plain.vcf_text(date=DATE)) if "VARTYPE=SUBR" in ln]
    assert subr and [ln for ln in _lines(c.vcf_text(date=DATE)) if "VARTYPE=SUBR" in ln] == subr and c.n_inv_records == plain.n_inv_records


def test_nothing_stale_in_the_shared_arenas():
    hip = HipDecomposer(0)
    try:
        g = W.braid(40, 8, 3, seed=5)  # a large braid first
        big = _setup(hip, g, W.random_sequences(g, 5, max_len=7), W.braid_haplotypes(40, 8, 3, 24, seed=5, mutate=0.08))
        assert hip.call(big[0], ["hap0#"], cluster="0.8").n_clustered_sites > 0
        setup, refs, t = _case_setup(hip, "best-fit")  # then a small different graph in the same context
        small = _digest(hip.call(setup[0], refs, cluster=t))
        gs, seqs, ps, refs_n = RC.workload("skip")  # and a plain nested call behind a clustered one
        nested_setup = _setup(hip, gs, list(seqs), ps)
        hip.call(nested_setup[0], list(refs_n), cluster="0.5")
        nested = hip.call(nested_setup[0], list(refs_n), flags=H.T_NESTED).vcf_text(date=DATE)
    finally:
        hip.close()
    fresh = HipDecomposer(0)
    try:
        setup, refs, t = _case_setup(fresh, "best-fit")
        assert _digest(fresh.call(setup[0], refs, cluster=t)) == small
        nested_setup = _setup(fresh, gs, list(seqs), ps)
        f, sites, names, steps, sq = nested_setup
        assert fresh.call(f, list(refs_n), flags=H.T_NESTED).vcf_text(date=DATE) == nested
        assert nested == N.vcf_text(names, steps, sq, N.call(sites, names, steps, sq, list(refs_n)), list(refs_n), date=DATE)
        fresh.call(f, list(refs_n), flags=H.T_NESTED)  # ... and a clustered call behind a nested one
        want, text, counters = CR.call(sites, names, steps, sq, list(refs_n), 500000, date=DATE)
        _same(fresh.call(f, list(refs_n), cluster="0.5"), want, text, counters)
    finally:
        fresh.close()


def test_refusals(hip, golden_dir):
    f = _fixture_setup(hip, golden_dir, CC.FIXTURE)[0]
    for kw, word in ((dict(flags=H.T_NESTED), "POVU_HIP_T_NESTED"), (dict(profile="top-level-only"), "POVU_HIP_T_NESTED"),
                     (dict(profile="popped"), "POVU_HIP_T_NESTED"), (dict(profile="left-normalized"), "left-normalized"),
                     (dict(profile="decomposed"), "decomposed"), (dict(profile="decomposed", flags=H.T_MERGE), "decomposed"),
                     (dict(flags=H.T_OFFREF), "POVU_HIP_T_OFFREF"), (dict(flags=H.T_UNTANGLE), "POVU_HIP_T_UNTANGLE")):
        with pytest.raises(RuntimeError, match="clustered call .*refused.*" + word):
            hip.call(f, ["HG1"], cluster="0.9", **kw)
    for bad in ("0", "1.0000001", "1.5", "-0.5", ".", "0.5x", "0.1234567", 0, 10 ** 6 + 1, 0.9, True):
        with pytest.raises(RuntimeError, match="cluster threshold"):
            hip.call(f, ["HG1"], cluster=bad)
    assert hip.call(f, ["HG1"], cluster=10 ** 6).cluster_ppm == hip.call(f, ["HG1"], cluster="1.000000").cluster_ppm == 10 ** 6
