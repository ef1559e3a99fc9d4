"""The plain-Python restatement of the clustered calls (tests/cluster_ref.py): the worked example of INTEGRATION.md "Clustered
calls" on the popped-parent-child-rescue fixture, derivable by hand, against the rows pinned in tests/golden/cluster_records.json;
the pair exactly at the threshold and one ppm above it; the parser; and for every case the GPU tests use (tests/cluster_cases.py)
that it is not vacuous and shows what it is there for.  No GPU."""
import functools
import json
from collections import Counter

import pytest

import cluster_cases as CC
import cluster_ref as CR
import oracle_lib as O
import vcf_ref as V
from povu_amd import workloads as W


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    out = tmp_path_factory.mktemp("cluster_fx")
    n = O.decompose_gfa(CC.GFA, str(out))
    texts = [(out / f"{i}.pvst").read_text() for i in range(1, n + 1) if (out / f"{i}.pvst").exists()]
    names, paths, seqs = CC.fixture_tables()
    sites = V.sites_of_pvst(texts)
    assert sorted(V.label(s["s"], s["z"]) for s in sites) == [">0>5", ">2>4"]
    return sites, names, paths, seqs


@functools.lru_cache(maxsize=None)
def _case(name):
    g, _seqs, _p, refs, t = CC.case(name)
    sites = V.sites_of_pvst(list(O.decompose(g).values()))
    names, paths, sq = CC.tables(name)
    return sites, names, paths, sq, list(refs), t


def _lines(text):
    return [ln for ln in text.splitlines() if not ln.startswith("#")]


def test_the_worked_example(fixture):
    sites, names, paths, seqs = fixture
    golden = json.load(open(CC.GOLDEN))
    plain = V.vcf_text(names, paths, seqs, V.call(sites, names, paths, seqs, ["HG1"]), ["HG1"])
    # the bags and the two similarities the section states
    found = CR.site_clusters(sites, names, paths, seqs, ["HG1"], 600000)
    q05 = next(q for q, s in enumerate(sites) if V.label(s["s"], s["z"]) == ">0>5")
    q24 = next(q for q, s in enumerate(sites) if V.label(s["s"], s["z"]) == ">2>4")
    bags = [CR.bag_of(a) for a in found[q05][0]]
    assert bags == [Counter([1, 2, 3, 4]), Counter(), Counter([1, 2, 6, 4])]
    w = {v: 1 for v in seqs}
    assert CR.frac(bags[0], bags[2], w) == (3, 5) and CR.frac(bags[1], bags[0], w) == (0, 4) and CR.frac(bags[1], bags[2], w) == (0, 4)
    assert found[q05][3:6] == ([0, 1, 0], [0, 1], 600000) and found[q24][3:6] == ([0, 1], [0, 1], 1000000)
    # exactly at the threshold
    recs, text, counters = CR.call(sites, names, paths, seqs, ["HG1"], CR.parse("0.6"))
    assert _lines(text) == golden["0.6"]["records"] and golden["0.6"]["header"] == [ln for ln in text.splitlines() if ln.startswith("#") and ln not in plain.splitlines()]
    big, small = recs
    assert (big["id"], big["pos"], big["ref"], big["alts"], big["gt"], big["ac"], big["an"]) == (">0>5", 1, "AAAAA", ["A"], ["0", "1", "0"], [1], 3)
    assert (big["nx"], big["minsim"], big["clustered"], big["tangled"]) == ([2, 1], 600000, True, False)
    assert _lines(text)[0].endswith(";ES=>0>5;LV=0;NX=2,1;MINSIM=600000\tGT\t0\t1\t0")
    assert (small["id"], small["clustered"], small["gt"]) == (">2>4", False, ["0", ".", "1"]) and "NX=" not in _lines(text)[1]
    assert _lines(text)[1] == _lines(plain)[1]  # site >2>4 is unchanged
    assert counters == dict(n_cluster_sites=2, n_clustered_sites=1, n_cluster_vanished=0, n_cluster_keys=10, n_cluster_pairs=4, n_cluster_pruned=2)
    # one ppm above it: the plain call's lines, and the three header lines
    recs, text, counters = CR.call(sites, names, paths, seqs, ["HG1"], CR.parse("0.600001"))
    assert _lines(text) == _lines(plain) == golden["0.600001"]["records"] and "\tA,AAAGA\t" in _lines(text)[0]
    assert [ln for ln in text.splitlines() if ln.startswith("#") and ln not in plain.splitlines()] == golden["0.600001"]["header"]
    assert golden["0.600001"]["header"][-1] == "##povu_call_cluster=0.600001" and golden["0.6"]["header"][-1] == "##povu_call_cluster=0.600000"
    assert counters["n_clustered_sites"] == 0 and counters["n_cluster_pairs"] == 4


def test_the_pair_at_the_threshold_and_one_ppm_above():
    assert CR.similar((3, 5), 600000) and not CR.similar((3, 5), 600001) and CR.sim_ppm((3, 5)) == 600000
    assert CR.similar((0, 0), CR.PPM) and CR.sim_ppm((0, 0)) == CR.PPM and not CR.similar((0, 4), 1)
    assert CR.better((2, 3), (3, 5)) and not CR.better((2, 4), (1, 2)) and CR.better((0, 0), (999999, 10 ** 6)) and not CR.better((7, 7), (0, 0))
    for i, u in ((1, 3), (2, 7), (10 ** 19, 3 * 10 ** 19), (123456789, 987654321)):  # floor: similar at sim_ppm, not one above
        s = CR.sim_ppm((i, u))
        assert CR.similar((i, u), s) and not CR.similar((i, u), s + 1)
    assert CR.prunable(0, 4, 1, None) and not CR.prunable(4, 4, CR.PPM, None) and CR.prunable(4, 5, 800001, None) and not CR.prunable(4, 5, 800000, None)
    assert CR.prunable(4, 5, 1, (4, 5)) and not CR.prunable(4, 5, 1, (3, 5))  # what cannot beat the best held is skipped, a tie too


def test_the_parser():
    assert [CR.parse(t) for t in ("1", "1.0", "0.6", "0.600001", "0.000001", ".5", "1.")] == [10 ** 6, 10 ** 6, 600000, 600001, 1, 500000, 10 ** 6]
    for bad in ("0", "1.0000001", "1.5", "-0.5", ".", "0.5x", "0.1234567", "", "1e-1", "0.5.1"):
        with pytest.raises(CR.ClusterError):
            CR.parse(bad)
    assert CR.header_line(10 ** 6) == "##povu_call_cluster=1.000000\n" and CR.header_line(1) == "##povu_call_cluster=0.000001\n"


@pytest.mark.parametrize("name", CC.CASES)
def test_no_case_is_vacuous(name):
    sites, names, paths, sq, refs, t = _case(name)
    recs, text, counters = CR.call(sites, names, paths, sq, refs, t)
    found = CR.site_clusters(sites, names, paths, sq, refs, t)
    assert any(len(f[4]) < len(f[0]) for f in found.values()) and recs
    assert len(_lines(text)) == len(recs) and counters["n_cluster_sites"] == len(found)
    plain = V.call(sites, names, paths, sq, refs)
    assert sum(len(r["alts"]) for r in recs) < sum(len(r["alts"]) for r in plain)  # fewer ALTs than the plain call writes


def test_what_the_cases_are_there_for():
    def clusters(name):
        sites, names, paths, sq, refs, t = _case(name)
        found = CR.site_clusters(sites, names, paths, sq, refs, t)
        return [found[q] for q in sorted(found)], CR.call(sites, names, paths, sq, refs, t)
    for layers in (64, 65, 129):  # bags of no key and of `layers` keys
        (f,), _ = clusters(f"braid-{layers}")
        assert sorted({len(a) - 2 for a in f[0]}) == [0, layers]
    (f,), _ = clusters("multiset")
    assert [CR.bag_of(a) for a in f[0]][:2] == [Counter({2: 3}), Counter({2: 2})] and f[3] == [0, 0, 1] and f[5] == 666666
    (f,), (recs, _, _) = clusters("empty-segments")
    assert [sum(CR.bag_of(a).values()) for a in f[0]] == [0, 1, 1, 1] and f[3] == [0, 0, 1, 0] and f[5] == CR.PPM
    (v, f), (recs, _, counters) = clusters("vanish")
    assert v[3] == [0, 0] and v[5] == 800000 and counters["n_cluster_vanished"] == 1 and {r["q"] for r in recs} == {1}
    (f,), _ = clusters("tie")
    assert f[3] == [0, 1, 0] and f[5] == 714285
    (f,), _ = clusters("best-fit")
    assert f[3] == [0, 1, 1] and f[5] == 857142
    (f,), (recs, _, _) = clusters("star")
    assert len(f[4]) == 130 and len(f[0]) == 135 and recs[0]["n_classes"] == 130 and sorted(set(recs[0]["nx"])) == [1, 2]
    _, (recs, _, _) = clusters("backward-reference")
    assert CC.case("backward-reference")[2].steps(0)[0][1] == 1 and len(recs) == 2
    for name in ("own-ref", "own-ref-backwards"):
        _, (recs, _, _) = clusters(name)
        assert [r["ref_is_rep"] for r in recs] == [False, False] and all(r["ref"] not in r["alts"] for r in recs)
    _, (recs, _, _) = clusters("two-references")
    best = [r for r in recs if r["q"] == 0]
    assert len(best) == 3 and {r["ref_class"] for r in best} == {0, 1} and [r["ref_is_rep"] for r in best] == [True, True, False]
    # the bound skips pairs in the prune case, and only there does it matter
    sites, names, paths, sq, refs, t = _case(CC.PRUNE_CASE)
    with_bound, without = CR.call(sites, names, paths, sq, refs, t), CR.call(sites, names, paths, sq, refs, t, no_bound=True)
    assert with_bound[:2] == without[:2] and with_bound[2]["n_cluster_pruned"] > 0 == without[2]["n_cluster_pruned"]
    assert with_bound[2]["n_cluster_pairs"] == without[2]["n_cluster_pairs"]


@pytest.mark.parametrize("name", [c for c in CC.CASES if c.startswith("braid")])
def test_every_braid_site_is_a_called_leaf_site(name):
    sites, names, paths, sq, refs, t = _case(name)
    g = CC.case(name)[0]
    n_sites = 5 if name == "braid-chain" else 1
    per = (g.n_vtx - 1) // n_sites
    assert sorted(V.label(s["s"], s["z"]) for s in sites) == sorted(f">{1 + i * per}>{1 + (i + 1) * per}" for i in range(n_sites))
    assert all(s["fam"] == "F" and s["parent"] == V.NO_PARENT for s in sites)
    index_paths = {k: paths[k] for k in V.ref_paths(names, refs)}
    assert all(V.called_sites(sites, index_paths))


def test_braid_shapes():
    g = W.braid(3, 4, 2, seed=1)
    assert g.n_vtx == 3 * 9 + 1 and g.n_links == 3 * (1 + 2 + 3 * 4 + 2)
    p = W.braid_haplotypes(3, 4, 2, 6, seed=1, skip=0.3, mutate=0.3, reverse_every=2)
    links = {(int(g.vid[a]), int(g.vid[b])) for a, b in zip(g.v1.tolist(), g.v2.tolist())}
    for k in range(len(p)):
        st = p.steps(k)
        fwd = st if st[0][1] == 0 else [(s, 0) for s, _ in reversed(st)]
        assert fwd[0][0] == 1 and fwd[-1][0] == g.n_vtx and all((a[0], b[0]) in links for a, b in zip(fwd, fwd[1:]))
    assert W.braid(2, 0, 3).n_links == 2  # no layer: the deletion links alone
