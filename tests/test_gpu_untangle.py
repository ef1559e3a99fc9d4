"""GPU untangled calls (povu_hip_call with POVU_HIP_T_UNTANGLE, `povu call --untangle`) against the plain-Python restatement
(tests/untangle_ref.py), every output array and the VCF text: the graph the feature was stated on; chains of loop sites
(workloads.vntr_haplotypes), forwards, with haplotypes walking backwards and with a slot on two contigs; one site at the edges
of the aligner (64 laps a side, the 65th, one lap against many); 131 samples on one looped site; a graph without loops; the
same call repeated and after release_workspace; with inversion records; the refusals; the VCF checks; the command line."""
import os
import subprocess

import numpy as np
import pytest

import cohort_cases as CC
import untangle_cases as UC
import untangle_ref as U
import vcf_ref as V
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W
from test_gpu_norm import _fixture_setup, _setup

pytestmark = pytest.mark.gpu

POVU = os.path.join(UC.ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"
UNT_ARRAYS = ("rec_unt", "lap", "n_laps", "lap_count")


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _same(c, want, counts, names, steps, sq, prefixes):
    """The call's arrays and text equal the restatement's records."""
    n = len(want)
    assert c.untangled and c.n_records == n
    assert [(int(c.path[i]), int(c.pos[i]), int(c.query[i]), int(c.first[i])) for i in range(n)] == \
        [(r["path"], r["pos"], r["q"], r["first"]) for r in want]
    assert c.gt.tolist() == [[H.GT_MISSING if g is None else g for g in r["slots"]] for r in want]
    for i, r in enumerate(want):
        a0, a1 = int(c.ac_off[i]), int(c.ac_off[i + 1])
        assert [int(x) for x in c.ac[a0:a1]] == r["ac"] and int(c.an[i]) == r["an"] and int(c.ns[i]) == r["ns"], i
    assert [bool(f & H.CALL_TANGLED) for f in c.flags.tolist()] == [bool(r["tangled"]) for r in want]
    assert c.rec_unt.tolist() == [int(r["unt"]) for r in want]
    assert c.lap.tolist() == [r["lap"] for r in want] and c.n_laps.tolist() == [r["n_laps"] for r in want]
    assert c.lap_count.tolist() == [r["lap_count"] for r in want]
    assert {k: getattr(c, k) for k in H.UNTANGLE_COUNTERS} == counts
    assert c.vcf_text(date=DATE) == U.vcf_text(names, steps, sq, want, prefixes, date=DATE)


def _check(d, setup, prefixes, tflags=0):
    f, sites, names, steps, sq = setup
    want, counts = U.call(sites, names, steps, sq, prefixes, inversions=bool(tflags & H.T_INVERSIONS))
    c = d.call(f, prefixes, flags=tflags | H.T_UNTANGLE)
    _same(c, want, counts, names, steps, sq, prefixes)
    return c, want, counts


def _without_the_flag(c):
    assert not c.untangled and all(getattr(c, k).size == 0 for k in UNT_ARRAYS)
    assert all(not getattr(c._p.contents, k) for k in UNT_ARRAYS)  # NULL
    assert [getattr(c, k) for k in H.UNTANGLE_COUNTERS] == [0] * 5


def _workload(d, g, p, seed=3):
    return _setup(d, g, UC.sequences(g, seed), p)


def test_the_fixture(hip, golden_dir):
    setup = _fixture_setup(hip, golden_dir, UC.FIXTURE)
    c, want, counts = _check(hip, setup, ["HG1"])
    gold = UC.golden()
    assert [ln for ln in c.vcf_text(date=DATE).splitlines() if not ln.startswith("#")] == gold["lines"]
    assert counts == gold["counters"] and counts["n_unt_tasks"] == 2
    assert c.lap_count.tolist() == [[3, 2, 4]] * 3
    plain = hip.call(setup[0], ["HG1"])
    _without_the_flag(plain)
    assert [ln for ln in plain.vcf_text(date=DATE).splitlines() if not ln.startswith("#")] == gold["plain_lines"]


@pytest.mark.parametrize("seed,reverse_every,two_contigs", [(1, 0, False), (2, 3, False), (3, 0, True)],
                         ids=["forwards", "backwards", "two-contigs"])
def test_chains_of_loop_sites(hip, seed, reverse_every, two_contigs):
    g, p = W.vntr_haplotypes(40, 12, 6, seed, reverse_every=reverse_every)
    if two_contigs:  # haplotypes 4 and 5 become two contigs of one slot: its entries fall back
        p.names[5] = "hap4#1#chr2"
    c, want, counts = _check(hip, _workload(hip, g, p, seed), ["hap0#"])
    assert counts["n_unt_tasks"] > 300 and counts["n_unt_missing"] > 0 and counts["n_unt_extra"] > 0
    assert len(c.samples) == (11 if two_contigs else 12)
    if two_contigs:
        sl = c.samples.index("hap4")
        assert all(r["lap_count"][sl] >= 2 for r in want) and counts["n_unt_fallback"] >= len(want)


@pytest.mark.parametrize("n,m", [(64, 64), (64, 65), (65, 3), (33, 1), (1, 33)])
def test_one_site_at_the_edges_of_the_aligner(hip, n, m):
    g, p = UC.two_paths(n, m, seed=n * 100 + m)
    c, want, counts = _check(hip, _workload(hip, g, p), ["ref#"])
    assert len(want) == n and c.n_laps.tolist() == [n] * n and c.lap_count.tolist() == [[n, m]] * n
    if max(n, m) <= 64:
        assert counts["n_unt_tasks"] == 1 and counts["n_unt_records"] == n and counts["n_unt_fallback"] == (n if n >= 2 else 0)
        assert counts["n_unt_missing"] - counts["n_unt_extra"] == n - m
    elif n == 64:  # the haplotype's 65 laps: its entries fall back, and so do the reference's own
        assert counts["n_unt_tasks"] == 0 and counts["n_unt_fallback"] == 2 * n and not c.rec_unt.any()
    else:  # the reference's 65 laps leave the whole site to the old rule
        assert counts["n_unt_tasks"] == 0 and counts["n_unt_fallback"] == 2 * n and not c.rec_unt.any()
        plain = hip.call(_workload(hip, g, p)[0], ["ref#"])
        assert np.array_equal(plain.gt, c.gt) and np.array_equal(plain.flags, c.flags)


def test_131_samples_on_one_looped_site(hip):
    g, p = UC.wide_site()
    c, want, counts = _check(hip, _workload(hip, g, p), [CC.REF_LOW])
    assert len(c.samples) == 131 and c.n_slots == 261 and counts["n_unt_tasks"] >= 200
    sample_of = CC.sample_of_slots(list(p.names))
    for r in want:  # a loop that stopped after one or two rounds of 64 samples would count otherwise
        assert CC.restricted_differs(r["slots"], sample_of, 64, r["ac"], r["an"], r["ns"])
        assert CC.restricted_differs(r["slots"], sample_of, 128, r["ac"], r["an"], r["ns"])


def test_a_graph_without_loops(hip):
    g = W.chain_of_bubbles(60)
    p = W.pansn(W.chain_haplotypes(60, 9, seed=3), samples=5)
    setup = _setup(hip, g, W.random_sequences(g, 4, max_len=5), p)
    plain = hip.call(setup[0], ["sample0#1"])
    _without_the_flag(plain)
    c, want, counts = _check(hip, setup, ["sample0#1"])
    assert counts["n_unt_tasks"] == 0 and counts["n_unt_records"] == 0 and c.n_records > 20
    for a in ("gt", "ac", "an", "ns", "flags", "pos", "seq", "at"):
        assert np.array_equal(getattr(c, a), getattr(plain, a)), a
    a, b = plain.vcf_text(date=DATE).splitlines(), c.vcf_text(date=DATE).splitlines()
    k = len(V.HEADER.splitlines())
    assert b[:k] == a[:k] and b[k + 3:] == a[k:] and [ln + "\n" for ln in b[k:k + 3]] == U.HEADER_LINES.splitlines(True)


def _digest(c):
    return [np.ascontiguousarray(getattr(c, k)).tobytes() for k in ("query", "path", "first", "pos", "gt", "ac", "an", "ns", "flags") + UNT_ARRAYS] + \
        [c.vcf_text(date=DATE)] + [getattr(c, k) for k in H.UNTANGLE_COUNTERS]


def test_the_same_call_twice_and_after_release_workspace():
    hip = HipDecomposer(0)
    try:
        g, p = W.vntr_haplotypes(20, 8, 5, 11, reverse_every=4)
        setup = _workload(hip, g, p, 5)
        plain = hip.call(setup[0], ["hap0#"]).vcf_text(date=DATE)
        first = _digest(_check(hip, setup, ["hap0#"])[0])
        assert _digest(hip.call(setup[0], ["hap0#"], flags=H.T_UNTANGLE)) == first
        assert hip.call(setup[0], ["hap0#"]).vcf_text(date=DATE) == plain  # (the flag-less call behind one with the flag)
        hip.release_workspace()
        assert _digest(hip.call(setup[0], ["hap0#"], flags=H.T_UNTANGLE)) == first
    finally:
        hip.close()


def test_with_inversions_the_subr_records_stay(hip):
    g, p = W.vntr_haplotypes(12, 6, 4, 21)
    q = W.inverted_haplotypes(p, 3, 2, 5, seed=4, keep=(0,))
    setup = _workload(hip, g, q, 6)
    c, want, counts = _check(hip, setup, ["hap0#"], H.T_INVERSIONS)
    plain = hip.call(setup[0], ["hap0#"], flags=H.T_INVERSIONS)
    subr = lambda x: [ln for ln in x.vcf_text(date=DATE).splitlines() if "VARTYPE=SUBR" in ln]  # noqa: E731
    assert c.n_inv_records == plain.n_inv_records and subr(c) == subr(plain)
    for i in np.flatnonzero(c.flags & H.CALL_SUBR).tolist():
        assert not c.rec_unt[i] and c.lap[i] == 0 and c.n_laps[i] == 0 and not c.lap_count[i].any()


def test_refusals(hip, golden_dir):
    f = _fixture_setup(hip, golden_dir, UC.FIXTURE)[0]
    with pytest.raises(RuntimeError, match="POVU_HIP_T_UNTANGLE .*POVU_HIP_T_NESTED"):
        hip.call(f, ["HG1"], flags=H.T_UNTANGLE | H.T_NESTED)
    with pytest.raises(RuntimeError, match="POVU_HIP_T_UNTANGLE .*POVU_HIP_T_MERGE"):
        hip.call(f, ["HG1"], flags=H.T_UNTANGLE | H.T_MERGE)
    with pytest.raises(RuntimeError, match="POVU_HIP_T_UNTANGLE .*POVU_HIP_T_OFFREF"):
        hip.call(f, ["HG1"], flags=H.T_UNTANGLE | H.T_OFFREF)
    for profile in ("top-level-only", "popped", "left-normalized", "decomposed"):
        with pytest.raises(RuntimeError, match=f"POVU_HIP_T_UNTANGLE .*profile {profile}"):
            hip.call(f, ["HG1"], flags=H.T_UNTANGLE, profile=profile)
    assert hip.call(f, ["HG1"], flags=H.T_UNTANGLE, profile="raw-graph").n_unt_records == 3


def test_the_vcf_checks_accept_the_untangled_text(hip):
    g, p = W.vntr_haplotypes(15, 7, 5, 31, reverse_every=3)
    setup = _workload(hip, g, p, 8)
    c, _, _ = _check(hip, setup, ["hap0#"])
    rep = hip.check_vcf(c.vcf_text(date=DATE), spelling=True)
    assert rep.n_records == c.n_records and rep.n_invalid == 0 and rep.n_misspelled == 0 and rep.summary_text() == "No errors\n"


def _body(text):
    return [ln for ln in text.splitlines() if not ln.startswith("##fileDate")]


def test_the_command_line(hip, golden_dir, tmp_path):
    c = hip.call(_fixture_setup(hip, golden_dir, UC.FIXTURE)[0], ["HG1"], flags=H.T_UNTANGLE)
    forest = tmp_path / "forest"
    forest.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", UC.GFA, "-o", str(forest)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for cmd in ([POVU, "call", "-i", UC.GFA, "-f", str(forest), "-P", "HG1", "--untangle", "--stdout"],
                [POVU, "gfa2vcf", "-i", UC.GFA, "-P", "HG1", "--stdout", "--untangle"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, POVU_CALL_EXE=POVU))
        assert r.returncode == 0, r.stderr
        assert _body(r.stdout) == _body(c.vcf_text()), cmd
    for more, word in ((["--nested"], "--nested"), (["--off-reference"], "--off-reference"), (["--profile", "decomposed"], "raw-graph"),
                       (["--profile", "decomposed", "--merge-primitives"], "--merge-primitives")):
        r = subprocess.run([POVU, "call", "-i", UC.GFA, "-f", str(forest), "-P", "HG1", "--untangle"] + more, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and "--untangle" in r.stderr and word in r.stderr, (more, r.stderr)
