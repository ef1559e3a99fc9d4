"""GPU off-reference calls (povu_hip_call with POVU_HIP_T_OFFREF, `povu call --off-reference`) against the plain-Python
restatement (tests/offref_ref.py), array for array and VCF text for VCF text: the graph the feature was stated on, the hand
cases and the reference's nested-child-inside-insertion fixture -- plain, with the tier-2 scans forced, under a four-bit hash
and with inversion records; insertion_units with more samples than a wave has lanes and with diploid samples; skip_nested
with the reference through skips; 120 random small graphs, each with the flag-less call before and after; -o DIR;
the wide cohort of 131 samples in 261 slots (tests/cohort_cases.py) with a reference that ends in the middle of the chain."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cohort_cases as CC
import offref_cases as OC
import offref_ref as F
import vcf_ref as V
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W
from test_gpu_norm import _fixture_setup, _setup

pytestmark = pytest.mark.gpu

ROOT = OC.ROOT
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"
NIL = 0xFFFFFFFF
OFF_ARRAYS = ("rec_offref", "host_query", "host_allele", "off_contig_path", "off_contig_len")
GRAPHS = ["offref/" + n for n in sorted(OC.golden()["cases"])] + ["downstream_repetitive/nested-child-inside-insertion"]


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _same(c, want, counts, sites, names, steps, sq, prefixes):
    """The call's arrays and text equal the restatement's records."""
    n = len(want)
    assert c.offref and c.n_records == n
    assert [(int(c.path[i]), int(c.pos[i]), int(c.query[i]), int(c.first[i])) for i in range(n)] == \
        [(r["path"], r["pos"], r["q"], r["first"]) for r in want]
    for i, r in enumerate(want):
        a0, a1 = int(c.ac_off[i]), int(c.ac_off[i + 1])
        assert [int(x) for x in c.ac[a0:a1]] == r["ac"] and int(c.an[i]) == r["an"] and int(c.ns[i]) == r["ns"], i
    assert c.gt.tolist() == [[H.GT_MISSING if g is None else g for g in r["slots"]] for r in want]
    assert c.rec_offref.tolist() == [int(r["offref"]) for r in want]
    assert c.host_query.tolist() == [NIL if r["host"] is None else r["host"] for r in want]
    assert c.host_allele.tolist() == [NIL if r["ha"] is None else r["ha"] for r in want]
    contigs = F.off_contigs(names, want, prefixes)
    assert c.off_contig_path.tolist() == contigs
    assert c.off_contig_len.tolist() == [sum(len(sq[x[0]]) for x in steps[k]) for k in contigs]
    assert {k: getattr(c, k) for k in H.OFFREF_COUNTERS} == counts
    assert c.vcf_text(date=DATE) == F.vcf_text(sites, names, steps, sq, want, prefixes, date=DATE)
    assert c.vcf_rest_text(prefixes, date=DATE) == F.vcf_text(sites, names, steps, sq, want, prefixes, date=DATE, rest=True)


def _check(d, setup, prefixes, tflags=0):
    f, sites, names, steps, sq = setup
    want, counts = F.call(sites, names, steps, sq, prefixes, inversions=bool(tflags & H.T_INVERSIONS))
    c = d.call(f, prefixes, flags=tflags | H.T_OFFREF)
    _same(c, want, counts, sites, names, steps, sq, prefixes)
    return c, want, counts


def _without_the_flag(c):
    assert not c.offref and all(getattr(c, k).size == 0 for k in OFF_ARRAYS)
    assert all(not getattr(c._p.contents, k) for k in OFF_ARRAYS)  # NULL
    assert [getattr(c, k) for k in H.OFFREF_COUNTERS] == [0, 0, 0] and c._p.contents.n_off_contigs == 0


# ---- the graphs of the CPU tests
@pytest.mark.parametrize("tflags", [0, H.T_FORCE_TIER2, H.T_INVERSIONS], ids=["plain", "tier2", "inversions"])
def test_hand_cases_and_fixture(hip, golden_dir, tflags):
    golden = OC.golden()["cases"]
    for name in GRAPHS:
        setup = _fixture_setup(hip, golden_dir, name)
        c, want, counts = _check(hip, setup, ["HG1"], tflags)
        if name.startswith("offref/") and not tflags & H.T_INVERSIONS:
            assert OC.records_of(c.vcf_text(date=DATE)) == golden[name[len("offref/"):]]["lines"], name
            assert OC.contigs_of(c.vcf_text(date=DATE)) == golden[name[len("offref/"):]]["contigs"], name
        if not name.startswith("offref/"):  # nothing is fabricated: the records are those of the call without the flag
            plain = hip.call(setup[0], ["HG1"], flags=tflags)
            _without_the_flag(plain)
            assert c.n_offref_records == 0 and OC.records_of(c.vcf_text(date=DATE)) == OC.records_of(plain.vcf_text(date=DATE))


def _digest(c):
    h = hashlib.sha256()
    for k in ("query", "path", "first", "pos", "gt", "ac") + OFF_ARRAYS:
        h.update(np.ascontiguousarray(getattr(c, k)).tobytes())
    h.update(c.vcf_text(date=DATE).encode())
    return h.hexdigest()


def child_narrow_hash():
    """Run in a child process under POVU_HIP_TRAV_HASH_BITS=4: every graph against the restatement, the digests printed."""
    d = HipDecomposer(0)
    for name in GRAPHS:
        c, _, _ = _check(d, _fixture_setup(d, OC.GOLDEN, name), ["HG1"])
        print("DIGEST", name, _digest(c))
    d.close()


def test_narrow_hash_does_not_change_the_answer(hip, golden_dir):
    env = dict(os.environ, POVU_HIP_TRAV_HASH_BITS="4",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_offref as T; T.child_narrow_hash()"], capture_output=True, text=True,
                       timeout=600, env=env, cwd=os.path.join(ROOT, "tests"))
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("DIGEST"))
    assert got == {name: _digest(hip.call(_fixture_setup(hip, golden_dir, name)[0], ["HG1"], flags=H.T_OFFREF)) for name in GRAPHS}


# ---- the workloads
def _workload(d, g, p, seed, max_len=6):
    return _setup(d, g, W.random_sequences(g, seed, max_len=max_len), p)


def test_insertion_units_more_samples_than_lanes(hip):
    g = W.insertion_units(300, 0)
    p = W.insertion_haplotypes(300, 70, seed=5)
    c, want, counts = _check(hip, _workload(hip, g, p, 2), ["hap0#"])
    assert len(c.samples) == 70 and c.n_offref_records > 0 and c.n_offref_hosted > 0
    assert counts["n_offref_records"] == 300  # (among 69 haplotypes every insertion is carried)


def test_insertion_units_diploid(hip):
    g = W.insertion_units(300, 0)
    p = W.pansn(W.insertion_haplotypes(300, 6, seed=5), samples=3)
    c, want, counts = _check(hip, _workload(hip, g, p, 2), ["sample0#1"])
    assert len(c.samples) == 3 and c.n_slots == 6 and c.n_offref_records > 0 and c.n_offref_hosted > 0
    assert len(set(c.off_contig_path.tolist())) > 1
    _check(hip, _workload(hip, g, p, 3), ["sample0#1"], H.T_FORCE_TIER2 | H.T_INVERSIONS)


@pytest.mark.parametrize("tflags", [0, H.T_FORCE_TIER2 | H.T_INVERSIONS], ids=["plain", "tier2-inversions"])
def test_wide_cohort_partial_reference(hip, tflags):
    """131 samples, 261 slots (tests/cohort_cases.py) with the haplotype that ends in the middle of the chain as the reference: the
    six sites behind its end are called on a surrogate, the first of more than 256 paths that traverse them."""
    g, p = CC.wide_chain()
    c, want, counts = _check(hip, _setup(hip, g, CC.wide_sequences(g), p), [CC.REF_PARTIAL], tflags)
    assert c.n_slots == 261 and counts["n_offref_sites"] == counts["n_offref_records"] == 6
    assert all(r["an"] >= 258 for r in want if r["offref"])


def test_skip_nested_with_the_reference_through_skips(hip):
    g = W.skip_nested(40, 2)
    p = W.skip_haplotypes(40, 2, 6, seed=1)
    assert len(p.steps(0)) < g.n_vtx // 2  # (haplotype 0, the reference, takes skips)
    c, want, counts = _check(hip, _workload(hip, g, p, 3), ["hap0"])
    assert c.n_offref_records > 0 and c.n_offref_hosted > 0
    _check(hip, _workload(hip, g, p, 3), ["hap0"], H.T_INVERSIONS)


# ---- random small graphs
def random_case(k):
    rng = np.random.default_rng(1000 + k)
    sizes = [int(rng.integers(12, 40))] + ([int(rng.integers(10, 30))] if k % 3 == 0 else [])
    g = W.hprc_shaped(sizes, seed=500 + k, tiny=int(k % 4 == 1))
    n = 4 + k % 9
    p = W.pansn(W.random_walk_paths(g, n, int(rng.integers(20, 80)), seed=700 + k), samples=(n + 1) // 2)
    prefixes = ["sample0#1"] if k % 2 else ["sample0#1", "sample1#"]
    return g, p, prefixes, W.random_sequences(g, 900 + k, max_len=5)


def test_random_small_graphs():
    """In a context of its own: the flag-less call made before any call with the flag on the context, and behind one on
    every graph (stale workspace), is today's output."""
    hip = HipDecomposer(0)
    try:
        yielding = 0
        for k in range(120):
            g, p, prefixes, seqs = random_case(k)
            assert 4 <= len(p) <= 12
            setup = _setup(hip, g, seqs, p)
            f, sites, names, steps, sq = setup
            plain = V.vcf_text(names, steps, sq, V.call(sites, names, steps, sq, prefixes), prefixes, date=DATE)
            before = hip.call(f, prefixes)
            _without_the_flag(before)
            assert before.vcf_text(date=DATE) == plain, k
            c, want, counts = _check(hip, setup, prefixes, H.T_FORCE_TIER2 if k % 5 == 4 else 0)
            yielding += c.n_offref_records > 0
            after = hip.call(f, prefixes)
            _without_the_flag(after)
            assert after.vcf_text(date=DATE) == plain, k
            for a in ("query", "path", "first", "pos", "gt", "ac", "an", "ns", "flags", "seq", "at"):
                assert np.array_equal(getattr(after, a), getattr(before, a)), (k, a)
        assert 3 * yielding >= 120, yielding
    finally:
        hip.close()


# ---- refusals
def test_refusals(hip, golden_dir):
    f = _fixture_setup(hip, golden_dir, "offref/" + OC.ISSUE)[0]
    with pytest.raises(RuntimeError, match="POVU_HIP_T_OFFREF .*POVU_HIP_T_NESTED"):
        hip.call(f, ["HG1"], flags=H.T_OFFREF | H.T_NESTED)
    with pytest.raises(RuntimeError, match="POVU_HIP_T_OFFREF .*POVU_HIP_T_MERGE"):
        hip.call(f, ["HG1"], flags=H.T_OFFREF | H.T_MERGE, profile="decomposed")
    for profile in ("top-level-only", "popped", "left-normalized", "decomposed"):
        with pytest.raises(RuntimeError, match=f"POVU_HIP_T_OFFREF .*profile {profile}"):
            hip.call(f, ["HG1"], flags=H.T_OFFREF, profile=profile)
    assert hip.call(f, ["HG1"], flags=H.T_OFFREF, profile="raw-graph").n_offref_records == 1


# ---- the CLI
def test_output_dir_splits_off_the_off_reference_records(golden_dir, tmp_path):
    gfa = OC.gfa_of(OC.ISSUE)
    forest = tmp_path / "forest"
    forest.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", gfa, "-o", str(forest)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = OC.golden()["cases"][OC.ISSUE]["lines"]
    out = tmp_path / "vcf"
    r = subprocess.run([POVU, "call", "-i", gfa, "-f", str(forest), "-P", "HG1", "-o", str(out), "--off-reference"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == ["HG1.vcf", "off-reference.vcf"]
    assert OC.records_of((out / "HG1.vcf").read_text()) == want[:1]
    rest = (out / "off-reference.vcf").read_text()
    assert OC.records_of(rest) == want[1:] and OC.contigs_of(rest) == ["HG2#1#chr1,length=6"]
    # --stdout and gfa2vcf: one file; without the flag: the text of before, no third file
    for cmd in ([POVU, "call", "-i", gfa, "-f", str(forest), "-P", "HG1", "--off-reference"],
                [POVU, "gfa2vcf", "-i", gfa, "-P", "HG1", "--stdout", "--off-reference"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, POVU_CALL_EXE=POVU))
        assert r.returncode == 0, r.stderr
        assert OC.records_of(r.stdout) == want and OC.contigs_of(r.stdout) == OC.golden()["cases"][OC.ISSUE]["contigs"], cmd
    out2 = tmp_path / "vcf2"
    r = subprocess.run([POVU, "call", "-i", gfa, "-f", str(forest), "-P", "HG1", "-o", str(out2)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.listdir(out2) == ["HG1.vcf"]
    assert OC.records_of((out2 / "HG1.vcf").read_text()) == want[:1] and "OFFREF" not in (out2 / "HG1.vcf").read_text()
