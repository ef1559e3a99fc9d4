"""GPU merged primitives (povu_hip_call_profile under POVU_HIP_PROFILE_DECOMPOSED with POVU_HIP_T_MERGE, `povu call --profile
decomposed --merge-primitives`) against the plain-Python restatement (tests/merge_ref.py): all mrow_* arrays, the counters and the
VCF text, exactly; the record arrays and the row arrays against the same call without the flag.  The reference's two fixtures
through the library, the CLI and gfa2vcf; a hand-built chain (tests/merge_cases.py, whose conditions tests/test_merge_ref.py
checks without a GPU); complex_alleles through the striped kernel and under a nested call; skip_nested for groups across
records; the chain again under a four-bit hash; the refusals; calls without the flag, which stay as they were; and
the wide cohort of 131 samples in 261 slots (tests/cohort_cases.py)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cohort_cases as CC
import merge_cases as MC
import merge_ref as MR
import prim_cases as PC
import prim_ref as PR
import vcf_ref as V
from povu_amd import HipDecomposer
from povu_amd import hip as H
from test_gpu_norm import _fixture_setup, _setup
from test_gpu_prim import RECORD_ARRAYS, ROW_ARRAYS, _restated, _same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"
POPPED = "downstream_repetitive/popped-parent-child-rescue"
VCFWAVE = "downstream_repetitive/vcfwave-complex-decomposition"
MROW_ARRAYS = ("mrow_off", "mrow_member", "mrow_gt", "mrow_ac", "mrow_an", "mrow_ns")


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _same_merged(c, merged, counters, n_rows):
    assert c.merged and c.n_mrows == len(merged)
    off = np.cumsum([0] + [len(m["members"]) for m in merged])
    assert c.mrow_off.tolist() == off.tolist() and int(c.mrow_off[-1]) == n_rows
    assert c.mrow_member.tolist() == [x for m in merged for x in m["members"]]
    assert c.mrow_gt.tolist() == [[0xFF if v is None else v for v in m["slots"]] for m in merged]
    for k in ("ac", "an", "ns"):
        assert getattr(c, "mrow_" + k).tolist() == [m[k] for m in merged], k
    assert dict(n_mrows=c.n_mrows, **{k: getattr(c, k) for k in H.MERGE_COUNTERS}) == counters


def _check(d, setup, prefixes, tflags=0, cap=0):
    """The merged call equals the restatement, and its records and rows the call's without the flag; returns (calls, records,
    rows, merged rows, counters)."""
    f, sites, names, steps, sq = setup
    raw, rows, _, line = _restated(setup, prefixes, tflags, cap)
    merged, counters = MR.merge(raw, rows, names)
    c = d.call(f, prefixes, flags=tflags | H.T_MERGE, profile=PR.PROFILE, max_allele_length=cap)
    _same_merged(c, merged, counters, len(rows))
    plain = d.call(f, prefixes, flags=tflags, profile=PR.PROFILE, max_allele_length=cap)
    _same_records(c, plain)
    assert c.n_rows == plain.n_rows == len(rows) and not plain.merged
    for k in ROW_ARRAYS:
        assert np.array_equal(getattr(c, k), getattr(plain, k)), k
    assert (c.n_decomposed_alts, c.n_passthrough_alts, c.n_prim_tier2, c.n_prim_cells) == \
        (plain.n_decomposed_alts, plain.n_passthrough_alts, plain.n_prim_tier2, plain.n_prim_cells)
    nested = bool(tflags & H.T_NESTED)
    assert c.vcf_text(date=DATE) == MR.vcf_text(names, steps, sq, raw, rows, merged, prefixes, raw_line=line, date=DATE, nested=nested)
    assert plain.vcf_text(date=DATE) == PR.vcf_text(names, steps, sq, raw, rows, prefixes, raw_line=line, date=DATE, nested=nested)
    return c, raw, rows, merged, counters


# ---- the fixtures
def test_popped_fixture(hip, golden_dir):
    c, raw, rows, merged, counters = _check(hip, _fixture_setup(hip, golden_dir, POPPED), ["HG1"])
    assert counters == dict(n_mrows=2, n_merged_groups=1, n_merged_members=2, n_merge_splits=0, n_ref_consistent=0, n_gt_conflicts=0)
    lines = [ln.split("\t") for ln in c.vcf_text(date=DATE).splitlines() if not ln.startswith("#")]
    assert [f[1:5] + f[9:] for f in lines] == [["1", ">0>5:1:passthrough", "AAAAA", "A", "0", "1", "."], ["4", ">0>5:2:snp1", "A", "G", "0", ".", "1"]]
    assert ";MERGED=2;MERGED_FROM=>0>5:2:snp1,>2>4:1:snp1;" in lines[1][7]


def test_vcfwave_fixture(hip, golden_dir):
    setup = _fixture_setup(hip, golden_dir, VCFWAVE)
    c, raw, rows, merged, counters = _check(hip, setup, ["HG1"])
    assert counters == dict(n_mrows=4, n_merged_groups=0, n_merged_members=0, n_merge_splits=0, n_ref_consistent=2, n_gt_conflicts=0)
    by_id = {f[2]: f[9:] for f in (ln.split("\t") for ln in c.vcf_text(date=DATE).splitlines() if not ln.startswith("#"))}
    assert by_id[">9>14:1:snp1"] == ["0", "1", "0"] and by_id[">9>14:1:snp2"] == ["0", "1", "."]
    _check(hip, setup, ["HG1"], cap=8)  # a row kept whole beside the SNPs: its carrier stays '.'
    _check(hip, setup, ["HG1"], tflags=H.T_FORCE_TIER2)


@pytest.mark.parametrize("name,extra,cap", [(POPPED, [], 0), (VCFWAVE, [], 0), (VCFWAVE, ["--max-allele-length", "8"], 8)])
def test_fixtures_through_the_cli_and_gfa2vcf(golden_dir, tmp_path, name, extra, cap):
    gfa = os.path.join(golden_dir, "gfa", name + ".gfa")
    out = tmp_path / "forest"
    out.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", gfa, "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names, paths, seqs = V.read_gfa(gfa)
    sites = V.sites_of_pvst([(out / p).read_text() for p in sorted(os.listdir(out), key=lambda x: int(x.split(".")[0])) if p.endswith(".pvst")])
    raw, rows, _, line = _restated((None, sites, names, paths, seqs), ["HG1"], 0, cap)
    merged, _ = MR.merge(raw, rows, names)
    want = MR.vcf_text(names, paths, seqs, raw, rows, merged, ["HG1"], raw_line=line, date=DATE).split("\n", 2)[2]
    for cmd in ([POVU, "call", "-i", gfa, "-f", str(out), "-P", "HG1", "--profile", "decomposed", "--merge-primitives"] + extra,
                [POVU, "gfa2vcf", "-i", gfa, "-P", "HG1", "--stdout", "--profile=decomposed", "--merge-primitives"] + extra):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, POVU_CALL_EXE=POVU))
        assert r.returncode == 0, r.stderr
        assert r.stdout.split("\n", 2)[2] == want, cmd  # (behind the date line)
    assert ("MERGED_FROM=>0>5:2:snp1,>2>4:1:snp1" in want) == (name == POPPED)


# ---- the chain
def test_chain(hip):
    setup = _setup(hip, *MC.chain_case())
    c, raw, rows, merged, counters = _check(hip, setup, MC.CHAIN_REFS, cap=MC.CHAIN_CAP)
    MC.chain_coverage(raw, rows, merged, counters)
    c2, _, _, _, _ = _check(hip, setup, MC.CHAIN_REFS, tflags=H.T_FORCE_TIER2 | H.T_INVERSIONS, cap=MC.CHAIN_CAP)
    assert c2.vcf_text(date=DATE) == c.vcf_text(date=DATE)


# ---- differential
def test_complex_alleles(hip):
    setup = _setup(hip, *PC.complex_case(1))
    c, raw, rows, merged, counters = _check(hip, setup, ["hap0"], tflags=H.T_FORCE_TIER2, cap=PC.COMPLEX_CAP)
    MC.carrying(rows, merged, counters)
    c2, _, rows2, merged2, counters2 = _check(hip, setup, ["hap0", "hap3"], tflags=H.T_NESTED)
    assert c2.nested and counters2["n_merged_groups"] >= 1


def test_skip_nested_groups_across_records(hip):
    setup = _setup(hip, *MC.skip_case())
    c, raw, rows, merged, counters = _check(hip, setup, ["hap0"])
    MC.carrying(rows, merged, counters)
    assert sum(len({rows[x]["rec"] for x in m["members"]}) > 1 for m in merged) >= 10


# ---- more samples than lanes, three times over
@pytest.mark.parametrize("ref, groups", [(CC.REF_LOW, 4), (CC.REF_HIGH, 1)])
def test_wide_cohort(hip, ref, groups):
    """131 samples, 261 slots (tests/cohort_cases.py): the vote's lane-per-sample loop takes three rounds; merged rows and the
    counters, both tiers."""
    g, p = CC.wide_chain()
    setup = _setup(hip, g, CC.wide_sequences(g), p)
    c, raw, rows, merged, counters = _check(hip, setup, [ref], tflags=H.T_INVERSIONS)
    assert c.n_slots == 261 and counters["n_merged_groups"] == groups and counters["n_ref_consistent"] >= 100
    c2, _, _, _, counters2 = _check(hip, setup, [ref], tflags=H.T_INVERSIONS | H.T_FORCE_TIER2)
    assert counters2 == counters and c2.vcf_text(date=DATE) == c.vcf_text(date=DATE)


# ---- collisions
def _digest(c):
    h = hashlib.sha256()
    for k in RECORD_ARRAYS + ROW_ARRAYS + MROW_ARRAYS:
        h.update(np.ascontiguousarray(getattr(c, k)).tobytes())
    h.update(repr([getattr(c, k) for k in H.MERGE_COUNTERS if k != "n_merge_splits"]).encode())
    h.update(c.vcf_text(date=DATE).encode())
    return h.hexdigest()


def child_narrow_hash():
    """Run in a child process under POVU_HIP_TRAV_HASH_BITS=4: the chain against the restatement but for the splits, its digest
    printed."""
    d = HipDecomposer(0)
    setup = _setup(d, *MC.chain_case())
    f, sites, names, steps, sq = setup
    raw, rows, _, line = _restated(setup, MC.CHAIN_REFS, 0, MC.CHAIN_CAP)
    merged, counters = MR.merge(raw, rows, names)
    c = d.call(f, MC.CHAIN_REFS, flags=H.T_MERGE, profile=PR.PROFILE, max_allele_length=MC.CHAIN_CAP)
    assert c.n_merge_splits > 0  # (the hook is in force: sixteen hash values collide)
    _same_merged(c, merged, dict(counters, n_merge_splits=c.n_merge_splits), len(rows))
    print("DIGEST", _digest(c))
    d.close()


def test_narrow_hash_does_not_change_the_answer(hip):
    setup = _setup(hip, *MC.chain_case())
    c = hip.call(setup[0], MC.CHAIN_REFS, flags=H.T_MERGE, profile=PR.PROFILE, max_allele_length=MC.CHAIN_CAP)
    assert c.n_merge_splits == 0
    env = dict(os.environ, POVU_HIP_TRAV_HASH_BITS="4",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_merge as T; T.child_narrow_hash()"], capture_output=True, text=True,
                       timeout=600, env=env, cwd=os.path.join(ROOT, "tests"))
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()
    assert line[1] == _digest(c)


# ---- refusals
def test_refusals(hip, golden_dir):
    setup = _fixture_setup(hip, golden_dir, VCFWAVE)
    for profile in (None, "raw-graph", "top-level-only", "popped", "left-normalized"):
        with pytest.raises(RuntimeError, match=f"POVU_HIP_T_MERGE .*decomposed.* {profile or 'raw-graph'}"):
            hip.call(setup[0], ["HG1"], flags=H.T_MERGE, profile=profile)
    for extra in ([], ["--profile", "left-normalized"], ["--nested"]):
        r = subprocess.run([POVU, "call", "-i", "x.gfa", "-P", "a", "--merge-primitives"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--merge-primitives" in r.stderr + r.stdout and "--profile decomposed" in r.stderr + r.stdout


# ---- the flag off
def test_without_the_flag():
    """In a context of its own: `before` is a decomposed call made before any merged call there (none of the step's arenas exists
    yet) and `after` one made behind one."""
    hip = HipDecomposer(0)
    try:
        setup = _setup(hip, *PC.complex_case(1))
        f = setup[0]
        kw = dict(profile=PR.PROFILE, max_allele_length=PC.COMPLEX_CAP)
        before = hip.call(f, ["hap0"], **kw)
        with_flag = hip.call(f, ["hap0"], flags=H.T_MERGE, **kw)
        assert with_flag.merged and 0 < with_flag.n_mrows < with_flag.n_rows
        after = hip.call(f, ["hap0"], **kw)
        for c in (before, after, hip.call(f, ["hap0"], flags=H.T_NESTED, **kw), hip.call(f, ["hap0"])):
            assert not c.merged and c.n_mrows == 0 and all(getattr(c, k).size == 0 for k in MROW_ARRAYS)
            assert all(not getattr(c._p.contents, k) for k in MROW_ARRAYS)  # NULL
            assert [getattr(c, k) for k in H.MERGE_COUNTERS] == [0] * len(H.MERGE_COUNTERS)
        _same_records(after, before)
        for k in ROW_ARRAYS:
            assert np.array_equal(getattr(after, k), getattr(before, k)), k
        assert after.vcf_text(date=DATE) == before.vcf_text(date=DATE)
    finally:
        hip.close()
