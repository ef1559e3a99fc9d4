"""GPU decomposed calls (povu_hip_call_profile under POVU_HIP_PROFILE_DECOMPOSED, `povu call --profile decomposed`) against the
plain-Python restatement (tests/prim_ref.py): all 14 row arrays, the four counters, the record arrays against the raw call's
and the VCF text, exactly.  The reference's two fixtures through the library, the CLI and gfa2vcf; a hand-built chain with texts
on and around the stripes of the second-tier kernel and the cap, anchors on the context, the row rules and the sort
(tests/prim_cases.py, whose conditions tests/test_prim_inputs.py checks without a GPU); complex_alleles against the
restatement; everything again through the striped kernel; the nested call and the inversion records beside it; the refusals;
calls without the profile, which stay as they were; and the wide cohort of 131 samples in 261 slots (tests/cohort_cases.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import cohort_cases as CC
import inversions_ref as I
import nested_ref as N
import prim_cases as PC
import prim_ref as PR
import vcf_ref as V
from povu_amd import HipDecomposer
from povu_amd import hip as H
from test_gpu_norm import _fixture_setup, _setup, chain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"
VCFWAVE = "downstream_repetitive/vcfwave-complex-decomposition"
SUBR = "downstream_repetitive/subr-inversion-preservation"
ROW_ARRAYS = ("row_record", "row_alt", "row_kind", "row_reason", "row_index", "row_pos", "row_ref_start", "row_ref_len", "row_alt_start",
              "row_alt_len", "row_lead", "row_ac", "row_an", "row_ns")
ROW_KEYS = ("rec", "alt", "kind", "reason", "index", "pos", "ref_start", "ref_len", "alt_start", "alt_len", "lead", "ac", "an", "ns")
RECORD_ARRAYS = ("query", "path", "first", "ref_allele", "n_alleles", "an", "ns", "block", "pos", "flags", "ac_off", "ac", "gt", "block_off",
                 "seq_off", "at_off", "seq", "at", "n_steps", "level", "parent_query", "ref_spelled", "raw_pos", "norm_block")


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _restated(setup, prefixes, tflags=0, cap=0):
    """(raw records, rows, counters, the writer of a raw line) by the restatement."""
    f, sites, names, steps, sq = setup
    nested = bool(tflags & H.T_NESTED)
    raw = N.call(sites, names, steps, sq, prefixes) if nested else V.call(sites, names, steps, sq, prefixes)
    line = N.record_line if nested else V.record_line
    if tflags & H.T_INVERSIONS:
        raw = I.merge(raw, I.records(names, steps, sq, prefixes)[0])
        flubble_line = line
        line = lambda r: I.record_line(r) if r["vartype"] == "SUBR" else flubble_line(r)  # noqa: E731
    rows, counters = PR.decompose(raw, names, steps, sq, max_allele_length=cap, force_tier2=bool(tflags & H.T_FORCE_TIER2))
    return raw, rows, counters, line


def _same_records(c, plain):
    assert c.n_records == plain.n_records
    for k in RECORD_ARRAYS:
        assert np.array_equal(np.asarray(getattr(c, k)), np.asarray(getattr(plain, k))), k


def _check(d, setup, prefixes, tflags=0, cap=0):
    """The call under the profile equals the restatement, and its records the raw call's; returns (calls, records, rows, counters)."""
    f, sites, names, steps, sq = setup
    raw, rows, counters, line = _restated(setup, prefixes, tflags, cap)
    c = d.call(f, prefixes, flags=tflags, profile=PR.PROFILE, max_allele_length=cap)
    assert c.n_rows == len(rows) == counters["n_rows"]
    for name, key in zip(ROW_ARRAYS, ROW_KEYS):
        want = [ord(r[key]) if r[key] else 0 for r in rows] if key == "lead" else [r[key] for r in rows]
        assert getattr(c, name).tolist() == want, name
    assert dict(n_rows=c.n_rows, n_decomposed_alts=c.n_decomposed_alts, n_passthrough_alts=c.n_passthrough_alts, n_prim_tier2=c.n_prim_tier2,
                n_prim_cells=c.n_prim_cells) == counters
    _same_records(c, d.call(f, prefixes, flags=tflags))
    nested = bool(tflags & H.T_NESTED)
    assert c.vcf_text(date=DATE) == PR.vcf_text(names, steps, sq, raw, rows, prefixes, raw_line=line, date=DATE, nested=nested)
    return c, raw, rows, counters


def _both_tiers(d, setup, prefixes, tflags=0, cap=0):
    """... and again with every aligned pair through the striped kernel: the same rows."""
    c, raw, rows, counters = _check(d, setup, prefixes, tflags, cap)
    c2, _, rows2, counters2 = _check(d, setup, prefixes, tflags | H.T_FORCE_TIER2, cap)
    assert rows2 == rows and c2.vcf_text(date=DATE) == c.vcf_text(date=DATE)
    aligned = sum(PR.pair_rows(r["ref"], a, r["pos"], "N" * r["pos"], cap or PR.MAX_LENGTH, r["vartype"] == "SUBR")[1] > 0 for r in raw for a in r["alts"])
    assert counters2["n_prim_tier2"] == c2.n_prim_tier2 == aligned
    return c, raw, rows, counters


# ---- the fixtures
def test_vcfwave_fixture(hip, golden_dir):
    """The three rows INTEGRATION.md spells out, and the four of the fixture without a cap."""
    setup = _fixture_setup(hip, golden_dir, VCFWAVE)
    c, raw, rows, counters = _both_tiers(hip, setup, ["HG1"], cap=8)
    assert counters == dict(n_rows=3, n_decomposed_alts=1, n_passthrough_alts=1, n_prim_tier2=0, n_prim_cells=16)
    lines = [ln.split("\t") for ln in c.vcf_text(date=DATE).splitlines() if not ln.startswith("#")]
    assert [(f[1], f[2], f[3], f[4]) for f in lines] == [("2", ">9>14:1:snp1", "C", "T"), ("2", ">9>14:2:passthrough", "CGT", "CGTACGTACGTA"),
                                                        ("4", ">9>14:1:snp2", "T", "A")]
    c, raw, rows, counters = _both_tiers(hip, setup, ["HG1"])
    assert counters == dict(n_rows=4, n_decomposed_alts=2, n_passthrough_alts=0, n_prim_tier2=0, n_prim_cells=16 + 4 * 13)
    assert [(r["alt"], r["kind"], r["index"], r["pos"]) for r in rows] == [(2, PR.ROW_INS, 1, 1), (1, PR.ROW_SNP, 1, 2), (1, PR.ROW_SNP, 2, 4),
                                                                         (2, PR.ROW_INS, 2, 4)]


def test_subr_fixture(hip, golden_dir):
    want = json.load(open(os.path.join(golden_dir, "reference_decomposed_records.json")))["fixtures"][SUBR]
    setup = _fixture_setup(hip, golden_dir, SUBR)
    c, raw, rows, counters = _both_tiers(hip, setup, [want["reference_prefix"]], tflags=H.T_INVERSIONS)
    (w,) = want["rows"]
    line = next(ln for ln in c.vcf_text(date=DATE).splitlines() if "SUBR_ORIGIN=T" in ln).split("\t")
    assert line[:7] == [w["chrom"], str(w["pos"]), w["id"], w["ref"], w["alt"], "60", "PASS"] and line[9:] == w["gt"]
    assert line[7] == ";".join(f"{k}={w['info'][k]}" for k in w["info_keys_in_order"])
    assert PR.REASON_SUBR in c.row_reason.tolist()


@pytest.mark.parametrize("name,prefix,extra,tflags,cap", [(VCFWAVE, "HG1", ["--max-allele-length", "8"], 0, 8), (VCFWAVE, "HG1", [], 0, 0),
                                                         (SUBR, None, ["--inversions"], H.T_INVERSIONS, 0)])
def test_fixtures_through_the_cli_and_gfa2vcf(golden_dir, tmp_path, name, prefix, extra, tflags, cap):
    want_json = json.load(open(os.path.join(golden_dir, "reference_decomposed_records.json")))["fixtures"][name]
    prefix = prefix or want_json["reference_prefix"]
    gfa = os.path.join(golden_dir, "gfa", name + ".gfa")
    out = tmp_path / "forest"
    out.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", gfa, "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names, paths, seqs = V.read_gfa(gfa)
    sites = V.sites_of_pvst([(out / p).read_text() for p in sorted(os.listdir(out), key=lambda x: int(x.split(".")[0])) if p.endswith(".pvst")])
    raw, rows, counters, line = _restated((None, sites, names, paths, seqs), [prefix], tflags, cap)
    want = PR.vcf_text(names, paths, seqs, raw, rows, [prefix], raw_line=line, date=DATE).split("\n", 2)[2]
    for cmd in ([POVU, "call", "-i", gfa, "-f", str(out), "-P", prefix, "--profile", "decomposed"] + extra,
                [POVU, "gfa2vcf", "-i", gfa, "-P", prefix, "--stdout", "--profile=decomposed"] + extra):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, POVU_CALL_EXE=POVU))
        assert r.returncode == 0, r.stderr
        assert r.stdout.split("\n", 2)[2] == want, cmd  # (behind the date line)
    if cap == 8:
        assert "\t2\t>9>14:1:snp1\tC\tT\t" in want and "\t4\t>9>14:1:snp2\tT\tA\t" in want and "\t2\t>9>14:2:passthrough\tCGT\tCGTACGTACGTA\t" in want


def test_cli_refusals(tmp_path):
    r = subprocess.run([POVU, "call", "-i", "x.gfa", "-P", "a", "--profile", "shuffled"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "raw-graph, top-level-only, popped, left-normalized or decomposed" in r.stderr + r.stdout


# ---- the chain
@pytest.fixture(scope="module")
def chain_setup(hip):
    return PC.chain_case()


def test_chain(hip, chain_setup):
    setup = _setup(hip, *chain_setup)
    c, raw, rows, counters = _both_tiers(hip, setup, PC.CHAIN_REFS)
    _, _, rows_inv, _ = _both_tiers(hip, setup, ["hap0"], tflags=H.T_INVERSIONS)
    PC.chain_coverage(rows, raw, rows_inv)
    PC.coverage(rows_inv)
    assert counters["n_prim_tier2"] >= 10


def test_chain_nested_and_inversions(hip, chain_setup):
    setup = _setup(hip, *chain_setup)
    c, raw, rows, counters = _check(hip, setup, PC.CHAIN_REFS, tflags=H.T_NESTED)
    PC.coverage(rows)
    assert c.nested
    _check(hip, setup, ["hap0"], tflags=H.T_INVERSIONS | H.T_NESTED | H.T_FORCE_TIER2, cap=64)


# ---- differential
@pytest.mark.parametrize("seed", PC.COMPLEX_SEEDS)
def test_complex_alleles(hip, seed):
    setup = _setup(hip, *PC.complex_case(seed))
    c, raw, rows, counters = _both_tiers(hip, setup, ["hap0"], cap=PC.COMPLEX_CAP)
    PC.coverage(rows)
    if seed == 1:
        _check(hip, setup, ["hap0", "hap3"], tflags=H.T_NESTED)


# ---- more samples than lanes
@pytest.mark.parametrize("ref", CC.REFS)
def test_wide_cohort(hip, ref):
    """131 samples, 261 slots (tests/cohort_cases.py): the rows' genotype counts come from three rounds of the lane-per-sample
    loop, plain and with the inversion records."""
    g, p = CC.wide_chain()
    setup = _setup(hip, g, CC.wide_sequences(g), p)
    c, raw, rows, counters = _both_tiers(hip, setup, [ref], tflags=H.T_INVERSIONS)
    assert c.n_slots == 261 and len(rows) >= 59 and max(r["an"] for r in rows) >= 187
    _both_tiers(hip, setup, [ref])


# ---- refusals
def test_refusals(hip, golden_dir):
    setup = _fixture_setup(hip, golden_dir, VCFWAVE)
    with pytest.raises(RuntimeError, match="max_allele_length 513 is above the ceiling 512"):
        hip.call(setup[0], ["HG1"], profile=PR.PROFILE, max_allele_length=513)
    hip.call(setup[0], ["HG1"], profile=PR.PROFILE, max_allele_length=512)
    # the base in front of POS that anchors an indel at offset 0 is no nucleotide code: the raw call never spells it
    g, seqs, p = chain([("s", "AC", 0), ("s", "!", 0), ("b", ["AA", "A"], False), ("s", "GT", 0)], [[1], [2]])
    setup = _setup(hip, g, seqs, p)
    assert hip.call(setup[0], ["hap0"]).n_records == 1
    with pytest.raises(RuntimeError, match="segment 2 holds a byte that is no nucleotide code"):
        hip.call(setup[0], ["hap0"], profile=PR.PROFILE)


# ---- the profile off
def test_without_the_profile():
    """In a context of its own, so that `before` is a call made before any decomposed call there (none of the step's arenas
    exists yet) and `after` one made behind them."""
    hip = HipDecomposer(0)
    try:
        _without_the_profile(hip)
    finally:
        hip.close()


def _without_the_profile(hip):
    setup = _setup(hip, *PC.complex_case(1))
    f = setup[0]
    before = hip.call(f, ["hap0"])
    with_profile = hip.call(f, ["hap0"], profile=PR.PROFILE, max_allele_length=PC.COMPLEX_CAP)
    assert with_profile.n_rows > 0
    for kw in (dict(), dict(profile="raw-graph"), dict(profile="left-normalized"), dict(flags=H.T_NESTED)):
        c = hip.call(f, ["hap0"], **kw)
        assert c.n_rows == 0 and all(getattr(c, k).size == 0 for k in ROW_ARRAYS)
        assert all(not getattr(c._p.contents, k) for k in ROW_ARRAYS)  # NULL
        assert (c.n_decomposed_alts, c.n_passthrough_alts, c.n_prim_tier2, c.n_prim_cells) == (0, 0, 0, 0)
    after = hip.call(f, ["hap0"])
    _same_records(after, before)
    assert after.vcf_text(date=DATE) == before.vcf_text(date=DATE)
