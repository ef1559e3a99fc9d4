"""GPU region calls (povu_hip_call_restricted, HipDecomposer.call(regions=...), `povu call --region`) against the plain-Python
restatement (tests/region_ref.py) composed with the restatements of the modes: the VCF text, the records' keys, and every
per-record array, genotype row, count and spelled allele against the same call without regions at the records the restatement
keeps; each case again with region_no_mask (every site scanned, the records selected at the end): the same digest.  The cases are
those of tests/region_cases.py, none of them vacuous (tests/test_region_ref.py): the fixture's rows; a chain whose marks span
six words with regions around a boundary segment's first and last base, overlapping, on two paths, seventy at once, on a
haplotype and on one that walks backwards; loop sites with one lap inside; wide segment ids; every mode.  Then a region without
records, the same call twice and after release_workspace, a call without regions behind one with, the refusals, the command
line and `povu vcf --report --spelling` on a region call's text."""
import json
import os
import subprocess

import numpy as np
import pytest

import region_cases as RC
import region_ref as R
from povu_amd import HipDecomposer
from povu_amd import hip as H
from test_gpu_norm import _fixture_setup, _setup

pytestmark = pytest.mark.gpu

POVU = os.path.join(RC.ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"
NESTED_MODES = ("nested", "top-level-only", "popped")
RECORD_ARRAYS = ("query", "path", "first", "ref_allele", "n_alleles", "an", "ns", "pos", "flags", "n_steps", "level", "parent_query", "raw_pos",
                 "norm_shift", "norm_chop", "norm_trim")
UNT_ARRAYS = ("rec_unt", "lap", "n_laps", "lap_count")
ALL_ARRAYS = RECORD_ARRAYS + UNT_ARRAYS + ("block", "ref_spelled", "norm_block", "gt", "ac_off", "ac", "block_off", "seq_off", "at_off", "seq", "at",
                                           "contig_len", "row_record", "row_alt", "row_kind", "row_reason", "row_index", "row_pos", "row_ref_start",
                                           "row_ref_len", "row_alt_start", "row_alt_len", "row_lead", "row_ac", "row_an", "row_ns", "mrow_off",
                                           "mrow_member", "mrow_gt", "mrow_ac", "mrow_an", "mrow_ns")


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _kw(mode, opts):
    kw = {"plain": {}, "inversions": dict(flags=H.T_INVERSIONS), "nested": dict(flags=H.T_NESTED), "top-level-only": dict(profile="top-level-only"),
          "popped": dict(profile="popped"), "left-normalized": dict(profile="left-normalized"), "decomposed": dict(profile="decomposed"),
          "merged": dict(profile="decomposed", flags=H.T_MERGE), "untangle": dict(flags=H.T_UNTANGLE)}[mode]
    kw = dict(kw, **{k: v for k, v in opts.items() if k != "tier2"})
    if opts.get("tier2"):
        kw["flags"] = kw.get("flags", 0) | H.T_FORCE_TIER2
    return kw


def _text(c, k, which="seq"):
    off = c.seq_off if which == "seq" else c.at_off
    return bytes(getattr(c, which)[int(off[k]):int(off[k + 1])])


def _record(c, i):
    """Everything record i says that is no index into the call's own tables."""
    b = int(c.block[i])
    spelled = [(_text(c, k), _text(c, k, "at")) for k in range(int(c.block_off[b]), int(c.block_off[b + 1]))]
    nb = int(c.norm_block[i])
    norm = None if nb == 0xFFFFFFFF else [_text(c, k) for k in range(int(c.block_off[nb]), int(c.block_off[nb + 1]))]
    return ([int(getattr(c, a)[i]) for a in RECORD_ARRAYS], c.gt[i].tolist(), c.ac[int(c.ac_off[i]):int(c.ac_off[i + 1])].tolist(), spelled,
            _text(c, int(c.ref_spelled[i])), norm, [np.asarray(getattr(c, a)[i]).tolist() for a in UNT_ARRAYS] if c.untangled else None)


def _key(c, i):
    return int(c.path[i]), int(c.raw_pos[i]), int(c.query[i]), int(c.first[i]), int(c.n_steps[i])


def _digest(c):
    return [np.ascontiguousarray(getattr(c, a)).tobytes() for a in ALL_ARRAYS] + [c.vcf_text(date=DATE), c.n_records, c.n_inv_records]


def _check(d, setup, refs, mode, regions, opts=None, vacuous_ok=False):
    """The region call equals the restatement and, record for record, the full call; returns (calls, kept records, full records)."""
    f, sites, names, steps, sq = setup
    opts = opts or {}
    kw = _kw(mode, opts)
    popt = {k: v for k, v in opts.items() if k != "tier2"}
    want, text, full = R.call(mode, sites, names, steps, sq, list(refs), regions, date=DATE, **popt)
    if not vacuous_ok:
        assert 0 < len(want) < len(full)
    c = d.call(f, list(refs), regions=regions, **kw)
    assert c.vcf_text(date=DATE) == text
    assert c.n_records == len(want)
    assert [(int(c.path[i]), int(c.pos[i]), int(c.query[i]), int(c.first[i])) for i in range(c.n_records)] == \
        [(r["path"], r["pos"], r["q"], r["first"]) for r in want]
    # ... and every field is the full call's
    whole = d.call(f, list(refs), **kw)
    assert [getattr(whole, k) for k in H.REGION_COUNTERS] == [0, 0, 0, 0]
    at = {_key(whole, i): i for i in range(whole.n_records)}
    assert len(at) == whole.n_records
    rows = [at[_key(c, i)] for i in range(c.n_records)]
    assert rows == sorted(rows) or mode == "left-normalized"  # (the same order; a normalisation may make two records swap places)
    for i, j in enumerate(rows):
        assert _record(c, i) == _record(whole, j), (i, j)
    assert c.contig_len.tolist() == whole.contig_len.tolist()
    # the counters
    passing = R.passing_sites(sites, names, steps, sq, regions)
    n_fl_full, n_fl = sum(r["q"] != R.NIL for r in full), sum(r["q"] != R.NIL for r in want)
    masked = mode not in NESTED_MODES
    assert c.n_regions >= 1 and c.n_region_sites == sum(passing)
    assert c.n_region_masked == (len(sites) - sum(passing) if masked else 0)
    assert c.n_region_dropped == (0 if masked else n_fl_full - n_fl)
    if mode == "inversions":
        assert c.n_inv_records == sum(r["q"] == R.NIL for r in want)
    # ... and once more with every site scanned
    late = d.call(f, list(refs), regions=regions, region_no_mask=True, **kw)
    assert _digest(late) == _digest(c)
    assert late.n_region_masked == 0 and late.n_region_dropped == n_fl_full - n_fl and late.n_region_sites == c.n_region_sites
    if not vacuous_ok:
        assert late.n_region_dropped > 0
    return c, want, full


def _workload_setup(d, name):
    g, seqs, p, refs = RC.workload(name)
    return _setup(d, g, list(seqs), p), refs


@pytest.mark.parametrize("row", sorted(RC.FIXTURE_ROWS))
def test_the_fixture_rows(hip, golden_dir, row):
    setup = _fixture_setup(hip, golden_dir, RC.FIXTURE)
    regions, sites_left = RC.FIXTURE_ROWS[row]
    c, want, full = _check(hip, setup, ["HG1"], "plain", regions, vacuous_ok=True)
    lines = [ln for ln in c.vcf_text(date=DATE).splitlines() if not ln.startswith("#")]
    assert sorted(ln.split("\t")[2] for ln in lines) == sites_left and lines == json.load(open(RC.GOLDEN))["plain"][row]
    assert c.n_regions == len(regions)
    strings = [f"{n}:{s}-{e}" for n, s, e in regions]  # the same regions as text
    assert hip.call(setup[0], ["HG1"], regions=strings).vcf_text(date=DATE) == c.vcf_text(date=DATE)


def test_the_fixture_nested_and_popped(hip, golden_dir):
    setup = _fixture_setup(hip, golden_dir, RC.FIXTURE)
    c, want, _ = _check(hip, setup, ["HG1"], "nested", [(RC.HG1, 3, 4)], vacuous_ok=True)
    (line,) = [ln for ln in c.vcf_text(date=DATE).splitlines() if not ln.startswith("#")]
    assert line.split("\t")[7].endswith(";ES=>2>4;LV=1;PS=>0>5") and [line] == json.load(open(RC.GOLDEN))["nested"]["second-boundary-of-the-child"]
    popt = json.load(open(os.path.join(golden_dir, "reference_nested_records.json")))["popped_options"]
    c, want, _ = _check(hip, setup, ["HG1"], "popped", [(RC.HG1, 3, 4)], popt, vacuous_ok=True)  # the popped parent is outside
    assert [r["id"] for r in want] == [">2>4:rescued"] and c.n_rescued == 1 and c.n_popped == 1 and int(c.flags[0]) & H.CALL_RESCUED
    c, want, _ = _check(hip, setup, ["HG1"], "popped", [(RC.HG1, 1, 2)], popt, vacuous_ok=True)  # ... inside: popped all the same
    assert c.n_records == 0 and want == []


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_the_cases(hip, case):
    workload, mode, regions, opts = RC.CASES[case]
    setup, refs = _workload_setup(hip, workload)
    c, want, full = _check(hip, setup, refs, mode, regions, opts)
    if case == "chain-70-regions":
        assert c.n_regions == 70
    if case == "chain-overlapping":
        assert c.n_regions == 1
    if case == "chain-two-paths":
        assert c.n_regions == 2


def test_the_whole_path_is_the_full_call(hip):
    setup, refs = _workload_setup(hip, "chain")
    whole = hip.call(setup[0], list(refs))
    c = hip.call(setup[0], list(refs), regions=[(setup[2][0], 1, 2 ** 62)])
    assert _digest(c) == _digest(whole) and c.n_region_masked == 0 and c.n_region_sites == len(setup[1])


def test_a_region_without_records(hip):
    setup, refs = _workload_setup(hip, "chain")
    whole = hip.call(setup[0], list(refs))
    head = [ln for ln in whole.vcf_text(date=DATE).splitlines() if ln.startswith("#")]
    for no_mask in (False, True):  # beyond the path's end: fine, and nothing passes
        c = hip.call(setup[0], list(refs), regions=[(setup[2][0], 10 ** 6, 10 ** 6 + 5)], region_no_mask=no_mask)
        assert c.n_records == 0 and c.n_region_sites == 0 and c.n_regions == 1
        assert c.n_region_masked == (0 if no_mask else len(setup[1])) and (c.n_region_dropped > 0) == no_mask
        assert all(getattr(c, a).size == 0 for a in RECORD_ARRAYS + ("gt", "ac", "seq", "at", "block"))
        assert c.ac_off.size == c.block_off.size == c.seq_off.size == c.at_off.size == 1
        assert c.vcf_text(date=DATE).splitlines() == head and any(ln.startswith("##contig") for ln in head)


def test_the_same_call_twice_after_release_and_without_regions_behind_it():
    hip = HipDecomposer(0)
    try:
        setup, refs = _workload_setup(hip, "chain")
        f, regions = setup[0], RC.CASES["chain-middle"][2]
        plain = _digest(hip.call(f, list(refs)))
        first = _digest(hip.call(f, list(refs), regions=regions))
        assert first != plain
        assert _digest(hip.call(f, list(refs), regions=regions)) == first
        assert _digest(hip.call(f, list(refs))) == plain  # (a mask left in the arena would show here)
        other = _digest(hip.call(f, list(refs), regions=RC.CASES["chain-two-paths"][2]))
        assert other != first and _digest(hip.call(f, list(refs), regions=regions)) == first
        hip.release_workspace()
        assert _digest(hip.call(f, list(refs), regions=regions)) == first
        assert _digest(hip.call(f, list(refs))) == plain
    finally:
        hip.close()


def test_refusals(hip, golden_dir):
    f = _fixture_setup(hip, golden_dir, RC.FIXTURE)[0]
    with pytest.raises(RuntimeError, match="regions .*POVU_HIP_T_OFFREF"):
        hip.call(f, ["HG1"], flags=H.T_OFFREF, regions=[(RC.HG1, 1, 2)])
    for bad, word in (((RC.HG1, 5, 5), "start < end"), ((RC.HG1, 9, 3), "start < end"), ((RC.HG1, 1, 2 ** 63), "2\\^63")):
        with pytest.raises(RuntimeError, match=word):
            hip.call(f, ["HG1"], regions=[bad])
    for bad in ("HG1:1-2", ("HG9#1#chr1", 1, 2)):
        with pytest.raises(RuntimeError, match="no path is named HG"):
            hip.call(f, ["HG1"], regions=[bad])
    with pytest.raises(RuntimeError, match="more than 65536"):
        hip.call(f, ["HG1"], regions=[(RC.HG1, 1, 2)] * 65537)
    names = hip._path_names
    try:  # a name the library's table has and the device does not: its index is no resident path
        hip._path_names = list(names) + ["ghost#1#chr1"]
        with pytest.raises(RuntimeError, match="path 3 is no resident path"):
            hip.call(f, ["HG1"], regions=[("ghost#1#chr1", 1, 2)])
    finally:
        hip._path_names = names
    assert hip.call(f, ["HG1"], regions=[(RC.HG1, 1, 2)] * 65536).n_regions == 1  # (the most regions; they merge into one)
    assert hip.call(f, ["HG1"], regions=[]).n_regions == 0


def _body(text):
    return [ln for ln in text.splitlines() if not ln.startswith("##fileDate")]


def test_the_command_line_and_the_vcf_checks(hip, golden_dir, tmp_path):
    f = _fixture_setup(hip, golden_dir, RC.FIXTURE)[0]
    forest = tmp_path / "forest"
    forest.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", RC.GFA, "-o", str(forest)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, POVU_CALL_EXE=POVU)
    for flags, regions, kw in ((["--region", f"{RC.HG1}:3-4"], [(RC.HG1, 3, 4)], {}),
                               ([f"--region={RC.HG1}:1-2", "--region", f"{RC.HG1}:3-4"], [(RC.HG1, 1, 2), (RC.HG1, 3, 4)], {}),
                               (["--region", f"{RC.HG2}:2-3", "--nested"], [(RC.HG2, 2, 3)], dict(flags=H.T_NESTED)),
                               (["--region", f"{RC.HG1}:7-9"], [(RC.HG1, 7, 9)], {})):
        want = hip.call(f, ["HG1"], regions=regions, **kw).vcf_text()
        for cmd in ([POVU, "call", "-i", RC.GFA, "-f", str(forest), "-P", "HG1", "--stdout"] + flags,
                    [POVU, "gfa2vcf", "-i", RC.GFA, "-P", "HG1", "--stdout"] + flags):
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
            assert r.returncode == 0, r.stderr
            assert _body(r.stdout) == _body(want), cmd
    r = subprocess.run([POVU, "call", "-i", RC.GFA, "-f", str(forest), "-P", "HG1", "--region", "HG1:3-4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "no path is named HG1" in r.stderr  # exact names: a prefix is no path
    # povu vcf --report --spelling accepts the text of a plain region call
    vcf = tmp_path / "region.vcf"
    vcf.write_text(hip.call(f, ["HG1"], regions=[(RC.HG1, 5, 7)]).vcf_text())
    out = tmp_path / "report"
    r = subprocess.run([POVU, "vcf", "-i", RC.GFA, "-c", str(vcf), "--report", "-o", str(out), "--spelling"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (out / "summary.txt").read_text() == "No errors\n"
    setup, refs = _workload_setup(hip, "chain")
    c = hip.call(setup[0], list(refs), regions=RC.CASES["chain-middle"][2])
    rep = hip.check_vcf(c.vcf_text(date=DATE), spelling=True)
    assert rep.n_records == c.n_records > 0 and rep.n_invalid == 0 and rep.n_misspelled == 0 and rep.summary_text() == "No errors\n"
