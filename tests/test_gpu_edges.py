"""The query and call family on empty, minimal and wide-id inputs (tests/edge_cases.py, whose conditions
tests/test_edge_inputs.py checks without a GPU), through the comparisons of the family's own test files, exactly: every case
through traversals, walks and the call under every option set, each again with the forced second tier; every degenerate call in
a fresh context, behind a normal call and in front of one; the VCF checks on what the calls write and on VCFs without a record,
a genotype or a sample column; every wide-id case next to the same graph under small ids; the refusals at the id edge; the CLI."""
import os
import subprocess

import numpy as np
import pytest

import edge_cases as E
import inversions_ref as I
import merge_ref as MR
import prim_ref as PR
import test_gpu_inversions as TI
import test_gpu_merge as TM
import test_gpu_nested as TN
import test_gpu_norm as TNM
import test_gpu_offref as TO
import test_gpu_prim as TP
import test_gpu_traversals as TT
import test_gpu_vcfcheck as TV
import test_gpu_walks as TW
import vcf_ref as V
import vcfcheck_ref as R
from povu_amd import HipDecomposer
from povu_amd import hip as H
from test_gpu_call import POVU

pytestmark = pytest.mark.gpu
DATE = "00000000"
TIERS = [0, H.T_FORCE_TIER2]
INV = H.T_INVERSIONS
# the option sets of a call: (flags, profile)
OPTIONS = dict(plain=(0, None), inversions=(INV, None), nested=(H.T_NESTED, None), top=(H.T_NESTED, "top-level-only"),
               popped=(H.T_NESTED, "popped"), norm=(0, "left-normalized"), norm_inv=(INV, "left-normalized"), prim=(0, "decomposed"),
               merge=(H.T_MERGE, "decomposed"), merge_inv=(INV | H.T_MERGE, "decomposed"), offref=(H.T_OFFREF, None),
               offref_inv=(H.T_OFFREF | INV, None))
COUNTERS = ("n_records", "n_inv_heads", "n_inv_records", "n_inv_long", "n_inv_tier2", "n_rows", "n_mrows", "n_normalized", "n_popped",
            "n_rescued") + H.OFFREF_COUNTERS
CASES = list(E.MINIMAL) + ["zero_step_paths_2"]


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def case_of(name):
    return E.zero_step_paths(True) if name == "zero_step_paths_2" else E.MINIMAL[name]()


def call_kw(opt, case, tier=0):
    """The keywords of HipDecomposer.call for an option set."""
    flags, profile = OPTIONS[opt]
    kw = dict(flags=flags | tier)
    if profile:
        kw["profile"] = profile
    if profile == "popped":
        kw.update(case.popped)
    if opt in ("plain", "inversions"):
        kw["max_steps"] = case.max_steps
    return kw


def checked_call(d, setup, case, refs, opt, tier):
    """The call under an option set through the comparison of that option's own test file; returns the calls."""
    f, sites, names, steps, sq = setup
    flags, profile = OPTIONS[opt]
    inv = flags & INV
    if opt in ("plain", "inversions"):
        found, stats = I.records(names, steps, sq, refs, case.max_steps) if inv else ([], dict(records=0, heads=0, long=0, tier2=0))
        want = I.merge(V.call(sites, names, steps, sq, refs, case.max_steps), found)
        c = d.call(f, refs, **call_kw(opt, case, tier))
        TI._same(c, want, names, steps, sq, refs, I.vcf_text if inv else V.vcf_text)
        assert (c.n_inv_records, c.n_inv_heads, c.n_inv_long) == (stats["records"], stats["heads"], stats["long"])
        assert c.n_inv_tier2 == (stats["heads"] if tier and inv else stats["tier2"])
        return c
    if flags & H.T_NESTED:
        popt = case.popped if profile == "popped" else {}
        return TN._check(d, case.g, case.paths, refs, tflags=tier, profile=profile, setup=(f, sites, steps, sq), **popt)[0]
    if profile == "left-normalized":
        return TNM._check(d, setup, refs, tflags=inv | tier)[0]
    if flags & H.T_MERGE:
        return TM._check(d, setup, refs, tflags=inv | tier)[0]
    if profile == "decomposed":
        return (TP._both_tiers(d, setup, refs) if tier else TP._check(d, setup, refs))[0]
    return TO._check(d, setup, refs, tflags=inv | tier)[0]


def counters_of(c):
    return {k: getattr(c, k) for k in COUNTERS if getattr(c, k)}


# ---- every case, every option set, both tiers

@pytest.mark.parametrize("tier", TIERS, ids=["tier1", "tier2"])
@pytest.mark.parametrize("name", CASES)
def test_traversals_and_walks(hip, name, tier):
    case = case_of(name)
    f, t, qs = TT._check(hip, case.g, case.paths, force2=bool(tier), max_steps=case.max_steps)
    assert t.n_hash_splits == 0 and (tier or t.n_tier2 == 0)  # (no scan of a minimal case is long)
    f, w, _ = TW._check(hip, case.g, force2=bool(tier))
    print(f"EDGE {name} tier2={int(bool(tier))} n_queries={t.n_queries} n_traversals={t.n_traversals} n_alleles={int(t.allele_off[-1])} "
          f"n_tier2={t.n_tier2} n_walks={w.n_walks}")


@pytest.mark.parametrize("tier", TIERS, ids=["tier1", "tier2"])
@pytest.mark.parametrize("name", CASES)
def test_call_under_every_option_set(hip, name, tier):
    case = case_of(name)
    setup = TNM._setup(hip, *case.triple())
    for refs in case.refs:
        for opt in OPTIONS:
            c = checked_call(hip, setup, case, refs, opt, tier)
            print(f"EDGE {name} refs={','.join(refs)} {opt} tier2={int(bool(tier))} {counters_of(c)}")


# ---- a degenerate call in a fresh context, behind a normal call, in front of one

def _resident(d, case):
    return TNM._setup(d, *case.triple())[0]


@pytest.mark.parametrize("name", CASES)
def test_workspace_before_and_behind_a_normal_call(name):
    """Per option set, in a context of its own: the degenerate call where no arena of that call exists yet, the normal call
    (chain_case of tests/test_gpu_inversions.py), the degenerate call right behind it -- a skipped memset or kernel would read
    the normal call's leftovers -- and the normal call again, which a counter or list left behind would change."""
    case = case_of(name)
    g, p = TI.chain_case()
    normal = E.Case(g, E.bases(g, 1), p, [["sample0#1"]])
    for opt in OPTIONS:
        d = HipDecomposer(0)
        try:
            got = []
            for which in (case, normal, case, normal):
                f = _resident(d, which)
                got.append(d.call(f, which.refs[0], **call_kw(opt, which)))
            for a, b in ((got[0], got[2]), (got[1], got[3])):
                TP._same_records(a, b)
                for k in TP.ROW_ARRAYS + TM.MROW_ARRAYS + TO.OFF_ARRAYS:
                    assert np.array_equal(getattr(a, k), getattr(b, k)), (opt, k)
                assert counters_of(a) == counters_of(b) and a.vcf_text(date=DATE) == b.vcf_text(date=DATE), opt
            assert got[1].n_records > 100  # (the normal call is one)
        finally:
            d.close()


# ---- the VCF checks

@pytest.mark.parametrize("name", CASES)
def test_vcf_round_trip(hip, name):
    """What the plain call and the call with inversions write checks clean with the spelling on: records where the case has any,
    the header alone where it has none."""
    case = case_of(name)
    for refs in case.refs:
        (_, _, plain), (_, _, inv) = TV.round_trip(hip, case.g, case.paths, case.seqs, refs)
        print(f"EDGE {name} refs={','.join(refs)} vcf records plain={len(plain['records'])} inversions={len(inv['records'])}")


def test_vcfs_without_a_record_a_genotype_or_a_sample_column(hip):
    case = E.zero_step_paths()
    f, sites, names, steps, sq = TNM._setup(hip, *case.triple())
    refs = case.refs[0]
    text = hip.call(f, refs).vcf_text(date=DATE)
    lines = text.splitlines()
    records = [ln.split("\t") for ln in lines if not ln.startswith("#")]
    head = [ln for ln in lines if ln.startswith("#")]
    assert len(records) == 3 and len(records[0]) == 9 + 6  # (a column per path: those without a step as well)
    header_only = "\n".join(head) + "\n"
    no_genotype = "\n".join(head + ["\t".join(f[:9] + ["."] * 6) for f in records]) + "\n"
    no_samples = "\n".join(head[:-1] + ["\t".join(head[-1].split("\t")[:8])] + ["\t".join(f[:8]) for f in records]) + "\n"
    for doc_text, n_records in ((header_only, 0), (no_genotype, 3), (no_samples, 3)):
        rep, want, doc = TV.check(hip, doc_text, names, steps, sq.keys(), sq, spelling=True)
        assert (rep.n_records, rep.n_tasks, rep.n_invalid, rep.summary_text()) == (n_records, 0, 0, "No errors\n")
    assert R.parse(no_samples)["samples"] == [] and len(R.parse(no_genotype)["samples"]) == 6
    # the columns of the paths without a step carry no call; a genotype put there names a slot that holds no walk
    rep, want, doc = TV.check(hip, text, names, steps, sq.keys(), sq, spelling=True)
    assert rep.n_invalid == 0 and all(f[9 + k] == "." for f in records for k in (0, 3, 5))
    moved = "\n".join(head + ["\t".join(f[:9] + ["0"] + f[10:]) for f in records]) + "\n"
    rep, want, doc = TV.check(hip, moved, names, steps, sq.keys(), sq, spelling=True)
    assert want["n_status"][R.ABSENT] == 3 and rep.n_invalid == 3


# ---- wide ids: the same graph under small ids and under ids of every width

INDEX_ARRAYS = tuple(k for k in TP.RECORD_ARRAYS if k not in ("at", "at_off")) + TP.ROW_ARRAYS + TM.MROW_ARRAYS + TO.OFF_ARRAYS


@pytest.mark.parametrize("name", E.WIDE)
def test_wide_ids_traversals_and_walks(hip, name):
    plain, wide, ids = E.wide_cases()[name]
    m = np.zeros(int(plain.g.vid.max()) + 1, np.uint32)
    m[plain.g.vid] = ids
    for tier in (False, True):
        _, a, _ = TT._check(hip, plain.g, plain.paths, force2=tier)
        sa = hip.decompose().sites()
        _, b, _ = TT._check(hip, wide.g, wide.paths, force2=tier)
        sb = hip.decompose().sites()
        for k in TT.KEYS:
            assert np.array_equal(getattr(b, k), m[a.step_id] if k == "step_id" else getattr(a, k)), k
        assert int(b.step_id.max()) >= 2 ** 31
        for k in ("or1", "or2", "parent", "height", "family", "tree"):
            assert np.array_equal(getattr(sa, k), getattr(sb, k)), k
        assert np.array_equal(sb.id1, m[sa.id1]) and np.array_equal(sb.id2, m[sa.id2])
        _, wa, _ = TW._check(hip, plain.g, force2=tier)
        _, wb, _ = TW._check(hip, wide.g, force2=tier)
        for k in ("walk_off", "step_off", "step_or", "status"):
            assert np.array_equal(getattr(wa, k), getattr(wb, k)), k
        assert np.array_equal(wb.step_id, m[wa.step_id])


@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("name", E.WIDE)
def test_wide_ids_call(hip, name, opt):
    """The call on the relabelled graph equals the restatement's on it, in both tiers; every index-valued array is the
    original's bit for bit, the spelled bases as well; the AT bytes are longer."""
    plain, wide, ids = E.wide_cases()[name]
    refs = plain.refs[0]
    a = hip.call(_resident(hip, plain), refs, **call_kw(opt, plain))
    setup = TNM._setup(hip, *wide.triple())
    for tier in TIERS:
        b = checked_call(hip, setup, wide, refs, opt, tier)
        for k in INDEX_ARRAYS:
            assert np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), k
        forced = {"n_inv_tier2"} if tier else set()  # (every head through the second tier)
        assert {k: v for k, v in counters_of(a).items() if k not in forced} == {k: v for k, v in counters_of(b).items() if k not in forced}
        assert b.n_at_bytes > a.n_at_bytes and b.n_seq_bytes == a.n_seq_bytes
    print(f"EDGE wide {name} {opt} {counters_of(a)}")


@pytest.mark.parametrize("name", E.WIDE)
def test_wide_ids_vcf_round_trip(hip, name):
    """The device tokenizer reads the 10-digit steps back."""
    plain, wide, ids = E.wide_cases()[name]
    (_, _, doc), (_, _, inv) = TV.round_trip(hip, wide.g, wide.paths, wide.seqs, wide.refs[0])
    read = {i for d in (doc, inv) for rec in d["records"] for al in rec["alleles"] for i, _ in al["walk"]}
    assert {len(str(i)) for i in read} == set(range(1, 11)) and max(read) >= 2 ** 31


# ---- refusals at the id edge

def test_refusals_at_the_id_edge(hip):
    case = E.no_sites_wide()
    hip.upload(case.g)
    hip.decompose()
    with pytest.raises(RuntimeError, match="path 0 step 1: segment 3000000000 is not in the resident graph"):
        hip.upload_paths([[(7, 0), (3000000000, 0)]])
    with pytest.raises(RuntimeError, match="path 1 step 0: segment 4294967293 is not in the resident graph"):
        hip.upload_paths([[(7, 0)], [(4294967293, 1), (E.WIDE_TOP, 1)]])
    with pytest.raises(RuntimeError, match="path 0 step 0: segment 2147483647 is not in the resident graph"):
        hip.upload_paths([[(2 ** 31 - 1, 0), (2 ** 31, 0)]])
    # an AT step that names a legal id the graph lacks is a bad step, at 2^31 and at the largest id; 2^32 - 1 is no id at
    # all, for the restatement and the library alike
    lacking = E.relabel(case.g, case.paths, [7, 1000000, 99999999, 2147483648, E.WIDE_TOP - 1])
    small = E.Case(lacking[0], case.seqs, lacking[1], case.refs)
    TV.resident(hip, small.g, small.names, small.steps, small.seqs)
    recs = [("top", [[(E.WIDE_TOP, 0)]], ["0", ".", "."]), ("mid", [[(2 ** 31 + 1, 1)], [(2 ** 31, 0)]], ["0", "1", "."]),
            ("there", [[(E.WIDE_TOP - 1, 0)], [(E.WIDE_TOP - 1, 1)]], ["0", ".", "1"])]
    text = TV.vcf_of([n.split("#")[0] for n in small.names], recs, {**small.sq, E.WIDE_TOP: "A", 2 ** 31 + 1: "C"})
    rep, want, _ = TV.check(hip, text, small.names, small.steps, small.sq.keys())
    assert want["task_status"] == [R.BAD_STEP, R.BAD_STEP, R.FOUND_FWD, R.FOUND_FWD, R.FOUND_FWD]
    beyond = text.replace(f"AT=>{E.WIDE_TOP}", "AT=>4294967295")
    assert beyond != text
    with pytest.raises(R.VcfError, match="line 3: AT walk 0 is no walk of \\[<>\\]id steps: >4294967295") as refused:
        R.parse(beyond)
    with pytest.raises(RuntimeError) as got:
        hip.check_vcf(beyond)
    assert str(got.value) == str(refused.value)


# ---- the CLI

def _run(*args):
    return subprocess.run([POVU] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


CLI_RECORDS = dict(no_sites=(0, 1, 0), all_agree=(0, 0, 0))  # record lines: plain, --inversions, decomposed and merged


@pytest.mark.parametrize("name", ["no_sites", "all_agree", "long"])
def test_cli(tmp_path, name):
    case = E.wide_cases()[name][1] if name in E.WIDE else E.MINIMAL[name]()
    assert all(case.seqs)  # (a GFA S line needs a sequence)
    refs = case.refs[0]
    gfa = tmp_path / "g.gfa"
    gfa.write_text(case.g.to_gfa(case.seqs) + case.paths.to_gfa())
    forest = tmp_path / "forest"
    forest.mkdir()
    r = _run("decompose", "-i", gfa, "-o", forest)
    assert r.returncode == 0, r.stderr
    names, steps, sq = case.names, case.steps, case.sq
    sites = V.sites_of_pvst([x.read_text() for x in sorted(forest.glob("*.pvst"), key=lambda x: int(x.stem))])
    raw = V.call(sites, names, steps, sq, refs)
    with_inv = I.merge([dict(x) for x in raw], I.records(names, steps, sq, refs)[0])
    rows, _ = PR.decompose([dict(x) for x in raw], names, steps, sq)
    merged, _ = MR.merge(raw, rows, names)
    texts = [([], V.vcf_text(names, steps, sq, raw, refs, date=DATE)),
             (["--inversions"], I.vcf_text(names, steps, sq, with_inv, refs, date=DATE)),
             (["--profile", "decomposed", "--merge-primitives"], MR.vcf_text(names, steps, sq, raw, rows, merged, refs, date=DATE))]
    prefixes = [x for p in refs for x in ("-P", p)]
    for k, (extra, want) in enumerate(texts):
        r = _run("call", "-i", gfa, "-f", forest, *prefixes, *extra)
        assert r.returncode == 0, r.stderr
        assert r.stdout.split("\n", 2)[2] == want.split("\n", 2)[2], extra  # (behind the date line)
        n = sum(not ln.startswith("#") for ln in r.stdout.splitlines())
        assert n == CLI_RECORDS[name][k] if name in CLI_RECORDS else n > 0, extra
        vcf = tmp_path / f"calls{k}.vcf"
        vcf.write_text(r.stdout)
        out = tmp_path / f"report{k}"
        r = _run("vcf", "-i", gfa, "-c", vcf, "--report", "-o", out)
        assert r.returncode == 0, r.stderr
        assert (out / "summary.txt").read_text() == "No errors\n"
