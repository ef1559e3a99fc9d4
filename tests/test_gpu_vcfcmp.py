"""GPU VCF comparison (povu_hip_vcf_compare, HipDecomposer.compare_vcfs) against the plain-Python restatement
(tests/vcfcmp_ref.py), array for array and text for text, every case again with the forced second tier (equal but for n_tier2):
the golden VCFs against themselves and raw against profile; this project's own `decomposed` and `left-normalized` calls against
the golden VCFs of those profiles; the trims on the edges of a ballot's 64 bytes and of the tiers; groups of 1 to 130 members
and keys that differ in one field; every run colliding (POVU_HIP_TRAV_HASH_BITS); the wide cohort's VCF against a copy with
its columns permuted, renamed, dropped and its genotypes edited; ploidies, an ALT with more than 64 tasks, no common sample,
no sample columns; empty inputs; a context without a graph; the arenas; the refusals."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cohort_cases as CC
import vcfcmp_cases as K
import vcfcmp_ref as M
from povu_amd import HipDecomposer
from povu_amd import hip as H

pytestmark = pytest.mark.gpu
ROOT = K.ROOT
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 128, 200)
SHARED_ENDS = (0, 1, 63, 64, 65)


@pytest.fixture(scope="module")
def hip():
    """A context that never sees a graph: the comparison needs none."""
    d = HipDecomposer(0)
    yield d
    d.close()


# ---- the golden VCFs

@pytest.mark.parametrize("fixture", sorted(K.GOLDEN_FILES))
def test_golden_vcfs_against_themselves_and_raw_against_profile(hip, fixture):
    names = K.GOLDEN_FILES[fixture]
    for name in names:
        text = K.golden(fixture, name)
        c, want = K.both_tiers(hip, text, text)
        assert c.n_only_a == c.n_only_b == 0 and c.n_shared == c.n_groups > 0
        assert c.sample_fp.sum() == c.sample_fn.sum() == 0 and c.sample_gteq.tolist() == c.sample_tp.tolist()
    for name in names[1:]:
        K.both_tiers(hip, K.golden(fixture, names[0]), K.golden(fixture, name))
    if fixture == "vcfwave-complex-decomposition":  # (worked by hand: tests/test_vcfcmp_ref.py)
        c, _ = K.both_tiers(hip, K.golden(fixture, "raw_graph"), K.golden(fixture, "decomposed"))
        assert (c.n_shared, c.n_only_a, c.n_only_b) == (1, 1, 2)
        assert (c.sample_tp.tolist(), c.sample_fp.tolist(), c.sample_fn.tolist(), c.sample_gteq.tolist()) == ([0, 0, 1], [0, 1, 0], [0, 2, 0], [0, 0, 1])


# This project's own calls against the golden VCFs of their profiles: (fixture, golden file, the options of the call, what
# the comparison finds: shared, only A, only B, tp, fp, fn, gteq -- A is the call made here).
OWN_CALLS = [
    # nothing shared: the fixture's POS values are its own, nine more than a position on the path HG1#1#chr1 (its raw record stands
    # at 10 on the path's first base; its SNVs at 11 and 13, this project's at 2 and 4), and it passes the insertion through as
    # one row (T -> TACTACGTACGTA at 13 once trimmed) where the aligner here writes two (A -> ACGTACGTA at 1, T -> TA at 4).
    # HG2 carries the SNVs and HG3 the insertion on either side: every row a cell of its own.
    ("vcfwave-complex-decomposition", "decomposed", ["--profile=decomposed"], (0, 4, 3, 0, 4, 3, 0)),
    # the one SUBR row, passed through whole by both (ACGTA -> TACGT at 2 on `ref`): shared, one sample carries it on both sides
    ("subr-inversion-preservation", "decomposed_passthrough", ["--profile=decomposed", "--inversions"], (1, 0, 0, 1, 0, 0, 1)),
    # both alleles of the repeat, left-normalised to POS 1 by both (AA -> A and A -> AA): shared, a carrier each, equal doses.  (The
    # golden file writes them as two records, the call here as one with two ALTs: the key is per ALT.)
    ("tandem-repeat-left-normalization", "left_normalized", ["--profile=left-normalized"], (2, 0, 0, 2, 0, 0, 2)),
]


@pytest.mark.parametrize("fixture, name, options, found", OWN_CALLS)
def test_own_profile_calls_against_the_golden_vcfs(hip, fixture, name, options, found):
    gfa = os.path.join(ROOT, "tests", "golden", "gfa", "downstream_repetitive", fixture + ".gfa")
    prefix = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_decomposed_records.json")))["fixtures"].get(
        "downstream_repetitive/" + fixture, {}).get("reference_prefix", "HG1")
    r = subprocess.run([POVU, "gfa2vcf", "-i", gfa, "-P", prefix, "--stdout"] + options, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, POVU_CALL_EXE=POVU))
    assert r.returncode == 0, r.stderr
    c, want = K.both_tiers(hip, r.stdout, K.golden(fixture, name))
    got = (c.n_shared, c.n_only_a, c.n_only_b) + tuple(int(getattr(c, k).sum()) for k in ("sample_tp", "sample_fp", "sample_fn", "sample_gteq"))
    print("own call against golden:", fixture, name, got, "\n" + c.compare_text())
    assert got == found


# ---- the trims

def _trim_rows():
    """Rows whose (REF, ALT) have a shared end and a shared front of every length around a ballot's 64 bytes, cores of every
    length around the tiers' 32; trims that stop because a text reaches one byte; either case; skipped ALTs of each kind."""
    rng = np.random.default_rng(5)
    rows, pos = [], 1
    def add(ref, alt):
        nonlocal pos
        rows.append(("c", pos, f"r{len(rows)}", ref, alt, ["1"]))
        pos += 1000
    for n in LENGTHS:
        core = K.bases(rng, n)
        add(core, K.other(core[0]) + core[1:])                      # a SNV at the front: the whole rest is a shared end
        add(core, core[:-1] + K.other(core[-1]))                    # ... at the end: the whole front is shared
        add(core, core.lower())                                     # equal but for the case: both keep one byte
        add(core, core + core)                                      # the end trim stops at REF's one byte
        add(core + core, core)
        add("a" + core, "A" + core.lower() + "t")
    for front in SHARED_ENDS:
        for end in SHARED_ENDS:
            f, e = K.bases(rng, front), K.bases(rng, end)
            add(f + "A" + e, f.lower() + "CG" + e)                  # differing cores of 1 and 2 bytes
            add(f + "AC" + K.bases(rng, 40) + e, f + "GT" + K.bases(rng, 70) + e.lower())  # ... of more than 32
            add(f + "G" + e, f + e if front + end else "GT")        # a deletion inside a shared run
    long = K.bases(rng, 200)
    for alt in ("*", "<DEL>", "<INS:ME>", "G[c:5[", "]c:5]G", long + "[", "C" * 70 + "]" + "C" * 70, "**", "C"):
        add("G", alt)
        add(long, alt)
    add(".", "A")
    add("..", "A")
    add("A", "C,*,G,<X>,T")
    return rows


def test_trim_edges_on_both_tiers(hip):
    rows = _trim_rows()
    a = K.vcf(["s"], rows)
    # B: the same alleles written another way -- one more shared base in front, the other case.  (An allele that has no base
    # in front of its change on A, or none at all, keeps another anchor there: not every key is shared.)
    b = K.vcf(["s"], [(c, p - 1, i, "t" + r.swapcase(), ",".join(x if M.skipped("A", x) else "T" + x.swapcase() for x in alt.split(",")), g)
                      if r not in (".", "..") else (c, p, i, r, alt, g) for c, p, i, r, alt, g in rows])
    c, want = K.both_tiers(hip, a, b)
    assert c.n_skipped_a == c.n_skipped_b >= 17
    print("trim edges:", c.n_shared, c.n_only_a, c.n_only_b, want["n_tier2"])
    assert c.n_shared > c.n_only_a == c.n_only_b > 0
    assert 0 < want["n_tier2"] < c.n_items_a + c.n_items_b
    assert {0, 1, 63, 64, 65} <= set(c.item_suffix_a.tolist()) and {0, 1, 63, 64, 65} <= set(c.item_prefix_a.tolist())
    K.both_tiers(hip, a, a)


# ---- grouping

def test_the_same_key_many_times_and_near_keys(hip):
    rng = np.random.default_rng(9)
    core = K.bases(rng, 80)
    rows_a, rows_b = [], []
    for n, (ref, alt) in zip((1, 2, 64, 65, 130), (("A", "C"), ("AT", "A"), (core, "G"), ("G", core), ("C", "CT"))):
        rows_a += [("c", 100 * n, f"a{n}.{k}", ref, alt, ["1"]) for k in range(n)]          # n times on A
        rows_b += [("c", 100 * n, f"b{n}.{k}", ref, alt, ["1"]) for k in range(n)]          # ... and on both
        rows_a += [("d", 100 * n, f"d{n}.{k}", ref, alt, ["1"]) for k in range(n)]          # ... on A only
    # keys equal but for CHROM, for POS' only, for one byte only (a short and a long text)
    near = [("e", 5, "AC", "A"), ("E", 5, "AC", "A"), ("e", 6, "AC", "A"), ("e", 5, "AG", "A"), ("e", 5, core, "A"), ("e", 5, core[:-1] + K.other(core[-1]), "A"),
            ("e", 5, "A", core), ("e", 5, "A", core[:40] + K.other(core[40]) + core[41:])]
    rows_a += [(c, p, f"n{k}", r, a, ["1"]) for k, (c, p, r, a) in enumerate(near)]
    rows_b += [(c, p, f"m{k}", r, a, ["0"]) for k, (c, p, r, a) in enumerate(near[::2])]
    a, b = K.vcf(["s"], rows_a), K.vcf(["s"], rows_b)
    c, want = K.both_tiers(hip, a, b)
    sizes = sorted(zip(c.group_n_a.tolist(), c.group_n_b.tolist()))
    assert all((n, n) in sizes and (n, 0) in sizes for n in (1, 2, 64, 65, 130))
    assert (c.n_shared, c.n_only_a, c.n_only_b) == (5 + 4, 5 + 4, 0) and c.n_splits == 0
    K.both_tiers(hip, b, a)


COLLIDE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import json
import vcfcmp_cases as K
from povu_amd import HipDecomposer
a, b = open(sys.argv[2]).read(), open(sys.argv[3]).read()
d = HipDecomposer(0)
c, _ = K.both_tiers(d, a, b)
print(json.dumps(dict(digest=K.digest(c), n_splits=c.n_splits)))
d.close()
"""


@pytest.mark.parametrize("bits", [1, 4])
def test_every_run_collides_with_few_hash_bits(hip, tmp_path, bits):
    rng = np.random.default_rng(bits)
    rows_a = [("c", 10 + k % 7, f"a{k}", K.bases(rng, 1 + k % 3), K.bases(rng, 1 + k % 2), ["1"]) for k in range(150)]
    rows_a += [("c", 500, f"l{k}", K.bases(rng, 70), K.bases(rng, 70), ["1"]) for k in range(6)] + [("c", 9, "s", "A", "*", ["1"])] * 3
    rows_b = rows_a[::3] + [("c", 40 + k % 5, f"b{k}", K.bases(rng, 2), K.bases(rng, 1), ["1"]) for k in range(40)]
    a, b = K.vcf(["s"], rows_a), K.vcf(["s"], rows_b)
    (tmp_path / "a.vcf").write_text(a)
    (tmp_path / "b.vcf").write_text(b)
    c, _ = K.both_tiers(hip, a, b)
    r = subprocess.run([sys.executable, "-c", COLLIDE, os.path.join(ROOT, "tests"), str(tmp_path / "a.vcf"), str(tmp_path / "b.vcf")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, POVU_HIP_TRAV_HASH_BITS=str(bits), PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.splitlines()[-1])
    assert out["digest"] == json.loads(json.dumps(K.digest(c))) and out["n_splits"] > 0 and c.n_splits == 0


# ---- samples

@pytest.fixture(scope="module")
def cohort_vcf():
    """The wide cohort's VCF (131 sample columns), called here on a context of its own."""
    d = HipDecomposer(0)
    try:
        g, p = CC.wide_chain()
        d.upload(g)
        f = d.decompose()
        d.upload_paths(p)
        d.upload_sequences(CC.wide_sequences(g))
        return d.call(f, [CC.REF_LOW]).vcf_text(date=DATE)
    finally:
        d.close()


def _edited_cohort(text):
    """The columns permuted, three renamed, two dropped, every fifth genotype of every third record edited."""
    rng = np.random.default_rng(3)
    lines = text.rstrip("\n").split("\n")
    at = next(k for k, ln in enumerate(lines) if ln.startswith("#CHROM"))
    n = len(lines[at].split("\t")) - 9
    order = [int(x) for x in rng.permutation(n)][:-2]
    out = lines[:at]
    head = lines[at].split("\t")
    names = [head[9 + c] for c in order]
    for k in (0, 64, 100):
        names[k] = "renamed" + str(k)
    out.append("\t".join(head[:9] + names))
    for r, ln in enumerate(lines[at + 1:]):
        f = ln.split("\t")
        n_alts = len(f[4].split(","))
        gts = [f[9 + c] for c in order]
        if r % 3 == 0:
            for k in range(0, len(gts), 5):
                gts[k] = "|".join("." if x == "." else str((int(x) + 1) % (n_alts + 1)) for x in gts[k].split("|"))
        out.append("\t".join(f[:9] + gts))
    return "\n".join(out) + "\n"


def test_wide_cohort_against_an_edited_copy(hip, cohort_vcf):
    doc = M.parse(cohort_vcf)
    assert len(doc["samples"]) == CC.SAMPLES == 131 and len(doc["records"]) >= 10
    c, want = K.both_tiers(hip, cohort_vcf, _edited_cohort(cohort_vcf))
    assert (c.n_common_samples, c.n_samples_only_a, c.n_samples_only_b) == (126, 5, 3)
    assert c.n_only_a == c.n_only_b == 0 and c.n_shared == c.n_groups
    assert c.sample_fp.sum() > 0 and c.sample_fn.sum() > 0 and (c.sample_gteq < c.sample_tp).any()
    assert c.sample_col_a.max() > 128 and (c.sample_tp[64:] > 0).all()  # the third batch of 64 lanes counts too
    assert (np.sort(c.sample_col_b) == np.arange(129)[np.isin(np.arange(129), c.sample_col_b)]).all()
    same, _ = K.both_tiers(hip, cohort_vcf, cohort_vcf)
    assert same.sample_fp.sum() == same.sample_fn.sum() == 0 and same.sample_gteq.tolist() == same.sample_tp.tolist()


def test_ploidies_many_tasks_and_no_common_sample(hip):
    samples = [f"s{k}" for k in range(70)]
    # ploidies 1 to 3 within a record; ALT 1 of record 1 has 70 * 3 = 210 tasks on A, ALT 2 none
    gt = lambda k, r: ["1", "0/1", "1|1|0", "1/2", ".", "./1"][(k + r) % 6]
    rows_a = [("c", 10, "r0", "A", "C,G", [gt(k, 0) for k in range(70)]), ("c", 20, "r1", "A", "T,TT", ["1|1|1"] * 70),
              ("c", 30, "r2", "AC", "A", [gt(k, 2) for k in range(70)])]
    rows_b = [("c", 10, "q0", "A", "G,C", [gt(k, 3) for k in range(70)]), ("c", 20, "q1", "A", "T", ["1/1"] * 69 + ["1|1|1"]),
              ("c", 20, "q1b", "A", "T", ["0|1"] * 35 + ["0"] * 35), ("c", 30, "q2", "ACC", "AC", [gt(k, 1) for k in range(70)])]
    a, b = K.vcf(samples, rows_a), K.vcf(samples[::-1], rows_b)
    c, want = K.both_tiers(hip, a, b)
    assert c.n_common_samples == 70 and c.sample_col_b.tolist() == list(range(69, -1, -1))
    t_group = int(c.item_group_a[2])
    assert (int(c.group_n_a[t_group]), int(c.group_n_b[t_group])) == (1, 2)
    assert M.totals(want)[0] > M.totals(want)[3] > 0
    # no common sample; no sample columns at all on one side, on both
    for sa, sb in ((samples, ["x", "y"]), (samples, []), ([], [])):
        ra = [(ch, p, i, r, alt, g[:len(sa)]) for ch, p, i, r, alt, g in rows_a]
        rb = [(ch, p, i, r, alt, g[:len(sb)]) for ch, p, i, r, alt, g in rows_b]
        c, _ = K.both_tiers(hip, K.vcf(sa, ra), K.vcf(sb, rb))
        assert c.n_common_samples == 0 and c.sample_tp.size == 0 and (c.n_samples_only_a, c.n_samples_only_b) == (len(sa), len(sb))
        assert (c.n_shared, c.n_only_a, c.n_only_b) == (4, 1, 0) and "Genotypes: precision nan, recall nan, F1 nan\n" in c.summary_text()


# ---- empty inputs, contexts, arenas

def test_empty_inputs(hip):
    full = K.vcf(["s"], [("c", 1, "x", "A", "C", ["1"]), ("c", 2, "y", "AT", "A,ATT", ["1/2"])])
    none, dots = K.HEAD + "s\n", K.vcf(["s"], [("c", 1, "x", "A", ".", ["0"]), ("c", 2, "y", "G", ".", ["0"])])
    for a, b in ((none, full), (full, none), (none, none), (dots, full), (full, dots), (dots, dots), (dots, none)):
        c, want = K.both_tiers(hip, a, b)
        assert c.n_shared == 0 and c.n_groups == c.n_only_a + c.n_only_b == (3 if full in (a, b) else 0)
    c = hip.compare_vcfs(H.parse_vcf(full, threads=2), full)  # a VcfDoc for either side
    assert (c.n_shared, c.n_groups) == (3, 3)


def _vcs(d):
    return {a["name"]: a["bytes"] for a in d.arenas() if a["name"] in ("vc_ws", "vc_hit")}


def test_arenas_release_and_a_check_after_a_comparison(cohort_vcf):
    import vcfcheck_ref as R
    d = HipDecomposer(0)
    try:
        assert len(d.arenas()) == 54 and set(_vcs(d).values()) == {0}
        other = _edited_cohort(cohort_vcf)
        first = K.digest(d.compare_vcfs(cohort_vcf, other))  # a fresh context, no graph uploaded
        assert all(v > 0 for v in _vcs(d).values()) and len(d.arenas()) == 54
        d.release_workspace()
        assert set(_vcs(d).values()) == {0}
        assert K.digest(d.compare_vcfs(cohort_vcf, other)) == first
        # a check of the same context after a comparison, in the arenas the comparison used
        g, p = CC.wide_chain()
        d.upload(g)
        d.decompose()
        d.upload_paths(p)
        names, steps = list(p.names), CC.steps_of(p)
        rep = d.check_vcf(cohort_vcf)
        want = R.check(R.parse(cohort_vcf), names, steps, set(g.vid.tolist()))
        assert rep.task_status.tolist() == want["task_status"] and rep.rec_invalid.tolist() == want["rec_invalid"]
        assert K.digest(d.compare_vcfs(cohort_vcf, other)) == first
    finally:
        d.close()


def test_refusals(hip):
    lib = H.load_lib()
    err = C.create_string_buffer(512)
    doc = H.parse_vcf(K.vcf(["s"], [("c", 1, "x", "A", "C", ["1"])]))
    assert not lib.povu_hip_vcf_compare(hip._ctx, None, doc._p, None, err, 512) and "null" in err.value.decode()
    assert not lib.povu_hip_vcf_compare(hip._ctx, doc._p, None, None, err, 512) and "null" in err.value.decode()
    assert not lib.povu_hip_vcf_compare(None, doc._p, doc._p, None, err, 512) and "null" in err.value.decode()
    # 2^32 of anything on a side, or in the two together: refused by the counts, before an array is read
    for field, what in (("n_tasks", "tasks"), ("n_text_bytes", "text bytes"), ("n_alleles", "alleles"), ("n_records", "records")):
        for n, together in ((2 ** 32, False), (2 ** 31, True)):
            big = H._VcfDoc()
            setattr(big, field, n)
            sides = (C.byref(big), C.byref(big)) if together else (doc._p, C.byref(big))
            assert not lib.povu_hip_vcf_compare(hip._ctx, sides[0], sides[1], None, err, 512)
            msg = err.value.decode()
            assert what in msg and "2^32 or more are refused" in msg and (together or "of a document" in msg), msg
    # a document whose arrays do not belong together
    bad = H._VcfDoc()
    C.memmove(C.byref(bad), doc._p, C.sizeof(H._VcfDoc))
    bad.n_chroms = 0
    assert not lib.povu_hip_vcf_compare(hip._ctx, doc._p, C.byref(bad), None, err, 512) and "document B" in err.value.decode()
    assert hip.compare_vcfs(doc, doc).n_shared == 1  # the context is as good as before
