"""GPU VCF checks (povu_hip_vcf_check, HipDecomposer.check_vcf) against the plain-Python restatement (tests/vcfcheck_ref.py),
array for array and text for text, every case again with the forced second tier (equal but for n_tier2): the round trip of this
project's own calls (plain and with inversions, spelling on: no invalid record, no misspelled allele) on the eleven conformance
GFAs, PanSN haplotypes of a chain and a -s forest; references that run backwards (FOUND_REV, ABSENT under forward_only); walks
at the ends of paths; walks of 65, 128 and 200 steps; a repeat one path visits 70 times; the slot rules; mutations of a clean
VCF; two graphs in one context and the refusals.  Past 64: the wide cohort's VCF (tests/cohort_cases.py: 131 columns, 261
tasks a record) and first failures in its later batches of tasks; a record of 71 alleles; segments of 64 to 200 bases in the
spelling; walks and anchors on the edges of the tiers; documents beyond the capped grids of the counting kernels.  What those
inputs reach is checked without a GPU in tests/test_cohort_inputs.py."""
import os

import numpy as np
import pytest

import cohort_cases as CC
import vcf_ref as V
import vcfcheck_cases as K
import vcfcheck_ref as R
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W

pytestmark = pytest.mark.gpu
DATE = "00000000"
TIER1 = 64  # steps of a walk / occurrences of its anchor a lane per search still takes (DESIGN.md "VCF checks")
CONFORMANCE = [("complex_substitution_span", "HG1"), ("deletion_flubble", "HG1"), ("insertion_flubble", "HG1"), ("linear_no_variant", "HG1"),
               ("minimal_substitution", "HG1"), ("nested_deletion", "HG1"), ("nested_substitution_missing_outer", "HG1"),
               ("repeat_anchor_deletion", "HG1"), ("repeat_anchor_insertion", "HG1"), ("two_ordered_substitutions", "HG1"),
               ("hairpin_inversion_subr", "ref")]


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


# ---- the graphs and the VCFs (module level: what they are meant to reach can be checked with the restatement alone)

def links_of_gfa(path):
    ids, links = [], []
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if f[0] == "S":
            ids.append(int(f[1]))
        elif f[0] == "L":
            links.append((int(f[1]), f[2], int(f[3]), f[4]))
    ids = sorted(ids)
    at = {v: i for i, v in enumerate(ids)}
    return W._mk(np.array(ids), np.array([at[a] for a, _, _, _ in links]), np.array([W.R if o == "+" else W.L for _, o, _, _ in links]),
                 np.array([at[b] for _, _, b, _ in links]), np.array([W.L if o == "+" else W.R for _, _, _, o in links]))


def paths_of(names, steps):
    off = np.concatenate([[0], np.cumsum([len(p) for p in steps])]).astype(np.uint64)
    flat = [s for p in steps for s in p]
    return W.Paths(list(names), off, np.array([a for a, _ in flat], dtype=np.uint32), np.array([b for _, b in flat], dtype=np.uint8))


def chain(n):
    """Segments 1 .. n in a row."""
    return W.from_plus_links(np.arange(1, n + 1), np.arange(n - 1), np.arange(1, n))


def fwd(ids):
    return [(int(i), 0) for i in ids]


def at_of(w):
    return "".join((">" if o == 0 else "<") + str(i) for i, o in w)


def spell(w, sq):
    return "".join(R._oriented(s, sq) for s in w)


def vcf_of(samples, records, sq):
    """records: (id, walks, one GT string per sample); every allele spelled whole."""
    out = ["##fileformat=VCFv4.2\n", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples) + "\n"]
    for k, (ident, walks, gts) in enumerate(records):
        texts = [spell(w, sq) or "." for w in walks]
        out.append("\t".join(["c", str(k + 1), ident, texts[0], ",".join(texts[1:]) or ".", "60", "PASS",
                              "NS=1;AT=" + ",".join(at_of(w) for w in walks), "GT"] + gts) + "\n")
    return "".join(out)


# ---- the comparison

def n_searches(doc, steps, segments, forward_only, force):
    """(allele, direction) searches the second tier runs: all of them with force, else those of a walk of more than TIER1 steps
    or an anchor with more than TIER1 occurrences; none at all when the paths have no step."""
    if not any(steps):
        return 0
    count = {}
    for p in steps:
        for x in p:
            count[tuple(x)] = count.get(tuple(x), 0) + 1
    n = 0
    for rec in doc["records"]:
        for al in rec["alleles"]:
            w = al["walk"]
            if not w or any(s[0] not in segments for s in w):
                continue
            for pattern in ([w] if forward_only else [w, R.flipped(w)]):
                n += force or len(w) > TIER1 or count.get(tuple(pattern[0]), 0) > TIER1
    return n


def check(d, text, names, steps, segments, sq=None, forward_only=False, spelling=False, restated=None):
    """Both tiers equal the restatement; returns (the report of the first, the restatement's result, its document).  `restated`:
    (document, result) of the restatement when the caller has them already."""
    segments = set(segments)
    doc = restated[0] if restated else R.parse(text)
    want = restated[1] if restated else R.check(doc, names, steps, segments, sq, forward_only=forward_only, spelling=spelling)
    first = None
    for force in (False, True):
        rep = d.check_vcf(text, forward_only=forward_only, spelling=spelling, force_tier2=force)
        assert K.lib_arrays(rep.doc) == R.doc_arrays(doc)
        for k in ("task_status", "allele_spell", "rec_invalid", "rec_reason", "rec_allele", "rec_task"):
            assert getattr(rep, k).tolist() == want[k], (k, force)
        assert (rep.n_records, rep.n_tasks) == (len(doc["records"]), len(want["task_status"]))
        assert (rep.n_status, rep.n_invalid, rep.n_misspelled) == (want["n_status"], want["n_invalid"], want["n_misspelled"])
        assert rep.report_text() == R.report_text(doc, want, names) and rep.summary_text() == R.summary_text(doc, want)
        assert rep.n_tier2 == n_searches(doc, steps, segments, forward_only, force), force
        assert rep.device_ms > 0
        first = first or rep
    return first, want, doc


def resident(d, g, names, steps, seqs=None):
    d.upload(g)
    d.upload_paths(paths_of(names, steps))
    if seqs is not None:
        d.upload_sequences(seqs)


def round_trip(d, g, paths, seqs, prefixes, flags=0):
    """The VCF of the plain call and of the call with inversions, checked with spelling: nothing invalid, nothing misspelled."""
    d.upload(g)
    f = d.decompose(flags=flags)
    d.upload_paths(paths)
    d.upload_sequences(seqs)
    names, steps = list(paths.names), [paths.steps(k) for k in range(len(paths))]
    sq = dict(zip(g.vid.tolist(), seqs))
    out = []
    for tflags in (0, H.T_INVERSIONS):
        text = d.call(f, prefixes, flags=tflags).vcf_text(date=DATE)
        rep, want, doc = check(d, text, names, steps, sq.keys(), sq, spelling=True)
        assert rep.n_invalid == 0 and rep.n_misspelled == 0 and rep.summary_text() == "No errors\n", rep.report_text()
        assert set(want["task_status"]) <= {R.FOUND_FWD, R.FOUND_REV}
        out.append((text, want, doc))
    return out


# ---- round trip

@pytest.mark.parametrize("name, prefix", CONFORMANCE)
def test_round_trip_conformance_gfas(hip, golden_dir, name, prefix):
    gfa = os.path.join(golden_dir, "gfa", name + ".gfa")
    names, steps, seqs = V.read_gfa(gfa)
    g = links_of_gfa(gfa)
    (_, plain, _), (_, inv, doc) = round_trip(hip, g, paths_of(names, steps), [seqs[i] for i in g.vid.tolist()], [prefix])
    if name == "hairpin_inversion_subr":
        assert len(doc["records"]) == 1 and len(inv["task_status"]) >= 2
    elif name != "linear_no_variant":
        assert len(plain["task_status"]) >= 2


def test_round_trip_chain_haplotypes_forward_and_reversed_reference(hip):
    g = W.chain_of_bubbles(120)
    p = W.pansn(W.chain_haplotypes(120, 16, seed=5), samples=8)
    seqs = W.random_sequences(g, 1, max_len=40)
    (_, want, doc), _ = round_trip(hip, g, p, seqs, ["sample0#1"])
    assert len(doc["records"]) > 40 and want["n_status"][R.FOUND_FWD] > 400
    # a reference that is written '<' (every fourth haplotype): the calls spell the sites in its direction, the haplotypes
    # that walk them the other way carry their alleles reversed
    (text, want, doc), _ = round_trip(hip, g, p, seqs, ["sample1#2"])
    assert want["n_status"][R.FOUND_REV] > 100 and want["n_status"][R.FOUND_FWD] > 100
    names, steps = list(p.names), [p.steps(k) for k in range(len(p))]
    sq = dict(zip(g.vid.tolist(), seqs))
    rep, only, _ = check(hip, text, names, steps, sq.keys(), sq, forward_only=True)
    assert [s for s, t in zip(only["task_status"], want["task_status"]) if t == R.FOUND_REV] == [R.ABSENT] * want["n_status"][R.FOUND_REV]
    assert [s for s, t in zip(only["task_status"], want["task_status"]) if t != R.FOUND_REV] == [R.FOUND_FWD] * want["n_status"][R.FOUND_FWD]
    assert rep.n_invalid > 0 and rep.summary_text().startswith("Error rate: ")


def test_round_trip_subflubble_forest(hip):
    g = W.bubble_zoo(6, 8, 2)
    p = W.pansn(W.random_walk_paths(g, 10, 300, seed=7), samples=5)
    (_, want, doc), _ = round_trip(hip, g, p, W.random_sequences(g, 7, max_len=60), ["sample0#1"], flags=H.F_SUBFLUBBLES)
    assert len(doc["records"]) >= 1


def test_backwards_reference_fixture(hip, golden_dir):
    gfa = os.path.join(golden_dir, "gfa", "offref", "backwards.gfa")
    names, steps, seqs = V.read_gfa(gfa)
    g = links_of_gfa(gfa)
    # HG2 walks the graph backwards: as the reference its sites are spelled backwards, HG3 carries them reversed
    (text, want, doc), _ = round_trip(hip, g, paths_of(names, steps), [seqs[i] for i in g.vid.tolist()], ["HG2"])
    assert want["n_status"][R.FOUND_REV] > 0 and want["n_status"][R.FOUND_FWD] > 0
    _, only, _ = check(hip, text, names, steps, seqs.keys(), seqs, forward_only=True)
    assert [(a, b) for a, b in zip(want["task_status"], only["task_status"]) if a != b] == [(R.FOUND_REV, R.ABSENT)] * want["n_status"][R.FOUND_REV]


# ---- the ends of a path

def path_end_case():
    """s#1#a ends with 2 and s#1#b begins with 3 4: `>2>3>4` starts on the last step of a path and the next path in upload order
    begins with exactly its other steps -- and so for its reverse reading; what fits exactly at either end of a path is found."""
    names = ["s#1#a", "s#1#b", "t#1#a"]
    steps = [fwd([1, 2]), fwd([3, 4]), fwd([5, 6])]
    recs = [("over", [fwd([2, 3, 4]), R.flipped(fwd([2, 3, 4]))], ["0|1", "."]),
            ("over1", [fwd([2, 3]), R.flipped(fwd([2, 3]))], ["0|1", "."]),
            ("fits", [fwd([1, 2]), fwd([3, 4]), R.flipped(fwd([3, 4])), R.flipped(fwd([1, 2]))], ["0|1|2|3", "."]),
            ("last", [fwd([5, 6]), R.flipped(fwd([5, 6])), fwd([6, 1])], [".", "0|1|2"]),
            ("ends", [fwd([2]), fwd([3]), [(1, 1)], [(4, 1)], fwd([6])], ["0|1|2|3", "4"])]
    return names, steps, recs


def test_walks_at_the_ends_of_paths(hip):
    names, steps, recs = path_end_case()
    sq = {i: "ACGT"[i % 4] for i in range(1, 7)}
    resident(hip, chain(6), names, steps, [sq[i] for i in range(1, 7)])
    text = vcf_of(["s", "t"], recs, sq)
    rep, want, _ = check(hip, text, names, steps, sq.keys(), sq, spelling=True)
    A, F, B = R.ABSENT, R.FOUND_FWD, R.FOUND_REV
    # (phases 1 and more are beyond the one slot of s and of t: those tasks have no slot)
    assert want["task_status"] == [A, R.NO_SLOT, A, R.NO_SLOT, F, R.NO_SLOT, R.NO_SLOT, R.NO_SLOT, F, R.NO_SLOT, R.NO_SLOT,
                                   F, R.NO_SLOT, R.NO_SLOT, R.NO_SLOT, F]


def test_walks_at_the_ends_of_paths_every_allele_on_its_own_record(hip):
    """The same walks, one record and one sample column each: every status is the walk's own."""
    names, steps, recs = path_end_case()
    sq = {i: "A" for i in range(1, 7)}
    resident(hip, chain(6), names, steps)
    flat = [(f"{ident}{k}", [w], ["0", "."] if ident != "last" and not (ident == "ends" and k == 4) else [".", "0"])
            for ident, walks, _ in recs for k, w in enumerate(walks)]
    rep, want, _ = check(hip, vcf_of(["s", "t"], flat, sq), names, steps, sq.keys())
    A, F, B = R.ABSENT, R.FOUND_FWD, R.FOUND_REV
    assert want["task_status"] == [A, A, A, A, F, F, B, B, F, B, A, F, F, B, B, F]
    assert rep.n_invalid == 5
    _, only, _ = check(hip, vcf_of(["s", "t"], flat, sq), names, steps, sq.keys(), forward_only=True)
    assert only["task_status"] == [A if s == B else s for s in want["task_status"]]


# ---- long walks, many candidates

def long_case():
    """A row of 204 segments; `ref` walks it, `back` walks it backwards; q#1#a ends with 7 and q#1#b goes on with 8 .. 76."""
    names = ["ref#1#c", "back#1#c", "q#1#a", "q#1#b"]
    row = fwd(range(1, 205))
    steps = [row, R.flipped(row), fwd([5, 6, 7]), fwd(range(8, 77))]
    recs = []
    for m in (65, 128, 200):
        w = fwd(range(3, 3 + m))
        recs.append((f"del{m}", [w, fwd([3, 3 + m])], ["0", "0", "."]))                    # found; found reversed
        recs.append((f"last{m}", [w[:-1] + [(3 + m, 0)], w[:-1] + [(w[-1][0], 1)]], ["0|1", "0|1", "."]))  # the last step differs
        recs.append((f"first{m}", [[(2 + m, 0)] + w[1:]], ["0", "0", "."]))               # the first step differs
    recs.append(("end70", [fwd(range(7, 77))], ["0", "0", "0"]))  # 70 steps from the last step of q#1#a: absent in q
    recs.append(("in69", [fwd(range(8, 77)), fwd(range(8, 78))], ["0", "1", "0|1"]))  # fits q#1#b exactly; one more does not
    return names, steps, recs


def test_long_walks(hip):
    names, steps, recs = long_case()
    g = chain(204)
    seqs = W.random_sequences(g, 3, max_len=9)
    sq = dict(zip(g.vid.tolist(), seqs))
    resident(hip, g, names, steps, seqs)
    text = vcf_of(["ref", "back", "q"], recs, sq)
    rep, want, doc = check(hip, text, names, steps, sq.keys(), sq, spelling=True)
    A, F, B = R.ABSENT, R.FOUND_FWD, R.FOUND_REV
    # (phase 1 of `last` is beyond the one slot of ref and of back: no slot; what is left, by record: del found in ref and
    # reversed in back, last and first absent in both; end70 absent in q alone; in69 in q, in ref, one more step in back)
    got = [s for s in want["task_status"] if s != R.NO_SLOT]
    assert got[:18] == [F, B, A, A, A, A] * 3 and got[18:] == [F, B, A, F, F, B]
    # the walks of more than 64 steps reach the second tier unforced, lanes across their steps
    assert sum(len(al["walk"]) > 64 for r in doc["records"] for al in r["alleles"]) == 15
    assert rep.n_misspelled == 0 and rep.n_tier2 == 30


def repeat_case():
    """`many` visits 7 seventy times and only the last visit goes on to 9; `never` visits it seventy times and never does."""
    names = ["many#1#c", "never#1#c"]
    steps = [fwd([2, 7] * 69 + [2, 7, 9]), fwd([3, 7] * 70 + [3, 9])]
    recs = [("go", [fwd([7, 9]), fwd([7, 2, 7, 9]), fwd([7, 3, 9])], ["0|1", "0|2"]),
            ("one", [fwd([7]), [(7, 1)], fwd([9]), [(8, 0)]], ["0", "1"]),
            ("one2", [fwd([7]), [(7, 1)], fwd([9]), [(8, 0)]], ["2", "3"])]
    return names, steps, recs


def test_many_candidates_and_walks_of_one_step(hip):
    names, steps, recs = repeat_case()
    sq = {i: "ACGT"[i % 4] * (i % 3) for i in range(1, 10)}
    resident(hip, chain(9), names, steps, [sq[i] for i in range(1, 10)])
    rep, want, _ = check(hip, vcf_of(["many", "never"], recs, sq), names, steps, sq.keys(), sq, spelling=True)
    got = [s for s in want["task_status"] if s != R.NO_SLOT]
    assert got == [R.FOUND_FWD, R.ABSENT, R.FOUND_FWD, R.FOUND_REV, R.FOUND_FWD, R.ABSENT]
    assert 0 < rep.n_tier2 < n_searches(R.parse(vcf_of(["many", "never"], recs, sq)), steps, set(sq), False, True)


# ---- slots

def test_slot_rules(hip):
    names = ["two#1#c", "two#2#c", "pair#1#a", "pair#1#b", "lonely", "two#2#d"]
    steps = [fwd([1, 2, 3]), fwd([1, 4, 3]), fwd([5, 6]), fwd([1, 2, 3]), fwd([1, 4, 3]), fwd([7, 8])]
    sq = {i: "ACGT"[i % 4] for i in range(1, 9)}
    resident(hip, chain(8), names, steps, [sq[i] for i in range(1, 9)])
    a, b, c = fwd([1, 2, 3]), fwd([1, 4, 3]), fwd([7, 8])
    recs = [("r0", [a, b], ["0|1", "0", "1", "0"]),       # both haplotypes of `two`; the walk in the second path of `pair`'s slot
            ("r1", [a, b, c], ["1|2", "1", "0", "1|0"]),  # two: absent, found in the second path of hap 2; pair, lonely: absent
            ("r2", [a, b], ["0|1|0", "./0", "0|0", "."])]  # a phase beyond the slots of two, of pair, of lonely
    # (ghost is a column no sample is named like)
    rep, want, doc = check(hip, vcf_of(["two", "pair", "lonely", "ghost"], recs, sq), names, steps, sq.keys(), sq, spelling=True)
    F, A, N = R.FOUND_FWD, R.ABSENT, R.NO_SLOT
    by_rec = [want["task_status"][int(rep.doc.task_off[r]):int(rep.doc.task_off[r + 1])] for r in range(3)]
    assert by_rec == [[F, F, N, F, F], [A, N, A, A, N, F], [F, N, N, A, N, F]]  # (the tasks of a record come by allele)
    lines = rep.report_text().splitlines()[1:]
    assert [ln.split("\t")[4:] for ln in lines] == [["1", "ghost", "no_slot"], ["1", "lonely", "absent"], ["1", "two", "no_slot"]]
    # the hap number of a slot: two's second haplotype
    recs = [("h", [a, b], ["1|0", ".", ".", "."])]
    rep, want, _ = check(hip, vcf_of(["two", "pair", "lonely", "ghost"], recs, sq), names, steps, sq.keys())
    assert rep.report_text().splitlines()[1].split("\t")[3:] == [">1>2>3", "2", "two", "absent"]


# ---- mutations of a clean VCF

def mutate(text, pick, change):
    """The text with the first record line `pick` accepts rewritten by `change` (both take the fields), and that record's index."""
    lines = text.split("\n")
    k = 0
    for i, ln in enumerate(lines):
        if not ln or ln.startswith("#"):
            continue
        f = ln.split("\t")
        if pick(f):
            lines[i] = "\t".join(change(f))
            return "\n".join(lines), k
        k += 1
    raise AssertionError("no record to mutate")


def info_with(f, fn):
    """The fields with the AT key of INFO rewritten by `fn` (None: removed)."""
    out = []
    for kv in f[7].split(";"):
        if kv.startswith("AT="):
            kv = fn(kv)
            if kv is None:
                continue
        out.append(kv)
    return f[:7] + [";".join(out)] + f[8:]


def test_mutations_of_a_clean_vcf(hip):
    g = W.chain_of_bubbles(40)
    p = W.pansn(W.chain_haplotypes(40, 8, seed=9, reverse_every=0), samples=8, haps=1)
    seqs = W.random_sequences(g, 9, max_len=12, empty=0.0)
    (text, want, doc), _ = round_trip(hip, g, p, seqs, ["sample0#1"])
    names, steps = list(p.names), [p.steps(k) for k in range(len(p))]
    sq = dict(zip(g.vid.tolist(), seqs))
    n_steps = lambda f, a: sum(c in "<>" for c in f[7].split("AT=")[1].split(";")[0].split(",")[a])  # noqa: E731
    gt0 = lambda f: "0" in f[9:] and "1" in f[9:] and n_steps(f, 0) >= 2 and n_steps(f, 1) >= 2  # noqa: E731
    swap = lambda f: f[:9] + [{"0": "1", "1": "0"}.get(x, x) if k == f[9:].index("1") else x for k, x in enumerate(f[9:])]  # noqa: E731
    flip = lambda kv: "AT=" + kv[3:].replace(">", "<", 1)  # noqa: E731
    ghost = lambda kv: "AT=" + kv[3:kv.index(",") + 2] + "999999999" + kv[kv.index(",") + 2:].lstrip("0123456789")  # noqa: E731
    anchored = lambda f: "VARTYPE=INS" in f[7] and len(f[4].split(",")[0]) >= 2  # noqa: E731
    other = lambda c: "A" if c != "A" else "C"  # noqa: E731
    cases = [
        ("one GT swapped", gt0, swap, "absent", False),
        ("one step's orientation flipped", gt0, lambda f: info_with(f, flip), "absent", False),
        ("an id the graph lacks", gt0, lambda f: info_with(f, ghost), "bad_step", False),
        ("AT removed", gt0, lambda f: info_with(f, lambda kv: None), "no_at", False),
        ("one ALT base changed", gt0, lambda f: f[:4] + [f[4][:-1] + other(f[4][-1])] + f[5:], "misspelled", True),
        ("an anchored ALT without its anchor base", anchored, lambda f: f[:4] + [f[4][1:]] + f[5:], "misspelled", True),
    ]
    for what, pick, change, reason, spelling in cases:
        bad, r = mutate(text, pick, change)
        rep, res, _ = check(hip, bad, names, steps, sq.keys(), sq, spelling=spelling)
        assert res["rec_invalid"] == [int(k == r) for k in range(len(doc["records"]))], what
        assert rep.report_text().splitlines()[1].split("\t")[0] == str(r) and rep.report_text().splitlines()[1].endswith("\t" + reason), what
        assert rep.summary_text() == "Error rate: %.2f%%\n" % (100 / len(doc["records"])), what
        if not spelling:  # (without the flag nothing is spelled)
            assert not rep.allele_spell.any()


# ---- past 64: tasks, alleles, bases, steps and occurrences (the builders at module level; tests/test_cohort_inputs.py
# checks on the restatement what they reach)

NIL = R.NIL
other = lambda c: "A" if c != "A" else "C"  # noqa: E731


def set_gt(col, phase, allele):
    """A change for `mutate`: the genotype of sample column `col` at `phase` becomes `allele`."""
    def change(f):
        gt = f[9 + col].split("|")
        gt[phase] = str(allele)
        return f[:9 + col] + ["|".join(gt)] + f[10 + col:]
    return change


def first_failure_in(text, names, steps, segments, lo, hi, allele=None, pick=lambda f: True):
    """(record id, column, phase, allele, in-record task index): one genotype of a clean VCF that, set to another allele of its
    record (to `allele` when given), is that record's first failing task, at an in-record index in [lo, hi)."""
    head = [ln for ln in text.split("\n") if ln.startswith("#")]
    for ln in text.split("\n"):
        f = ln.split("\t")
        if not ln or ln.startswith("#") or not pick(f):
            continue
        for b in (range(1 + len(f[4].split(","))) if allele is None else [allele]):
            for c in range(len(f) - 9):
                for j, a in enumerate(f[9 + c].split("|")):
                    if a in (".", str(b)):
                        continue
                    doc = R.parse("\n".join(head + ["\t".join(set_gt(c, j, b)(f))]))
                    at = doc["records"][0]["tasks"].index((b, c, j))
                    if lo <= at < hi and R.check(doc, names, steps, segments)["rec_task"][0] == at:
                        return f[2], c, j, b, at
    raise AssertionError("no genotype to change")


def late_failures(text, names, steps, segments):
    """Mutations of the wide cohort's clean VCF: (what, text, record, (reason, allele, in-record task or None))."""
    spelled = lambda f: f[3] and all(f[4].split(","))  # noqa: E731
    out = []
    for what, lo, hi in (("the first failing task in the second batch", 64, 128), ("the first failing task in the third batch or later", 128, 1 << 30)):
        ident, c, j, b, at = first_failure_in(text, names, steps, segments, lo, hi)
        bad, r = mutate(text, lambda f: f[2] == ident, set_gt(c, j, b))
        out.append((what, bad, r, (R.ABSENT, b, at)))
    ident, c, j, b, at = first_failure_in(text, names, steps, segments, 64, 128, allele=0, pick=spelled)
    alt1 = lambda f: f[:4] + [f[4][:f[4].index(",") - 1] + other(f[4][f[4].index(",") - 1]) + f[4][f[4].index(","):]] + f[5:]  # noqa: E731
    bad, r = mutate(text, lambda f: f[2] == ident, lambda f: alt1(set_gt(c, j, b)(f)))
    out.append(("allele 1 misspelled, a task of allele 0 fails in the second batch: the task's reason", bad, r, (R.ABSENT, 0, at)))
    ref = lambda f: f[:3] + [f[3][:-1] + other(f[3][-1])] + f[4:]  # noqa: E731
    bad, r = mutate(text, lambda f: f[2] == ident, lambda f: ref(set_gt(c, j, b)(f)))
    out.append(("allele 0 misspelled and a task of allele 0 fails: misspelled", bad, r, (R.MISSPELLED, 0, None)))
    return out


@pytest.mark.parametrize("ref", CC.REFS)
def test_wide_cohort_round_trip_and_first_failures_in_later_batches(hip, ref):
    g, p = CC.wide_chain()
    seqs = CC.wide_sequences(g)
    (text, want, doc), _ = round_trip(hip, g, p, seqs, [ref])
    assert len(doc["samples"]) == 131 and min(len(r["tasks"]) for r in doc["records"]) >= 258
    names, steps, sq = list(p.names), CC.steps_of(p), dict(zip(g.vid.tolist(), seqs))
    for what, bad, r, (reason, allele, at) in late_failures(text, names, steps, set(sq)):
        rep, res, _ = check(hip, bad, names, steps, sq.keys(), sq, spelling=True)
        task = NIL if at is None else int(rep.doc.task_off[r]) + at
        assert (int(rep.rec_reason[r]), int(rep.rec_allele[r]), int(rep.rec_task[r])) == (reason, allele, task), what
        assert rep.rec_invalid.tolist() == [int(k == r) for k in range(len(doc["records"]))], what
        assert rep.report_text().splitlines()[1].endswith("\t" + R.STATUS_NAME[reason]), what


def many_alleles_case(misspelled):
    """A row of 71 segments under one path and one record of REF >1 and the 70 ALTs >2 .. >71, the ALTs `misspelled` (allele
    numbers) with a wrong first base: (names, steps, sequences by id, VCF text)."""
    names, steps = ["s#1#c"], [fwd(range(1, 72))]
    sq = {i: "ACGT"[i % 4] * (1 + i % 3) for i in range(1, 72)}
    text = vcf_of(["s"], [("many", [fwd([i]) for i in range(1, 72)], ["0"])], sq)

    def change(f):
        alts = f[4].split(",")
        for a in misspelled:
            alts[a - 1] = other(alts[a - 1][0]) + alts[a - 1][1:]
        return f[:4] + [",".join(alts)] + f[5:]
    return names, steps, sq, mutate(text, lambda f: True, change)[0]


@pytest.mark.parametrize("misspelled", [(66,), (3, 66)])
def test_more_than_64_alleles_in_a_record(hip, misspelled):
    names, steps, sq, text = many_alleles_case(misspelled)
    resident(hip, chain(71), names, steps, [sq[i] for i in range(1, 72)])
    rep, want, _ = check(hip, text, names, steps, sq.keys(), sq, spelling=True)
    assert (int(rep.rec_reason[0]), int(rep.rec_allele[0]), int(rep.rec_task[0])) == (R.MISSPELLED, misspelled[0], NIL)
    assert rep.n_misspelled == len(misspelled) and rep.allele_spell.tolist() == [R.SPELL_MISSPELLED if a in misspelled else R.SPELL_WHOLE for a in range(71)]


LONG = (64, 65, 130, 200)  # bases of segments 2 .. 5 of long_segments_case


def long_segments_case():
    """Segment 1 is AC, segments 2 .. 5 have LONG bases, 6 .. 8 are segment 4 with a byte that is no nucleotide code at index 70,
    as the last base and as the first.  One record an allele: (names, steps, sequences in id order, VCF text, the spelling
    expected of every allele).  Every long segment is spelled '>' and '<', whole and behind the anchor base of segment 1,
    rightly and with one wrong base at oriented index 63, 64, 129 and at the last index, where it has them."""
    rng = np.random.default_rng(7)
    seqs = ["AC"] + ["".join("ACGT"[k] for k in rng.integers(0, 4, size=n)) for n in LONG]
    seqs += [seqs[3][:70] + "Q" + seqs[3][71:], seqs[3][:-1] + "Q", "Q" + seqs[3][1:]]
    sq = dict(enumerate(seqs, 1))
    wrong = lambda t, i: t[:i] + other(t[i]) + t[i + 1:]  # noqa: E731
    rows = [([(2, 0)], seqs[1], R.SPELL_WHOLE, "0")]  # (the one allele with a task)
    for x, n in zip(range(2, 6), LONG):
        for o in (0, 1):
            t = R._oriented((x, o), sq)
            rows += [([(x, o)], t, R.SPELL_WHOLE, "."), ([(1, 0), (x, o)], "C" + t, R.SPELL_ANCHORED, ".")]
            for i in sorted({63, 64, 129, n - 1}):
                if i < n:
                    rows += [([(x, o)], wrong(t, i), R.SPELL_MISSPELLED, "."), ([(1, 0), (x, o)], "C" + wrong(t, i), R.SPELL_MISSPELLED, ".")]
    # the first step of an anchored reading gives its last base alone: a byte that is no code elsewhere in it does no harm,
    # as the last oriented base it does; read whole it does wherever it stands
    rows += [([(6, 0), (2, 0)], seqs[5][-1] + seqs[1], R.SPELL_ANCHORED, "."), ([(6, 1), (2, 0)], V._COMP[seqs[5][0]] + seqs[1], R.SPELL_ANCHORED, "."),
             ([(7, 0), (2, 0)], "Q" + seqs[1], R.SPELL_MISSPELLED, "."), ([(8, 1), (2, 0)], "Q" + seqs[1], R.SPELL_MISSPELLED, "."),
             ([(6, 0)], seqs[5], R.SPELL_MISSPELLED, "."), ([(6, 1)], "".join(V._COMP.get(c, "Q") for c in reversed(seqs[5])), R.SPELL_MISSPELLED, ".")]
    out = ["##fileformat=VCFv4.2\n", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT", "s"]) + "\n"]
    for k, (w, t, _, gt) in enumerate(rows):
        out.append("\t".join(["c", str(k + 1), f"r{k}", t, ".", "60", "PASS", "AT=" + at_of(w), "GT", gt]) + "\n")
    return ["s#1#c"], [fwd(range(1, 9))], seqs, "".join(out), [r[2] for r in rows]


def test_long_segments_in_the_spelling(hip):
    names, steps, seqs, text, expected = long_segments_case()
    sq = dict(enumerate(seqs, 1))
    resident(hip, chain(8), names, steps, seqs)
    rep, want, _ = check(hip, text, names, steps, sq.keys(), sq, spelling=True)
    assert want["allele_spell"] == expected and rep.allele_spell.tolist() == expected
    assert rep.n_misspelled == expected.count(R.SPELL_MISSPELLED) >= 40


def tier_edges_case():
    """(names, steps, records, the status expected of every task that has a slot).  `row` walks 101 .. 200: walks of exactly 64
    and 65 steps; a64 visits 7 exactly 64 times, a65 visits 8 exactly 65 times; `late` visits 15 sixty-six times and only behind
    the last visit go 20 .. 90 (a walk of 72 steps); m1, m2 and m3 visit 11 fifty, fifty and forty-one times, 141 times in
    three slots, and only the last visit goes on to 13."""
    names = [n + "#1#c" for n in ("row", "a64", "a65", "late", "m1", "m2", "m3")]
    steps = [fwd(range(101, 201)), fwd([2, 7] * 64), fwd([3, 8] * 65), fwd([15, 14] * 65 + [15] + list(range(20, 91))),
             fwd([11, 12] * 50), fwd([11, 12] * 50), fwd([11, 12] * 40 + [11, 13])]
    tail = fwd([15] + list(range(20, 91)))
    gt = lambda **kw: [kw.get(n.split("#")[0], ".") for n in names]  # noqa: E731
    miss = lambda w: w[:-1] + [(w[-1][0] + 2, 0)]  # noqa: E731  (the last step differs)
    w64, w65 = fwd(range(103, 167)), fwd(range(103, 168))
    recs = [("w64", [w64], gt(row="0")), ("w64x", [miss(w64)], gt(row="0")), ("w65", [w65], gt(row="0")), ("w65x", [miss(w65)], gt(row="0")),
            ("a64", [fwd([7, 2])], gt(a64="0")), ("a64x", [fwd([7, 3])], gt(a64="0")),
            ("a65", [fwd([8, 3])], gt(a65="0")), ("a65x", [fwd([8, 2])], gt(a65="0")),
            ("late", [tail], gt(late="0")), ("latex", [miss(tail)], gt(late="0")), ("lateb", [R.flipped(tail)], gt(late="0")),
            ("many", [fwd([11, 13])], gt(m1="0", m2="0", m3="0"))]
    F, B, A = R.FOUND_FWD, R.FOUND_REV, R.ABSENT
    return names, steps, recs, [F, A, F, A, F, A, F, A, F, A, B, A, A, F]


TIER_EDGES_TIER2 = 13  # searches the second tier takes unforced: by the rule of n_searches, counted in tests/test_cohort_inputs.py


def test_tier_edges(hip):
    names, steps, recs, expected = tier_edges_case()
    sq = {i: "A" for i in range(1, 201)}
    resident(hip, chain(200), names, steps)
    text = vcf_of([n.split("#")[0] for n in names], recs, sq)
    rep, want, doc = check(hip, text, names, steps, sq.keys())
    assert want["task_status"] == expected
    # unforced, the second tier takes the walks of 65 and 72 steps and the anchors of 65, 66 and 141 occurrences, not those of 64
    assert rep.n_tier2 == n_searches(doc, steps, set(sq), False, False) == TIER_EDGES_TIER2


# ---- beyond the capped grids: COUNT_BLOCKS = 2048 workgroups of four waves, of 256 lanes

CAP_WAVES, CAP_LANES = 8192, 524288


def capped_records_case(n=8300, absent=8250, misspelled=8260):
    """More records and alleles than the record and the spelling kernels have waves: `n` records of two alleles and one column on
    a row of six segments, clean but for record `absent` (its genotype's walk skips a segment) and record `misspelled` (its
    ALT has a wrong base), both from record CAP_WAVES on: (names, steps, sequences by id, VCF text)."""
    names, steps = ["s#1#c"], [fwd(range(1, 7))]
    sq = {i: "ACGT"[i % 4] * (1 + i % 3) for i in range(1, 7)}
    recs = []
    for k in range(n):
        a = 1 + k % 4
        walks = [fwd([a, a + 1]), fwd([a + 1, a + 2])]
        if k == absent:
            walks[k % 2] = fwd([a, a + 2])
        recs.append((f"r{k}", walks, [str(k % 2)]))
    text = vcf_of(["s"], recs, sq)
    text, _ = mutate(text, lambda f: f[2] == f"r{misspelled}", lambda f: f[:4] + [other(f[4][0]) + f[4][1:]] + f[5:])
    return names, steps, sq, text


def test_more_records_and_alleles_than_waves(hip):
    names, steps, sq, text = capped_records_case()
    resident(hip, chain(6), names, steps, [sq[i] for i in range(1, 7)])
    rep, want, doc = check(hip, text, names, steps, sq.keys(), sq, spelling=True)
    assert rep.n_records == 8300 > CAP_WAVES and len(want["allele_spell"]) == 16600
    assert np.flatnonzero(rep.rec_invalid).tolist() == [8250, 8260] and (rep.n_invalid, rep.n_misspelled) == (2, 1)
    assert rep.rec_reason[[8250, 8260]].tolist() == [R.ABSENT, R.MISSPELLED] and np.flatnonzero(rep.allele_spell == R.SPELL_MISSPELLED).tolist() == [2 * 8260 + 1]


def capped_tasks_case(text, names, steps, segments, copies=168):
    """More tasks than the task kernel has lanes: the wide cohort's clean VCF `copies` times over, with one genotype of the
    very last record changed so that the only failing task of the document lies behind task CAP_LANES: (header lines, the
    record lines of a copy, those of the last copy)."""
    block = [ln for ln in text.split("\n") if ln and not ln.startswith("#")]
    head = [ln for ln in text.split("\n") if ln.startswith("#")]
    ident, c, j, b, at = first_failure_in(text, names, steps, segments, 128, 1 << 30, pick=lambda f: f[2] == block[-1].split("\t")[2])
    return head, block, block[:-1] + ["\t".join(set_gt(c, j, b)(block[-1].split("\t")))]


def restated_copies(head, block, last, copies, names, steps, segments):
    """(document, result) of the VCF of `head`, `block` copies - 1 times and `last` (as many lines as `block`): the restatement
    reads and checks one block and the last one, and numpy repeats the first.  A record's tasks, alleles and verdict are its own
    (vcfcheck_ref.check carries nothing from one record to the next but the count of tasks), so this is the restatement of the
    whole document; tests/test_cohort_inputs.py compares the two once."""
    docs = [R.parse("\n".join(head + lines)) for lines in (block, last)]
    res = [R.check(doc, names, steps, segments) for doc in docs]
    n, n_tasks = len(block), len(res[0]["task_status"])
    records = [dict(r, line=r["line"] + c * n) for c in range(copies) for r in docs[c == copies - 1]["records"]]
    want = {}
    for k in ("task_status", "allele_spell", "rec_invalid", "rec_reason", "rec_allele"):
        want[k] = np.concatenate([np.tile(np.array(res[0][k], dtype=np.int64), copies - 1), np.array(res[1][k], dtype=np.int64)]).tolist()
    task = np.concatenate([np.tile(np.array(res[0]["rec_task"], dtype=np.int64), copies - 1), np.array(res[1]["rec_task"], dtype=np.int64)])
    want["rec_task"] = np.where(task == NIL, NIL, task + np.repeat(np.arange(copies, dtype=np.int64) * n_tasks, n)).tolist()
    want["n_status"] = [(copies - 1) * x + y for x, y in zip(res[0]["n_status"], res[1]["n_status"])]
    for k in ("n_invalid", "n_misspelled"):
        want[k] = (copies - 1) * res[0][k] + res[1][k]
    return dict(samples=docs[0]["samples"], records=records), want


def test_more_tasks_than_lanes(hip):
    g, p = CC.wide_chain()
    seqs = CC.wide_sequences(g)
    names, steps, sq = list(p.names), CC.steps_of(p), dict(zip(g.vid.tolist(), seqs))
    (text, _, _), _ = round_trip(hip, g, p, seqs, [CC.REF_LOW])
    head, block, last = capped_tasks_case(text, names, steps, set(sq))
    big = "\n".join(head + block * 167 + last) + "\n"
    rep, want, doc = check(hip, big, names, steps, sq.keys(), restated=restated_copies(head, block, last, 168, names, steps, set(sq)))
    r = 168 * len(block) - 1
    assert rep.n_tasks > CAP_LANES and rep.n_records == r + 1 == 2016
    assert np.flatnonzero(rep.rec_invalid).tolist() == [r] and int(rep.rec_task[r]) >= CAP_LANES and rep.n_status[R.ABSENT] == rep.n_invalid == 1
    assert int(rep.task_status[int(rep.rec_task[r])]) == R.ABSENT and int(np.count_nonzero(rep.task_status > R.FOUND_REV)) == 1


# ---- state

def test_two_graphs_in_one_context_and_the_refusals(hip):
    names, steps, recs = path_end_case()
    sq = {i: "A" for i in range(1, 7)}
    text = vcf_of(["s", "t"], recs, sq)
    hip.upload(chain(6))
    with pytest.raises(RuntimeError, match="no paths are resident"):
        hip.check_vcf(text)
    hip.upload_paths(paths_of(names, steps))
    with pytest.raises(RuntimeError, match="spelling check needs the sequences"):
        hip.check_vcf(text, spelling=True)
    with pytest.raises(RuntimeError, match=r"^line 3: POS is no number: x$"):
        hip.check_vcf(text.replace("\t1\tover\t", "\tx\tover\t"))
    # segment ids that do not ascend with the vertex index: the path upload refuses them, so no check meets such a graph (its
    # own refusal of them is never reached) and the paths of the graph before are gone
    g = chain(6)
    hip.upload(W._mk(g.vid[::-1].copy(), g.v1, g.s1, g.v2, g.s2))
    with pytest.raises(RuntimeError, match="paths need segment ids that ascend with the vertex index"):
        hip.upload_paths(paths_of(names, steps))
    with pytest.raises(RuntimeError, match="no paths are resident"):
        hip.check_vcf(text)
    hip.upload(g)
    hip.upload_paths(paths_of(names, steps))
    first, _, _ = check(hip, text, names, steps, sq.keys())
    # a larger graph, then the first again: nothing of the other is left
    n2, s2, r2 = repeat_case()
    sq2 = {i: "C" for i in range(1, 10)}
    resident(hip, chain(9), n2, s2)
    with pytest.raises(RuntimeError, match="spelling check needs the sequences"):
        hip.check_vcf(text, spelling=True)  # (the upload dropped them)
    check(hip, vcf_of(["many", "never"], r2, sq2), n2, s2, sq2.keys())
    # the first VCF against the second graph: its columns name nobody
    rep, want, _ = check(hip, text, n2, s2, sq2.keys())
    assert set(want["task_status"]) == {R.NO_SLOT}
    resident(hip, chain(6), names, steps)
    again, _, _ = check(hip, text, names, steps, sq.keys())
    assert again.task_status.tolist() == first.task_status.tolist() and again.report_text() == first.report_text()
    # an empty VCF and one without records
    rep, _, _ = check(hip, "", names, steps, sq.keys())
    assert (rep.n_records, rep.n_tasks, rep.summary_text()) == (0, 0, "No errors\n")
    # paths without a step: nothing is found, nothing is searched
    resident(hip, chain(6), ["s#1#a", "t#1#a"], [[], []])
    rep, want, _ = check(hip, text, ["s#1#a", "t#1#a"], [[], []], sq.keys())
    assert R.FOUND_FWD not in want["task_status"] and R.ABSENT in want["task_status"]
