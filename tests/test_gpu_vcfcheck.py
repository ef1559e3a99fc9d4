"""GPU VCF checks (povu_hip_vcf_check, HipDecomposer.check_vcf) against the plain-Python restatement (tests/vcfcheck_ref.py),
array for array and text for text, every case again with the forced second tier (equal but for n_tier2): the round trip of this
project's own calls (plain and with inversions, spelling on: no invalid record, no misspelled allele) on the eleven conformance
GFAs, PanSN haplotypes of a chain and a -s forest; references that run backwards (FOUND_REV, ABSENT under forward_only); walks
at the ends of paths; walks of 65, 128 and 200 steps; a repeat one path visits 70 times; the slot rules; mutations of a clean
VCF; two graphs in one context and the refusals."""
import os

import numpy as np
import pytest

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


def check(d, text, names, steps, segments, sq=None, forward_only=False, spelling=False):
    """Both tiers equal the restatement; returns (the report of the first, the restatement's result, its document)."""
    doc = R.parse(text)
    segments = set(segments)
    want = R.check(doc, names, steps, segments, sq, forward_only=forward_only, spelling=spelling)
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
