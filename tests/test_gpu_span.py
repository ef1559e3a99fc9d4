"""GPU spanning alleles (povu_hip_call with POVU_HIP_T_SPANNING, HipDecomposer.call(..., spanning=True); INTEGRATION.md
"Spanning alleles") against the plain-Python restatement (tests/span_ref.py): records, gt, ac, an, ns, rec_star, the
counters and the VCF text.  The fixture against the stored lines, raw-graph and popped; the same calls without the flag,
byte-equal to the nested call; skip_nested haplotypes in 5, 64, 65 and 130 slots (the lane stride over the slots, two slots
of one sample); towers of width 1 whose innermost record has 1, 2, 64, 65 and 71 ancestors (the chain rounds at 64: a slot
crossed at the outermost ancestor alone); a haplotype that ends before a unit ('.' beside `*` in one record); a truncated
search (no `*` there); two reference paths; inversion records; regions; the VCF checks and the VCF comparison on the
flag's own text.  The VCF checks against their own restatement with the `*` rule (tests/span_vcfcheck_ref.py): an input whose
nested call checks clean without the flag checks clean with it, every task of a `*` allele found_fwd; mutations of that text;
the text of a skip_nested call."""
import json
import os

import numpy as np
import pytest

import nested_ref as N
import span_ref as S
import span_vcfcheck_ref as SR
import vcf_ref as V
import vcfcheck_cases as K
import vcfcheck_ref as R
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W
from test_gpu_nested import _flags, _setup
from test_oracle import _load_gfa_links

pytestmark = pytest.mark.gpu

DATE = "00000000"
NIL = 0xFFFFFFFF
FIXTURE = "downstream_repetitive/popped-parent-child-rescue"


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _same(c, want, counters):
    """The device's arrays equal the restatement's records; the counters are those of the arrays."""
    assert c.nested and c.spanning and c.n_records == len(want)
    assert [(int(c.path[i]), int(c.pos[i]), int(c.query[i]), int(c.first[i])) for i in range(c.n_records)] == \
        [(r["path"], r["pos"], r["q"], r["first"]) for r in want]
    assert c.n_alleles.tolist() == [r["n_alleles"] for r in want]
    assert c.rec_star.tolist() == [1 if r["star"] else 0 for r in want]
    assert c.ref_allele.tolist() == [r["ref_class"] for r in want]
    assert c.gt.tolist() == [[H.GT_MISSING if g is None else g for g in r["slots"]] for r in want]
    assert c.ac_off.tolist() == np.concatenate([[0], np.cumsum([len(r["ac"]) for r in want])]).tolist()
    assert c.ac.tolist() == [x for r in want for x in r["ac"]]
    assert c.an.tolist() == [r["an"] for r in want] and c.ns.tolist() == [r["ns"] for r in want]
    assert c.level.astype(np.int32).tolist() == [r["lv"] for r in want]
    assert c.parent_query.tolist() == [NIL if r["parent"] is None else r["parent"] for r in want]
    assert c.flags.tolist() == [_flags(r) for r in want]
    got = dict(n_enclosed=c.n_enclosed, n_collapsed_sites=c.n_collapsed_sites, n_popped=c.n_popped, n_rescued=c.n_rescued,
               n_star_records=c.n_star_records, n_star_entries=c.n_star_entries)
    assert got == counters
    assert c.n_star_records == int(c.rec_star.sum())
    assert c.n_star_entries == sum(int((c.gt[i] == c.n_alleles[i] - 1).sum()) for i in range(c.n_records) if c.rec_star[i])


def _check(d, setup, names, prefixes, tflags=0, profile=None, max_steps=65536, **popt):
    f, sites, steps, sq = setup
    c = d.call(f, prefixes, flags=tflags | H.T_NESTED, profile=profile, spanning=True, max_steps=max_steps, **popt)
    want, counters = S.call_full(sites, names, steps, sq, prefixes, max_steps=max_steps, profile=profile, **popt)
    _same(c, want, counters)
    assert c.vcf_text(date=DATE) == S.vcf_text(names, steps, sq, want, prefixes, date=DATE, profile=profile)
    return c, want, counters


def _off_is_nested(d, setup, names, prefixes, profile=None, **popt):
    """Without the flag: today's nested call, byte for byte; no array, no count."""
    f, sites, steps, sq = setup
    c = d.call(f, prefixes, flags=H.T_NESTED, profile=profile, **popt)
    want = N.call(sites, names, steps, sq, prefixes, profile=profile, **popt)
    assert c.vcf_text(date=DATE) == N.vcf_text(names, steps, sq, want, prefixes, date=DATE, profile=profile)
    assert not c.spanning and c.rec_star.size == 0 and (c.n_star_records, c.n_star_entries) == (0, 0)
    assert c.n_alleles.tolist() == [r["n_classes"] for r in want]
    assert c.gt.tolist() == [[H.GT_MISSING if g is None else g for g in r["slots"]] for r in want]
    return c


def _fixture_setup(d, golden_dir, name=FIXTURE):
    gfa = os.path.join(golden_dir, "gfa", name + ".gfa")
    names, paths, seqs = V.read_gfa(gfa)
    g = _load_gfa_links(gfa)
    p = W._paths(names, [([i for i, _ in st], [r for _, r in st]) for st in paths])
    d.upload(g)
    f = d.decompose()
    d.upload_paths(p)
    d.upload_sequences([seqs[i] for i in g.vid.tolist()])
    sites = V.sites_of_pvst([f.text(i) for i in range(len(f))])
    return (f, sites, paths, seqs), names


def _records(text):
    return [ln for ln in text.splitlines() if ln and not ln.startswith("#")]


def test_fixture_raw_graph_and_popped(hip, golden_dir):
    golden = json.load(open(os.path.join(golden_dir, "span_records.json")))
    setup, names = _fixture_setup(hip, golden_dir)
    c, want, counters = _check(hip, setup, names, ["HG1"])
    assert _records(c.vcf_text(date=DATE)) == golden["profiles"]["raw-graph"]
    inner = _records(c.vcf_text(date=DATE))[1].split("\t")
    assert inner[2:5] == [">2>4", "A", "G,*"] and inner[7].startswith("AC=1,1;AF=0.3,0.3;AN=3;NS=3;AT=>3,>6,*;") and inner[9:] == ["0", "2", "1"]
    assert (c.n_star_records, c.n_star_entries) == (1, 1) and c.rec_star.tolist() == [0, 1]
    cp, _, _ = _check(hip, setup, names, ["HG1"], profile="popped", **golden["popped_options"])
    assert _records(cp.vcf_text(date=DATE)) == golden["profiles"]["popped"] and (cp.n_rescued, cp.n_star_records) == (1, 1)
    ct, _, _ = _check(hip, setup, names, ["HG1"], profile="top-level-only")
    assert _records(ct.vcf_text(date=DATE)) == golden["profiles"]["top-level-only"] and ct.n_star_records == 0
    # the same calls without the flag
    _off_is_nested(hip, setup, names, ["HG1"])
    _off_is_nested(hip, setup, names, ["HG1"], profile="popped", **golden["popped_options"])
    # the refusals of the library name the flag
    f = setup[0]
    for kw, word in ((dict(), "POVU_HIP_T_NESTED"), (dict(flags=H.T_NESTED, profile="left-normalized"), "left-normalized"),
                     (dict(profile="decomposed"), "decomposed")):
        with pytest.raises(RuntimeError, match="POVU_HIP_T_SPANNING") as e:
            hip.call(f, ["HG1"], spanning=True, **kw)
        assert word in str(e.value)
    # regions: the lines of the unrestricted call for the sites that pass, the counters those of the records written
    sel = hip.call(f, ["HG1"], flags=H.T_NESTED, spanning=True, regions="HG1#1#chr1:3-4")
    assert _records(sel.vcf_text(date=DATE)) == golden["profiles"]["raw-graph"][1:] and (sel.n_star_records, sel.n_star_entries) == (1, 1)
    assert sel.rec_star.tolist() == [1] and sel.n_region_dropped == 1
    sel = hip.call(f, ["HG1"], flags=H.T_NESTED, spanning=True, regions="HG1#1#chr1:1-2")
    assert _records(sel.vcf_text(date=DATE)) == golden["profiles"]["raw-graph"][:1] and (sel.n_star_records, sel.n_star_entries) == (0, 0)
    # the VCF checks: the `*` entry is no failure -- the record of >2>4 is valid, and the report is that of the text without
    # the flag (whose >0>5 hides HG3's walk in REF's class: invalid with and without)
    text = c.vcf_text(date=DATE)
    rep, rep0 = hip.check_vcf(text), hip.check_vcf(hip.call(f, ["HG1"], flags=H.T_NESTED).vcf_text(date=DATE))
    assert rep.rec_invalid.tolist() == rep0.rec_invalid.tolist() and rep.rec_invalid[1] == 0
    assert rep.n_tasks == rep0.n_tasks + 1 and rep.n_status[3] == rep0.n_status[3] == 0 and rep.n_status[4] == 0
    # the VCF comparison: only the skipped `*` item differs
    cmp = hip.compare_vcfs(text, hip.call(f, ["HG1"], flags=H.T_NESTED).vcf_text(date=DATE))
    assert (cmp.n_only_a, cmp.n_only_b, cmp.n_skipped_a, cmp.n_skipped_b) == (0, 0, 1, 0) and cmp.n_shared == 2


def _skip(units, depth, haps, seed, samples=None):
    g = W.skip_nested(units, depth, seed)
    p = W.skip_haplotypes(units, depth, haps, seed)
    return g, W.pansn(p, samples=samples or (haps + 1) // 2)


@pytest.mark.parametrize("haps", [5, 64, 65, 130])
def test_skip_haplotypes_slot_rounds(hip, haps):
    # (two haplotypes a sample: the slots of a sample are two lanes' worth of one column)
    g, p = _skip(3, 2, haps, seed=haps)
    setup = _setup(hip, g, p, seed=2, max_len=4)
    names = list(p.names)
    c, want, counters = _check(hip, setup, names, [names[0]])
    assert c.n_slots == haps and counters["n_star_records"] >= 3 and counters["n_star_entries"] > counters["n_star_records"]
    assert any(r["star"] and any(sl >= 64 for sl in r["spanned"]) for r in want) == (haps > 64)
    assert any("|" in x for r in want for x in r["gt"])
    _off_is_nested(hip, setup, names, [names[0]])
    if haps == 65:
        _check(hip, setup, names, [names[0]], tflags=H.T_FORCE_TIER2)
        _check(hip, setup, names, [names[0]], profile="popped", max_level=0, max_ref_length=6, max_allele_length=6)


def _tower(depth, ref_skip=-1):
    """skip_nested(1, depth, width=1) with a reference that walks everything (or takes the skip of unit `ref_skip`, the
    outermost being 0), a haplotype that walks everything, one on the SNP's other branch, and one haplotype per unit that takes
    that unit's skip alone: the SNP's record has depth + 1 ancestors, and the haplotype of the outermost skip crosses the
    outermost ancestor alone."""
    anc, snp, _, n_dec, _ = W._skip_template(depth, 1)
    g = W.skip_nested(1, depth, width=1)

    def walk(skip, branch):
        ids = [k + 1 for k in range(len(anc)) if skip not in anc[k] and (snp[k][0] < 0 or snp[k][1] == branch)]
        return np.array(ids, dtype=np.uint32), np.zeros(len(ids), dtype=np.uint8)
    pieces = ([walk(ref_skip, 0)] if ref_skip >= 0 else []) + [walk(-1, 0), walk(-1, 1)] + [walk(j, 0) for j in range(n_dec)]
    assert n_dec == depth + 1
    return g, W._paths([f"hap{h}#1#chr1" for h in range(len(pieces))], pieces)


@pytest.mark.parametrize("depth", [0, 1, 63, 64, 70])
def test_tower_chain_rounds(hip, depth):
    g, p = _tower(depth)
    setup = _setup(hip, g, p, seed=3, max_len=3)
    names = list(p.names)
    c, want, counters = _check(hip, setup, names, ["hap0#"])
    snp = max(want, key=lambda r: r["lv"])
    assert snp["lv"] == depth + 1 and len(want) == depth + 2
    # every skipping haplotype is spanned at the SNP; the outermost one (slot 2) by the outermost ancestor alone
    assert snp["spanned"] == list(range(2, depth + 3)) and snp["gt"][1] == "1" and snp["ac"] == [1, depth + 1]
    assert counters["n_star_records"] == depth + 1 and counters["n_star_entries"] == (depth + 1) * (depth + 2) // 2
    top = min(want, key=lambda r: r["lv"])
    assert not top["star"] and top["parent"] is None


def test_missing_and_spanned_in_one_record(hip):
    units, depth, haps = 3, 2, 8
    g = W.skip_nested(units, depth)
    full = W.skip_haplotypes(units, depth, haps, seed=1)
    size = int(g.vid.size) // units
    # haplotype 3 ends behind the first unit: no path of its slot at the later loci at all
    pieces = []
    for k in range(haps):
        st = [x for x in full.steps(k) if k != 3 or x[0] <= size]
        pieces.append(([i for i, _ in st], [r for _, r in st]))
    p = W.pansn(W._paths(list(full.names), pieces), samples=haps)
    setup = _setup(hip, g, p, seed=5, max_len=4)
    names = list(p.names)
    c, want, _ = _check(hip, setup, names, [names[0]])
    sites = setup[1]
    later = [r for r in want if sites[r["q"]]["s"][0] > size]
    assert later and all(r["slots"][3] is None for r in later)
    assert any(r["star"] and r["slots"][3] is None for r in later)  # both kinds of missing in one record


def test_truncated_search_gives_no_star(hip):
    # units 0 > 1 > 2 > SNP; the reference takes the innermost unit's skip, so its traversal of unit 1 has 5 steps and of unit
    # 0 8, while the full walks have 9 and 12: with max_steps 8 both sites are TRAV_LONG and still have two alleles each.  The
    # haplotype of the outermost skip is empty at unit 1 and crosses unit 0: spanned, were unit 1 not cut short
    g, p = _tower(2, ref_skip=2)
    setup = _setup(hip, g, p, seed=4, max_len=3)
    names = list(p.names)
    _, whole, _ = _check(hip, setup, names, ["hap0#"])
    c, want, _ = _check(hip, setup, names, ["hap0#"], max_steps=8)
    sites = setup[1]
    index = N.TR.PathIndex(setup[2])
    cut = {r["q"] for r in want if N.TR.traversals_of(index, sites[r["q"]]["s"], sites[r["q"]]["z"], 8)[2] != 0}
    assert any(r["q"] in cut and r["parent"] is not None for r in want) and not any(r["star"] for r in want if r["q"] in cut)
    assert any(r["star"] for r in want if r["q"] not in cut)  # (an untruncated child of the same call keeps its `*`)
    by_site = {r["q"]: r for r in whole}
    assert any(by_site[q]["star"] for q in cut if q in by_site)  # (without the limit the same site has one)


def _report(d, text, names, steps, sq, spelling=False):
    """The device's report of `text`, both tiers, equal to the restatement's: the document, every array, the counts, both
    files.  Returns (report, restatement's result, its document)."""
    doc = SR.parse(text)
    want = SR.check(doc, names, steps, set(sq), sq, spelling=spelling)
    first = None
    for force in (False, True):
        rep = d.check_vcf(text, spelling=spelling, force_tier2=force)
        assert K.lib_arrays(rep.doc) == R.doc_arrays(doc)
        for k in ("task_status", "allele_spell", "rec_invalid", "rec_reason", "rec_allele", "rec_task"):
            assert getattr(rep, k).tolist() == want[k], (k, force)
        assert (rep.n_status, rep.n_invalid, rep.n_misspelled) == (want["n_status"], want["n_invalid"], want["n_misspelled"])
        assert rep.report_text() == R.report_text(doc, want, names) and rep.summary_text() == R.summary_text(doc, want)
        first = first or rep
    return first, want, doc


def _star_tasks(doc):
    """Indices of the tasks that name an allele spelled `*`."""
    out, t0 = [], 0
    for rec in doc["records"]:
        out += [t0 + k for k, (a, _c, _j) in enumerate(rec["tasks"]) if SR.is_star(rec, a)]
        t0 += len(rec["tasks"])
    return out


def test_check_vcf_is_clean_on_the_flags_own_text(hip, golden_dir):
    # the fixture's graph with HG3 on segments 2, 6, 4 alone: it carries the SNP's ALT and does not traverse >0>5, so no class
    # of >0>5 hides a walk and the nested call checks clean, spelling included, without the flag
    setup, names = _fixture_setup(hip, golden_dir)
    f, sites, paths, sq = setup
    paths = [paths[0], paths[1], [(2, 0), (6, 0), (4, 0)]]
    hip.upload_paths(W._paths(names, [([i for i, _ in st], [r for _, r in st]) for st in paths]))
    setup = (f, sites, paths, sq)
    off = _off_is_nested(hip, setup, names, ["HG1"])
    rep0, want0, _ = _report(hip, off.vcf_text(date=DATE), names, paths, sq, spelling=True)
    assert rep0.n_invalid == 0 and rep0.n_misspelled == 0 and rep0.summary_text() == "No errors\n" and rep0.n_tasks == 4
    c, recs, _ = _check(hip, setup, names, ["HG1"])
    assert [(r["es"], r["gt"], r["alts"], r["collapsed"]) for r in recs] == [(">0>5", ["0", "1", "."], ["A"], False),
                                                                            (">2>4", ["0", "2", "1"], ["G", "*"], False)]
    text = c.vcf_text(date=DATE)
    rep, want, doc = _report(hip, text, names, paths, sq, spelling=True)
    assert rep.n_invalid == 0 and rep.n_misspelled == 0 and rep.summary_text() == "No errors\n" and rep.n_tasks == 5
    star = _star_tasks(doc)
    assert star == [4] and [int(rep.task_status[t]) for t in star] == [R.FOUND_FWD] and rep.n_status == [5, 0, 0, 0, 0, 0]
    assert rep.allele_spell.tolist() == [R.SPELL_WHOLE] * 4 + [R.SPELL_NONE]  # (`*` is not spelled)
    # mutations: the `*` entry left out of AT, every sample on `*`, a wrong walk on the other ALT, `*` in AT of an allele that is
    # not spelled so (an empty walk: no_at), a `*` ALT with a walk of its own (still not searched)
    inner = text.splitlines()[-1]
    for old, new, invalid, reason in (("AT=>3,>6,*", "AT=>3,>6", 0, None), ("\t0\t2\t1", "\t2\t2\t2", 0, None),
                                      ("AT=>3,>6,*", "AT=>3,>1,*", 1, R.ABSENT), ("\tG,*\t", "\tG,T\t", 1, R.NO_AT),
                                      ("AT=>3,>6,*", "AT=>3,>6,>1", 0, None)):
        assert old in inner
        r2, w2, d2 = _report(hip, text.replace(inner, inner.replace(old, new)), names, paths, sq)
        assert r2.rec_invalid.tolist() == [0, invalid] and (reason is None or int(r2.rec_reason[1]) == reason), (old, new)
        assert all(int(r2.task_status[t]) == R.FOUND_FWD for t in _star_tasks(d2))


def test_check_vcf_equals_its_restatement_on_a_skip_call(hip):
    g, p = _skip(3, 2, 12, seed=4)
    setup = _setup(hip, g, p, seed=4, max_len=4)
    names = list(p.names)
    c, want, counters = _check(hip, setup, names, [names[0]])
    rep, res, doc = _report(hip, c.vcf_text(date=DATE), names, setup[2], setup[3])
    star = _star_tasks(doc)
    assert len(star) == counters["n_star_entries"] > 0 and all(int(rep.task_status[t]) == R.FOUND_FWD for t in star)
    # the records that fail fail without the flag too, for the same task of the same allele
    rep0, _, _ = _report(hip, hip.call(setup[0], [names[0]], flags=H.T_NESTED).vcf_text(date=DATE), names, setup[2], setup[3])
    assert rep.rec_invalid.tolist() == rep0.rec_invalid.tolist() and rep.rec_allele.tolist() == rep0.rec_allele.tolist()
    assert rep.rec_reason.tolist() == rep0.rec_reason.tolist()


def test_two_reference_paths_and_inversions(hip, golden_dir):
    g, p = _skip(4, 2, 10, seed=6, samples=10)
    setup = _setup(hip, g, p, seed=6, max_len=4)
    names = list(p.names)
    c, want, _ = _check(hip, setup, names, [names[0], names[3]])
    assert len({r["path"] for r in want if r["star"]}) == 2  # per-reference chains
    # inversion records never carry a `*` and stay as they are
    inv = W.inverted_haplotypes(p, 6, 3, 9, seed=4, keep=(0,))
    hip.upload_paths(inv)
    f = setup[0]
    a = hip.call(f, [names[0]], flags=H.T_NESTED | H.T_INVERSIONS)
    b = hip.call(f, [names[0]], flags=H.T_NESTED | H.T_INVERSIONS, spanning=True)
    subr = lambda c: [ln for ln in _records(c.vcf_text(date=DATE)) if "VARTYPE=SUBR" in ln]  # noqa: E731
    assert a.n_inv_records > 0 and subr(a) == subr(b) and b.n_star_records > 0
    assert not any(b.rec_star[i] for i in range(b.n_records) if b.flags[i] & H.CALL_SUBR)
    steps = [inv.steps(k) for k in range(len(inv))]
    want, counters = S.call_full(setup[1], names, steps, setup[3], [names[0]])
    flub = [ln for ln in _records(b.vcf_text(date=DATE)) if "VARTYPE=SUBR" not in ln]
    assert flub == [S.record_line(r) for r in want] and b.n_star_entries == counters["n_star_entries"]
    # the hairpin fixture: its SUBR rows with and without the flag
    setup, names = _fixture_setup(hip, golden_dir, "hairpin_inversion_subr")
    f = setup[0]
    prefix = names[0].split("#")[0]
    a = hip.call(f, [prefix], flags=H.T_NESTED | H.T_INVERSIONS)
    b = hip.call(f, [prefix], flags=H.T_NESTED | H.T_INVERSIONS, spanning=True)
    assert a.n_inv_records > 0 and subr(a) == subr(b)
