"""The wide cohort (tests/cohort_cases.py) reaches what the GPU tests put it through for, on the restatements and the CPU oracle
alone.  "Restricted to n" is a record's AC / AN / NS recomputed from the restatement's own `slots` of the samples of index < n:
what a kernel would give whose lane-per-sample loop stopped after ceil(n / 64) rounds.  No GPU."""
import functools

import pytest

import cohort_cases as CC
import inversions_ref as I
import merge_ref as MR
import norm_ref as NR
import offref_ref as F
import oracle_lib as O
import prim_ref as PR
import test_gpu_vcfcheck as TV
import vcf_ref as V
import vcfcheck_ref as R

LATE_TANGLED = {">7>10", ">22>25", ">31>34"}  # the sites of CC.SECOND_DIFFERS: units 2, 7 and 10


@functools.lru_cache(maxsize=None)
def cohort():
    g, p = CC.wide_chain()
    names, steps = list(p.names), CC.steps_of(p)
    sq = dict(zip(g.vid.tolist(), CC.wide_sequences(g)))
    sites = V.sites_of_pvst(list(O.decompose(g).values()))
    return g, p, names, steps, sq, sites


@functools.lru_cache(maxsize=None)
def plain(ref):
    g, p, names, steps, sq, sites = cohort()
    return V.call(sites, names, steps, sq, [ref])


@functools.lru_cache(maxsize=None)
def inversions(ref):
    g, p, names, steps, sq, sites = cohort()
    return I.records(names, steps, sq, [ref])


def late(sample_of, slots, value):
    """{False, True}: whether the slots that hold `value` belong to samples below 64, to samples from 64 on."""
    return {sample_of[sl] >= 64 for sl, v in enumerate(slots) if v == value}


def test_shape_of_the_cohort():
    g, p, names, steps, sq, sites = cohort()
    samples, slot, sample_of = V.slots_of(names)
    assert len(names) == 263 and len(samples) == 131 and len(sample_of) == 261 and len(sites) == CC.UNITS == 12
    per_sample = [sample_of.count(s) for s in range(len(samples))]
    assert per_sample[:6] == [1, 2, 3, 1, 2, 3] and {per_sample[s] for s in range(64, 131)} == {1, 2, 3}  # mixed along the order
    assert sum(V.pansn(n)[1] is None for n in names) == 3 and all(samples[s] == f"bare{s}" for s in CC.BARE)
    for s in CC.TWO_CONTIGS:  # two contigs in one slot, past lane 63
        k = [i for i, n in enumerate(names) if n.startswith(f"s{s}#1#")]
        assert s >= 64 and len(k) == 2 and slot[k[0]] == slot[k[1]] and sample_of[slot[k[0]]] == s
        differ = [u for u in range(CC.UNITS) if {3 * u + 2, 3 * u + 3} & ({x for x, _ in steps[k[0]]} ^ {x for x, _ in steps[k[1]]})]
        assert tuple(differ) == CC.SECOND_DIFFERS[s]
    assert sum(st[0][1] for st in steps) == 66  # haplotypes written '<': every fourth, and one of the second contigs
    (lo,), (hi,), (cut,) = (V.ref_paths(names, [r]) for r in (CC.REF_LOW, CC.REF_HIGH, CC.REF_PARTIAL))
    assert sample_of[slot[lo]] == 1 and slot[lo] == 1        # the reference's slot in the first round
    assert sample_of[slot[hi]] == 130 and slot[hi] == 260    # ... and in the third (the fifth of a loop over slots)
    assert sample_of[slot[cut]] == CC.CUT_SAMPLE and {x for x, _ in steps[cut]} <= set(range(1, CC.CUT_AT + 1)) and steps[cut][-1][0] == CC.CUT_AT
    assert max(map(len, sq.values())) <= CC.MAX_LEN


@pytest.mark.parametrize("ref", CC.REFS)
def test_plain_call(ref):
    g, p, names, steps, sq, sites = cohort()
    samples, slot, sample_of = V.slots_of(names)
    raw = plain(ref)
    assert len(raw) == 12 and {len(r["alts"]) for r in raw} == {2}
    assert sum(CC.restricted_differs(r["slots"], sample_of, 64, r["ac"], r["an"], r["ns"]) for r in raw) == 12
    assert sum(CC.restricted_differs(r["slots"], sample_of, 128, r["ac"], r["an"], r["ns"]) for r in raw) >= 1
    # every ALT is carried on both sides of lane 63 and REF (code 0) as well: no count comes from one round alone
    assert all(late(sample_of, r["slots"], v) == {False, True} for r in raw for v in (0, 1, 2))
    # TANGLED through a slot of a late sample alone: without the second contigs of CC.TWO_CONTIGS it is not raised
    p2 = CC.without_second_contigs(p)
    raw2 = V.call(sites, list(p2.names), CC.steps_of(p2), sq, [ref])
    assert [r["id"] for r in raw2] == [r["id"] for r in raw]
    assert {r["id"] for r, r2 in zip(raw, raw2) if r["tangled"] and not r2["tangled"]} == LATE_TANGLED
    assert sum(not r["tangled"] for r in raw) == 8
    # no call in a sample past lane 63: the ambiguous one-slot sample 69, and the haplotype that ends in the middle of the chain
    missing = [{s for s in range(64, 131) if r["gt"][s] == "."} for r in raw]
    assert sum(bool(m) for m in missing) == 7 and {69} in missing and {CC.CUT_SAMPLE} in missing
    assert all((r["ns"] != 131) == bool(m) for r, m in zip(raw, missing))


@pytest.mark.parametrize("ref, all_late, both", [(CC.REF_LOW, 5, 20), (CC.REF_HIGH, 2, 23)])
def test_inversions(ref, all_late, both):
    g, p, names, steps, sq, sites = cohort()
    sample_of = CC.sample_of_slots(names)
    inv, stats = inversions(ref)
    assert len(inv) >= 32 and stats["max_opposite"] >= 65
    sides = [late(sample_of, r["slots"], 1) for r in inv]
    assert sum(s == {True} for s in sides) == all_late and sum(s == {False, True} for s in sides) == both
    assert sum(CC.restricted_differs(r["slots"], sample_of, 64, r["ac"], r["an"], r["ns"]) for r in inv) >= all_late + both
    assert len(sample_of) - 1 > 256  # the slot key of the sort has nine bits


@pytest.mark.parametrize("ref, groups", [(CC.REF_LOW, 4), (CC.REF_HIGH, 1)])
def test_decomposed_and_merged(ref, groups):
    g, p, names, steps, sq, sites = cohort()
    samples, slot, sample_of = V.slots_of(names)
    raw = I.merge([dict(r) for r in plain(ref)], [dict(r) for r in inversions(ref)[0]])
    rows, counters = PR.decompose(raw, names, steps, sq)
    assert counters["n_decomposed_alts"] >= 17 and counters["n_passthrough_alts"] >= 37
    cut = [dict(r, slots=[v if sample_of[sl] < 64 else None for sl, v in enumerate(r["slots"])]) for r in raw]
    differ = []
    for row in rows:
        _, _, ac, an, ns = PR.project(cut[row["rec"]]["slots"], row["alt"], sample_of, len(samples))
        differ.append((ac, an, ns) != (row["ac"], row["an"], row["ns"]))
    # (a row that stays is one of an inversion record with the reference and every supporter below 64)
    assert len(rows) >= 59 and sum(differ) >= 52 and all(d for d, row in zip(differ, rows) if raw[row["rec"]]["vartype"] != "SUBR")
    merged, c = MR.merge(raw, rows, names)
    merged64, c64 = MR.merge(cut, rows, names)
    assert [m["members"] for m in merged64] == [m["members"] for m in merged]
    wide = [k for k, m in enumerate(merged) if len(m["members"]) >= 2]
    assert len(wide) == groups == c["n_merged_groups"]
    assert all((merged[k]["ac"], merged[k]["an"], merged[k]["ns"]) != (merged64[k]["ac"], merged64[k]["an"], merged64[k]["ns"]) for k in wide)
    # the wide chain yields reference-consistent slots (and no conflict): their count is another under the restriction
    assert c["n_ref_consistent"] >= 100 and c["n_gt_conflicts"] == 0 and 0 < c64["n_ref_consistent"] < c["n_ref_consistent"]


@pytest.mark.parametrize("ref, compared", [(CC.REF_LOW, 28), (CC.REF_HIGH, 26)])
def test_left_normalized(ref, compared):
    """Nothing moves in the wide chain; one record has two ALTs that both read as REF does (x and y are empty segments), which
    stays as it is and still counts REF's length for each ALT."""
    g, p, names, steps, sq, sites = cohort()
    want, counters = NR.normalise(plain(ref), steps, sq)
    same = [r for r in want if {a.upper() for a in r["alts"]} == {r["ref"].upper()}]
    assert len(same) == 1 and len(same[0]["ref"]) == 1 and not same[0]["normalized"]
    assert counters == dict(n_normalized=0, max_shift=0, n_norm_compared=compared)
    assert [r["slots"] for r in want] == [r["slots"] for r in plain(ref)]


def test_off_reference():
    g, p, names, steps, sq, sites = cohort()
    sample_of = CC.sample_of_slots(names)
    want, counts = F.call(sites, names, steps, sq, [CC.REF_PARTIAL])
    assert counts["n_offref_sites"] == counts["n_offref_records"] == 6
    off = [r for r in want if r["offref"]]
    assert len(want) - len(off) == 6  # the sites the partial reference still crosses
    assert all(sum(v is not None for v in r["slots"]) >= 258 for r in off)  # the surrogate is one of more than 64 paths
    assert all(CC.restricted_differs(r["slots"], sample_of, 64, r["ac"], r["an"], r["ns"]) for r in want)


@pytest.mark.parametrize("ref", CC.REFS)
def test_vcf_of_the_call(ref):
    g, p, names, steps, sq, sites = cohort()
    doc = R.parse(V.vcf_text(names, steps, sq, plain(ref), [ref]))
    assert len(doc["samples"]) == 131 and min(len(r["tasks"]) for r in doc["records"]) >= 258 > 128
    res = R.check(doc, names, steps, set(sq), sq, spelling=True)
    assert res["n_invalid"] == 0 and res["n_misspelled"] == 0 and res["n_status"][R.FOUND_REV] >= 700


# ---- the VCF checks past 64 (the builders of tests/test_gpu_vcfcheck.py)

def clean_text(ref):
    g, p, names, steps, sq, sites = cohort()
    return V.vcf_text(names, steps, sq, plain(ref), [ref])


@pytest.mark.parametrize("ref", CC.REFS)
def test_first_failures_in_later_batches(ref):
    g, p, names, steps, sq, sites = cohort()
    cases = TV.late_failures(clean_text(ref), names, steps, set(sq))
    for what, bad, r, (reason, allele, at) in cases:
        doc = R.parse(bad)
        res = R.check(doc, names, steps, set(sq), sq, spelling=True)
        off = sum(len(x["tasks"]) for x in doc["records"][:r])
        assert (res["rec_reason"][r], res["rec_allele"][r], res["rec_task"][r]) == (reason, allele, R.NIL if at is None else off + at), what
        assert res["rec_invalid"] == [int(k == r) for k in range(12)], what
    (_, _, _, (_, _, second)), (_, _, _, (_, _, third)), (_, bad1, r1, (_, _, at1)), (_, bad0, r0, _) = cases
    assert 64 <= second < 128 <= third and 64 <= at1 < 128
    # the third case has allele 1 misspelled and a failing task of allele 0, the fourth allele 0 misspelled and the same task
    for bad, r, which in ((bad1, r1, 1), (bad0, r0, 0)):
        doc = R.parse(bad)
        res = R.check(doc, names, steps, set(sq), sq, spelling=True)
        first = sum(len(x["alleles"]) for x in doc["records"][:r])
        assert [a - first for a, s in enumerate(res["allele_spell"]) if s == R.SPELL_MISSPELLED] == [which]
        off = sum(len(x["tasks"]) for x in doc["records"][:r])
        failing = [t - off for t, s in enumerate(res["task_status"]) if s > R.FOUND_REV]
        assert failing == [at1] and doc["records"][r]["tasks"][at1][0] == 0


@pytest.mark.parametrize("misspelled", [(66,), (3, 66)])
def test_more_than_64_alleles_in_a_record(misspelled):
    names, steps, sq, text = TV.many_alleles_case(misspelled)
    doc = R.parse(text)
    res = R.check(doc, names, steps, set(sq), sq, spelling=True)
    assert len(doc["records"]) == 1 and len(doc["records"][0]["alleles"]) == 71
    assert [a for a, s in enumerate(res["allele_spell"]) if s == R.SPELL_MISSPELLED] == list(misspelled) and max(misspelled) >= 64
    assert (res["rec_reason"], res["rec_allele"], res["task_status"]) == ([R.MISSPELLED], [misspelled[0]], [R.FOUND_FWD])


def test_long_segments_in_the_spelling():
    names, steps, seqs, text, expected = TV.long_segments_case()
    assert [len(s) for s in seqs] == [2, 64, 65, 130, 200, 130, 130, 130] and [s.find("Q") for s in seqs[5:]] == [70, 129, 0]
    doc = R.parse(text)
    res = R.check(doc, names, steps, set(range(1, 9)), dict(enumerate(seqs, 1)), spelling=True)
    assert res["allele_spell"] == expected
    assert (expected.count(R.SPELL_WHOLE), expected.count(R.SPELL_ANCHORED), expected.count(R.SPELL_MISSPELLED)) == (9, 10, 44)
    # a wrong base at oriented index 63, 64, 129 and at the last index of every segment that has it, in either orientation
    walks = [(al["walk"], al["text"]) for rec in doc["records"] for al in rec["alleles"]]
    sq = dict(enumerate(seqs, 1))
    at = {(w[-1], len(w), next(i for i, (a, b) in enumerate(zip(t[len(w) - 1:], R._oriented(w[-1], sq))) if a != b))
          for (w, t), e in zip(walks, expected) if e == R.SPELL_MISSPELLED and w[0][0] <= 5}
    assert at == {((x, o), m, i) for x, n in zip(range(2, 6), TV.LONG) for o in (0, 1) for m in (1, 2) for i in (63, 64, 129, n - 1) if i < n}


def test_tier_edges():
    names, steps, recs, expected = TV.tier_edges_case()
    sq = {i: "A" for i in range(1, 201)}
    doc = R.parse(TV.vcf_of([n.split("#")[0] for n in names], recs, sq))
    assert R.check(doc, names, steps, set(sq))["task_status"] == expected
    count = {}
    for p in steps:
        for x in p:
            count[x] = count.get(x, 0) + 1
    edges = {rec["id"]: (len(rec["alleles"][0]["walk"]), count[rec["alleles"][0]["walk"][0]] if rec["id"] != "lateb" else count[(15, 0)]) for rec in doc["records"]}
    assert edges == dict(w64=(64, 1), w64x=(64, 1), w65=(65, 1), w65x=(65, 1), a64=(2, 64), a64x=(2, 64), a65=(2, 65), a65x=(2, 65),
                         late=(72, 66), latex=(72, 66), lateb=(72, 66), many=(2, 141))
    assert TV.n_searches(doc, steps, set(sq), False, False) == TV.TIER_EDGES_TIER2 == 13 and TV.n_searches(doc, steps, set(sq), False, True) == 24
    # found only at the last occurrence of the anchor: (15, 0) in `late`, (11, 0) over three paths of three slots
    assert steps[3].index((20, 0)) - 1 == max(i for i, x in enumerate(steps[3]) if x == (15, 0))
    assert [p.count((11, 0)) for p in steps[4:]] == [50, 50, 41] and steps[6][-2:] == [(11, 0), (13, 0)] and all((13, 0) not in p for p in steps[4:6])


def test_documents_beyond_the_capped_grids():
    names, steps, sq, text = TV.capped_records_case()
    doc = R.parse(text)
    res = R.check(doc, names, steps, set(sq), sq, spelling=True)
    assert len(doc["records"]) == 8300 > TV.CAP_WAVES and len(res["allele_spell"]) == 16600
    assert [r for r, bad in enumerate(res["rec_invalid"]) if bad] == [8250, 8260] and min(8250, 8260) >= TV.CAP_WAVES
    assert [a for a, s in enumerate(res["allele_spell"]) if s == R.SPELL_MISSPELLED] == [2 * 8260 + 1]
    assert (res["rec_reason"][8250], res["rec_reason"][8260], res["n_invalid"], res["n_misspelled"]) == (R.ABSENT, R.MISSPELLED, 2, 1)
    # the tasks: just over the cap, the one failing task behind it; the restatement of one copy repeated by numpy is the
    # restatement of the whole document
    g, p, names, steps, sq, sites = cohort()
    head, block, last = TV.capped_tasks_case(clean_text(CC.REF_LOW), names, steps, set(sq))
    doc = R.parse("\n".join(head + block * 167 + last) + "\n")
    res = R.check(doc, names, steps, set(sq))
    tiled_doc, tiled = TV.restated_copies(head, block, last, 168, names, steps, set(sq))
    assert tiled_doc == doc and tiled == res
    n_tasks = len(res["task_status"])
    assert len(doc["records"]) == 2016 and TV.CAP_LANES < n_tasks < TV.CAP_LANES + 261  # (just over: less than a record more)
    assert [t for t, s in enumerate(res["task_status"]) if s > R.FOUND_REV] == [res["rec_task"][2015]] and res["rec_task"][2015] >= TV.CAP_LANES
    assert res["rec_task"][2015] - (n_tasks - len(doc["records"][2015]["tasks"])) >= 128
