"""The plain-Python restatement of the decomposed calls (tests/prim_ref.py): its table against an edit distance computed a
second way and against the anti-diagonal fill, its canonical alignment (the primitives applied to REF give ALT, no insertion
next to a deletion, gaps leftmost), what may be stripped before the table is filled and what may not, the rows of the
reference's vcfwave-complex-decomposition and subr-inversion-preservation fixtures
(tests/golden/reference_decomposed_records.json), the differential workload's floors, and the Python constants.  No GPU."""
import json
import os
import random
from functools import lru_cache

import pytest

import inversions_ref as I
import oracle_lib as O
import prim_ref as PR
import vcf_ref as V
from povu_amd import hip as H
from povu_amd import workloads as W
from test_norm_ref import _graph

VCFWAVE = "downstream_repetitive/vcfwave-complex-decomposition"
SUBR = "downstream_repetitive/subr-inversion-preservation"


def two_row_distance(a: str, b: str) -> int:
    a, b = a.upper(), b.upper()
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def memo_distance(a: str, b: str) -> int:
    a, b = a.upper(), b.upper()

    @lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j - 1) + (a[i - 1] != b[j - 1]), d(i - 1, j) + 1, d(i, j - 1) + 1)
    return d(len(a), len(b))


def random_pairs(n, seed, max_len=14):
    rng = random.Random(seed)
    for _ in range(n):
        a = "".join(rng.choice("AC") if rng.random() < .6 else rng.choice("ACGTacgt") for _ in range(rng.randint(0, max_len)))
        b = list(a)
        for _ in range(rng.randint(0, 4)):
            r, p = rng.random(), rng.randint(0, len(b))
            if r < .4 and p < len(b):
                b[p] = rng.choice("ACGT")
            elif r < .7:
                b[p:p] = [rng.choice("ACGT") for _ in range(rng.randint(1, 3))]
            else:
                del b[p:p + rng.randint(1, 3)]
        yield a, "".join(b)


def test_hand_alignments():
    assert PR.traceback("CGT", "TGA") == "XMX"
    assert PR.primitives("CGT", "TGA") == [(PR.ROW_SNP, 0, 0, 1, 1), (PR.ROW_SNP, 2, 2, 1, 1)]
    assert PR.traceback("CGT", "CGTACGTACGTA") == "I" * 8 + "MMMI"  # (the diagonal first from the far corner: gaps go left)
    assert PR.traceback("GAA", "G") == "MDD" and PR.traceback("GAA", "GA") == "MDM"  # gaps as far left as the optimum allows
    assert PR.traceback("AA", "A") == "DM" and PR.primitives("AA", "A") == [(PR.ROW_DEL, 0, 0, 1, 0)]
    assert PR.traceback("AC", "CA") == "XX"  # adjacent mismatches stay two SNPs
    assert PR.traceback("acgt", "ACGT") == "MMMM" and PR.primitives("acgt", "ACGT") == []
    assert PR.traceback("", "AC") == "II" and PR.traceback("AC", "") == "DD"


def test_cost_alignment_and_fill_order_on_random_pairs():
    adjacent = multi = lead = 0
    for a, b in random_pairs(4000, 20261018):
        D = PR.table(a, b)
        assert D[len(a)][len(b)] == two_row_distance(a, b) == memo_distance(a, b)
        assert PR.table_by_antidiagonals(a, b) == D
        ops = PR.traceback(a, b, D)
        prims = PR.primitives(a, b, ops)
        assert PR.apply(a, b, prims) == "".join(a[i] if o == "M" else b[j] for o, i, j in _columns(ops) if o != "D")
        assert PR.apply(a, b, prims).upper() == b.upper()
        assert sum(1 if k == PR.ROW_SNP else la + lb for k, _i, _j, la, lb in prims) == D[len(a)][len(b)]
        adjacent += "ID" in ops or "DI" in ops
        multi += len(prims) > 1
        lead += bool(prims) and prims[0][0] != PR.ROW_SNP and prims[0][1] == 0
    assert adjacent == 0
    assert multi >= 1000 and lead >= 400  # (what the definition calls common is common here)


def _columns(ops):
    i = j = 0
    for o in ops:
        yield o, i, j
        i += o != "I"
        j += o != "D"


def test_suffix_strip_changes_nothing_prefix_strip_would():
    for a, b in random_pairs(2000, 7):
        n = 0
        while n < len(a) and n < len(b) and a[len(a) - 1 - n].upper() == b[len(b) - 1 - n].upper():
            n += 1
        assert PR.traceback(a[:len(a) - n], b[:len(b) - n]) + "M" * n == PR.traceback(a, b)
    # a common first base is not always a match column: the leftmost gap deletes it
    assert PR.traceback("AA", "A") == "DM" and "M" + PR.traceback("A", "") == "MD"


def test_rows_of_a_pair():
    rows, cells = PR.pair_rows("CGT", "TGA", 2, "A", 8)
    assert cells == 16 and [(r["kind"], r["index"], r["pos"], r["ref_start"], r["alt_start"], r["lead"]) for r in rows] == [
        (PR.ROW_SNP, 1, 2, 0, 0, ""), (PR.ROW_SNP, 2, 4, 2, 2, "")]
    # an indel inside the allele is anchored on the REF base in front of it, one at offset 0 on the context base
    (row,), _ = PR.pair_rows("GAA", "G", 5, "TTTT", 8)
    assert (row["kind"], row["pos"]) + PR.row_texts(row, "GAA", "G") == (PR.ROW_DEL, 5, "GAA", "G")
    (row,), _ = PR.pair_rows("AA", "A", 5, "TTTC", 8)
    assert (row["kind"], row["pos"], row["lead"]) + PR.row_texts(row, "AA", "A") == (PR.ROW_DEL, 4, "C", "CA", "C")
    (row,), _ = PR.pair_rows("A", "TTA", 3, "Gc", 8)
    assert (row["kind"], row["pos"]) + PR.row_texts(row, "A", "TTA") == (PR.ROW_INS, 2, "c", "cTT")
    # kept whole, and why
    for args, reason, cells in ((("AA", "A", 1, "", 8), PR.REASON_CONTIG_START, 6), (("", "A", 4, "CCC", 8), PR.REASON_EMPTY_ALLELE, 0),
                                (("AC", "", 4, "CCC", 8), PR.REASON_EMPTY_ALLELE, 0), (("ACGTACGTA", "A", 4, "CCC", 8), PR.REASON_MAX_ALLELE_LENGTH, 0),
                                (("A", "ACGTACGTA", 4, "CCC", 8), PR.REASON_MAX_ALLELE_LENGTH, 0), (("acgt", "ACGT", 4, "CCC", 8), PR.REASON_EQUALS_REF, 25),
                                (("ACGTACGT", "ACGTACGA", 4, "CCC", 8), PR.REASON_NONE, 81)):
        rows, got_cells = PR.pair_rows(*args)
        assert (rows[0]["reason"], got_cells) == (reason, cells), args
        assert (rows[0]["kind"] == PR.ROW_PASS) == (reason != PR.REASON_NONE) and len(rows) == 1
    rows, _ = PR.pair_rows("AC", "TG", 9, "", 8, subr=True)
    assert rows[0]["reason"] == PR.REASON_SUBR
    # a SNP at POS 1 needs no anchor
    assert PR.pair_rows("A", "C", 1, "", 8)[0][0]["kind"] == PR.ROW_SNP
    with pytest.raises(V.CallError):
        PR.decompose([], [], [], {}, max_allele_length=PR.MAX_LENGTH + 1)


def test_projection():
    got, gt, ac, an, ns = PR.project([0, 1, 2, None, 2, 0], 2, [0, 0, 1, 1, 2, 3], 4)
    assert got == [0, None, 1, None, 1, 0] and gt == ["0|.", "1|.", "1", "0"] and (ac, an, ns) == (2, 4, 4)
    got, gt, ac, an, ns = PR.project([0, 1, None], 2, [0, 1, 2], 3)
    assert gt == ["0", ".", "."] and (ac, an, ns) == (0, 1, 1)


def test_vcfwave_fixture_rows(golden_dir, tmp_path):
    """What the fixture pins (INTEGRATION.md "Decomposed calls"): with max_allele_length 8 the first ALT is two SNPs two
    bases apart, the second is kept whole; IDs, REF / ALT of the SNPs, the projected genotypes and counts, the INFO keys and
    their order, and the header lines are the fixture's.  AT (not cut per step), POS (this project's SUB record has no leading
    anchor base) and the second ALT's text (the fixture's does not spell its own GFA) are this project's."""
    want = json.load(open(os.path.join(golden_dir, "reference_decomposed_records.json")))["fixtures"][VCFWAVE]
    (names, paths, seqs), texts = _graph(golden_dir, tmp_path, VCFWAVE)
    raw = V.call(V.sites_of_pvst(texts), names, paths, seqs, [want["reference_prefix"]])
    assert [(r["pos"], r["ref"], r["alts"]) for r in raw] == [(2, "CGT", ["TGA", "CGTACGTACGTA"])]
    rows, counters = PR.decompose(raw, names, paths, seqs, max_allele_length=8)
    assert counters == dict(n_rows=3, n_decomposed_alts=1, n_passthrough_alts=1, n_prim_tier2=0, n_prim_cells=16)
    lines = [PR.row_line(row, raw[row["rec"]], V.record_line).split("\t") for row in rows]
    by_id = {f[2]: f for f in lines}
    assert sorted(by_id) == sorted(w["id"] for w in want["rows"]) == [">9>14:1:snp1", ">9>14:1:snp2", ">9>14:2:passthrough"]
    for w in want["rows"]:
        f = by_id[w["id"]]
        info = dict(kv.split("=", 1) for kv in f[7].split(";"))
        assert [kv.split("=", 1)[0] for kv in f[7].split(";")] == w["info_keys_in_order"]
        assert f[0] == w["chrom"] and f[9:] == w["gt"] and (info["AC"], info["AN"], info["NS"]) == ("1", "2", "2")
        for k in ("AC", "AF", "AN", "NS", "VARTYPE", "ORIGIN", "RAW_ALT_INDEX", "PROFILE", "DECOMPOSED", "PASSTHROUGH", "PASS_THROUGH_REASON"):
            assert info.get(k) == w["info"].get(k), (w["id"], k)
        assert int(f[1]) - int(info["RAW_POS"]) == w["pos"] - int(w["info"]["RAW_POS"]) - (0 if "passthrough" in w["id"] else 1)
        if "snp" in w["id"]:
            assert (f[3], f[4], info["TANGLED"]) == (w["ref"], w["alt"], w["info"]["TANGLED"])
    assert (by_id[">9>14:1:snp1"][3:5], by_id[">9>14:1:snp2"][3:5]) == (["C", "T"], ["T", "A"])
    assert int(by_id[">9>14:1:snp2"][1]) - int(by_id[">9>14:1:snp1"][1]) == 2
    assert (by_id[">9>14:1:snp1"][9:], by_id[">9>14:2:passthrough"][9:]) == (["0", "1", "."], ["0", ".", "1"])
    assert "PASS_THROUGH_REASON=max_allele_length;RAW_POS=2;RAW_REF=CGT;RAW_ALT=CGTACGTACGTA" in by_id[">9>14:2:passthrough"][7]
    # rows in (POS, record, ALT, alignment order): the whole ALT at the record's POS comes after the SNP there
    assert [f[2] for f in lines] == [">9>14:1:snp1", ">9>14:2:passthrough", ">9>14:1:snp2"]
    text = PR.vcf_text(names, paths, seqs, raw, rows, ["HG1"])
    for k, d in want["info_lines"].items():
        if k in dict((x[0], 1) for x in PR._DESC):
            assert text.count(f'##INFO=<ID={k},Number={d["number"]},Type={d["type"]},Description="{d["description"]}">\n') == 1, k
    head = text.splitlines()
    assert head[len(V.HEADER.splitlines())].startswith("##INFO=<ID=ORIGIN,")  # where the other profiles' lines go
    # under the ceiling the second ALT is two insertions: eight bases in front of REF (anchored on the base in front of POS)
    # and one behind its last base
    rows, counters = PR.decompose(raw, names, paths, seqs)
    assert [(r["alt"], r["kind"], r["index"], r["pos"]) for r in rows] == [
        (2, PR.ROW_INS, 1, 1), (1, PR.ROW_SNP, 1, 2), (1, PR.ROW_SNP, 2, 4), (2, PR.ROW_INS, 2, 4)]
    assert PR.row_texts(rows[0], "CGT", "CGTACGTACGTA") == ("A", "ACGTACGTA") and PR.row_texts(rows[3], "CGT", "CGTACGTACGTA") == ("T", "TA")
    assert counters == dict(n_rows=4, n_decomposed_alts=2, n_passthrough_alts=0, n_prim_tier2=0, n_prim_cells=16 + 4 * 13)


def test_subr_fixture_passes_through(golden_dir, tmp_path):
    want = json.load(open(os.path.join(golden_dir, "reference_decomposed_records.json")))["fixtures"][SUBR]
    (names, paths, seqs), texts = _graph(golden_dir, tmp_path, SUBR)
    raw = I.call(V.sites_of_pvst(texts), names, paths, seqs, [want["reference_prefix"]])
    subr = [r for r in raw if r["vartype"] == "SUBR"]
    assert len(subr) == 1
    rows, counters = PR.decompose(raw, names, paths, seqs)
    line = next(PR.row_line(row, raw[row["rec"]], I.record_line) for row in rows if row["reason"] == PR.REASON_SUBR).split("\t")
    (w,) = want["rows"]
    assert line[:7] == [w["chrom"], str(w["pos"]), w["id"], w["ref"], w["alt"], "60", "PASS"] and line[9:] == w["gt"]
    assert line[7] == ";".join(f"{k}={w['info'][k]}" for k in w["info_keys_in_order"])
    text = PR.vcf_text(names, paths, seqs, raw, rows, ["ref"], raw_line=I.record_line)
    d = want["info_lines"]["SUBR_ORIGIN"]
    assert text.count(f'##INFO=<ID=SUBR_ORIGIN,Number={d["number"]},Type={d["type"]},Description="{d["description"]}">\n') == 1


def test_unchanged_record_is_the_raw_line():
    # one ALT, one primitive that spells the raw POS, REF and ALT: a SNP, an anchored deletion, an anchored insertion
    names = ["R#1#c", "A#1#c"]
    recs = [dict(path=0, q=0, first=1, chrom="R#1#c", pos=p, id=f">{p}>{p + 2}", ref=ref, alts=[alt], at=[">1", ">2"], vartype=vt, tangled=False,
                 lv=0, gt=["0", "1"], slots=[0, 1], ac=[1], an=2, ns=2)
            for p, ref, alt, vt in ((3, "A", "C", "SUB"), (6, "GAA", "G", "DEL"), (11, "G", "GTT", "INS"), (15, "GA", "gT", "SUB"), (20, "gA", "G", "DEL"))]
    seqs = {1: "ACGTACGTACGTACGTACGTACGT"}
    rows, counters = PR.decompose(recs, names, [[(1, 0)], [(1, 0)]], seqs)
    assert [r["kind"] for r in rows] == [PR.ROW_RAW, PR.ROW_RAW, PR.ROW_RAW, PR.ROW_SNP, PR.ROW_DEL]  # (lower case: the texts differ)
    assert counters["n_decomposed_alts"] == 2 and counters["n_passthrough_alts"] == 0
    assert [PR.row_line(row, recs[row["rec"]], V.record_line) for row in rows[:3]] == [V.record_line(r) for r in recs[:3]]
    assert PR.row_line(rows[4], recs[4], V.record_line).split("\t")[1:5] == ["20", ">20>22:1:del1", "gA", "g"]


# complex_alleles(300, seed) with complex_haplotypes(300, seed, 6), reference hap0, max_allele_length 10, on the restatement
# alone (the floors a GPU test of the device step can rely on):
#   seed  records  rows  raw / snp / ins / del / pass   max_allele_length / contig_start / empty_allele / equals_ref   aligned  multi
#   1     296      935   4 / 292 / 245 / 251 / 143      85 / 2 / 10 / 46                                                459      253
#   2     297      962   1 / 297 / 250 / 282 / 132      78 / 1 / 14 / 39                                                482      260
#   3     294      1008  5 / 328 / 299 / 256 / 120      84 / 2 / 7 / 27                                                 493      285
COMPLEX_CAP = 10


def complex_case(seed, units=300, haps=6):
    g, seqs = W.complex_alleles(units, seed)
    p = W.complex_haplotypes(units, seed, haps)
    return g, seqs, p


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_complex_alleles_floors(seed):
    g, seqs, p = complex_case(seed)
    names, paths = list(p.names), [p.steps(i) for i in range(len(p))]
    sq = dict(zip(g.vid.tolist(), seqs))
    sites = V.sites_of_pvst(list(O.decompose(g).values()))
    raw = V.call(sites, names, paths, sq, ["hap0"])
    rows, counters = PR.decompose(raw, names, paths, sq, max_allele_length=COMPLEX_CAP)
    kinds = {k: sum(r["kind"] == k for r in rows) for k in range(5)}
    reasons = {k: sum(r["reason"] == k for r in rows) for k in range(1, 5)}
    aligned = multi = 0
    for r in raw:
        for alt in r["alts"]:
            got, cells = PR.pair_rows(r["ref"], alt, r["pos"], "N" * r["pos"], COMPLEX_CAP)
            aligned += cells > 0
            multi += len(got) > 1
    print(seed, len(raw), len(rows), kinds, reasons, aligned, multi)
    assert all(kinds.values()) and all(reasons.values()), (kinds, reasons)
    assert 2 * multi >= aligned, (multi, aligned)
    assert any(len(r["alts"]) >= 3 for r in raw) and counters["n_prim_cells"] > 0


def test_python_constants():
    assert H.PROFILES["decomposed"] == 4 and H.PRIM_MAX_LENGTH == PR.MAX_LENGTH == 512
    assert (H.ROW_RAW, H.ROW_SNP, H.ROW_INS, H.ROW_DEL, H.ROW_PASS) == (PR.ROW_RAW, PR.ROW_SNP, PR.ROW_INS, PR.ROW_DEL, PR.ROW_PASS)
    assert (H.REASON_MAX_ALLELE_LENGTH, H.REASON_CONTIG_START, H.REASON_EMPTY_ALLELE, H.REASON_EQUALS_REF, H.REASON_SUBR) == (1, 2, 3, 4, 5)
