"""Plain-Python restatement of the VCF comparison ("VCF comparison"), the yardstick of the reader's CHROM
table, of povu_hip_vcf_compare, povu_hip_vcf_cmp_text and of `povu vcf --compare`.

`parse` is the document of vcfcheck_ref.parse with every record's CHROM, `compare` gives every (record, ALT) item its state, its
trimmed key and its group, every group its class and every common sample its cells; `compare_text` / `summary_text` are the two
files.  Everything is written the slow, obvious way: strings, dictionaries, loops.
"""
from __future__ import annotations

import string

import vcfcheck_ref as R

KEYED, SKIPPED = 0, 1
SHARED, ONLY_A, ONLY_B = 0, 1, 2
NIL = 0xFFFFFFFF
TIER1_BYTES = 32  # the shorter text a lane per item still takes (DESIGN.md "VCF comparison")
_FOLD = str.maketrans(string.ascii_lowercase, string.ascii_uppercase)


def parse(text: str) -> dict:
    """vcfcheck_ref.parse, and per record `chrom`; `chroms`: the distinct CHROM strings in order of first appearance."""
    doc = R.parse(text)
    lines = [ln[:-1] if ln.endswith("\r") else ln for ln in text.split("\n")]
    chrom = [ln.split("\t")[0] for ln in lines if ln and not ln.startswith("#")]
    assert len(chrom) == len(doc["records"])
    doc["chroms"] = []
    for rec, c in zip(doc["records"], chrom):
        rec["chrom"] = c
        if c not in doc["chroms"]:
            doc["chroms"].append(c)
    return doc


def rec_chrom(doc: dict):
    return [doc["chroms"].index(rec["chrom"]) for rec in doc["records"]]


def skipped(ref: str, alt: str) -> bool:
    return alt == "*" or alt.startswith("<") or "[" in alt or "]" in alt or ref in ("", ".")


def trim(pos: int, ref: str, alt: str):
    """(POS', REF', ALT', bytes taken at the end, bytes taken at the front): folded, the suffix first."""
    ref, alt = ref.translate(_FOLD), alt.translate(_FOLD)
    s = p = 0
    while len(ref) >= 2 and len(alt) >= 2 and ref[-1] == alt[-1]:
        ref, alt, s = ref[:-1], alt[:-1], s + 1
    while len(ref) >= 2 and len(alt) >= 2 and ref[0] == alt[0]:
        ref, alt, p = ref[1:], alt[1:], p + 1
    return pos + p, ref, alt, s, p


def items_of(doc: dict):
    """One item per (record, ALT k >= 1) in document order."""
    out = []
    for r, rec in enumerate(doc["records"]):
        texts = [al["text"] for al in rec["alleles"] if al["text"] is not None]
        for k in range(1, len(texts)):
            it = dict(record=r, alt=k, ref=texts[0], text=texts[k], state=KEYED, pos=0, suffix=0, prefix=0, group=NIL, key=None)
            if skipped(texts[0], texts[k]):
                it["state"] = SKIPPED
            else:
                pos, ref, alt, it["suffix"], it["prefix"] = trim(rec["pos"], texts[0], texts[k])
                it["pos"], it["key"] = pos, (rec["chrom"], pos, ref, alt)
            out.append(it)
    return out


def dose(doc: dict, item: dict, col: int) -> int:
    """GT entries of column `col` in the item's record that name the item's ALT."""
    return sum(1 for a, c, _ in doc["records"][item["record"]]["tasks"] if a == item["alt"] and c == col)


def compare(doc_a: dict, doc_b: dict, force_tier2: bool = False) -> dict:
    ia, ib = items_of(doc_a), items_of(doc_b)
    # groups, numbered in the order of their first items: A's, then B's
    group_of, groups = {}, []
    for side, items in ((0, ia), (1, ib)):
        for i, it in enumerate(items):
            if it["state"] == SKIPPED:
                continue
            g = group_of.setdefault(it["key"], len(groups))
            if g == len(groups):
                groups.append(dict(key=it["key"], members=([], []), first=i + (len(ia) if side else 0)))
            groups[g]["members"][side].append(i)
            it["group"] = g
    for g in groups:
        na, nb = len(g["members"][0]), len(g["members"][1])
        g["n_a"], g["n_b"], g["cls"] = na, nb, SHARED if na and nb else ONLY_A if na else ONLY_B
    # sample columns by name: of several columns of one name on a side the first counts
    sa, sb = doc_a["samples"], doc_b["samples"]
    samples, taken = [], set()
    for c, name in enumerate(sa):
        if name in sb and name not in taken:
            taken.add(name)
            samples.append(dict(name=name, col_a=c, col_b=sb.index(name), tp=0, fp=0, fn=0, gteq=0))
    for g in groups:
        for s in samples:
            da = sum(dose(doc_a, ia[i], s["col_a"]) for i in g["members"][0])
            db = sum(dose(doc_b, ib[i], s["col_b"]) for i in g["members"][1])
            s["tp"] += da > 0 and db > 0
            s["fp"] += da > 0 and db == 0
            s["fn"] += da == 0 and db > 0
            s["gteq"] += da > 0 and da == db
    n_tier2 = sum(1 for it in ia + ib if force_tier2 or min(len(it["ref"]), len(it["text"])) > TIER1_BYTES)
    return dict(items_a=ia, items_b=ib, groups=groups, samples=samples,
                n_shared=sum(g["cls"] == SHARED for g in groups), n_only_a=sum(g["cls"] == ONLY_A for g in groups),
                n_only_b=sum(g["cls"] == ONLY_B for g in groups),
                n_skipped_a=sum(it["state"] == SKIPPED for it in ia), n_skipped_b=sum(it["state"] == SKIPPED for it in ib),
                n_items_a=len(ia), n_items_b=len(ib), n_common_samples=len(samples),
                n_samples_only_a=len(sa) - len(samples), n_samples_only_b=len(sb) - len(samples), n_tier2=n_tier2)


def totals(res: dict):
    return tuple(sum(s[k] for s in res["samples"]) for k in ("tp", "fp", "fn", "gteq"))


def compare_text(doc_a: dict, doc_b: dict, res: dict) -> str:
    out = ["side\tCHROM\tPOS\tREF\tALT\trec_idx\tID\tn\n"]
    for g in res["groups"]:
        if g["cls"] == SHARED:
            continue
        b = g["cls"] == ONLY_B
        it = (res["items_b"] if b else res["items_a"])[g["members"][b][0]]
        rec = (doc_b if b else doc_a)["records"][it["record"]]
        chrom, pos, ref, alt = g["key"]
        out.append(f"{'B' if b else 'A'}\t{chrom}\t{pos}\t{ref}\t{alt}\t{it['record']}\t{rec['id']}\t{g['n_a'] + g['n_b']}\n")
    return "".join(out)


def _ratio(num: int, den: int) -> str:
    return "nan" if not den else "%.4f" % (num / den)


def _rates(both: int, only_a: int, only_b: int) -> str:
    return (f"precision {_ratio(both, both + only_a)}, recall {_ratio(both, both + only_b)}, "
            f"F1 {_ratio(2 * both, 2 * both + only_a + only_b)}")


def summary_text(res: dict) -> str:
    tp, fp, fn, gteq = totals(res)
    out = [f"Alleles: shared {res['n_shared']}, only A {res['n_only_a']}, only B {res['n_only_b']}\n",
           f"Alleles: {_rates(res['n_shared'], res['n_only_a'], res['n_only_b'])}\n",
           f"Genotypes: tp {tp}, fp {fp}, fn {fn}, gteq {gteq}\n", f"Genotypes: {_rates(tp, fp, fn)}\n"]
    for s in res["samples"]:
        out.append(f"Sample {s['name']}: tp {s['tp']}, fp {s['fp']}, fn {s['fn']}, gteq {s['gteq']}\n")
    if res["n_skipped_a"] or res["n_skipped_b"]:
        out.append(f"Skipped alleles: A {res['n_skipped_a']}, B {res['n_skipped_b']}\n")
    if res["n_samples_only_a"] or res["n_samples_only_b"]:
        out.append(f"Unmatched sample columns: A {res['n_samples_only_a']}, B {res['n_samples_only_b']}\n")
    return "".join(out)
