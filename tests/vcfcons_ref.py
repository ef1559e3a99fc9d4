"""Plain-Python restatement of the consensus haplotypes ("Consensus haplotypes"), the yardstick of
povu_hip_vcf_consensus, povu_hip_vcf_cons_text and of `povu vcf --consensus`.

`consensus` takes one document of vcfcmp_ref.parse, the path names in resident order and the bases of every path by name (of
several paths of one name the first counts).  It gives every (CHROM, column, phase) with a task on a placed record of that CHROM
its applied edits in order, what the three drop rules take away, its text, and with `roundtrip` the verdict against the one path
of its slot.  `fasta_text` / `roundtrip_text` / `summary_text` are the three files.  Everything is written the slow, obvious
way: strings, dictionaries, loops.  Coordinates are 0-based and half-open.
"""
from __future__ import annotations

import vcfcheck_ref as R
import vcfcmp_ref as M
import vcfhap_ref as HR

RT_NONE, RT_EQUAL, RT_DIFFER, RT_NO_PATH, RT_AMBIGUOUS = range(5)
RT_NAME = ["none", "equal", "differ", "no_path", "ambiguous"]
NIL, NIL64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
COUNTS = ("n_applied", "n_duplicate", "n_enclosed", "n_overlap", "n_unspelled", "n_nocall")
OUTPUT_LIMIT = 2 ** 32 - 64


def order_key(ed):
    """An applied edit (s, e, T folded, group, item): s ascending, insertions first, e descending, then the group number (and,
    among the copies of one group, the item)."""
    s, e, _, group, item = ed
    return (s, 0 if s == e else 1, -e, group, item)


def decide(edits):
    """edits in order_key order -> (kept, n_duplicate, n_enclosed, n_overlap)."""
    kept, n_dup, n_enc, n_ovl = [], 0, 0, 0
    most, prev = None, None  # the largest e in front, kept or not; the edit in front
    for ed in edits:
        s, e, t, _, _ = ed
        if prev is not None and (prev[0], prev[1], prev[2]) == (s, e, t):
            n_dup += 1
        elif most is not None and s < most:
            if e <= most:
                n_enc += 1
            else:
                n_ovl += 1
        elif prev is not None and s == e and prev[0] == prev[1] == s:
            n_ovl += 1
        else:
            kept.append(ed)
        most = e if most is None else max(most, e)
        prev = ed
    return kept, n_dup, n_enc, n_ovl


def apply(text: str, kept, raw) -> str:
    """text with the kept edits applied; raw[item]: T as the VCF has it."""
    out, at = [], 0
    for s, e, _, _, item in kept:
        out.append(text[at:s])
        out.append(raw[item])
        at = e
    out.append(text[at:])
    return "".join(out)


def third_field(name: str):
    f = name.split("#", 2)
    return f[2] if len(f) == 3 else None


def consensus(doc: dict, names, ref: dict, roundtrip: bool = False, columns=None, chroms=None, force_tier2: bool = False) -> dict:
    """columns / chroms: the selected sample columns / CHROM ids, None for all."""
    first_of = {}
    for n in names:
        first_of.setdefault(n, ref[n])
    # ---- records, items, edits (those of the haplotype comparison in reference mode, without reaches)
    recs, items, raw, groups = [], [], {}, {}
    n_tier2 = 0
    for r, rec in enumerate(doc["records"]):
        texts = [al["text"] for al in rec["alleles"] if al["text"] is not None]
        rtext, pos = texts[0], rec["pos"]
        placed = rtext not in ("", ".") and rec["chrom"] in first_of and pos >= 1 and pos - 1 + len(rtext) <= len(first_of[rec["chrom"]])
        recs.append(dict(placed=placed, edits={}, n_alts=len(texts) - 1, chrom=doc["chroms"].index(rec["chrom"])))
        for k in range(1, len(texts)):
            item = len(items)
            items.append((r, k))
            n_tier2 += force_tier2 or min(len(rtext), len(texts[k])) > HR.TIER1_BYTES
            if not placed or M.skipped(rtext, texts[k]):
                continue
            s, e, t, sfx, pre = HR.edit_of(pos, rtext, texts[k])
            group = groups.setdefault((rec["chrom"], s, e, t), len(groups))
            recs[r]["edits"][k] = (s, e, t, group, item)
            raw[item] = texts[k][pre:len(texts[k]) - sfx]
    # ---- haplotypes
    found = {}
    for r, rec in enumerate(doc["records"]):
        info = recs[r]
        if not info["placed"] or (chroms is not None and info["chrom"] not in chroms):
            continue
        for a, c, j in rec["tasks"]:
            if columns is not None and c not in columns:
                continue
            h = found.setdefault((info["chrom"], c, j), dict(recs=set(), edits=[], n_unspelled=0))
            h["recs"].add(r)
            if a == 0:
                continue
            if a > info["n_alts"] or a not in info["edits"]:
                h["n_unspelled"] += 1
            else:
                h["edits"].append(info["edits"][a])
    samples, slot_of_path, first, count, hap_no = R.slot_haps(names)
    haps, at = [], 0
    for (c, col, j) in sorted(found):
        f = found[(c, col, j)]
        name = doc["chroms"][c]
        path = first_of[name]
        kept, n_dup, n_enc, n_ovl = decide(sorted(f["edits"], key=order_key))
        text = apply(path, kept, raw)
        n_placed = sum(1 for info in recs if info["placed"] and info["chrom"] == c)
        h = dict(chrom=c, col=col, phase=j, len=len(text), off=at, text=text, n_applied=len(kept), n_duplicate=n_dup, n_enclosed=n_enc,
                 n_overlap=n_ovl, n_unspelled=f["n_unspelled"], n_nocall=n_placed - len(f["recs"]), rt_status=RT_NONE, rt_path=NIL, rt_path_len=0,
                 rt_first_diff=NIL64)
        at += len(text)
        if roundtrip:
            sample = doc["samples"][col]
            cands = []
            if sample in samples and j < count[samples.index(sample)]:
                slot = first[samples.index(sample)] + j
                cands = [p for p, sl in enumerate(slot_of_path) if sl == slot]
                if third_field(name) is not None:
                    cands = [p for p in cands if third_field(names[p]) == third_field(name)]
            if not cands:
                h["rt_status"] = RT_NO_PATH
            elif len(cands) > 1:
                h["rt_status"] = RT_AMBIGUOUS
            else:
                spelled = ref[names[cands[0]]] if names.index(names[cands[0]]) == cands[0] else None
                assert spelled is not None, "the restatement reads a path by its name: test paths have distinct names"
                a, b = HR.fold(text), HR.fold(spelled)
                h.update(rt_path=cands[0], rt_path_len=len(spelled))
                if a == b:
                    h["rt_status"] = RT_EQUAL
                else:
                    h.update(rt_status=RT_DIFFER, rt_first_diff=HR.first_difference(a, b))
        haps.append(h)
    if at >= OUTPUT_LIMIT:
        raise ValueError("output")
    return dict(haps=haps, n_haps=len(haps), n_text_bytes=at, n_unplaced=sum(not r["placed"] for r in recs), n_tier2=n_tier2, roundtrip=roundtrip,
                hap_no=[[(-1 if hap_no[first[samples.index(s)] + j] is None else hap_no[first[samples.index(s)] + j])
                         for j in range(count[samples.index(s)])] if s in samples else [] for s in doc["samples"]])


def record_name(doc: dict, res: dict, h: dict) -> str:
    nos = res["hap_no"][h["col"]]
    no = nos[h["phase"]] if h["phase"] < len(nos) and nos[h["phase"]] >= 0 else h["phase"]
    return f"{doc['samples'][h['col']]}#{no}#{doc['chroms'][h['chrom']]}"


def fasta_text(doc: dict, res: dict, width: int = 60) -> str:
    out = []
    for h in res["haps"]:
        out.append(">" + record_name(doc, res, h) + "\n")
        t = h["text"]
        if width == 0:
            if t:
                out.append(t + "\n")
        else:
            for k in range(0, len(t), width):
                out.append(t[k:k + width] + "\n")
    return "".join(out)


def roundtrip_text(doc: dict, res: dict, names) -> str:
    out = ["CHROM\tsample\tphase\tstatus\tlen\tpath\tpath_len\tfirst_diff\tapplied\tduplicate\tenclosed\toverlap\tunspelled\tnocall\n"]
    for h in res["haps"]:
        if h["rt_status"] == RT_EQUAL:
            continue
        has = h["rt_path"] != NIL
        out.append("\t".join([doc["chroms"][h["chrom"]], doc["samples"][h["col"]], str(h["phase"]), RT_NAME[h["rt_status"]], str(h["len"]),
                              names[h["rt_path"]] if has else ".", str(h["rt_path_len"]) if has else ".",
                              str(h["rt_first_diff"]) if h["rt_status"] == RT_DIFFER else "."] + [str(h[k]) for k in COUNTS]) + "\n")
    return "".join(out)


def summary_text(res: dict) -> str:
    haps = res["haps"]
    return "".join([f"Haplotypes: {len(haps)}, bases {res['n_text_bytes']}\n",
                    "Round trip: " + ", ".join(f"{RT_NAME[k]} {sum(h['rt_status'] == k for h in haps)}" for k in range(5)) + "\n",
                    "Edits: " + ", ".join(f"{k[2:]} {sum(h[k] for h in haps)}" for k in COUNTS) + "\n"] +
                   ([f"Unplaced records: {res['n_unplaced']}\n"] if res["n_unplaced"] else []))
