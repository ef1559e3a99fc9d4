"""Plain-Python restatement of the merged primitives ("Merged primitives"), the yardstick of
POVU_HIP_T_MERGE under POVU_HIP_PROFILE_DECOMPOSED: the mrow_* arrays, the counters and the VCF text.

Built on the rows of prim_ref.decompose.  `groups` puts equal primitive rows together through a dict, `member_vote` is what one
member says about one slot, `merge` the merged rows with their joint genotypes and counts, `vcf_text` the VCF.  Whether a
(record, ALT) leaves a span alone is decided by brute force over all of its rows.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import prim_ref as PR
import vcf_ref as V

MISSING = None
VOTE_NONE, VOTE_REF, VOTE_ALT, VOTE_REF_ELSEWHERE = 0, 1, 2, 3  # prim_merge.hpp
MERGE_LINES = ('##INFO=<ID=MERGED,Number=1,Type=Integer,Description="Rows of equal primitives merged into this record">\n'
               '##INFO=<ID=MERGED_FROM,Number=.,Type=String,Description="Decomposed ids of the merged rows">\n')


def texts_of(row, recs):
    r = recs[row["rec"]]
    return PR.row_texts(row, r["ref"], r["alts"][row["alt"] - 1])


def span_of(row, recs):
    """[POS, POS + len(written REF) - 1] of a row."""
    return row["pos"], row["pos"] + len(texts_of(row, recs)[0]) - 1


def row_key(row, recs):
    ref_t, alt_t = texts_of(row, recs)
    return row["path"], row["pos"], ref_t.upper(), alt_t.upper()


def groups(rows, recs) -> List[List[int]]:
    """The groups as lists of row indices in row order, in the order of their first members.  A PASS row is a group of its own."""
    out, at = [], {}
    for x, row in enumerate(rows):
        if row["kind"] == PR.ROW_PASS:
            out.append([x])
            continue
        k = row_key(row, recs)
        if k not in at:
            at[k] = len(out)
            out.append([])
        out[at[k]].append(x)
    return out


def member_vote(g, k, span, pair_spans):
    """What member (j, k) says about a slot that carries allele g of record j.  pair_spans(k') gives the spans of the rows of
    (j, k') when they are primitive rows, None when the pair was kept whole."""
    if g is MISSING:
        return VOTE_NONE
    if g == k:
        return VOTE_ALT
    if g == 0:
        return VOTE_REF
    other = pair_spans(g)
    if other is None:
        return VOTE_NONE
    a, b = span
    if any(lo <= b and a <= hi for lo, hi in other):  # (another member of the group overlaps too: it casts its own vote)
        return VOTE_NONE
    return VOTE_REF_ELSEWHERE


def merge(recs: List[dict], rows: List[dict], names):
    """(merged rows, counters).  A merged row: dict(members=[row index...], slots=[0 / 1 / None per slot], gt, ac, an, ns)."""
    samples, _, sample_of = V.slots_of(names)
    S = len(sample_of)
    of_pair: Dict[tuple, List[int]] = {}
    for x, row in enumerate(rows):
        of_pair.setdefault((row["rec"], row["alt"]), []).append(x)
    out = []
    c = dict(n_mrows=0, n_merged_groups=0, n_merged_members=0, n_merge_splits=0, n_ref_consistent=0, n_gt_conflicts=0)
    for members in groups(rows, recs):
        first = rows[members[0]]
        span = span_of(first, recs)
        passed = first["kind"] == PR.ROW_PASS
        slots = []
        for s in range(S):
            votes = []
            for x in members:
                j, k = rows[x]["rec"], rows[x]["alt"]

                def pair_spans(other, j=j):
                    got = of_pair.get((j, other))
                    if passed or not got or rows[got[0]]["kind"] == PR.ROW_PASS:
                        return None
                    return [span_of(rows[y], recs) for y in got]
                votes.append(member_vote(recs[j]["slots"][s], k, span, pair_spans))
            one = VOTE_ALT in votes
            zero = VOTE_REF in votes or VOTE_REF_ELSEWHERE in votes
            slots.append(1 if one else 0 if zero else None)
            c["n_gt_conflicts"] += one and zero
            c["n_ref_consistent"] += (not one) and VOTE_REF_ELSEWHERE in votes and VOTE_REF not in votes
        gt = []
        for si in range(len(samples)):
            vals = [slots[sl] for sl in range(S) if sample_of[sl] == si]
            gt.append("." if all(v is None for v in vals) else "|".join("." if v is None else str(v) for v in vals))
        out.append(dict(members=members, slots=slots, gt=gt, ac=sum(1 for v in slots if v == 1), an=sum(1 for v in slots if v is not None),
                        ns=len({sample_of[sl] for sl, v in enumerate(slots) if v is not None})))
        c["n_merged_groups"] += len(members) > 1
        c["n_merged_members"] += len(members) if len(members) > 1 else 0
    c["n_mrows"] = len(out)
    c = {k: int(v) for k, v in c.items()}
    return out, c


def decomposed_id(row, r) -> str:
    """The ID of a row under the decomposed profile; a RAW row's as a member of a group."""
    origin = r.get("es", r["id"])
    if row["kind"] == PR.ROW_RAW:
        prims = PR.primitives(r["ref"], r["alts"][0])
        return f"{origin}:1:{PR.KIND_NAME[prims[0][0]]}1"
    return f"{origin}:{row['alt']}:{PR.KIND_NAME[row['kind']]}{row['index']}"


def mrow_line(m, recs, rows, raw_line) -> str:
    rep = rows[m["members"][0]]
    r = recs[rep["rec"]]
    if len(m["members"]) == 1:
        if rep["kind"] == PR.ROW_RAW:
            return raw_line(dict(r, gt=m["gt"], ac=[m["ac"]], an=m["an"], ns=m["ns"]))
        return PR.row_line(dict(rep, gt=m["gt"], ac=m["ac"], an=m["an"], ns=m["ns"]), r, raw_line)
    row = dict(rep, gt=m["gt"], ac=m["ac"], an=m["an"], ns=m["ns"])
    if rep["kind"] == PR.ROW_RAW:  # its one primitive, under the decomposed ID and INFO
        row.update(kind=PR.primitives(r["ref"], r["alts"][0])[0][0], index=1)
    line = PR.row_line(row, r, raw_line)
    ids = ",".join(decomposed_id(rows[x], recs[rows[x]["rec"]]) for x in m["members"])
    return line.replace("DECOMPOSED=T;RAW_POS=", f"DECOMPOSED=T;MERGED={len(m['members'])};MERGED_FROM={ids};RAW_POS=", 1)


def vcf_text(names, paths, seqs, recs, rows, merged, prefixes, raw_line=V.record_line, date="00000000", only=None, nested=False) -> str:
    import nested_ref as N
    samples, _, _ = V.slots_of(names)
    refs = V.ref_paths(names, prefixes if only is None else [only])
    out = [V.HEADER.format(date=date), N.PS_LINE if nested else "", PR.PROFILE_LINES, MERGE_LINES]
    for r in refs:
        out.append(f"##contig=<ID={names[r]},length={sum(len(seqs[x[0]]) for x in paths[r])}>\n")
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples) + "\n")
    keep = set(refs)
    out += [mrow_line(m, recs, rows, raw_line) + "\n" for m in merged if rows[m["members"][0]]["path"] in keep]
    return "".join(out)
