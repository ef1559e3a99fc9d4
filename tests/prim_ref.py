"""Plain-Python restatement of the decomposed calls ("Decomposed calls"), the yardstick of the rows of
POVU_HIP_PROFILE_DECOMPOSED and of their VCF text (povu_hip_calls_vcf_profile).

Built on the records of vcf_ref.call / nested_ref.call (and, merged in by the caller, inversions_ref's SUBR records, which pass
through whole).  `table` is the full unit-cost edit-distance table, `traceback` the canonical alignment (diagonal, else
deletion, else insertion, from the far corner), `primitives` its SNPs, DELs and INSs left to right, `decompose` the rows of
the profile in file order with their projected genotypes and counts, `vcf_text` the VCF.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import vcf_ref as V

PROFILE = "decomposed"
MAX_LENGTH = 512  # POVU_HIP_PRIM_MAX_LENGTH
ROW_RAW, ROW_SNP, ROW_INS, ROW_DEL, ROW_PASS = 0, 1, 2, 3, 4
REASON_NONE, REASON_MAX_ALLELE_LENGTH, REASON_CONTIG_START, REASON_EMPTY_ALLELE, REASON_EQUALS_REF, REASON_SUBR = 0, 1, 2, 3, 4, 5
REASON_NAME = ["", "max_allele_length", "contig_start", "empty_allele", "equals_ref", "subr_inversion_preservation"]
KIND_NAME = ["raw", "snp", "ins", "del", "passthrough"]
KIND_VARTYPE = {ROW_SNP: "SUB", ROW_INS: "INS", ROW_DEL: "DEL"}
_DESC = (
    ("ORIGIN", "1", "String", "Raw record id"),
    ("RAW_ALT_INDEX", "1", "Integer", "Raw ALT index"),
    ("PROFILE", "1", "String", "Downstream profile name"),
    ("DECOMPOSED", "1", "String", "Record came from allele decomposition"),
    ("PASSTHROUGH", "1", "String", "Record was kept because policy forbids decomposition"),
    ("PASS_THROUGH_REASON", "1", "String", "Reason pass-through was selected"),
    ("RAW_POS", "1", "Integer", "Raw POS before profile rewrite"),
    ("RAW_REF", "1", "String", "Raw REF before profile rewrite"),
    ("RAW_ALT", "1", "String", "Raw ALT before profile rewrite"),
    ("SUBR_ORIGIN", "1", "String", "Raw SUBR semantics were preserved"),
)
PROFILE_LINES = "".join(f'##INFO=<ID={k},Number={n},Type={t},Description="{d}">\n' for k, n, t, d in _DESC)


def table(a: str, b: str) -> List[List[int]]:
    """D[i][j]: the edit distance of a[:i] and b[:j], upper-cased, row by row."""
    a, b = a.upper(), b.upper()
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D


def table_by_antidiagonals(a: str, b: str) -> List[List[int]]:
    """The same table filled the way the device fills it: every cell of i + j = t before any of t + 1."""
    a, b = a.upper(), b.upper()
    n, m = len(a), len(b)
    D = [[None] * (m + 1) for _ in range(n + 1)]
    for t in range(n + m + 1):
        for j in range(max(0, t - n), min(m, t) + 1):
            i = t - j
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D


def traceback(a: str, b: str, D=None) -> str:
    """The canonical alignment as a string of columns, left to right: M match, X mismatch, D deletion, I insertion."""
    D = table(a, b) if D is None else D
    au, bu = a.upper(), b.upper()
    i, j, ops = len(a), len(b), []
    while i or j:
        if i and j and D[i - 1][j - 1] + (au[i - 1] != bu[j - 1]) == D[i][j]:
            ops.append("M" if au[i - 1] == bu[j - 1] else "X")
            i, j = i - 1, j - 1
        elif i and D[i - 1][j] + 1 == D[i][j]:
            ops.append("D")
            i -= 1
        else:
            ops.append("I")
            j -= 1
    return "".join(reversed(ops))


def primitives(a: str, b: str, ops: str = None):
    """[(kind, offset in a, offset in b, bases of a, bases of b)] of the alignment, left to right: every X an SNP, every
    maximal run of D a DEL, of I an INS."""
    ops = traceback(a, b) if ops is None else ops
    out, i, j, k = [], 0, 0, 0
    while k < len(ops):
        o = ops[k]
        if o == "M":
            i, j, k = i + 1, j + 1, k + 1
        elif o == "X":
            out.append((ROW_SNP, i, j, 1, 1))
            i, j, k = i + 1, j + 1, k + 1
        else:
            e = k
            while e < len(ops) and ops[e] == o:
                e += 1
            if o == "D":
                out.append((ROW_DEL, i, j, e - k, 0))
                i += e - k
            else:
                out.append((ROW_INS, i, j, 0, e - k))
                j += e - k
            k = e
    return out


def apply(a: str, b: str, prims) -> str:
    """`a` with the primitives applied (the bases of `b` they name)."""
    out, at = [], 0
    for _kind, i, j, la, lb in prims:
        out.append(a[at:i])
        out.append(b[j:j + lb])
        at = i + la
    out.append(a[at:])
    return "".join(out)


def pair_rows(ref: str, alt: str, pos: int, context: str, cap: int, subr=False):
    """The rows of one (REF, ALT): [dict(kind, reason, index, pos, ref_start, ref_len, alt_start, alt_len, lead)] and the cells
    of its table (0 when it is not aligned).  context: the bases of the reference path in front of POS."""
    whole = dict(kind=ROW_PASS, index=0, pos=pos, ref_start=0, ref_len=len(ref), alt_start=0, alt_len=len(alt), lead="")
    if subr:
        return [dict(whole, reason=REASON_SUBR)], 0
    if not ref or not alt:
        return [dict(whole, reason=REASON_EMPTY_ALLELE)], 0
    if len(ref) > cap or len(alt) > cap:
        return [dict(whole, reason=REASON_MAX_ALLELE_LENGTH)], 0
    cells = (len(ref) + 1) * (len(alt) + 1)
    if ref.upper() == alt.upper():
        return [dict(whole, reason=REASON_EQUALS_REF)], cells
    prims = primitives(ref, alt)
    if prims[0][0] != ROW_SNP and prims[0][1] == 0 and pos == 1:
        return [dict(whole, reason=REASON_CONTIG_START)], cells
    rows, count = [], {ROW_SNP: 0, ROW_INS: 0, ROW_DEL: 0}
    for kind, i, j, la, lb in prims:
        count[kind] += 1
        row = dict(kind=kind, reason=REASON_NONE, index=count[kind], ref_start=i, ref_len=la, alt_start=j, alt_len=lb)
        if kind == ROW_SNP:
            row.update(pos=pos + i, lead="")
        else:
            row.update(pos=pos + i - 1, lead=ref[i - 1] if i else context[pos - 2])
        rows.append(row)
    return rows, cells


def row_texts(row, ref: str, alt: str):
    return (row["lead"] + ref[row["ref_start"]:row["ref_start"] + row["ref_len"]],
            row["lead"] + alt[row["alt_start"]:row["alt_start"] + row["alt_len"]])


def project(slots: Sequence, alt: int, sample_of: Sequence[int], n_samples: int):
    """(per-slot codes, gt strings, ac, an, ns) of a record's slots seen from ALT `alt`: 0 stays, `alt` is 1, anything else is
    missing."""
    got = [0 if g == 0 else 1 if g == alt else None for g in slots]
    gt = []
    for si in range(n_samples):
        vals = [got[sl] for sl in range(len(sample_of)) if sample_of[sl] == si]
        gt.append("." if all(v is None for v in vals) else "|".join("." if v is None else str(v) for v in vals))
    return (got, gt, sum(1 for g in got if g == 1), sum(1 for g in got if g is not None),
            len({sample_of[sl] for sl, g in enumerate(got) if g is not None}))


def decompose(recs: List[dict], names, paths, seqs: Dict[int, str], max_allele_length: int = 0, force_tier2: bool = False):
    """The rows of the profile from the raw records, in file order, and the counters (n_prim_tier2: the aligned pairs with a
    text of more than 64 bytes, all of them with force_tier2)."""
    if max_allele_length > MAX_LENGTH:
        raise V.CallError(f"max_allele_length {max_allele_length} is above the ceiling {MAX_LENGTH}")
    cap = max_allele_length or MAX_LENGTH
    samples, _, sample_of = V.slots_of(names)
    text: Dict[int, str] = {}
    rows, cells, n_dec, n_pass, n_t2 = [], 0, 0, 0, 0
    for ri, r in enumerate(recs):
        subr = r["vartype"] == "SUBR"
        if r["path"] not in text:
            text[r["path"]] = "".join(V._spell(x, seqs) for x in paths[r["path"]])
        for k, alt in enumerate(r["alts"], 1):
            got, c = pair_rows(r["ref"], alt, r["pos"], text[r["path"]], cap, subr)
            cells += c
            n_t2 += c > 0 and (force_tier2 or max(len(r["ref"]), len(alt)) > 64)
            if (len(r["alts"]) == 1 and len(got) == 1 and got[0]["kind"] != ROW_PASS
                    and (got[0]["pos"],) + row_texts(got[0], r["ref"], alt) == (r["pos"], r["ref"], alt)):
                got = [dict(got[0], kind=ROW_RAW, index=0)]
            elif got[0]["kind"] == ROW_PASS:
                n_pass += 1
            else:
                n_dec += 1
            _, gt, ac, an, ns = project(r["slots"], k, sample_of, len(samples))
            for order, row in enumerate(got):
                rows.append(dict(row, rec=ri, alt=k, order=order, path=r["path"], gt=gt, ac=ac, an=an, ns=ns))
    rows.sort(key=lambda x: (x["path"], x["pos"], x["rec"], x["alt"], x["order"]))
    return rows, dict(n_rows=len(rows), n_decomposed_alts=n_dec, n_passthrough_alts=n_pass, n_prim_tier2=n_t2, n_prim_cells=cells)


def row_line(row, r, raw_line) -> str:
    """The line of a row of record r; raw_line(r) writes a raw record's line (vcf_ref / nested_ref / inversions_ref)."""
    if row["kind"] == ROW_RAW:
        return raw_line(r)
    alt = r["alts"][row["alt"] - 1]
    ref_t, alt_t = row_texts(row, r["ref"], alt)
    origin = r.get("es", r["id"])
    subr = row["reason"] == REASON_SUBR
    if subr:
        rid = f"{r['id']}:subr-passthrough"
    elif row["kind"] == ROW_PASS:
        rid = f"{origin}:{row['alt']}:passthrough"
    else:
        rid = f"{origin}:{row['alt']}:{KIND_NAME[row['kind']]}{row['index']}"
    passed = row["kind"] == ROW_PASS
    info = (f"AC={row['ac']};AF={'%.1f' % (row['ac'] / row['an'] if row['an'] else 0.0)};AN={row['an']};NS={row['ns']};"
            f"AT={r['at'][0]},{r['at'][row['alt']]};VARTYPE={r['vartype'] if passed else KIND_VARTYPE[row['kind']]};"
            f"TANGLED={'T' if passed and r['tangled'] else 'F'};ORIGIN={origin};RAW_ALT_INDEX={row['alt']};PROFILE={PROFILE};")
    info += f"PASSTHROUGH=T;PASS_THROUGH_REASON={REASON_NAME[row['reason']]}" if passed else "DECOMPOSED=T"
    info += ";SUBR_ORIGIN=T" if subr else f";RAW_POS={r['pos']};RAW_REF={r['ref']};RAW_ALT={alt}"
    return "\t".join([r["chrom"], str(row["pos"]), rid, ref_t, alt_t, "60", "PASS", info, "GT"] + row["gt"])


def vcf_text(names, paths, seqs, recs, rows, prefixes, raw_line=V.record_line, date="00000000", only=None, nested=False) -> str:
    import nested_ref as N
    samples, _, _ = V.slots_of(names)
    refs = V.ref_paths(names, prefixes if only is None else [only])
    out = [V.HEADER.format(date=date), N.PS_LINE if nested else "", PROFILE_LINES]
    for r in refs:
        out.append(f"##contig=<ID={names[r]},length={sum(len(seqs[x[0]]) for x in paths[r])}>\n")
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples) + "\n")
    keep = set(refs)
    out += [row_line(row, recs[row["rec"]], raw_line) + "\n" for row in rows if row["path"] in keep]
    return "".join(out)
