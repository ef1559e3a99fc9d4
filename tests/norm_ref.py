"""Plain-Python restatement of the left-normalised calls ("Left-normalised calls"), the yardstick of
povu_hip_call_profile under POVU_HIP_PROFILE_LEFT_NORMALIZED and of `povu call --profile left-normalized`.

Built on the records of vcf_ref.call / nested_ref.call (and, merged in by the caller, inversions_ref's SUBR records, which pass
unchanged).  `closed_form` is the definition; `literal_loop` restates, independently, the loop it is the fixed point of
(chop a common last base, extend left where an allele is empty, repeat; then trim common first bases while every allele
keeps two).  `normalise` gives the records of the profile in file order, `vcf_text` the VCF.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import vcf_ref as V

PROFILE = "left-normalized"
_DESC = (
    ("ORIGIN", "1", "String", "Raw record id"),
    ("RAW_ALT_INDEX", "A", "Integer", "Raw ALT index"),
    ("PROFILE", "1", "String", "Downstream profile name"),
    ("LEFT_NORMALIZED", "1", "String", "Record was left-normalized"),
    ("RAW_POS", "1", "Integer", "Raw POS before profile rewrite"),
    ("RAW_REF", "1", "String", "Raw REF before profile rewrite"),
    ("RAW_ALT", "A", "String", "Raw ALT before profile rewrite"),
)
PROFILE_LINES = "".join(f'##INFO=<ID={k},Number={n},Type={t},Description="{d}">\n' for k, n, t, d in _DESC)


def _suffix(a: str, b: str) -> int:
    n = 0
    while n < len(a) and n < len(b) and a[len(a) - 1 - n] == b[len(b) - 1 - n]:
        n += 1
    return n


def _prefix(xs: Sequence[str]) -> int:
    n = 0
    while all(n < len(x) for x in xs) and len({x[n] for x in xs}) == 1:
        n += 1
    return n


def closed_form(context: str, alleles: Sequence[str]):
    """(r, s, u, alleles', compared) of REF alleles[0] and the ALTs behind `context` (the bases in front of POS); None when
    the record stays unchanged whatever the context (an empty text, or no ALT that differs from REF).  compared: the
    positions the backward comparisons look at (up to and with the first difference; the allele's length for an ALT whose
    text is REF's)."""
    if any(not a for a in alleles):
        return None
    up = [a.upper() for a in alleles]
    cu = context.upper()
    other = [i for i in range(1, len(up)) if up[i] != up[0]]
    compared = sum(len(up[0]) for i in range(1, len(up)) if up[i] == up[0])
    if not other:
        return None
    ls = [_suffix(cu + up[0], cu + up[i]) for i in other]
    compared += sum(x + 1 for x in ls)
    min_len = min(len(a) for a in alleles)
    r = min(min(ls), len(context) + min_len - 1)
    s = max(0, r + 1 - min_len)
    out = [(context[len(context) - s:] + a)[:s + len(a) - r] for a in alleles]
    u = 0
    if s == 0:
        u = min(_prefix([x.upper() for x in out]), min(len(x) for x in out) - 1)
    return r, s, u, [x[u:] for x in out], compared


def literal_loop(context: str, alleles: Sequence[str]):
    """(POS shift to the left, bases trimmed in front, alleles') by the loop itself."""
    if any(not a for a in alleles) or len({a.upper() for a in alleles}) == 1:
        return 0, 0, list(alleles)
    al, left = list(alleles), len(context)
    while True:
        if all(al) and len({a[-1].upper() for a in al}) == 1 and (min(len(a) for a in al) > 1 or left > 0):
            al = [a[:-1] for a in al]
            changed = True
        else:
            changed = False
        if any(not a for a in al):
            left -= 1
            al = [context[left] + a for a in al]
            changed = True
        if not changed:
            break
    u = 0
    while min(len(a) for a in al) >= 2 and len({a[0].upper() for a in al}) == 1:
        al = [a[1:] for a in al]
        u += 1
    return len(context) - left, u, al


def path_text(steps, seqs) -> str:
    return "".join(V._spell(x, seqs) for x in steps)


def normalise(recs: List[dict], paths, seqs: Dict[int, str]):
    """The records of the profile from the raw ones (each a copy; raw_pos, raw_ref, raw_alts, r, s, u, normalized added), in
    file order, and the counters."""
    text: Dict[int, str] = {}
    out, compared = [], 0
    for r0 in recs:
        r = dict(r0)
        r.update(raw_pos=r["pos"], raw_ref=r["ref"], raw_alts=list(r["alts"]), r=0, s=0, u=0, normalized=False)
        if r["vartype"] != "SUBR":
            if r["path"] not in text:
                text[r["path"]] = path_text(paths[r["path"]], seqs)
            got = closed_form(text[r["path"]][:r["pos"] - 1], [r["ref"]] + r["alts"])
            if got is None and r["ref"] and all(r["alts"]):
                # every ALT's text is REF's: the record stays, and each ALT still counts its allele's length (INTEGRATION.md
                # "Left-normalised calls", Counters: per (record, ALT))
                compared += len(r["ref"]) * len(r["alts"])
            if got is not None:
                compared += got[4]
                if got[0] or got[2]:
                    r.update(r=got[0], s=got[1], u=got[2], ref=got[3][0], alts=got[3][1:], pos=r["pos"] - got[1] + got[2],
                             normalized=True, id=r["id"] + ":norm")
        out.append(r)
    # (path, POS, query, first[, steps]) as the raw order, with the normalised POS; a SUBR record has no query: the device's NIL
    out.sort(key=lambda r: (r["path"], r["pos"], 0xFFFFFFFF if r["vartype"] == "SUBR" else r["q"], r["first"], r.get("n_steps", 0)))
    counters = dict(n_normalized=sum(r["normalized"] for r in out), max_shift=max([r["s"] for r in out], default=0),
                    n_norm_compared=compared)
    return out, counters


def info_suffix(r) -> str:
    if not r["normalized"]:
        return ""
    es = r["id"][:-len(":norm")]
    return (f";ORIGIN={es};RAW_ALT_INDEX={','.join(str(k + 1) for k in range(len(r['alts'])))};PROFILE={PROFILE};"
            f"LEFT_NORMALIZED=T;RAW_POS={r['raw_pos']};RAW_REF={r['raw_ref']};RAW_ALT={','.join(r['raw_alts'])}")


def record_line(r, raw_line) -> str:
    """The line of a record of the profile; raw_line(r) writes the raw record's line (vcf_ref / nested_ref / inversions_ref)."""
    f = raw_line(dict(r, id=r["id"][:-len(":norm")]) if r["normalized"] else r).split("\t")
    f[2] = r["id"]
    f[7] += info_suffix(r)
    return "\t".join(f)


def vcf_text(names, paths, seqs, recs, prefixes, raw_line=V.record_line, date="00000000", only=None, nested=False) -> str:
    import nested_ref as N
    samples, _, _ = V.slots_of(names)
    refs = V.ref_paths(names, prefixes if only is None else [only])
    out = [V.HEADER.format(date=date), N.PS_LINE if nested else "", PROFILE_LINES]
    for r in refs:
        out.append(f"##contig=<ID={names[r]},length={sum(len(seqs[x[0]]) for x in paths[r])}>\n")
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples) + "\n")
    keep = set(refs)
    out += [record_line(r, raw_line) + "\n" for r in recs if r["path"] in keep]
    return "".join(out)
