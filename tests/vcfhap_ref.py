"""Plain-Python restatement of the haplotype comparison ("Haplotype comparison"), the yardstick of
povu_hip_vcf_haplotypes, povu_hip_vcf_hap_text and of `povu vcf --compare --haplotypes`.

`compare` takes two documents of vcfcmp_ref.parse and, in reference mode, the bases of every path by name.  It gives every
record its placement and window, every (record, ALT) item its edit, reaches and edit group, every window its bounds, text and
verdict, every (window, common sample, phase) cell its status; `haplotypes_text` / `summary_text` are the two files.
Everything is written the slow, obvious way: strings, dictionaries, loops.  Coordinates are 0-based and half-open.
"""
from __future__ import annotations

import string

import vcfcmp_ref as M

EDIT, UNSPELLED, UNPLACED = 0, 1, 2  # state of an item
(INCONSISTENT, NOCALL_A, NOCALL_B, UNSPELLED_A, UNSPELLED_B, CONFLICT_A, CONFLICT_B, EQUAL_REF, EQUAL, DIFFER) = range(10)
STATUS_NAME = ["inconsistent", "nocall_a", "nocall_b", "unspelled_a", "unspelled_b", "conflict_a", "conflict_b", "equal_ref", "equal", "differ"]
NIL, NIL64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
TIER1_BYTES = 32
MAX_REACH_DEFAULT, MAX_REACH_MOST = 256, 65536
_FOLD = str.maketrans(string.ascii_lowercase, string.ascii_uppercase)


def fold(t: str) -> str:
    return t.translate(_FOLD)


def full_trim(ref: str, alt: str):
    """(bytes taken at the end, bytes taken at the front) of the folded texts: the whole common suffix, then the whole common
    prefix of what is left; either text may become empty."""
    ref, alt = fold(ref), fold(alt)
    s = p = 0
    while s < len(ref) and s < len(alt) and ref[len(ref) - 1 - s] == alt[len(alt) - 1 - s]:
        s += 1
    ref, alt = ref[:len(ref) - s], alt[:len(alt) - s]
    while p < len(ref) and p < len(alt) and ref[p] == alt[p]:
        p += 1
    return s, p


def edit_of(pos: int, ref: str, alt: str):
    """(s, e, T, suffix, prefix): the reference bases [s, e) are replaced by T."""
    sfx, pre = full_trim(ref, alt)
    return pos - 1 + pre, pos - 1 + len(ref) - sfx, fold(alt)[pre:len(alt) - sfx], sfx, pre


def reach(path: str, s: int, e: int, unit: str, max_reach: int):
    """(left, right, capped) of an indel whose non-empty side is `unit` (folded), on the folded bases `path`."""
    m = len(unit)
    right = 0
    while e + right < len(path) and path[e + right] == unit[right % m]:
        right += 1
    left = 0
    while s - 1 - left >= 0 and path[s - 1 - left] == unit[m - 1 - (left % m)]:
        left += 1
    return min(left, max_reach), min(right, max_reach), left > max_reach or right > max_reach


def conflict(edits) -> bool:
    """edits: distinct (s, e, T), sorted by (s, e)."""
    most = None
    for k, (s, e, _) in enumerate(edits):
        if most is not None and s < most:
            return True
        if k and s == e and edits[k - 1][0] == edits[k - 1][1] == s:
            return True
        most = e if most is None else max(most, e)
    return False


def apply(text: str, lo: int, edits) -> str:
    out, at = [], lo
    for s, e, t in edits:
        out.append(text[at - lo:s - lo])
        out.append(t)
        at = e
    out.append(text[at - lo:])
    return "".join(out)


def first_difference(a: str, b: str) -> int:
    n = min(len(a), len(b))
    for k in range(n):
        if a[k] != b[k]:
            return k
    return n


def compare(doc_a: dict, doc_b: dict, ref: dict | None = None, max_reach: int = MAX_REACH_DEFAULT, force_tier2: bool = False) -> dict:
    docs = (doc_a, doc_b)
    paths = None if ref is None else {name: fold(seq) for name, seq in ref.items()}
    chroms = list(doc_a["chroms"]) + [c for c in doc_b["chroms"] if c not in doc_a["chroms"]]
    n_ra = len(doc_a["records"])
    # ---- records, items, edits, reaches, spans
    recs, items, spans = ([], []), ([], []), []
    n_capped = 0
    keys = {}  # (chrom, s, e, T) -> group
    for side, doc in enumerate(docs):
        for r, rec in enumerate(doc["records"]):
            texts = [al["text"] for al in rec["alleles"] if al["text"] is not None]
            rtext, pos = texts[0], rec["pos"]
            placed = rtext not in ("", ".")
            if placed and paths is not None:
                placed = rec["chrom"] in paths and pos >= 1 and pos - 1 + len(rtext) <= len(paths[rec["chrom"]])
            recs[side].append(dict(placed=placed, window=NIL, edits={}, n_alts=len(texts) - 1))
            lo, hi = pos - 1, pos - 1 + len(rtext)
            for k in range(1, len(texts)):
                it = dict(record=r, alt=k, state=UNPLACED, s=0, e=0, suffix=0, prefix=0, left=0, right=0, group=NIL,
                          tier2=force_tier2 or min(len(rtext), len(texts[k])) > TIER1_BYTES)
                items[side].append(it)
                if not placed:
                    continue
                if M.skipped(rtext, texts[k]):
                    it["state"] = UNSPELLED
                    continue
                s, e, t, it["suffix"], it["prefix"] = edit_of(pos, rtext, texts[k])
                it.update(state=EDIT, s=s, e=e, t=t)
                if paths is not None and (s == e) != (t == ""):
                    unit = t if s == e else fold(rtext)[s - (pos - 1):e - (pos - 1)]
                    it["left"], it["right"], capped = reach(paths[rec["chrom"]], s, e, unit, max_reach)
                    n_capped += capped
                    lo, hi = min(lo, s - it["left"]), max(hi, e + it["right"])
                key = (rec["chrom"], s, e, t)
                it["group"] = keys.setdefault(key, len(keys))
                recs[side][r]["edits"][k] = (s, e, t)
            if placed:
                spans.append((chroms.index(rec["chrom"]), lo, hi, side, r))
    # ---- windows
    spans.sort(key=lambda x: (x[0], x[1]))  # (stable: A's records before B's, each in document order)
    windows = []
    for c, lo, hi, side, r in spans:
        if not windows or windows[-1]["chrom"] != c or lo > windows[-1]["hi"]:
            windows.append(dict(chrom=c, lo=lo, hi=hi, members=([], []), inconsistent=0, offender=NIL))
        w = windows[-1]
        w["hi"] = max(w["hi"], hi)
        w["members"][side].append(r)
        recs[side][r]["window"] = len(windows) - 1
    # ---- window texts and verdicts
    for w in windows:
        lo, hi = w["lo"], w["hi"]
        members = [(side, r) for side in (0, 1) for r in sorted(w["members"][side])]
        fields = []
        for side, r in members:
            rec = docs[side]["records"][r]
            fields.append((rec["pos"] - 1, fold([al["text"] for al in rec["alleles"] if al["text"] is not None][0])))
        if paths is not None:
            w["text"] = paths[chroms[w["chrom"]]][lo:hi]
        else:  # every base lies in some REF field; where several do, the greatest byte stands (any choice gives the verdict)
            text = [""] * (hi - lo)
            for at, t in fields:
                for k, ch in enumerate(t):
                    text[at - lo + k] = max(text[at - lo + k], ch)
            w["text"] = "".join(text)
        assert len(w["text"]) == hi - lo and all(w["text"])
        for (side, r), (at, t) in zip(members, fields):
            if w["text"][at - lo:at - lo + len(t)] != t:
                w["inconsistent"] = 1
                w["offender"] = min(w["offender"], r + (n_ra if side else 0))
        w["n_a"], w["n_b"] = len(w["members"][0]), len(w["members"][1])
    # ---- common samples, cells
    sa, sb = doc_a["samples"], doc_b["samples"]
    samples, taken = [], set()
    for c, name in enumerate(sa):
        if name in sb and name not in taken:
            taken.add(name)
            samples.append(dict(name=name, col_a=c, col_b=sb.index(name), counts=[0] * 10))
    col_of = ({s["col_a"]: x for x, s in enumerate(samples)}, {s["col_b"]: x for x, s in enumerate(samples)})
    found = {}  # (window, sample, phase) -> per side [called, unspelled, set of edits]
    for side, doc in enumerate(docs):
        for r, rec in enumerate(doc["records"]):
            info = recs[side][r]
            if not info["placed"]:
                continue
            for a, c, j in rec["tasks"]:
                if c not in col_of[side]:
                    continue
                cell = found.setdefault((info["window"], col_of[side][c], j), ([False, False, set()], [False, False, set()]))[side]
                cell[0] = True
                if a == 0:
                    continue
                if a > info["n_alts"] or a not in info["edits"]:
                    cell[1] = True
                else:
                    cell[2].add(info["edits"][a])
    cells = []
    for (wi, x, j) in sorted(found):
        w = windows[wi]
        sides = found[(wi, x, j)]
        edits = [sorted(sd[2], key=lambda ed: (ed[0], ed[1])) for sd in sides]
        cell = dict(window=wi, sample=x, phase=j, edits_a=len(edits[0]), edits_b=len(edits[1]), len_a=0, len_b=0, first_diff=NIL64)
        if w["inconsistent"]:
            st = INCONSISTENT
        elif not sides[0][0]:
            st = NOCALL_A
        elif not sides[1][0]:
            st = NOCALL_B
        elif sides[0][1]:
            st = UNSPELLED_A
        elif sides[1][1]:
            st = UNSPELLED_B
        elif conflict(edits[0]):
            st = CONFLICT_A
        elif conflict(edits[1]):
            st = CONFLICT_B
        else:
            ha, hb = apply(w["text"], w["lo"], edits[0]), apply(w["text"], w["lo"], edits[1])
            cell.update(len_a=len(ha), len_b=len(hb), hap_a=ha, hap_b=hb)
            if ha == hb:
                st = EQUAL if edits[0] or edits[1] else EQUAL_REF
            else:
                st, cell["first_diff"] = DIFFER, first_difference(ha, hb)
        cell["status"] = st
        samples[x]["counts"][st] += 1
        cells.append(cell)
    n_status = [sum(c["status"] == k for c in cells) for k in range(10)]
    return dict(recs_a=recs[0], recs_b=recs[1], items_a=items[0], items_b=items[1], windows=windows, cells=cells, samples=samples, chroms=chroms,
                n_status=n_status, n_windows=len(windows), n_inconsistent=sum(w["inconsistent"] for w in windows), n_cells=len(cells),
                n_unplaced_a=sum(not r["placed"] for r in recs[0]), n_unplaced_b=sum(not r["placed"] for r in recs[1]),
                n_reach_capped=n_capped, n_tier2=sum(it["tier2"] for it in items[0] + items[1]), n_groups=len(keys),
                n_records_a=len(recs[0]), n_records_b=len(recs[1]), n_items_a=len(items[0]), n_items_b=len(items[1]), n_common_samples=len(samples), reference=paths is not None)


def haplotypes_text(res: dict) -> str:
    out = ["CHROM\tSTART\tEND\tsample\tphase\tstatus\tlen_a\tlen_b\tfirst_diff\tedits_a\tedits_b\n"]
    for c in res["cells"]:
        if c["status"] in (EQUAL_REF, EQUAL):
            continue
        w = res["windows"][c["window"]]
        compared = c["status"] == DIFFER
        out.append("\t".join([res["chroms"][w["chrom"]], str(w["lo"] + 1), str(w["hi"]), res["samples"][c["sample"]]["name"], str(c["phase"]),
                              STATUS_NAME[c["status"]], str(c["len_a"]) if compared else ".", str(c["len_b"]) if compared else ".",
                              str(c["first_diff"]) if compared else ".", str(c["edits_a"]), str(c["edits_b"])]) + "\n")
    return "".join(out)


def _ratio(num: int, den: int) -> str:
    return "nan" if not den else "%.4f" % (num / den)


def summary_text(res: dict) -> str:
    n = res["n_status"]
    out = [f"Windows: {res['n_windows']}, inconsistent {res['n_inconsistent']}\n",
           "Cells: " + ", ".join(f"{STATUS_NAME[k]} {n[k]}" for k in range(10)) + "\n",
           f"Concordance: {_ratio(n[EQUAL_REF] + n[EQUAL], n[EQUAL_REF] + n[EQUAL] + n[DIFFER])}\n",
           f"Non-reference concordance: {_ratio(n[EQUAL], n[EQUAL] + n[DIFFER])}\n"]
    for s in res["samples"]:
        out.append(f"Sample {s['name']}: " + ", ".join(f"{STATUS_NAME[k]} {s['counts'][k]}" for k in range(10)) + "\n")
    if res["n_unplaced_a"] or res["n_unplaced_b"]:
        out.append(f"Unplaced records: A {res['n_unplaced_a']}, B {res['n_unplaced_b']}\n")
    if res["n_reach_capped"]:
        out.append(f"Capped reaches: {res['n_reach_capped']}\n")
    return "".join(out)


def path_bases(names, paths, seqs) -> dict:
    """The bases of every path of vcf_ref.read_gfa by name ('<' steps reverse-complemented)."""
    comp = str.maketrans("ACGTNacgtn", "TGCANtgcan")
    return {n: "".join(seqs[i] if not rv else seqs[i].translate(comp)[::-1] for i, rv in st) for n, st in zip(names, paths)}
