"""Plain-Python restatement of the untangled calls ("Untangled calls (decided here, modelled on
`ita::untangle`)"), the yardstick of povu_hip_call with POVU_HIP_T_UNTANGLE and of `povu call --untangle`.

Built on vcf_ref (the plain call, whose records stay and whose rows are rewritten where a haplotype laps a site) and
traversals_ref.  `align` is the unit-cost alignment of two lap sequences with the tie rule of "Decomposed calls", `call` the
record list (vcf_ref's dicts with `lap`, `n_laps`, `lap_count`, `unt` added) and the counters, `vcf_text` the VCF.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import inversions_ref as IR
import traversals_ref as TR
import vcf_ref as VR

MAX_LAPS = 64
CN_MAX = 65535
HEADER_LINES = (
    '##INFO=<ID=LN,Number=1,Type=Integer,Description="Lap of the reference path through the site this record is, from 1">\n'
    '##INFO=<ID=LC,Number=1,Type=Integer,Description="Laps of the reference path through the site">\n'
    '##FORMAT=<ID=CN,Number=.,Type=Integer,Description="Laps of the sample\'s haplotypes through the site">\n'
)
COUNTERS = ("n_unt_tasks", "n_unt_records", "n_unt_missing", "n_unt_extra", "n_unt_fallback")
DIAG, DEL, INS = 0, 1, 2


class UntangleError(ValueError):
    pass


def align(a: Sequence[int], b: Sequence[int]) -> Tuple[List[Optional[int]], int, int]:
    """(partner of every row, extra columns, cost) of the unit-cost alignment of a (rows) and b (columns): a cell's code names
    the first of diagonal, deletion, insertion that gives its value; the traceback follows the codes from (n, m)."""
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    code = [[INS] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        D[i][0] = i
        code[i][0] = DEL
    for j in range(m + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            d, dl, ins = D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1
            v = min(d, dl, ins)
            D[i][j] = v
            code[i][j] = DIAG if d == v else DEL if dl == v else INS
    partner: List[Optional[int]] = [None] * n
    extra = 0
    i, j = n, m
    while i or j:
        c = INS if i == 0 else DEL if j == 0 else code[i][j]
        if c == DIAG:
            partner[i - 1] = j - 1
            i, j = i - 1, j - 1
        elif c == DEL:
            i -= 1
        else:
            extra += 1
            j -= 1
    return partner, extra, D[n][m]


def refuse(nested=False, merge=False, offref=False, profile="raw-graph"):
    """The refusals of the flag."""
    if nested:
        raise UntangleError("POVU_HIP_T_UNTANGLE is refused together with POVU_HIP_T_NESTED")
    if merge:
        raise UntangleError("POVU_HIP_T_UNTANGLE is refused together with POVU_HIP_T_MERGE")
    if offref:
        raise UntangleError("POVU_HIP_T_UNTANGLE is refused together with POVU_HIP_T_OFFREF")
    if profile != "raw-graph":
        raise UntangleError(f"POVU_HIP_T_UNTANGLE is refused with profile {profile}: only raw-graph")


def laps_of(travs) -> Dict[int, list]:
    """path -> its traversals of the site, ascending first."""
    L: Dict[int, list] = {}
    for t in travs:
        L.setdefault(t[0], []).append(t)
    return L


def unmixed(laps) -> bool:
    return len({t[3] for t in laps}) == 1


def call(sites, names, paths, seqs, prefixes, max_steps=TR.DEFAULT_MAX_STEPS, inversions=False, **flags):
    """(records in file order, counters) of the call with the flag."""
    refuse(**flags)
    recs = VR.call(sites, names, paths, seqs, prefixes, max_steps)
    samples, slot, sample_of = VR.slots_of(names)
    S = len(sample_of)
    index = TR.PathIndex(paths)
    found = {}
    tasks: Dict[tuple, tuple] = {}
    counts = dict.fromkeys(COUNTERS, 0)
    for r in recs:
        q, R = r["q"], r["path"]
        if q not in found:
            st = sites[q]
            found[q] = TR.traversals_of(index, st["s"], st["z"], max_steps)
        alleles, travs, status = found[q]
        L = laps_of(travs)
        mine = L[R]
        j = [t[1] for t in mine].index(r["first"])
        ra = mine[j][4]
        order = [ra] + [a for a in range(len(alleles)) if a != ra]
        code = {a: k for k, a in enumerate(order)}
        by_slot: Dict[int, list] = {}
        for p in L:
            by_slot.setdefault(slot[p], []).append(p)
        n = len(mine)
        ref_ok = unmixed(mine) and 1 <= n <= MAX_LAPS
        gts, tangled, unt = [], status != 0, False
        lap_count = [0] * S
        for sl in range(S):
            ps = by_slot.get(sl, [])
            lap_count[sl] = min(CN_MAX, sum(len(L[p]) for p in ps))
            aligned = (ref_ok and sl != slot[R] and len(ps) == 1 and ps[0] != R and unmixed(L[ps[0]])
                       and len(L[ps[0]]) <= MAX_LAPS)
            if not aligned:
                got = {ra} if sl == slot[R] else {t[4] for p in ps for t in L[p]}
                gts.append(code[next(iter(got))] if len(got) == 1 else None)
                tangled |= len(got) > 1
                counts["n_unt_fallback"] += sum(len(L[p]) for p in ps) >= 2
                continue
            p = ps[0]
            m = len(L[p])
            a = [t[4] for t in mine]
            b = [t[4] for t in L[p]]
            if L[p][0][3] != mine[0][3]:
                b.reverse()
            key = (q, R, p)
            if key not in tasks:
                tasks[key] = align(a, b)
                if max(n, m) >= 2:
                    counts["n_unt_tasks"] += 1
                    counts["n_unt_missing"] += sum(x is None for x in tasks[key][0])
                    counts["n_unt_extra"] += tasks[key][1]
            unt |= max(n, m) >= 2
            pj = tasks[key][0][j]
            gts.append(None if pj is None else code[b[pj]])
        gt = []
        for si in range(len(samples)):
            vals = [gts[sl] for sl in range(S) if sample_of[sl] == si]
            gt.append("." if all(v is None for v in vals) else "|".join("." if v is None else str(v) for v in vals))
        r.update(slots=gts, gt=gt, tangled=tangled, ac=[sum(1 for g in gts if g == i) for i in range(1, len(order))],
                 an=sum(1 for g in gts if g is not None),
                 ns=len({sample_of[sl] for sl, g in enumerate(gts) if g is not None}),
                 lap=j + 1, n_laps=n, lap_count=lap_count, unt=unt)
        counts["n_unt_records"] += unt
    if inversions:
        inv = IR.records(names, paths, seqs, prefixes, max_steps)[0]
        for r in inv:
            r.update(lap=0, n_laps=0, lap_count=[0] * S, unt=False)
        recs = IR.merge(recs, inv)
    return recs, counts


def record_line(r, names) -> str:
    line = IR.record_line(r)
    if not r["unt"]:
        return line
    _, _, sample_of = VR.slots_of(names)
    f = line.split("\t")
    f[7] += f";LN={r['lap']};LC={r['n_laps']}"
    f[8] = "GT:CN"
    for si in range(len(f) - 9):
        cn = [r["lap_count"][sl] for sl in range(len(sample_of)) if sample_of[sl] == si]
        f[9 + si] += ":" + ",".join("." if c == 0 else str(c) for c in cn)
    return "\t".join(f)


def vcf_text(names, paths, seqs, recs, prefixes, date="00000000", only=None) -> str:
    samples, _, _ = VR.slots_of(names)
    refs = VR.ref_paths(names, prefixes if only is None else [only])
    out = [VR.HEADER.format(date=date), HEADER_LINES]
    for r in refs:
        out.append(f"##contig=<ID={names[r]},length={sum(len(seqs[x[0]]) for x in paths[r])}>\n")
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples) + "\n")
    keep = set(refs)
    out += [record_line(r, names) + "\n" for r in recs if r["path"] in keep]
    return "".join(out)
