"""Plain-Python restatement of the inversion calls ("Inversion calls"), the yardstick of povu_hip_call with
POVU_HIP_T_INVERSIONS and of `povu call --inversions`.

Built on vcf_ref / traversals_ref.  A step of another path A matches a step of a reference path R when it is the same
segment in the opposite orientation; a run is a maximal anti-diagonal of matches (i, j), (i + 1, j - 1), ...; a run of 2 to
max_steps steps that spells a base supports the record (R, i, L).  `runs` lists the run heads with their lengths, `records`
the SUBR records (dicts like vcf_ref.call's), `call` / `merge` the one record list of a call with inversions and `vcf_text`
its VCF.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import traversals_ref as TR
import vcf_ref as V

NIL = 0xFFFFFFFF
TIER1_STEPS = 64  # a run that is longer goes to the wave-per-run kernel


def runs(paths, refs: Sequence[int], max_steps: int = TR.DEFAULT_MAX_STEPS):
    """([(R, i, L, A, j)], stats): every run head of every reference path, L counted up to max_steps + 1.  stats: heads,
    long (L > max_steps), tier2 (L > 64), max_opposite (the longest list of opposite occurrences a reference step has)."""
    paths = [[(int(a), int(b)) for a, b in p] for p in paths]
    occ: Dict[tuple, list] = {}
    for a, p in enumerate(paths):
        for j, s in enumerate(p):
            occ.setdefault(s, []).append((a, j))
    out, max_opp = [], 0
    for r in refs:
        p = paths[r]
        for i, s in enumerate(p):
            lst = occ.get(TR.flip(s), ())
            max_opp = max(max_opp, len(lst))
            for a, j in lst:
                if a == r:
                    continue
                q = paths[a]
                if i > 0 and j + 1 < len(q) and q[j + 1] == TR.flip(p[i - 1]):
                    continue  # (i - 1, j + 1) is a match: not the head of its run
                n = 1
                while n <= max_steps and i + n < len(p) and j - n >= 0 and q[j - n] == TR.flip(p[i + n]):
                    n += 1
                out.append((r, i, n, a, j))
    stats = dict(heads=len(out), long=sum(1 for x in out if x[2] > max_steps), tier2=sum(1 for x in out if x[2] > TIER1_STEPS),
                 max_opposite=max_opp)
    return out, stats


def step_label(a, z) -> str:
    """ID of a record whose REF runs from step a to step z: both written '>' when both are '<'."""
    if a[1] == 1 and z[1] == 1:
        a, z = (a[0], 0), (z[0], 0)
    return V.label(a, z)


def records(names, paths, seqs: Dict[int, str], prefixes, max_steps: int = TR.DEFAULT_MAX_STEPS):
    """(records sorted by (path, pos, first, n_steps), stats)."""
    refs = V.ref_paths(names, prefixes)
    samples, slot, sample_of = V.slots_of(names)
    paths = [[(int(a), int(b)) for a, b in p] for p in paths]
    found, stats = runs(paths, refs, max_steps)
    groups: Dict[tuple, set] = {}
    for r, i, n, a, _j in found:
        if 2 <= n <= max_steps:
            groups.setdefault((r, i, n), set()).add(slot[a])
    off = {}
    for r in refs:
        off[r] = [0]
        for x in paths[r]:
            off[r].append(off[r][-1] + len(seqs[x[0]]))
    recs = []
    for (r, i, n), sup in groups.items():
        steps = paths[r][i:i + n]
        ref = "".join(V._spell(x, seqs) for x in steps)
        if not ref:
            continue
        back = [TR.flip(x) for x in reversed(steps)]
        alt = "".join(V._spell(x, seqs) for x in back)
        gts = [0 if sl == slot[r] else 1 if sl in sup else None for sl in range(len(sample_of))]
        gt = []
        for si in range(len(samples)):
            vals = [gts[sl] for sl in range(len(sample_of)) if sample_of[sl] == si]
            gt.append("." if all(v is None for v in vals) else "|".join("." if v is None else str(v) for v in vals))
        pos = off[r][i + 1] + 1  # the locus of the run's second step
        recs.append(dict(path=r, q=NIL, first=i, n_steps=n, chrom=names[r], pos=pos, id=step_label(steps[0], steps[-1]),
                         ref=ref, alts=[alt], at=[TR.as_text(steps), TR.as_text(back)], vartype="SUBR", tangled=False, lv=None,
                         gt=gt, slots=gts, ac=[sum(1 for g in gts if g == 1)], an=sum(1 for g in gts if g is not None),
                         ns=len({sample_of[sl] for sl, g in enumerate(gts) if g is not None})))
    recs.sort(key=lambda x: (x["path"], x["pos"], x["first"], x["n_steps"]))
    stats["records"] = len(recs)
    return recs, stats


def call(sites, names, paths, seqs, prefixes, max_steps: int = TR.DEFAULT_MAX_STEPS) -> List[dict]:
    """The one record list of a call with inversions: the flubble records and the SUBR records by (path, POS, query, first,
    steps), an inversion record's query being NIL (at one POS the flubble records come first)."""
    return merge(V.call(sites, names, paths, seqs, prefixes, max_steps), records(names, paths, seqs, prefixes, max_steps)[0])


def merge(flub: List[dict], inv: List[dict]) -> List[dict]:
    """Flubble records (vcf_ref.call) and inversion records (records) in the order of one call."""
    for r in flub:
        r["n_steps"] = 0
    return sorted(flub + inv, key=lambda x: (x["path"], x["pos"], x["q"], x["first"], x["n_steps"]))


def record_line(r) -> str:
    if r["vartype"] != "SUBR":
        return V.record_line(r)
    info = (f"AC={','.join(map(str, r['ac']))};AF={','.join('%.1f' % (c / r['an']) for c in r['ac'])};AN={r['an']};"
            f"NS={r['ns']};AT={','.join(r['at'])};VARTYPE=SUBR;TANGLED=F")
    return "\t".join([r["chrom"], str(r["pos"]), r["id"], r["ref"], ",".join(r["alts"]), "60", "PASS", info, "GT"] + r["gt"])


def vcf_text(names, paths, seqs, recs, prefixes, date="00000000", only=None) -> str:
    head = V.vcf_text(names, paths, seqs, [], prefixes, date=date, only=only)
    keep = set(V.ref_paths(names, prefixes if only is None else [only]))
    return head + "".join(record_line(r) + "\n" for r in recs if r["path"] in keep)
