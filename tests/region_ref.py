"""Plain-Python restatement of the region calls ("Region calls"), the yardstick of povu_hip_call_restricted,
HipDecomposer.call(regions=...) and `povu call --region`.

A region is (name, s, e): the 1-based bases [s, e) of the path named exactly `name`.  `marked_segments` gives the segments
with a step in a region, `passing_sites` and `passing_subr` the two rules, `select` the records of a call that remain.
`call` composes them with the other restatements at the places the definition names: the records of the full call (vcf_ref,
inversions_ref, nested_ref with its profiles, untangle_ref) are selected; the rewriting profiles (norm_ref, prim_ref,
merge_ref) then work on the selected records alone.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import inversions_ref as I
import merge_ref as MR
import nested_ref as N
import norm_ref as NR
import prim_ref as PR
import untangle_ref as U
import vcf_ref as V

NIL = I.NIL
MAX_REGIONS = 65536
MODES = ("plain", "inversions", "nested", "top-level-only", "popped", "left-normalized", "decomposed", "merged", "untangle")


class RegionError(ValueError):
    pass


def parse(text: str):
    """`name:start-end` -> (name, start, end): split at the last ':' and at the first '-' behind it."""
    what = f"region '{text}'"
    if ":" not in text:
        raise RegionError(what + " has no ':'")
    name, _, span = text.rpartition(":")
    if not name:
        raise RegionError(what + " has an empty path name")
    if "-" not in span:
        raise RegionError(what + " has no '-' behind the ':'")
    a, _, b = span.partition("-")
    for v, side in ((a, "start"), (b, "end")):
        if not v or len(v) > 18 or any(c not in "0123456789" for c in v):
            raise RegionError(what + f": the {side} '{v}' is no number of at most 18 digits")
    if int(a) >= int(b):
        raise RegionError(what + ": the start must be below the end")
    return name, int(a), int(b)


def regions_of(regions, names: Sequence[str]):
    """[(path index, s, e)] of strings or (name, s, e) tuples, with the refusals of the definition."""
    if isinstance(regions, (str, tuple)):
        regions = [regions]
    if len(regions) > MAX_REGIONS:
        raise RegionError(f"{len(regions)} regions: more than {MAX_REGIONS} are refused")
    out = []
    for r in regions:
        name, s, e = parse(r) if isinstance(r, str) else r
        if name not in names:
            raise RegionError(f"no path is named {name}")
        if not s < e < 2 ** 63:
            raise RegionError(f"[{s}, {e}) is no interval with start < end < 2^63")
        out.append((list(names).index(name), s, e))
    return out


def step_in_region(off: int, length: int, s: int, e: int) -> bool:
    """Step of `length` bases behind `off` bases of its path: its bases meet [s, e); no bases count as one position."""
    return off + 1 < e and s < off + 1 + max(length, 1)


def marked_segments(names, paths, seqs: Dict[int, str], regions) -> set:
    marked = set()
    for pi, s, e in regions_of(regions, names):
        off = 0
        for seg, _rev in paths[pi]:
            ln = len(seqs[seg])
            if step_in_region(off, ln, s, e):
                marked.add(seg)
            off += ln
    return marked


def passing_sites(sites, names, paths, seqs, regions) -> List[bool]:
    """Per site: its S or its Z segment is marked."""
    marked = marked_segments(names, paths, seqs, regions)
    return [st["s"][0] in marked or st["z"][0] in marked for st in sites]


def passing_subr(recs, names, paths, seqs, regions) -> List[bool]:
    """Per record of `recs`: it is an inversion record (R, i, L) and the segment of R[i] or of R[i + L - 1] is marked."""
    marked = marked_segments(names, paths, seqs, regions)
    return [r["q"] == NIL and (paths[r["path"]][r["first"]][0] in marked or paths[r["path"]][r["first"] + r["n_steps"] - 1][0] in marked)
            for r in recs]


def select(recs: List[dict], sites, names, paths, seqs, regions) -> List[dict]:
    """The records of `recs` (any restatement's, in its order) whose site or inversion passes."""
    ok_site = passing_sites(sites, names, paths, seqs, regions)
    ok_subr = passing_subr(recs, names, paths, seqs, regions)
    return [r for k, r in enumerate(recs) if (ok_subr[k] if r["q"] == NIL else ok_site[r["q"]])]


def call(mode, sites, names, paths, seqs, prefixes, regions, date="00000000", inversions=False, **popt):
    """(records written, VCF text, records of the full call) of the region call in `mode`; regions None: the full call."""
    assert mode in MODES
    if mode == "untangle":
        full, _ = U.call(sites, names, paths, seqs, prefixes, inversions=inversions)
    elif mode in ("nested", "top-level-only", "popped"):
        full = N.call(sites, names, paths, seqs, prefixes, profile=None if mode == "nested" else mode, **popt)
    else:
        full = V.call(sites, names, paths, seqs, prefixes)
    line = N.record_line if mode in ("nested", "top-level-only", "popped") else V.record_line
    if (inversions or mode == "inversions") and mode != "untangle":
        full = I.merge(full, I.records(names, paths, seqs, prefixes)[0])
        flubble_line = line
        line = lambda r: I.record_line(r) if r["vartype"] == "SUBR" else flubble_line(r)  # noqa: E731
    recs = full if regions is None else select(full, sites, names, paths, seqs, regions)
    if mode == "untangle":
        return recs, U.vcf_text(names, paths, seqs, recs, prefixes, date=date), full
    if mode in ("nested", "top-level-only", "popped"):
        head = N.vcf_text(names, paths, seqs, [], prefixes, date=date, profile=None if mode == "nested" else mode)
        return recs, head + "".join(line(r) + "\n" for r in recs), full
    if mode == "left-normalized":
        out, _ = NR.normalise(recs, paths, seqs)
        return out, NR.vcf_text(names, paths, seqs, out, prefixes, raw_line=line, date=date), full
    if mode in ("decomposed", "merged"):
        rows, _ = PR.decompose(recs, names, paths, seqs)
        if mode == "decomposed":
            return recs, PR.vcf_text(names, paths, seqs, recs, rows, prefixes, raw_line=line, date=date), full
        merged, _ = MR.merge(recs, rows, names)
        return recs, MR.vcf_text(names, paths, seqs, recs, rows, merged, prefixes, raw_line=line, date=date), full
    head = V.vcf_text(names, paths, seqs, [], prefixes, date=date)
    return recs, head + "".join(line(r) + "\n" for r in recs), full
