"""Plain-Python restatement of the spanning alleles of a nested call ("Spanning alleles"), the yardstick of
povu_hip_call with POVU_HIP_T_SPANNING and of `povu call --spanning-alleles`.

Built on nested_ref.call_full, which it does not change: the records of the raw nested call give the chain of enclosing
records (`parent_rec`, before any profile drops one), traversals_ref gives per site the slots that traverse it and whether
its search was cut short.  An entry (record, slot) is spanned when the slot is not the record's own, no path of the slot
traverses the record's site, the site's status is 0, and some ancestor's site is traversed by a path of the slot.  A record
with a spanned entry gains the ALT `*` as its last: the spanned entries carry its number (the record's class count), AC has
an entry for it, AN and NS count them, its AT entry is `*`.  `call_full` gives the records the profile keeps (the dicts of
nested_ref plus star, n_alleles, spanned) and the counters, `vcf_text` the VCF (no header line is added).
"""
from __future__ import annotations

from typing import Dict, List

import nested_ref as N
import traversals_ref as TR
import vcf_ref as V


def spanned_entries(sites, names, paths, raw, max_steps=TR.DEFAULT_MAX_STEPS) -> Dict[tuple, List[int]]:
    """Of every record of the raw nested call `raw` (nested_ref.call_full without a profile), by (site, path, first): its
    spanned slots, ascending."""
    _samples, slot, sample_of = V.slots_of(names)
    index = TR.PathIndex(paths)
    crossed, status = {}, {}
    for q in {r["q"] for r in raw}:
        _al, travs, st = TR.traversals_of(index, sites[q]["s"], sites[q]["z"], max_steps)
        crossed[q] = {slot[t[0]] for t in travs}
        status[q] = st
    out = {}
    for r in raw:
        q, own = r["q"], slot[r["path"]]
        got = []
        for sl in range(len(sample_of)):
            if sl == own or sl in crossed[q] or status[q] != 0:
                continue
            k = r["parent_rec"]
            while k is not None and sl not in crossed[raw[k]["q"]]:
                k = raw[k]["parent_rec"]
            if k is not None:
                got.append(sl)
        out[(q, r["path"], r["first"])] = got
    return out


def call_full(sites, names, paths, seqs, prefixes, max_steps=TR.DEFAULT_MAX_STEPS, profile=None, spanning=True, **popt):
    recs, counters = N.call_full(sites, names, paths, seqs, prefixes, max_steps=max_steps, profile=profile, **popt)
    counters = dict(counters, n_star_records=0, n_star_entries=0)
    for r in recs:
        r["star"], r["spanned"], r["n_alleles"] = False, [], r["n_classes"]
    if not spanning:
        return recs, counters
    # the choice is made on the raw call, before the profile's filter
    raw = recs if profile is None else N.call_full(sites, names, paths, seqs, prefixes, max_steps=max_steps)[0]
    spanned = spanned_entries(sites, names, paths, raw, max_steps)
    samples, _slot, sample_of = V.slots_of(names)
    for r in recs:
        got = spanned[(r["q"], r["path"], r["first"])]
        if not got:
            continue
        star = r["n_classes"]  # the `*` code: the class count of the record
        assert all(r["slots"][sl] is None for sl in got)
        for sl in got:
            r["slots"][sl] = star
        gts = r["slots"]
        r["star"], r["spanned"], r["n_alleles"] = True, got, star + 1
        r["alts"] = r["alts"] + ["*"]
        r["at"] = r["at"] + ["*"]
        r["ac"] = r["ac"] + [len(got)]
        r["an"] = sum(1 for g in gts if g is not None)
        r["ns"] = len({sample_of[sl] for sl, g in enumerate(gts) if g is not None})
        r["gt"] = []
        for si in range(len(samples)):
            vals = [gts[sl] for sl in range(len(sample_of)) if sample_of[sl] == si]
            r["gt"].append("." if all(v is None for v in vals) else "|".join("." if v is None else str(v) for v in vals))
        counters["n_star_records"] += 1
        counters["n_star_entries"] += len(got)
    return recs, counters


def call(*a, **k) -> List[dict]:
    return call_full(*a, **k)[0]


record_line = N.record_line


def vcf_text(names, paths, seqs, recs, prefixes, date="00000000", only=None, profile=None) -> str:
    """The VCF of `recs` (of call_full with the same profile): nested_ref's text -- `*` needs no header line."""
    return N.vcf_text(names, paths, seqs, recs, prefixes, date=date, only=only, profile=profile)
