"""Plain-Python restatement of the off-reference calls ("Off-reference calls (decided here, not reference
behaviour)"), the yardstick of povu_hip_call with POVU_HIP_T_OFFREF and of `povu call --off-reference`.

Built on vcf_ref (the calls by the reference paths, which stay as they are) and traversals_ref.  `site_states` gives per
site what the rule decides, `call` the one record list (vcf_ref's dicts with `offref`, `host` and `ha` added), `vcf_text`
the VCF of a prefix, of every prefix, or of the records no prefix takes (`rest=True`: the off-reference.vcf of -o DIR).
"""
from __future__ import annotations

from typing import Dict, List

import inversions_ref as IR
import traversals_ref as TR
import vcf_ref as VR

INFO_LINES = (
    '##INFO=<ID=OFFREF,Number=0,Type=Flag,Description="Called off the reference paths: CHROM is the surrogate path, the first '
    'path that traverses the site">\n'
    '##INFO=<ID=HOST,Number=1,Type=String,Description="ID of the tightest site called on the reference paths that encloses the '
    'record on its path">\n'
    '##INFO=<ID=HA,Number=1,Type=Integer,Description="Allele of the record\'s path in HOST, numbered in traversal order">\n'
)


def site_states(sites, ref_paths: Dict[int, list], travs: List[list]):
    """(callable, called on-reference, candidate, called off-reference, surrogate path or None) per site; travs[q] the
    traversals of site q in traversal order."""
    n = len(sites)
    segs = {r: {x[0] for x in p} for r, p in ref_paths.items()}
    skipped: Dict[int, bool] = {}

    def skip(q):
        if q not in skipped:
            p = sites[q]["parent"]
            skipped[q] = sites[q]["fam"] in VR.SUBFLUBBLE or (p != VR.NO_PARENT and skip(p))
        return skipped[q]
    present: Dict[int, set] = {}
    for st in sites:
        pr = present.setdefault(st["tree"], set())
        for r, sg in segs.items():
            if st["s"][0] in sg or st["z"][0] in sg:
                pr.add(r)
    callable_ = []
    for q, st in enumerate(sites):
        pr = present[st["tree"]]
        callable_.append(not skip(q) and bool(pr) and all(st["s"][0] in segs[r] and st["z"][0] in segs[r] for r in pr))
    called = list(callable_)
    candidate = [not skip(q) and not callable_[q] and len(travs[q]) > 0 for q in range(n)]
    called_off = list(candidate)
    for q, st in enumerate(sites):
        if st["parent"] == VR.NO_PARENT:
            continue
        if callable_[q]:
            called[st["parent"]] = False
        if callable_[q] or candidate[q]:
            called_off[st["parent"]] = False
    sur = [travs[q][0][0] if called_off[q] else None for q in range(n)]
    return callable_, called, candidate, called_off, sur


def encloses(f_host, l_host, f, l) -> bool:
    """The steps [f, l] lie within [f_host, l_host], which is longer."""
    return f_host <= f and l <= l_host and l - f < l_host - f_host


def call(sites, names, paths, seqs, prefixes, max_steps=TR.DEFAULT_MAX_STEPS, inversions=False):
    """The records of the call with the flag, in file order, and the counters; with `inversions` the SUBR records of the
    reference paths (inversions_ref) in the same list."""
    refs = VR.ref_paths(names, prefixes)
    isref = set(refs)
    samples, slot, sample_of = VR.slots_of(names)
    index = TR.PathIndex(paths)
    found = [TR.traversals_of(index, st["s"], st["z"], max_steps) for st in sites]
    travs = [f[1] for f in found]
    _callable, called, _cand, called_off, sur = site_states(sites, {r: index.paths[r] for r in refs}, travs)
    recs = VR.call(sites, names, paths, seqs, prefixes, max_steps)
    for r in recs:
        r.update(offref=False, host=None, ha=None)
    hosts: Dict[int, list] = {}  # per path the traversals of the sites the references call (two alleles or more)
    for q in range(len(sites)):
        if called[q] and len(found[q][0]) >= 2:
            for ph, fh, lh, _rh, ah in travs[q]:
                hosts.setdefault(ph, []).append((fh, lh, q, ah))
    off: Dict[int, list] = {}

    def offsets(p):
        if p not in off:
            o = [0]
            for x in index.paths[p]:
                o.append(o[-1] + len(seqs[x[0]]))
            off[p] = o
        return off[p]
    n_sites = 0
    for q, st in enumerate(sites):
        if not called_off[q]:
            continue
        alleles, tv, status = found[q]
        if len(alleles) < 2:
            continue
        n_sites += 1
        by_slot: Dict[int, set] = {}
        for pi, _i, _j, _r, a in tv:
            by_slot.setdefault(slot[pi], set()).add(a)
        inner_len = [sum(len(seqs[x[0]]) for x in a[1:-1]) for a in alleles]
        anchored = min(inner_len) == 0
        for pi, first, last, rev, ra in tv:
            if pi != sur[q]:
                continue
            order = [ra] + [a for a in range(len(alleles)) if a != ra]
            code = {a: k for k, a in enumerate(order)}
            texts, ats = [], []
            for a in order:
                steps = alleles[a] if not rev else [TR.flip(x) for x in reversed(alleles[a])]
                inner = steps[1:-1]
                body = "".join(VR._spell(x, seqs) for x in inner)
                if anchored:
                    texts.append(VR._spell(steps[0], seqs, True) + body)
                    ats.append(TR.as_text([steps[0]] + inner))
                else:
                    texts.append(body)
                    ats.append(TR.as_text(inner))
            gts, tangled = [], status != 0
            for sl in range(len(sample_of)):
                got = {ra} if sl == slot[pi] else by_slot.get(sl, set())
                if len(got) == 1:
                    gts.append(code[next(iter(got))])
                else:
                    gts.append(None)
                    tangled |= len(got) > 1
            ac = [sum(1 for g in gts if g == i) for i in range(1, len(order))]
            an = sum(1 for g in gts if g is not None)
            ns = len({sample_of[sl] for sl, g in enumerate(gts) if g is not None})
            gt = []
            for si in range(len(samples)):
                vals = [gts[sl] for sl in range(len(sample_of)) if sample_of[sl] == si]
                gt.append("." if all(v is None for v in vals) else "|".join("." if v is None else str(v) for v in vals))
            pos = offsets(pi)[first + 1] + (0 if anchored else 1)
            vt = "SUB" if not anchored else "INS" if inner_len[ra] == 0 else "DEL"
            best = None
            for fh, lh, qh, ah in hosts.get(pi, []):
                if encloses(fh, lh, first, last):
                    key = (lh - fh, qh, fh)
                    if best is None or key < best[0]:
                        best = (key, qh, ah)
            recs.append(dict(path=pi, q=q, first=first, chrom=names[pi], pos=pos, id=VR.label(st["s"], st["z"]),
                             ref=texts[0], alts=texts[1:], at=ats, vartype=vt, tangled=tangled, lv=st["height"] - 1,
                             gt=gt, slots=gts, ac=ac, an=an, ns=ns, offref=True,
                             host=None if best is None else best[1], ha=None if best is None else best[2]))
    for r in recs:
        r["n_steps"] = 0
    if inversions:
        inv = IR.records(names, paths, seqs, prefixes, max_steps)[0]
        for r in inv:
            r.update(offref=False, host=None, ha=None)
        recs += inv
    recs.sort(key=lambda r: (r["path"], r["pos"], r["q"], r["first"], r["n_steps"]))
    counts = dict(n_offref_sites=n_sites, n_offref_records=sum(r["offref"] for r in recs),
                  n_offref_hosted=sum(r["host"] is not None for r in recs))
    return recs, counts


def record_line(r, sites) -> str:
    line = IR.record_line(r)
    if not r["offref"]:
        return line
    f = line.split("\t")
    f[7] += ";OFFREF=T"
    if r["host"] is not None:
        h = sites[r["host"]]
        f[7] += f";HOST={VR.label(h['s'], h['z'])};HA={r['ha']}"
    return "\t".join(f)


def off_contigs(names, recs, prefixes) -> List[int]:
    """The surrogate paths that are no reference path and carry a record, in GFA order."""
    refs = set(VR.ref_paths(names, prefixes))
    return sorted({r["path"] for r in recs if r["offref"] and r["path"] not in refs})


def vcf_text(sites, names, paths, seqs, recs, prefixes, date="00000000", only=None, rest=False) -> str:
    """The VCF of `recs` with the flag: of the paths whose name starts with `only` (None: every record), or with `rest`
    of the records whose CHROM starts with none of the prefixes."""
    samples, _, _ = VR.slots_of(names)
    refs = VR.ref_paths(names, prefixes)

    def takes(name):
        if rest:
            return not any(name.startswith(p) for p in prefixes)
        return only is None or name.startswith(only)
    out = [VR.HEADER.format(date=date), INFO_LINES]
    length = lambda k: sum(len(seqs[x[0]]) for x in paths[k])  # noqa: E731
    for r in refs:
        if takes(names[r]):
            out.append(f"##contig=<ID={names[r]},length={length(r)}>\n")
    for k in off_contigs(names, recs, prefixes):
        if takes(names[k]):
            out.append(f"##contig=<ID={names[k]},length={length(k)}>\n")
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples) + "\n")
    out += [record_line(r, sites) + "\n" for r in recs if takes(r["chrom"])]
    return "".join(out)
