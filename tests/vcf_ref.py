"""Plain-Python restatement of the variant calls ("Variant calls"), the yardstick of povu_hip_call and
of `povu call`.

Built on traversals_ref (the traversals and alleles of every query).  Sites are the queries with what the call needs of
their PVST vertex: `sites_of_pvst` reads PVST texts (component order), `sites_of_trees` a forest's arrays.  `call` gives
the records (dicts; `slots` holds the allele of every genotype slot in record numbering, None for '.') and `vcf_text` the
VCF.
"""
from __future__ import annotations

import re
from typing import Dict, List, Sequence

import traversals_ref as TR

SUBFLUBBLE = set("TOCMS")
NO_PARENT = -1
_LABEL = re.compile(r"^([<>])(\d+)([<>])(\d+)$")
_COMP = {}
for _a, _b in zip("ACGTNRYKMSWBDHV", "TGCANYRMKSWVHDB"):
    _COMP[_a], _COMP[_a.lower()] = _b, _b.lower()

HEADER = (
    "##fileformat=VCFv4.2\n"
    "##fileDate={date}\n"
    "##source=povu\n"
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    '##INFO=<ID=AC,Number=A,Type=Integer,Description="Total number of alternate alleles in called genotypes">\n'
    '##INFO=<ID=AT,Number=R,Type=String,Description="Allele traversal path through the graph">\n'
    '##INFO=<ID=AN,Number=1,Type=String,Description="Total number of alleles in called genotypes">\n'
    '##INFO=<ID=AF,Number=A,Type=Float,Description="Allele frequency in the population">\n'
    '##INFO=<ID=NS,Number=1,Type=Integer,Description="Number of samples with data">\n'
    '##INFO=<ID=VARTYPE,Number=1,Type=String,Description="Type of variation: INS (insertion), DEL (deletion), '
    'SUB (substitution), SUBR(substitution in reverse) ">\n'
    '##INFO=<ID=TANGLED,Number=1,Type=String,Description="Variant lies in a tangled region of the graph: T or F">\n'
    '##INFO=<ID=LV,Number=1,Type=Integer,Description="Level in the PVST (0=top level)">\n'
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
)


class CallError(ValueError):
    pass


def label(s, z) -> str:
    return (">" if s[1] == 0 else "<") + str(s[0]) + (">" if z[1] == 0 else "<") + str(z[0])


def _site(s, z, parent, height, fam, tree):
    return dict(s=s, z=z, parent=parent, height=height, fam=fam, tree=tree)


def sites_of_pvst(texts: Sequence[str]) -> List[dict]:
    """Sites of PVST files in component order: every vertex line but the root, in file order."""
    out = []
    for tree, text in enumerate(texts):
        rows = [ln.split("\t") for ln in text.splitlines() if ln and not ln.startswith("H")]
        qnum, parent, height = {}, {}, {}
        for f in rows:
            for c in ([] if f[3] == "." else [int(x) for x in f[3].split(", ")]):
                parent[c] = int(f[1])
        def h(v):
            if v not in height:
                height[v] = 0 if v not in parent else h(parent[v]) + 1
            return height[v]
        for f in rows:
            if f[0] != "D":
                qnum[int(f[1])] = len(out) + len(qnum)
        for f in rows:
            v = int(f[1])
            if f[0] == "D":
                continue
            m = _LABEL.match(f[2])
            s = (int(m.group(2)), 0 if m.group(1) == ">" else 1)
            z = (int(m.group(4)), 0 if m.group(3) == ">" else 1)
            out.append(_site(s, z, qnum.get(parent.get(v), NO_PARENT), h(v), f[0], tree))
    return out


def sites_of_trees(trees) -> List[dict]:
    """Sites of a forest's trees: per tree (id1, or1, id2, or2, parent, fam) indexed by PVST vertex, entry 0 the root
    (parent < 0 or >= n for the root; fam None = every vertex a flubble)."""
    out = []
    for tree, (id1, or1, id2, or2, par, fam) in enumerate(trees):
        n = len(id1)
        base = len(out) - 1
        height = [0] * n
        def h(v):
            if v and not height[v]:
                height[v] = h(int(par[v])) + 1
            return height[v]
        for v in range(1, n):
            p = int(par[v])
            out.append(_site((int(id1[v]), int(or1[v])), (int(id2[v]), int(or2[v])), NO_PARENT if p == 0 else base + p,
                             h(v), "F" if fam is None else chr(int(fam[v])), tree))
    return out


def pansn(name: str):
    f = name.split("#")
    if len(f) >= 3 and f[1].isdigit():
        return f[0], int(f[1])
    return name, None


def slots_of(names: Sequence[str]):
    """(samples in order, slot of every path, sample of every slot)."""
    samples, haps = [], {}
    for n in names:
        s, h = pansn(n)
        if s not in haps:
            samples.append(s)
            haps[s] = set()
        haps[s].add(h)
    slot, sample_of = {}, []
    for si, s in enumerate(samples):
        for h in sorted(haps[s], key=lambda x: -1 if x is None else x):
            slot[(s, h)] = len(sample_of)
            sample_of.append(si)
    return samples, [slot[pansn(n)] for n in names], sample_of


def ref_paths(names: Sequence[str], prefixes: Sequence[str]) -> List[int]:
    got = [k for k, n in enumerate(names) if any(n.startswith(p) for p in prefixes)]
    if not got:
        raise CallError("no path name starts with any of the reference prefixes " + ", ".join(prefixes))
    return got


def _spell(step, seqs, last_only=False) -> str:
    """The bases of `step` in its orientation (only the last one with last_only); a byte it spells that is no nucleotide
    code is refused."""
    s = seqs[step[0]]
    if last_only:
        s = s[-1:] if step[1] == 0 else s[:1]
    for c in s:
        if c not in _COMP:
            raise CallError(f"segment {step[0]}: byte {c!r} is no nucleotide code")
    return s if step[1] == 0 else "".join(_COMP[c] for c in reversed(s))


def called_sites(sites, paths) -> List[bool]:
    """called[q] of the definition (the reference paths are `paths`, a dict path index -> step list)."""
    segs = {r: {x[0] for x in p} for r, p in paths.items()}
    n = len(sites)
    skipped: Dict[int, bool] = {}

    def skip(q):
        if q not in skipped:
            p = sites[q]["parent"]
            skipped[q] = sites[q]["fam"] in SUBFLUBBLE or (p != NO_PARENT and skip(p))
        return skipped[q]
    present: Dict[int, set] = {}
    for st in sites:
        pr = present.setdefault(st["tree"], set())
        for r, sg in segs.items():
            if st["s"][0] in sg or st["z"][0] in sg:
                pr.add(r)
    callable_ = [False] * n
    for q, st in enumerate(sites):
        pr = present[st["tree"]]
        callable_[q] = (not skip(q) and bool(pr) and
                        all(st["s"][0] in segs[r] and st["z"][0] in segs[r] for r in pr))
    called = list(callable_)
    for q, st in enumerate(sites):
        if callable_[q] and st["parent"] != NO_PARENT:
            called[st["parent"]] = False
    return called


def call(sites, names, paths, seqs: Dict[int, str], prefixes, max_steps=TR.DEFAULT_MAX_STEPS):
    """Records of the definition, in file order.  paths: step lists in GFA order; seqs: segment id -> sequence."""
    refs = ref_paths(names, prefixes)
    samples, slot, sample_of = slots_of(names)
    index = TR.PathIndex(paths)
    called = called_sites(sites, {r: index.paths[r] for r in refs})
    isref = set(refs)
    off = {}
    for r in refs:
        o = [0]
        for x in index.paths[r]:
            o.append(o[-1] + len(seqs[x[0]]))
        off[r] = o
    recs = []
    for q, st in enumerate(sites):
        if not called[q]:
            continue
        alleles, travs, status = TR.traversals_of(index, st["s"], st["z"], max_steps)
        if len(alleles) < 2:
            continue
        by_slot: Dict[int, set] = {}
        for pi, _i, _j, _r, a in travs:
            by_slot.setdefault(slot[pi], set()).add(a)
        inner_len = [sum(len(seqs[x[0]]) for x in a[1:-1]) for a in alleles]
        anchored = min(inner_len) == 0
        for pi, first, _last, rev, ra in travs:
            if pi not in isref:
                continue
            order = [ra] + [a for a in range(len(alleles)) if a != ra]
            code = {a: k for k, a in enumerate(order)}
            texts, ats = [], []
            for a in order:
                steps = alleles[a] if not rev else [TR.flip(x) for x in reversed(alleles[a])]
                inner = steps[1:-1]
                body = "".join(_spell(x, seqs) for x in inner)
                if anchored:
                    texts.append(_spell(steps[0], seqs, True) + body)
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
            pos = off[pi][first + 1] + (0 if anchored else 1)
            vt = "SUB" if not anchored else "INS" if inner_len[ra] == 0 else "DEL"
            recs.append(dict(path=pi, q=q, first=first, chrom=names[pi], pos=pos, id=label(st["s"], st["z"]),
                             ref=texts[0], alts=texts[1:], at=ats, vartype=vt, tangled=tangled, lv=st["height"] - 1,
                             gt=gt, slots=gts, ac=ac, an=an, ns=ns))
    recs.sort(key=lambda r: (r["path"], r["pos"], r["q"], r["first"]))
    return recs


def record_line(r) -> str:
    info = (f"AC={','.join(map(str, r['ac']))};AF={','.join('%.1f' % (c / r['an']) for c in r['ac'])};AN={r['an']};"
            f"NS={r['ns']};AT={','.join(r['at'])};VARTYPE={r['vartype']};TANGLED={'T' if r['tangled'] else 'F'};"
            f"ES={r['id']};LV={r['lv']}")
    return "\t".join([r["chrom"], str(r["pos"]), r["id"], r["ref"], ",".join(r["alts"]), "60", "PASS", info, "GT"] + r["gt"])


def vcf_text(names, paths, seqs, recs, prefixes, date="00000000", only=None) -> str:
    """The VCF of `recs`: header, one contig line per reference path (those of prefix `only` when given), records."""
    samples, _, _ = slots_of(names)
    refs = ref_paths(names, prefixes if only is None else [only])
    out = [HEADER.format(date=date)]
    for r in refs:
        out.append(f"##contig=<ID={names[r]},length={sum(len(seqs[x[0]]) for x in paths[r])}>\n")
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples) + "\n")
    keep = set(refs)
    out += [record_line(r) + "\n" for r in recs if r["path"] in keep]
    return "".join(out)


def read_gfa(path: str):
    """(names, step lists, {segment id: sequence}) of a GFA's S and P lines."""
    names, paths, seqs = [], [], {}
    for ln in open(path):
        f = ln.rstrip("\n").split("\t")
        if f[0] == "S":
            seqs[int(f[1])] = f[2]
        elif f[0] == "P":
            names.append(f[1])
            paths.append([(int(x[:-1]), 0 if x[-1] == "+" else 1) for x in f[2].split(",") if x])
    return names, paths, seqs
