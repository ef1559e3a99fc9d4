"""Plain-Python restatement of the clustered calls ("Clustered calls"), the yardstick of
povu_hip_call_clustered, HipDecomposer.call(cluster=...) and `povu call --cluster`.

Built on vcf_ref (called sites, slots, spelling, POS) and traversals_ref (traversals and exact alleles); composed with
inversions_ref and region_ref at the places the definition names.  The rule itself is restated with collections.Counter and
Python integers: `parse` reads F to T = F * 10^6, `frac` gives (I, U) of two bags, `similar`, `better` and `sim_ppm` compare
them, `prunable` is the weight bound, `leader` clusters the bags of one site.  `call_full` gives the records (the dicts of
vcf_ref.call plus n_classes, ref_class, ref_exact, ref_is_rep, nx, minsim, clustered) and the counters, `call` the records and
the VCF text of a mode.
"""
from __future__ import annotations

from collections import Counter
from typing import Dict, List

import inversions_ref as I
import region_ref as R
import traversals_ref as TR
import vcf_ref as V

PPM = 10 ** 6
NX_LINE = ('##INFO=<ID=NX,Number=R,Type=Integer,Description="Exact alleles of the site behind every written allele, the cluster of REF '
           'first">\n')
MINSIM_LINE = ('##INFO=<ID=MINSIM,Number=1,Type=Integer,Description="Lowest similarity, in parts per million, of an exact allele of the '
               'site to the representative of its cluster">\n')
COUNTERS = ("n_cluster_sites", "n_clustered_sites", "n_cluster_vanished", "n_cluster_keys", "n_cluster_pairs", "n_cluster_pruned")


class ClusterError(ValueError):
    pass


def parse(text: str) -> int:
    """F as decimal text, at most six decimals, 0 < F <= 1 -> T."""
    what = f"cluster threshold '{text}'"
    ip, dot, fp = text.partition(".")
    if any(c not in "0123456789" for c in ip + fp) or not ip + fp:
        raise ClusterError(what + ": expected a decimal number such as 0.9")
    if len(fp) > 6:
        raise ClusterError(what + ": more than six decimals")
    t = int(ip or "0") * PPM + int((fp + "000000")[:6])
    if not 0 < t <= PPM:
        raise ClusterError(what + ": must be above 0 and at most 1")
    return t


def header_line(t: int) -> str:
    return f"##povu_call_cluster={t // PPM}.{t % PPM:06d}\n"


def weight_of(bag: Counter, w: Dict[int, int]) -> int:
    return sum(c * w[v] for v, c in bag.items())


def frac(a: Counter, b: Counter, w: Dict[int, int]):
    i = sum(min(c, b[v]) * w[v] for v, c in a.items())
    return i, weight_of(a, w) + weight_of(b, w) - i


def _canon(f):
    return (1, 1) if f[1] == 0 else f


def similar(f, t: int) -> bool:
    i, u = _canon(f)
    return i * PPM >= t * u


def better(f, g) -> bool:
    (i, u), (j, v) = _canon(f), _canon(g)
    return i * v > j * u


def sim_ppm(f) -> int:
    i, u = _canon(f)
    return i * PPM // u


def prunable(wa: int, wr: int, t: int, best) -> bool:
    """The pair is not read: I <= min(wa, wr) and U >= max(wa, wr) already rule it out, or cannot beat the best held."""
    bound = (min(wa, wr), max(wa, wr))
    return not similar(bound, t) or (best is not None and not better(bound, best))


def leader(bags: List[Counter], w: Dict[int, int], t: int, no_bound=False):
    """(cluster of every allele, representatives, minsim, pairs, pruned) of one site's bags, alleles in order."""
    of, rep, low, pairs, pruned = [], [], PPM, 0, 0
    for a, bag in enumerate(bags):
        best, at = None, None
        for k, r in enumerate(rep):
            pairs += 1
            if not no_bound and prunable(weight_of(bag, w), weight_of(bags[r], w), t, best):
                pruned += 1
                continue
            f = frac(bag, bags[r], w)
            if similar(f, t) and (best is None or better(f, best)):
                best, at = f, k
        if best is None:
            of.append(len(rep))
            rep.append(a)
        else:
            of.append(at)
            low = min(low, sim_ppm(best))
    return of, rep, low, pairs, pruned


def bag_of(allele) -> Counter:
    """The segments of the inner steps of an exact allele (its steps S -> Z), orientation ignored."""
    return Counter(x[0] for x in allele[1:-1])


def site_clusters(sites, names, paths, seqs, prefixes, t, max_steps=TR.DEFAULT_MAX_STEPS, no_bound=False):
    """Per called site of two exact alleles or more: q -> (exact alleles, traversals, status, of, rep, minsim, pairs, pruned)."""
    refs = V.ref_paths(names, prefixes)
    index = TR.PathIndex(paths)
    called = V.called_sites(sites, {r: index.paths[r] for r in refs})
    w = {v: len(s) for v, s in seqs.items()}
    out = {}
    for q, st in enumerate(sites):
        if not called[q]:
            continue
        alleles, travs, status = TR.traversals_of(index, st["s"], st["z"], max_steps)
        if len(alleles) < 2:
            continue
        out[q] = (alleles, travs, status) + leader([bag_of(a) for a in alleles], w, t, no_bound)
    return out


def call_full(sites, names, paths, seqs: Dict[int, str], prefixes, t: int, max_steps=TR.DEFAULT_MAX_STEPS, no_bound=False):
    refs = V.ref_paths(names, prefixes)
    samples, slot, sample_of = V.slots_of(names)
    index = TR.PathIndex(paths)
    isref = set(refs)
    off = {}
    for r in refs:
        o = [0]
        for x in index.paths[r]:
            o.append(o[-1] + len(seqs[x[0]]))
        off[r] = o
    found = site_clusters(sites, names, paths, seqs, prefixes, t, max_steps, no_bound)
    counters = dict.fromkeys(COUNTERS, 0)
    recs = []
    for q, (alleles, travs, status, cls, rep, minsim, pairs, pruned) in sorted(found.items()):
        st = sites[q]
        counters["n_cluster_sites"] += 1
        counters["n_cluster_keys"] += sum(len(a) - 2 for a in alleles)
        counters["n_cluster_pairs"] += pairs
        counters["n_cluster_pruned"] += pruned
        if len(rep) < 2:
            counters["n_cluster_vanished"] += 1
            continue
        clustered = len(rep) < len(alleles)
        counters["n_clustered_sites"] += clustered
        size = Counter(cls)
        by_slot: Dict[int, set] = {}
        for pi, _i, _j, _r, a in travs:
            by_slot.setdefault(slot[pi], set()).add(cls[a])
        inner_len = [sum(len(seqs[x[0]]) for x in a[1:-1]) for a in alleles]
        for pi, first, last, rev, ra in travs:
            if pi not in isref:
                continue
            rc = cls[ra]
            others = [c for c in range(len(rep)) if c != rc]
            order = [ra] + [rep[c] for c in others]
            code = {c: k for k, c in enumerate([rc] + others)}
            anchored = min(inner_len[a] for a in order) == 0
            texts, ats = [], []
            for a in order:
                steps = alleles[a] if not rev else [TR.flip(x) for x in reversed(alleles[a])]
                inner = steps[1:-1]
                body = "".join(V._spell(x, seqs) for x in inner)
                if anchored:
                    texts.append(V._spell(steps[0], seqs, True) + body)
                    ats.append(TR.as_text([steps[0]] + inner))
                else:
                    texts.append(body)
                    ats.append(TR.as_text(inner))
            gts, tangled = [], status != 0  # (clustering alone does not set TANGLED)
            for sl in range(len(sample_of)):
                got = {rc} if sl == slot[pi] else by_slot.get(sl, set())
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
            lab = V.label(st["s"], st["z"])
            recs.append(dict(path=pi, q=q, first=first, last=last, chrom=names[pi], pos=pos, id=lab, ref=texts[0], alts=texts[1:], at=ats,
                             vartype=vt, tangled=tangled, anchored=anchored, lv=st["height"] - 1, gt=gt, slots=gts, ac=ac, an=an, ns=ns,
                             ref_class=rc, n_classes=len(rep), n_exact=len(alleles), ref_exact=ra, ref_is_rep=rep[rc] == ra,
                             clustered=clustered, nx=[size[rc]] + [size[c] for c in others], minsim=minsim))
    recs.sort(key=lambda r: (r["path"], r["pos"], r["q"], r["first"]))
    return recs, counters


def record_line(r) -> str:
    line = V.record_line(r)
    if not r.get("clustered"):
        return line
    f = line.split("\t")
    f[7] += f";NX={','.join(map(str, r['nx']))};MINSIM={r['minsim']}"
    return "\t".join(f)


def head_text(names, paths, seqs, prefixes, t, date="00000000", only=None) -> str:
    """vcf_ref's header, the two INFO lines and the threshold's line, the contig lines, the column line."""
    plain = V.vcf_text(names, paths, seqs, [], prefixes, date=date, only=only)
    at = plain.index("##contig")
    return plain[:at] + NX_LINE + MINSIM_LINE + header_line(t) + plain[at:]


def call(sites, names, paths, seqs, prefixes, t, regions=None, inversions=False, date="00000000", no_bound=False):
    """(records written, VCF text, counters) of the clustered call; with `inversions` the SUBR records merged in untouched,
    with `regions` the records of the passing sites and inversions alone."""
    recs, counters = call_full(sites, names, paths, seqs, prefixes, t, no_bound=no_bound)
    line = record_line
    if inversions:
        recs = I.merge(recs, I.records(names, paths, seqs, prefixes)[0])
        line = lambda r: I.record_line(r) if r["vartype"] == "SUBR" else record_line(r)  # noqa: E731
    if regions is not None:
        recs = R.select(recs, sites, names, paths, seqs, regions)
    return recs, head_text(names, paths, seqs, prefixes, t, date) + "".join(line(r) + "\n" for r in recs), counters
