"""Plain-Python restatement of the nested calls ("Nested calls"), the yardstick of povu_hip_call with
POVU_HIP_T_NESTED and of `povu call --nested`.

Built on vcf_ref (called sites, slots, spelling, POS) and traversals_ref (traversals and exact alleles).  A traversal
encloses another of the same path by geometry alone; the steps of an allele that enclosed traversals cover are left out
of its skeleton; the exact alleles of a site with equal skeletons are one class, and records count classes.  `call_full`
gives the records (the dicts of vcf_ref.call plus level, parent, collapsed, rescued, ref_exact, info) and the counters,
`call` the records alone, `vcf_text` the VCF.
"""
from __future__ import annotations

import bisect
from typing import Dict, List

import traversals_ref as TR
import vcf_ref as V

PROFILES = ("raw-graph", "top-level-only", "popped")
PS_LINE = '##INFO=<ID=PS,Number=1,Type=String,Description="ID of the enclosing record of the same reference path">\n'
_DESC = {
    "ORIGIN": "Raw record id",
    "PARENT": "Raw parent record id",
    "PROFILE": "Downstream profile name",
    "PASSTHROUGH": "Record was kept without allele rewrite",
    "RESCUED_CHILD": "Child was kept because its parent was popped",
    "POPPED_PARENT": "Popped parent id that enabled rescue",
}
PROFILE_KEYS = {
    "top-level-only": ("ORIGIN", "PROFILE", "PASSTHROUGH"),
    "popped": ("ORIGIN", "PARENT", "PROFILE", "PASSTHROUGH", "RESCUED_CHILD", "POPPED_PARENT"),
}


def profile_lines(profile) -> str:
    return "".join(f'##INFO=<ID={k},Number=1,Type=String,Description="{_DESC[k]}">\n' for k in PROFILE_KEYS.get(profile, ()))


def encloses(t, u) -> bool:
    """t = (q, path, f, l) encloses u."""
    return t[1] == u[1] and t[0] != u[0] and t[2] <= u[2] and u[3] <= t[3] and u[3] - u[2] < t[3] - t[2]


def skeleton(t, rev, path_steps, by_path):
    """The steps of traversal t = (q, path, f, l) at uncovered positions, S -> Z (by_path: the called sites' traversals of
    every path as (f, q, path, l), sorted: an enclosed one starts within [f, l])."""
    q, pi, f, l = t
    row = by_path.get(pi, [])
    inside = []
    for k in range(bisect.bisect_left(row, (f,)), len(row)):
        if row[k][0] > l:
            break
        u = (row[k][1], pi, row[k][0], row[k][3])
        if encloses(t, u):
            inside.append(u)
    keep = [k for k in range(f, l + 1) if not any(u[2] < k < u[3] for u in inside)]
    steps = [path_steps[k] for k in keep]
    return tuple(TR.flip(x) for x in reversed(steps)) if rev else tuple(steps)


def call_full(sites, names, paths, seqs: Dict[int, str], prefixes, max_steps=TR.DEFAULT_MAX_STEPS, profile=None,
              max_level=0, max_ref_length=0, max_allele_length=0):
    if profile is not None and profile not in PROFILES:
        raise V.CallError(f"unknown profile {profile}")
    refs = V.ref_paths(names, prefixes)
    samples, slot, sample_of = V.slots_of(names)
    index = TR.PathIndex(paths)
    called = V.called_sites(sites, {r: index.paths[r] for r in refs})
    isref = set(refs)
    off = {}
    for r in refs:
        o = [0]
        for x in index.paths[r]:
            o.append(o[-1] + len(seqs[x[0]]))
        off[r] = o
    found = {q: TR.traversals_of(index, st["s"], st["z"], max_steps) for q, st in enumerate(sites) if called[q]}
    by_path: Dict[int, list] = {}
    for q, (_al, travs, _st) in found.items():
        for pi, f, l, _rev, _a in travs:
            by_path.setdefault(pi, []).append((f, q, pi, l))
    for row in by_path.values():
        row.sort()
    recs, n_collapsed = [], 0
    for q, st in enumerate(sites):
        if not called[q]:
            continue
        alleles, travs, status = found[q]
        if len(alleles) < 2:
            continue
        # classes: skeleton of every exact allele, from its first traversal
        cls, rep, seen = [None] * len(alleles), [], {}
        for pi, f, l, rev, a in travs:
            if cls[a] is not None:
                continue
            sk = skeleton((q, pi, f, l), rev, index.paths[pi], by_path)
            if sk not in seen:
                seen[sk] = len(rep)
                rep.append(a)
            cls[a] = seen[sk]
        assert all(c is not None for c in cls) and rep == sorted(rep)
        if len(rep) < 2:
            continue
        collapsed = len(rep) < len(alleles)
        n_collapsed += collapsed
        by_slot: Dict[int, set] = {}
        for pi, _i, _j, _r, a in travs:
            by_slot.setdefault(slot[pi], set()).add(cls[a])
        inner_len = [sum(len(seqs[x[0]]) for x in a[1:-1]) for a in alleles]
        for pi, first, last, rev, ra in travs:
            if pi not in isref:
                continue
            rc = cls[ra]
            order = [ra] + [rep[c] for c in range(len(rep)) if c != rc]
            code = {rc: 0}
            for c in range(len(rep)):
                if c != rc:
                    code[c] = len(code)
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
            gts, tangled = [], status != 0 or collapsed
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
            recs.append(dict(path=pi, q=q, first=first, last=last, chrom=names[pi], pos=pos, id=lab, es=lab, ref=texts[0],
                             alts=texts[1:], at=ats, vartype=vt, tangled=tangled, anchored=anchored, gt=gt, slots=gts, ac=ac, an=an,
                             ns=ns, ref_class=rc, n_classes=len(rep), ref_exact=ra, ref_is_rep=rep[rc] == ra, collapsed=collapsed,
                             height=st["height"], rescued=False, info=[]))
    recs.sort(key=lambda r: (r["path"], r["pos"], r["q"], r["first"]))
    # parent, level
    rows: Dict[int, list] = {}
    for k, r in enumerate(recs):
        rows.setdefault(r["path"], []).append((r["first"], k))
    span = max([r["last"] - r["first"] for r in recs], default=0)
    for row in rows.values():
        row.sort()
    for r in recs:
        t = (r["q"], r["path"], r["first"], r["last"])
        best, row = None, rows[r["path"]]
        for j in range(bisect.bisect_right(row, (r["first"], len(recs))) - 1, -1, -1):  # (an enclosing one starts at or before)
            if row[j][0] + span < r["last"]:
                break
            k = row[j][1]
            p = recs[k]
            u = (p["q"], p["path"], p["first"], p["last"])
            if encloses(u, t) and (best is None or (u[3] - u[2], u[0]) < best[0]):
                best = ((u[3] - u[2], u[0]), k)
        r["parent_rec"] = None if best is None else best[1]
        r["parent"] = None if best is None else recs[best[1]]["q"]
        r["ps"] = None if best is None else recs[best[1]]["es"]

    def level(k):
        r = recs[k]
        if "lv" not in r:
            r["lv"] = r["height"] - 1 if r["parent_rec"] is None else level(r["parent_rec"]) + 1
        return r["lv"]
    for k in range(len(recs)):
        r = recs[k]
        r["level"] = level(k)
    counters = dict(n_enclosed=sum(r["parent"] is not None for r in recs), n_collapsed_sites=n_collapsed, n_popped=0, n_rescued=0)
    if profile in (None, "raw-graph"):
        return recs, counters

    def big(r):
        return bool((max_ref_length and len(r["ref"]) > max_ref_length) or
                    (max_allele_length and any(len(x) > max_allele_length for x in [r["ref"]] + r["alts"])))
    kept = []
    if profile == "top-level-only":
        for r in recs:
            if r["lv"] == 0:
                r["info"] = [("ORIGIN", r["es"]), ("PROFILE", profile), ("PASSTHROUGH", "T")]
                r["id"] = r["es"] + ":top"
                kept.append(r)
    else:
        def reach(k):
            r = recs[k]
            if "reach" not in r:
                p = r["parent_rec"]
                r["reach"] = r["lv"] <= max_level or (p is not None and big(recs[p]) and reach(p))
            return r["reach"]
        for k, r in enumerate(recs):
            if not reach(k):
                continue
            if big(r):
                counters["n_popped"] += 1
                continue
            if r["lv"] > max_level:
                r["rescued"] = True
                counters["n_rescued"] += 1
                r["id"] = r["es"] + ":rescued"
                r["info"] = [("ORIGIN", r["es"]), ("PARENT", r["ps"]), ("PROFILE", profile), ("RESCUED_CHILD", "T"),
                             ("POPPED_PARENT", r["ps"])]
            else:
                r["info"] = [("ORIGIN", r["es"]), ("PROFILE", profile), ("PASSTHROUGH", "T")]
            kept.append(r)
    return kept, counters


def call(*a, **k) -> List[dict]:
    return call_full(*a, **k)[0]


def record_line(r) -> str:
    info = (f"AC={','.join(map(str, r['ac']))};AF={','.join('%.1f' % (c / r['an']) for c in r['ac'])};AN={r['an']};"
            f"NS={r['ns']};AT={','.join(r['at'])};VARTYPE={r['vartype']};TANGLED={'T' if r['tangled'] else 'F'};"
            f"ES={r['es']};LV={r['lv']}")
    if r["ps"] is not None:
        info += f";PS={r['ps']}"
    for k, v in r["info"]:
        info += f";{k}={v}"
    return "\t".join([r["chrom"], str(r["pos"]), r["id"], r["ref"], ",".join(r["alts"]), "60", "PASS", info, "GT"] + r["gt"])


def vcf_text(names, paths, seqs, recs, prefixes, date="00000000", only=None, profile=None) -> str:
    """The VCF of `recs` (of call with the same profile): vcf_ref's header, the PS line, the profile's INFO lines, the contig
    lines, the records."""
    samples, _, _ = V.slots_of(names)
    refs = V.ref_paths(names, prefixes if only is None else [only])
    out = [V.HEADER.format(date=date), PS_LINE, profile_lines(profile)]
    for r in refs:
        out.append(f"##contig=<ID={names[r]},length={sum(len(seqs[x[0]]) for x in paths[r])}>\n")
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples) + "\n")
    keep = set(refs)
    out += [record_line(r) + "\n" for r in recs if r["path"] in keep]
    return "".join(out)
