"""Plain-Python restatement of the VCF checks ("VCF checks"), the yardstick of povu_hip_vcf_parse,
povu_hip_vcf_check, povu_hip_vcf_report_text and of `povu vcf --report`.

`parse` reads VCF text into the arrays of povu_hip_vcf_doc (plain lists), `check` gives every task its status, every allele its
spelling and every record its verdict and first failure, `report_text` / `summary_text` the two files.  Samples and slots are
those of the variant calls (vcf_ref.slots_of).
"""
from __future__ import annotations

import re
from typing import Dict, List, Sequence

import vcf_ref as V

FOUND_FWD, FOUND_REV, ABSENT, NO_AT, BAD_STEP, NO_SLOT, MISSPELLED = range(7)
STATUS_NAME = ["found_fwd", "found_rev", "absent", "no_at", "bad_step", "no_slot", "misspelled"]
SPELL_NONE, SPELL_WHOLE, SPELL_ANCHORED, SPELL_MISSPELLED = range(4)
NIL = 0xFFFFFFFF
_STEP = re.compile(r"([<>])(\d+)")


class VcfError(ValueError):
    pass


def walk_of(text: str):
    """The steps [(id, 0 '>' | 1 '<')] of a walk `[<>]id` repeated; None for a text that is no walk."""
    out, at = [], 0
    while at < len(text):
        m = _STEP.match(text, at)
        if not m or int(m.group(2)) >= NIL:
            return None
        out.append((int(m.group(2)), 0 if m.group(1) == ">" else 1))
        at = m.end()
    return out


def _number(s: str, most: int):
    return int(s) if s and len(s) <= 19 and all("0" <= c <= "9" for c in s) and int(s) <= most else None


def parse(text: str) -> dict:
    """The document: samples; per record line, pos, id, alleles (dicts: walk None without one in AT, text None beyond REF and
    the ALTs) and tasks (allele, column, phase) in (allele, column, phase) order."""
    samples, records, have_columns = [], [], False
    for no, ln in enumerate(text.split("\n"), 1):
        if ln.endswith("\r"):
            ln = ln[:-1]
        if not ln:
            continue
        if ln.startswith("#"):
            if ln == "#CHROM" or ln.startswith("#CHROM\t"):
                f = ln.split("\t")
                if have_columns:
                    raise VcfError(f"line {no}: a second #CHROM line")
                if len(f) < 8:
                    raise VcfError(f"line {no}: the #CHROM line needs at least 8 columns, this one has {len(f)}")
                samples, have_columns = f[9:], True
            continue
        if not have_columns:
            raise VcfError(f"line {no}: a record in front of the #CHROM line")
        f = ln.split("\t")
        if len(f) < 8:
            raise VcfError(f"line {no}: a record needs at least 8 columns, this one has {len(f)}")
        if len(f) > 8 and len(f) != 9 + len(samples):
            raise VcfError(f"line {no}: the #CHROM line names {len(samples)} sample columns, this record has {len(f) - 9}")
        pos = _number(f[1], 2 ** 64 - 1)
        if pos is None:
            raise VcfError(f"line {no}: POS is no number: {f[1]}")
        texts = [f[3]] + ([] if f[4] == "." else f[4].split(","))
        walks = []
        for kv in f[7].split(";"):
            if kv.startswith("AT="):
                walks = kv[3:].split(",")
                break
        alleles = []
        for a in range(max(len(texts), len(walks))):
            w = None
            if a < len(walks):
                w = walk_of(walks[a])
                if w is None:
                    raise VcfError(f"line {no}: AT walk {a} is no walk of [<>]id steps: {walks[a]}")
            alleles.append(dict(walk=w, text=texts[a] if a < len(texts) else None))
        tasks = []
        if len(f) > 8:
            keys = f[8].split(":")
            if "GT" in keys:
                at = keys.index("GT")
                for s in range(len(samples)):
                    sub = f[9 + s].split(":")
                    if at >= len(sub):
                        continue
                    for j, g in enumerate(re.split(r"[|/]", sub[at])):
                        if g == ".":
                            continue
                        a = _number(g, NIL - 1)
                        if a is None:
                            raise VcfError(f"line {no}: GT of sample column {s} is no genotype: {sub[at]}")
                        tasks.append((a, s, j))
        tasks.sort(key=lambda t: t[0])  # (stable: column, then phase within an allele)
        records.append(dict(line=no, pos=pos, id=f[2], alleles=alleles, tasks=tasks))
    return dict(samples=samples, records=records)


def doc_arrays(doc: dict) -> dict:
    """The flat arrays of povu_hip_vcf_doc."""
    o = dict(sample=list(doc["samples"]), rec_line=[], rec_pos=[], rec_id=[], allele_off=[0], task_off=[0], step_off=[0],
             text_off=[0], allele_walk=[], step_id=[], step_or=[], text="", task_record=[], task_allele=[], task_col=[],
             task_phase=[])
    for r, rec in enumerate(doc["records"]):
        o["rec_line"].append(rec["line"])
        o["rec_pos"].append(rec["pos"])
        o["rec_id"].append(rec["id"])
        for al in rec["alleles"]:
            for sid, so in al["walk"] or []:
                o["step_id"].append(sid)
                o["step_or"].append(so)
            o["text"] += al["text"] or ""
            o["allele_walk"].append((1 if al["walk"] is not None else 0) | (2 if al["text"] is not None else 0))
            o["step_off"].append(len(o["step_id"]))
            o["text_off"].append(len(o["text"]))
        for a, c, j in rec["tasks"]:
            o["task_record"].append(r)
            o["task_allele"].append(a)
            o["task_col"].append(c)
            o["task_phase"].append(j)
        o["allele_off"].append(len(o["allele_walk"]))
        o["task_off"].append(len(o["task_allele"]))
    return o


def slot_haps(names: Sequence[str]):
    """(samples, slot of every path, first slot and slots of every sample, hap number of every slot or None)."""
    samples, slot_of_path, sample_of = V.slots_of(names)
    first, count = [0] * len(samples), [0] * len(samples)
    for sl in reversed(range(len(sample_of))):
        first[sample_of[sl]] = sl
        count[sample_of[sl]] += 1
    hap = [None] * len(sample_of)
    for n, sl in zip(names, slot_of_path):
        hap[sl] = V.pansn(n)[1]
    return samples, slot_of_path, first, count, hap


def occurs(path, w) -> bool:
    """w occurs contiguously in `path`, entirely inside it."""
    m = len(w)
    return any(path[g:g + m] == w for g in range(len(path) - m + 1))


def _occurs_indexed(path, where, w) -> bool:
    """occurs(path, w), trying only the positions of w's first step (where: step -> positions of `path`)."""
    m = len(w)
    return any(path[g:g + m] == w for g in where.get(w[0], ()) if g + m <= len(path))


def flipped(w):
    return [(i, o ^ 1) for i, o in reversed(w)]


def _oriented(step, seqs):
    """The bases of a step as oriented, None when a byte it reads is no nucleotide code."""
    s = seqs[step[0]]
    if any(c not in V._COMP for c in s):
        return None
    return s if step[1] == 0 else "".join(V._COMP[c] for c in reversed(s))


def spelling_of(walk, text, seqs) -> int:
    parts = [_oriented(st, seqs) for st in walk]
    if all(p is not None for p in parts) and text == "".join(parts):
        return SPELL_WHOLE
    # anchored: the first step's last base as oriented (only that byte of it is read), then the other steps
    s0 = seqs[walk[0][0]]
    if s0:
        c = s0[-1] if walk[0][1] == 0 else s0[0]
        if c in V._COMP and all(p is not None for p in parts[1:]):
            if text == (c if walk[0][1] == 0 else V._COMP[c]) + "".join(parts[1:]):
                return SPELL_ANCHORED
    return SPELL_MISSPELLED


def check(doc: dict, names: Sequence[str], paths, segments, seqs: Dict[int, str] = None, forward_only=False, spelling=False) -> dict:
    """names, paths: of the graph's paths (step lists of (id, orientation)); segments: the segment ids the graph has; seqs:
    id -> sequence, for spelling."""
    samples, slot_of_path, first, count, hap = slot_haps(names)
    segments = set(segments)
    by_slot: Dict[int, list] = {}
    for p, sl in zip(paths, slot_of_path):
        p, where = [tuple(x) for x in p], {}
        for g, x in enumerate(p):
            where.setdefault(x, []).append(g)
        by_slot.setdefault(sl, []).append((p, where))
    out = dict(task_status=[], allele_spell=[], rec_invalid=[], rec_reason=[], rec_allele=[], rec_task=[], n_status=[0] * 6,
               n_invalid=0, n_misspelled=0)
    found: Dict[tuple, tuple] = {}
    n_tasks = 0
    for r, rec in enumerate(doc["records"]):
        spell = []
        for al in rec["alleles"]:
            w = al["walk"]
            ok = spelling and w and al["text"] is not None and all(s[0] in segments for s in w)
            spell.append(spelling_of(w, al["text"], seqs) if ok else SPELL_NONE)
        out["allele_spell"] += spell
        out["n_misspelled"] += spell.count(SPELL_MISSPELLED)
        first_fail = None  # (allele, 0 misspelled | 1 task, reason, task)
        for k, (a, c, j) in enumerate(rec["tasks"]):
            w = rec["alleles"][a]["walk"] if a < len(rec["alleles"]) else None
            name = doc["samples"][c]
            si = samples.index(name) if name in samples else None
            if not w:
                st = NO_AT
            elif any(s[0] not in segments for s in w):
                st = BAD_STEP
            elif si is None or j >= count[si]:
                st = NO_SLOT
            else:
                sl = first[si] + j
                key = (r, a, sl)
                if key not in found:
                    ps = by_slot.get(sl, [])
                    found[key] = (any(_occurs_indexed(p, i, w) for p, i in ps), any(_occurs_indexed(p, i, flipped(w)) for p, i in ps))
                fwd, rev = found[key]
                st = FOUND_FWD if fwd else FOUND_REV if rev and not forward_only else ABSENT
            out["task_status"].append(st)
            out["n_status"][st] += 1
            if st > FOUND_REV and first_fail is None:
                first_fail = (a, 1, st, n_tasks + k)
        n_tasks += len(rec["tasks"])
        if SPELL_MISSPELLED in spell:
            m = (spell.index(SPELL_MISSPELLED), 0, MISSPELLED, NIL)
            if first_fail is None or m < first_fail:
                first_fail = m
        out["rec_invalid"].append(int(first_fail is not None))
        out["n_invalid"] += first_fail is not None
        out["rec_reason"].append(0xFF if first_fail is None else first_fail[2])
        out["rec_allele"].append(NIL if first_fail is None else first_fail[0])
        out["rec_task"].append(NIL if first_fail is None else first_fail[3])
    return out


def report_text(doc: dict, res: dict, names: Sequence[str]) -> str:
    samples, _, first, count, hap = slot_haps(names)
    flat = [t for rec in doc["records"] for t in rec["tasks"]]
    out = ["rec_idx\tID\tPOS\tAT\tHap ID\tsample\treason\n"]
    for r, rec in enumerate(doc["records"]):
        if not res["rec_invalid"][r]:
            continue
        a, reason = res["rec_allele"][r], res["rec_reason"][r]
        w = rec["alleles"][a]["walk"] if a < len(rec["alleles"]) else None
        at = "".join((">" if o == 0 else "<") + str(i) for i, o in w or [])
        if reason == MISSPELLED:
            h, name = ".", "."
        else:
            _, c, j = flat[res["rec_task"][r]]
            name = doc["samples"][c]
            h = 1
            if name in samples and j < count[samples.index(name)] and hap[first[samples.index(name)] + j] is not None:
                h = hap[first[samples.index(name)] + j]
        out.append(f"{r}\t{rec['id']}\t{rec['pos']}\t{at}\t{h}\t{name}\t{STATUS_NAME[reason]}\n")
    return "".join(out)


def summary_text(doc: dict, res: dict) -> str:
    bad = sum(res["rec_invalid"])
    return "No errors\n" if not bad else "Error rate: %.2f%%\n" % (bad / len(doc["records"]) * 100)
