"""Plain-Python restatement of what the VCF checks do with the spanning allele `*` ("Spanning alleles", the
paragraph "VCF checks"), on top of vcfcheck_ref, which it does not change and which states everything else.

The rule, independent of the device's code: an AT entry that is the one character `*` is a walk without steps, not a bad
walk; an allele whose text (REF or ALT) is `*` is not searched and not spelled, and a task that names it reads found_fwd
whatever its AT entry, its column or its phase; every other task, and every record without such an allele, is
vcfcheck_ref's.  `parse` and `check` have vcfcheck_ref's signatures and results.
"""
from __future__ import annotations

import vcfcheck_ref as R

STAR = "*"


def _without_star_walks(text: str) -> str:
    """The text with every AT entry `*` emptied: vcfcheck_ref reads an empty entry as a walk without steps."""
    out = []
    for ln in text.split("\n"):
        f = ln.split("\t")
        if not ln.startswith("#") and len(f) >= 8:
            info = f[7].split(";")
            for k, kv in enumerate(info):
                if kv.startswith("AT="):
                    info[k] = "AT=" + ",".join("" if w == STAR else w for w in kv[3:].split(","))
                    break
            f[7] = ";".join(info)
            ln = "\t".join(f)
        out.append(ln)
    return "\n".join(out)


def parse(text: str) -> dict:
    return R.parse(_without_star_walks(text))


def is_star(rec: dict, allele: int) -> bool:
    return allele < len(rec["alleles"]) and rec["alleles"][allele]["text"] == STAR


def check(doc: dict, names, paths, segments, seqs=None, forward_only=False, spelling=False) -> dict:
    res = R.check(doc, names, paths, segments, seqs, forward_only=forward_only, spelling=spelling)
    status, spell = list(res["task_status"]), list(res["allele_spell"])
    out = dict(task_status=status, allele_spell=spell, rec_invalid=[], rec_reason=[], rec_allele=[], rec_task=[], n_status=[0] * 6,
               n_invalid=0, n_misspelled=0)
    t0 = a0 = 0
    for rec in doc["records"]:
        for k, (a, _c, _j) in enumerate(rec["tasks"]):
            if is_star(rec, a):
                status[t0 + k] = R.FOUND_FWD
        for a in range(len(rec["alleles"])):
            if is_star(rec, a):
                spell[a0 + a] = R.SPELL_NONE
        # the record's first failure in (allele, misspelled before its tasks, task) order, as vcfcheck_ref states it
        fails = [(a, 1, t0 + k, status[t0 + k]) for k, (a, _c, _j) in enumerate(rec["tasks"]) if status[t0 + k] > R.FOUND_REV]
        fails += [(a, 0, R.NIL, R.MISSPELLED) for a in range(len(rec["alleles"])) if spell[a0 + a] == R.SPELL_MISSPELLED]
        first = min(fails, key=lambda f: (f[0], f[1], f[2] if f[1] else 0)) if fails else None
        out["rec_invalid"].append(int(first is not None))
        out["rec_reason"].append(0xFF if first is None else first[3])
        out["rec_allele"].append(R.NIL if first is None else first[0])
        out["rec_task"].append(R.NIL if first is None else first[2])
        t0 += len(rec["tasks"])
        a0 += len(rec["alleles"])
    for st in status:
        out["n_status"][st] += 1
    out["n_invalid"] = sum(out["rec_invalid"])
    out["n_misspelled"] = spell.count(R.SPELL_MISSPELLED)
    return out
