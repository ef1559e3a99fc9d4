"""Inputs of the decomposed calls' GPU tests (tests/test_gpu_prim.py) and the conditions they must meet, which
tests/test_prim_inputs.py checks on the restatement alone (tests/prim_ref.py), without a GPU."""
import random

import prim_ref as PR
from povu_amd import workloads as W
from test_gpu_norm import chain

COMPLEX_UNITS, COMPLEX_HAPS, COMPLEX_CAP, COMPLEX_SEEDS = 200, 6, 10, (1, 2, 3)
CHAIN_HAPS = 6
CHAIN_REFS = ["hap0", "back"]


def edited(text, rng, n_edits=3):
    """`text` with n_edits bases changed, inserted or deleted."""
    b = list(text)
    for _ in range(n_edits):
        r, p = rng.random(), rng.randrange(len(b))
        if r < .4:
            b[p] = "ACGT"[("ACGT".index(b[p].upper()) + 1 + rng.randrange(3)) % 4]
        elif r < .7:
            b[p:p] = [rng.choice("ACGT") for _ in range(rng.randint(1, 2))]
        else:
            del b[p:p + rng.randint(1, 2)]
    return "".join(b)


def chain_case():
    """(graph, sequences, paths) of a chain whose bubbles carry what the striped sweep, the anchors and the row rules can get
    wrong.  Haplotype h takes allele h % (number of choices) of every bubble, so haplotype 0, the reference, always the first;
    one more path walks the reference backwards."""
    rng = random.Random(20261018)
    text = lambda n: "".join(rng.choice("AACCGT") for _ in range(n))  # noqa: E731
    items = [("s", "A", 0), ("b", ["A"], True)]  # POS 1, anchored: REF AA, ALT A deletes at offset 0 (contig_start)
    items += [("s", "TG", 0), ("b", ["AA", "A", "AAA"], False)]  # an indel at offset 0 behind ...
    items += [("s", "G", 0), ("b", ["CC", "C", "ACC"], False)]  # ... a one-base segment
    items += [("s", "CT", 1), ("b", ["TT", "T"], False)]  # ... a '-' step
    for n in (63, 64, 65, 128, 129, 512):  # texts on and around the stripes and at the cap
        a = text(n)
        shorter = a[1:] if n in (64, 512) else edited(a, rng)
        items += [("s", text(3), 0), ("b", [a, shorter[:n], edited(a, rng)[:n], a[:n // 2].lower() + a[n // 2:]], False)]
    a = text(513)
    items += [("s", "GA", 0), ("b", [a, a[:200] + "T" + a[201:], "ACG"], False)]  # one base too long: kept whole
    items += [("s", "CA", 0), ("b", ["ACGT", "AGGT", "AGGA", "ACT", "acgt"], False)]  # four ALTs, two with the same SNP, one REF's text
    items += [("s", "TC", 0), ("b", ["A", "C"], False)]  # one ALT, one base: the raw record
    items += [("s", "TG", 0), ("b", ["TT"], True)]  # one ALT, an anchored deletion: the raw record
    items += [("s", "ca", 0), ("b", ["gattaca", "GATCACA", "gtaca"], False)]  # lower case
    items += [("s", "", 0), ("b", ["AC"], True)]  # an empty anchor: an empty ALT
    # rows that change places: the second ALT's SNP lies in front of the first's, and the next record (behind an empty flank)
    # begins with a deletion anchored on the base the first ALT changes
    items += [("s", "GG", 0), ("b", ["ACGTACGTAC", "ACGTACGTAT", "TCGTACGTAC"], False), ("s", "", 0), ("b", ["GG", "G"], False)]
    items += [("s", "TT", 0)]
    haps = []
    for h in range(CHAIN_HAPS):
        choice = []
        for it in items:
            if it[0] == "b":
                opts = list(range(1, len(it[1]) + 1)) + ([0] if it[2] else [])
                choice.append(opts[h % len(opts)])
        haps.append(choice)
    return chain(items, haps, reversed_copy=True)


def complex_case(seed):
    g, seqs = W.complex_alleles(COMPLEX_UNITS, seed)
    return g, seqs, W.complex_haplotypes(COMPLEX_UNITS, seed, COMPLEX_HAPS)


def coverage(rows):
    """What a differential case must hold, on the restatement's rows."""
    kinds = {r["kind"] for r in rows}
    assert {PR.ROW_RAW, PR.ROW_SNP, PR.ROW_INS, PR.ROW_DEL, PR.ROW_PASS} <= kinds, kinds
    assert any(r["kind"] in (PR.ROW_INS, PR.ROW_DEL) and r["ref_start"] == 0 and r["lead"] for r in rows)  # anchored on the context


def chain_coverage(rows, recs, rows_with_inversions):
    """... of the chain case: all five reasons.  Four arise in the call by both references; the fifth, SUBR, needs the
    inversion records, which are called against the forward reference alone (rows_with_inversions: that call's rows)."""
    coverage(rows)
    assert PR.REASON_SUBR in {r["reason"] for r in rows_with_inversions}
    assert {r["reason"] for r in rows} == {PR.REASON_NONE, PR.REASON_MAX_ALLELE_LENGTH, PR.REASON_CONTIG_START, PR.REASON_EMPTY_ALLELE,
                                           PR.REASON_EQUALS_REF}
    lens = {len(r["ref"]) for r in recs} | {len(a) for r in recs for a in r["alts"]}
    assert {63, 64, 65, 128, 129, 512, 513} <= lens
    assert any(len(r["alts"]) == 4 for r in recs) and len({r["path"] for r in recs}) == 2
    assert any(r["ref"] != r["ref"].upper() for r in recs)
    # the sort moves rows: within a record, and two records meet at one POS
    made = sorted(rows, key=lambda x: (x["rec"], x["alt"], x["order"]))
    assert made != rows
    assert any(a["path"] == b["path"] and a["pos"] == b["pos"] and a["rec"] != b["rec"] for a, b in zip(rows, rows[1:]))
