"""Inputs of the merged primitives' tests (tests/test_gpu_merge.py, tests/test_merge_ref.py) and the conditions they must meet,
stated on the restatement's output (tests/merge_ref.py) as prim_cases.coverage states those of the decomposed calls."""
import itertools

import merge_ref as MR
import prim_ref as PR
from povu_amd import workloads as W
from test_gpu_norm import chain

CHAIN_HAPS = 70  # more than 64 samples: the lane-per-sample loop of the vote takes a second trip
CHAIN_CAP = 8  # max_allele_length of the chain's calls: one ALT is longer and is kept whole
CHAIN_REFS = ["hap0#"]
MANY = 65  # ALTs of one bubble that share a primitive: a group of more than 64 members


def chain_case():
    """(graph, sequences, paths) of a chain of nine bubbles.  Haplotype h takes allele h % (number of choices) of every bubble,
    haplotype 0, the reference, always the first."""
    items = [("s", "GATTACA", 0)]
    # an SNP shared by ALTs 1 and 2, the second with one more SNP; another base at the same POS; the first again in lower case;
    # an insertion anchored on the base the SNP changes
    items += [("b", ["ACGTAC", "AGGTAC", "AGGTAT", "ATGTAC", "AgGTAC", "ACTGTAC"], False)]
    # an SNP at offset 5; a deletion of offsets 3 .. 5, which covers it; one of offsets 2 .. 4, which ends one base short
    items += [("s", "TT", 0), ("b", ["ACGTTCAG", "ACGTTGAG", "ACGAG", "ACCAG"], False)]
    # a text over the cap beside an SNP
    items += [("s", "CA", 0), ("b", ["ACG", "ATG", "ACGTTTTTTTTT"], False)]
    # MANY ALTs that share the SNP at offset 0 and differ in one or two bases behind it
    ref = "ACGTACGT"
    alts = []
    for n in (1, 2):
        for at in itertools.combinations(range(2, 8), n):
            for sub in itertools.product((1, 2, 3), repeat=n):
                b = list("T" + ref[1:])
                for p, d in zip(at, sub):
                    b[p] = "ACGT"[("ACGT".index(ref[p]) + d) % 4]
                alts.append("".join(b))
    items += [("s", "GC", 0), ("b", [ref] + alts[:MANY], False)]
    # two records that meet at one POS: a deletion anchored on the base an SNP of the record before changes
    items += [("s", "GG", 0), ("b", ["ACGTACGA", "ACGTACGT"], False), ("s", "", 0), ("b", ["CC", "C"], False)]
    # a record that stays the raw line (the reference skips the bubble: A -> AT) and, behind an empty flank, a record whose
    # insertion at offset 0 is anchored on that A: the same primitive, the raw line first.  Both have two choices, so a
    # haplotype carries both insertions or neither
    items += [("s", "GA", 0), ("b", ["T"], True), ("s", "", 0), ("b", ["CC", "TCC"], False)]
    # twenty insertions of five bases behind one anchor: one POS, the same two lengths, more texts than a four-bit hash has
    # values, so that under POVU_HIP_TRAV_HASH_BITS=4 two of them must collide
    items += [("s", "CA", 0), ("b", ["AC"] + ["A" + "".join(t) + "C" for t in itertools.product("GT", repeat=5)][:20], False)]
    items += [("s", "TT", 0)]
    haps = []
    for h in range(CHAIN_HAPS):
        opts = [([0] if it[2] else []) + list(range(1, len(it[1]) + 1)) for it in items if it[0] == "b"]
        haps.append([o[h % len(o)] for o in opts])
    return chain(items, haps)


def skip_case(units=12, depth=1, haps=8, seed=9):
    """skip_nested under a plain call: the outer site of a unit spells its inner sites' SNPs inside its own alleles, so equal
    primitives come from different records.  Every level of the nesting has a letter of its own (K: a unit's entry and exit, G:
    those of the units inside it, T or W: what lies inside those, A / C or R / Y: the two branches of an SNP), so that a skipped unit aligns
    as one deletion of the same bases in the record of every site that spells it: the rightmost match of the base in front of
    it is that base itself.  With random sequences the alignments of an outer and an inner record place the same skip
    differently, and the genotypes they vote for contradict each other.  The same happens where the reference skips one inner
    unit and a haplotype the other (the outer record's alignment substitutes one unit for the other): the seed is one whose
    haplotypes keep the invariants of tests/test_merge_ref.py, which asserts them."""
    g = W.skip_nested(units, depth, seed)
    anc, snp, _, _, _ = W._skip_template(depth, 2)
    inner = sorted({a[1] for a in anc if len(a) > 1})  # the units inside a unit: each its own letters, so that none aligns as another
    unit = ["KG"[len(a)] if len(a) < 2 else ("AC", "RY")[inner.index(a[1]) % 2][s[1]] if s[0] >= 0 else "TW"[inner.index(a[1]) % 2]
            for a, s in zip(anc, snp)]
    return g, unit * units, W.skip_haplotypes(units, depth, haps, seed)


def carrying(rows, merged, counters):
    """What every differential input must hold."""
    assert counters["n_merged_groups"] >= 1 and counters["n_ref_consistent"] >= 1, counters
    assert counters["n_gt_conflicts"] == 0, counters
    assert counters["n_merged_members"] == sum(len(m["members"]) for m in merged if len(m["members"]) > 1)
    assert sorted(x for m in merged for x in m["members"]) == list(range(len(rows)))


def chain_coverage(recs, rows, merged, counters):
    """... and the chain: every case named in its docstring arises."""
    carrying(rows, merged, counters)
    key = lambda x: MR.row_key(rows[x], recs)  # noqa: E731
    pair = lambda x: (rows[x]["rec"], rows[x]["alt"])  # noqa: E731
    n_of_pair = {}
    for r in rows:
        n_of_pair[(r["rec"], r["alt"])] = n_of_pair.get((r["rec"], r["alt"]), 0) + 1
    groups = [m["members"] for m in merged]
    # one primitive shared by two ALTs of a record, one of which has a second primitive
    assert any(len(g) >= 2 and len({rows[x]["rec"] for x in g}) == 1 and any(n_of_pair[pair(x)] >= 2 for x in g) for g in groups)
    # equal POS and REF, another ALT: two groups
    heads = [key(g[0]) for g in groups if rows[g[0]]["kind"] != PR.ROW_PASS]
    assert any(a[:3] == b[:3] and a[3] != b[3] for a, b in itertools.combinations(heads, 2))
    # texts equal only after upper-casing
    assert any(len({MR.texts_of(rows[x], recs) for x in g}) >= 2 for g in groups)
    # an INS and an SNP at one POS
    kinds_at = {}
    for r in rows:
        kinds_at.setdefault((r["path"], r["pos"]), set()).add(r["kind"])
    assert any({PR.ROW_INS, PR.ROW_SNP} <= k for k in kinds_at.values())
    # a deletion that covers another ALT's SNP ('.'), one that ends one base short of it (0)
    dels = [x for x, r in enumerate(rows) if r["kind"] == PR.ROW_DEL]
    snps = [m for m in merged if rows[m["members"][0]]["kind"] == PR.ROW_SNP]
    covered = short = False
    for m in snps:
        a, _ = MR.span_of(rows[m["members"][0]], recs)
        for x in dels:
            if rows[x]["rec"] != rows[m["members"][0]]["rec"]:
                continue
            lo, hi = MR.span_of(rows[x], recs)
            carriers = [s for s, g in enumerate(recs[rows[x]["rec"]]["slots"]) if g == rows[x]["alt"]]
            covered |= lo <= a <= hi and bool(carriers) and all(m["slots"][s] is None for s in carriers)
            short |= hi == a - 1 and bool(carriers) and all(m["slots"][s] == 0 for s in carriers)
    assert covered and short
    # a PASS row beside primitives of its record
    assert any(r["kind"] == PR.ROW_PASS and n_of_pair.keys() & {(r["rec"], k) for k in range(1, 9) if k != r["alt"]} for r in rows)
    # more samples than lanes, a group of more members than lanes, records that meet at one POS
    assert len(merged[0]["gt"]) >= 65 and max(len(g) for g in groups) >= 65
    assert any(a["pos"] == b["pos"] and a["rec"] != b["rec"] for a, b in zip(rows, rows[1:]))
    # more than sixteen groups in one (POS, lengths) run: a four-bit hash must collide
    runs = {}
    for g in groups:
        if rows[g[0]]["kind"] != PR.ROW_PASS:
            k = key(g[0])
            runs[(k[0], k[1], len(k[2]), len(k[3]))] = runs.get((k[0], k[1], len(k[2]), len(k[3])), 0) + 1
    assert max(runs.values()) > 16
    # a record that stays the raw line is the representative of a group
    assert any(len(g) > 1 and rows[g[0]]["kind"] == PR.ROW_RAW for g in groups)
