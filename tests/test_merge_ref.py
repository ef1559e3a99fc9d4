"""The plain-Python restatement of the merged primitives (tests/merge_ref.py): its grouping against a second, quadratic one,
the invariants that tie every merged genotype back to the raw GT rows, the inputs of the GPU tests (tests/merge_cases.py), and
the rows the definition gives on the reference's popped-parent-child-rescue and vcfwave-complex-decomposition graphs
(INTEGRATION.md "Merged primitives").  No GPU."""
import pytest

import merge_cases as MC
import merge_ref as MR
import oracle_lib as O
import prim_cases as PC
import prim_ref as PR
import vcf_ref as V
from povu_amd import hip as H
from test_norm_ref import _graph

POPPED = "downstream_repetitive/popped-parent-child-rescue"
VCFWAVE = "downstream_repetitive/vcfwave-complex-decomposition"


def restated(g, seqs, p, prefixes, cap=0):
    names, paths = list(p.names), [p.steps(i) for i in range(len(p))]
    sq = dict(zip(g.vid.tolist(), seqs))
    raw = V.call(V.sites_of_pvst(list(O.decompose(g).values())), names, paths, sq, prefixes)
    rows, _ = PR.decompose(raw, names, paths, sq, max_allele_length=cap)
    return raw, rows, names


def groups_by_all_pairs(rows, recs):
    """The grouping a second way: every pair of rows compared, the classes of the relation read off a union-find."""
    up = list(range(len(rows)))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x
    text = [tuple(t.upper() for t in MR.texts_of(r, recs)) for r in rows]
    for x in range(len(rows)):
        for y in range(x):
            a, b = rows[x], rows[y]
            if PR.ROW_PASS in (a["kind"], b["kind"]):
                continue
            if a["path"] == b["path"] and a["pos"] == b["pos"] and text[x] == text[y]:
                up[find(x)] = find(y)
    out = {}
    for x in range(len(rows)):
        out.setdefault(find(x), []).append(x)
    return sorted(out.values())  # (by first member: a list's first entry is its lowest row)


def invariants(recs, rows, merged):
    """Every carried ALT is 1 on all of its rows' groups, and no group says 0 where a row of the carried ALT overlaps it."""
    group_of = {x: m for m in merged for x in m["members"]}
    of_pair = {}
    for x, r in enumerate(rows):
        of_pair.setdefault((r["rec"], r["alt"]), []).append(x)
    for j, r in enumerate(recs):
        touching = [m for m in merged if any(rows[x]["rec"] == j for x in m["members"])]
        for s, g in enumerate(r["slots"]):
            if g is None or g == 0:
                continue
            mine = of_pair[(j, g)]
            assert all(group_of[x]["slots"][s] == 1 for x in mine), (j, s, g)
            for m in touching:
                if m["slots"][s] == 0:
                    a, b = MR.span_of(rows[m["members"][0]], recs)
                    assert all(not (lo <= b and a <= hi) for lo, hi in (MR.span_of(rows[x], recs) for x in mine)), (j, s, g)


CASES = [("chain", MC.chain_case, MC.CHAIN_REFS, MC.CHAIN_CAP), ("skip", MC.skip_case, ["hap0"], 0)] + \
    [(f"complex{seed}", lambda seed=seed: PC.complex_case(seed), ["hap0"], PC.COMPLEX_CAP) for seed in PC.COMPLEX_SEEDS]


@pytest.mark.parametrize("name,make,prefixes,cap", CASES, ids=[c[0] for c in CASES])
def test_second_implementation_invariants_and_carrying_inputs(name, make, prefixes, cap):
    raw, rows, names = restated(*make(), prefixes, cap)
    merged, counters = MR.merge(raw, rows, names)
    assert [m["members"] for m in merged] == groups_by_all_pairs(rows, raw)
    MC.carrying(rows, merged, counters)
    assert counters["n_gt_conflicts"] == 0 and counters["n_merge_splits"] == 0 and counters["n_mrows"] == len(merged)
    invariants(raw, rows, merged)
    if name == "chain":
        MC.chain_coverage(raw, rows, merged, counters)
    if name == "skip":  # groups across records
        assert sum(len({rows[x]["rec"] for x in m["members"]}) > 1 for m in merged) >= 10
    # without the non-overlap rule a group of one is the projected row
    for m in merged:
        if len(m["members"]) == 1:
            r = rows[m["members"][0]]
            proj = PR.project(raw[r["rec"]]["slots"], r["alt"], V.slots_of(names)[2], len(m["gt"]))[0]
            assert all(a == b or (a == 0 and b is None) for a, b in zip(m["slots"], proj))
            if r["kind"] == PR.ROW_PASS:
                assert m["slots"] == proj and (m["ac"], m["an"], m["ns"]) == (r["ac"], r["an"], r["ns"])


def test_member_vote():
    spans = {2: [(5, 5), (9, 12)], 3: None}
    other = lambda k: spans[k]  # noqa: E731
    assert MR.member_vote(None, 1, (7, 7), other) == MR.VOTE_NONE
    assert MR.member_vote(1, 1, (7, 7), other) == MR.VOTE_ALT
    assert MR.member_vote(0, 1, (7, 7), other) == MR.VOTE_REF
    assert MR.member_vote(2, 1, (6, 8), other) == MR.VOTE_REF_ELSEWHERE  # between the rows
    assert MR.member_vote(2, 1, (6, 9), other) == MR.VOTE_NONE and MR.member_vote(2, 1, (5, 5), other) == MR.VOTE_NONE
    assert MR.member_vote(2, 1, (13, 20), other) == MR.VOTE_REF_ELSEWHERE and MR.member_vote(2, 1, (12, 20), other) == MR.VOTE_NONE
    assert MR.member_vote(3, 1, (1, 1), other) == MR.VOTE_NONE  # kept whole


def _fixture(golden_dir, tmp_path, name, cap=0):
    (names, paths, seqs), texts = _graph(golden_dir, tmp_path, name)
    raw = V.call(V.sites_of_pvst(texts), names, paths, seqs, ["HG1"])
    rows, _ = PR.decompose(raw, names, paths, seqs, max_allele_length=cap)
    merged, counters = MR.merge(raw, rows, names)
    lines = [ln.split("\t") for ln in MR.vcf_text(names, paths, seqs, raw, rows, merged, ["HG1"]).splitlines() if not ln.startswith("#")]
    return raw, rows, merged, counters, lines


def test_popped_parent_child_rescue_under_a_plain_call(golden_dir, tmp_path):
    """>0>5 AAAAA -> A,AAAGA: the SNP A -> G of ALT 2 at POS 4 is the whole >2>4 record.  One group of two at one POS; the
    deleting haplotype is '.' there (its ALT is kept whole: a gap at offset 0 of a record at POS 1 has no base to anchor on, and
    an ALT kept whole casts no vote; were it a DEL row, its span would cover POS 4 all the same)."""
    raw, rows, merged, counters, lines = _fixture(golden_dir, tmp_path, POPPED)
    assert [(r["id"], r["pos"], r["ref"], r["alts"]) for r in raw] == [(">0>5", 1, "AAAAA", ["A", "AAAGA"]), (">2>4", 4, "A", ["G"])]
    assert [(r["rec"], r["alt"], r["kind"], r["pos"]) for r in rows] == [(0, 1, PR.ROW_PASS, 1), (0, 2, PR.ROW_SNP, 4), (1, 1, PR.ROW_RAW, 4)]
    assert rows[0]["reason"] == PR.REASON_CONTIG_START
    assert [m["members"] for m in merged] == [[0], [1, 2]]
    assert counters == dict(n_mrows=2, n_merged_groups=1, n_merged_members=2, n_merge_splits=0, n_ref_consistent=0, n_gt_conflicts=0)
    assert merged[1]["slots"] == [0, None, 1] and (merged[1]["ac"], merged[1]["an"], merged[1]["ns"]) == (1, 2, 2)
    assert [f[1:5] + f[9:] for f in lines] == [["1", ">0>5:1:passthrough", "AAAAA", "A", "0", "1", "."],
                                               ["4", ">0>5:2:snp1", "A", "G", "0", ".", "1"]]
    assert ";DECOMPOSED=T;MERGED=2;MERGED_FROM=>0>5:2:snp1,>2>4:1:snp1;RAW_POS=1;RAW_REF=AAAAA;RAW_ALT=AAAGA" in lines[1][7]
    assert lines[1][7].startswith("AC=1;AF=0.5;AN=2;NS=2;") and "MERGED" not in lines[0][7]


def test_vcfwave_complex_decomposition_without_a_cap(golden_dir, tmp_path):
    """Nothing merges.  ALT 2 is an insertion at POS 1 and one at POS 4: its carrier is reference at the SNP of POS 2 and stays
    '.' at the SNP of POS 4."""
    raw, rows, merged, counters, lines = _fixture(golden_dir, tmp_path, VCFWAVE)
    assert counters == dict(n_mrows=4, n_merged_groups=0, n_merged_members=0, n_merge_splits=0, n_ref_consistent=2, n_gt_conflicts=0)
    by_id = {f[2]: f for f in lines}
    assert [f[2] for f in lines] == [">9>14:2:ins1", ">9>14:1:snp1", ">9>14:1:snp2", ">9>14:2:ins2"]
    assert by_id[">9>14:1:snp1"][9:] == ["0", "1", "0"] and by_id[">9>14:1:snp1"][7].startswith("AC=1;AF=0.3;AN=3;NS=3;")
    assert by_id[">9>14:1:snp2"][9:] == ["0", "1", "."] and by_id[">9>14:2:ins2"][9:] == ["0", ".", "1"]
    assert by_id[">9>14:2:ins1"][9:] == ["0", "0", "1"]
    assert not any("MERGED" in f[7] for f in lines)
    text = "\n".join("\t".join(f) for f in lines)
    # ... and the rows themselves are the decomposed profile's, but for GT and the counts
    names, paths, seqs = _graph(golden_dir, tmp_path, VCFWAVE)[0]
    plain = [ln.split("\t") for ln in PR.vcf_text(names, paths, seqs, raw, rows, ["HG1"]).splitlines() if not ln.startswith("#")]
    assert [f[:7] + [f[7].split(";AT=")[1]] for f in plain] == [f[:7] + [f[7].split(";AT=")[1]] for f in lines] and text


def test_header_lines_and_python_constants(golden_dir, tmp_path):
    (names, paths, seqs), texts = _graph(golden_dir, tmp_path, POPPED)
    raw = V.call(V.sites_of_pvst(texts), names, paths, seqs, ["HG1"])
    rows, _ = PR.decompose(raw, names, paths, seqs)
    head = MR.vcf_text(names, paths, seqs, raw, rows, MR.merge(raw, rows, names)[0], ["HG1"]).splitlines()
    at = next(k for k, ln in enumerate(head) if ln.startswith("##INFO=<ID=SUBR_ORIGIN,"))
    assert head[at + 1].startswith("##INFO=<ID=MERGED,Number=1,Type=Integer,") and head[at + 2].startswith("##INFO=<ID=MERGED_FROM,Number=.,Type=String,")
    assert head[at + 3].startswith("##contig=")
    assert H.T_MERGE == 8 and H.T_MERGE not in (H.T_FORCE_TIER2, H.T_INVERSIONS, H.T_NESTED)
    assert (MR.VOTE_NONE, MR.VOTE_REF, MR.VOTE_ALT, MR.VOTE_REF_ELSEWHERE) == (0, 1, 2, 3)
