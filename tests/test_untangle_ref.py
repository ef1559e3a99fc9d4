"""The restatement of the untangled calls (tests/untangle_ref.py; INTEGRATION.md "Untangled calls") against what the
definition says: the graph it was stated on (PVST from the CPU oracle) and its stored lines, the alignment against an
independently written edit distance, the tie cases, a haplotype walking backwards, the entries that fall back, a site nobody
loops, and the refusals.  No GPU."""
import itertools

import pytest

import offref_cases as OC
import untangle_cases as UC
import untangle_ref as U
import vcf_ref as V
from povu_amd import workloads as W


def _load(g, p, out, seed=3):
    out.mkdir(exist_ok=True)
    gfa = out / "g.gfa"
    gfa.write_text(g.to_gfa(UC.sequences(g, seed)) + p.to_gfa())
    return OC.load(str(gfa), out / "pvst")


def test_the_example_of_the_definition(tmp_path):
    sites, names, paths, seqs, texts = OC.load(UC.GFA, tmp_path)
    assert [ln.split("\t")[2] for ln in texts[0].splitlines() if ln.startswith("F")] == [">0>5", ">1>4"]
    gold = UC.golden()
    assert [V.record_line(r) for r in V.call(sites, names, paths, seqs, ["HG1"])] == gold["plain_lines"]
    recs, counts = U.call(sites, names, paths, seqs, ["HG1"])
    assert [U.record_line(r, names) for r in recs] == gold["lines"] and counts == gold["counters"]
    assert [(r["pos"], r["gt"], r["lap_count"], r["ac"], r["an"], r["ns"], r["tangled"], r["lap"], r["n_laps"]) for r in recs] == [
        (4, ["0", "0", "1"], [3, 2, 4], [1], 3, 3, False, 1, 3), (9, ["0", ".", "0"], [3, 2, 4], [0], 2, 2, False, 2, 3),
        (14, ["0", "0", "0"], [3, 2, 4], [0], 3, 3, False, 3, 3)]
    assert [ln.split("\t")[7].split(";")[:4] for ln in gold["lines"]] == [["AC=1", "AF=0.3", "AN=3", "NS=3"], ["AC=0", "AF=0.0", "AN=2", "NS=2"],
                                                                        ["AC=0", "AF=0.0", "AN=3", "NS=3"]]
    assert (counts["n_unt_tasks"], counts["n_unt_missing"], counts["n_unt_extra"]) == (2, 1, 1)
    assert U.align([0, 1, 0], [0, 0])[0] == [0, None, 1] and U.align([0, 1, 0], [1, 1, 0, 0])[:2] == ([0, 1, 3], 1)
    text = U.vcf_text(names, paths, seqs, recs, ["HG1"])
    head = text.splitlines()
    k = len(V.HEADER.splitlines())
    assert [ln[:ln.index(",")] for ln in head[k:k + 3]] == ["##INFO=<ID=LN", "##INFO=<ID=LC", "##FORMAT=<ID=CN"]
    assert head[k + 3].startswith("##contig=<ID=HG1#1#chr1,")


def levenshtein(a, b):
    """Written on its own: one row at a time."""
    row = list(range(len(b) + 1))
    for x in a:
        prev, row = row, [row[0] + 1]
        for j, y in enumerate(b):
            row.append(min(prev[j] + (x != y), prev[j + 1] + 1, row[j] + 1))
    return row[-1]


def test_every_alignment_is_optimal_and_monotone():
    seqs = [list(s) for n in range(5) for s in itertools.product(range(3), repeat=n)]
    for a in seqs:
        for b in seqs:
            partner, extra, cost = U.align(a, b)
            assert cost == levenshtein(a, b)
            got = [x for x in partner if x is not None]
            assert got == sorted(set(got)) and len(got) + extra == len(b)
            assert sum(x is None for x in partner) + extra + sum(a[i] != b[x] for i, x in enumerate(partner) if x is not None) == cost


def test_the_tie_cases():
    assert U.align([0], [1, 2])[0] == [1]
    assert U.align([0], [0, 2])[0] == [0]
    assert U.align([0, 1, 0], [1])[0] == [None, 0, None]


def _gts(recs):
    return [(r["q"], r["first"], r["slots"], r["lap_count"], r["unt"]) for r in recs]


def test_a_haplotype_walking_backwards_is_its_forward_twin(tmp_path):
    units = [[0, 1, 0, 0, 1], [1, 0, 0], [0, 0, 1, 1, 0, 1, 1]]
    names = ["ref#1#c", "a#1#c", "b#1#c"]
    fwd = _load(*UC.looped_paths(names, units), tmp_path / "f")
    bwd = _load(*UC.looped_paths(names, units, reverse={1, 2}), tmp_path / "b")
    got_f, counts_f = U.call(*fwd[:4], ["ref#"])
    got_b, counts_b = U.call(*bwd[:4], ["ref#"])
    assert _gts(got_f) == _gts(got_b) and counts_f == counts_b and counts_f["n_unt_tasks"] == 2
    assert any(None in r["slots"] for r in got_f) and all(r["unt"] for r in got_f)


def test_the_entries_that_fall_back(tmp_path):
    # paths 1 and 2 are two contigs of one slot, path 4 is a second contig of the reference's own slot; path 3 alone is aligned
    names = ["ref#1#c", "two#1#c", "two#1#d", "clean#1#c", "ref#1#d"]
    g, p = UC.looped_paths(names, [[0, 1, 0], [0, 0], [1, 1], [1, 1, 0], [1]])
    sites, names, paths, seqs, _ = _load(g, p, tmp_path / "a")
    recs, counts = U.call(sites, names, paths, seqs, ["ref#1#c"])
    plain = V.call(sites, names, paths, seqs, ["ref#1#c"])
    slot = V.slots_of(names)[1]
    for r, o in zip(recs, plain):
        assert r["slots"][slot[1]] == o["slots"][slot[1]] is None and r["tangled"]  # two contigs with different alleles: '.', tangled
        assert r["slots"][slot[0]] == 0 and r["lap_count"] == [4, 4, 3]
    assert counts["n_unt_tasks"] == 1 and counts["n_unt_fallback"] == 2 * 3
    # a mixed path: one path that walks the site forwards and then backwards
    mixed = paths[3][:4] + [(x[0], 1 - x[1]) for x in reversed(paths[3][:4])]
    paths2 = [paths[0], mixed]
    recs2, counts2 = U.call(sites, ["ref#1#c", "mixed#1#c"], paths2, seqs, ["ref#"])
    plain2 = V.call(sites, ["ref#1#c", "mixed#1#c"], paths2, seqs, ["ref#"])
    assert counts2["n_unt_tasks"] == 0 and [r["slots"] for r in recs2] == [r["slots"] for r in plain2] and not any(r["unt"] for r in recs2)
    assert [r["lap_count"] for r in recs2] == [[3, 2]] * 3 and counts2["n_unt_fallback"] == 6
    # 65 laps on either side
    g, p = UC.two_paths(64, 65, 1)
    recs3, counts3 = U.call(*_load(g, p, tmp_path / "c")[:4], ["ref#"])
    assert counts3["n_unt_tasks"] == 0 and counts3["n_unt_fallback"] == 128 and not any(r["unt"] for r in recs3)


def test_a_site_nobody_loops_gives_the_plain_records(tmp_path):
    g = W.chain_of_bubbles(12)
    p = W.pansn(W.chain_haplotypes(12, 7, seed=3), samples=4)
    sites, names, paths, seqs, _ = _load(g, p, tmp_path / "a")
    recs, counts = U.call(sites, names, paths, seqs, ["sample0#1"])
    plain = V.call(sites, names, paths, seqs, ["sample0#1"])
    assert len(recs) > 5 and counts == dict.fromkeys(U.COUNTERS, 0) and not any(r["unt"] for r in recs)
    assert [U.record_line(r, names) for r in recs] == [V.record_line(r) for r in plain]
    a, b = V.vcf_text(names, paths, seqs, plain, ["sample0#1"]), U.vcf_text(names, paths, seqs, recs, ["sample0#1"])
    assert b == a.replace(V.HEADER.format(date="00000000"), V.HEADER.format(date="00000000") + U.HEADER_LINES)


def test_the_refusals(tmp_path):
    sites, names, paths, seqs, _ = OC.load(UC.GFA, tmp_path)
    for kw, word in ((dict(nested=True), "POVU_HIP_T_NESTED"), (dict(merge=True), "POVU_HIP_T_MERGE"), (dict(offref=True), "POVU_HIP_T_OFFREF"),
                     (dict(profile="popped"), "profile popped"), (dict(profile="decomposed"), "profile decomposed")):
        with pytest.raises(U.UntangleError, match="POVU_HIP_T_UNTANGLE .*" + word):
            U.call(sites, names, paths, seqs, ["HG1"], **kw)
    assert len(U.call(sites, names, paths, seqs, ["HG1"], profile="raw-graph")[0]) == 3
