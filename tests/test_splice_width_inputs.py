"""The inputs of tests/test_gpu_splice_widths.py reach what their names claim, on the CPU: every case of
splice_width_cases.CASES gives, by the oracle's width counters (orc_sub_widths), exactly the figures pinned in the table, and
the rules of its seed still fire.  These figures are the evidence that the device's second and third rounds are reached; a
seed or a generator that drifts fails here, not silently on the GPU."""
import re

import pytest

import oracle_lib as O
import splice_width_cases as S
from test_oracle_subflubbles import RULES, _check_shape, sub_stats

SPLICE_WAVES = 8192  # povu_amd/csrc/hip/sub_kernels.hip


def test_width_words_match_the_oracle():
    """one word per name, and a run without -s vertices leaves every word 0"""
    assert len(set(S.WIDTHS)) == len(S.WIDTHS) == 4 * 12 + 21
    from povu_amd import workloads as W
    _, w, _ = S.measure(W.chain_of_bubbles(50))
    assert not any(w.values()), w


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_case_reaches_its_figures(name):
    seed, links, figures, rules = S.CASES[name]
    assert set(figures) <= set(S.WIDTHS) and set(rules) <= set(RULES)
    g, tips = S.case_graph(name)
    got_rules, got, full = S.measure(g, tips)
    assert {k: got[k] for k in figures} == figures
    assert got_rules == {r: rules.get(r, 0) for r in RULES}
    # not vacuous: some vector of the case is longer than a round
    assert max(figures.values()) >= 63 or name == "two_links_one_flubble"
    for w in S.NOT_FOUND:
        assert got[w] == 0, w
    plain = O.decompose(g, tips=tips, leaf=1)
    assert plain.keys() == full.keys()
    for c in plain:
        _check_shape(plain[c], full[c])


def test_the_table_reaches_every_round():
    """per loop of the splice, the rounds the table reaches (round = index // 64; *_rnd and *_idx words are + 1)"""
    fig = {n: c[2] for n, c in S.CASES.items()}

    def values(word):
        return {f[word] for f in fig.values() if word in f}
    edges = {63, 64, 65, 127, 128, 129}
    assert edges | {257} <= values("ai_movers") and edges | {257} <= values("zi_movers")
    # filter: a mixed round 2, 3 and later; stayers behind movers over a whole later round; movers in round 3 and 5
    assert {2, 3, 4, 5} <= values("ai_mixed_rnd") and {2, 3, 5} <= values("zi_mixed_rnd")
    assert max(values("ai_stay_behind_n")) > 64 and max(values("zi_stay_behind_n")) > 64
    # reserve: the first push onto a seeded vector of 64 / 65 / 129; a destination copied with 64, 128 and 256 in it
    assert {64, 65, 129} <= values("first_push_seeded")
    assert {64, 128, 256} <= values("ai_reserve_copy")
    assert {32, 64, 128} <= values("push_full_s")
    # find_midi: the second trunk concealed child in round 2, 3 and 5, in another round than the first and in the same
    assert {64, 65, 129, 130, 257} <= values("midi_second_idx") and values("midi_split_rounds") == {0, 1}
    assert {65, 129, 257} <= values("midi_copy_len")
    # smothered::nest
    assert {63, 64, 65, 129} <= values("smo_erasures") and max(values("smo_old_end")) >= 270
    assert {63, 64, 65, 129} <= values("pinned_len") and values("pinned_wide") == {0, 1}


def _no_ids(text):
    return re.sub(r"([<>])\d+", r"\1#", text)


# links of the table's cases whose seed keeps its text when one segment is put into them
KEEP = (("ai_trunk", 6), ("midi_same_kind", 0), ("nest_over_pinned", 0), ("nest_trunk_zi", 0), ("pinned10", 0), ("pinned3", 18),
        ("pinned3", 22), ("smo_stale_read", 13), ("smo_stale_read", 14))


def test_widen_by_nothing_keeps_the_pvst():
    """k = 0 puts one segment into the link: the PVST text of the seed but for the ids -- where the link is not one the passes
    read.  A segment in series turns one link into two: a back edge of the spanning tree may become a tree path, and a link
    that is cycle equivalent to a segment gives a new boundary, so a flubble moves, turns from F to T or loses its concealed
    vertex (smo_stale_read, link 45).  677 of the 966 (seed, link) pairs of today's seeds keep the text: most must, and those
    of KEEP must.  The other four links the table widens (smo_stale_read 43, 45, 47, pinned10 24) do not: their cases are the
    seed's graph changed by the chain, not the seed plus a chain, and stand on their own pinned figures."""
    kept = total = 0
    for seed, (g, tips) in S.all_seeds().items():
        want = sorted(_no_ids(t) for t in O.decompose(g, tips=tips, leaf=2).values())  # (the components may come in another order)
        for link in range(g.n_links):
            wg, wtips = S.widened(seed, [(link, 0)])
            assert wg.n_vtx == g.n_vtx + 1 and wg.n_links == g.n_links + 1 and (wg.vid[1:] > wg.vid[:-1]).all()
            got = sorted(_no_ids(t) for t in O.decompose(wg, tips=wtips, leaf=2).values())
            total += 1
            kept += got == want
            if (seed, link) in KEEP:
                assert got == want, (seed, link)
    assert 3 * kept >= 2 * total, (kept, total)


def test_widen_adds_a_chain_of_bubbles():
    g, _ = S.all_seeds()["nest_trunk_zi"]
    wg = S.widen(g, 0, 5)
    assert wg.n_vtx == g.n_vtx + 11 and wg.n_links == g.n_links + 16
    assert (wg.vid[1:] > wg.vid[:-1]).all() and int(wg.vid[g.n_vtx]) == int(g.vid.max()) + 1
    assert (wg.v1[17:] == g.v1[1:]).all() and (wg.s2[17:] == g.s2[1:]).all()  # the 17 links of the chain stand where link 0 stood
    assert (int(wg.v1[0]), int(wg.s1[0])) == (int(g.v1[0]), int(g.s1[0])) and (int(wg.v2[16]), int(wg.s2[16])) == (int(g.v2[0]), int(g.s2[0]))
    plain, wide = O.decompose(g, leaf=1), O.decompose(wg, leaf=1)
    assert sum(len(t.splitlines()) for t in wide.values()) == sum(len(t.splitlines()) for t in plain.values()) + 5


def test_stride_graph_lists_more_flubbles_than_two_rounds_of_waves():
    sub_stats()
    _, w, texts = S.measure(S.stride_graph())
    assert w["cn_list"] > 2 * SPLICE_WAVES and w["n_concealed"] > SPLICE_WAVES and w["n_smo_cn"] > 400
    # wide flubbles among the first 8192 entries, the middle and the last: the union keeps every figure of its parts
    for n in ("several_wide", "ai_movers_129", "smo_erasures_65", "midi_second_at_64", "pinned_len_65"):
        for word, v in S.CASES[n][2].items():
            if word not in ("cn_list", "n_concealed", "pinned_wide") and not word.endswith(("_ge64", "_round")):
                assert w[word] >= v, (n, word)
    assert len(texts) > 5000
