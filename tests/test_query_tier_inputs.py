"""The inputs of tests/test_gpu_query_tiers.py reach what they are there for (tests/query_tier_cases.py), shown on the restatement
of the tiering (tests/query_tier_model.py): the constants mirror the sources, the model's search agrees with walks_ref on every
case, every case has the figures written here, and every hand-over threshold is met from both sides.  Plain Python and the CPU
oracle, no GPU."""
import os
import re

import pytest

import query_tier_cases as K
import query_tier_model as M
import traversals_ref as TR
import walks_ref as WR
from povu_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "povu_amd", "csrc", "hip")

# name: (queries, frames, expansions, status, walks, steps of the longest walk, tier 1 hands the case's query over, n_tier2 of
# the graph, slots of the fullest side)
WALK_FIGURES = {
    "arm14": (1, 15, 17, 0, 2, 16, False, 0, 2),
    "arm15": (1, 16, 18, 0, 2, 17, False, 0, 2),  # the last that tier 1 finishes: 16 frames, a walk of 17 steps
    "arm16": (1, 17, 19, 0, 2, 18, True, 1, 2),
    "arm17": (1, 18, 20, 0, 2, 19, True, 1, 2),
    "nested13": (2, 16, 21, 0, 3, 17, False, 0, 2),
    "nested14": (2, 17, 22, 0, 3, 18, True, 1, 2),  # the parent alone: its child's arm is one segment short of the hand-over
    "nested15": (2, 18, 23, 0, 3, 19, True, 1, 2),
    "nested16": (2, 19, 24, 0, 3, 20, True, 2, 2),
    "site4095": (1, 3, 4095, 0, 2047, 4, False, 0, 2047),
    "site4096": (1, 2, 4096, 0, 2048, 3, False, 0, 2048),  # the 4096th expansion is the last: no hand-over
    "site4097": (1, 3, 4097, 0, 2048, 4, True, 1, 2048),
    "budget4095": (1, 3, 4095, WR.BUDGET, 2047, 4, False, 0, 2049),
    "budget4096": (1, 3, 4096, WR.BUDGET, 2047, 4, False, 0, 2049),  # max_expansions == T1_EXPANSIONS: BUDGET wins
    "budget4097": (1, 3, 4097, WR.BUDGET, 2048, 4, True, 1, 2049),
    "slots63": (1, 2, 100, 0, 50, 3, False, 0, 63),
    "slots64": (1, 2, 102, 0, 51, 3, False, 0, 64),
    "slots64d": (1, 2, 64, 0, 32, 3, False, 0, 64),
    "slots65": (1, 2, 104, 0, 52, 3, False, 0, 65),
    "wrap4_2": (1, 1, 56, WR.LONG, 0, 0, False, 0, 56),
    "wrap4_7": (1, 6, 116, WR.LONG, 55, 3, False, 0, 56),
    "wrap4_8": (1, 7, 117, WR.LONG, 55, 3, False, 0, 56),
    "wrap4_9": (1, 8, 118, 0, 56, 9, False, 0, 56),
    "wrap5_2": (1, 1, 152, WR.LONG, 0, 0, False, 0, 152),
    "wrap5_7": (1, 6, 308, WR.LONG, 151, 3, False, 0, 152),
    "wrap5_8": (1, 7, 309, WR.LONG, 151, 3, False, 0, 152),
    "wrap5_9": (1, 8, 310, 0, 152, 9, False, 0, 152),
}
# name: (table bits, entries at most, probes that wrapped, entries a deletion left in place); none is ever moved (below)
WRAP_FIGURES = {"wrap4_7": (4, 6, 10, 10), "wrap4_8": (4, 7, 12, 10), "wrap5_9": (5, 8, 18, 8)}

# max_steps: (tasks handed over, {case: (status of its query, traversals, alleles, tasks, handed over)})
_CLOSED, _LONG, _OPEN, _STRAY = (0, 2, 1), (TR.LONG, 0, 0), (TR.OPEN, 0, 0), (TR.STRAY, 0, 0)
TRAV_FIGURES = {
    65536: (19, dict(close63=_CLOSED + (2, 0), close64=_CLOSED + (2, 0), close65=_CLOSED + (2, 2), close66=_CLOSED + (2, 2),
                     close127=_CLOSED + (2, 2), close128=_CLOSED + (2, 2), close129=_CLOSED + (2, 2), close193=_CLOSED + (2, 2),
                     end64=_OPEN + (2, 0), end65=_OPEN + (2, 0), end66=_OPEN + (2, 2), stray64=_STRAY + (2, 0),
                     stray65=_STRAY + (2, 2), dedup130=(0, 3, 2, 3, 3))),
    # the window ends before offset 65: nothing is handed over; a traversal of 64 steps fits, one of 65 is LONG
    64: (0, dict(close63=_CLOSED + (2, 0), close64=_LONG + (2, 0), close65=_LONG + (2, 0), end64=_OPEN + (2, 0), end65=_LONG + (2, 0),
                 stray64=_LONG + (2, 0), dedup130=_LONG + (3, 0))),
    65: (0, dict(close64=_CLOSED + (2, 0), close65=_LONG + (2, 0), end65=_OPEN + (2, 0), end66=_LONG + (2, 0), stray64=_STRAY + (2, 0),
                 stray65=_LONG + (2, 0))),
    # the window goes on past offset 65 by one step: handed over, and the second ballot has one lane in the window
    66: (19, dict(close65=_CLOSED + (2, 2), close66=_LONG + (2, 2), end66=_OPEN + (2, 2), stray65=_STRAY + (2, 2), dedup130=_LONG + (3, 3))),
    129: (19, dict(close128=_CLOSED + (2, 2), close129=_LONG + (2, 2), dedup130=_LONG + (3, 3))),
    130: (19, dict(close129=_CLOSED + (2, 2), close193=_LONG + (2, 2), dedup130=(0, 3, 2, 3, 3))),
}


def test_constants_mirror_the_sources():
    rules = open(os.path.join(HIP, "walk_rules.hpp")).read()
    walk = open(os.path.join(HIP, "walk_kernels.hip")).read()
    trav = open(os.path.join(HIP, "trav_kernels.hip")).read()

    def const(text, name):
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))
    assert const(rules, "T1_DEPTH") == M.T1_DEPTH and const(rules, "T1_EXPANSIONS") == M.T1_EXPANSIONS
    assert const(rules, "SORT_IN_LANE") == M.SORT_IN_LANE and "if (e - b > SORT_IN_LANE)" in walk
    assert "static constexpr uint32_t cap = T1_DEPTH;" in rules and "if (depth == st.cap)" in rules
    assert "return (u * 2654435761u) >> (32 - tbits);" in rules and M.HASH == 2654435761
    assert "c.E < T1_EXPANSIONS ? c.E : T1_EXPANSIONS" in walk
    assert "std::max(4u, bits_for(2 * (uint64_t)c.L - 1))" in walk and "(size_t)2 * c.L + (size_t(1) << tbits)" in walk
    assert "std::min<size_t>({(size_t)n2, 16384, (size_t(256) << 20) / (lane_words * 4)})" in walk
    assert M.T2_MAX_LANES == 16384 and M.T2_SCRATCH == 256 << 20
    assert "if (c.L > (1u << 24))" in walk and M.MAX_STEPS_CAP == 1 << 24
    assert const(trav, "T1_STEPS") == M.T1_STEPS and "const uint64_t stop = t.pos + 1 + T1_STEPS;" in trav
    assert "if (!found && j < t.lim) {" in trav and "std::min<uint64_t>(((uint64_t)t.n2 + Q_TPB / 64 - 1) / (Q_TPB / 64), 4096)" in trav
    # the budget is tested before the tier's own limit, both before the expansion is counted
    assert rules.index("if (exp == c.E) {") < rules.index("if (exp == ecap) {") < rules.index("exp++;")
    assert [M.tbits_of(L) for L in (1, 2, 7, 8, 9, 16, 17, 1000, 1 << 20, 1 << 24)] == [4, 4, 4, 4, 5, 5, 6, 11, 21, 25]
    assert [M.t2_lanes(n2, L) for n2, L in ((0, 8), (5, 8), (20000, 8), (300, 1 << 20), (300, 1 << 22), (300, 1 << 24), (3, 1 << 22))] == \
        [0, 5, 16384, 16, 4, 1, 3]


def test_the_sites_are_the_ones_the_model_finds():
    assert [K.site_spending(x) for x in (4095, 4096, 4097, 4099)] == [(2046, 1), (2048, 0), (2047, 1), (2048, 1)]


@pytest.mark.parametrize("name", sorted(WALK_FIGURES))
def test_walk_case_has_its_figures(name):
    g, caps, q = K.walk_cases()[name]
    qs = K.queries_of(g)
    assert q in qs
    c, succ = K.caps_of(caps), WR.successors(g)
    full, t1 = M.search(succ, *q, **c), M.search(succ, *q, tier1=True, **c)
    ws, st = WR.walks_of(succ, *q, **c)
    assert (full["status"], full["walks"]) == (st, len(ws))  # (the model runs the search of the restatement)
    got = (len(qs), full["frames"], full["expansions"], st, len(ws), max(map(len, ws), default=0), t1["handover"],
           M.walks_n_tier2(succ, qs, **c), M.max_side_slots(g))
    assert got == WALK_FIGURES[name]
    assert t1["handover"] == (full["frames"] > M.T1_DEPTH or full["expansions"] > M.T1_EXPANSIONS)
    assert M.has_hub(g) == (WALK_FIGURES[name][8] > 64)


def test_every_walk_case_is_listed():
    assert set(K.walk_cases()) == set(WALK_FIGURES)


@pytest.mark.parametrize("name", sorted(WRAP_FIGURES))
def test_path_set_of_the_pinned_indices_wraps(name):
    """the search of the case's query on a tier-2 lane: probes wrap past the last slot and deletions meet entries that stay.  No
    entry is ever moved: a search pops what it pushed last, and then the table is what pushing the stack from the bottom gives --
    an entry older than the one that leaves found the hole empty when it was pushed and did not probe past it."""
    g, caps, q = K.walk_cases()[name]
    c = K.caps_of(caps)
    ps = M.PathSet(M.tbits_of(c["max_steps"]))
    M.search(WR.successors(g), *q, path_set=ps, index_of=K.index_of(g), **c)
    e = ps.events()
    assert (ps.tbits, e["max_load"], e["wrap_probe"], e["stayed"]) == WRAP_FIGURES[name]
    assert e["max_load"] == c["max_steps"] - 1 and e["moved"] == 0 and e["shift_across"] == 0


def test_union_and_lane_reuse():
    u = K.union()
    qs = K.queries_of(u)
    succ = WR.successors(u)
    assert (u.n_vtx, len(qs)) == (9804, 248)
    assert M.walks_n_tier2(succ, qs, **WR.DEFAULTS) == 6
    lanes = [M.t2_lanes(len(qs), L) for L in K.REUSE_MAX_STEPS]
    assert lanes == [16, 4, 1] and all(n < len(qs) for n in lanes)
    # queries that stop with frames still on the stack: what the unwinding loop takes off the lane's path set
    left = [sum(1 for s, z in qs if M.search(succ, s, z, **K.caps_of(dict(caps, max_steps=1 << 20)))["left_on_path"]) for caps in K.REUSE_CAPS]
    assert left == [5, 113]


@pytest.mark.parametrize("max_steps", sorted(TRAV_FIGURES))
def test_traversal_cases_have_their_figures(max_steps):
    g, paths, cases = K.trav_inputs()
    qs = K.queries_of(g)
    assert len(qs) == K.TRAV_UNITS and len(paths) == 29
    index = TR.PathIndex(paths)
    tasks = M.trav_tasks(paths, qs, max_steps)
    n2, rows = TRAV_FIGURES[max_steps]
    assert len(tasks) == 52 and sum(t[4] for t in tasks) == n2 == M.trav_n_tier2(paths, qs, max_steps)
    for name, want in rows.items():
        unit, mine = cases[name]
        q = qs.index(K._unit(unit))
        al, tr, st = TR.traversals_of(index, *qs[q], max_steps)
        of_q = [t for t in tasks if t[0] == q]
        assert (st, len(tr), len(al), len(of_q), sum(t[4] for t in of_q)) == want, name
        assert {t[1] for t in of_q} == set(mine)  # (the scans of the case's unit start in the case's paths)
    assert set(cases) == set(TRAV_FIGURES[65536][1])


def test_every_threshold_is_met_from_both_sides():
    f = WALK_FIGURES
    # frames: 16 stay, 17 go (in a leaf and in a parent); expansions: 4096 stay, 4097 go; the budget at, below and above the limit
    assert [f[n][1] for n in ("arm15", "arm16", "nested13", "nested14")] == [16, 17, 16, 17]
    assert [f[n][6] for n in ("arm15", "arm16", "nested13", "nested14")] == [False, True, False, True]
    assert [(f[n][2], f[n][6]) for n in ("site4095", "site4096", "site4097")] == [(4095, False), (4096, False), (4097, True)]
    assert [(f[n][3], f[n][7]) for n in ("budget4095", "budget4096", "budget4097")] == [(WR.BUDGET, 0), (WR.BUDGET, 0), (WR.BUDGET, 1)]
    assert [f[n][8] for n in ("slots63", "slots64", "slots64d", "slots65")] == [63, 64, 64, 65]
    # the table: 16 slots up to L = 8 (7 entries: half load), 32 from L = 9
    assert [M.tbits_of(L) for L in (2, 7, 8, 9)] == [4, 4, 4, 5]
    # traversals: a close, an end and a stray step at the last offset tier 1 looks at and at the next
    t = TRAV_FIGURES[65536][1]
    assert [t[n][4] for n in ("close64", "close65", "end65", "end66", "stray64", "stray65")] == [0, 2, 0, 2, 0, 2]
    # a window of the traversal's length and one less, at lengths 64, 65, 66, 129 and 130
    for ms, fits, long_ in ((64, "close63", "close64"), (65, "close64", "close65"), (66, "close65", "close66"), (129, "close128", "close129"),
                            (130, "close129", "close193")):
        assert TRAV_FIGURES[ms][1][fits][:2] == (0, 2) and TRAV_FIGURES[ms][1][long_][:2] == (TR.LONG, 0)


def test_more_tasks_than_tier2_has_waves():
    k, n = K.TASKS_CHAIN
    hp = W.chain_haplotypes(k, n, 4)
    paths = TR.paths_from_arrays(hp.off, hp.ids, hp.rev)
    qs = K.queries_of(W.chain_of_bubbles(k))
    assert len(qs) == k
    assert len(M.trav_tasks(paths, qs)) == k * n == 16392 > 4 * 4096 >= (k - 1) * n
