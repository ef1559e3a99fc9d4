"""Inputs that take the splice of `-s` (k_sub_splice_cn .. k_sub_smothered: one wave per flubble, 64 children a round) past
its first round.  No graph the suite builds by name gives a flubble with a concealed vertex more than 3 children; these do,
by widen(): one link of a seed graph becomes a chain of k bubbles, each a child of the flubble whose interior held the link.
How wide a run was is read from the oracle (orc_sub_widths: WIDTHS names its words); CASES pins (seed, widened links) with
the exact figures each reaches, found by `python tests/splice_width_cases.py` (a bounded search: see search())."""
import ctypes as C
import functools
import sys

import numpy as np

import oracle_lib as O
from povu_amd import workloads as W
from test_oracle_subflubbles import (HAND_TRACED, PINNED_SEEDS, RULE_SEEDS, disjoint_union, hand_traced_graph, rule_tips,
                                     seed_graph, sub_stats)

KINDS = ("ai", "aib", "zi", "midi")  # nestings: a-side trunk, a-side branch, z-side trunk (to_child), add_midi
_PER_KIND = ("copy_len movers stayers mover_ge64 stay_behind_ge64 mixed_round mover_idx stay_behind_idx mixed_rnd tail_movers "
             "reserve_copy stay_behind_n").split()
# the words of orc_sub_widths in order (oracle/povu_oracle_sub.inc, the SW_ enums); an *_idx / *_rnd word is index + 1, 0 = never
WIDTHS = tuple(f"{k}_{w}" for k in KINDS for w in _PER_KIND) + tuple(
    "push_len push_full_f push_full_c push_full_s first_push_seeded midi_first_idx midi_second_idx midi_ntrunk midi_split_rounds "
    "midi_third_later midi_find_len smo_old_end smo_erasures smo_stale cn_per_flubble smo_per_cn pinned_wide pinned_len cn_list "
    "n_concealed n_smo_cn".split())


def sub_widths(reset=True):
    lib = O.lib()
    lib.orc_sub_widths.argtypes = [C.c_void_p, C.c_int]
    out = (C.c_uint64 * len(WIDTHS))()
    lib.orc_sub_widths(out, 1 if reset else 0)
    return dict(zip(WIDTHS, list(out)))


def widen(g, link, k):
    """link number `link` of g, (a, sa) -- (b, sb), becomes (a, sa) -- n0- ... nk+ -- (b, sb) over a chain of k bubbles: new
    segments n0 x0 n1 x1 .. nk (ids above the largest of g, in that order) with nj+ -> xj+, xj+ -> n(j+1)+, nj+ -> n(j+1)+.
    The new links stand where the old one stood, so both of its sides keep their place among the links of their segment; the
    links behind it move up by 3 k + 1."""
    nv, top = g.n_vtx, int(g.vid.max())
    vid = np.concatenate([g.vid.astype(np.int64), top + 1 + np.arange(2 * k + 1)])
    n = nv + 2 * np.arange(k + 1, dtype=np.int64)  # vertex idx of nj; xj = nj + 1
    a1 = np.concatenate([[g.v1[link]], n[:-1], n[:-1] + 1, n[:-1], n[-1:]])
    a2 = np.concatenate([n[:1], n[:-1] + 1, n[1:], n[1:], [g.v2[link]]])
    t1 = np.concatenate([[g.s1[link]], np.full(3 * k + 1, W.R)])
    t2 = np.concatenate([np.full(3 * k + 1, W.L), [g.s2[link]]])
    put = lambda old, new: np.concatenate([old[:link].astype(np.int64), new, old[link + 1:].astype(np.int64)])
    return W._mk(vid, put(g.v1, a1), put(g.s1, t1), put(g.v2, a2), put(g.s2, t2))


@functools.lru_cache(maxsize=None)
def all_seeds():
    """name -> (graph, tips) of every seed the `-s` tests name: RULE_SEEDS, PINNED_SEEDS, HAND_TRACED"""
    out = {}
    for rule in RULE_SEEDS:
        g = seed_graph(RULE_SEEDS[rule])
        out[rule] = (g, rule_tips(rule, g))
    for i, p in enumerate(PINNED_SEEDS):
        out[f"pinned{i}"] = (seed_graph(p), None)
    for name in HAND_TRACED:
        out[f"hand_{name}"] = (hand_traced_graph(name), None)
    return out


def widened(seed, links):
    """the graph and tips of one case: `seed` of all_seeds() with every (link, k) of `links` widened (link numbers are the
    seed's: widen() keeps them)"""
    g, tips = all_seeds()[seed]
    for i, (link, k) in enumerate(links):  # (link numbers are the seed's: the links behind a widened one have moved up)
        g = widen(g, link + sum(3 * kj + 1 for lj, kj in links[:i] if lj < link), k)
    if tips is not None:
        tips = np.zeros(g.n_vtx, dtype=np.uint8)
    return g, tips


def measure(g, tips=None):
    """(rule counters, width words, texts) of one oracle run of `-s`"""
    sub_stats()
    sub_widths()
    texts = O.decompose(g, tips=tips, leaf=2)
    return sub_stats(), sub_widths(), texts


def _ai(k):
    """smo_stale_read, link 13 by k: an a-side trunk concealed vertex takes k + 20 children, all but itself of a seeded vector
    that is full at the first push; a smothered vertex then walks the k + 21 of the concealed one"""
    m = k + 20
    rc = 0 if m <= 64 else 64 if m <= 128 else 128 if m <= 256 else 256  # what the destination holds when it is copied last
    return ("smo_stale_read", [(13, k)],
            dict(ai_movers=m, ai_copy_len=m + 1, ai_stayers=1, ai_mover_idx=m, ai_stay_behind_idx=m + 1, ai_mixed_rnd=0 if m % 64 == 0 else m // 64 + 1,
                 ai_reserve_copy=rc, first_push_seeded=m, push_full_f=m, smo_old_end=m + 1, smo_erasures=4),
            dict(ai_trunk=1, nest_trunk_ai=m, smo_g_trunk_src=1, smo_nest=4, smo_stale_read=4))


def _zi(k):
    """nest_trunk_zi, link 0 by k: k + 1 children leave for a z-side trunk concealed vertex (to_child: each takes it in by
    k_sub_pin, so k + 2 flubbles are listed)"""
    m = k + 1
    return ("nest_trunk_zi", [(0, k)],
            dict(zi_movers=m, zi_copy_len=m + 1, zi_stayers=1, zi_mover_idx=m, zi_stay_behind_idx=m + 1, zi_mixed_rnd=0 if m % 64 == 0 else m // 64 + 1,
                 first_push_seeded=m, push_full_f=m, cn_list=m + 1),
            dict(zi_trunk=1, nest_trunk_zi=m, smo_s_trunk=1))


def _midi(k):
    """smo_stale_read, link 43 by k: a flubble keeps k + 2 children, its two trunk concealed children last (index k, k + 1), and
    gets a midi bubble: find_midi walks k + 2, add_midi filters k + 2 (nothing moves) and pushes"""
    return ("smo_stale_read", [(43, k)],
            dict(midi_first_idx=k + 1, midi_second_idx=k + 2, midi_split_rounds=int(k // 64 != (k + 1) // 64), midi_copy_len=k + 2, midi_stayers=k + 2,
                 midi_movers=0, midi_find_len=k + 2, midi_ntrunk=2, midi_third_later=0, push_full_f=k + 3),
            dict(ai_trunk=2, zi_trunk=1, nest_trunk_ai=23, midi=1, smo_g_trunk_src=1, smo_nest=4, smo_stale_read=4))


def _smo(k, erased, full_s):
    """smo_stale_read, link 14 by k: smothered::nest over the k + 21 children of a concealed vertex erases every other one
    (`erased` of them: the element behind an erased one is skipped) and reads the stale tail as often; full_s = the
    greatest length at which the smothered vertex's vector was full at a push"""
    return ("smo_stale_read", [(14, k)],
            dict(smo_old_end=k + 21, smo_erasures=erased, smo_stale=erased, push_full_s=full_s, ai_movers=k + 20, smo_per_cn=1),
            dict(ai_trunk=1, nest_trunk_ai=k + 20, smo_g_trunk_src=1, smo_nest=erased, smo_stale_read=erased))


def _pinned(k):
    """midi_same_kind, link 0 by k: a flubble that took a pinned vertex in runs its z-side nesting over k + 2 children, k of
    which leave"""
    return ("midi_same_kind", [(0, k)],
            dict(pinned_len=k + 2, pinned_wide=int(k + 2 >= 64), zi_copy_len=k + 2, zi_movers=k, zi_stayers=2, first_push_seeded=k),
            dict(zi_trunk=2, nest_trunk_zi=k + 1, midi_same_kind=1, smo_s_trunk=1, nest_over_pinned=1))


# name -> (seed of all_seeds(), [(link, k) ..], width words it reaches EXACTLY, rule counters EXACTLY (every rule not named: 0)).
# The figures are literals worked out per family above and checked against the oracle by tests/test_splice_width_inputs.py.
# Links 43, 45 and 47 of smo_stale_read and 24 of pinned10 change the seed's PVST already when one segment is put into them
# (test_widen_by_nothing_keeps_the_pvst): those cases are a graph of their own, not "the seed plus a chain".
CASES = {
    # filter, movers only: 63 / 64 / 65 / 127 / 128 / 129 / 257 children leave; also the first push onto a seeded vector of that
    # length, and the destination growing from 0 over two, three and five rounds (ai_reserve_copy)
    **{f"ai_movers_{k + 20}": _ai(k) for k in (43, 44, 45, 107, 108, 109, 237)},
    **{f"zi_movers_{k + 1}": _zi(k) for k in (62, 63, 64, 126, 127, 128, 256)},
    # filter, mixed.  M^129 S^100 M S: the first two rounds movers only, the third and fourth mixed, 101 stayers behind movers
    "ai_movers_then_stayers": ("pinned10", [(0, 129), (24, 100)],
                               dict(ai_movers=130, ai_copy_len=231, ai_stayers=101, ai_mixed_rnd=4, ai_mover_idx=230, ai_stay_behind_idx=231,
                                    ai_stay_behind_n=101, ai_reserve_copy=128, first_push_seeded=230, midi_second_idx=102),
                               dict(ai_trunk=1, ai_branch=1, zi_trunk=1, nest_trunk_ai=130, midi=1)),
    # S^69 M^103 S: the movers start in round 1 and fill round 2 up to its last child, which stays
    "ai_stayers_then_movers": ("smo_stale_read", [(43, 69), (47, 100)],
                               dict(ai_movers=103, ai_copy_len=173, ai_stayers=70, ai_mixed_rnd=3, ai_mover_idx=172, ai_stay_behind_idx=173,
                                    ai_stay_behind_n=1, ai_reserve_copy=59, first_push_seeded=172, midi_second_idx=71),
                               dict(ai_trunk=2, zi_trunk=1, nest_trunk_ai=123, midi=1, smo_g_trunk_src=1, smo_nest=4, smo_stale_read=4)),
    "zi_movers_then_stayers": ("pinned3", [(18, 130), (22, 100)],
                               dict(zi_movers=130, zi_copy_len=232, zi_stayers=102, zi_mixed_rnd=3, zi_mover_idx=130, zi_stay_behind_idx=232,
                                    zi_stay_behind_n=102, first_push_seeded=230, cn_list=132, pinned_len=232, pinned_wide=1),
                               dict(zi_trunk=2, nest_trunk_zi=131, midi_same_kind=1, nest_over_pinned=1)),
    # a long vector from which nothing moves
    "ai_nothing_moves_65": ("ai_trunk", [(6, 64)], dict(ai_movers=0, ai_copy_len=65, ai_stayers=65, first_push_seeded=64), dict(ai_trunk=1)),
    "ai_nothing_moves_129": ("ai_trunk", [(6, 128)], dict(ai_movers=0, ai_copy_len=129, ai_stayers=129, first_push_seeded=128), dict(ai_trunk=1)),
    "zi_nothing_moves_65": ("smo_stale_read", [(45, 61)], dict(zi_movers=0, zi_copy_len=65, zi_stayers=65, first_push_seeded=64, midi_first_idx=65),
                            dict(ai_trunk=1, zi_trunk=1, nest_trunk_ai=20, smo_g_trunk_src=1, smo_nest=4, smo_stale_read=4)),
    "zi_nothing_moves_129": ("smo_stale_read", [(45, 125)], dict(zi_movers=0, zi_copy_len=129, zi_stayers=129, first_push_seeded=128, midi_first_idx=129),
                             dict(ai_trunk=1, zi_trunk=1, nest_trunk_ai=20, smo_g_trunk_src=1, smo_nest=4, smo_stale_read=4)),
    # midi: the two trunk concealed children at index 62|63 (one round), 63|64, 127|128, 255|256 (two rounds), 128|129 (one)
    **{f"midi_second_at_{k + 1}": _midi(k) for k in (62, 63, 127, 128, 255)},
    "midi_second_at_64_b": ("pinned10", [(24, 63)],
                            dict(midi_first_idx=64, midi_second_idx=65, midi_split_rounds=1, midi_copy_len=65, midi_stayers=65, midi_movers=0, midi_ntrunk=2),
                            dict(ai_trunk=1, ai_branch=1, zi_trunk=1, nest_trunk_ai=1, midi=1)),
    # smothered: 63 / 64 / 65 / 66 / 129 erasures in one call; the smothered vertex's vector is copied at 32, 64, 128
    "smo_erasures_63": _smo(117, 63, 32), "smo_erasures_64": _smo(119, 64, 32), "smo_erasures_65": _smo(121, 65, 64),
    "smo_erasures_66": _smo(123, 66, 64), "smo_erasures_129": _smo(249, 129, 128),
    # a flubble that took a pinned vertex in and has 63 / 64 / 65 / 129 children when its nestings run
    **{f"pinned_len_{k + 2}": _pinned(k) for k in (61, 62, 63, 127)},
    "pinned_len_65_b": ("nest_over_pinned", [(0, 63)], dict(pinned_len=65, pinned_wide=1, zi_copy_len=65, zi_movers=63, zi_stayers=2),
                        dict(zi_trunk=2, nest_trunk_zi=64, midi_same_kind=1, nest_over_pinned=1)),
    # several wide flubbles in one component (their waves bump one pool_top): 250 children leave one flubble for a concealed
    # vertex, a smothered vertex takes 65 of them; the other flubble keeps 128
    "several_wide": ("smo_stale_read", [(13, 109), (14, 121), (43, 63), (45, 61)],
                     dict(ai_movers=250, ai_copy_len=251, ai_mixed_rnd=4, ai_reserve_copy=128, zi_copy_len=128, zi_stayers=128, zi_movers=0,
                          smo_old_end=251, smo_erasures=65, push_full_s=64, cn_list=2, n_concealed=2),
                     dict(ai_trunk=1, zi_trunk=1, nest_trunk_ai=250, smo_g_trunk_src=1, smo_nest=65, smo_stale_read=65)),
    "two_links_one_flubble": ("smo_stale_read", [(43, 40), (47, 50)],
                              dict(ai_movers=53, ai_copy_len=94, ai_stayers=41, ai_mover_idx=93, ai_mixed_rnd=2, ai_reserve_copy=24, midi_second_idx=42),
                              dict(ai_trunk=2, zi_trunk=1, nest_trunk_ai=73, midi=1, smo_g_trunk_src=1, smo_nest=4, smo_stale_read=4)),
}
# What the search did not find (search(): every seed x every link at k = 70, then every ordered pair of the links that gave a
# copy of >= 70 children alone, at k = 70 and 80): a third trunk concealed child of one flubble (midi_ntrunk stays 2), a
# nesting under a midi bubble or an a-side branch record that moves anything (midi_nest, nest_branch_ai: UNREACHED_RULES), more
# than 2 concealed records of a flubble or 3 smothered ones of a concealed vertex.  "Movers only in the last round" cannot be:
# the copy ends with the new concealed vertex itself, which stays (*_tail_movers is 0 everywhere).
NOT_FOUND = ("midi_third_later", "midi_movers", "aib_movers", "ai_tail_movers", "zi_tail_movers")


def case_graph(name):
    seed, links, _, _ = CASES[name]
    return widened(seed, links)


def stride_graph():
    """More listed flubbles than the 8192 waves of a splice kernel take in two rounds, more concealed vertices than in one:
    [wide] pinned x 200, zi_movers_257 x 20, [wide] pinned x 180, zi_movers_257 x 20, [wide], so wide flubbles stand among
    the first 8192 list entries, in the middle and at the end (some 1.1 * 10^5 vertices)."""
    wide = [case_graph(n)[0] for n in ("several_wide", "ai_movers_129", "smo_erasures_65", "midi_second_at_64", "pinned_len_65")]
    pins = [seed_graph(p) for p in PINNED_SEEDS]
    zi = [case_graph("zi_movers_257")[0]] * 20
    return disjoint_union(wide + pins * 200 + zi + wide + pins * 180 + zi + wide)


def search(k=70, out=sys.stdout):
    """every seed x every link, widened by k: prints the width words that reach 64.  The bound of the search that CASES came
    from: single links at k = 70, pairs of links among those that gave one of the figures alone."""
    for seed, (g, _) in all_seeds().items():
        for link in range(g.n_links):
            wg, tips = widened(seed, [(link, k)])
            rules, w, _ = measure(wg, tips)
            hit = {n: v for n, v in w.items() if v >= 64 and not n.startswith(("cn_list", "n_"))}
            calls = {n: v for n, v in w.items() if v and n.endswith(("ge64", "mixed_round", "tail_movers", "split_rounds", "third_later", "pinned_wide"))}
            if hit or calls:
                print(seed, link, hit, calls, file=out)


if __name__ == "__main__":
    search(int(sys.argv[1]) if len(sys.argv) > 1 else 70)
