"""Hand-made inputs at the tier hand-overs of the walks and the traversals (walk_kernels.hip, trav_kernels.hip), shared by
tests/test_query_tier_inputs.py (no GPU: every case held to the figures of tests/query_tier_model.py) and
tests/test_gpu_query_tiers.py (the device held to walks_ref / traversals_ref and to the model's n_tier2).

Walks, one flubble each unless said otherwise (WALK_CASES: name -> (graph, caps, the query the case is about)):
  arm14 .. arm17      a bubble with one arm of k chained segments: k + 1 frames, a walk of k + 2 steps
  nested13 .. 16      the same bubble inside another: the parent's query needs one frame more
  site4095 .. 4097    m one-segment alleles (one allele of two segments where the count is odd): that many expansions
  budget4095 .. 4097  the site of 4099 expansions with that budget
  slots63 .. 65       boundary sides of exactly that many slots, links shuffled, some doubled; slots64d: 32 doubled links
  wrap4_L, wrap5_L    vertex indices pinned so that the path set of the query's search wraps (16 slots: L = 2, 7, 8; 32: L = 9)
UNION: all of these graphs and a bubble_zoo side by side, a few hundred queries.

Traversals (trav_inputs): chain_of_bubbles, every case on a unit of its own (its neighbours unused), filler steps from the
segments inside the units (never a boundary); every path also written reversed."""
from __future__ import annotations

import functools

import numpy as np

import query_tier_model as M
import traversals_ref as TR
import walks_ref as WR
from povu_amd import workloads as W
from test_walks_ref import graph


def queries_of(g):
    """the queries of a graph in the order the device numbers them, from the CPU oracle"""
    import oracle_lib
    out = oracle_lib.decompose(g)
    return [q for c in sorted(out) for q in WR.queries_of_pvst_text(out[c])]


def index_of(g):
    return {int(v): i for i, v in enumerate(g.vid.tolist())}


# ---- walks

def arm(k: int):
    """1 -> 5 -> 100 and 1 -> 10 -> 11 .. -> 10 + k - 1 -> 100"""
    ids = [1, 5, 100] + list(range(10, 10 + k))
    links = [("1+", "5+"), ("5+", "100+"), ("1+", "10+"), (f"{10 + k - 1}+", "100+")]
    links += [(f"{10 + i}+", f"{11 + i}+") for i in range(k - 1)]
    return graph(ids, links)


def nested(k: int):
    """the arm bubble between 2 and 100, inside 1 -> 2 .. 100 -> 200 | 1 -> 101 -> 200"""
    ids = [1, 2, 5, 100, 101, 200] + list(range(10, 10 + k))
    links = [("1+", "2+"), ("2+", "5+"), ("5+", "100+"), ("2+", "10+"), (f"{10 + k - 1}+", "100+"), ("100+", "200+"), ("1+", "101+"),
             ("101+", "200+")]
    links += [(f"{10 + i}+", f"{11 + i}+") for i in range(k - 1)]
    return graph(ids, links)


def site(m: int, chained: int):
    """m one-segment alleles between 1 and 100000 (two expansions each) and `chained` alleles of two segments (three each)"""
    ids, links = [1, 100000], []
    for i in range(m):
        a = 10 + 3 * i
        ids.append(a)
        links += [("1+", f"{a}+"), (f"{a}+", "100000+")]
    for i in range(chained):
        a = 10 + 3 * (m // 2) + 1 + 3 * i  # (between two alleles, by id)
        ids += [a, a + 1]
        links += [("1+", f"{a}+"), (f"{a}+", f"{a + 1}+"), (f"{a + 1}+", "100000+")]
    return graph(ids, links)


SITE_CAPS = dict(max_walks=4096)
SITE_QUERY = ((1, 0), (100000, 0))


@functools.lru_cache(maxsize=None)
def site_spending(expansions: int):
    """(m, chained) of the site whose search spends exactly that many expansions -- found with the model"""
    for m in range(M.T1_EXPANSIONS // 2 - 8, M.T1_EXPANSIONS // 2 + 8):
        for chained in (0, 1):
            g = site(m, chained)
            if M.search(WR.successors(g), *SITE_QUERY, **dict(WR.DEFAULTS, **SITE_CAPS))["expansions"] == expansions:
                return m, chained
    raise AssertionError(expansions)


def slots_site(singles: int, doubled: int, seed: int):
    """`singles` + `doubled` one-segment alleles between 1 and 5000, both links of the last `doubled` written twice, all links
    shuffled: the two boundary sides have singles + 2 doubled slots"""
    ids, links = [1, 5000], []
    for k in range(singles + doubled):
        a = 10 * (k + 1)
        ids.append(a)
        pair = [("1+", f"{a}-"), (f"{a}-", "5000+")] if k % 5 == 4 else [("1+", f"{a}+"), (f"{a}+", "5000+")]
        links += pair * (2 if k >= singles else 1)
    rng = np.random.default_rng(seed)
    return graph(ids, [links[i] for i in rng.permutation(len(links))])


SLOTS = dict(slots63=(37, 13), slots64=(38, 13), slots64d=(0, 32), slots65=(39, 13))
SLOTS_QUERY = ((1, 0), (5000, 0))

# vertex indices found on the CPU (a random search over the segments whose homes lie in the last two and first two slots, scored
# by the model's events): (segments, S, Z, the arm in link order).  Every other segment is a one-segment allele of the site.
WRAP4 = (64, 9, 1, (27, 40, 61, 14, 17, 51, 19))
WRAP5 = (160, 145, 158, (82, 103, 69, 43, 153, 48, 98))
WRAP_CAPS = dict(max_walks=256)


def wrap_graph(n, s, z, arm_ids):
    ids = list(range(1, n + 1))
    links = [(f"{s}+", f"{arm_ids[0]}+"), (f"{arm_ids[-1]}+", f"{z}+")] + [(f"{a}+", f"{b}+") for a, b in zip(arm_ids, arm_ids[1:])]
    for f in ids:
        if f not in (s, z) and f not in arm_ids:
            links += [(f"{s}+", f"{f}+"), (f"{f}+", f"{z}+")]
    return graph(ids, links)


@functools.lru_cache(maxsize=None)
def walk_cases():
    """name -> (graph, caps, (S, Z) of the query the case is about)"""
    cases = {}
    for k in (14, 15, 16, 17):
        cases[f"arm{k}"] = (arm(k), {}, ((1, 0), (100, 0)))
    for k in (13, 14, 15, 16):
        cases[f"nested{k}"] = (nested(k), {}, ((1, 0), (200, 0)))
    for x in (M.T1_EXPANSIONS - 1, M.T1_EXPANSIONS, M.T1_EXPANSIONS + 1):
        cases[f"site{x}"] = (site(*site_spending(x)), dict(SITE_CAPS), SITE_QUERY)
    big = site(*site_spending(M.T1_EXPANSIONS + 3))
    for e in (M.T1_EXPANSIONS - 1, M.T1_EXPANSIONS, M.T1_EXPANSIONS + 1):
        cases[f"budget{e}"] = (big, dict(SITE_CAPS, max_expansions=e), SITE_QUERY)
    for name, (singles, doubled) in SLOTS.items():
        cases[name] = (slots_site(singles, doubled, 11), dict(max_walks=200), SLOTS_QUERY)
    for L in (2, 7, 8, 9):
        for tag, (n, s, z, arm_ids) in (("wrap4", WRAP4), ("wrap5", WRAP5)):
            cases[f"{tag}_{L}"] = (wrap_graph(n, s, z, arm_ids), dict(WRAP_CAPS, max_steps=L), ((s, 0), (z, 0)))
    return cases


def caps_of(caps):
    return dict(WR.DEFAULTS, **caps)


def side_by_side(graphs):
    """the graphs as the components of one, ids shifted so that they ascend with the vertex index"""
    vid, v1, s1, v2, s2 = [], [], [], [], []
    base, first = 0, 0
    for g in graphs:
        vid.append(g.vid.astype(np.int64) + base)
        v1.append(g.v1.astype(np.int64) + first)
        v2.append(g.v2.astype(np.int64) + first)
        s1.append(g.s1)
        s2.append(g.s2)
        base = int(vid[-1].max()) + 1
        first += g.n_vtx
    return W._mk(np.concatenate(vid), np.concatenate(v1), np.concatenate(s1), np.concatenate(v2), np.concatenate(s2))


UNION_ZOO = (60, 8, 3)


@functools.lru_cache(maxsize=None)
def union():
    c = walk_cases()
    names = ["wrap4_8", "wrap5_9"] + [n for n in c if n.startswith(("arm", "nested", "site", "slots"))] + ["budget4096"]
    return side_by_side([c[n][0] for n in names] + [W.bubble_zoo(*UNION_ZOO)])


# caps of the lane-reuse runs: tier 2 forced, the lane's stack of max_steps frames; the caps that stop searches early in the same call
REUSE_MAX_STEPS = (1 << 20, 1 << 22, 1 << 24)
REUSE_CAPS = (dict(), dict(max_walks=2, max_expansions=30))


# ---- traversals

TRAV_UNITS = 64
CLOSE_AT = (63, 64, 65, 66, 127, 128, 129, 193)
END_AT = (64, 65, 66)
STRAY_AT = (64, 65)
TRAV_MAX_STEPS = (TR.DEFAULT_MAX_STEPS, 64, 65, 66, 129, 130)  # a traversal's length and one less: lengths 65, 66, 130
TASKS_CHAIN = (1366, 12)  # chain_of_bubbles(k) under n haplotypes: the smallest k whose k n tasks exceed 4 x 4096 waves


def _unit(u):
    return (3 * u + 1, 0), (3 * u + 4, 0)


def _filler(n, at):
    """n steps inside the units (ids 3 i + 2 and 3 i + 3: no boundary of any query), both orientations"""
    out = []
    for k in range(at, at + n):
        i = k % (2 * TRAV_UNITS)
        out.append((3 * (i // 2) + 2 + (i % 2), k % 3 == 0))
    return [(a, int(o)) for a, o in out]


def _reversed(p):
    return [TR.flip(x) for x in reversed(p)]


@functools.lru_cache(maxsize=None)
def trav_inputs():
    """(graph, paths, {case name: (unit, [its paths])}): a closing step at every offset of CLOSE_AT, a path that ends at every
    offset of END_AT, a stray boundary step at those of STRAY_AT, and three 130-step traversals of one unit, two of them equal"""
    g = W.chain_of_bubbles(TRAV_UNITS)
    paths, cases = [], {}
    unit = 1

    def add(name, *ps):
        nonlocal unit
        mine = []
        for p in ps:
            mine.append(len(paths))
            paths.append(p)
        cases[name] = (unit, mine)
        unit += 2
        assert unit < TRAV_UNITS

    for d in CLOSE_AT:
        s, z = _unit(unit)
        p = [s] + _filler(d - 1, d) + [z] + _filler(3, 7)
        add(f"close{d}", p, _reversed(p))
    for e in END_AT:
        s, z = _unit(unit)
        add(f"end{e}", [s] + _filler(e - 1, e), [TR.flip(z)] + _filler(e - 1, 2 * e))  # (a forward and a reverse scan)
    for d in STRAY_AT:
        s, z = _unit(unit)
        p = [s] + _filler(d - 1, d) + [TR.flip(s)] + _filler(5, 9)
        add(f"stray{d}", p, _reversed(p))
    s, z = _unit(unit)
    same = [s] + _filler(128, 40) + [z]
    other = list(same)
    other[128] = TR.flip(other[128])
    add("dedup130", same, other, _reversed(same))
    return g, paths, cases
