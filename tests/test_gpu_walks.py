"""povu_hip_forest_walks (HipDecomposer.walks) and povu_flubbles_get on the MI355X, array for array against the plain-Python
restatement of tests/walks_ref.py: both tiers, every cap, plain and -s forests, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import walks_ref as R
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W
from test_walks_ref import HAND, NESTED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _queries(f, sub):
    qs = []
    for i in range(len(f)):
        if sub:
            t = f.subtree(i)
            qs += [((int(t["id1"][v]), int(t["or1"][v])), (int(t["id2"][v]), int(t["or2"][v]))) for v in range(1, t["n_total"])]
        else:
            t = f.tree(i)
            qs += R.queries_of_arrays(t.a_id, t.a_or, t.z_id, t.z_or)
    return qs


def _check(d, g, flags=0, force2=False, sample=None, **caps):
    """decompose + walks of graph g, compared with the restatement (all queries, or `sample` random ones)."""
    d.upload(g)
    f = d.decompose(flags=flags)
    c = dict(R.DEFAULTS, **caps)
    w = d.walks(f, flags=H.W_FORCE_TIER2 if force2 else 0, **c)
    qs = _queries(f, bool(flags & H.F_SUBFLUBBLES))
    assert w.n_queries == len(qs)
    assert int(w.walk_off[-1]) == w.n_walks and int(w.step_off[-1]) == w.n_steps
    assert np.all(np.diff(w.walk_off.astype(np.int64)) >= 0) and np.all(np.diff(w.step_off.astype(np.int64)) >= 0)
    if force2:
        assert w.n_tier2 == len(qs)
    succ = R.successors(g)
    if sample is None:
        want = R.flat(succ, qs, **c)
        for k in ("walk_off", "step_off", "step_id", "step_or", "status"):
            assert np.array_equal(getattr(w, k), want[k]), k
    else:
        rng = np.random.default_rng(7)
        for q in rng.choice(len(qs), size=min(sample, len(qs)), replace=False).tolist():
            ws, st = R.walks_of(succ, *qs[q], **c)
            assert w.walks_of_query(q) == [[(i, ">" if o == 0 else "<") for i, o in x] for x in ws], q
            assert int(w.status[q]) == st, q
    return f, w, qs


@pytest.mark.parametrize("force2", [False, True])
def test_hand_cases(hip, force2):
    seen = 0
    for name, (g, s, z) in HAND.items():
        f, w, qs = _check(hip, g, force2=force2)
        if (s, z) in qs:  # the hand answer where the decomposition has that flubble
            q = qs.index((s, z))
            ws, st = R.walks_of(R.successors(g), s, z)
            assert w.walks_of_query(q) == [[(i, ">" if o == 0 else "<") for i, o in x] for x in ws], name
            seen += 1
    assert seen >= 3
    g, s, z = NESTED
    hip.upload(g)
    f = hip.decompose()
    w = hip.walks(f)
    t = f.tree(0)
    v = [k for k in range(1, len(t.a_id)) if (t.a_id[k], t.z_id[k]) == (1, 6)]
    assert len(v) == 1
    ws, st = w.of(0, v[0])
    assert st == 0
    assert ["".join(o + str(i) for i, o in x) for x in ws] == [">1>2>3>5>6", ">1>2>4>5>6", ">1>7>8>10>6", ">1>7>9>10>6"]


@pytest.mark.parametrize("force2", [False, True])
def test_hand_cases_with_small_caps(hip, force2):
    for g, _, _ in HAND.values():
        _check(hip, g, force2=force2, max_walks=1)
        _check(hip, g, force2=force2, max_steps=2)
        _check(hip, g, force2=force2, max_steps=1)
        _check(hip, g, force2=force2, max_expansions=3)


@pytest.mark.parametrize("force2", [False, True])
def test_zoo_chain_towers_hprc(hip, force2):
    for g in (W.bubble_zoo(6, 8, 3), W.bubble_zoo(4, 10, 11), W.chain_of_bubbles(300), W.nested_towers(5, 4),
              W.hprc_shaped([400, 150], seed=3, tiny=5)):
        _check(hip, g, force2=force2)


def test_zoo_ids_are_shuffled_and_not_contiguous(hip):
    g = W.bubble_zoo(6, 8, 3)
    g = W._mk(g.vid * 3 + 7, g.v1, g.s1, g.v2, g.s2)  # ascending, with gaps
    _check(hip, g)
    _check(hip, g, force2=True)


@pytest.mark.parametrize("force2", [False, True])
def test_every_cap_and_both_truncation_paths(hip, force2):
    # nested towers: deep sites with many walks -- every status bit, and (without force2) hand-overs from tier 1
    g = W.nested_towers(7, 3)
    for caps in (dict(max_walks=2), dict(max_steps=5), dict(max_expansions=20), dict(max_walks=3, max_steps=6, max_expansions=40),
                 dict(max_steps=40, max_expansions=5000)):
        f, w, qs = _check(hip, g, force2=force2, **caps)
    _, w, _ = _check(hip, g, force2=force2, max_walks=2, max_steps=6, max_expansions=30)
    bits = np.bitwise_or.reduce(w.status)
    assert bits & R.MORE and bits & R.LONG


def test_tier1_hands_over_deep_and_long_searches(hip):
    # a chain of 40 bubbles inside one flubble: walks deeper than tier 1's stack, and 2^40 of them (MORE at K)
    k = 40
    links = [("1+", "2+"), ("1+", f"{3 * k + 5}+"), (f"{3 * k + 5}+", f"{3 * k + 4}+")]
    for i in range(k):
        a = 2 + 3 * i
        links += [(f"{a}+", f"{a + 1}+"), (f"{a}+", f"{a + 2}+"), (f"{a + 1}+", f"{a + 3}+"), (f"{a + 2}+", f"{a + 3}+")]
    links.append((f"{3 * k + 2}+", f"{3 * k + 4}+"))
    from test_walks_ref import graph
    g = graph(range(1, 3 * k + 6), links)
    f, w, qs = _check(hip, g)
    assert w.n_tier2 >= 1
    assert np.bitwise_or.reduce(w.status) & R.MORE
    _check(hip, g, max_expansions=100000)
    _check(hip, g, max_steps=30)


def _hub_site(n_alleles=100, seed=5):
    """A site of `n_alleles` one-segment alleles between 1 and 5000 (every fifth allele inverted, one allele holding a
    bubble of its own), its links in shuffled order and every seventh link doubled: both sides of the site's boundary
    segments carry more than 64 links."""
    from test_walks_ref import graph
    links, ids = [], [1, 5000]
    for k in range(n_alleles):
        a = 10 * (k + 1)
        ids.append(a)
        if k % 5 == 4:
            links += [("1+", f"{a}-"), (f"{a}-", "5000+")]
        elif k == 3:
            ids += [a + 1, a + 2, a + 3]
            links += [("1+", f"{a}+"), (f"{a}+", f"{a + 1}+"), (f"{a}+", f"{a + 2}+"), (f"{a + 1}+", f"{a + 3}+"),
                      (f"{a + 2}+", f"{a + 3}+"), (f"{a + 3}+", "5000+")]
        else:
            links += [("1+", f"{a}+"), (f"{a}+", "5000+")]
    links += [links[i] for i in range(0, len(links), 7)]
    rng = np.random.default_rng(seed)
    links = [links[i] for i in rng.permutation(len(links))]
    return graph(ids, links)


@pytest.mark.parametrize("force2", [False, True])
def test_hub_sides_sorted_by_the_radix_path(hip, force2):
    g = _hub_site()
    succ = R.successors(g)
    assert max(np.bincount(np.concatenate([g.v1 * 2 + g.s1, g.v2 * 2 + g.s2]))) > 64
    assert len(succ[(1, 1)]) == 100
    for caps in (dict(), dict(max_walks=200), dict(max_walks=200, max_expansions=150), dict(max_steps=3)):
        f, w, qs = _check(hip, g, force2=force2, **caps)
        q = qs.index(((1, 0), (5000, 0)))
        got = w.walks_of_query(q)
        assert got[0] == [(1, ">"), (10, ">"), (5000, ">")]
        if not caps:
            assert len(got) == 64 and int(w.status[q]) == R.MORE
        if caps == dict(max_walks=200):
            assert len(got) == 101 and int(w.status[q]) == 0
            assert [(50, "<")] == [s for s in got[5] if s[0] == 50]


@pytest.mark.parametrize("seed", range(6))
def test_random_bidirected_fuzz(hip, seed):
    g = W.random_bidirected(60 + 20 * seed, 90 + 30 * seed, 100 + seed)
    _check(hip, g, max_expansions=4000)
    _check(hip, g, max_walks=4, max_steps=12, max_expansions=300)
    _check(hip, g, force2=True, max_walks=4, max_steps=12, max_expansions=300)


def test_subflubble_forest_queries(hip):
    for g in (W.bubble_zoo(6, 8, 3), W.bubble_zoo(8, 8, 5)):
        f, w, qs = _check(hip, g, flags=H.F_SUBFLUBBLES)
        fams = set()
        for i in range(len(f)):
            fams |= set(bytes(f.subtree(i)["fam"]).decode())
        assert {"C", "M", "S"} & fams  # inserted vertices are queries too
        assert len(qs) > sum(len(f.tree(i).a_id) - 1 for i in range(len(f)))
        _check(hip, g, flags=H.F_SUBFLUBBLES, force2=True, max_walks=2)


def test_million_segments_totals_and_sample(hip):
    g = W.hprc_shaped([600000], seed=3, tiny=5)
    assert g.n_vtx >= 900000
    f, w, qs = _check(hip, g, sample=2000)
    # the walks of every query: segments of the graph, starting at S and ending at Z
    assert w.n_queries == len(qs)
    firsts = w.step_off[w.walk_off[:-1][np.diff(w.walk_off) > 0]]
    assert np.isin(w.step_id, g.vid).all()
    q_with = np.flatnonzero(np.diff(w.walk_off) > 0)
    assert np.array_equal(w.step_id[firsts], np.array([qs[q][0][0] for q in q_with], np.uint32))
    lasts = w.step_off[w.walk_off[1:][np.diff(w.walk_off) > 0]] - 1
    assert np.array_equal(w.step_id[lasts], np.array([qs[q][1][0] for q in q_with], np.uint32))


def test_refused_after_a_second_upload_and_for_sharded_forests(hip):
    g = W.chain_of_bubbles(50)
    hip.upload(g)
    f = hip.decompose()
    hip.walks(f)
    hip.upload(g)
    with pytest.raises(RuntimeError, match="uploaded again"):
        hip.walks(f)
    f2 = hip.decompose()
    assert hip.walks(f2).n_queries == sum(len(f2.tree(i).a_id) - 1 for i in range(len(f2)))
    fs = hip.decompose(rank=0, world=2)
    with pytest.raises(RuntimeError, match="sharded"):
        hip.walks(fs)
    merged = hip.merge_forests([f2.pack()])
    assert len(merged) == len(f2)
    with pytest.raises(RuntimeError, match="merged"):
        hip.walks(merged)
    other = HipDecomposer(0)
    try:
        other.upload(g)
        with pytest.raises(RuntimeError, match="another context"):
            other.walks(f2)
    finally:
        other.close()


class _Step(C.Structure):
    _fields_ = [("vertex_id", C.c_uint64), ("orientation", C.c_int)]


class _Flubble(C.Structure):
    _fields_ = [("id", C.c_uint64), ("type_name", C.c_char_p), ("start_vertex_id", C.c_uint64), ("end_vertex_id", C.c_uint64),
                ("walks", C.POINTER(C.POINTER(_Step))), ("walk_lengths", C.POINTER(C.c_size_t)), ("walks_count", C.c_size_t)]


def test_ffi_flubbles_get_end_to_end():
    from test_cabi_and_host import _Err, _ffi
    lib = _ffi()
    lib.povu_flubbles_get.restype = C.POINTER(_Flubble)
    lib.povu_flubble_free.argtypes = [C.POINTER(_Flubble)]
    lib.povu_flubbles_free.argtypes = [C.c_void_p]
    lib.povu_graph_finalize.argtypes = [C.c_void_p]
    # builder graph with ids 10, 20, 30 ...: NESTED and a SNP next to it, as a second component
    g, _, _ = NESTED
    gh = lib.povu_graph_new(16, 16, 0)
    ids = [int(x) * 10 for x in g.vid.tolist()] + [200, 210, 220, 230]
    for i in ids:
        assert lib.povu_graph_add_vertex(gh, i, b"A") != 2 ** 64 - 1
    edges = [(ids[a], s1, ids[b], s2) for a, s1, b, s2 in zip(g.v1.tolist(), g.s1.tolist(), g.v2.tolist(), g.s2.tolist())]
    edges += [(200, W.R, 210, W.L), (200, W.R, 220, W.L), (210, W.R, 230, W.L), (220, W.R, 230, W.L)]
    for a, sa, b, sb in edges:  # FORWARD = left end, REVERSE = right end
        assert lib.povu_graph_add_edge(gh, a, 0 if sa == W.L else 1, b, 0 if sb == W.L else 1) != 2 ** 64 - 1
    lib.povu_graph_finalize(gh)
    err = _Err(0, None)
    fl = lib.povu_graph_find_flubbles(gh, C.byref(err))
    assert fl, err.message
    n = lib.povu_flubbles_count(fl)
    assert n >= 4
    assert not lib.povu_flubbles_get(fl, 0)
    assert not lib.povu_flubbles_get(fl, n)
    links = W._mk(np.array(ids), [ids.index(a) for a, _, _, _ in edges], [s for _, s, _, _ in edges],
                  [ids.index(b) for _, _, b, _ in edges], [s for _, _, _, s in edges])
    succ = R.successors(links)
    got_any = 0
    for i in range(1, n):
        p = lib.povu_flubbles_get(fl, i)
        assert p, i
        x = p.contents
        assert x.id == i and x.type_name == b"flubble"
        assert x.start_vertex_id in ids and x.end_vertex_id in ids
        walks = [[(x.walks[k][j].vertex_id, x.walks[k][j].orientation) for j in range(x.walk_lengths[k])]
                 for k in range(x.walks_count)]
        s = (x.walks[0][0].vertex_id, x.walks[0][0].orientation) if x.walks_count else None
        if s is not None:
            z = walks[0][-1]
            assert s[0] == x.start_vertex_id and z[0] == x.end_vertex_id
            want, st = R.walks_of(succ, s, z)
            assert walks == [[(a, o) for a, o in w] for w in want], i
            got_any += 1
        lib.povu_flubble_free(p)
    assert got_any >= 3
    # the outer site of NESTED, ids x10: four walks in id order
    outer = [lib.povu_flubbles_get(fl, i) for i in range(1, n)]
    texts = []
    for p in outer:
        x = p.contents
        if x.start_vertex_id == 10 and x.end_vertex_id == 60:
            texts = ["".join((">" if x.walks[k][j].orientation == 0 else "<") + str(x.walks[k][j].vertex_id)
                             for j in range(x.walk_lengths[k])) for k in range(x.walks_count)]
        lib.povu_flubble_free(p)
    assert texts == [">10>20>30>50>60", ">10>20>40>50>60", ">10>70>80>100>60", ">10>70>90>100>60"]
    lib.povu_flubbles_free(fl)
    lib.povu_graph_free(gh)
