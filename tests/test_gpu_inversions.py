"""GPU inversion calls (povu_hip_call with POVU_HIP_T_INVERSIONS) against the plain-Python restatement
(tests/inversions_ref.py), array for array and VCF text for VCF text: haplotypes of a chain with a forward and a reversed
reference, random walks, a -s forest, references on two components, haplotypes with inverted intervals (runs of more than
64 steps: the wave-per-run kernel), a repeat that 70 paths walk backwards (the wave-per-step head kernel), a graph of more
than 10^5 segments, a small max_steps that drops runs -- each again with the forced second tier --, the same call without
the flag, two graphs in one context, the refusals,
the wide cohort of 131 samples in 261 slots (tests/cohort_cases.py)."""
import numpy as np
import pytest

import cohort_cases as CC
import inversions_ref as I
import vcf_ref as V
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W

pytestmark = pytest.mark.gpu
DATE = "00000000"
NIL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _flags(r):
    if r["vartype"] == "SUBR":
        return H.CALL_SUBR
    return ((H.CALL_ANCHORED if r["vartype"] != "SUB" else 0) | (H.CALL_TANGLED if r["tangled"] else 0) |
            (H.CALL_INS if r["vartype"] == "INS" else 0) | (H.CALL_DEL if r["vartype"] == "DEL" else 0))


def _same(c, want, names, steps, sq, prefixes, text):
    assert c.n_records == len(want)
    cols = dict(path=[r["path"] for r in want], pos=[r["pos"] for r in want], query=[r["q"] for r in want],
                first=[r["first"] for r in want], n_steps=[r["n_steps"] for r in want], flags=[_flags(r) for r in want],
                an=[r["an"] for r in want], ns=[r["ns"] for r in want])
    for k, col in cols.items():
        assert getattr(c, k).tolist() == col, k
    assert c.ac_off.tolist() == np.concatenate([[0], np.cumsum([len(r["ac"]) for r in want], dtype=np.int64)]).tolist()
    assert c.ac.tolist() == [x for r in want for x in r["ac"]]
    gt = [[H.GT_MISSING if g is None else g for g in r["slots"]] for r in want]
    assert c.gt.tolist() == gt
    assert c.vcf_text(date=DATE) == text(names, steps, sq, want, prefixes, date=DATE)


def _check(d, g, paths, prefixes, flags=0, tflags=0, seed=1, max_len=300, max_steps=65536):
    """The call with inversions equals the restatement; the same call without the flag equals the flubble calls alone.
    Returns (calls, records of the restatement, its run statistics)."""
    d.upload(g)
    f = d.decompose(flags=flags)
    d.upload_paths(paths)
    seqs = W.random_sequences(g, seed, max_len=max_len)
    d.upload_sequences(seqs)
    names, steps = list(paths.names), [paths.steps(k) for k in range(len(paths))]
    sq = dict(zip(g.vid.tolist(), seqs))
    sites = V.sites_of_pvst([f.text(i) for i in range(len(f))])
    inv, stats = I.records(names, steps, sq, prefixes, max_steps)
    want = I.merge(V.call(sites, names, steps, sq, prefixes, max_steps), inv)
    c = d.call(f, prefixes, max_steps=max_steps, flags=H.T_INVERSIONS | tflags)
    _same(c, want, names, steps, sq, prefixes, I.vcf_text)
    assert c.n_inv_records == stats["records"] == sum(1 for r in want if r["vartype"] == "SUBR")
    assert c.n_inv_heads == stats["heads"] and c.n_inv_long == stats["long"]
    assert c.n_inv_tier2 == (stats["heads"] if tflags & H.T_FORCE_TIER2 else stats["tier2"])
    plain = d.call(f, prefixes, max_steps=max_steps, flags=tflags)
    flub = [r for r in want if r["vartype"] != "SUBR"]
    _same(plain, flub, names, steps, sq, prefixes, V.vcf_text)
    assert (plain.n_inv_records, plain.n_inv_heads, plain.n_inv_long, plain.n_inv_tier2) == (0, 0, 0, 0)
    return c, want, stats


def _subr(want):
    return [r for r in want if r["vartype"] == "SUBR"]


TIERS = [0, H.T_FORCE_TIER2]


def _component_of(g, v):
    """Segment ids of the connected component of vertex index v."""
    adj = {}
    for a, b in zip(g.v1.tolist(), g.v2.tolist()):
        adj.setdefault(a, []).append(b)
        adj.setdefault(b, []).append(a)
    seen, todo = {v}, [v]
    while todo:
        for u in adj.get(todo.pop(), ()):
            if u not in seen:
                seen.add(u)
                todo.append(u)
    return g.vid[sorted(seen)].tolist()


# ---- the inputs (module level: their conditions can be checked with the restatement alone)

def chain_case():
    return W.chain_of_bubbles(300), W.pansn(W.chain_haplotypes(300, 16, seed=5), samples=8)


def inverted_case(k=400, n_hap=8, n_inv=40, max_len=250, seed=31):
    """Haplotypes of a chain, four of them copies of the first (the reference), with random intervals of every
    haplotype but the first walked backwards: where a copy is inverted the run is as long as the interval."""
    g = W.chain_of_bubbles(k)
    base = W.chain_haplotypes(k, n_hap, seed=seed, reverse_every=0)
    cut = lambda j: (base.ids[int(base.off[j]):int(base.off[j + 1])], base.rev[int(base.off[j]):int(base.off[j + 1])])  # noqa: E731
    p = W._paths(base.names, [cut(0 if 1 <= j <= 4 else j) for j in range(n_hap)])
    return g, W.pansn(W.inverted_haplotypes(p, n_inv, 2, max_len, seed + 1, keep=(0,)), samples=n_hap // 2)


def repeat_case():
    """Four haplotypes of a chain and 70 short paths that each walk a stretch of the first one backwards, all of them ending
    on its step 20: that step has 70 opposite occurrences, its neighbours nearly as many."""
    g = W.chain_of_bubbles(60)
    base = W.chain_haplotypes(60, 4, seed=41, reverse_every=0)
    ref = base.steps(0)
    pieces = [(base.ids[int(base.off[k]):int(base.off[k + 1])], base.rev[int(base.off[k]):int(base.off[k + 1])]) for k in range(4)]
    for k in range(70):
        cut = ref[20:20 + 2 + k % 9][::-1]
        pieces.append((np.array([s for s, _ in cut], np.uint32), np.array([1 - o for _, o in cut], np.uint8)))
    return g, W.pansn(W._paths([f"p{k}" for k in range(len(pieces))], pieces), samples=12)


@pytest.mark.parametrize("tflags", TIERS)
def test_chain_haplotypes_forward_and_reversed_reference(hip, tflags):
    g, p = chain_case()
    c, want, _ = _check(hip, g, p, ["sample0#1"], tflags=tflags)
    assert len(_subr(want)) >= 100 and sum(1 for r in _subr(want) if r["ac"][0] > 1) >= 10
    assert c.device_ms > 0
    c, want, _ = _check(hip, g, p, ["sample1#2"], tflags=tflags, seed=2)  # (every fourth haplotype is written '<')
    assert len(_subr(want)) >= 100 and sum(1 for r in _subr(want) if r["ac"][0] > 1) >= 10
    assert any(r["at"][0].startswith("<") for r in _subr(want))


@pytest.mark.parametrize("tflags", TIERS)
def test_random_walks_subflubbles_and_two_components(hip, tflags):
    g = W.hprc_shaped([500, 300], seed=9, tiny=3)
    rw = W.random_walk_paths(g, 10, 800, seed=4)
    nz = W.noise_paths(g, 4, 300, seed=5)
    both = W.Paths(list(rw.names) + list(nz.names), np.concatenate([rw.off, rw.off[-1] + nz.off[1:]]),
                   np.concatenate([rw.ids, nz.ids]), np.concatenate([rw.rev, nz.rev]))
    _check(hip, g, both, ["walk0", "walk3"], tflags=tflags, seed=4)
    g = W.bubble_zoo(6, 8, 2)
    p = W.pansn(W.random_walk_paths(g, 10, 300, seed=7), samples=5)
    _check(hip, g, p, ["sample0#1"], flags=H.F_SUBFLUBBLES, tflags=tflags, seed=7)
    g = W.hprc_shaped([300, 200], seed=11)
    p = W.pansn(W.random_walk_paths(g, 16, 600, seed=8), samples=4)
    _, want, _ = _check(hip, g, p, ["sample0#", "sample3#2"], tflags=tflags, seed=8)
    # the reference paths with records lie on both components: hprc_shaped numbers the segments component by component
    # (the link arrays join no segment of the first to one of the second), and a random walk stays on its component
    first = set(_component_of(g, 0))
    sides = {all(s in first for s, _ in p.steps(k)) for k in {r["path"] for r in want}}
    assert sides == {True, False}


@pytest.mark.parametrize("tflags", TIERS)
def test_inverted_haplotypes_long_runs_and_dropped_runs(hip, tflags):
    g, p = inverted_case()
    c, want, stats = _check(hip, g, p, ["sample0#1"], tflags=tflags, seed=3, max_len=20)
    assert stats["tier2"] > 0 and max(r["n_steps"] for r in _subr(want)) > 64  # runs the first tier hands over
    assert c.n_inv_tier2 > 0
    # a small max_steps: the longer runs are dropped and counted, in both tiers alike
    c, want, stats = _check(hip, g, p, ["sample0#1"], tflags=tflags, seed=3, max_len=20, max_steps=40)
    assert stats["long"] > 0 and c.n_inv_long == stats["long"] and max(r["n_steps"] for r in _subr(want)) <= 40
    c, want, stats = _check(hip, g, p, ["sample0#1"], tflags=tflags, seed=3, max_len=20, max_steps=100)
    assert stats["long"] > 0 and stats["tier2"] > stats["long"]  # (runs of 65 .. 100 steps are reported by tier 2)


@pytest.mark.parametrize("tflags", TIERS)
def test_a_repeat_with_64_or_more_opposite_occurrences(hip, tflags):
    g, p = repeat_case()
    c, want, stats = _check(hip, g, p, ["sample0#1"], tflags=tflags, seed=6, max_len=8)
    assert stats["max_opposite"] >= 64
    groups = [r for r in _subr(want) if r["first"] == 20]
    assert len(groups) >= 8 and any(r["ac"][0] >= 3 for r in groups)  # one first step, many lengths, several supporters


@pytest.mark.parametrize("tflags", TIERS)
def test_a_graph_of_more_than_1e5_segments_then_a_small_one(hip, tflags):
    g, p = inverted_case(k=40000, n_hap=6, n_inv=40, max_len=3000, seed=13)
    assert g.n_vtx > 100000
    c, want, stats = _check(hip, g, p, ["sample0#1"], tflags=tflags, seed=13, max_len=40)
    assert c.n_records > 10000 and stats["tier2"] > 0 and len(_subr(want)) >= 40
    # the next, smaller graph in the same context: nothing of the large call's workspace shows
    g, p = chain_case()
    _check(hip, g, p, ["sample0#1"], tflags=tflags)


@pytest.mark.parametrize("ref", CC.REFS)
@pytest.mark.parametrize("tflags", TIERS)
def test_wide_cohort(hip, tflags, ref):
    """131 samples, 261 slots (tests/cohort_cases.py): supporters on both sides of lane 63 and past it alone, the reference's
    slot in the first round or in the last, a slot key of nine bits in the sort."""
    g, p = CC.wide_chain()
    c, want, stats = _check(hip, g, p, [ref], tflags=tflags, seed=CC.SEQ_SEED, max_len=CC.MAX_LEN)
    assert c.n_slots == 261 > 256 and len(_subr(want)) >= 32 and stats["max_opposite"] >= 65
    assert max(r["ac"][0] for r in _subr(want)) >= 17


def test_refusals_and_entry_points_that_ignore_the_flag(hip):
    g, p = chain_case()
    hip.upload(g)
    f = hip.decompose()
    hip.upload_paths(p)
    with pytest.raises(RuntimeError, match="no sequences"):
        hip.call(f, ["sample0#1"], flags=H.T_INVERSIONS)
    hip.upload_sequences(["AQ"] * g.n_vtx)
    with pytest.raises(RuntimeError, match="segment \\d+ holds a byte"):
        hip.call(f, ["sample0#1"], flags=H.T_INVERSIONS)
    hip.upload_sequences(W.random_sequences(g, 1))
    with pytest.raises(RuntimeError, match="at least 2"):
        hip.call(f, ["sample0#1"], max_steps=1, flags=H.T_INVERSIONS)
    assert hip.call(f, ["sample0#1"], flags=H.T_INVERSIONS).n_inv_records > 0
    a, b = hip.traversals(f), hip.traversals(f, flags=H.T_INVERSIONS)
    for k in ("path", "first", "last", "allele", "reverse", "step_id", "step_or", "status"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
