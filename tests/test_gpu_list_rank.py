"""The tree stage's list ranking (rank_tour / rank_events, list_rank.hip) against a host suffix-sum reference.

Level 0 of the ranking leaves a record per element on its only walk ({owner, partial sums}); the kernels that
read a rank resolve it as R[owner] - partial.  These tests resolve every element the same way
(povu_hip_debug_list_rank) and compare with numpy: the tour's 0/1 weights and the pre-order events' pair of
sums, many heads and one-element lists, segments longer than the events' 16-bit partials can count (the
fallback that walks the list a second time), and lists that leave too many elements for the one-workgroup top
level (the global-memory pointer jumping)."""
import numpy as np
import pytest

import oracle_lib as O
from povu_amd import HipDecomposer, workloads as W

pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
RANK_TOP = 8192  # elements the top level ranks in one workgroup (list_rank.hip)


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def make_lists(order, cuts):
    """Lists that visit `order` in sequence, a new list starting at every index in `cuts` (and at 0)."""
    n_all = int(order.max()) + 1 if order.size else 0
    nxt = np.full(n_all, NIL, dtype=np.uint32)
    start = np.zeros(order.size, dtype=bool)
    start[0] = True
    start[np.asarray(cuts, dtype=np.int64)] = True
    follow = ~start[1:]
    nxt[order[:-1][follow]] = order[1:][follow]
    return nxt, order[start].astype(np.uint32)


def weights(n, events, wbit):
    """(a, b) weights of every element: the tour's 0/1 weight, or the events' pair (rank_l0_weights)."""
    if not events:
        return wbit.astype(np.int64), None
    t = np.arange(n) % 3
    wa = np.where(t == 0, 2, 0)
    wb = np.where(t == 0, 2, np.where((t == 1) & (wbit != 0), -2, -1))
    return wa.astype(np.int64), wb.astype(np.int64)


def suffix_sums(order, heads_mask, w):
    """Inclusive suffix sums of w along the lists that visit `order` in sequence (a list begins where heads_mask)."""
    wo = w[order]
    c = np.concatenate([[0], np.cumsum(wo)])
    starts = np.flatnonzero(heads_mask)
    ends = np.concatenate([starts[1:], [order.size]])
    end_of = np.repeat(ends, ends - starts)
    out = np.zeros(w.size, dtype=np.int64)
    out[order] = c[end_of] - c[np.arange(order.size)]
    return (out & 0xFFFFFFFF).astype(np.uint32)


def check(hip, n, order, cuts, wbit, events, bits=0):
    nxt, heads = make_lists(order, cuts)
    if nxt.size < n:  # elements in no list: inert words
        nxt = np.concatenate([nxt, np.full(n - nxt.size, NIL, dtype=np.uint32)])
    hm = np.zeros(order.size, dtype=bool)
    hm[0] = True
    hm[np.asarray(cuts, dtype=np.int64)] = True
    wa, wb = weights(n, events, wbit)
    got = hip.debug_list_rank(nxt, wbit, heads, events=events, bits=bits)
    if events:
        ga, gb = got
        assert np.array_equal(ga[order], suffix_sums(order, hm, wa)[order])
        assert np.array_equal(gb[order], suffix_sums(order, hm, wb)[order])
    else:
        assert np.array_equal(got[order], suffix_sums(order, hm, wa)[order])


def bucket_splitter(q, b):
    q = np.asarray(q, dtype=np.uint64)
    return ((q << np.uint64(b)) | (((q * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - b))).astype(np.int64)


def top_level_size(n, nh, b):
    """Elements of the top level the ranking plans for n elements and nh heads."""
    cur, levels = n, 0
    while True:
        m = (cur + (1 << b) - 1) >> b
        nxt = m + nh
        levels += 1
        if nxt <= RANK_TOP or nxt > cur // 2 or levels == 12:
            return nxt
        cur = nxt


@pytest.mark.parametrize("events", [False, True])
@pytest.mark.parametrize("n", [1, 7, 8193, 1_000_003])
def test_one_list(hip, n, events):
    rng = np.random.default_rng(n + events)
    order = rng.permutation(n).astype(np.int64)
    check(hip, n, order, [], rng.integers(0, 2, n).astype(np.uint8), events)


@pytest.mark.parametrize("events", [False, True])
def test_many_heads_and_one_element_lists(hip, events):
    n = 600_000
    rng = np.random.default_rng(11 + events)
    order = rng.permutation(n).astype(np.int64)
    lens = rng.integers(1, 40, n)  # many short lists; about one in 20 has a single element
    lens[::7] = 1
    cuts = np.cumsum(lens)
    cuts = cuts[cuts < n]
    check(hip, n, order, cuts, rng.integers(0, 2, n).astype(np.uint8), events)


@pytest.mark.parametrize("events", [False, True])
def test_elements_in_no_list(hip, events):
    """Inert elements (no successor, no head; the tour's non-arc slots) around the lists leave the ranks alone."""
    n = 300_000
    rng = np.random.default_rng(21 + events)
    members = rng.permutation(n)[: n // 2].astype(np.int64)
    cuts = np.sort(rng.choice(np.arange(1, members.size), 500, replace=False))
    check(hip, n, members, cuts, rng.integers(0, 2, n).astype(np.uint8), events)


@pytest.mark.parametrize("bits", [3, 6])
@pytest.mark.parametrize("events", [False, True])
def test_segments_longer_than_any_packed_field(hip, events, bits):
    """A list that runs through every non-splitter element before any splitter: its first segment holds all but
    n / 2^bits elements, so its partial sums reach ~2n -- beyond the 16 bits of an event record (the fallback runs)
    and far beyond any segment of the other tests (the tour's records hold 32-bit partials)."""
    n = 3 * (1 << 18)
    b = bits
    spl = bucket_splitter(np.arange((n + (1 << b) - 1) >> b), b)
    spl = spl[spl < n]
    is_spl = np.zeros(n, dtype=bool)
    is_spl[spl] = True
    order = np.concatenate([np.flatnonzero(~is_spl), np.flatnonzero(is_spl)]).astype(np.int64)
    assert (~is_spl).sum() > 100_000  # one segment of > 10^5 elements
    rng = np.random.default_rng(31 + events + bits)
    check(hip, n, order, [], rng.integers(0, 2, n).astype(np.uint8), events, bits=bits)


@pytest.mark.parametrize("events", [False, True])
def test_global_memory_top_level(hip, events):
    """So many lists that the levels stop shrinking with more than one workgroup's worth left on top."""
    n = 240_000
    rng = np.random.default_rng(41 + events)
    order = rng.permutation(n).astype(np.int64)
    cuts = np.arange(2, n, 2)  # lists of two
    assert top_level_size(n, cuts.size + 1, 3) > RANK_TOP
    check(hip, n, order, cuts, rng.integers(0, 2, n).astype(np.uint8), events, bits=3)


def test_many_tiny_components_match_oracle(hip):
    """Whole passes whose two rankings both take the global-memory top level (tens of thousands of components,
    one list each), against the oracle."""
    g = W.hprc_shaped([300], seed=17, tiny=20000)
    n_seg = int(g.vid.size)
    assert top_level_size(3 * n_seg, 20001, 3) > RANK_TOP
    hip.upload(g)
    assert hip.decompose().texts() == O.decompose(g)
