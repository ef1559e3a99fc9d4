"""Hand-made lists for the level-0 records of the tree stage's list rankings (list_rank.hip / list_rank.hpp: rec_store /
rec_decode), and the walk that writes them restated in numpy.

A record is one narrow word -- the owner (the walking lane) as a signed delta to the element's bucket x >> b, the
partial sums in small fields -- or, where a field does not fit, an escaped pair of words.  Every case below is named
for the condition it is built to reach; `model_walk` says which elements must escape, `test_rank_records_inputs.py`
checks on the CPU that every case does reach its condition, and `test_gpu_rank_records.py` runs them on the GPU."""
import functools

import numpy as np

NIL = 0xFFFFFFFF
# field widths (list_rank.hpp: REC_T_*, REC_E_*); the GPU test compares them with what the hook reports
DELTA_BITS = 16
TOUR_PBITS = 15
EVT_PBITS = 7
REC_MAX = 0xFFFF  # the events' escaped partials: beyond it the fallback stores final ranks
HALF = 1 << (DELTA_BITS - 1)


def bucket_splitter(q, b):
    q = np.asarray(q, dtype=np.uint64)
    return ((q << np.uint64(b)) | (((q * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - b))).astype(np.int64)


def event_weights(x, wbit):
    """(wa, wb) of event x (rank_l0_weights)."""
    t = x % 3
    if t == 0:
        return 2, 2
    return 0, (-2 if (t == 1 and wbit) else -1)


def model_walk(nxt, heads, wbit, b, events):
    """owner, pa, pd of every element a walk reaches (owner -1 elsewhere), as k_rank_up leaves them: lane q < m starts
    at the splitter of bucket q unless that element heads a list, lane m + h at heads[h]; a walk ends in front of the
    next splitter.  pa = the partial of the first sum, pd = partial(a) - partial(b) (the tour: 0)."""
    n = nxt.size
    m = (n + (1 << b) - 1) >> b
    spl = bucket_splitter(np.arange(m), b)
    is_spl = np.zeros(n, dtype=bool)
    is_spl[spl[spl < n]] = True
    is_head = np.zeros(n, dtype=bool)
    hv = heads[heads != NIL].astype(np.int64)
    is_head[hv] = True
    owner = np.full(n, -1, dtype=np.int64)
    pa = np.zeros(n, dtype=np.int64)
    pd = np.zeros(n, dtype=np.int64)
    starts = [(q, int(spl[q])) for q in range(m) if spl[q] < n and not is_head[spl[q]]]
    starts += [(m + h, int(heads[h])) for h in range(heads.size) if heads[h] != NIL]
    nx = nxt.astype(np.int64)
    nx[nxt == NIL] = -1
    nx = nx.tolist()
    wl = wbit.tolist()
    spl_l = is_spl.tolist()
    for lane, x in starts:
        sa = sb = 0
        while True:
            owner[x], pa[x], pd[x] = lane, sa, sa - sb
            if events:
                wa, wb = event_weights(x, wl[x])
            else:
                wa = 1 if wl[x] else 0
                wb = wa  # (pd stays 0: the tour has one sum)
            sa += wa
            sb += wb
            x = nx[x]
            if x < 0 or spl_l[x]:
                break
    return owner, pa, pd


def must_escape(owner, pa, pd, b, events):
    """The elements whose record cannot be narrow; with a partial beyond REC_MAX the whole ranking stores final ranks."""
    x = np.arange(owner.size)
    d = owner - (x >> b)
    pmax = (1 << (EVT_PBITS if events else TOUR_PBITS)) - 1
    esc = (d < -HALF) | (d >= HALF) | (pa > pmax) | (pd > pmax)
    return esc & (owner >= 0)


class Case:
    """One list set: `order` is visited in sequence, a new list starting at 0 and at every index in `cuts`."""

    def __init__(self, name, n, order, cuts, wbit, events, bits):
        self.name, self.n, self.events, self.bits = name, n, events, bits
        self.order = np.asarray(order, dtype=np.int64)
        self.cuts = np.asarray(cuts, dtype=np.int64)
        self.wbit = np.asarray(wbit, dtype=np.uint8)

    def lists(self):
        nxt = np.full(self.n, NIL, dtype=np.uint32)
        start = np.zeros(self.order.size, dtype=bool)
        start[0] = True
        start[self.cuts] = True
        follow = ~start[1:]
        nxt[self.order[:-1][follow]] = self.order[1:][follow]
        heads = self.order[start].astype(np.uint32)
        return nxt, heads, start

    @functools.lru_cache(maxsize=None)
    def model(self):
        nxt, heads, _ = self.lists()
        owner, pa, pd = model_walk(nxt, heads, self.wbit, self.bits, self.events)
        return owner, pa, pd, must_escape(owner, pa, pd, self.bits, self.events)

    def delta(self):
        owner = self.model()[0]
        return np.where(owner >= 0, owner - (np.arange(self.n) >> self.bits), 0)


def _pools(n, b):
    """splitter of every bucket, and the non-splitter elements of every bucket (lists)."""
    m = (n + (1 << b) - 1) >> b
    spl = bucket_splitter(np.arange(m), b)
    return spl, lambda q: [x for x in range(q << b, min(n, (q + 1) << b)) if x != spl[q]]


def _wbits(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


def delta_edges(events, bits):
    """Four two-element segments whose second element sits in a far bucket: owner delta exactly the smallest value the
    field holds (-HALF) and one below it, exactly the largest (HALF - 1) and one above it."""
    b = bits
    n = (HALF + 64) << b
    spl, members = _pools(n, b)
    order = [members(0)[0]]  # the list's head: the lane of the first splitter behind it keeps its own id
    for own, far in ((1, 1 + HALF), (2, 2 + HALF + 1), (HALF + 10, 11), (HALF + 20, 20)):
        order += [int(spl[own]), members(far)[0]]
    for q in range(40, 48):  # and a local run behind them
        order += [int(spl[q])] + members(q)
    return Case(f"delta_edges-{'events' if events else 'tour'}-b{bits}", n, order, [], _wbits(n, 5 + bits), events, bits)


def partial_edges(events, bits):
    """Segments whose last partial is exactly the field's maximum, and one past it.  The tour: runs of weight-1 elements of
    PMAX + 1 and PMAX + 2 elements.  The events: partial(a) grows by 2 per enter event (x % 3 == 0) -- 126, the largest value
    it can take in 7 bits, and 128; partial(a) - partial(b) grows by 1 per single leave (x % 3 == 2) -- 127 and 128."""
    b = bits
    pmax = (1 << (EVT_PBITS if events else TOUR_PBITS)) - 1
    per = 4 * (pmax + 8) if not events else 4 * 3 * (pmax + 8)
    n = ((per * 8) // 7 + (64 << b)) & ~7
    m = (n + (1 << b) - 1) >> b
    spl = bucket_splitter(np.arange(m), b)
    is_spl = np.zeros(n, dtype=bool)
    is_spl[spl[spl < n]] = True
    free = np.flatnonzero(~is_spl)
    wbit = np.zeros(n, dtype=np.uint8)
    order = [int(free[0])]
    free = free[1:]
    unused = spl[spl < n][4:].tolist()  # a splitter in front of every run: the run is one segment

    def start(residue):
        s = next(x for x in unused if x % 3 == residue)
        unused.remove(s)
        return s

    def take(k, residue=None):
        nonlocal free
        pick = free if residue is None else free[free % 3 == residue]
        got = pick[:k]
        assert got.size == k
        free = np.setdiff1d(free, got, assume_unique=True)
        return got.tolist()

    if not events:
        for length in (pmax + 1, pmax + 2):  # the k-th element behind the splitter has partial k (the splitter's weight is 1 too)
            run = [unused.pop(0)] + take(length - 1)
            wbit[run] = 1
            order += run
    else:
        # (the splitter counts too: a leave in front of the enters adds 1 to the difference, an enter in front of the leaves 2 to partial(a))
        for enters in ((pmax - 1) // 2, (pmax + 1) // 2):  # pa of the element behind them: 126, 128
            order += [start(2)] + take(enters, 0) + take(1, 2)
        for leaves in (pmax, pmax + 1):  # pd of the element behind them: 127, 128
            order += [start(0)] + take(leaves, 2) + take(1, 2)
    return Case(f"partial_edges-{'events' if events else 'tour'}-b{bits}", n, order, [], wbit, events, bits)


def side_by_side(events, bits):
    """Neighbouring buckets alternate between a local run (the bucket's splitter and its own elements: delta 0) and a far
    jump (the splitter, then elements of a bucket beyond the field): narrow and escaped records from neighbouring lanes of
    one wave, and in neighbouring words where they are read."""
    b = bits
    n = (HALF + 600) << b
    spl, members = _pools(n, b)
    order = [members(0)[0]]
    for k in range(1, 130):
        order += [int(spl[2 * k])] + members(2 * k)
        order += [int(spl[2 * k + 1])] + members(2 * k + 1 + HALF + 7)[:3]
    return Case(f"side_by_side-{'events' if events else 'tour'}-b{bits}", n, order, [], _wbits(n, 9 + bits), events, bits)


def many_heads(events, n=200_000):
    """One- and two-element lists over a random permutation: a third of the elements lead their own segment from a head
    lane m + h, whose delta to the element's bucket is whatever h happens to be -- in the field for the early lists of the
    early buckets, beyond it for most."""
    rng = np.random.default_rng(17 + events)
    order = rng.permutation(n).astype(np.int64)
    lens = rng.integers(1, 3, n)
    cuts = np.cumsum(lens)
    cuts = cuts[cuts < n]
    return Case(f"many_heads-{'events' if events else 'tour'}-n{n}", n, order, cuts, _wbits(n, 19), events, 3)


def tiny(events, n):
    return Case(f"tiny-{'events' if events else 'tour'}-n{n}", n, np.random.default_rng(n).permutation(n), [], _wbits(n, n), events, 3)


def three_modes():
    """Events only: local runs (narrow), far jumps (escaped) and one segment of so many enter events that partial(a)
    outgrows REC_MAX: the fallback then stores final ranks over both planes."""
    b = 3
    n = (HALF + 600) << b
    spl, members = _pools(n, b)
    order = [members(0)[0]]
    for k in range(1, 20):
        order += [int(spl[2 * k])] + members(2 * k)
        order += [int(spl[2 * k + 1])] + members(2 * k + 1 + HALF + 7)[:3]
    is_spl = np.zeros(n, dtype=bool)
    is_spl[spl[spl < n]] = True
    x = np.arange(1000 << b, n)
    enters = x[(x % 3 == 0) & ~is_spl[x]][: REC_MAX // 2 + 2]
    assert enters.size == REC_MAX // 2 + 2
    order += [int(spl[900])] + enters.tolist() + [int(x[(x % 3 == 2) & ~is_spl[x]][0])]
    return Case("three_modes-events-b3", n, order, [], _wbits(n, 23), True, b)


EDGE_CASES = [f(ev, bits) for f in (delta_edges, partial_edges, side_by_side) for ev in (False, True) for bits in (3, 6)]
HEAD_CASES = [many_heads(False), many_heads(True)] + [tiny(ev, n) for ev in (False, True) for n in (1, 7)]
