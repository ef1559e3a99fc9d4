"""Inputs and references of the look-up structures' GPU tests (tests/test_gpu_lookups.py): the coarse min segment tree
(segtree.hpp), the bit-rank directory and append_in_order (common.hpp).  Every generator exists for a property of its
output -- a place where a build or a query takes another path --, and tests/test_lookups_inputs.py asserts those
properties on the references alone, without a GPU.  None of the references shares the logic of the structure it checks:
the segment tree's are a brute force over a (query x value) matrix at small sizes, sorted hit lists and chunked minima
(chunks of 1000, unrelated to the blocks of 16) at large ones."""
import numpy as np

from primitives_cases import rng_of

# ---- these MIRROR constants of povu_amd/csrc/hip/segtree.hpp, par_kernels.hpp, common.hpp and primitives.hip: when one
# changes there, change it here, and the sizes below move with it
SEG_BLK = 16  # values a leaf of the tree stands for (SegTree::BLK): the queries read whole blocks with four 16-byte loads
SEG_TPB = 256  # blocks a workgroup of k_seg_bottom reduces: its subtree's levels are written by that workgroup
SEG_TOP_LANES = 1024  # lanes of k_seg_top's one workgroup: a level of more nodes than that makes its loop stride
BR_FLAGS = 64  # flags a record of the bit-rank directory
BR_WAVE = 256  # positions a wave hands to bitrank_store_wave (four a lane): four records
LIST_ITER, LIST_TPB = 16, 256  # rounds and lanes of a workgroup of append_in_order
LIST_SPAN = LIST_TPB * 4 * LIST_ITER  # positions a workgroup covers with one atomic add
NIL = 0xFFFFFFFF

SEG_MIN, SEG_FIRST_LESS, SEG_LAST_LESS = range(3)  # query kinds (include/povu_hip.h)
CHUNK = 1000  # of the chunked minima of the reference


# ============================================================================================== segment tree: sizes
SEG_SMALL_N = [0, 1, 15, 16, 17, 33, 213]  # every range is asked
SEG_LARGE_N = [4095, 4096, 4097, 8193, 100003, 1 << 23, (1 << 23) + 1]  # about 2 * 10^4 queries each
SEG_N = SEG_SMALL_N + SEG_LARGE_N
SEG_VALUES = ["random", "small", "flags", "ascending", "descending", "sparse", "low0", "low15"]
LOW, HIGH = 5, 1000  # the low kinds: the value of the chosen positions, and a lower bound of all others


def seg_P(n):
    """Leaves of the tree over n values: their blocks, rounded up to a power of two, at least 1 (seg_build)."""
    p = 1
    while p * SEG_BLK < n:
        p *= 2
    return p


def seg_top_nodes(n):
    """The `top_nodes` k_seg_top is launched with; 0 when the bottom kernel's one workgroup writes the whole tree."""
    return seg_P(n) // SEG_TPB if seg_P(n) > SEG_TPB else 0


def low_blocks(n):
    """The blocks of the low kinds that hold a low value: random gaps of 1..5 blocks up to 1000 values, 1..8 up to 10 000, 1..60 beyond."""
    blocks = (n + SEG_BLK - 1) // SEG_BLK
    rng = rng_of("low_blocks", n)
    gaps = rng.integers(1, 6 if n <= 1000 else 9 if n <= 10000 else 61, blocks + 1)
    b = np.cumsum(gaps) - gaps[0] + int(rng.integers(0, 2))
    return b[b < blocks]


def seg_values(kind, n):
    """n values of one of SEG_VALUES (uint32)."""
    rng = rng_of("seg_" + kind, n)
    full = lambda k: rng.integers(0, 1 << 32, k, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    if kind == "random":  # the whole range, one value in 16 NIL
        v = full(n)
        v[rng.random(n) < 1 / 16] = NIL
    elif kind == "small":  # ties everywhere: strictness of <, first != last
        v = rng.integers(0, 4, n).astype(np.uint32)
    elif kind == "flags":  # 0 / 1, asked with threshold 1 (the hairpin flags of the inserting passes)
        v = (rng.random(n) < 0.9).astype(np.uint32)
    elif kind == "ascending":  # every range's minimum at its left edge
        v = np.arange(n, dtype=np.uint32) + np.uint32(7)
    elif kind == "descending":  # ... at its right edge
        v = (np.arange(n, dtype=np.uint32) + np.uint32(7))[::-1].copy()
    elif kind == "sparse":  # like `prev`: mostly NIL
        v = np.full(n, NIL, dtype=np.uint32)
        hit = rng.random(n) < 1 / 50
        v[hit] = rng.integers(0, max(n, 1), int(hit.sum())).astype(np.uint32)
    elif kind in ("low0", "low15"):  # one low value a chosen block, at its first / last offset
        v = (rng.integers(HIGH, 1 << 31, n)).astype(np.uint32)
        p = low_blocks(n) * SEG_BLK + (0 if kind == "low0" else SEG_BLK - 1)
        v[p[p < n]] = LOW
    else:
        raise ValueError(kind)
    return v


def seg_thresholds(kind, val):
    """The thresholds every range is asked at: 0 (nothing qualifies), 1, a value that occurs, that value + 1, NIL."""
    live = val[val != NIL]
    if kind in ("low0", "low15") and (val == LOW).any():
        v = LOW  # v + 1: the chosen positions qualify and nothing else
    elif live.size:
        v = int(np.partition(live, live.size // 2)[live.size // 2])  # the median of the values that are not NIL
    else:
        v = 7
    return sorted({0, 1, v, v + 1, NIL})


# ============================================================================================== segment tree: references
def _pairs_reduce(a, lo, hi):
    """min(a[lo[k]:hi[k]]) for every k, NIL where lo[k] >= hi[k]; a: uint32, hi <= a.size."""
    out = np.full(lo.size, NIL, dtype=np.uint32)
    ok = np.flatnonzero(lo < hi)
    ok = ok[np.argsort(-lo[ok], kind="stable")]  # (descending lo: the stretches between two pairs, reduced as well, are single elements)
    if ok.size:
        ext = np.concatenate([a, np.array([NIL], dtype=np.uint32)])  # (reduceat wants indices below the length)
        idx = np.empty(2 * ok.size, dtype=np.int64)
        idx[0::2], idx[1::2] = lo[ok], hi[ok]
        out[ok] = np.minimum.reduceat(ext, idx)[0::2]
    return out


class SegRef:
    """References of the three queries over `val`.  Small arrays: a brute force over the (query x value) matrix.  Large
    ones: per threshold the sorted list of the positions below it and a bisection; minima of chunks of CHUNK values
    combined with direct minima over the two ragged ends."""

    def __init__(self, val):
        self.val = np.ascontiguousarray(val, dtype=np.uint32)
        self.n = self.val.size
        self.small = self.n <= 1000
        self._hits = {}
        if not self.small:
            self.chunk_min = np.minimum.reduceat(self.val, np.arange(0, self.n, CHUNK))

    # -- range minimum
    def min(self, l, r):
        l, r = np.asarray(l, dtype=np.int64), np.asarray(r, dtype=np.int64)
        if self.small:
            out = np.full(l.size, NIL, dtype=np.uint32)
            if self.n:
                i = np.arange(self.n)
                inside = (i >= l[:, None]) & (i < r[:, None])
                out = np.where(inside, self.val[None, :], np.uint32(NIL)).min(axis=1).astype(np.uint32)
            return out
        r = np.maximum(l, r)  # (l > r: empty)
        cl, cr = (l + CHUNK - 1) // CHUNK, r // CHUNK  # whole chunks [cl, cr) when cl <= cr
        split = cl <= cr
        left_hi = np.where(split, cl * CHUNK, r)
        right_lo = np.where(split, cr * CHUNK, r)
        m = _pairs_reduce(self.val, l, left_hi)
        m = np.minimum(m, _pairs_reduce(self.chunk_min, cl, cr))
        return np.minimum(m, _pairs_reduce(self.val, right_lo, r))

    # -- first / last index below one threshold
    def _hit_list(self, x):
        if x not in self._hits:
            self._hits[x] = np.flatnonzero(self.val < np.uint32(x))
        return self._hits[x]

    def first_less(self, l, r, x):
        """x: one threshold for all ranges."""
        l, r = np.asarray(l, dtype=np.int64), np.asarray(r, dtype=np.int64)
        if self.small:
            return self.first_less_each(l, r, np.full(l.size, x, dtype=np.uint32))
        hits = np.concatenate([self._hit_list(x), [self.n + 1]])  # (a sentinel behind every range)
        h = hits[np.searchsorted(hits, l, side="left")]
        return np.where(h < r, h, NIL).astype(np.uint32)

    def last_less(self, l, r, x):
        l, r = np.asarray(l, dtype=np.int64), np.asarray(r, dtype=np.int64)
        if self.small:
            return self.last_less_each(l, r, np.full(l.size, x, dtype=np.uint32))
        hits = np.concatenate([[-1], self._hit_list(x)])  # (a sentinel in front of every range)
        h = hits[np.searchsorted(hits, r, side="left") - 1]
        return np.where((h >= l) & (h < r), h, NIL).astype(np.uint32)

    # -- a threshold of its own for every range (small arrays only: brute force, 32768 ranges at a time)
    def _each(self, l, r, x, first):
        assert self.small
        l, r, x = np.asarray(l, dtype=np.int64), np.asarray(r, dtype=np.int64), np.asarray(x, dtype=np.uint32)
        out = np.full(l.size, NIL, dtype=np.uint32)
        i = np.arange(self.n)
        for a in range(0, l.size if self.n else 0, 32768):
            s = slice(a, a + 32768)
            b = (i >= l[s, None]) & (i < r[s, None]) & (self.val[None, :] < x[s, None])
            at = b.argmax(axis=1) if first else self.n - 1 - b[:, ::-1].argmax(axis=1)
            out[s] = np.where(b.any(axis=1), at, NIL)
        return out

    def first_less_each(self, l, r, x):
        return self._each(l, r, x, True)

    def last_less_each(self, l, r, x):
        return self._each(l, r, x, False)

    # -- a threshold of its own for every range, large arrays: the answer is unique, so an answer that has the defining
    # property IS the answer.  got = NIL: nothing in [l, r) is below x; else l <= got < r, val[got] < x and nothing
    # in [l, got) (first) / in (got, r) (last) is below x.  Returns the indices of the ranges whose answer is wrong.
    def wrong_answers_each(self, kind, l, r, x, got):
        l, r, x = np.asarray(l, dtype=np.int64), np.asarray(r, dtype=np.int64), np.asarray(x, dtype=np.uint32)
        got = np.asarray(got, dtype=np.uint32)
        none = got == NIL
        g = np.where(none, 0, got).astype(np.int64)
        inside = ~none & (g >= l) & (g < r) & (g < self.n)
        hit = np.zeros(l.size, dtype=bool)
        hit[inside] = self.val[g[inside]] < x[inside]
        if kind == SEG_FIRST_LESS:
            rest = self.min(l, np.where(none, r, g))
        else:
            rest = self.min(np.where(none, l, g + 1), r)
        ok = (none | (inside & hit)) & ~(rest < x)
        return np.flatnonzero(~ok)

    def answers(self, q):
        """The expected word of every query of q, rows (kind, l, r, x).  Over a large array the first / last queries of q
        must share few thresholds (one hit list each)."""
        q = np.asarray(q, dtype=np.uint32).reshape(-1, 4)
        kind, l, r, x = q[:, 0], q[:, 1].astype(np.int64), q[:, 2].astype(np.int64), q[:, 3]
        want = np.zeros(q.shape[0], dtype=np.uint32)
        m = kind == SEG_MIN
        want[m] = self.min(l[m], r[m])
        for k, each, one in ((SEG_FIRST_LESS, self.first_less_each, self.first_less), (SEG_LAST_LESS, self.last_less_each, self.last_less)):
            sel = np.flatnonzero(kind == k)
            if self.small:
                want[sel] = each(l[sel], r[sel], x[sel])
                continue
            xs = np.unique(x[sel])
            assert xs.size <= 8, "per-range thresholds over a large array are checked (wrong_answers_each), not computed"
            for t in xs:
                s = sel[x[sel] == t]
                want[s] = one(l[s], r[s], int(t))
        return want


def ref_tree(val):
    """The tree seg_build leaves: nodes [0, 2 P), node 0 undefined (0 here), leaves at [P, 2 P) = the block minima,
    NIL where a block holds no value."""
    n, P = val.size, seg_P(val.size)
    padded = np.full(P * SEG_BLK, NIL, dtype=np.uint32)
    padded[:n] = val
    tree = np.zeros(2 * P, dtype=np.uint32)
    tree[P:] = padded.reshape(P, SEG_BLK).min(axis=1)
    w = P
    while w > 1:
        tree[w // 2:w] = tree[w:2 * w].reshape(w // 2, 2).min(axis=1)
        w //= 2
    return tree


# ============================================================================================== segment tree: ranges
def all_ranges(n):
    """Every 0 <= l <= r <= n, and some l > r."""
    l, r = np.triu_indices(n + 1)
    rng = rng_of("inverted", n)
    k = min(4 * n, 64)
    a, b = rng.integers(0, n + 1, k), rng.integers(0, n + 1, k)
    inv = a != b
    lo, hi = np.minimum(a, b)[inv], np.maximum(a, b)[inv]
    return np.concatenate([np.stack([l, r], axis=1), np.stack([hi, lo], axis=1)]).astype(np.int64)


def _sorted_pairs(a, b):
    return np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1)


def sampled_ranges(n, val=None, kind=None):
    """About 1400 ranges over [0, n] for a large n (2100 for the low kinds):
    - one for every pair (l mod 16, r mod 16);
    - both ends from {b - 1, b, b + 1} around multiples b of 16 * 2^j, for every j with 16 * 2^j <= n;
    - ranges that end at n, empty ranges, ranges with l > r, ranges whose length is log-uniform;
    - for the low kinds (val given): ranges placed around low values so that the only qualifying value of threshold
      LOW + 1 lies just outside the range, in an end block, or under the tree (probe_ranges)."""
    rng = rng_of("ranges", n)
    blocks = n // SEG_BLK
    out = []
    # every pair of offsets inside a block
    a, b = np.divmod(np.arange(SEG_BLK * SEG_BLK), SEG_BLK)
    bi = rng.integers(0, blocks - 1, (2, a.size))
    lo, hi = np.minimum(bi[0], bi[1]), np.maximum(bi[0], bi[1])
    hi = np.where((lo == hi) & (a > b), hi + 1, hi)  # (same block and l's offset behind r's: move r one block on)
    out.append(np.stack([lo * SEG_BLK + a, hi * SEG_BLK + b], axis=1))
    # ends around the edges of the tree's subtrees
    js = [j for j in range(32) if SEG_BLK << j <= n]
    per = max(520 // len(js), 8)
    for j in js:
        step = SEG_BLK << j
        e = rng.integers(0, n // step + 1, (2, per)) * step + rng.integers(-1, 2, (2, per))
        e = np.clip(e, 0, n)
        out.append(_sorted_pairs(e[0], e[1]))
    # ranges that end at n: from a block's edge, from anywhere
    l = np.concatenate([rng.integers(0, blocks + 1, 50) * SEG_BLK + rng.integers(-1, 2, 50), rng.integers(0, n + 1, 50)])
    out.append(np.stack([np.clip(l, 0, n), np.full(l.size, n)], axis=1))
    # empty, and l > r
    e = np.concatenate([[0, n], rng.integers(0, blocks + 1, 29) * SEG_BLK, rng.integers(0, n + 1, 29)])
    e = np.clip(e, 0, n)
    out.append(np.stack([e, e], axis=1))
    a, b = rng.integers(0, n + 1, 40), rng.integers(0, n + 1, 40)
    p = _sorted_pairs(a, b)
    out.append(p[p[:, 0] != p[:, 1]][:, ::-1])
    # log-uniform lengths
    length = np.exp(rng.random(400) * np.log(n)).astype(np.int64)
    start = (rng.random(400) * (n - length + 1)).astype(np.int64)
    out.append(np.stack([start, np.minimum(start + length, n)], axis=1))
    if kind in ("low0", "low15"):
        out.append(probe_ranges(val, n))
    return np.concatenate(out).astype(np.int64)


def probe_ranges(val, n):
    """Ranges around 100 draws of the low values p of a low kind, each at most reaching its neighbours q0 < p < q1:
    (p + 1, r) and (l, p): the low value sits at l - 1 / at r; l in p's block up to p with r blocks behind; l blocks in
    front and r blocks behind; l blocks in front with r in p's block behind p; and ranges that end (begin) up to three
    blocks in front of (behind) p and reach far the other way: subtrees that begin inside such a range hold p."""
    rng = rng_of("probes", n)
    lows = np.flatnonzero(val == LOW)
    pick = np.sort(rng.choice(np.arange(1, lows.size - 1), 100))  # (with repeats where the lows are fewer)
    out = []
    for k in pick:
        q0, p, q1 = int(lows[k - 1]), int(lows[k]), int(lows[k + 1])
        b0 = p // SEG_BLK * SEG_BLK
        far_l = lambda: int(rng.integers(q0 + 1, max(b0 - 2 * SEG_BLK, q0 + 1) + 1))  # noqa: E731
        far_r = lambda: int(rng.integers(min(b0 + 3 * SEG_BLK, q1), q1 + 1))  # noqa: E731
        out += [(p + 1, int(rng.integers(p + 1, q1 + 1))), (int(rng.integers(q0 + 1, p + 1)), p),
                (int(rng.integers(b0, p + 1)), far_r()), (far_l(), far_r()), (far_l(), int(rng.integers(p + 1, b0 + SEG_BLK + 1))),
                (far_l(), int(rng.integers(max(p - 3 * SEG_BLK, q0 + 1), p + 1))), (int(rng.integers(p + 1, min(p + 3 * SEG_BLK, q1) + 1)), far_r())]
    r = np.array(out, dtype=np.int64).reshape(-1, 2)
    r = np.clip(r, 0, n)
    return r[r[:, 0] <= r[:, 1]]


def seg_queries(kind, n, val, ref):
    """All queries of one (value kind, n) and a mask of those that carry a threshold of their own: the three kinds over
    all_ranges (n <= 213) or sampled_ranges, first / last at every threshold of seg_thresholds and at m + 1, m the
    range's own minimum (NIL + 1 wraps to 0); shuffled, so that neighbouring lanes hold unrelated queries."""
    ranges = all_ranges(n) if n in SEG_SMALL_N else sampled_ranges(n, val, kind)
    l, r = ranges[:, 0], ranges[:, 1]
    m1 = (ref.min(l, r) + np.uint32(1)).astype(np.int64)  # (uint32: wraps)
    rows = [np.stack([np.full(l.size, SEG_MIN), l, r, np.zeros(l.size, dtype=np.int64)], axis=1)]
    own = [np.zeros(l.size, dtype=bool)]
    for k in (SEG_FIRST_LESS, SEG_LAST_LESS):
        for x in seg_thresholds(kind, val):
            rows.append(np.stack([np.full(l.size, k), l, r, np.full(l.size, x)], axis=1))
            own.append(np.zeros(l.size, dtype=bool))
        rows.append(np.stack([np.full(l.size, k), l, r, m1], axis=1))
        own.append(np.ones(l.size, dtype=bool))
    q, own = np.concatenate(rows).astype(np.uint32), np.concatenate(own)
    order = rng_of("shuffle", n).permutation(q.shape[0])
    return q[order], own[order]


def seg_case(kind, n):
    """(values, reference, queries, mask of the queries with a threshold of their own) of one case."""
    val = seg_values(kind, n)
    ref = SegRef(val)
    return (val, ref) + seg_queries(kind, n, val, ref)


def where_answers_lie(val, ref, q):
    """Counts, over the first / last queries of q (few thresholds), of the situations a query can be wrong in alone --
    stated on the values and the reference's answers, in blocks of SEG_BLK values (bl = l's block, br = (r - 1)'s):
      miss_at_l-1 / miss_at_r    nothing in [l, r) is below x, but the value just outside is;
      left_block / middle / right_block   the answer lies in block bl / strictly between / in block br, of a range
                                 that spans at least three blocks;
      overhang_first             nothing in [l, r) is below x, yet the largest aligned group of 2^k blocks that holds block
                                 br - 1 and begins behind block bl + 1 reaches beyond br - 1 and holds a value below x;
      overhang_last              the mirror image: the largest aligned group that holds block bl + 1 and ends in front of
                                 block br - 1 begins at or in front of bl and holds a value below x."""
    q = np.asarray(q, dtype=np.int64)
    sel = (q[:, 0] != SEG_MIN) & (q[:, 1] < q[:, 2])
    kind, l, r, x = q[sel, 0], q[sel, 1], q[sel, 2], q[sel, 3]
    n = val.size
    v = np.concatenate([val, [NIL]]).astype(np.int64)
    want = ref.answers(q[sel]).astype(np.int64)
    none = want == NIL
    bl, br = l // SEG_BLK, (r - 1) // SEG_BLK
    c = {"miss_at_l-1": int((none & (l > 0) & (v[np.maximum(l - 1, 0)] < x)).sum()),
         "miss_at_r": int((none & (r < n) & (v[np.minimum(r, n)] < x)).sum())}
    wide = ~none & (br >= bl + 2)
    wb = want // SEG_BLK
    c["left_block"] = int((wide & (wb == bl)).sum())
    c["middle"] = int((wide & (wb > bl) & (wb < br)).sum())
    c["right_block"] = int((wide & (wb == br)).sum())
    # minima of the aligned groups, level by level (NIL behind the values)
    P = seg_P(n)
    padded = np.full(P * SEG_BLK, NIL, dtype=np.int64)
    padded[:n] = val
    level = padded.reshape(P, SEG_BLK).min(axis=1)
    f_min, f_end = np.full(l.size, NIL, dtype=np.int64), np.zeros(l.size, dtype=np.int64)
    l_min, l_start = np.full(l.size, NIL, dtype=np.int64), np.full(l.size, P, dtype=np.int64)
    k = 0
    while True:
        gf, gl = np.clip((br - 1) >> k, 0, level.size - 1), np.clip((bl + 1) >> k, 0, level.size - 1)
        ok = (gf << k) >= bl + 2  # (true for a prefix of the levels: the group only grows)
        f_min, f_end = np.where(ok, level[gf], f_min), np.where(ok, (gf + 1) << k, f_end)
        ok = ((gl + 1) << k) <= br - 1
        l_min, l_start = np.where(ok, level[gl], l_min), np.where(ok, gl << k, l_start)
        if level.size == 1:
            break
        level = level.reshape(-1, 2).min(axis=1)
        k += 1
    three = br >= bl + 3  # (two blocks or more strictly between the end blocks)
    c["overhang_first"] = int((none & three & (kind == SEG_FIRST_LESS) & (f_end > br) & (f_min < x)).sum())
    c["overhang_last"] = int((none & three & (kind == SEG_LAST_LESS) & (l_start <= bl) & (l_min < x)).sum())
    return c


# ============================================================================================== bit-rank directory
BITRANK_N = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 131007, 131008, 131071, 131072, 131073, (1 << 20) + 77]
BITRANK_ONE_HOT = [0, 1, 3, 4, 15, 16, 31, 32, 63, 64, 255, 256]
BITRANK_ALL_POSITIONS_UP_TO = 1025


def bitrank_patterns(n):
    return ["zero", "all", "half", "percent"] + [f"one_hot_{p}" for p in BITRANK_ONE_HOT if p < n]


def bitrank_flags(pattern, n):
    rng = rng_of("br_" + pattern, n)
    f = np.zeros(n, dtype=np.uint8)
    if pattern == "all":
        f[:] = 1
    elif pattern == "half":
        f = rng.integers(0, 2, n).astype(np.uint8)
    elif pattern == "percent":
        f = (rng.random(n) < 0.01).astype(np.uint8)
    elif pattern.startswith("one_hot_"):
        f[int(pattern[8:])] = 1
    elif pattern != "zero":
        raise ValueError(pattern)
    return f


def bitrank_positions(n):
    """Every x in [0, n] up to n = 1025; beyond: about 10^4 of them -- 0, n - 1, n, both sides of record edges, random ones."""
    if n <= BITRANK_ALL_POSITIONS_UP_TO:
        return np.arange(n + 1, dtype=np.uint32)
    rng = rng_of("br_pos", n)
    edges = rng.integers(0, n // BR_FLAGS + 1, 1500) * BR_FLAGS
    x = np.concatenate([[0, 1, n - 1, n, n // BR_FLAGS * BR_FLAGS], edges - 1, edges, edges + 1, edges + 31, edges + 32, rng.integers(0, n + 1, 2500)])
    return np.clip(x, 0, n).astype(np.uint32)


def ref_bitrank_records(flags):
    """The n // 64 + 2 records (bits 0..31, bits 32..63, set flags in front, 0); the last one closes the array."""
    n = flags.size
    n_rec = n // BR_FLAGS + 1
    bits = np.zeros(n_rec * BR_FLAGS, dtype=np.uint8)
    bits[:n] = flags != 0
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(n_rec, 2)
    per = bits.reshape(n_rec, BR_FLAGS).sum(axis=1, dtype=np.uint64)
    rec = np.zeros((n_rec + 1, 4), dtype=np.uint32)
    rec[:n_rec, :2] = words
    rec[1:, 2] = np.cumsum(per).astype(np.uint32)
    return rec


def ref_rank(flags, x):
    """Set flags in front of each position of x (x <= n)."""
    return np.concatenate([[0], np.cumsum(flags != 0, dtype=np.uint64)]).astype(np.uint32)[x]


# ============================================================================================== ordered append
APPEND_N = [1, 4, 1023, 1024, 1025, 16383, 16384, 16385, 5 * 16384 + 123]
APPEND_PATTERNS = ["none", "all", "half", "sparse", "first", "last", "one_wave", "one_round"]


def append_flags(pattern, n):
    """Byte flags of one of APPEND_PATTERNS.  one_wave / one_round: set flags (half of them) only inside the 256 positions
    one wave holds in one round / the 1024 positions of one round of one workgroup, chosen among those that begin below n."""
    rng = rng_of("ap_" + pattern, n)
    f = np.zeros(n, dtype=np.uint8)
    if pattern == "all":
        f[:] = 1
    elif pattern == "half":
        f = rng.integers(0, 2, n).astype(np.uint8)
    elif pattern == "sparse":
        f = (rng.random(n) < 1e-3).astype(np.uint8)
    elif pattern == "first":
        f[0] = 1
    elif pattern == "last":
        f[n - 1] = 1
    elif pattern in ("one_wave", "one_round"):
        width = 4 * 64 if pattern == "one_wave" else 4 * LIST_TPB
        a = int(rng.integers(0, (n + width - 1) // width)) * width
        f[a:a + width] = rng.integers(0, 2, f[a:a + width].size)
        f[min(a + width, n) - 1] = 1  # (never empty)
    elif pattern != "none":
        raise ValueError(pattern)
    return f
