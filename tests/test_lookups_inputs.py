"""The inputs of tests/test_gpu_lookups.py have the properties they are there for (tests/lookups_cases.py), the
references agree with a plain loop, and the constants stated there are the ones of the sources.  numpy alone, no GPU."""
import os
import re

import numpy as np
import pytest

import lookups_cases as LC
import primitives_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "povu_amd", "csrc", "hip")
NIL = LC.NIL


def src(name):
    return open(os.path.join(HIP, name)).read()


def test_constants_mirror_the_sources():
    seg, par, com = src("segtree.hpp"), src("par_kernels.hpp"), src("common.hpp")
    assert re.search(r"static constexpr uint32_t BLK = (\d+);", par).group(1) == str(LC.SEG_BLK)
    assert "SEG_BLK = SegTree::BLK" in seg
    assert re.search(r"#define SEG_TPB (\d+)", seg).group(1) == str(LC.SEG_TPB)
    assert f"__launch_bounds__({LC.SEG_TOP_LANES}) k_seg_top" in seg and f"dim3(1), dim3({LC.SEG_TOP_LANES}), 0, s, st.P / SEG_TPB" in seg
    assert "if (st.P > SEG_TPB)" in seg  # (seg_top_nodes)
    it, tpb = re.search(r"LIST_ITER = (\d+), LIST_TPB = (\d+), LIST_SPAN = LIST_TPB \* 4 \* LIST_ITER;", com).groups()
    assert (int(it), int(tpb)) == (LC.LIST_ITER, LC.LIST_TPB) and LC.LIST_SPAN == 16384
    assert "rec[x >> 6]" in com and LC.BR_FLAGS == 1 << 6
    # a wave stores four records of 64 flags: lanes 0..3, sixteen lanes' four flags each
    assert "if (lane < 4 && in_range)" in com and "const unsigned sh = 16u * lane;" in com and LC.BR_WAVE == 4 * LC.BR_FLAGS == 64 * 4
    head = open(os.path.join(ROOT, "include", "povu_hip.h")).read()
    kinds = {k: int(v) for k, v in re.findall(r"#define POVU_HIP_SEG_(MIN|FIRST_LESS|LAST_LESS) (\d)", head)}
    assert kinds == {"MIN": LC.SEG_MIN, "FIRST_LESS": LC.SEG_FIRST_LESS, "LAST_LESS": LC.SEG_LAST_LESS}
    assert PC.SC_TILE == 2048  # (bit-rank sizes below)


# ---------------------------------------------------------------------------------------------- segment tree
def test_segment_tree_sizes_take_every_build_path():
    P = {n: LC.seg_P(n) for n in LC.SEG_N}
    assert [P[n] for n in (0, 1, 15, 16, 17, 33)] == [1, 1, 1, 1, 2, 4]
    assert {n % LC.SEG_BLK == 0 for n in LC.SEG_N if n} == {True, False}  # the 16-byte path alone, and with a tail
    assert -(-213 // LC.SEG_BLK) == 14 and P[213] == 16  # blocks that are no power of two
    # one workgroup and no top kernel up to 4096 values; the smallest top from 4097
    assert P[4096] == LC.SEG_TPB and LC.seg_top_nodes(4096) == 0 and LC.seg_top_nodes(4097) == 2 and LC.seg_top_nodes(8193) == 4
    wgs = P[100003] // LC.SEG_TPB
    assert wgs == 32 and sum(w * LC.SEG_TPB * LC.SEG_BLK >= 100003 for w in range(wgs)) >= 3  # workgroups of padding only
    # k_seg_top's widest level has top_nodes / 2 nodes: one round of its lanes at 2^23 values, two from 2^23 + 1
    assert LC.seg_top_nodes(1 << 23) // 2 == LC.SEG_TOP_LANES and LC.seg_top_nodes((1 << 23) + 1) // 2 == 2 * LC.SEG_TOP_LANES
    assert max(LC.SEG_N) == (1 << 23) + 1


@pytest.mark.parametrize("n", [213, 4097])
def test_segment_tree_values(n):
    v = {k: LC.seg_values(k, n) for k in LC.SEG_VALUES}
    assert all(a.dtype == np.uint32 and a.size == n for a in v.values())
    assert (v["random"] == NIL).any() and int(v["random"][v["random"] != NIL].max()) > 1 << 31
    assert set(np.unique(v["small"]).tolist()) == {0, 1, 2, 3}
    assert set(np.unique(v["flags"]).tolist()) == {0, 1}
    assert (np.diff(v["ascending"].astype(np.int64)) > 0).all() and (np.diff(v["descending"].astype(np.int64)) < 0).all()
    assert 0.9 < (v["sparse"] == NIL).mean() < 1 and (v["sparse"] != NIL).any()
    for kind, off in (("low0", 0), ("low15", LC.SEG_BLK - 1)):
        at = np.flatnonzero(v[kind] == LC.LOW)
        assert at.size >= 3 and (at % LC.SEG_BLK == off).all() and np.unique(at // LC.SEG_BLK).size == at.size
        assert int(np.delete(v[kind], at).min()) >= LC.HIGH
        assert LC.seg_thresholds(kind, v[kind]) == [0, 1, LC.LOW, LC.LOW + 1, NIL]
    for kind in LC.SEG_VALUES:
        t = LC.seg_thresholds(kind, v[kind])
        occurring = [x for x in t if (v[kind] == x).any() and x + 1 in t]
        assert t[0] == 0 and 1 in t and t[-1] == NIL and occurring, (kind, t)


def test_segment_tree_values_of_edge_sizes():
    for n in (0, 1, 15, 16, 17, 33):
        for kind in LC.SEG_VALUES:
            v = LC.seg_values(kind, n)
            assert v.size == n and v.dtype == np.uint32
            assert {0, 1, NIL} <= set(LC.seg_thresholds(kind, v))


def spans_and_offsets(q):
    live = q[q[:, 1] < q[:, 2]].astype(np.int64)
    span = (live[:, 2] - 1) // LC.SEG_BLK - live[:, 1] // LC.SEG_BLK
    return set(np.minimum(span, 3).tolist()), {(int(a), int(b)) for a, b in zip(live[:, 1] % LC.SEG_BLK, live[:, 2] % LC.SEG_BLK)}


EVERY_OFFSET_PAIR = {(a, b) for a in range(LC.SEG_BLK) for b in range(LC.SEG_BLK)}
SITUATIONS = ["miss_at_l-1", "miss_at_r", "left_block", "middle", "right_block", "overhang_first", "overhang_last"]


@pytest.mark.parametrize("kind", ["low0", "low15", "small", "sparse"])
def test_small_query_sets_ask_everything(kind):
    n = 213
    val, ref, q, own = LC.seg_case(kind, n)
    ranges = {(int(a), int(b)) for a, b in q[q[:, 0] == LC.SEG_MIN][:, 1:3]}
    assert {(l, r) for l in range(n + 1) for r in range(l, n + 1)} <= ranges and any(l > r for l, r in ranges)
    t = LC.seg_thresholds(kind, val)
    for k in (LC.SEG_FIRST_LESS, LC.SEG_LAST_LESS):
        for x in t:
            assert int(((q[:, 0] == k) & (q[:, 3] == x) & ~own).sum()) == len(ranges)
        assert int(((q[:, 0] == k) & own).sum()) == len(ranges)
    spans, offsets = spans_and_offsets(q)
    assert spans == {0, 1, 2, 3} and offsets == EVERY_OFFSET_PAIR
    # the thresholds of their own are the ranges' minima + 1, NIL + 1 = 0 among them where a range holds NIL alone
    o = q[own]
    assert np.array_equal(o[:, 3], ref.min(o[:, 1], o[:, 2]) + np.uint32(1))
    assert kind != "sparse" or ((o[:, 3] == 0) & (o[:, 1] < o[:, 2])).any()
    if kind.startswith("low"):
        c = LC.where_answers_lie(val, ref, q[~own])
        assert all(c[s] >= 10 for s in SITUATIONS), c


@pytest.mark.parametrize("n", [4097, 100003])
@pytest.mark.parametrize("kind", ["low0", "low15", "random"])
def test_large_query_sets(kind, n):
    val, ref, q, own = LC.seg_case(kind, n)
    assert 15000 <= q.shape[0] <= 35000 and q.dtype == np.uint32 and int(q[:, 2].max()) == n
    m = q[q[:, 0] == LC.SEG_MIN]
    l, r = m[:, 1].astype(np.int64), m[:, 2].astype(np.int64)
    spans, offsets = spans_and_offsets(q)
    assert spans == {0, 1, 2, 3} and offsets == EVERY_OFFSET_PAIR
    assert ((r == n) & (l < r)).sum() >= 100 and (l == r).sum() >= 50 and (l > r).sum() >= 30
    length = (r - l)[r > l]
    assert all(((length >= 10 ** e) & (length < 10 ** (e + 1))).sum() >= 30 for e in range(int(np.log10(n))))
    # ends one in front of, on and one behind the edges of the subtrees of every height
    j = 0
    while LC.SEG_BLK << j <= n:
        step = LC.SEG_BLK << j
        for d in (-1, 0, 1):
            for e in (l, r):
                on = ((e - d) % step == 0) & (e - d >= 0)
                assert (on & (((e - d) // step) % 2 == 1)).any() or n < 3 * step, (j, d)  # (an odd multiple: of no larger step)
                assert on.any(), (j, d)
        j += 1
    assert j == int(np.log2(n // LC.SEG_BLK)) + 1
    # every range at every threshold, by all three queries
    for k in (LC.SEG_FIRST_LESS, LC.SEG_LAST_LESS):
        for x in LC.seg_thresholds(kind, val):
            assert int(((q[:, 0] == k) & (q[:, 3] == x) & ~own).sum()) == m.shape[0]
        assert int(((q[:, 0] == k) & own).sum()) == m.shape[0]
    o = q[own]
    assert np.array_equal(o[:, 3], ref.min(o[:, 1], o[:, 2]) + np.uint32(1))
    # neighbouring lanes hold unrelated queries
    assert (np.diff(q[:, 0].astype(np.int64)) != 0).mean() > 0.4
    if kind.startswith("low"):
        c = LC.where_answers_lie(val, ref, q[~own])
        assert all(c[s] >= 10 for s in SITUATIONS), c


def test_largest_size_reaches_every_height():
    n = (1 << 23) + 1
    r = LC.sampled_ranges(n)
    assert 1000 <= r.shape[0] <= 2500 and int(r.max()) == n and int(r.min()) == 0
    top = LC.SEG_BLK << 19
    assert top <= n < 2 * top and any(((r - d) % top == 0).any() for d in (-1, 0, 1))


def loop_answers(val, q):
    out = []
    for kind, l, r, x in q.tolist():
        hit = [i for i in range(l, r) if val[i] < x]
        if kind == LC.SEG_MIN:
            out.append(min([int(v) for v in val[l:r]], default=NIL) if l < r else NIL)
        else:
            out.append((hit[0] if kind == LC.SEG_FIRST_LESS else hit[-1]) if hit else NIL)
    return np.array(out, dtype=np.uint32)


@pytest.mark.parametrize("kind", ["small", "sparse", "low15"])
def test_references_agree_with_a_loop(kind):
    """Both forms of the reference -- the matrix at 213 values, hit lists and chunked minima at 3001 -- against a plain
    loop; and the check of answers at per-range thresholds accepts the right answer and nothing else."""
    for n in (213, 3001):
        val = LC.seg_values(kind, n)
        ref = LC.SegRef(val)
        assert ref.small == (n == 213)
        rng = PC.rng_of("loop", n)
        a, b = rng.integers(0, n + 1, 300), rng.integers(0, n + 1, 300)
        a[:20], b[:20] = np.minimum(rng.integers(0, 40, 20) * 50, n), np.minimum(rng.integers(0, 61, 20) * 50, n)  # (ends on chunk edges, l > r among them)
        t = LC.seg_thresholds(kind, val)
        q = np.stack([rng.integers(0, 3, 300), a, b, np.array(t)[rng.integers(0, len(t), 300)]], axis=1).astype(np.uint32)
        want = loop_answers(val, q)
        assert np.array_equal(ref.answers(q), want)
        if not ref.small:
            m1 = ref.min(a, b) + np.uint32(1)
            for k in (LC.SEG_FIRST_LESS, LC.SEG_LAST_LESS):
                qq = np.stack([np.full(300, k), a, b, m1], axis=1).astype(np.uint32)
                right = loop_answers(val, qq)
                assert LC.SegRef(val).wrong_answers_each(k, a, b, m1, right).size == 0
                found = np.flatnonzero(right != NIL)
                assert found.size >= 100
                for wrong in (right + np.uint32(1), right - np.uint32(1), np.full(300, NIL, dtype=np.uint32)):
                    # (a neighbour of the answer is never the answer as well; where there is one, "none" is wrong)
                    bad = ref.wrong_answers_each(k, a, b, m1, np.where(right != NIL, wrong, right))
                    assert np.array_equal(bad, found)
                none = np.flatnonzero((right == NIL) & (a < b))
                bad = ref.wrong_answers_each(k, a, b, m1, np.where(right == NIL, a.astype(np.uint32), right))
                assert set(none.tolist()) <= set(bad.tolist())


def test_reference_tree():
    val = np.array([9, 8, 7] + [50] * 13 + [3] + [60] * 20, dtype=np.uint32)  # 37 values: blocks {7, 3, 60}, P = 4
    t = LC.ref_tree(val)
    assert t.tolist()[1:] == [3, 3, 60, 7, 3, 60, NIL]
    assert LC.ref_tree(np.zeros(0, dtype=np.uint32)).tolist()[1:] == [NIL]
    assert LC.ref_tree(np.full(16, 4, dtype=np.uint32)).tolist()[1:] == [4]


# ---------------------------------------------------------------------------------------------- bit-rank directory
def test_bitrank_sizes_and_patterns():
    N = set(LC.BITRANK_N)
    for edge in (LC.BR_FLAGS, LC.BR_WAVE, 4 * LC.BR_WAVE):  # a record, a wave's four records, a workgroup's sixteen
        assert {edge - 1, edge, edge + 1} <= N
    assert any(n % LC.BR_FLAGS == 0 for n in N) and any(n % LC.BR_FLAGS for n in N)  # rank(n) reads a record of no flags
    scanned = {n: n // LC.BR_FLAGS + 2 for n in N}  # counts bitrank_build scans in place: the records and the closing one
    assert PC.SC_TILE in scanned.values() and PC.SC_TILE + 1 in scanned.values()  # one scan tile, and two
    assert scanned[131072] == 2050 and max(N) > 4 * PC.SC_TILE * LC.BR_FLAGS
    assert len(LC.BITRANK_ONE_HOT) == 12
    for n in (1, 65, 257, 131073):
        pats = LC.bitrank_patterns(n)
        assert pats[:4] == ["zero", "all", "half", "percent"]
        assert [int(p[8:]) for p in pats[4:]] == [p for p in LC.BITRANK_ONE_HOT if p < n]
        for p in pats:
            f = LC.bitrank_flags(p, n)
            assert f.dtype == np.uint8 and f.size == n
            if p.startswith("one_hot_"):
                assert np.flatnonzero(f).tolist() == [int(p[8:])]
        assert not LC.bitrank_flags("zero", n).any() and LC.bitrank_flags("all", n).all()
    f = LC.bitrank_flags("percent", 131073)
    assert 0.005 < f.mean() < 0.02 and 0.4 < LC.bitrank_flags("half", 131073).mean() < 0.6
    # one-hot positions on every nibble lane of the interleave: offsets 0..3 inside a lane's four flags, and the lanes
    # that start a 32-bit word, a record and a wave
    assert {p % 4 for p in LC.BITRANK_ONE_HOT} == {0, 1, 3} and {31, 32, 63, 64, 255, 256} <= set(LC.BITRANK_ONE_HOT)


def test_bitrank_positions():
    for n in LC.BITRANK_N:
        x = LC.bitrank_positions(n)
        assert x.dtype == np.uint32 and int(x.max()) == n and int(x.min()) == 0
        if n <= 1025:
            assert np.array_equal(x, np.arange(n + 1))
        else:
            assert 8000 <= x.size <= 12000 and n - 1 in x
            assert {0, 1, 31, 32, 63} <= set((x % LC.BR_FLAGS).tolist())


def test_bitrank_reference():
    f = np.zeros(130, dtype=np.uint8)
    f[[0, 31, 32, 63, 64, 129]] = [1, 2, 1, 0x80, 1, 1]
    rec = LC.ref_bitrank_records(f)
    assert rec.tolist() == [[0x80000001, 0x80000001, 0, 0], [1, 0, 4, 0], [2, 0, 5, 0], [0, 0, 6, 0]]
    assert LC.ref_rank(f, np.array([0, 1, 32, 64, 65, 129, 130])).tolist() == [0, 1, 2, 4, 5, 5, 6]
    assert LC.ref_bitrank_records(np.ones(64, dtype=np.uint8)).tolist() == [[NIL, NIL, 0, 0], [0, 0, 64, 0], [0, 0, 64, 0]]


# ---------------------------------------------------------------------------------------------- ordered append
def test_append_sizes_and_patterns():
    N = set(LC.APPEND_N)
    round_ = 4 * LC.LIST_TPB
    assert {round_ - 1, round_, round_ + 1, LC.LIST_SPAN - 1, LC.LIST_SPAN, LC.LIST_SPAN + 1} <= N and {1, 4} <= N
    assert any(n > 5 * LC.LIST_SPAN and n % LC.LIST_SPAN for n in N)  # several workgroups, the last one partial
    for n in LC.APPEND_N:
        f = {p: LC.append_flags(p, n) for p in LC.APPEND_PATTERNS}
        assert all(v.dtype == np.uint8 and v.size == n for v in f.values())
        assert not f["none"].any() and f["all"].all()
        assert np.flatnonzero(f["first"]).tolist() == [0] and np.flatnonzero(f["last"]).tolist() == [n - 1]
        for p, width in (("one_wave", 256), ("one_round", round_)):
            at = np.flatnonzero(f[p])
            assert at.size and at[0] // width == at[-1] // width
            assert n < 1024 or at.size > width // 4
        if n > 16384:
            assert 0.4 < f["half"].mean() < 0.6 and 0 < f["sparse"].sum() < n // 300
