"""The look-up structures one layer above the primitives, each alone against numpy; every comparison is exact.

The hooks (povu_hip_debug_segtree, _bitrank, _append) include the real headers and call the real functions; scratch and
unwritten outputs hold a non-zero byte and every device output lies between guard bands -- a structure that writes outside
its output raises GuardBandError with its name.  Inputs and references come from tests/lookups_cases.py, whose conditions
tests/test_lookups_inputs.py checks without a GPU.

    structure                                      test function
    ---------------------------------------------  ------------------------------------------------------------
    seg_build (k_seg_bottom, k_seg_top)            test_segment_tree (the built tree, node for node)
    seg_min, seg_first_less, seg_last_less         test_segment_tree (every range up to 213 values, about 2 * 10^4
                                                   queries a case beyond), test_segment_tree_refuses_ranges_beyond_n
    bitrank_store_wave, bitrank_build              test_bitrank (the records and the closing record)
    bitrank, bitrank_test                          test_bitrank
    append_in_order                                test_append
    all three hooks, twice, mixed sizes            test_lookup_hooks_in_a_mixed_sequence

(cseg_first_less's exit `node == 0` IS taken from seg_first_less, and is needed: the walk moves right through the leaf
bl + 1 and then the largest aligned subtrees that begin where the last one ended; when one of them begins in front of
block br, reaches the tree's right edge and holds nothing below x, the climb from it passes the root.  With 16 leaves
that is every range with bl + 1 < 8 < br asked at a threshold nothing is below -- threshold 0 at 213 values asks them all.)"""
import numpy as np
import pytest

import lookups_cases as LC
from povu_amd import HipDecomposer

pytestmark = pytest.mark.gpu

NIL = LC.NIL


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def first_difference(got, want, q):
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return None
    i = int(bad[0])
    return f"{bad.size} of {got.size} differ; first: query (kind, l, r, x) = {q[i].tolist()} gave {int(got[i])}, expected {int(want[i])}"


def check_segment_tree(hip, kind, n):
    val, ref, q, own = LC.seg_case(kind, n)
    got, tree, P = hip.debug_segtree(val, q, want_tree=True)
    # the tree: leaves = block minima, NIL behind the values; every node the minimum of its two children
    want_tree = LC.ref_tree(val)
    assert P == LC.seg_P(n) and tree.size == 2 * P
    assert np.array_equal(tree[1:], want_tree[1:]), (kind, n, np.flatnonzero(tree[1:] != want_tree[1:])[:8] + 1)
    # the queries whose thresholds are few: computed
    want = ref.answers(q[~own])
    assert first_difference(got[~own], want, q[~own]) is None, (kind, n, first_difference(got[~own], want, q[~own]))
    # the queries at m + 1, m the range's own minimum: computed by brute force at small sizes; beyond, the one answer
    # that has the defining property (SegRef.wrong_answers_each)
    qo, go = q[own], got[own]
    if ref.small:
        want = ref.answers(qo)
        assert first_difference(go, want, qo) is None, (kind, n, first_difference(go, want, qo))
    else:
        for k in (LC.SEG_FIRST_LESS, LC.SEG_LAST_LESS):
            s = qo[:, 0] == k
            bad = ref.wrong_answers_each(k, qo[s, 1], qo[s, 2], qo[s, 3], go[s])
            assert bad.size == 0, (kind, n, bad.size, qo[s][bad[0]].tolist(), int(go[s][bad[0]]))


# ---- segment tree
@pytest.mark.parametrize("n", LC.SEG_N)
@pytest.mark.parametrize("kind", LC.SEG_VALUES)
def test_segment_tree(hip, kind, n):
    """The built tree and all three queries: every 0 <= l <= r <= n (and some l > r) up to 213 values, about 2 * 10^4 queries
    beyond -- every pair of offsets inside a block, ends around the edges of the subtrees of every height, ranges up to n,
    empty ones -- at the thresholds 0, 1, a value that occurs, that value + 1, NIL and the range's own minimum + 1."""
    check_segment_tree(hip, kind, n)


def test_segment_tree_refuses_ranges_beyond_n(hip):
    """No call site asks beyond the values: return code 1, before anything runs."""
    val = LC.seg_values("small", 33)
    for row in ([LC.SEG_MIN, 0, 34, 0], [LC.SEG_FIRST_LESS, 40, 34, 1], [3, 0, 1, 0]):
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            hip.debug_segtree(val, np.array([row], dtype=np.uint32))
    assert hip.debug_segtree(val, np.array([[LC.SEG_LAST_LESS, 40, 33, NIL]], dtype=np.uint32)).tolist() == [NIL]  # (l > r)


# ---- bit-rank directory
def check_bitrank(hip, flags, what):
    n = flags.size
    x = LC.bitrank_positions(n)
    rank, test, rec = hip.debug_bitrank(flags, x)
    want = LC.ref_bitrank_records(flags)
    assert rec.shape == (n // LC.BR_FLAGS + 2, 4)
    assert np.array_equal(rec, want), (what, np.flatnonzero((rec != want).any(axis=1))[:8])
    assert rec[-1].tolist() == [0, 0, int(np.count_nonzero(flags)), 0], what  # the closing record
    assert np.array_equal(rank, LC.ref_rank(flags, x)), what
    assert x[-1] == n or n in x
    assert int(rank[x == n][0]) == int(np.count_nonzero(flags)), what  # rank(n)
    inside = x < n
    assert np.array_equal(test[inside], (flags[x[inside]] != 0).astype(np.uint32)), what


@pytest.mark.parametrize("n", LC.BITRANK_N)
def test_bitrank(hip, n):
    """Records (bits, ranks, closing record), bitrank(x) and bitrank_test(x): all x up to 1025 flags, about 10^4 of them
    beyond, rank(n) always; no flag, all, half, one in a hundred, and single flags on every lane of the interleave."""
    for pattern in LC.bitrank_patterns(n):
        check_bitrank(hip, LC.bitrank_flags(pattern, n), (pattern, n))


# ---- ordered append
def check_append(hip, flags, what):
    n = flags.size
    want = np.flatnonzero(flags).astype(np.uint32)
    got, cnt = hip.debug_append(flags)
    assert cnt == want.size and got.size == cnt, what
    assert np.array_equal(np.sort(got), want), what  # nothing lost, nothing twice
    # the positions of each workgroup's span: one contiguous stretch of the list, ascending
    group = got // LC.LIST_SPAN
    starts = np.flatnonzero(np.concatenate([[True], group[1:] != group[:-1]])) if cnt else np.zeros(0, dtype=np.int64)
    assert np.unique(group[starts]).size == starts.size, what  # (no workgroup's stretch is split)
    assert (np.diff(got.astype(np.int64))[group[1:] == group[:-1]] > 0).all(), what
    if n <= LC.LIST_SPAN:
        assert np.array_equal(got, want), what


@pytest.mark.parametrize("n", LC.APPEND_N)
def test_append(hip, n):
    """The list's length, its content, and its order inside every workgroup's stretch; the order of the stretches is up
    to the atomics."""
    for pattern in LC.APPEND_PATTERNS:
        check_append(hip, LC.append_flags(pattern, n), (pattern, n))


# ---- all three hooks twice on one context, other sizes in between
def test_lookup_hooks_in_a_mixed_sequence(hip):
    for n in (100003, 17, 4097, 100003, 1, 16385):
        check_segment_tree(hip, "small", n)
        check_bitrank(hip, LC.bitrank_flags("half", n), ("half", n))
        check_append(hip, LC.append_flags("half", n), ("half", n))
        check_segment_tree(hip, "low15", n)
