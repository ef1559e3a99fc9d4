"""GPU tests of the third bracket count per tree vertex as bytes: `incnt` (brackets that END at a tree vertex) is kept one
byte each, like `ordcnt` and `srccnt`, whenever no side of the graph has more than 253 links.  The byte form does not count
the brackets that end at a root (nothing reads a root's count), and a byte that would pass 255 -- capping brackets on top of
the ordinary back edges that end at one vertex -- makes the pass run its tree and class stages again with words.  Every
forest is compared with the CPU oracle's, every case runs as built and with the word form forced, and the form that ran is
asserted; the properties the shapes are built for are read off the oracle's bracket lists first."""
import numpy as np
import pytest

import oracle_lib as O
import primitives_cases as PC
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_ALL_VERTEX_CLASSES, F_CHECK_LAMINAR, F_NO_STAGE_TIMES
from test_gpu_narrow_counts import comb, fan_in, max_side_links
from test_gpu_stack_lookups import concat, sized_components
from test_oracle import dump_component

pytestmark = pytest.mark.gpu

FLAGS = (0, F_NO_STAGE_TIMES, F_CHECK_LAMINAR, F_ALL_VERTEX_CLASSES)
NIL = 0xFFFFFFFF
ALL_BYTES, ALL_WORDS = (True, True, True), (False, False, False)


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def ladder(k, more=0, into_r=0):
    """A chain 0 > 1 > ... > k+2 closed by k+2 > 0, and for i in 1..k a segment x_i with i > x_i > 1: the k links x_i > 1 are
    ordinary back edges that end at the l side of segment 1, and every segment i in 1..k is a branching vertex whose second
    reach is that side, so k capping brackets end there too: 2 k brackets at one tree vertex that is no root, on a side with
    k + 1 links.  `more` adds ordinary back edges into the same side (from the far end of the chain), `into_r` links into
    the r side of segment 1: back edges that end at the NEXT tree vertex."""
    n = k + 3
    src, dst, m = list(range(n - 1)), list(range(1, n)), n
    for i in range(1, k + 1):
        src += [i, m]
        dst += [m, 1]
        m += 1
    src.append(n - 1)
    dst.append(0)
    for j in range(more):
        src.append(n - 2 - j)
        dst.append(1)
    e = len(src)
    v1 = np.array(src + [n - 2 - j for j in range(into_r)], dtype=np.uint32)
    v2 = np.array(dst + [1] * into_r, dtype=np.uint32)
    s1 = np.full(e + into_r, W.R, dtype=np.uint8)
    s2 = np.array([W.L] * e + [W.R] * into_r, dtype=np.uint8)
    return W._mk(np.arange(1, m + 1), v1, s1, v2, s2)


def in_counts(g, c=0):
    """Brackets of every kind that end at each tree vertex of component c (the oracle's lists), and its parents."""
    d = dump_component(g, c)
    return np.bincount(d["be_tgt"], minlength=len(d["par"])), d["par"], d


def run_forms(hip, monkeypatch, g, want, forms, repeats=0, flags=FLAGS):
    """The forests of `g` as built (expecting `forms` = which of ordcnt / srccnt / incnt are bytes, and `repeats` passes that
    ran again with words), with incnt alone forced wide and with everything forced wide."""
    hip.upload(g)
    for env, expect in ((None, forms), ("3", (forms[0], forms[1], False)), ("1", ALL_WORDS)):
        if env is None:
            monkeypatch.delenv("POVU_HIP_WIDE_COUNTS", raising=False)
        else:
            monkeypatch.setenv("POVU_HIP_WIDE_COUNTS", env)
        for fl in flags:
            before = hip.wide_repeat_count()
            assert hip.decompose(flags=fl).texts() == want, (env, fl)
            rep = repeats if env is None else 0
            assert hip.wide_repeat_count() - before == rep, (env, fl)
            assert hip.last_narrow_forms() == (ALL_WORDS if rep else expect), (env, fl)
            assert hip.seq_redo_count() == 0
    monkeypatch.delenv("POVU_HIP_WIDE_COUNTS")


@pytest.mark.parametrize("d", [1, 2, 252, 253])
@pytest.mark.parametrize("shape", [fan_in, comb])
def test_in_counts_at_the_byte_edge(hip, monkeypatch, shape, d):
    """fan_in(d) / comb(d): 253 links on the fat side (d = 252) is the last graph the byte form takes; with 254 the word
    form must be reported."""
    g = shape(d)
    assert max_side_links(g) == d + 1
    if shape is comb:
        cnt, par, _ = in_counts(g)
        assert cnt[par != NIL].max() >= d
    run_forms(hip, monkeypatch, g, O.decompose(g), ALL_BYTES if d <= 252 else ALL_WORDS)


@pytest.mark.parametrize("shift", range(4))
def test_a_full_byte_beside_its_neighbours(hip, monkeypatch, shift):
    """No carry between the bytes of one word: a tree vertex with 255 brackets ending at it -- the most a byte holds, 128
    ordinary and 127 capping ones -- directly in front of one with a single bracket and behind one with none, the fat byte in
    every position of its aligned word (components of one segment in front shift T-space by three slots each)."""
    fat = ladder(127, more=1, into_r=1)
    cnt, par, _ = in_counts(fat)
    assert par[2] != NIL and cnt[1:5].tolist() == [0, 255, 1, 0] and cnt[par != NIL].max() == 255
    assert max_side_links(fat) + 2 <= 255
    g = concat([sized_components([1] * shift), fat]) if shift else fat
    # T-space: component c owns the slots from 2 * (segments before it) + c on
    assert (3 * shift + 2) % 4 == [2, 1, 0, 3][shift]
    run_forms(hip, monkeypatch, g, O.decompose(g), ALL_BYTES)


def tips_on_a_backbone(n_tips):
    """A backbone 0 > 1 > ... > n_tips + 1 with a dead-end segment hanging off every inner segment: n_tips + 2 tips in all,
    each sends a back edge to the dummy root."""
    n = n_tips + 2
    src = list(range(n - 1)) + list(range(1, n_tips + 1))
    dst = list(range(1, n)) + list(range(n, n + n_tips))
    return W.from_plus_links(np.arange(1, n + n_tips + 1), np.array(src, dtype=np.uint32), np.array(dst, dtype=np.uint32))


def chain(n):
    return W.from_plus_links(np.arange(1, n + 1), np.arange(n - 1, dtype=np.uint32), np.arange(1, n, dtype=np.uint32))


def bridges_on_a_ring(n):
    """A ring 0 > 1 > ... > n-1 > 0 with a segment hanging off every ring segment by a bridge link and closed by a hairpin
    link (its r side to itself) instead of a tip: every one of the n bridges gets a simplifying bracket of its own, and all
    of them end at the root."""
    ring_src, ring_dst = list(range(n)), [(i + 1) % n for i in range(n)]
    v1 = np.array(ring_src + list(range(n)) + list(range(n, 2 * n)), dtype=np.uint32)
    v2 = np.array(ring_dst + list(range(n, 2 * n)) + list(range(n, 2 * n)), dtype=np.uint32)
    s1 = np.full(3 * n, W.R, dtype=np.uint8)
    s2 = np.array([W.L] * (2 * n) + [W.R] * n, dtype=np.uint8)
    return W._mk(np.arange(1, 2 * n + 1), v1, s1, v2, s2)


def ring(n):
    """A circular component without tips: the tree's root is a segment side, reached by the 0 -> 0 back edge."""
    return W.from_plus_links(np.arange(1, n + 1), np.arange(n, dtype=np.uint32), (np.arange(n, dtype=np.uint32) + 1) % n)


def root_count(g, kind):
    """Brackets of type `kind` (0 ordinary, 1 capping, 2 simplifying; None: any) that end at the root of component 0."""
    d = dump_component(g, 0)
    root = int(np.flatnonzero(d["par"] == NIL)[0])
    at_root = d["be_tgt"] == root
    return int(at_root.sum() if kind is None else (at_root & (d["be_type"] == kind)).sum()), d


def test_brackets_that_end_at_a_root_are_not_counted(hip, monkeypatch):
    """More than 255 brackets on one root, of any kind, leave the byte form alone: 300 tips under a dummy root, 300 bridge
    segments with a simplifying bracket each (a plain chain of 300 bridges has ONE, at its deepest bridge: both are run), a
    ring (a real root with its own back edge) and components of one and two segments, each alone and all in one pass."""
    tips, bridges, circle = tips_on_a_backbone(300), bridges_on_a_ring(300), ring(12)
    n, _ = root_count(tips, 0)
    assert n > 255
    n, _ = root_count(bridges, 2)
    assert n > 255
    n, d = root_count(circle, None)
    assert n >= 1 and (d["typ"][d["par"] == NIL] != 2).all()  # (no dummy root)
    for g in (tips, bridges, chain(300), circle, sized_components([1]), sized_components([2]),
              concat([sized_components([1, 2]), tips, circle, sized_components([2, 1]), bridges, W.hprc_circular(300)])):
        assert g.n_links == 0 or max_side_links(g) + 2 <= 255
        run_forms(hip, monkeypatch, g, O.decompose(g), ALL_BYTES, flags=(0, F_ALL_VERTEX_CLASSES))


def test_a_byte_that_would_overflow_repeats_the_pass_with_words(hip, monkeypatch):
    """ladder(128): 128 ordinary back edges and 128 capping brackets end at one tree vertex that is no root, on a side with
    129 links -- the gate lets the byte form start, the 256th bracket finds its byte at 255.  The pass runs again with words
    (one repeat, the word form reported) and gives the oracle's forest; an ordinary graph behind it on the same context takes
    the byte form again without a repeat.  (The smallest such graph: a byte holds the ordinary brackets too, so 128 capping
    ones are enough; 256 capping brackets on one target need a side with more links than the gate admits for this shape.)"""
    g = ladder(128)
    cnt, par, d = in_counts(g)
    t = int(cnt.argmax())
    assert par[t] != NIL and cnt[t] == 256 and np.bincount(d["be_type"][d["be_tgt"] == t]).tolist() == [128, 128]
    assert max_side_links(g) == 129
    just_fits = ladder(127, more=1)
    assert in_counts(just_fits)[0][2] == 255
    want, want_fits = O.decompose(g), O.decompose(just_fits)
    monkeypatch.delenv("POVU_HIP_WIDE_COUNTS", raising=False)
    hip.upload(just_fits)
    base = hip.wide_repeat_count()
    assert hip.decompose().texts() == want_fits
    assert hip.last_narrow_forms() == ALL_BYTES and hip.wide_repeat_count() == base
    run_forms(hip, monkeypatch, g, want, ALL_BYTES, repeats=1)
    after = hip.wide_repeat_count()
    assert after == base + len(FLAGS)
    beside = concat([sized_components([5, 1]), g, fan_in(40), comb(7)])  # ... and with other components around it
    run_forms(hip, monkeypatch, beside, O.decompose(beside), ALL_BYTES, repeats=1, flags=(F_NO_STAGE_TIMES,))
    after += 1
    hip.upload(just_fits)
    assert hip.decompose().texts() == want_fits
    assert hip.last_narrow_forms() == ALL_BYTES and hip.wide_repeat_count() == after


# one tile of the one-launch form and its two neighbours, the longest two-launch scans (5 * 10^7 is still below
# primitives_cases.LB_MIN) and the one-launch (look-back) form
SCAN_N = [1, 16383, 16384, 16385, 50_000_000, PC.LB_N]


@pytest.mark.parametrize("n", SCAN_N)
def test_scan_of_bytes_minus_bytes(hip, n):
    """scan_exclusive_diff_u8_u8 against numpy: values up to 255 on both sides, the subtrahend larger than the minuend in about
    half the places (the difference wraps mod 2^32 as the word form's does)."""
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    sub = rng.integers(0, 256, n, dtype=np.uint8)
    a[0], sub[0] = 0, 255
    d =a.astype(np.uint32) - sub.astype(np.uint32)
    want = np.zeros(n, dtype=np.uint32)
    np.cumsum(d[:-1], dtype=np.uint32, out=want[1:])
    assert np.array_equal(hip.debug_scan_diff_u8_u8(a, sub), want)


@pytest.mark.parametrize("n", SCAN_N)
def test_scan_of_two_byte_jobs(hip, n):
    """The pair scan of the byte in-counts and the byte source counts (scan_exclusive_u8 with two jobs) against numpy, the
    jobs of different lengths."""
    rng = np.random.default_rng(n + 7)
    m = PC.second_job_len(n)
    a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, m, dtype=np.uint8)
    wa, wb = np.zeros(n, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    np.cumsum(a[:-1], dtype=np.uint32, out=wa[1:])
    np.cumsum(b[:-1], dtype=np.uint32, out=wb[1:])
    ga, gb = hip.debug_scan_u8(a, b)
    assert np.array_equal(ga, wa) and np.array_equal(gb, wb)
