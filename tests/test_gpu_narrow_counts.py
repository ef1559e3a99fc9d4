"""GPU tests of the bracket counts per tree vertex as bytes: `ordcnt` (ordinary back edges leaving a vertex) and `srccnt`
(brackets per mirror pre-order position) are kept one byte each between the tree stage's emit kernel and the placing of the
brackets whenever no side of the graph has more than 253 links (max(max_side_links, 1) + 2 <= 255); otherwise, and with
POVU_HIP_WIDE_COUNTS=1 in the environment, the word kernels run.  Every case is decided by the CPU oracle, and the two
scans the byte forms go through are checked against numpy."""
import numpy as np
import pytest

import oracle_lib as O
import primitives_cases as PC
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_ALL_VERTEX_CLASSES, F_CHECK_LAMINAR, F_NO_STAGE_TIMES, F_SUBFLUBBLES
from test_gpu_stack_lookups import concat, sized_components
from test_oracle import dump_component

pytestmark = pytest.mark.gpu

FLAGS = (0, F_NO_STAGE_TIMES, F_CHECK_LAMINAR, F_ALL_VERTEX_CLASSES)
D_SORT_FREE = [1, 2, 3, 40, 47]                  # at most 48 links a side: the sort-free path
D_DENSE = list(range(250, 259)) + [300]           # the dense re-index path, on both sides of the gate
NIL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def fan_in(d):
    """A chain 0 > 1 > ... > d+3 and links i > d+1 for i < d: d ordinary back edges leave ONE tree vertex, and the l side
    of segment d+1 carries d+1 links."""
    n = d + 4
    src = list(range(n - 1)) + list(range(d))
    dst = list(range(1, n)) + [d + 1] * d
    return W.from_plus_links(np.arange(1, n + 1), np.array(src, dtype=np.uint32), np.array(dst, dtype=np.uint32))


def comb(d):
    """A chain 0 > ... > d+2 and links d > i for i < d: d back edges END at one vertex, one per source."""
    n = d + 3
    src = list(range(n - 1)) + [d] * d
    dst = list(range(1, n)) + list(range(d))
    return W.from_plus_links(np.arange(1, n + 1), np.array(src, dtype=np.uint32), np.array(dst, dtype=np.uint32))


def max_side_links(g):
    """Most links on one side of a segment (what the gate of the byte form is decided from)."""
    side = np.concatenate([2 * g.v1.astype(np.int64) + g.s1.astype(np.int64), 2 * g.v2.astype(np.int64) + g.s2.astype(np.int64)])
    return int(np.bincount(side).max())


def fits_bytes(g):
    return max(max_side_links(g), 1) + 2 <= 255


def run_both_forms(hip, monkeypatch, g, want, expect_narrow=None):
    """The forests of `g` under every flag, as built and with the word kernels forced; the context says which form ran."""
    narrow = fits_bytes(g) if expect_narrow is None else expect_narrow
    hip.upload(g)
    monkeypatch.delenv("POVU_HIP_WIDE_COUNTS", raising=False)
    for fl in FLAGS:
        assert hip.decompose(flags=fl).texts() == want, fl
        assert hip.last_narrow_counts() == narrow, fl
    monkeypatch.setenv("POVU_HIP_WIDE_COUNTS", "1")
    for fl in FLAGS:
        assert hip.decompose(flags=fl).texts() == want, ("wide", fl)
        assert not hip.last_narrow_counts()
    monkeypatch.delenv("POVU_HIP_WIDE_COUNTS")


def test_the_shapes_have_the_stated_counts():
    """The oracle's dump: fan_in(d) has a tree vertex with d ordinary back edges and a side with d + 1 links, comb(d) a
    vertex where d back edges end, one per source."""
    for d in (3, 47, 252):
        a = dump_component(fan_in(d), 0)
        src, tgt, typ = a["be_src"], a["be_tgt"], a["be_type"]
        ordinary = typ == 0
        assert np.bincount(src[ordinary]).max() == d, d
        assert max_side_links(fan_in(d)) == d + 1
        b = dump_component(comb(d), 0)
        ordinary = b["be_type"] == 0
        assert np.bincount(b["be_tgt"][ordinary]).max() >= d, d
        assert np.bincount(b["be_src"][ordinary]).max() <= 2, d


@pytest.mark.parametrize("d", D_SORT_FREE + D_DENSE)
def test_many_back_edges_out_of_one_source(hip, monkeypatch, d):
    """ordcnt / srccnt up to the byte limit: the byte form below the gate (d + 1 links on the fat side, so d <= 252), the word
    form above it, the same forests either way."""
    g = fan_in(d)
    assert fits_bytes(g) == (d <= 252)
    run_both_forms(hip, monkeypatch, g, O.decompose(g), expect_narrow=d <= 252)


@pytest.mark.parametrize("d", D_SORT_FREE + D_DENSE)
def test_many_brackets_into_one_target(hip, monkeypatch, d):
    """incnt stays a word beside the byte ordcnt: d back edges end at one vertex (and the side they leave from has d + 1
    links, so the gate is crossed at the same d)."""
    g = comb(d)
    run_both_forms(hip, monkeypatch, g, O.decompose(g))


def mixed_graph():
    tiny = lambda: sized_components([1, 2, 1])
    return concat([tiny(), W.bubble_zoo(12, 3, 5, shuffle_ids=False), sized_components([2, 1]), fan_in(252), tiny(),
                   W.nested_towers(6, 4), sized_components([1, 3, 2]), comb(40), W.hprc_circular(300), tiny()])


def test_counts_near_the_limit_beside_capping_and_simplifying_brackets(hip, monkeypatch):
    """One pass with a count of 252 (+ capping / simplifying brackets where they occur) next to ordinary sites, towers, a
    circular component and components of one or two segments in front of, between and behind them (slots of T-space
    without a vertex, which the emit kernel clears in the byte arrays)."""
    g = mixed_graph()
    assert max_side_links(g) == 253
    run_both_forms(hip, monkeypatch, g, O.decompose(g), expect_narrow=True)
    g2 = concat([mixed_graph(), fan_in(253)])  # one fat side more: the whole pass takes the word form
    run_both_forms(hip, monkeypatch, g2, O.decompose(g2), expect_narrow=False)


TILE_SIZES = [
    [128, 8192 - 128 - 1, 3, 8193, 5],  # T-space: 2 * segments + 1 slots a component; a component ends / starts on 16384
    [8192, 3, 8193, 1, 127, 128, 129],  # the spare slot of the first component IS position 16384
    [127, 1, 128, 2, 8190, 3, 64, 8193],
    [3, 125, 128, 3, 8191, 8192],
]


@pytest.mark.parametrize("k", range(len(TILE_SIZES)))
def test_counts_on_tile_edges(hip, monkeypatch, k):
    """Tree vertices with counts on the last and first positions of a 16 384-element scan tile (2 048 in the two-launch form)
    and of a 256-vertex tile of k_bracket_extra; both forms, equal forests."""
    g = sized_components(TILE_SIZES[k])
    run_both_forms(hip, monkeypatch, g, O.decompose(g), expect_narrow=True)


def test_parents_and_sub_pass_behind_a_byte_pass(hip, monkeypatch):
    """debug_tree's parents after a plain pass and after one without stage times equal the oracle's for every component, twice
    in a row, and a -s pass right behind a plain pass on the same context equals the oracle's."""
    monkeypatch.delenv("POVU_HIP_WIDE_COUNTS", raising=False)
    g = concat([mixed_graph(), sized_components([3]), fan_in(47), comb(3)])
    hip.upload(g)
    want, want_sub = O.decompose(g), O.decompose(g, leaf=2)
    for fl in (0, F_NO_STAGE_TIMES):
        assert hip.decompose(flags=fl).texts() == want
        assert hip.last_narrow_counts()
        for again in range(2):
            c = checked = 0
            while True:
                d = dump_component(g, c)
                if d is None:
                    break
                if len(d["gid"]):
                    assert np.array_equal(hip.debug_tree(c)["par"], d["par"]), (fl, again, c)
                    checked += 1
                c += 1
            assert checked >= 20
        assert hip.decompose(flags=F_SUBFLUBBLES).texts() == want_sub


SCAN_N = [1, 15, 16, 17, 2047, 2048, 2049, 16384, 16385, 64 * 2048 + 1, 1024 * 2048 * 3 + 5, PC.LB_N]


@pytest.mark.parametrize("n", SCAN_N)
def test_scan_of_bytes_minus_words(hip, n):
    """scan_exclusive_diff_u8_u32 against numpy: one tile, the two-launch form (tails of chunks) and the look-back form."""
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    sub = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    sub[rng.random(n) < 0.5] = 0
    d = a.astype(np.uint32) - sub
    want = np.zeros(n, dtype=np.uint32)
    np.cumsum(d[:-1], dtype=np.uint32, out=want[1:])
    assert np.array_equal(hip.debug_scan_diff_u8(a, sub), want)


@pytest.mark.parametrize("n", SCAN_N)
def test_scan_of_a_word_job_and_a_byte_job(hip, n):
    """scan_exclusive_u32_u8_pair against numpy, the two jobs of different lengths."""
    rng = np.random.default_rng(n + 1)
    m = PC.second_job_len(n)
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 256, m, dtype=np.uint8)
    wa, wb = np.zeros(n, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    np.cumsum(a[:-1], dtype=np.uint32, out=wa[1:])
    np.cumsum(b[:-1], dtype=np.uint32, out=wb[1:])
    ga, gb = hip.debug_scan_mixed_pair(a, b)
    assert np.array_equal(ga, wa) and np.array_equal(gb, wb)
