"""GPU tests of the packed count records: the prefix sums of the byte in-counts (psin) and of the byte source counts (the range
starts of the bracket lists) as one 16-byte record per twelve counts instead of a word per element.  The primitive
(scan_count_records_u8) and both look-ups (cntrec_prefix, cntrec_count) against numpy through the debug entry, the inclusive
word scan against numpy, and whole passes in every form (records, POVU_HIP_WORD_PREFIX = 1 / 2 / 3, POVU_HIP_WIDE_COUNTS = 1 /
2 / 3) against the CPU oracle, with the form that ran asserted."""
import numpy as np
import pytest

import count_records_cases as CR
import oracle_lib as O
import primitives_cases as PC
from povu_amd import HipDecomposer
from povu_amd.hip import F_ALL_VERTEX_CLASSES, F_CHECK_LAMINAR, F_NO_STAGE_TIMES
from test_gpu_narrow_counts import comb, fan_in, fits_bytes, mixed_graph
from test_gpu_narrow_incnt import ladder
from test_gpu_stack_lookups import concat, sized_components

pytestmark = pytest.mark.gpu

FLAGS = (0, F_NO_STAGE_TIMES, F_CHECK_LAMINAR, F_ALL_VERTEX_CLASSES)
REC_PSIN, REC_BSTART = 1, 2


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def tiles(hip):
    """(tile of the two-launch form, tile of the one-launch form) of the record scan, as the library reports them."""
    t = hip.count_record_tiles()
    assert t[0] % CR.R == 0 and t[1] % t[0] == 0 and t[0] > CR.R
    return t


# ---- the primitive and the look-ups
def check_job(got, a, sums):
    rec, pre, cnt, pos = got
    assert np.array_equal(rec, CR.records(a))
    assert np.array_equal(pre, sums[pos])
    assert np.array_equal(cnt, a[pos].astype(np.uint32))


def run_one(hip, a, sums):
    pos = CR.positions(a.size)
    rec, pre, cnt = hip.debug_count_records(a, pos)
    check_job((rec, pre, cnt, pos), a, sums)


@pytest.mark.parametrize("content", CR.CONTENTS)
@pytest.mark.parametrize("which", (0, 1))
def test_records_and_look_ups_against_numpy(hip, tiles, which, content):
    """Every size around a record and around a tile (of either form), every content: the records equal the model's, and
    cntrec_prefix / cntrec_count equal the plain exclusive sums / the bytes at every position."""
    tile = tiles[which]
    for n in CR.sizes(tile):
        run_one(hip, CR.byte_case(n, content, tile), CR.byte_case_sums(n, content, tile))


@pytest.mark.parametrize("content", [c for c in CR.CONTENTS if c != "full"])
def test_the_look_back_form(hip, tiles, content):
    """Just above LB_MIN elements -- the form the headline pass takes -- at 10^5 random positions and both ends.  (Not all
    255: those sums would pass 2^32.  Nothing of this size is kept between tests.)"""
    n = PC.LB_N
    a = CR.byte_case.__wrapped__(n, content, tiles[1])
    run_one(hip, a, CR.exclusive(a))


def test_pairs_of_jobs(hip, tiles):
    """Two jobs of unequal length in one launch (short and long first, one of them in the look-back form's one-tile case),
    and a pair with one empty job."""
    t0, t1 = tiles
    for n, m in ((CR.R + 1, 2 * t0 + 5), (65 * t0 + 7, t0 - 1), (t1 + 1, 1), (2 * t1 + 5, 65 * t1 + 7), (t1, 0), (0, t0 + 1)):
        a = CR.byte_case(n, "sparse", t0) if n else np.zeros(0, dtype=np.uint8)
        b = CR.byte_case(m, "sparse", t0) if m else np.zeros(0, dtype=np.uint8)
        pa, pb = CR.positions(n), CR.positions(m)
        ga, gb = hip.debug_count_records(a, pa, b, pb)
        check_job(ga + (pa,), a, CR.exclusive(a))
        check_job(gb + (pb,), b, CR.exclusive(b))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, 16383, 16384, 16385, 2 * 16384 + 5, 65 * 2048 + 7, PC.LB_N])
def test_inclusive_scan_of_words(hip, n):
    """scan_inclusive_u32 against numpy.cumsum around a lane's eight elements, a tile of the two-launch form (2 048) and of
    the look-back form (16 384), and in the look-back form itself."""
    rng = np.random.default_rng(n)
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(hip.debug_scan_inclusive(a), np.cumsum(a, dtype=np.uint32))


# ---- whole passes
def expected_records(g, word_prefix, wide):
    """Records exactly where the matching count is a byte and the switch is off."""
    fits = fits_bytes(g)
    srccnt8, incnt8 = fits and wide not in (1, 2), fits and wide == 0
    return (REC_PSIN if incnt8 and word_prefix not in (1, 2) else 0) | (REC_BSTART if srccnt8 and word_prefix not in (1, 3) else 0)


def run_every_form(hip, monkeypatch, g, want=None, flags=FLAGS):
    want = O.decompose(g) if want is None else want
    hip.upload(g)
    for var, values in (("POVU_HIP_WORD_PREFIX", (0, 1, 2, 3)), ("POVU_HIP_WIDE_COUNTS", (1, 2, 3))):
        for val in values:
            monkeypatch.delenv("POVU_HIP_WORD_PREFIX", raising=False)
            monkeypatch.delenv("POVU_HIP_WIDE_COUNTS", raising=False)
            if val:
                monkeypatch.setenv(var, str(val))
            wp, wide = (val, 0) if var == "POVU_HIP_WORD_PREFIX" else (0, val)
            for fl in flags:
                assert hip.decompose(flags=fl).texts() == want, (var, val, fl)
                assert hip.last_prefix_records() == expected_records(g, wp, wide), (var, val, fl)
    monkeypatch.delenv("POVU_HIP_WORD_PREFIX", raising=False)
    monkeypatch.delenv("POVU_HIP_WIDE_COUNTS", raising=False)


D = [1, 3, CR.R - 1, CR.R, CR.R + 1, 47, 252, 253]


@pytest.mark.parametrize("d", D)
@pytest.mark.parametrize("shape", [fan_in, comb])
def test_counts_up_to_the_byte_limit(hip, monkeypatch, shape, d):
    """d brackets out of one source / into one target, around a record's twelve and up to the byte gate; 253 takes the word
    form."""
    g = shape(d)
    assert expected_records(g, 0, 0) == (3 if d <= 252 else 0)
    run_every_form(hip, monkeypatch, g)


def test_mixed_graph(hip, monkeypatch):
    run_every_form(hip, monkeypatch, mixed_graph())


@pytest.mark.parametrize("which", (0, 1, 2))
def test_components_on_record_and_tile_edges(hip, monkeypatch, tiles, which):
    """A component's last vertex, its spare slot and the next component's first vertex on the positions around a record
    edge (0) and around an edge of the record scan's two-launch tile (1) and look-back tile (2), as the library reports
    them: five size lists each (count_records_cases.edge_size_lists)."""
    lists = CR.edge_size_lists(tiles[0])[:5] if which == 0 else CR.edge_size_lists(tiles[which - 1])[5:]
    assert len(lists) == 5
    for sizes in lists:
        run_every_form(hip, monkeypatch, sized_components(sizes))


def test_subtree_stretches_inside_one_record_over_two_and_on_the_last(hip, monkeypatch):
    run_every_form(hip, monkeypatch, sized_components(CR.STRETCH_SIZES))


def test_overflow_repeat_takes_words_and_the_next_pass_records_again(hip, monkeypatch):
    """ladder(128): the byte in-counts overflow, nothing has indexed with the records yet, the pass runs again with words."""
    monkeypatch.delenv("POVU_HIP_WORD_PREFIX", raising=False)
    monkeypatch.delenv("POVU_HIP_WIDE_COUNTS", raising=False)
    g, small = ladder(128), fan_in(3)
    want, want_small = O.decompose(g), O.decompose(small)
    for fl in FLAGS:
        hip.upload(g)
        before = hip.wide_repeat_count()
        assert hip.decompose(flags=fl).texts() == want, fl
        assert hip.wide_repeat_count() == before + 1 and hip.last_prefix_records() == 0
        hip.upload(small)
        assert hip.decompose(flags=fl).texts() == want_small, fl
        assert hip.last_prefix_records() == 3 and hip.wide_repeat_count() == before + 1


def test_stale_records_of_a_larger_graph_are_not_read(hip, monkeypatch):
    """Two different graphs one after the other on one context, the larger first."""
    monkeypatch.delenv("POVU_HIP_WORD_PREFIX", raising=False)
    monkeypatch.delenv("POVU_HIP_WIDE_COUNTS", raising=False)
    big = concat([mixed_graph(), sized_components([700, 3, 41])])
    small = concat([comb(CR.R + 1), sized_components([2, 9])])
    want_big, want_small = O.decompose(big), O.decompose(small)
    for fl in FLAGS:
        hip.upload(big)
        assert hip.decompose(flags=fl).texts() == want_big, fl
        assert hip.last_prefix_records() == 3
        hip.upload(small)
        assert hip.decompose(flags=fl).texts() == want_small, fl
        assert hip.last_prefix_records() == 3
