"""The device-wide primitives of primitives.hip, each against numpy: a differential suite whose every comparison is exact.

The hooks (povu_hip_debug_sort, _compact, _totals, _scan) hand the primitive scratch of exactly the size it asks for, filled
with a non-zero byte, and outputs between guard bands; a primitive that writes outside its output raises GuardBandError
with its name.  The inputs come from tests/primitives_cases.py, whose conditions tests/test_primitives_inputs.py checks.

    primitive                        test function
    -------------------------------  ----------------------------------------------------------------------
    sort_pairs_u32                   test_sort_uniform, test_sort_shapes, test_sort_keys_equal_to_the_padding,
                                     test_sort_random_values
    compact_flagged_u8               test_compaction
    scan_exclusive_u8                test_scan_bytes
    scan_exclusive_diff_u32          test_scan_difference
    scan_exclusive_xor_u32_pair      test_scan_xor_pair
    scan_exclusive_xor_u128          test_scan_xor_u128
    totals_u32                       test_totals
    scans with in == out             test_scan_in_place (u32 sum and maximum), test_scan_u64_in_place
    every hook, twice, mixed sizes   test_hooks_in_a_mixed_sequence

(scan_exclusive_u32, _max_u32, _u32_pair and _u64 out of place: test_single_pass_scans and test_scan_exclusive_u64 of
tests/test_gpu_parity.py, through the same hook.)"""
import numpy as np
import pytest

import primitives_cases as PC
from povu_amd import HipDecomposer

pytestmark = pytest.mark.gpu

M32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


# ---- references
def exclusive(inclusive):
    """An inclusive running reduction whose identity is 0, shifted to exclusive."""
    out = np.empty_like(inclusive)
    out[:1] = 0
    out[1:] = inclusive[:-1]
    return out


def ref_sum32(a):
    """Exclusive sums mod 2^32 of a (any unsigned type)."""
    return (exclusive(np.cumsum(a, dtype=np.uint64)) & M32).astype(np.uint32)


def ref_xor(a):
    return exclusive(np.bitwise_xor.accumulate(a, axis=0))


def check_sort(hip, keys, vals, bits, what):
    order = np.argsort(keys, kind="stable")
    ko, vo = hip.debug_sort(keys, vals, bits)
    assert np.array_equal(ko, keys[order]), what
    assert np.array_equal(vo, vals[order]), what


# ---- sort
@pytest.mark.parametrize("n,bits", PC.sort_grid())
def test_sort_uniform(hip, n, bits):
    """Uniform keys below 2^bits, values = positions (a stable sort is the only right answer): one to four places, on both
    sides of the switch of the digit width at 2^24 pairs."""
    check_sort(hip, PC.uniform_keys(n, bits), np.arange(n, dtype=np.uint32), bits, (n, bits, PC.rs_places(n, bits)))


@pytest.mark.parametrize("bits", PC.SORT_EVERY_N_AT)
@pytest.mark.parametrize("shape", PC.SORT_SHAPES)
def test_sort_shapes(hip, shape, bits):
    """Keys that are all equal, sorted, reversed, two values apart in the top bit, and in runs -- runs of 256 on and off
    the loads of single waves, so that the histogram's whole-wave path counts some loads and not their neighbours."""
    for n in PC.SORT_SHAPE_N:
        check_sort(hip, PC.shaped_keys(shape, n, bits), np.arange(n, dtype=np.uint32), bits, (shape, n, bits))


@pytest.mark.parametrize("n", PC.SORT_PAD_N)
def test_sort_keys_equal_to_the_padding(hip, n):
    """Every key is 0xFFFFFFFF at 32 bits -- what the scatter pads the tail tile with: the live keys of the tail keep their
    order and none is taken for padding."""
    check_sort(hip, PC.pad_keys(n), np.arange(n, dtype=np.uint32), 32, n)
    mixed = PC.pad_keys(n)
    mixed[::3] = PC.uniform_keys(n, 32)[::3]
    check_sort(hip, mixed, np.arange(n, dtype=np.uint32), 32, n)


def test_sort_random_values(hip):
    n, bits = 100003, 21
    check_sort(hip, PC.uniform_keys(n, bits), PC.scan_words(n, 7), bits, "random values")


# ---- compaction
@pytest.mark.parametrize("n", PC.COMPACT_N)
def test_compaction(hip, n):
    """Indices of the set bytes and their number, for no, one and two tiles and around the 1024 tiles from which a thread
    of the counts' scan takes more than one."""
    for kind in PC.COMPACT_FLAGS:
        f = PC.compact_flags(kind, n)
        want = np.flatnonzero(f)
        got, cnt = hip.debug_compact(f)
        assert cnt == want.size, (kind, n)
        assert np.array_equal(got, want.astype(np.uint32)), (kind, n)


# ---- scans
@pytest.mark.parametrize("n", PC.SCAN_N)
def test_scan_bytes(hip, n):
    """Byte inputs: one job, two jobs of different lengths in either order, and a job next to an empty one."""
    m = PC.second_job_len(n)
    a, b = PC.scan_bytes(n), PC.scan_bytes(m, 1)
    want_a, want_b = ref_sum32(a), ref_sum32(b)
    empty = np.zeros(0, dtype=np.uint8)
    assert np.array_equal(hip.debug_scan_u8(a), want_a)
    for x, y, wx, wy in ((a, b, want_a, want_b), (b, a, want_b, want_a), (a, empty, want_a, want_a[:0]), (empty, a, want_a[:0], want_a)):
        gx, gy = hip.debug_scan_u8(x, y)
        assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (n, x.size, y.size)


@pytest.mark.parametrize("n", PC.SCAN_N)
def test_scan_difference(hip, n):
    """Sums of in[i] - sub[i] mod 2^32, about half of the terms negative."""
    a, sub = PC.scan_words(n, 0), PC.scan_words(n, 1)
    want = ref_sum32(a - sub)  # (uint32 arithmetic wraps as the kernel's does)
    assert np.array_equal(hip.debug_scan_diff(a, sub), want)


@pytest.mark.parametrize("n", PC.XOR_PAIR_N)
def test_scan_xor_pair(hip, n):
    a, b = PC.scan_words(n, 2), PC.scan_words(n, 3)
    ga, gb = hip.debug_scan_xor_pair(a, b)
    assert np.array_equal(ga, ref_xor(a)) and np.array_equal(gb, ref_xor(b))


@pytest.mark.parametrize("n", PC.X128_N)
def test_scan_xor_u128(hip, n):
    """Running xor of 16-byte words as two uint64 columns; with a device-side length the words behind it stay untouched
    (the hook guards them)."""
    a = PC.x128_words(n)
    want = ref_xor(a)
    assert np.array_equal(hip.debug_scan_xor_u128(a), want)
    for n_dev in PC.x128_lens(n):
        live = min(n_dev + 1, n)
        got = hip.debug_scan_xor_u128(a, n_dev=n_dev)
        assert got.shape == (live, 2) and np.array_equal(got, want[:live]), (n, n_dev)


@pytest.mark.parametrize("n", PC.IN_PLACE_N)
def test_scan_in_place(hip, n):
    """out == in, as the sort scans its table and bitrank_build its counts: one tile, two launches, one launch."""
    a = PC.scan_words(n, 4)
    assert np.array_equal(hip.debug_scan(a, 0, in_place=True), ref_sum32(a))
    assert np.array_equal(hip.debug_scan(a, 1, in_place=True), exclusive(np.maximum.accumulate(a)))


@pytest.mark.parametrize("n", PC.IN_PLACE_U64_N)
def test_scan_u64_in_place(hip, n):
    a = PC.u64_values(n)
    got = hip.debug_scan(a, 2, in_place=True)
    assert got.dtype == np.uint64 and np.array_equal(got, exclusive(np.cumsum(a, dtype=np.uint64)))


# ---- totals
@pytest.mark.parametrize("n", PC.TOTALS_N)
def test_totals(hip, n):
    a, b = PC.totals_words(n, 0), PC.totals_words(n, 1)
    sa, sb = int(a.sum(dtype=np.uint64)), int(b.sum(dtype=np.uint64))
    assert hip.debug_totals(a) == sa
    assert hip.debug_totals(a, b) == (sa, sb)


# ---- every hook twice on one context, other sizes in between
def test_hooks_in_a_mixed_sequence(hip):
    for n in (100003, 5, 4097, 100003, 17, 2 * 8 * PC.SC_TILE + 1):
        k = PC.uniform_keys(n, 21)
        check_sort(hip, k, np.arange(n, dtype=np.uint32), 21, n)
        f = PC.compact_flags("half", n)
        got, cnt = hip.debug_compact(f)
        assert cnt == np.count_nonzero(f) and np.array_equal(got, np.flatnonzero(f))
        a, b = PC.scan_words(n, 5), PC.scan_words(n, 6)
        assert hip.debug_totals(a, b) == (int(a.sum(dtype=np.uint64)), int(b.sum(dtype=np.uint64)))
        assert np.array_equal(hip.debug_scan(a, 0), ref_sum32(a))
        assert np.array_equal(hip.debug_scan(a, 1, in_place=True), exclusive(np.maximum.accumulate(a)))
        ga, gb = hip.debug_scan(a, 0, b[:n // 2 + 1])
        assert np.array_equal(ga, ref_sum32(a)) and np.array_equal(gb, ref_sum32(b[:n // 2 + 1]))
        assert np.array_equal(hip.debug_scan_u8(f), ref_sum32(f))
        assert np.array_equal(hip.debug_scan_diff(a, b), ref_sum32(a - b))
        ga, gb = hip.debug_scan_xor_pair(a, b)
        assert np.array_equal(ga, ref_xor(a)) and np.array_equal(gb, ref_xor(b))
        w = PC.x128_words(n)
        assert np.array_equal(hip.debug_scan_xor_u128(w), ref_xor(w))
        assert np.array_equal(hip.debug_scan_xor_u128(w, n_dev=n // 2), ref_xor(w)[:n // 2 + 1])
        v = PC.u64_values(n)
        assert np.array_equal(hip.debug_scan(v, 2), exclusive(np.cumsum(v, dtype=np.uint64)))
