"""The inputs of tests/test_gpu_primitives.py have the properties they are there for (tests/primitives_cases.py), and
the tile constants stated there are the ones of primitives.hip.  numpy alone, no GPU."""
import os
import re

import numpy as np
import pytest

import primitives_cases as PC

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "povu_amd", "csrc", "hip", "primitives.hip")


def test_constants_mirror_the_source():
    text = open(SRC).read()
    c = {k: int(v) for k, v in re.findall(r"\b(SC_TPB|SC_ITEMS|CP_TPB|CP_ITEMS|RS_TPB|RS_ITEMS|RS_MAX_BINS|S64_E|X128_ITEMS) = (\d+)\b", text)}
    assert c["SC_TPB"] * c["SC_ITEMS"] == PC.SC_TILE
    assert c["CP_TPB"] * c["CP_ITEMS"] == PC.CP_TILE and c["RS_TPB"] * c["RS_ITEMS"] == PC.RS_TILE
    assert c["SC_TPB"] * c["S64_E"] == PC.S64_N and c["SC_TPB"] * c["X128_ITEMS"] == PC.X128_TILE
    assert 64 * 4 == PC.RS_WAVE_LOAD  # (a wave, four keys a lane and load)
    a, b = re.search(r"LB_MIN = (\d+)u << (\d+);", text).groups()
    assert int(a) << int(b) == PC.LB_MIN
    assert "n <= (size_t(1) << 24) ? 10u : 9u" in text and PC.RS_SWITCH == 1 << 24
    assert re.search(r"__launch_bounds__\(1024\) k_cp_scan_tiles", text) and PC.CP_SCAN_THREADS == 1024
    assert c["RS_MAX_BINS"] == 1 << 10


def test_sort_grid_takes_every_route():
    grid = PC.sort_grid()
    assert len(set(grid)) == len(grid)
    for b in PC.SORT_EVERY_N_AT:
        assert [n for n, bb in grid if bb == b] and {n for n, bb in grid if bb == b} == set(PC.SORT_N)
    for n in PC.SORT_EVERY_BITS_AT:
        want = PC.SORT_BITS_SMALL if n <= PC.RS_SWITCH else PC.SORT_BITS_LARGE
        assert set(want) <= {b for nn, b in grid if nn == n}
    # one to four places on either side of the switch: the last place reaches kout straight (odd) and through tmp (even)
    for side in (lambda n: n <= PC.RS_SWITCH, lambda n: n > PC.RS_SWITCH):
        assert {PC.rs_places(n, b)[0] for n, b in grid if side(n)} == {1, 2, 3, 4}
    # the digit never outgrows the table of its side, and the same `bits` splits differently across the switch
    for n, b in grid:
        assert 1 <= PC.rs_places(n, b)[1] <= (10 if n <= PC.RS_SWITCH else 9)
    assert PC.rs_places(1 << 24, 10) == (1, 10) and PC.rs_places((1 << 24) + 1, 10) == (2, 5)
    assert PC.rs_places(5, 0) == PC.rs_places(5, 1) == (1, 1)
    # sizes around a wave, a wave's load, one tile, several tiles, the switch (by one key and by more than a tile)
    assert {63, 64, 65, 255, 256, 257, PC.RS_TILE - 1, PC.RS_TILE, PC.RS_TILE + 1} <= set(PC.SORT_N)
    assert {PC.RS_SWITCH, PC.RS_SWITCH + 1, PC.RS_SWITCH + PC.RS_TILE + 5} <= set(PC.SORT_N)


@pytest.mark.parametrize("bits", [0, 1, 10, 21, 32])
def test_uniform_keys(bits):
    for n in (1, 4097, 100003):
        k = PC.uniform_keys(n, bits)
        assert k.dtype == np.uint32 and k.size == n and int(k.max()) < 1 << max(bits, 1)
    assert bits < 10 or np.unique(PC.uniform_keys(100003, bits)).size > 1000


@pytest.mark.parametrize("bits", PC.SORT_EVERY_N_AT)
@pytest.mark.parametrize("shape", PC.SORT_SHAPES)
def test_shaped_keys(shape, bits):
    for n in PC.SORT_SHAPE_N:
        k = PC.shaped_keys(shape, n, bits)
        assert k.dtype == np.uint32 and k.size == n and int(k.max()) < 1 << bits
        d = np.diff(k.astype(np.int64))
        rb = PC.rs_places(n, bits)[1]
        whole = PC.whole_wave_loads(k, 0, rb)
        if shape == "equal":
            assert np.unique(k).size == 1 and whole.all()
        elif shape == "sorted":
            assert (d >= 0).all() and (d > 0).any()
        elif shape == "reversed":
            assert (d <= 0).all() and (d < 0).any()
        elif shape == "top_bit":
            u = np.unique(k)
            assert u.size == 2 and int(u[0] ^ u[1]) == 1 << (bits - 1)
            # 256 coin tosses never agree: the two values meet inside every load, and at the last place inside every ballot
            assert not PC.whole_wave_loads(k, (PC.rs_places(n, bits)[0] - 1) * rb, rb).any()
        elif shape.startswith("runs256+"):
            shift = int(shape[-1])
            starts = np.arange(shift, n - PC.RS_WAVE_LOAD, 2 * PC.RS_WAVE_LOAD)
            assert starts.size >= 8 and all(np.unique(k[a:a + PC.RS_WAVE_LOAD]).size == 1 for a in starts)
            if shift == 0:  # the one-key stretches ARE wave loads, and the loads next to them are mixed
                assert whole[0::2].all() and not whole[1::2].any()
            else:  # every one-key stretch straddles two loads: (almost) no load is of one digit
                assert whole.mean() < 0.05
        elif shape == "runs_random":
            edges = np.flatnonzero(np.concatenate([[True], d != 0, [True]]))
            runs = np.diff(edges)
            assert runs.min() >= 1 and runs.max() <= 3 * 2000 and (runs > 2 * PC.RS_WAVE_LOAD).any()
            assert whole.any() and not whole.all()  # loads inside a run next to loads that hold a run's end
            if n == 100003:
                assert (runs < 64).any() and (runs > 1500).any()


def test_pad_keys_equal_the_tail_padding():
    assert {n % PC.RS_TILE for n in PC.SORT_PAD_N} == {1, 63, 4095}
    assert all(n % 64 for n in PC.SORT_PAD_N)
    assert any(n > 2 * PC.RS_TILE for n in PC.SORT_PAD_N)  # (a tail tile behind more than one whole tile)
    for n in PC.SORT_PAD_N:
        k = PC.pad_keys(n)
        assert k.dtype == np.uint32 and k.size == n and (k == 0xFFFFFFFF).all()


def test_compaction_sizes_and_flags():
    tiles = {(n + PC.CP_TILE - 1) // PC.CP_TILE for n in PC.COMPACT_N}
    # no tile, one, two; and one tile count a thread of the counts' scan against two for some threads
    assert {0, 1, 2, PC.CP_SCAN_THREADS - 1, PC.CP_SCAN_THREADS, PC.CP_SCAN_THREADS + 1} <= tiles
    assert {15, 16, 17} <= set(PC.COMPACT_N)  # the 16 flags of one lane's load
    assert any(n % PC.CP_TILE and n % 16 for n in PC.COMPACT_N if n > PC.CP_SCAN_THREADS * PC.CP_TILE)
    for n in (17, 4097, 1024 * 4096 + 1):
        f = {kind: PC.compact_flags(kind, n) for kind in PC.COMPACT_FLAGS}
        assert all(v.dtype == np.uint8 and v.size == n for v in f.values())
        assert not f["zero"].any() and f["all"].all()
        assert np.array_equal(np.flatnonzero(f["first"]), [0]) and np.array_equal(np.flatnonzero(f["last"]), [n - 1])
        if n >= 4097:
            assert 0.4 < f["half"].mean() < 0.6
            assert set(np.unique(f["values"]).tolist()) == {0, 2, 0x80, 0xFF}
        if n > 1 << 20:
            per_tile = np.add.reduceat(f["sparse"] != 0, np.arange(0, n, PC.CP_TILE))
            assert 0 < f["sparse"].sum() < n // 2000 and (per_tile == 0).any() and (per_tile > 0).any()
    assert PC.compact_flags("zero", 0).size == 0 and PC.compact_flags("last", 0).size == 0


def test_scan_sizes():
    lb_tile = 8 * PC.SC_TILE  # one workgroup of the one-launch form
    for sizes in (PC.SCAN_N, PC.XOR_PAIR_N):
        assert {7, 8, 9, 15, 16, 17} <= set(sizes)  # a lane's eight elements, the partials' sixteen bytes a load
        assert {PC.SC_TILE - 1, PC.SC_TILE, PC.SC_TILE + 1} <= set(sizes)
        assert any(lb_tile < n < PC.LB_MIN for n in sizes)  # two launches
        assert any(n >= PC.LB_MIN and n % lb_tile for n in sizes)  # one launch, many tiles, a partial last tile
    assert any(n > 1024 * PC.SC_TILE for n in PC.SCAN_N if n < PC.LB_MIN)  # two launches, several tiles a chunk
    for n in PC.SCAN_N:
        m = PC.second_job_len(n)
        assert 0 < m != n
    assert {PC.X128_TILE - 1, PC.X128_TILE, PC.X128_TILE + 1, 1024 * PC.X128_TILE + 1} <= set(PC.X128_N)
    assert any(n > 2 * 1024 * PC.X128_TILE for n in PC.X128_N)  # several tiles a chunk
    for n in PC.X128_N:
        live = [min(v + 1, n) for v in PC.x128_lens(n)]
        assert all(v >= 0 for v in PC.x128_lens(n)) and n in live
        assert any(v + 1 > n for v in PC.x128_lens(n)) and (n < 2 or any(0 < x < n for x in live))
    assert any(n <= lb_tile for n in PC.IN_PLACE_N) and any(lb_tile < n < PC.LB_MIN for n in PC.IN_PLACE_N)
    assert any(n >= PC.LB_MIN for n in PC.IN_PLACE_N)
    # u64, in place: two blocks (the block sums are scanned in place too), and block sums that fill more than one block
    assert PC.S64_N < PC.IN_PLACE_U64_N[0] <= 2 * PC.S64_N and PC.IN_PLACE_U64_N[1] > PC.S64_N * PC.S64_N


def test_scan_values():
    b = PC.scan_bytes(PC.LB_N)
    assert b.dtype == np.uint8 and int(b.min()) == 0 and int(b.max()) == 255
    assert int(b.sum(dtype=np.uint64)) >= 1 << 32  # the running sum wraps
    del b
    for n in (2049, 64 * 2048 + 1):
        a, sub = PC.scan_words(n, 0), PC.scan_words(n, 1)
        assert a.dtype == sub.dtype == np.uint32 and 0.4 < (sub > a).mean() < 0.6  # about half of the terms wrap
        assert not np.array_equal(PC.scan_bytes(n, 0)[:PC.second_job_len(n)], PC.scan_bytes(PC.second_job_len(n), 1))
    w = PC.x128_words(513)
    assert w.shape == (513, 2) and w.dtype == np.uint64 and int(w.max()) >= 1 << 63
    v = PC.u64_values(1025)
    assert int(np.cumsum(v, dtype=np.uint64)[-2]) >= 1 << 32


def test_totals_values():
    assert {0, 1, 255, 256, 257, 1024 * 256 + 1} <= set(PC.TOTALS_N)  # a block's 256 lanes; a grid capped at 1024 blocks
    assert any(n > 2 * 1024 * 256 for n in PC.TOTALS_N)
    for n in PC.TOTALS_N:
        a, b = PC.totals_words(n, 0), PC.totals_words(n, 1)
        assert a.size == b.size == n and a.dtype == np.uint32
        if n >= 255:
            assert (a == 0xFFFFFFFF).any() and (b == 0xFFFFFFFF).any() and not np.array_equal(a, b)
            assert int(a.sum(dtype=np.uint64)) >= 1 << 32 and int(b.sum(dtype=np.uint64)) >= 1 << 32
