"""CPU checks of count_records_cases: the numpy restatement of the count records agrees with plain prefix sums, and the case
generators of test_gpu_count_records contain what they claim (counts on record and tile edges, full bytes, all-zero
records, T-space positions on the edges)."""
import numpy as np
import pytest

import count_records_cases as CR

TILES = (3072, 24576)  # whatever the device reports, the generators must work for it; these are multiples of a record


@pytest.mark.parametrize("n", [1, 11, 12, 13, 24, 100, 3071, 3072, 3073, 30000])
def test_the_model_agrees_with_plain_prefix_sums(n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    rec = CR.records(a)
    assert rec.shape == (CR.n_records(n), 4)
    i = np.arange(n, dtype=np.uint32)
    assert np.array_equal(CR.prefix(rec, i), CR.exclusive(a))
    assert np.array_equal(CR.count(rec, i), a.astype(np.uint32))
    # the count bytes of the last record behind the end of the array are zero
    tail = np.ascontiguousarray(rec[-1, :3]).view(np.uint8)[n - 12 * (CR.n_records(n) - 1):]
    assert not tail.any()


def test_the_multiply_high_is_a_division_by_twelve():
    i = np.concatenate([np.arange(0, 5000), np.arange((1 << 32) - 5000, 1 << 32),
                        np.random.default_rng(0).integers(0, 1 << 32, 100000)]).astype(np.uint64)
    r, k = CR.split(i)
    assert np.array_equal(r, (i // 12).astype(np.int64)) and np.array_equal(k, (i % 12).astype(np.int64))


def test_record_sums_of_full_bytes():
    a = np.full(40, 255, dtype=np.uint8)
    rec = CR.records(a)
    assert rec[3, 3] == 36 * 255 and CR.prefix(rec, [39])[0] == 39 * 255


@pytest.mark.parametrize("tile", TILES)
def test_byte_cases_contain_what_they_claim(tile):
    for n in CR.sizes(tile):
        z, f, s = (CR.byte_case(n, c, tile) for c in ("zero", "full", "sparse"))
        assert z.size == f.size == s.size == n and not z.any() and (f == 255).all()
        if n > 1000:
            assert 0.75 < (s == 0).mean() < 0.85
            rec = CR.records(s)
            assert (rec[:, :3] == 0).all(axis=1).any()          # all-zero records
            nz = np.flatnonzero(s)
            assert {0, 11} <= set((nz % 12).tolist())           # counts on both edges of a record
            assert (s == 255).any() or n < 20000                # full bytes between small ones
        last, first = CR.byte_case(n, "tile_last", tile), CR.byte_case(n, "tile_first", tile)
        assert np.count_nonzero(last) == 1 and np.count_nonzero(first) == 1
        if n > tile:
            assert last[tile - 1] and first[tile]
        assert not last.flags.writeable
    assert CR.sizes(tile)[-1] * 255 < 1 << 32


def test_positions_cover_both_ends():
    assert np.array_equal(CR.positions(50), np.arange(50))
    p = CR.positions(10 ** 7)
    assert p.size == 100_000 and p.min() == 0 and p.max() == 10 ** 7 - 1


@pytest.mark.parametrize("tile", TILES)
def test_size_lists_put_components_on_the_edges(tile):
    hit = {e: set() for e in (12 * 7, tile)}
    for sizes in CR.edge_size_lists(tile):
        assert all(s >= 1 for s in sizes)
        rows = CR.component_ranges(sizes)
        # consecutive components: the next one's first vertex follows the spare slot
        assert (rows[1:, 0] == rows[:-1, 2] + 1).all() and rows[0, 0] == 0
        for c in range(len(sizes) - 1):
            last, spare, nxt = int(rows[c, 1]), int(rows[c, 2]), int(rows[c + 1, 0])
            for e in hit:
                for what, p in (("last", last), ("spare", spare), ("first", nxt)):
                    if abs(p - e) <= 1:
                        hit[e].add((what, p - e))
    want = {(w, d) for w in ("last", "spare", "first") for d in (-1, 0, 1)}
    for e in hit:
        assert hit[e] == want, e


def test_stretch_components_lie_where_they_should():
    rows = CR.component_ranges(CR.STRETCH_SIZES)
    touched = [CR.records_touched(int(f), int(s)) for f, _, s in rows]
    assert len(touched[0]) == 1                      # a component inside one record
    assert len(touched[2]) == 2                      # one over exactly two
    n = int(rows[-1, 2]) + 1                         # the scanned elements: T + 1
    assert max(touched[-1]) == CR.n_records(n) - 1   # the last component ends in the array's last record
