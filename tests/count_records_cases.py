"""Shared by the tests of the packed count records (common.hpp: cntrec_prefix / cntrec_count; primitives.hip:
scan_count_records_u8): a numpy restatement of the record layout and of both look-ups, and the generators of the inputs
the GPU tests run -- byte arrays with counts on record and tile edges, and component-size lists that put T-space positions
there.  test_count_records_inputs.py checks on the CPU that the generators contain what they claim."""
import functools

import numpy as np

R = 12  # elements a record


def n_records(n):
    """Records that hold an element of [0, n) (the device array carries one more, of slack)."""
    return (n + R - 1) // R


def records(a):
    """The records of the byte counts `a` as rows of four words: bytes 0..11 = the counts of elements 12 r .. 12 r + 11
    (zero behind the end of `a`), word 3 = the sum (mod 2^32) of every count in front of element 12 r."""
    a = np.asarray(a, dtype=np.uint8)
    nr = n_records(a.size)
    pad = np.zeros(nr * R, dtype=np.uint8)
    pad[:a.size] = a
    rec = np.zeros((nr, 4), dtype=np.uint32)
    if nr:
        rec[:, :3] = pad.view("<u4").reshape(nr, 3)
        sums = pad.reshape(nr, R).sum(axis=1, dtype=np.uint64)
        rec[1:, 3] = (np.cumsum(sums)[:-1] & 0xFFFFFFFF).astype(np.uint32)
    return rec


def split(i):
    """(record, place in it) of element i: i / 12 by a multiply-high with ceil(2^35 / 12), as the device does."""
    i = np.asarray(i, dtype=np.uint64)
    r = ((i * np.uint64(0xAAAAAAAB)) >> np.uint64(32)) >> np.uint64(3)
    return r.astype(np.int64), (i - np.uint64(R) * r).astype(np.int64)


def _count_bytes(rec, r):
    return np.ascontiguousarray(rec[r, :3]).view(np.uint8).reshape(-1, R)


def prefix(rec, i):
    """cntrec_prefix: word 3 of i's record plus the first i - 12 r count bytes of it."""
    r, k = split(i)
    b = _count_bytes(rec, r).astype(np.uint32)
    mask = np.arange(R)[None, :] < k[:, None]
    return (rec[r, 3] + (b * mask).sum(axis=1, dtype=np.uint32)).astype(np.uint32)


def count(rec, i):
    """cntrec_count: count byte i - 12 r of i's record."""
    r, k = split(i)
    return _count_bytes(rec, r)[np.arange(len(r)), k].astype(np.uint32)


def exclusive(a):
    """The word form the records replace: exclusive sums (mod 2^32) of the bytes."""
    a = np.asarray(a, dtype=np.uint8)
    out = np.zeros(a.size, dtype=np.uint32)
    if a.size > 1:
        np.cumsum(a[:-1], dtype=np.uint32, out=out[1:])
    return out


# ---- contents of the byte arrays
CONTENTS = ("zero", "full", "sparse", "tile_last", "tile_first")


@functools.lru_cache(maxsize=None)
def byte_case(n, content, tile):
    """n bytes: all zero / all 255 (n * 255 stays below 2^32 for every size used) / random with four zeros in five / a
    single non-zero byte on the last position of a tile of `tile` elements / on the first position of the next (the last
    / first element of the array where it is shorter than that).  Read-only: shared between tests."""
    if content == "zero":
        a = np.zeros(n, dtype=np.uint8)
    elif content == "full":
        assert n * 255 < 1 << 32
        a = np.full(n, 255, dtype=np.uint8)
    elif content == "sparse":
        rng = np.random.default_rng(n)
        a = rng.integers(1, 256, n, dtype=np.uint8)
        a[rng.random(n) < 0.8] = 0
    else:
        a = np.zeros(n, dtype=np.uint8)
        at = tile - 1 if content == "tile_last" else tile
        a[at if at < n else (n - 1 if content == "tile_last" else 0)] = 200
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def byte_case_sums(n, content, tile):
    s = exclusive(byte_case(n, content, tile))
    s.setflags(write=False)
    return s


def sizes(tile):
    """Array lengths around a record and around a tile of `tile` elements."""
    return [1, R - 1, R, R + 1, tile - 1, tile, tile + 1, 2 * tile + 5, 65 * tile + 7]


def positions(n, limit=100_000):
    """Every position of [0, n) where that is few, else `limit` random ones and both ends."""
    if n <= limit:
        return np.arange(n, dtype=np.uint32)
    rng = np.random.default_rng(n + 1)
    p = rng.integers(0, n, limit, dtype=np.uint64).astype(np.uint32)
    p[:2] = 0, n - 1
    return p


# ---- T-space positions on record and tile edges
def component_ranges(sizes_):
    """T-space of components with the given numbers of segments: component c owns [2 voff[c] + c, 2 voff[c+1] + c], its
    last vertex at the end of that range less one, its spare slot at the end.  Rows (first, last vertex, spare slot)."""
    voff = np.concatenate([[0], np.cumsum(sizes_)])
    c = np.arange(len(sizes_))
    first, spare = 2 * voff[:-1] + c, 2 * voff[1:] + c
    return np.stack([first, spare - 1, spare], axis=1)


def sizes_with_spare_at(p):
    """A size list whose first (p even) or second (p odd) component has its spare slot at T-space position p, so that its
    last vertex is p - 1 and the next component's first vertex p + 1; two components follow."""
    assert p >= 8
    return [p // 2, 3, 5] if p % 2 == 0 else [1, (p - 1) // 2 - 1, 3, 5]


def edge_size_lists(tile):
    """Size lists that put a component's last vertex, its spare slot and the next component's first vertex, each in turn,
    on the positions e - 1, e, e + 1 of an edge e: of a record in mid-array (e = 12 k) and of a tile of `tile` elements."""
    out = []
    for e in (R * 7, tile):
        for p in range(e - 2, e + 3):  # spare slot at p: (last, spare, first) = (p - 1, p, p + 1)
            out.append(sizes_with_spare_at(p))
    return out


# a component (and with it every subtree stretch [v, v + sz) and [m, m + sz) of it) inside ONE record, one over exactly
# TWO, and the graph's last component ending in the array's last record
STRETCH_SIZES = [5, 2, 8, 4]


def records_touched(first, spare):
    return set(range(first // R, spare // R + 1))
