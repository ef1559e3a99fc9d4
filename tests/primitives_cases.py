"""Inputs of the device-wide primitives' GPU tests (tests/test_gpu_primitives.py) and the sizes they run at.  Every
generator exists for a property of its output -- a place where a kernel of primitives.hip takes another path --, and
tests/test_primitives_inputs.py asserts those properties with numpy alone, without a GPU."""
import zlib

import numpy as np

# ---- these MIRROR constants of povu_amd/csrc/hip/primitives.hip: when a tile changes there, change it here, and the
# sizes below move with it
RS_TILE = CP_TILE = 4096  # pairs of a radix-sort tile / flags of a compaction tile
RS_WAVE_LOAD = 256  # consecutive keys one wave reads with one 16-byte load a lane (k_rs_hist's whole-wave path)
RS_SWITCH = 1 << 24  # up to here 10-bit digits and a 1024-row table, beyond 9 bits and 512 rows (rs_places)
CP_SCAN_THREADS = 1024  # k_cp_scan_tiles: one tile count a thread up to here, several beyond
SC_TILE = 2048  # elements of a scan tile; the one-launch form takes 8 of them a workgroup
S64_N = 1024  # u64 values a block of the u64 scan
X128_TILE = 512  # 16-byte words of a tile of the 128-bit xor scan
LB_MIN = 48 << 20  # elements from which a scan of more than one tile takes the one-launch (look-back) form

LB_N = LB_MIN + 12_345
PAD_KEY = 0xFFFFFFFF  # what k_rs_scatter pads the tail tile with


def _tag(s):
    """A stable number of a name (hash() of a str changes between runs)."""
    return zlib.crc32(s.encode())


def rng_of(name, *nums):
    return np.random.default_rng([_tag(name), *[int(x) for x in nums]])


# ---- sort
SORT_N = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 1, 100003, (1 << 20) + 3, 1 << 24,
          (1 << 24) + 1, (1 << 24) + 4096 + 5]
SORT_BITS_SMALL = [0, 1, 8, 10, 11, 20, 21, 30, 31, 32]  # n <= 2^24: one to four places
SORT_BITS_LARGE = [9, 10, 18, 19, 27, 28, 32]  # n > 2^24
SORT_EVERY_BITS_AT = [4097, 100003, (1 << 24) + 1]
SORT_EVERY_N_AT = [10, 21, 32]
SORT_SHAPES = ["equal", "sorted", "reversed", "top_bit", "runs256+0", "runs256+1", "runs256+2", "runs256+3", "runs_random"]
SORT_SHAPE_N = [4097, 3 * 4096 + 1, 100003]
SORT_PAD_N = [4097, 4096 + 63, 8191, 3 * 4096 + 1]  # all keys = the tail padding: n % 4096 in {1, 63, 4095}, n % 64 != 0


def rs_places(n, bits):
    """(places, digit bits) as rs_places of primitives.hip decides them (bits 0 counts as 1)."""
    bits = max(bits, 1)
    widest = 10 if n <= RS_SWITCH else 9
    places = (bits + widest - 1) // widest
    return places, (bits + places - 1) // places


def sort_grid():
    """The (n, bits) the uniform keys are sorted at: every `bits` at three sizes, every size at three `bits`."""
    grid = []
    for n in SORT_EVERY_BITS_AT:
        grid += [(n, b) for b in (SORT_BITS_SMALL if n <= RS_SWITCH else SORT_BITS_LARGE)]
    for b in SORT_EVERY_N_AT:
        grid += [(n, b) for n in SORT_N if (n, b) not in grid]
    return grid


def uniform_keys(n, bits):
    return rng_of("uniform", n, bits).integers(0, 1 << max(bits, 1), n, dtype=np.uint64).astype(np.uint32)


def shaped_keys(shape, n, bits):
    """Keys below 2^bits of one of SORT_SHAPES."""
    rng = rng_of(shape, n, bits)
    top = 1 << max(bits, 1)
    draw = lambda k: rng.integers(0, top, k, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    if shape == "equal":
        return np.full(n, draw(1)[0], dtype=np.uint32)
    if shape == "sorted":
        return np.sort(draw(n))
    if shape == "reversed":
        return np.sort(draw(n))[::-1].copy()
    if shape == "top_bit":  # two values that differ only in the highest of the `bits` bits
        lo = draw(1)[0] & np.uint32((top >> 1) - 1)
        return np.where(rng.integers(0, 2, n).astype(bool), lo | np.uint32(top >> 1), lo).astype(np.uint32)
    if shape.startswith("runs256+"):
        # stretches of 256 keys, alternately one key and random keys, the first beginning at key `shift`: with shift 0 the
        # one-key stretches are exactly the loads of single waves, and their neighbours are mixed loads
        shift = int(shape[-1])
        k = draw(n)
        for r, a in enumerate(range(shift, n, RS_WAVE_LOAD)):
            if r % 2 == 0:
                k[a:a + RS_WAVE_LOAD] = k[a]
        return k
    if shape == "runs_random":  # runs of one key, 1..2000 long
        lens = rng.integers(1, 2001, n // 1000 + 2)
        while lens.sum() < n:
            lens = np.concatenate([lens, rng.integers(1, 2001, 64)])
        return np.repeat(draw(lens.size), lens)[:n].copy()
    raise ValueError(shape)


def pad_keys(n):
    return np.full(n, PAD_KEY, dtype=np.uint32)


def whole_wave_loads(keys, shift, rb):
    """Per wave load of k_rs_hist that lies wholly inside the array (256 keys from a multiple of 256): do all its keys
    share the digit (keys >> shift) & (2^rb - 1)?  Those loads add 256 to one bin at once."""
    full = keys.size // RS_WAVE_LOAD
    d = ((keys[:full * RS_WAVE_LOAD] >> np.uint32(shift)) & np.uint32((1 << rb) - 1)).reshape(full, RS_WAVE_LOAD)
    return (d == d[:, :1]).all(axis=1)


# ---- compaction
COMPACT_N = [0, 1, 15, 16, 17, 4095, 4096, 4097, 1023 * 4096, 1024 * 4096, 1024 * 4096 + 1, 1025 * 4096 - 3]
COMPACT_FLAGS = ["zero", "all", "half", "sparse", "first", "last", "values"]


def compact_flags(kind, n):
    rng = rng_of(kind, n)
    f = np.zeros(n, dtype=np.uint8)
    if kind == "all":
        f[:] = 1
    elif kind == "half":
        f = rng.integers(0, 2, n).astype(np.uint8)
    elif kind == "sparse":
        f = (rng.random(n) < 1e-4).astype(np.uint8)
    elif kind == "first":
        f[:1] = 1
    elif kind == "last":
        f[n - 1:] = 1
    elif kind == "values":  # set bytes that are not 1: one bit of another byte lane, the sign bit, all bits
        f = np.array([0, 2, 0x80, 0xFF, 0], dtype=np.uint8)[rng.integers(0, 5, n)]
    elif kind != "zero":
        raise ValueError(kind)
    return f


# ---- scans
SCAN_SMALL_N = [1, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 64 * 2048 - 1, 64 * 2048 + 1]
SCAN_N = SCAN_SMALL_N + [30_000_001, LB_N]
XOR_PAIR_N = SCAN_SMALL_N + [LB_N]
X128_N = [1, 2, 511, 512, 513, 1024 * 512 + 1, 3_000_001]
IN_PLACE_N = [1, 2049, 100003, 30_000_001, LB_N]
IN_PLACE_U64_N = [1025, 1024 * 1024 + 3]
TOTALS_N = [0, 1, 255, 256, 257, 1024 * 256 + 1, 5_000_003]


def scan_bytes(n, salt=0):
    return rng_of("bytes", n, salt).integers(0, 256, n, dtype=np.uint8)


def second_job_len(n):
    """Length of the job that shares a launch with one of n elements: another length, never 0."""
    return n // 2 + 1 if n > 2 else n + 2


def scan_words(n, salt=0):
    return rng_of("words", n, salt).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def x128_words(n):
    return rng_of("x128", n).integers(0, 1 << 64, (n, 2), dtype=np.uint64)


def x128_lens(n):
    """Values of *n_dev for n words: *n_dev + 1 below n (where n allows), equal to n, above n."""
    return ([n // 2 - 1] if n >= 2 else []) + [n - 1, n + 5]


def u64_values(n):
    return rng_of("u64", n).integers(0, 1 << 40, n, dtype=np.uint64)


def totals_words(n, salt):
    """Counts of which every other one is 0xFFFFFFFF: from three elements on the total passes 2^32."""
    a = scan_words(n, 100 + salt)
    a[salt % 2::2] = 0xFFFFFFFF
    return a
