"""Inputs for the tests of the output table made on the GPU (hast_amd/csrc/rows_core.h, rows_kernels.hip): barcode texts and counters
chosen for what the order, the call and the formatting can get wrong.  A case is (name, texts, c0, c1, n0, n1, w0, w1); text16() and
counts4() give it the layout the device step reads."""
import functools
import random

import numpy as np

from tests import rows_model as rm

TILE = 512                                          # rows::kTile of rows_device.h
GRID_CAP = 2048                                     # kGridCap of rows_kernels.hip: the tile loops walk again past GRID_CAP tiles
SCAN_ROUND = 256                                    # tiles k_rows_scan takes a round; four 64-bit carries go from round to round
SORT_MERGE_LIMIT = 1 << 20                          # the library's radix sort: merge sort up to here, Onesweep past it
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 70001)
# 2050 tiles: workgroups 0 and 1 of k_rows_tile_sums and k_rows_write walk a second tile, the last tile holds one row; k_rows_key and
# k_rows_gather (256 ids a workgroup) walk three times; nine scan rounds, the last of two tiles; 513 rows past the merge sort's limit
BIG_N = (GRID_CAP + 1) * TILE + 1
TILE_SIZES = (SCAN_ROUND * TILE, SCAN_ROUND * TILE + 1)      # 256 and 257 tiles: one scan round; a second round of one tile of one row
WEIGHTED = (26, 25, 1.04, 1.0)                      # n0, n1, w0, w1: 25 m / 26 * 1.04 against 25 m / 25
PLAIN = (40, 37, 1.0, 1.0)                          # 40 m / 40 against 37 m / 37: exact ties


def special_names(sep):
    out = [b""] + [b"A" * k for k in range(1, 16)]                                   # every length
    chain = b"1_2_3_4_5_6_7_8"
    out += [chain[:k] for k in range(1, 16)]                                         # 1, 1_, 1_2, ...
    for pos in range(8, 15):                                                         # the same first 8 bytes: the second sort word decides
        for b in (0x30, 0x31, 0x7A):
            out.append(b"ABCDEFGH" + b"m" * (pos - 8) + bytes([b]))
            out.append(b"ABCDEFGH" + b"m" * (pos - 8) + bytes([b]) + b"z" * (14 - pos))
    out += [b"ABCDEFGH", b"ABCDEFG", b"ABCDEFGH\x80", b"ABCDEFGH\x7f", b"ABCDEFGH\x00", b"ABCDEFGH\x00\x00", b"ABCDEFGH\x00\x01"]
    out += [b"ab", b"ab\x00", b"ab\x00\x00", b"ab\x00\x00\x00", b"ab\x01", b"abcdefghijklmn", b"abcdefghijklmn\x00", b"abcdefghijklm\x00\x00"]
    out += [b"\x00" * k for k in range(1, 16)]                                        # only the length byte tells them apart
    for b in (0x00, 0x01, 0x7F, 0x80, 0xFF):
        out += [bytes([b]), b"q" + bytes([b]), b"q" + bytes([b]) + b"q", b"12345678" + bytes([b])]
    out += [b"0", b"0_0", b"0_0_0", b"00", b"0_", b"0_0_", b"0_0_1", b"0_0_0_0", b"1_0_0"]
    if sep:
        out += [b"a#b", b"a/b", b"#", b"/", b"12_34#5", b"x/1", b"123456789012#45", b"1234567890123/"]
    return out


def special_counts(big):
    out = [(0, 0), (5, 0), (0, 7), (1, 1), (9, 10), (10, 9), (99, 100), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1)]
    if big:
        out += [(2 ** 31, 1), (1, 2 ** 31), (2 ** 64 - 1, 1), (1, 2 ** 64 - 1), (2 ** 64 - 1, 2 ** 64 - 1), (2 ** 64 - 1, 0), (0, 2 ** 64 - 1)]
        for k in range(1, 20):
            out += [(10 ** k - 1, 10 ** k), (10 ** k, 10 ** k - 1), (10 ** k, 0), (0, 10 ** k - 1)]
    else:
        for k in range(1, 10):
            out += [(10 ** k - 1, 10 ** k), (10 ** k, 10 ** k - 1)]
    return out


def tie_counts(rng, n0, n1, how_many):
    """products m * n0, m * n1: equal densities before the weights; and their neighbours by one count"""
    out = []
    for _ in range(how_many):
        m = rng.randint(1, 50000)
        out += [(n1 * m if n0 == 26 else n0 * m, n1 * m + d) for d in (-1, 0, 1)]
    return out


def make_case(name, n, seed, weights, big, sep):
    rng = random.Random(seed)
    n0, n1, w0, w1 = weights
    names, seen = [], set()
    bulk = (b"%d_%d_%d" % (rng.randint(1, 1536), rng.randint(1, 1536), rng.randint(1, 1536)) for _ in iter(int, 1))
    for t in special_names(sep):
        if t not in seen:
            seen.add(t)
            names.append(t)
    rng.shuffle(names)                               # (ids are in the order of first sighting, not in any order of the texts)
    while len(names) < n:
        t = next(bulk)
        if t not in seen:
            seen.add(t)
            names.append(t)
    names = names[:n]
    ties = tie_counts(rng, n0, n1, 40)
    counts = special_counts(big) + ties
    while len(counts) < n:
        kind = rng.randrange(4)
        a = rng.randint(1, 3000)
        counts.append(((a, rng.randint(0, 3000)), (a, 0), (0, a), (rng.randint(0, 2 ** 31 - 1), rng.randint(0, 2 ** 31 - 1)))[kind])
    counts = counts[:n]
    if n > 2:                                        # texts and counters meet in another order in every case
        k = rng.randrange(1, n)
        counts = counts[k:] + counts[:k]
    c0, c1 = [c[0] for c in counts], [c[1] for c in counts]
    if n >= 600:                                     # all three calls among the ties and their neighbours
        tie_set = set(ties)
        calls = {rm.hap(t, a, b, n0, n1, w0, w1) for t, a, b in zip(names, c0, c1) if (a, b) in tie_set and t not in (b"0", b"0_0", b"0_0_0")}
        assert calls == {-1, 0, 1}, (name, calls)
    return (name, names, c0, c1, n0, n1, w0, w1)


def cases():
    out = []
    for i, n in enumerate(SIZES):
        weights = WEIGHTED if i % 2 == 0 else PLAIN
        out.append(make_case("n%d" % n, n, 1000 + n, weights, big=(n >= 256), sep=(i % 3 == 0 and n > 0)))
    out.append(make_case("n700_plain_no_sep", 700, 5, PLAIN, big=False, sep=False))
    out.append(make_case("n700_weighted_sep", 700, 6, WEIGHTED, big=True, sep=True))
    return out


@functools.lru_cache(maxsize=None)
def big_case(n=BIG_N, seed=4242):
    """A table past one grid of k_rows_write and past the library's merge sort (BIG_N; tests/test_rows_caps_cpu.py holds the thresholds to
    the sources and the conditions below to the model's output).  The special names, 6000 names that share the first key word
    "ABCDEFGH" and differ in the second, distinct a_b_c with fields 1..1536 (a few names to every first key word), shuffled: ids are in no
    order of the texts.  Counters with PLAIN's exact ties: the special ones, then (a, 0), (0, a), ties (40 m, 37 m) -- twice the share
    of the others -- and their neighbours (40 m + 1, 37 m), (40 m, 37 m + 1), shuffled: a third of the rows on every list, all over
    the sorted order.  Built once a process (the tuple is shared: nobody changes it)."""
    rng = np.random.default_rng(seed)
    n0, n1, w0, w1 = PLAIN
    names = list(dict.fromkeys(special_names(True)))
    seen = set(names)
    names += [b"ABCDEFGH%07d" % s for s in rng.choice(10 ** 7, size=6000, replace=False).tolist()]
    need = n - len(names)
    assert need > 0, n
    triples = np.unique(rng.integers(0, 1536 ** 3, size=need + need // 100 + 1000))          # distinct; (np.unique sorts: shuffled below)
    bulk = [b"%d_%d_%d" % (a, b, c) for a, b, c in zip((triples // 1536 ** 2 + 1).tolist(), (triples // 1536 % 1536 + 1).tolist(), (triples % 1536 + 1).tolist())]
    bulk = [t for t in bulk if t not in seen]
    assert len(bulk) >= need, (len(bulk), need)
    bulk = [bulk[i] for i in rng.permutation(len(bulk))[:need].tolist()]
    names += bulk
    names = [names[i] for i in rng.permutation(n).tolist()]
    counts = special_counts(True)
    m = n - len(counts)
    kind = rng.integers(0, 6, size=m)                                                         # 0: (a, 0)  1: (0, a)  2, 3: a tie  4, 5: its neighbours
    a = rng.integers(1, 3001, size=m)
    mm = rng.integers(1, 50001, size=m)
    c0 = np.select([kind == 0, kind == 1, kind == 4], [a, 0 * a, n0 * mm + 1], n0 * mm)
    c1 = np.select([kind == 0, kind == 1, kind == 5], [0 * a, a, n1 * mm + 1], n1 * mm)
    counts += list(zip(c0.tolist(), c1.tolist()))
    counts = [counts[i] for i in rng.permutation(n).tolist()]
    return ("big%d" % n, names, [c[0] for c in counts], [c[1] for c in counts], n0, n1, w0, w1)


M64 = 2 ** 64 - 1
TILE_KINDS = ("all_list3", "all_list1", "all_list2", "mixed")


def tile_kind(tile):
    return TILE_KINDS[tile % 4]


@functools.lru_cache(maxsize=None)
def tile_case(n, seed=77):
    """Whole tiles of one list, at a scan round's edge (n = TILE_SIZES).  The names are the 15 digits of a permutation of range(n), so a
    row's sorted rank is its number and every list line has 16 bytes; every counter has 20 digits; equal set sizes, equal weights.
    The tiles of the sorted order cycle through TILE_KINDS: all on list 3 (an exact tie of 2^64 - 1: rows of 61 bytes, the staging of
    k_rows_write full, 8192 bytes of lines to the one list), all on list 1 (2^64 - 1 against 10^19), all on list 2 (the mirror),
    and list 1 + rank % 3."""
    perm = np.random.default_rng(seed).permutation(n).tolist()
    names = [b"%015d" % r for r in perm]
    by_list = {1: (M64, 10 ** 19), 2: (10 ** 19, M64), 3: (M64, M64)}
    counts = []
    for r in perm:
        kind = tile_kind(r // TILE)
        counts.append(by_list[3 if kind == "all_list3" else 1 if kind == "all_list1" else 2 if kind == "all_list2" else 1 + r % 3])
    return ("tiles%d" % n, names, [c[0] for c in counts], [c[1] for c in counts], 5, 5, 1.0, 1.0)


def text16(names):
    """the text records as the device dictionary keeps them: the length, the text, zeros"""
    joined = b"".join([bytes((len(t),)) + t.ljust(15, b"\0") for t in names])
    assert len(joined) == 16 * len(names)                                                     # (no text longer than 15 bytes)
    return np.frombuffer(joined, dtype=np.uint8).reshape(len(names), 16).copy()


def counts4(c0, c1):
    a = np.zeros((len(c0), 4), dtype=np.uint64)
    a[:, 0], a[:, 1] = np.array(c0, dtype=np.uint64), np.array(c1, dtype=np.uint64)
    a[:, 2] = (a[:, 0] % np.uint64(1000) * np.uint64(7) + a[:, 1] % np.uint64(1000)) % np.uint64(1000)      # (neg: not part of the table)
    return a
