"""Inputs for the tests of the output table made on the GPU (hast_amd/csrc/rows_core.h, rows_kernels.hip): barcode texts and counters
chosen for what the order, the call and the formatting can get wrong.  A case is (name, texts, c0, c1, n0, n1, w0, w1); text16() and
counts4() give it the layout the device step reads."""
import random

import numpy as np

from tests import rows_model as rm

TILE = 512                                          # rows::kTile of rows_device.h
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 70001)
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


def text16(names):
    a = np.zeros((max(len(names), 1), 16), dtype=np.uint8)
    for i, t in enumerate(names):
        a[i, 0] = len(t)
        a[i, 1:1 + len(t)] = np.frombuffer(t, dtype=np.uint8)
    return a[:len(names)]


def counts4(c0, c1):
    a = np.zeros((max(len(c0), 1), 4), dtype=np.uint64)
    for i, (x, y) in enumerate(zip(c0, c1)):
        a[i, 0], a[i, 1], a[i, 2] = x, y, (x * 7 + y) % 1000          # (neg: not part of the table)
    return a[:len(c0)]
