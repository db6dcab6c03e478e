"""Cases and streams of tests/test_kc_geometry_gpu.py: stage 00's counter (hast_kc_*, kc_kernels.hip) at every K and minimizer length its
front ends dispatch on.  tests/test_kc_dispatch_cpu.py holds this list against the dispatch as the sources spell it: every front end the
sources can produce for 1 <= m <= K <= 32 must have a case here.

A case is (K, m or None for the default, mode, switches): mode "atomic" sets HAST_KC_COUNT=atomic, "partition" sets HAST_KC_COUNT=partition
and HAST_KC_FLUSH=sweep; a minimizer length goes through HAST_MINIMIZER; switches are further HAST_KC_* variables."""
import collections
import random

import numpy as np

from tests.test_kc_gpu import random_stream

Case = collections.namedtuple("Case", "group k m mode switches")

TABLE_BYTES = 64 << 20                      # 524 288 buckets of 8 keys
TABLE_SLOTS = TABLE_BYTES // 128 * 8
DEFAULT_TILE = 4096                         # kc_api.cpp: hast_kc::tile_bases (tests/test_kc_dispatch_cpu.py reads it there)
SIZES = dict(parent=120_000, shared=60_000, more=40_000)
SMALL = {"HAST_KC_RECORD_MB": "8"}          # a record buffer of 1 M records: a counter allocates little
TINY = {"HAST_KC_RECORD_MB": "1", "HAST_KC_FRESH": "0"}     # 131 072 records: several flushes, records without room counted on the spot


def default_m(k):
    """hast_api.cpp default_minimizer_plain (pinned to the source by tests/test_kc_dispatch_cpu.py)"""
    return k if k <= 16 else max(16, k - 8)


# ---- C: the minimizer matrix ---------------------------------------------------------------------------------------------------------
MINIMIZER_PAIRS = [
    (22, 16), (23, 16), (24, 16), (25, 16), (26, 16), (27, 16), (28, 16),
    (21, 1), (21, 8), (21, 15), (21, 17), (21, 21),
    (17, 9), (16, 8), (16, 9), (12, 7), (8, 1), (2, 1),
    (26, 18),
    (32, 32), (32, 16), (32, 1), (31, 17),
    # what tests/test_kc_dispatch_cpu.py asked for on top: the specialised W = 6 and W = 8 and the generic W with a 64-bit m-mer
    # (k_kc_count<6>: runs whole and cut; <8>: W = 8 under m > 16 is always cut; <0>: cut)
    (22, 17), (23, 18), (24, 17), (24, 20),
]
SLICE_PAIRS = [(23, 16), (21, 8)]
N_SLICES = 3


def cases():
    out = []
    for k in range(1, 33):                                                              # A
        out.append(Case("A", k, None, "atomic", {}))
    for k in range(1, 28):                                                              # B
        out.append(Case("B", k, None, "partition", dict(SMALL)))
    for k in range(17, 22):
        out.append(Case("B", k, None, "partition", dict(SMALL, HAST_KC_EMIT="lanes")))
    for k in (19, 21):
        for tile in ("1056", "288"):
            out.append(Case("B", k, None, "partition", dict(SMALL, HAST_KC_TILE=tile)))
    for k in (22, 23, 24):
        out.append(Case("B", k, None, "partition", dict(TINY)))
    for k, m in MINIMIZER_PAIRS:                                                        # C
        out.append(Case("C", k, m, "atomic", {}))
        out.append(Case("C", k, m, "partition", dict(SMALL)))
    return out


def slice_cases():                                                                      # D
    return [Case("D", k, m, mode, dict(SMALL) if mode == "partition" else {}) for k, m in SLICE_PAIRS for mode in ("atomic", "partition")]


def case_id(c):
    s = "%s-k%d" % (c.group, c.k) + ("m%d" % c.m if c.m is not None else "") + "-" + c.mode
    for name in sorted(c.switches):
        if c.switches[name] != SMALL.get(name):
            s += "-%s%s" % (name[len("HAST_KC_"):].lower(), c.switches[name])
    return s


def effective_m(c):
    return default_m(c.k) if c.m is None else c.m


def environment(c):
    """the variables a case sets; every other HAST_KC_* and HAST_MINIMIZER must be unset"""
    env = {"HAST_KC_COUNT": c.mode}
    if c.mode == "partition":
        env["HAST_KC_FLUSH"] = "sweep"
    if c.m is not None:
        env["HAST_MINIMIZER"] = str(c.m)
    env.update(c.switches)
    return env


CLEARED = ("HAST_KC_COUNT", "HAST_KC_FLUSH", "HAST_KC_EMIT", "HAST_KC_TILE", "HAST_KC_RECORD_MB", "HAST_KC_FRESH", "HAST_KC_L1_SPLIT", "HAST_MINIMIZER")


# ---- streams -------------------------------------------------------------------------------------------------------------------------
_RC = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s[::-1].translate(_RC)


def _bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def palindromes(rng, length):
    """reverse-complement palindromes of `length` bases.  One has an even length (no base is its own complement): for an odd length,
    the palindromes of length - 1 and length + 1 around the same centre, so that windows of `length` lie one base off it both ways"""
    if length % 2 == 0:
        half = _bases(rng, length // 2)
        return [half + revcomp(half)]
    half = _bases(rng, (length + 1) // 2)
    return [half + revcomp(half)] + ([half[1:] + revcomp(half[1:])] if length > 1 else [])


def geometry_stream(rng, n, k, m, motif):
    """random_stream's bytes (both cases, N, IUPAC, separators, CR, homopolymers, motifs on both strands) cut into pieces, and between the
    pieces what it lacks: tandem repeats of period 2 .. 5 longer than 3 K (one m-mer several times in a window: ties of the minimum
    between occurrences), reverse-complement palindromes of length m and K (an m-mer, a k-mer equal to its other strand), and `motif`
    (40 bases) repeated back to back on either strand.  Random flanks join the insertions to each other so that windows run across."""
    base = random_stream(rng, n, k).tobytes()
    out = bytearray()
    at = 0
    while len(out) < n:
        step = rng.randint(300, 2500)
        out += base[at:at + step]
        at += step
        for _ in range(rng.randint(1, 3)):
            r = rng.random()
            if r < 0.35:
                unit = _bases(rng, rng.randint(2, 5))
                s = (unit * (5 * k + 10))[:rng.randint(3 * k + 1, 5 * k + 5)]
            elif r < 0.55:
                s = rng.choice(palindromes(rng, m))
            elif r < 0.75:
                s = rng.choice(palindromes(rng, k))
            else:
                s = (motif if rng.random() < 0.5 else revcomp(motif)) * rng.randint(2, 6)
            if rng.random() < 0.15:
                s = s.lower()
            out += (_bases(rng, rng.randint(0, k + 3)) + s + _bases(rng, rng.randint(0, k + 3))).encode()
            if rng.random() < 0.3:
                out += rng.choice([b"\n", b"N", b"\r\n", b"n"])
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8).copy()


def streams(k, m):
    """(pat, mat, shared, more) for a (K, m): two parents, a stretch counted into both, and one counted into parent 1 after a read"""
    rng = random.Random(7000 + 40 * k + m)
    motif = _bases(rng, 40)
    return tuple(geometry_stream(rng, SIZES[name], k, m, motif) for name in ("parent", "parent", "shared", "more"))
