"""Inputs for tests/test_past_one_grid_gpu.py: views just past the grid caps of the framing, routing, binning and conversion kernels.

Those kernels walk tiles of 256 items with a grid capped on the host (`for (tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)`), and
one workgroup of 1024 scans the per-tile sums, every thread taking ceil(n / 1024) of them (scan_device.h).  The sizes below are the
smallest at which a workgroup walks its loop a second time and a scan thread takes more than one tile; tests/test_grid_caps_cpu.py
pins the caps they are derived from to the kernel sources.

Records are tiny, so that half a million of them stay a view of 8 to 35 MB, and nothing in them repeats with a period of whole tiles:
what a record holds is drawn by a hash of its number, so a tile that is read or written in another tile's place shows."""
import random

import numpy as np

from tests import rs_corpus as rc

GRID_CAP = 2048                                  # capped_grid (nl_index.h); the dim3(2048) launches of fq_kernels.hip
NAME_GRID_CAP = 1024                             # k_route_class, k_fq_field2 and the name, insert and tally launches of fq_kernels.hip
TILE = 256                                       # kRsTile, kSqRecTile, kSqFaTile, kTxTile, kRouteTile
COPY_TILE = 4096                                 # kSpanCopyTile
NL_TILE = 4096                                   # kNlTile
SCAN_THREADS = 1024                              # block_exclusive_scan_1024

# 2050 tiles: workgroups 0 and 1 walk a second tile, the last tile is partial and ends inside a wave; the tile scan has per = 3,
# thread 683 takes one tile and the threads behind it none
N2 = GRID_CAP * TILE + TILE + 65
N1 = NAME_GRID_CAP * TILE + TILE + 65            # the same for the kernels capped at 1024 workgroups
EDGES = (GRID_CAP * TILE, GRID_CAP * TILE + 1)   # no second pass; one item in the second pass
B = GRID_CAP * COPY_TILE                         # output bytes one pass of a span copy covers

K = 21
N_KEYS = (40, 37)                                # the two sets differ in size: the denser haplotype is not the one with more votes


def mix(i):
    """a hash of a record's number: what decides its class, its length and its text"""
    return (i * 2654435761 + (i >> 7) * 40503) >> 5 & 0xFFFFFF


def scan_runs(n, threads=SCAN_THREADS):
    """block_exclusive_scan_1024's index arithmetic restated: [(lo, hi)] per thread"""
    per = (n + threads - 1) // threads
    out = []
    for t in range(threads):
        lo = min(t * per, n)
        out.append((lo, min(lo + per, n)))
    return out


def keys():
    both = rc.make_keys(3, K)
    return [both[0][:N_KEYS[0]], both[1][:N_KEYS[1]]]


def _pools(keys, seed):
    """random bases to cut short reads from, and reads with planted keys of both sets (rs_corpus.seq_with_plants)"""
    rng = random.Random(seed)
    soup = bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, 1 << 16)])
    planted = []
    while len(planted) < 256:
        s = rc.seq_with_plants(rng, 30 + len(planted) % 31, keys)
        if any(k in s for k in keys[0] + keys[1]):
            planted.append(s)
    return rng, soup, planted


def read_of(i, keys, soup, planted):
    """the read of record i: one in sixteen from the planted pool; of the rest a third is a key of set 0, a third a key of set 1, a
    third 8 to 20 bases, too short for any vote"""
    h = mix(i)
    if h & 15 == 0:
        return planted[(h >> 4) % len(planted)]
    c = (h >> 4) % 3
    if c < 2:
        return keys[c][(h >> 8) % len(keys[c])]
    at = (h >> 6) % (len(soup) - 32)
    return soup[at:at + 8 + (h >> 3) % 13]


def rs_fastq(n, keys, seed=41):
    """-> ([record bytes] x n, tail): n complete four-line records and the start of one more"""
    _, soup, planted = _pools(keys, seed)
    recs = []
    for i in range(n):
        s = read_of(i, keys, soup, planted)
        recs.append(b"@q%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    return recs, b"@tail x\nACGTAC"


def rs_fasta(n, keys, seed=43, every=8191, width=3 * K):
    """FASTA with n records: junk and blank lines in front of the first header (one of them sequence-like: it counts in line_dst);
    a blank line inside every 97th record; every `every` records one whose `width`-column lines, a key across every line end, reach
    over the next edge of a 256-line tile; one read of 60 000 bases on one line laid where the compacted bases pass B; the other
    reads as read_of draws them, on one line.  -> (bytes, {"straddlers", "long_at", "long_len"}: the record numbers of the
    multi-line records, and the offset and the length of the long read in the compacted bases)"""
    rng, soup, planted = _pools(keys, seed)
    long_pool = rc.seq_with_plants(rng, 262 * width, keys, width)
    dense = rc.seq_with_plants(rng, 3000, keys, dense=True) * 20
    out = [b"junk line before any header\nACGTACGT\n\n   \n"]
    line = 4                                                      # lines so far
    cum = 0                                                       # sequence bytes of the records so far
    info = {"straddlers": [], "long_at": None, "long_len": len(dense)}
    for i in range(n):
        if info["long_at"] is None and cum >= B - len(dense) // 2 and i + 1 < n:
            out.append(b">long read %d\n%s\n" % (i, dense))
            info["long_at"] = cum
            cum += len(dense)
            line += 2
        elif i % every == every // 2 and i + 1 < n:
            n_lines = TILE - line % TILE + 3                      # header at `line`, sequence lines to three past the tile's edge
            s = long_pool[:n_lines * width - 5]
            out.append(b">multi %d\n" % i + b"".join(s[j:j + width] + b"\n" for j in range(0, len(s), width)))
            info["straddlers"].append(i)
            cum += len(s)
            line += 1 + n_lines
        else:
            s = read_of(i, keys, soup, planted)
            if i % 97 == 5 and len(s) > 4:
                out.append(b">a%d\n%s\n\n%s\n" % (i, s[:3], s[3:]))
                line += 4
            else:
                out.append(b">a%d\n%s\n" % (i, s))
                line += 2
            cum += len(s)
    return b"".join(out), info


def sq_fastq(n, seed=47):
    """[record bytes] x n of strict four-line FASTQ, reads of 1 to 9 bases cut from random bases at a hashed place"""
    soup = bytes(np.frombuffer(b"ACGTN", np.uint8)[np.random.default_rng(seed).integers(0, 5, 1 << 16)])
    qual = b"FI#5@+>I5" * 2                                       # (a quality line may start with '@' or '+')
    recs = []
    for i in range(n):
        h = mix(i)
        at, L = (h >> 4) % (len(soup) - 16), 1 + h % 9
        recs.append(b"@s%d\n%s\n+\n%s\n" % (i, soup[at:at + L], qual[(h >> 7) % 9:(h >> 7) % 9 + L]))
    return recs


def sq_fasta(n_lines, seed=53):
    """FASTA of at least n_lines lines for the stage-00 framer: a header every two to seven lines (so nearly every tile of 256 lines
    holds some), sequence lines of 12 to 43 bytes, a blank line now and then, CRLF on every fifth record"""
    soup = bytes(np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.default_rng(seed).integers(0, 9, 1 << 16)])
    out, lines, r = [], 0, 0
    while lines < n_lines:
        h = mix(r)
        brk = b"\r\n" if r % 5 == 0 else b"\n"
        out.append(b">c%d%s" % (r, brk))
        k = 1 + h % 6
        for j in range(k):
            g = mix(r * 8 + j + 1)
            at = (g >> 4) % (len(soup) - 48)
            out.append(soup[at:at + 12 + g % 32] + brk)
        lines += 1 + k
        if h % 11 == 3:
            out.append(b"\n")
            lines += 1
        r += 1
    return b"".join(out)


TX_KEYS = (b"k", b"none", b"one", b"sixteen", b"A_1", b"absent", b"K23456789012345", b"x", b"k", b"nope")


def tx_pairs(n, seed=59):
    """two sides of n four-line pairs for tests.test_tx_gpu.MAP: kept and dropped pairs mixed by a hash, every sixteenth tile of 256 pairs
    kept whole and another dropped whole; reads of 1 to 8 bases, '!' among the qualities; the start of one more record behind each"""
    soup = bytes(np.frombuffer(b"ACGTN", np.uint8)[np.random.default_rng(seed).integers(0, 5, 1 << 16)])
    qual = b"FI!,:5#I" * 2
    r1, r2 = [], []
    for i in range(n):
        h = mix(i)
        t = i // TILE % 16
        key = b"k" if t == 3 else b"absent" if t == 9 else TX_KEYS[h % len(TX_KEYS)]
        at, L1, L2 = (h >> 4) % (len(soup) - 16), 1 + (h >> 3) % 8, 1 + (h >> 9) % 8
        r1.append(b"@p%d#%s/1\n%s\n+\n%s\n" % (i, key, soup[at:at + L1], qual[h % 8:h % 8 + L1]))
        r2.append(b"@p%d#%s/2\n%s\n+\n%s\n" % (i, key, soup[at + 3:at + 3 + L2], qual[h % 7:h % 7 + L2]))
    return b"".join(r1) + b"@part#k/1\nAC", b"".join(r2) + b"@part#k/2\nACGT\n+"


def route_fastq(n):
    """-> (bytes, {field 2 -> class 1..3}): n records of one base ('N': no read is too short) whose header's second field is one of
    90 listed barcodes, "0_0_0" or missing -- the four classes mixed by a hash, nothing the host must take"""
    listed = [b"%d_%d_%d" % (1 + j * 17 % 1536, 1 + j * 5 % 1536, 1 + j) for j in range(90)]
    cls_of = {t: 1 + j % 3 for j, t in enumerate(listed)}
    recs = []
    for i in range(n):
        h = mix(i)
        c = h % 4
        if c == 0:
            head = b"@f%d" % i if h & 16 else b"@f%d#0_0_0/1" % i
        else:
            head = b"@f%d#%s/%d" % (i, listed[(h >> 5) % 30 * 3 + c - 1], 1 + (h >> 4 & 1))
        recs.append(head + b"\nN\n+\nI\n")
    return b"".join(recs), cls_of


def route_fastq_many_lists(n):
    """-> (bytes, {field 2 -> class 1..3}): n records, each with a listed barcode of its own -- the lists are n texts long"""
    listed = [b"%d_%d_%d" % (1 + i % 1536, 1 + i // 1536, 1 + mix(i) % 1536) for i in range(n)]
    cls_of = {t: 1 + mix(i) % 3 for i, t in enumerate(listed)}
    return b"".join(b"@g%d#%s/%d\nN\n+\nI\n" % (i, t, 1 + (i & 1)) for i, t in enumerate(listed)), cls_of


def tally_fastq(n):
    """n records for a tally stream: one key owns runs longer than a wave, the rest goes over some 400 keys; one record in 4001 has a
    key longer than a text record (the caller's), one in 89 no second field"""
    many = [b"%d_%d_%d" % (1 + j * 29 % 1536, j, 7 * j % 1536) for j in range(400)]
    recs = []
    for i in range(n):
        h = mix(i)
        if i % 4001 == 17:
            head = b"@V%d#LONG_KEY_NUMBER_%d/1" % (i, i % 3)
        elif h % 89 == 5:
            head = b"@no barcode %d" % i
        elif (i // 100) % 10 in (1, 4, 7):
            head = b"@V%d#0_0_0/1" % i
        else:
            head = b"@V%d#%s/1" % (i, many[(h >> 3) % 400])
        recs.append(head + b"\nA\n+\nI\n")
    return b"".join(recs)
