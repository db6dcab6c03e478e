"""The device deflate encoder against its host model, BYTE FOR BYTE: what hast_dz_compress_device (hast_amd/csrc/dz_kernels.hip) writes
for an input is the member tests/native/test_dz_core.cpp writes for it -- the 10-byte header, every piece, the CRC-32 / ISIZE trailer.
The driver restates the wave's steps with plain loops over the same dz_core.h functions and the design promises an output that is a
function of the input bytes alone, so a kernel that misses matches, drops or mis-orders table entries, builds another code, stores
a piece it should have coded or puts a piece in the wrong place differs from it somewhere, although zlib would inflate both.  (What
the model itself is worth -- zlib's round trip, the project's decoder, the size against zlib level 1 -- is tests/test_dz_core_cpu.py.)
  A  the corpus, the literals-only cases, a seeded fuzz, the sizes around the laps of k_dz_scan (256 pieces a lap), 21 MB of FASTQ
     (1 282 pieces), every alignment of source and destination
  B  the routing stream (hast_fq_set_route_gz): every device-made member of every block equals the model of its inflated bytes, at
     the small blocks of the goldens and at the 16-MB blocks `classify` frames (members of ~700 pieces at arbitrary byte offsets)
A difference is reported with its first byte offset and the piece it lies in (the driver's -v)."""
import gzip
import json
import os
import random
import re
import subprocess
import zlib

import numpy as np
import pytest

import hast_amd
from tests.conftest import GOLDEN
from tests.test_dz_core_cpu import (CORPUS, FUZZ_MAX, bound, build_driver, compress_with_sizes, fastq_150, fuzz_inputs, lap_content,
                                    lap_sizes)
from tests.test_dz_gpu import CANARY, compress, route_gz_through_abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    if not os.path.exists(hast_amd.lib_path()):
        hast_amd.build()
    with hast_amd.Context(21) as c:
        yield c


class Model:
    """model(data, literals_only=False) -> the member the host model writes; model.sizes: the bytes of its pieces (the last call's).
    sanitized=True: the ASAN + UBSAN build of the driver (4 x slower: the small inputs)."""

    def __init__(self, directory):
        self.dir = directory
        self.asan = build_driver(directory)
        self.fast = build_driver(directory, sanitize=False)
        self.piece = int(subprocess.run([self.fast, "-P"], stdout=subprocess.PIPE, check=True).stdout)
        self.sizes = []
        self.seen = {}

    def __call__(self, data, literals_only=False, sanitized=False):
        key = (data, literals_only) if len(data) <= (1 << 20) and not sanitized else None      # (the routed goldens: the same runs in several geometries)
        if key is not None and key in self.seen:
            blob, self.sizes = self.seen[key]
            return blob
        blob, self.sizes = compress_with_sizes(self.asan if sanitized else self.fast, self.dir, data, literals_only)
        if key is not None:
            self.seen[key] = (blob, self.sizes)
        return blob

    def same(self, got, want, what):
        """got (the device's member) == want (the model's, made by the last call); if not: where they part"""
        if got == want:
            return
        n = min(len(got), len(want))
        differ = np.nonzero(np.frombuffer(got, np.uint8, n) != np.frombuffer(want, np.uint8, n))[0]
        at = int(differ[0]) if differ.size else n
        where, start = "the member's header", 10
        if at >= 10:
            where = "the member's trailer (empty final block, CRC-32, ISIZE)"
            for i, sz in enumerate(self.sizes):
                if at < start + sz:
                    where = "piece %d of %d (input bytes %d ..; the model's piece: %d bytes from offset %d%s)" % (
                        i, len(self.sizes), i * self.piece, sz, start, ", a stored block" if sz > self.piece else "")
                    break
                start += sz
        pytest.fail("%s: the device's member (%d bytes) and the model's (%d bytes) differ first at byte %d, in %s: device %s, model %s" % (
            what, len(got), len(want), at, where, got[at:at + 8].hex(), want[at:at + 8].hex()))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("dzmodel"))


def inflates_to(blob, data):
    d = zlib.decompressobj(31)
    return d.decompress(blob) == data and d.eof and d.unused_data == b""


# ---- A: hast_dz_compress_device == the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CORPUS))
def test_the_corpus(ctx, model, name):
    data = CORPUS[name]
    model.same(compress(ctx, data), model(data, sanitized=len(data) <= 100_000), name)


@pytest.mark.parametrize("name", ["skewed", "fastq_generated", "zeros", "empty", "all_byte_values"])
def test_literals_only(ctx, model, name):
    """HAST_DZ_LITERALS_ONLY against the driver's -H: no match search, the codes of the input's own histogram (lengths over 15)"""
    data = CORPUS[name]
    model.same(compress(ctx, data, literals_only=True), model(data, literals_only=True, sanitized=True), name + ", literals only")


def test_fuzz(ctx, model):
    """tests/test_dz_core_cpu.py's fuzz corpus (HAST_FUZZ_SEED, HAST_FUZZ_ITERS): every input through the driver under ASAN + UBSAN
    first, then through the kernels"""
    inputs = fuzz_inputs()
    assert len(inputs) >= 150 and max(len(d) for d in inputs) <= FUZZ_MAX
    for k, data in enumerate(inputs):
        want = model(data, sanitized=True)
        assert inflates_to(want, data), k
        model.same(compress(ctx, data), want, "fuzz input %d of %d bytes (seed %s)" % (k, len(data), os.environ.get("HAST_FUZZ_SEED", "the default")))


@pytest.mark.parametrize("kind", ["fastq", "mixed_tiled"])
def test_sizes_around_the_laps_of_the_scan(ctx, model, kind):
    """k_dz_scan places 256 pieces a lap and carries the place and the CRC's XOR from lap to lap: 255, 256 (-1 byte, +1 byte), 257
    pieces, 512 pieces + 7 bytes, 1227 pieces - 100 bytes; FASTQ (coded pieces), and FASTQ / noise / zeros tiled (stored and coded
    pieces alternate: the places add n + 5 and coded sizes)"""
    P = model.piece
    content = lap_content(kind)
    sizes = [255 * P, 256 * P - 1, 256 * P, 256 * P + 1, 257 * P, 512 * P + 7, 1227 * P - 100]
    assert sizes == lap_sizes(P)
    for n in sizes:
        data = content[:n]
        assert len(data) == n
        model.same(compress(ctx, data), model(data), "%s, %d bytes" % (kind, n))


@pytest.mark.parametrize("noisy", [False, True], ids=["constant_quality", "noisy_quality"])
def test_21_mb_of_fastq(ctx, model, noisy):
    """one member of 1 282 pieces (five laps and a bit): the model's bytes, and -- independently of the model -- zlib's inflate with
    the CRC-32 and ISIZE of 21 MB checked"""
    data = fastq_150(21_000_000, noisy, 14 + noisy)
    assert len(data) >= 20 << 20 and (len(data) + model.piece - 1) // model.piece >= 1227
    blob = compress(ctx, data)
    assert inflates_to(blob, data)
    model.same(blob, model(data), "21 MB of FASTQ, %s quality lines" % ("noisy" if noisy else "constant"))
    print("21 MB of FASTQ, %s quality lines: %d -> %d bytes, %d pieces" % ("noisy" if noisy else "constant", len(data), len(blob), len(model.sizes)))


FRONT = 64


@pytest.mark.parametrize("name", ["three_pieces_and_7", "mixed", "random"])
def test_every_alignment_of_source_and_destination(ctx, model, name):
    """d_src + i, d_dst + j for i, j in 0 .. 3: load_word's shifted path in k_dz_piece (the input) and k_dz_gather (stored pieces
    from the input, coded ones from their slots), the gather's head / words / tail; canaries in front of the member and behind the
    bound.  The source has i + n + 8 bytes: the words a shifted load touches lie inside it."""
    data = CORPUS[name]
    n = len(data)
    want = model(data, sanitized=True)
    cap = hast_amd.dz_bound(n)
    assert cap == bound(n)
    for i in range(4):
        for j in range(4):
            host = np.zeros(i + n + 8, np.uint8)
            host[i:i + n] = np.frombuffer(data, np.uint8)
            d_src = ctx.to_device(host)
            d_dst = ctx.alloc(FRONT + j + cap + CANARY)
            try:
                assert d_src % 4 == 0 and d_dst % 4 == 0
                ctx.memset(d_dst, 0xA5, FRONT + j + cap + CANARY)
                ctx.sync()
                size = ctx.dz_compress_device(d_src + i, n, d_dst + FRONT + j, cap)
                out = ctx.to_host(d_dst, (FRONT + j + cap + CANARY,), np.uint8)
            finally:
                ctx.free(d_src)
                ctx.free(d_dst)
            assert size <= cap
            assert (out[:FRONT + j] == 0xA5).all(), "bytes in front of d_dst were written (i = %d, j = %d)" % (i, j)
            assert (out[FRONT + j + cap:] == 0xA5).all(), "bytes behind hast_dz_bound were written (i = %d, j = %d)" % (i, j)
            assert (out[FRONT + j + size:FRONT + j + cap] == 0xA5).all(), "bytes behind the member were written (i = %d, j = %d)" % (i, j)
            model.same(out[FRONT + j:FRONT + j + size].tobytes(), want, "%s at d_src + %d, d_dst + %d" % (name, i, j))


# ---- B: the routing stream's members == the model of their bytes ----------------------------------------------------------------
def lists_to_classes(texts):
    """paternal, maternal, homozygous lists (their bytes) -> barcode -> class, as the awk program reads them"""
    cls_of = {}
    for c, text in enumerate(texts, 1):
        for line in text.splitlines():
            cls_of.setdefault(re.split(rb"[#/]", line)[0], c)
    return cls_of


def members_equal_the_model(model, members, what):
    for k, (c, member, plain) in enumerate(members):
        model.same(member, model(plain), "%s: member %d (class %d, %d bytes inflated)" % (what, k, c, len(plain)))


@pytest.mark.parametrize("n_ctx,block", [(1, 16384), (2, 8192), (1, 262144), (3, 40960)])
def test_routed_members_of_the_goldens(model, n_ctx, block):
    """the inputs and geometries of tests/test_dz_gpu.py's routing test (which checks the classes' bytes against the awk program's):
    here every member the device made is the model's member of the bytes it inflates to"""
    exp = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))
    e = exp["edge"]
    members, n_members = [], 0
    route_gz_through_abi(e["inputs"]["e.fq"].encode(), lists_to_classes(e["inputs"][n].encode() for n in ("p.bc", "m.bc", "h.bc")), 4096, n_ctx, k=7, members=members)
    members_equal_the_model(model, members, "edge input, n_ctx %d" % n_ctx)         # (none where its one block is the caller's)
    cls_of = lists_to_classes(open(os.path.join(GOLDEN, "quartering", n + ".unique.barcodes"), "rb").read() for n in ("paternal", "maternal", "homozygous"))
    for fq in ("r1.fq", "r2.fq"):
        data = gzip.open(os.path.join(GOLDEN, "rand_k21", fq + ".gz")).read()
        if fq == "r2.fq":
            data = data[:-1] + b"\n" + exp["r2_tail"].encode()
        members = []
        _, _, st = route_gz_through_abi(data, cls_of, block, n_ctx, members=members)
        assert len(members) == st["members"]
        members_equal_the_model(model, members, "%s, n_ctx %d, blocks of %d" % (fq, n_ctx, block))
        n_members += len(members)
    assert n_members > 0 or block > 16384         # (large blocks: each holds a barcode of no list and is the caller's)


PRODUCTION_BLOCK = 16 << 20


def production_fastq(n_bytes, seed):
    """FASTQ as `classify` routes it, at least n_bytes: 150-bp records, the headers of tests.test_inflate_cpu.fastq, every barcode in
    one of three lists or 0_0_0: ~70 % of the records paternal, ~20 % maternal, ~5 % homozygous, ~5 % 0_0_0.  Barcodes of 5 to 14
    characters, and read numbers that pass 10^9 inside the first block (%09d then writes 10 digits: the 0_0_0 records, which lie in
    front of a block's other runs, are 328 and 329 bytes): the runs' sizes take every value mod 4.  Returns (records, the lists' classes)."""
    r = random.Random(seed)
    names = set()
    while len(names) < 950:
        names.add(b"%d_%d_%d" % (r.randint(1, 1536), r.randint(1, 1536), r.randint(1, 1536)))
    names = sorted(names)
    r.shuffle(names)
    lists = [names[:700], names[700:900], names[900:]]
    cls_of = {t: c for c, part in enumerate(lists, 1) for t in part}
    rng = np.random.default_rng(seed)
    n = n_bytes // 325 + 1
    bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, 150))
    qual = rng.choice(np.frombuffer(b"FFFFF:F,F#", np.uint8), (n, 150))
    u, pick = rng.random(n), rng.integers(0, 1 << 30, n)
    records = []
    for i in range(n):
        part = lists[0] if u[i] < 0.70 else lists[1] if u[i] < 0.90 else lists[2] if u[i] < 0.95 else (b"0_0_0",)
        records.append(b"@V300R%09d#%s/1\n" % (10**9 - 20_000 + i, part[pick[i] % len(part)]) + bases[i].tobytes() + b"\n+\n" + qual[i].tobytes() + b"\n")
    return records, cls_of


def split_by_awk_rule(records, cls_of):
    """the routing helper's `decide`, record by record: field 2 of the header split at # and /; none or 0_0_0 -> nobarcode"""
    out = [bytearray() for _ in range(4)]
    for rec in records:
        f = re.split(rb"[#/]", rec[:rec.index(b"\n")])
        c = 0 if len(f) <= 1 or f[1] == b"0_0_0" else cls_of[f[1]]         # (KeyError: a barcode of no list -- this input has none)
        out[c] += rec
    return [bytes(o) for o in out]


def run_starts_in_their_blocks(members):
    """where every member's plain run started in its block's routed bytes: the runs of a block lie one behind the other, class 0
    first (a block's members come with rising classes)"""
    starts, at, last = [], 0, 4
    for c, _, plain in members:
        if c <= last:
            at = 0
        starts.append(at)
        at += len(plain)
        last = c
    return starts


@pytest.mark.parametrize("n_ctx", [1, 2])
def test_routed_members_at_the_production_block_size(model, n_ctx):
    """87 MB of FASTQ in blocks of 16 MB, as `classify` frames them: the paternal run of a block is ~11 MB, ~700 pieces (more than
    two laps of k_dz_scan), the runs start at arbitrary byte offsets of the block's routed bytes; no block is handed to the host"""
    records, cls_of = production_fastq(5 * PRODUCTION_BLOCK + (3 << 20), 31)
    data = b"".join(records)
    assert len(data) >= 48 << 20 and all(rec.count(b"\n") == 4 and rec.index(b"\n") + 305 == len(rec) for rec in records[:1000])
    assert {len(rec) % 4 for rec in records if b"#0_0_0/" in rec[:40]} == {0, 1}
    want = split_by_awk_rule(records, cls_of)
    share = [len(w) / len(data) for w in want]
    assert 0.68 < share[1] < 0.72 and 0.18 < share[2] < 0.22 and 0.04 < share[3] < 0.06 and 0.04 < share[0] < 0.06, share
    members = []
    got, dropped, st = route_gz_through_abi(data, cls_of, PRODUCTION_BLOCK, n_ctx, members=members)
    assert dropped == [] and st["host_blocks"] == 0, st
    assert st["blocks"] >= len(data) // PRODUCTION_BLOCK and len(members) == st["members"] >= 4 * (len(data) // PRODUCTION_BLOCK)
    for c in range(4):
        assert got[c] == want[c], "class %d: %d bytes routed, %d expected" % (c, len(got[c]), len(want[c]))
    longest = max(len(plain) for _, _, plain in members)
    assert longest > 256 * model.piece, "no member of more than 256 pieces (the longest: %d bytes)" % longest
    starts = run_starts_in_their_blocks(members)
    assert {s % 4 for s in starts} == {0, 1, 2, 3}, sorted(s % 4 for s in starts)
    members_equal_the_model(model, members, "87 MB, n_ctx %d" % n_ctx)
    print("n_ctx=%d: %d blocks, %d members (the longest %d bytes = %d pieces), %d -> %d bytes, run starts mod 4: %s" % (
        n_ctx, st["blocks"], len(members), longest, (longest + model.piece - 1) // model.piece, st["raw"], st["compressed"], sorted(s % 4 for s in starts)))
