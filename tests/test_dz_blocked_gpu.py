"""The device deflate encoder writing BLOCKED gzip (BGZF), against its host model BYTE FOR BYTE: what hast_dz_compress_blocked_device
(hast_amd/csrc/dz_kernels.hip: k_dz_piece with the CRC terms advanced to the members' ends, k_dz_scan<true>, k_dz_gather) writes for
an input is what tests/native/test_dz_blocked.cpp writes for it -- every member's 18-byte header with BSIZE, its three pieces, its
CRC-32 / ISIZE.  (What the model is worth: tests/test_dz_blocked_cpu.py.)
  A  the corpus; the sizes around a piece, a member and the laps of the scan (member 85 = pieces 255, 256, 257 straddles the first
     lap's end); 1 227 pieces; every alignment of source and destination; canaries; too little room; the same bytes on every call;
     the project's own per-member device inflate (hast_gz_open_blocked) reads the files back
  B  hast_dz_compress_device on the same inputs still equals ITS model (the piece kernel is shared)
  C  the routing stream with hast_fq_set_route_gz(fq, 2) on the quartering goldens: every device-made run is a whole number of BGZF
     members equal to the model of its inflated bytes, and the classes inflate to the awk program's outputs"""
import ctypes as C
import gzip
import hashlib
import json
import os
import re
import zlib

import numpy as np
import pytest

import hast_amd
from tests.conftest import GOLDEN
from tests.test_dz_blocked_cpu import (EOF_BLOCK, LAP_SIZES, MANY_PIECES, SMALL_SIZES, bound_blocked, build_driver, check_blocked, compress_blocked,
                                       n_members, sized_input, walk_members)
from tests.test_dz_core_cpu import CORPUS, PIECE
from tests.test_dz_gpu import CANARY, compress
from tests.test_dz_model_gpu import Model, lists_to_classes

pytestmark = pytest.mark.gpu

FRONT = 64


@pytest.fixture(scope="module")
def ctx():
    if not os.path.exists(hast_amd.lib_path()):
        hast_amd.build()
    with hast_amd.Context(21) as c:
        yield c


class BlockedModel:
    """model(data) -> the blocked bytes the host model writes for one run (sanitized: the ASAN + UBSAN build, for the small inputs)"""

    def __init__(self, directory):
        self.dir = directory
        self.asan = build_driver(directory)
        self.fast = build_driver(directory, sanitize=False)
        self.seen = {}

    def __call__(self, data, sanitized=False, emit_empty=True):
        key = (data, emit_empty) if len(data) <= (1 << 20) else None
        if key not in self.seen:
            blob = compress_blocked(self.asan if sanitized else self.fast, self.dir, data, emit_empty)[0]
            if key is None:
                return blob
            self.seen[key] = blob
        return self.seen[key]


def same(got, want, what):
    """got (the device's bytes) == want (the model's); if not: the member and the byte they part at"""
    if got == want:
        return
    n = min(len(got), len(want))
    differ = np.nonzero(np.frombuffer(got, np.uint8, n) != np.frombuffer(want, np.uint8, n))[0]
    at = int(differ[0]) if differ.size else n
    where = "behind the model's last member"
    for k, (off, member, _, _) in enumerate(walk_members(want)):
        if off <= at < off + len(member):
            part = "header" if at - off < 18 else "trailer" if at - off >= len(member) - 10 else "pieces"
            where = "member %d (the model's: %d bytes from offset %d), byte %d of it: its %s" % (k, len(member), off, at - off, part)
    pytest.fail("%s: the device's bytes (%d) and the model's (%d) differ first at byte %d, in %s: device %s, model %s" % (
        what, len(got), len(want), at, where, got[at:at + 8].hex(), want[at:at + 8].hex()))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return BlockedModel(tmp_path_factory.mktemp("dzblockedmodel"))


@pytest.fixture(scope="module")
def ordinary_model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("dzordinarymodel"))


def compress_dev(ctx, data, i=0, j=0):
    """data at d_src + i through hast_dz_compress_blocked_device to d_dst + j; canaries in front, behind the bytes written and 4 KB
    behind the bound.  The source has i + n + 8 bytes: the words a shifted load touches lie inside it."""
    n = len(data)
    cap = hast_amd.dz_bound_blocked(n)
    assert cap == bound_blocked(n)
    host = np.zeros(i + n + 8, np.uint8)
    host[i:i + n] = np.frombuffer(data, np.uint8)
    d_src = ctx.to_device(host)
    d_dst = ctx.alloc(FRONT + j + cap + CANARY)
    try:
        ctx.memset(d_dst, 0xA5, FRONT + j + cap + CANARY)
        ctx.sync()
        size = ctx.dz_compress_blocked_device(d_src + i, n, d_dst + FRONT + j, cap)
        out = ctx.to_host(d_dst, (FRONT + j + cap + CANARY,), np.uint8)
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)
    assert size <= cap
    assert (out[:FRONT + j] == 0xA5).all(), "bytes in front of d_dst were written (i = %d, j = %d)" % (i, j)
    assert (out[FRONT + j + cap:] == 0xA5).all(), "bytes behind hast_dz_bound_blocked were written (i = %d, j = %d)" % (i, j)
    assert (out[FRONT + j + size:FRONT + j + cap] == 0xA5).all(), "bytes behind the last member were written (i = %d, j = %d)" % (i, j)
    return out[FRONT + j:FRONT + j + size].tobytes()


SIZED = [(kind, SMALL_SIZES) for kind in ("fastq", "mixed_tiled", "random")] + [(kind, LAP_SIZES) for kind in ("fastq", "mixed_tiled")] + [("mixed_tiled", (MANY_PIECES,))]
SIZED_IDS = ["%s-%s" % (kind, "small" if sizes is SMALL_SIZES else "laps" if sizes is LAP_SIZES else "1227_pieces") for kind, sizes in SIZED]


# ---- A: hast_dz_compress_blocked_device == the model ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CORPUS))
def test_the_corpus(ctx, model, name):
    data = CORPUS[name]
    got = compress_dev(ctx, data)
    same(got, model(data, sanitized=len(data) <= 100_000), name)
    check_blocked(got, data)
    if name == "random":
        assert len(got) == bound_blocked(len(data))
    if name == "empty":
        assert got == EOF_BLOCK


@pytest.mark.parametrize("kind,sizes", SIZED, ids=SIZED_IDS)
def test_the_sizes(ctx, model, kind, sizes):
    """around a piece and a member (0, 1, 16 383 .. 16 385, 49 151 .. 49 153, 98 304 + 7), around the laps of k_dz_scan (255 .. 258
    pieces, a byte less and a byte more each: member 85 lies in both laps), 1 227 pieces (409 members, five laps)"""
    for n in sizes:
        data = sized_input(kind, n)
        assert len(data) == n
        got = compress_dev(ctx, data)
        same(got, model(data), "%s, %d bytes" % (kind, n))
        assert len(walk_members(got)) == max(1, n_members(n))
        if kind == "random":
            assert len(got) == bound_blocked(n)


@pytest.mark.parametrize("name", ["three_pieces_and_7", "mixed", "random"])
def test_every_alignment_of_source_and_destination(ctx, model, name):
    """d_src + i, d_dst + j for i, j in 0 .. 3: the members' frames are byte stores at any address, the pieces' places shift by 28 a
    member against the ordinary layout (the gather's head / words / tail at other alignments)"""
    data = CORPUS[name]
    want = model(data, sanitized=True)
    for i in range(4):
        for j in range(4):
            same(compress_dev(ctx, data, i, j), want, "%s at d_src + %d, d_dst + %d" % (name, i, j))


def test_too_little_room_is_refused(ctx):
    for name in ("piece_plus_1", "empty"):
        data = CORPUS[name]
        d_src = ctx.to_device(np.frombuffer(data + b"\x00", dtype=np.uint8).copy())
        cap = hast_amd.dz_bound_blocked(len(data))
        d_dst = ctx.alloc(cap)
        try:
            with pytest.raises(hast_amd.HastError) as e:
                ctx.dz_compress_blocked_device(d_src, len(data), d_dst, cap - 1)
            assert e.value.status == 1
        finally:
            ctx.free(d_src)
            ctx.free(d_dst)


def test_same_input_same_bytes(ctx):
    for name in ("fastq_golden", "mixed", "distance_32768"):
        a = compress_dev(ctx, CORPUS[name])
        for _ in range(3):
            assert compress_dev(ctx, CORPUS[name]) == a, name


def test_the_projects_blocked_device_inflate_reads_it_back(ctx, tmp_path):
    """hast_gz_open_blocked (a wave per member, bz_kernels.hip) on the encoder's own files: the bytes, and as many members as the
    walk counts"""
    for name in ("fastq_golden", "mixed", "three_pieces_and_7", "random", "empty", "one_byte"):
        blob = compress_dev(ctx, CORPUS[name])
        p = tmp_path / (name + ".gz")
        p.write_bytes(blob)
        with hast_amd.GzReader.blocked(ctx, str(p)) as z:
            got = z.read_all()
            st = z.blocked_stats()
        assert got == CORPUS[name], name
        assert st["members"] == len(walk_members(blob)) == max(1, n_members(len(CORPUS[name]))), name


# ---- B: the ordinary member of the same inputs == its own model -----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CORPUS))
def test_the_ordinary_member_of_the_corpus(ctx, ordinary_model, name):
    data = CORPUS[name]
    ordinary_model.same(compress(ctx, data), ordinary_model(data, sanitized=len(data) <= 100_000), name)


@pytest.mark.parametrize("kind,sizes", SIZED, ids=SIZED_IDS)
def test_the_ordinary_member_of_the_sizes(ctx, ordinary_model, kind, sizes):
    for n in sizes:
        data = sized_input(kind, n)
        ordinary_model.same(compress(ctx, data), ordinary_model(data), "%s, %d bytes" % (kind, n))


# ---- C: the routing stream's runs as blocked gzip ---------------------------------------------------------------------------------
def route_blocked_through_abi(data, cls_of, block, n_ctx, k=21, runs=None):
    """tests/test_dz_gpu.py's route_gz_through_abi with hast_fq_set_route_gz(fq, 2): every run of a block the device routed is a
    whole number of BGZF members (an empty run: nothing, and never an end-of-file block), inflated here member by member and
    appended; blocks the device hands over and the tail are plain and decided by awk's rule.  Returns (the four classes' bytes, the
    dropped field-2 texts, counters).  runs: a list that gets a (class, the run's members, its inflated bytes) per device-made run."""
    from hast_amd.binding import FqRouted
    lib = hast_amd.lib()
    ctxs = [hast_amd.Context(k) for _ in range(n_ctx)]
    got, dropped = [bytearray() for _ in range(4)], []
    st = {"host_blocks": 0, "blocks": 0, "runs": 0, "members": 0, "raw": 0, "compressed": 0}
    try:
        short = [(t, c) for t, c in cls_of.items() if len(t) <= 15]
        text16 = np.zeros((max(len(short), 1), 16), np.uint8)
        ids = np.zeros(max(len(short), 1), np.uint32)
        for i, (t, c) in enumerate(short):
            text16[i, 0] = len(t)
            text16[i, 1:1 + len(t)] = np.frombuffer(t, np.uint8)
            ids[i] = c
        tab = C.c_void_p()
        assert lib.hast_names_create(ctxs[0]._h, max(4096, len(short)), C.byref(tab)) == 0, lib.hast_last_error()
        assert lib.hast_names_insert(tab, text16.ctypes.data_as(C.POINTER(C.c_uint8)), ids.ctypes.data_as(C.POINTER(C.c_uint32)), len(short)) == 0, lib.hast_last_error()
        fq = C.c_void_p()
        if n_ctx > 1:
            arr = (C.c_void_p * n_ctx)(*[c._h for c in ctxs])
            assert lib.hast_fq_create_striped(arr, n_ctx, block, 2, None, C.byref(fq)) == 0, lib.hast_last_error()
        else:
            assert lib.hast_fq_create(ctxs[0]._h, block, 3, None, C.byref(fq)) == 0, lib.hast_last_error()
        tabs = (C.c_void_p * n_ctx)(*[tab.value] * n_ctx)
        assert lib.hast_fq_set_route(fq, tabs, n_ctx) == 0, lib.hast_last_error()
        assert lib.hast_fq_set_route_gz(fq, 3) != 0                 # (0, 1 and 2 are all there is)
        assert lib.hast_fq_set_route_gz(fq, 1) == 0, lib.hast_last_error()
        assert lib.hast_fq_set_route_gz(fq, 2) == 0, lib.hast_last_error()      # (from ordinary members: the buffers grow)

        def decide(head):
            f = re.split(rb"[#/]", head)
            if len(f) <= 1 or f[1] == b"0_0_0":
                return 0
            c = cls_of.get(f[1], -1)
            if c < 0:
                dropped.append(f[1])
            return c

        def drain():
            b = FqRouted()
            assert lib.hast_fq_next_routed(fq, C.byref(b)) == 0, lib.hast_last_error()
            raw = (C.c_uint64 * 4)()
            assert lib.hast_fq_routed_raw_bytes(fq, raw) == 0, lib.hast_last_error()
            st["blocks"] += 1
            if not b.host_block:
                for c in range(4):
                    if b.count[c] == 0:
                        assert b.run_bytes[c] == 0 and raw[c] == 0
                        continue
                    blob = bytes(b.run[c][:b.run_bytes[c]])
                    plain = b"".join(zlib.decompress(m, 31) for _, m, _, _ in walk_members(blob))
                    assert len(plain) == raw[c]
                    assert check_blocked(blob, plain, emit_empty=False) == n_members(len(plain))
                    got[c] += plain
                    st["runs"] += 1
                    st["members"] += n_members(len(plain))
                    st["raw"] += len(plain)
                    st["compressed"] += len(blob)
                    if runs is not None:
                        runs.append((c, blob, plain))
            else:
                st["host_blocks"] += 1
                for i in range(b.n_slots):
                    cl = b.rec_class[i]
                    if cl == 0xFD:
                        continue
                    rec = bytes(b.bytes[b.rec_start[i]:b.rec_start[i] + b.rec_len[i]])
                    if cl > 3:
                        cl = decide(rec.split(b"\n", 1)[0])
                    if cl >= 0:
                        got[cl] += rec
            if b.tail_bytes:
                rest = bytes(b.tail[:b.tail_bytes])
                cl = decide(rest.split(b"\n", 1)[0])
                if cl >= 0:
                    got[cl] += rest + (b"" if rest.endswith(b"\n") else b"\n")
            assert lib.hast_fq_commit(fq) == 0, lib.hast_last_error()

        pos, pending = 0, 0
        while True:
            n = min(len(data) - pos, block)
            buf = C.POINTER(C.c_uint8)()
            assert lib.hast_fq_acquire(fq, C.byref(buf)) == 0, lib.hast_last_error()
            C.memmove(buf, data[pos:pos + n], n)
            pos += n
            last = pos >= len(data)
            assert lib.hast_fq_submit(fq, n, 1 if last else 0) == 0, lib.hast_last_error()
            pending += 1
            while pending > (0 if last else 1):
                drain()
                pending -= 1
            if last:
                break
        lib.hast_fq_destroy(fq)
        lib.hast_names_destroy(tab)
    finally:
        for c in ctxs:
            c.close()
    return [bytes(g) for g in got], dropped, st


@pytest.mark.parametrize("n_ctx,block", [(1, 16384), (2, 8192), (1, 262144), (3, 40960)])
def test_routed_runs_as_blocked_gzip(model, n_ctx, block):
    """the quartering goldens (inputs, lists and outputs of the REAL awk program) at the geometries of tests/test_dz_gpu.py: every
    device-made run equals the model of its inflated bytes, each class's runs put together have the bytes and md5 of expected.json"""
    exp = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))
    e = exp["edge"]
    runs = []
    got, dropped, st = route_blocked_through_abi(e["inputs"]["e.fq"].encode(), lists_to_classes(e["inputs"][n].encode() for n in ("p.bc", "m.bc", "h.bc")), 4096, n_ctx,
                                                 k=7, runs=runs)
    names = {0: "e.fq.nobarcode.fastq", 1: "e.fq.paternal.fastq", 2: "e.fq.maternal.fastq", 3: "e.fq.homozygous.fastq"}
    for c in range(4):
        assert got[c].decode() == e["outputs"].get(names[c], ""), names[c]
    assert "".join("ERROR : unclassify barcode : %s\n" % d.decode() for d in dropped) == e["stderr"]
    assert b"9_9_9" in dropped and st["host_blocks"] > 0
    cls_of = lists_to_classes(open(os.path.join(GOLDEN, "quartering", n + ".unique.barcodes"), "rb").read() for n in ("paternal", "maternal", "homozygous"))
    n_runs = 0
    for fq in ("r1.fq", "r2.fq"):
        data = gzip.open(os.path.join(GOLDEN, "rand_k21", fq + ".gz")).read()
        if fq == "r2.fq":
            data = data[:-1] + b"\n" + exp["r2_tail"].encode()
        got, dropped, st = route_blocked_through_abi(data, cls_of, block, n_ctx, runs=runs)
        want = exp["files"][fq]
        for c, cls in enumerate(("nobarcode", "paternal", "maternal", "homozygous")):
            if cls in want:
                assert (len(got[c]), hashlib.md5(got[c]).hexdigest()) == (want[cls]["bytes"], want[cls]["md5"]), (fq, cls)
            else:
                assert got[c] == b"", (fq, cls)
        err = "".join("ERROR : unclassify barcode : %s\n" % d.decode() for d in dropped).encode()
        assert hashlib.md5(err).hexdigest() == want["stderr_md5"], fq
        n_runs += st["runs"]
        if block <= 16384:
            assert st["runs"] > 0 and st["compressed"] < st["raw"]
    assert n_runs > 0 or block > 16384             # (large blocks: each holds a barcode of no list and is the caller's)
    for k, (c, blob, plain) in enumerate(runs):
        same(blob, model(plain, emit_empty=False), "n_ctx %d, blocks of %d: run %d (class %d, %d bytes inflated)" % (n_ctx, block, k, c, len(plain)))


def test_routed_runs_of_more_than_a_lap(model):
    """the goldens' runs are a member each: here 18 MB of FASTQ in blocks of 8 MB, whose paternal runs are ~5.6 MB (~340 pieces, ~115
    members: past the first lap of k_dz_scan) and start at arbitrary byte offsets of the block's routed bytes"""
    from tests.test_dz_model_gpu import production_fastq, split_by_awk_rule
    block = 8 << 20
    records, cls_of = production_fastq(2 * block + (2 << 20), 33)
    data = b"".join(records)
    want = split_by_awk_rule(records, cls_of)
    runs = []
    got, dropped, st = route_blocked_through_abi(data, cls_of, block, 1, runs=runs)
    assert dropped == [] and st["host_blocks"] == 0, st
    for c in range(4):
        assert got[c] == want[c], "class %d: %d bytes routed, %d expected" % (c, len(got[c]), len(want[c]))
    assert max(len(plain) for _, _, plain in runs) > 256 * PIECE
    assert st["members"] == sum(len(walk_members(blob)) for _, blob, _ in runs) > st["runs"] >= 8
    for k, (c, blob, plain) in enumerate(runs):
        same(blob, model(plain, emit_empty=False), "blocks of 8 MB: run %d (class %d, %d bytes inflated)" % (k, c, len(plain)))
