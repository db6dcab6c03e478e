"""The device deflate encoder (include/hast.h hast_dz_*, hast_amd/csrc/dz_kernels.hip) through the C ABI: the corpus of
tests/test_dz_core_cpu.py (where deflate encoders break: no distance code, one symbol, lengths over 15, stored fallback, runs, the
piece's borders) -- every output is one gzip member that zlib inflates to the input with CRC-32 and ISIZE checked, no longer than
hast_dz_bound, nothing written behind the bound, the same bytes on every call, and read back by the project's own device inflate.
Then the routing stream with hast_fq_set_route_gz against the quartering goldens (outputs of the real awk program)."""
import ctypes as C
import gzip
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import hast_amd
from tests.test_dz_core_cpu import CORPUS, PIECE, bound, huffman_only

pytestmark = pytest.mark.gpu

CANARY = 4096


@pytest.fixture(scope="module")
def ctx():
    if not os.path.exists(hast_amd.lib_path()):
        hast_amd.build()
    with hast_amd.Context(21) as c:
        yield c


def compress(ctx, data, literals_only=False):
    """data through hast_dz_compress_device; checks the canary behind the bound; returns the member"""
    n = len(data)
    cap = hast_amd.dz_bound(n)
    assert cap == bound(n)
    d_src = ctx.to_device(np.frombuffer(data + b"\x00", dtype=np.uint8).copy())
    d_dst = ctx.alloc(cap + CANARY)
    try:
        ctx.memset(d_dst, 0xA5, cap + CANARY)
        ctx.sync()
        size = ctx.dz_compress_device(d_src, n, d_dst, cap, literals_only=literals_only)
        out = ctx.to_host(d_dst, (cap + CANARY,), np.uint8)
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)
    assert size <= cap
    assert (out[cap:] == 0xA5).all(), "bytes behind hast_dz_bound were written"
    assert (out[size:cap] == 0xA5).all(), "bytes behind the member were written"
    return out[:size].tobytes()


def check_member(blob, data):
    d = zlib.decompressobj(31)
    assert d.decompress(blob) == data and d.eof and d.unused_data == b""


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_zlib_reads_it_back(ctx, name):
    data = CORPUS[name]
    blob = compress(ctx, data)
    check_member(blob, data)
    if name == "random":
        assert len(blob) == 10 + len(data) + 5 * ((len(data) + PIECE - 1) // PIECE) + 10        # (every piece a stored block)


def test_literals_only_and_lengths_over_15(ctx):
    """without the match search the block's histogram is the input's: the skewed input's tree is 18 deep and has to be limited"""
    for name in ("skewed", "fastq_generated", "zeros", "empty", "all_byte_values"):
        check_member(compress(ctx, CORPUS[name], literals_only=True), CORPUS[name])


def test_too_little_room_is_refused(ctx):
    data = CORPUS["piece_plus_1"]
    d_src = ctx.to_device(np.frombuffer(data, dtype=np.uint8).copy())
    cap = hast_amd.dz_bound(len(data))
    d_dst = ctx.alloc(cap)
    try:
        with pytest.raises(hast_amd.HastError) as e:
            ctx.dz_compress_device(d_src, len(data), d_dst, cap - 1)
        assert e.value.status == 1
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)


def test_same_input_same_bytes(ctx):
    for name in ("fastq_golden", "mixed", "distance_32768"):
        a = compress(ctx, CORPUS[name])
        for _ in range(3):
            assert compress(ctx, CORPUS[name]) == a, name


def test_the_projects_device_inflate_reads_it_back(ctx, tmp_path):
    for name in ("fastq_golden", "mixed", "three_pieces_and_7", "random"):
        p = tmp_path / (name + ".gz")
        p.write_bytes(compress(ctx, CORPUS[name]))
        with hast_amd.GzReader(ctx, str(p)) as z:
            got = z.read_all()
            st = z.stats()
        assert got == CORPUS[name], name
        assert st["members"] == 1


def test_it_compresses(ctx):
    """matches are found and coded: a FASTQ with constant quality lines gets smaller than zlib's Huffman-only coding of the same
    bytes, computed here (134 232 bytes; zlib level 1 on pieces of 16 KB: 79 861)"""
    data = CORPUS["fastq_golden"]
    assert len(data) == 347531
    blob = compress(ctx, data)
    print("fastq_golden: %d -> %d bytes (zlib Huffman-only %d)" % (len(data), len(blob), len(huffman_only(data))))
    assert len(blob) < len(huffman_only(data))


# ---- routing: the four runs of a block as gzip members --------------------------------------------------------------------------
def route_gz_through_abi(data, cls_of, block, n_ctx, k=21, members=None):
    """tests/test_fq_gpu.py's route_through_abi with hast_fq_set_route_gz on: every run of a block the device routed is ONE gzip member
    (an empty run: nothing), inflated here and appended; blocks the device hands over and the tail are plain and decided by awk's rule.
    Returns (the four classes' bytes, the dropped field-2 texts, counters).  members: a list that gets a (class, member, its inflated
    bytes) for every device-made member, block after block, the classes of a block rising."""
    import re
    from hast_amd.binding import FqRouted
    lib = hast_amd.lib()
    ctxs = [hast_amd.Context(k) for _ in range(n_ctx)]
    got, dropped = [bytearray() for _ in range(4)], []
    st = {"host_blocks": 0, "blocks": 0, "members": 0, "raw": 0, "compressed": 0}
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
        assert lib.hast_fq_set_route_gz(fq, 1) != 0                 # (a stream that does not route yet)
        tabs = (C.c_void_p * n_ctx)(*[tab.value] * n_ctx)
        assert lib.hast_fq_set_route(fq, tabs, n_ctx) == 0, lib.hast_last_error()
        assert lib.hast_fq_set_route_gz(fq, 1) == 0, lib.hast_last_error()

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
                        assert b.run_bytes[c] == 0 and raw[c] == 0  # (no member for an empty run: awk creates no file it never prints to)
                        continue
                    member = bytes(b.run[c][:b.run_bytes[c]])
                    d = zlib.decompressobj(31)
                    plain = d.decompress(member)
                    assert d.eof and d.unused_data == b"", "a run is exactly one member"
                    assert len(plain) == raw[c]
                    got[c] += plain
                    st["members"] += 1
                    st["raw"] += len(plain)
                    st["compressed"] += len(member)
                    if members is not None:
                        members.append((c, member, plain))
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
def test_routed_runs_as_gzip_members_equal_the_awk_program(n_ctx, block):
    """hast_fq_set_route_gz on the quartering goldens (inputs, lists and outputs of the REAL awk program), plain and striped streams,
    small blocks: each class's members inflated and put together have the bytes and md5 of expected.json; the edge case's records
    match byte for byte and its block with the barcode in no list (9_9_9) comes back as the caller's, as without the switch"""
    import re
    from tests.conftest import GOLDEN
    exp = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))
    e = exp["edge"]
    cls_of = {}
    for name, c in (("p.bc", 1), ("m.bc", 2), ("h.bc", 3)):
        for line in e["inputs"][name].encode().splitlines():
            cls_of.setdefault(re.split(rb"[#/]", line)[0], c)
    got, dropped, st = route_gz_through_abi(e["inputs"]["e.fq"].encode(), cls_of, 4096, n_ctx, k=7)
    names = {0: "e.fq.nobarcode.fastq", 1: "e.fq.paternal.fastq", 2: "e.fq.maternal.fastq", 3: "e.fq.homozygous.fastq"}
    for c in range(4):
        assert got[c].decode() == e["outputs"].get(names[c], ""), names[c]
    assert "".join("ERROR : unclassify barcode : %s\n" % d.decode() for d in dropped) == e["stderr"]
    assert b"9_9_9" in dropped and st["host_blocks"] > 0
    cls_of = {}
    for name, c in (("paternal", 1), ("maternal", 2), ("homozygous", 3)):
        for line in open(os.path.join(GOLDEN, "quartering", name + ".unique.barcodes"), "rb").read().splitlines():
            cls_of.setdefault(re.split(rb"[#/]", line)[0], c)
    for fq in ("r1.fq", "r2.fq"):
        data = gzip.open(os.path.join(GOLDEN, "rand_k21", fq + ".gz")).read()
        if fq == "r2.fq":
            data = data[:-1] + b"\n" + exp["r2_tail"].encode()
        got, dropped, st = route_gz_through_abi(data, cls_of, block, n_ctx)
        want = exp["files"][fq]
        for c, cls in enumerate(("nobarcode", "paternal", "maternal", "homozygous")):
            if cls in want:
                assert (len(got[c]), hashlib.md5(got[c]).hexdigest()) == (want[cls]["bytes"], want[cls]["md5"]), (fq, cls)
            else:
                assert got[c] == b"", (fq, cls)
        err = "".join("ERROR : unclassify barcode : %s\n" % d.decode() for d in dropped).encode()
        assert hashlib.md5(err).hexdigest() == want["stderr_md5"], fq
        assert st["members"] > 0 or st["host_blocks"] == st["blocks"]     # (large blocks: each holds a barcode of no list and is the caller's)
        if block <= 16384:
            assert st["members"] > 0 and st["compressed"] < st["raw"]
        print("%s n_ctx=%d block=%d: %d blocks, %d members, %d -> %d bytes" % (fq, n_ctx, block, st["blocks"], st["members"], st["raw"], st["compressed"]))
