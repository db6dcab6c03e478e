"""GPU test of the stage-00 device framer (hast_sq_*, hast_amd/csrc/sq_kernels.hip): every field of its result and every byte it
writes equal the host model's (tests/native/test_sq_core.cpp, which steps the same sq_core.h and is held to the host parser by
tests/test_sq_core_cpu.py), at every block size, alignment and cut; it writes nothing behind out_bytes and nothing at all for a
block it refuses; and its stream counts to the same table as the parser's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hast_amd
from hast_amd import KmerCounter, SqFeed, SqFramer, SqResult
from tests import sq_corpus as sc
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
CANARY, PAD = 0xEE, 64
NO_BAD = 0xFFFFFFFF
FIELDS = ("consumed", "out_bytes", "records", "bases", "flags", "first_bad")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = C.CDLL(sc.build_native(tmp_path_factory.mktemp("sq_model"), shared=True))
    lib.sq_model_frame.restype = None
    lib.sq_model_frame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(SqResult)]

    def frame(data: np.ndarray):
        out = np.zeros(data.size + 1, dtype=np.uint8)
        res = SqResult()
        lib.sq_model_frame(data.ctypes.data, data.size, out.ctypes.data, C.byref(res))
        return {f: getattr(res, f) for f in FIELDS}, out[:res.out_bytes]
    return frame


class Rig:
    """a count table (the framer runs on its stream), a context for raw device memory, and two reusable device buffers"""

    def __init__(self, cap):
        self.ctx = hast_amd.Context(21)
        self.kc = KmerCounter(21, table_bytes=64 << 20)
        self.cap = cap
        self.d_in = self.ctx.alloc(cap + 64)
        self.d_out = self.ctx.alloc(cap + PAD + 64)
        self.framers = {}

    def framer(self, max_in):
        if max_in not in self.framers:
            self.framers[max_in] = SqFramer(self.kc, max_in)
        return self.framers[max_in]

    def upload(self, data: np.ndarray, at=0):
        hast_amd.lib().hast_memcpy_h2d(self.ctx._h, C.c_void_p(self.d_in + at), data.ctypes.data, data.size)

    def frame(self, max_in, in_at, n, out_at=0):
        """frames d_in[in_at, in_at + n) into d_out + out_at; returns the result and d_out[out_at, out_at + n + PAD) as it stands after"""
        self.ctx.memset(self.d_out + out_at, CANARY, n + PAD)
        self.ctx.sync()
        res = self.framer(max_in).frame_device(self.d_in + in_at, n, self.d_out + out_at, n)
        return {f: getattr(res, f) for f in FIELDS}, self.ctx.to_host(self.d_out + out_at, (n + PAD,), np.uint8)

    def close(self):
        for f in self.framers.values():
            f.close()
        self.kc.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig(48 << 20)
    yield r
    r.close()


def check(got, written, want, want_bytes, what):
    assert got == want, (what, got, want)
    n = want["out_bytes"]
    assert np.array_equal(written[:n], want_bytes), what
    assert (written[n:] == CANARY).all(), (what, "written behind out_bytes")


def as_array(data: bytes):
    return np.frombuffer(data, dtype=np.uint8)


@pytest.mark.parametrize("max_in", (700, 4096, 65536, 16 << 20))
def test_corpus_block_by_block_equals_the_model(rig, model, max_in):
    """the file lies on the device once; a block is [pos, pos + max_in) and pos moves on by `consumed`: the carried bytes in front of
    the new ones, at whatever alignment that gives"""
    n_blocks = 0
    for name, data, longest in sc.valid_corpus():
        if longest > max_in or not data:
            continue
        arr = as_array(data)
        rig.upload(arr)
        pos = 0
        for _ in range(40):                              # (the first 40 blocks of a file say what the rest would)
            n = min(max_in, arr.size - pos)
            got, written = rig.frame(max_in, pos, n)
            want, want_bytes = model(arr[pos:pos + n])
            check(got, written, want, want_bytes, (name, max_in, pos))
            assert not got["flags"] & hast_amd.SQ_NOT_FOUR_LINE, (name, pos)
            n_blocks += 1
            if got["flags"] & hast_amd.SQ_NO_RECORD:
                assert got["consumed"] == 0 and pos + n == arr.size, (name, pos)      # only the end of a file holds no record
                break
            pos += got["consumed"]
            if pos == arr.size:
                break
    assert n_blocks > 50


def test_a_refused_block_leaves_the_output_untouched(rig, model):
    base = sc.fastq(3, 300, (150, 0, 1, 64, 65), b"\n")
    inputs = [sc.mutate(base, kind, seed) for kind in sc.MUTANTS for seed in (0, 1)]
    inputs.append(open(os.path.join(GOLDEN, "s00_edge_k31", "p.fq"), "rb").read())
    flagged = 0
    for i, data in enumerate(inputs):
        arr = as_array(data)
        rig.upload(arr)
        got, written = rig.frame(65536, 0, arr.size)
        want, want_bytes = model(arr)
        check(got, written, want, want_bytes, i)
        if got["flags"] & hast_amd.SQ_NOT_FOUR_LINE:
            flagged += 1
            assert got["out_bytes"] == 0 and got["first_bad"] != NO_BAD and (written == CANARY).all(), i
    assert flagged >= len(inputs) - 2 and model(as_array(inputs[-1]))[0]["flags"] == hast_amd.SQ_NOT_FOUR_LINE


def test_every_alignment_of_input_and_output(rig, model):
    inputs = [sc.fastq(1, 65, (150, 63, 0, 1), b"\n"), sc.fastq(2, 257, (1, 64, 65), b"\r\n"), sc.fastq(3, 5, (4097, 150), b"\r\r\n", False)]
    for i, data in enumerate(inputs):
        arr = as_array(data)
        want, want_bytes = model(arr)
        assert want["records"] > 0
        for a_in in range(16):
            rig.upload(arr, a_in)
            for a_out in range(16):
                got, written = rig.frame(65536, a_in, arr.size, a_out)
                check(got, written, want, want_bytes, (i, a_in, a_out))


def test_every_cut_of_a_small_input(rig, model):
    """[0, s) first, then what it left + [s, end): the two streams together are the whole input's, for every s"""
    data = sc.fastq(4, 3, (9, 0, 13), b"\r\n")
    arr = as_array(data)
    assert 80 <= arr.size <= 130
    whole, whole_bytes = model(arr)
    assert whole["records"] == 3
    rig.upload(arr)
    no_record = 0
    for s in range(arr.size + 1):
        got1, w1 = rig.frame(700, 0, s)
        want1, want1_bytes = model(arr[:s])
        check(got1, w1, want1, want1_bytes, ("first", s))
        if data[:s].count(b"\n") < 4:
            no_record += 1
            assert got1["flags"] == hast_amd.SQ_NO_RECORD and got1["consumed"] == 0 and got1["out_bytes"] == 0, s
        c = got1["consumed"]
        got2, w2 = rig.frame(700, c, arr.size - c)
        want2, want2_bytes = model(arr[c:])
        check(got2, w2, want2, want2_bytes, ("second", s))
        both = np.concatenate([w1[:got1["out_bytes"]], w2[:got2["out_bytes"]]])
        assert np.array_equal(both, whole_bytes) and got1["records"] + got2["records"] == 3, s
    assert no_record > 10


def big_fastq(n_records, read_len=150, seed=5):
    """n_records x (10-byte header, read_len bases, '+', read_len qualities), built as one array"""
    rng = np.random.default_rng(seed)
    width = 11 + read_len + 1 + 2 + read_len + 1
    rows = np.empty((n_records, width), dtype=np.uint8)
    rows[:, :11] = as_array(b"@r00000000\n")
    idx = np.arange(n_records)
    for d in range(8):
        rows[:, 9 - d] = ord("0") + (idx // 10 ** d) % 10
    rows[:, 11:11 + read_len] = as_array(b"ACGTN")[rng.integers(0, 5, (n_records, read_len))]
    rows[:, 11 + read_len] = 10
    rows[:, 12 + read_len:14 + read_len] = as_array(b"+\n")
    rows[:, 14 + read_len:14 + 2 * read_len] = as_array(b"@+FI#")[rng.integers(0, 5, (n_records, read_len))]
    rows[:, width - 1] = 10
    return rows.reshape(-1)


def test_40_mb_in_16_mb_blocks(rig, model):
    arr = big_fastq(133_000)
    assert 40e6 < arr.size < 48 << 20
    rig.upload(arr)
    pos, records, blocks = 0, 0, 0
    while pos < arr.size:
        n = min(16 << 20, arr.size - pos)
        got, written = rig.frame(16 << 20, pos, n)
        want, want_bytes = model(arr[pos:pos + n])
        check(got, written, want, want_bytes, pos)
        assert got["flags"] == 0
        pos += got["consumed"]
        records += got["records"]
        blocks += 1
    assert records == 133_000 and blocks == 3


def test_a_block_of_newlines_only(rig, model):
    """the worst case the scratch is sized for: a newline at every byte, a quarter as many records"""
    n = 16 << 20
    arr = np.full(n, 10, dtype=np.uint8)
    rig.upload(arr)
    got, written = rig.frame(n, 0, n)
    assert got == dict(consumed=0, out_bytes=0, records=0, bases=0, flags=hast_amd.SQ_NOT_FOUR_LINE, first_bad=0), got
    assert (written == CANARY).all()
    assert got == model(arr)[0]


def test_framed_stream_counts_to_the_parsers_table(rig, tmp_path):
    """s00_trio_k21/p1.fq: framed on the device and counted where it lies == parsed on the host and counted through the staging"""
    path = os.path.join(GOLDEN, "s00_trio_k21", "p1.fq")
    parsed = subprocess.run([sc.build_parser_driver(tmp_path), path], stdout=subprocess.PIPE, check=True).stdout
    arr = as_array(open(path, "rb").read())
    tables = []
    for device in (True, False):
        with KmerCounter(21, table_bytes=64 << 20) as kc:
            if device:
                d_in, d_out = rig.ctx.to_device(arr), rig.ctx.alloc(arr.size + 64)
                with SqFramer(kc, arr.size) as sq:
                    res = sq.frame_device(d_in, arr.size, d_out, arr.size)
                    assert res.flags == 0 and res.consumed == arr.size and res.out_bytes == len(parsed)
                    kc.count_device(0, d_out, res.out_bytes)
                    kc.sync()
                assert rig.ctx.to_host(d_out, (res.out_bytes,), np.uint8).tobytes() == parsed
            else:
                kc.count(0, as_array(parsed))
                kc.sync()
            histo, stats = kc.histo(0), kc.stats()
            n = kc.select(0, 2, 1000)
            kc.release_table()
            assert kc.selection_sort(0) == n and n > 0
            tables.append((histo, stats["distinct"], stats["total"], kc.selection_text(0, 0, n)))
            if device:
                rig.ctx.free(d_in)
                rig.ctx.free(d_out)
    assert np.array_equal(tables[0][0], tables[1][0]) and tables[0][1:] == tables[1][1:]


# ---- hast_sq_feed with host and device blocks in turn ----------------------------------------------------------------------------
def feed_files():
    """three small inputs: reads long enough for windows of 11 in records that fit a block of 64, '\\r\\n' without the last line
    break, and records of up to 340 bytes, which blocks of 64 and 100 cannot hold (HAST_SQ_TAIL_TOO_LONG)"""
    corpus = {name: data for name, data, _ in sc.valid_corpus()}
    return {"reads24": sc.fastq(31, 260, (24, 0, 13, 23, 1), b"\n"), "crlf20_nonl": sc.fastq(32, 200, (20, 11, 12), b"\r\n", False),
            "n65_b2_nonl": corpus["n65_b2_nonl"]}


def table_of(kc):
    kc.sync()
    histo, stats = kc.histo(0), kc.stats()
    n = kc.select(0, 1, 1000)
    kc.release_table()
    assert n == 0 or kc.selection_sort(0) == n
    return histo.tolist(), stats["distinct"], stats["total"], kc.selection_text(0, 0, n) if n else b""


def feed_model(model, data, block):
    """the feed restated on the host over the framer's model: (base stream, tail, None), or (base stream so far, None, i) where view i
    leaves more than a block"""
    carried, stream = b"", []
    for i, at in enumerate(range(0, len(data), block)):
        view = carried + data[at:at + block]
        res, out = model(as_array(view))
        assert not res["flags"] & hast_amd.SQ_NOT_FOUR_LINE
        if len(view) - res["consumed"] > block:
            return b"".join(stream), None, i
        stream.append(out.tobytes())
        carried = view[res["consumed"]:]
    return b"".join(stream), carried, None


def run_feed(ctx, data, block, mixed):
    """(table, tail, None) or (table so far, None, the view that left too much); mixed: every block with i % 3 == 1 is written into
    the feed's device block; the feed is always one block ahead of the framer"""
    blocks = [data[at:at + block] for at in range(0, len(data), block)]
    with KmerCounter(11, table_bytes=64 << 20) as kc:
        with SqFeed(kc, block) as feed:
            def submit(i):
                feed.submit(blocks[i], device=ctx if mixed and i % 3 == 1 else None)
            submit(0)
            for i in range(len(blocks)):
                if i + 1 < len(blocks):
                    submit(i + 1)
                res = feed.next(0)
                if res.flags & hast_amd.SQ_TAIL_TOO_LONG:
                    return table_of(kc), None, i
                assert res.flags & ~hast_amd.SQ_NO_RECORD == 0, (i, res.flags)
            return table_of(kc), feed.take_tail(), None


@pytest.mark.parametrize("block", (64, 100, 4096))
@pytest.mark.parametrize("name", sorted(feed_files()))
def test_feed_with_device_blocks_equals_host_blocks_and_the_model(rig, model, name, block):
    data = feed_files()[name]
    assert 1000 < len(data) < 20000
    stream, want_tail, want_stop = feed_model(model, data, block)
    assert (want_stop is not None) == (name == "n65_b2_nonl" and block < 4096)
    with KmerCounter(11, table_bytes=64 << 20) as kc:
        if stream:
            kc.count(0, as_array(stream))
        want = table_of(kc)
    assert want_stop is not None or (want[2][0] > 0 and len(data) > 2 * block)
    for mixed in (True, False):
        got, tail, stop = run_feed(rig.ctx, data, block, mixed)
        assert (tail, stop) == (want_tail, want_stop), (name, block, mixed)
        assert got == want, (name, block, mixed)
