"""GPU test of the stage-00 device framer for FASTA (hast_sq_frame_fasta_device, hast_amd/csrc/sq_fasta_kernels.hip) and of FASTA
through the feed (hast_sq_feed_set_formats / _next / _finish): every field of a view's result and every byte written equal the host
model's (tests/native/test_sq_fasta.cpp, which steps the same sq_core.h and is held to the host parser by tests/test_sq_fasta_cpu.py),
at every view size, alignment, cut and open state; nothing is written behind out_bytes; and the feed's table is the table counted from
the parser's stream.

The golden inputs and the feed's smallest blocks: tests/golden/s00_fasta_k11/p.fa has lines of up to 266 bytes and p_crlf.fa, beside
its 7-column CRLF lines, four of 154 to 303, so at blocks of 64 and 100 bytes both hold a line longer than a block and the feed answers
HAST_SQ_TAIL_TOO_LONG, as include/hast.h says it must.  That answer is asserted for them; the table comparison at 64 and 100 runs on
the same two files folded to 7 columns (the same records and therefore the same stream and table), and at 4096 on the files as they
are."""
import ctypes as C
import os

import numpy as np
import pytest

import hast_amd
from hast_amd import KmerCounter, SqFeed, SqFramer, SqResult, SQ_FA_LAST, SQ_FA_OPEN
from tests import sq_fasta_corpus as fc
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
CANARY, PAD = 0xEE, 64
FIELDS = ("consumed", "out_bytes", "records", "bases", "flags", "first_bad")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = C.CDLL(fc.build_model(tmp_path_factory.mktemp("sq_fasta_model"), shared=True))
    lib.sq_fasta_model_frame.restype = None
    lib.sq_fasta_model_frame.argtypes = [C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.POINTER(SqResult)]

    def frame(data: np.ndarray, flags):
        data = np.ascontiguousarray(data)
        out = np.zeros(data.size + 1, dtype=np.uint8)
        res = SqResult()
        lib.sq_fasta_model_frame(data.ctypes.data, data.size, flags, out.ctypes.data, C.byref(res))
        return {f: getattr(res, f) for f in FIELDS}, out[:res.out_bytes]
    return frame


class Rig:
    """a count table (the framer runs on its stream), a context for raw device memory, and two reusable device buffers"""

    def __init__(self, cap):
        self.ctx = hast_amd.Context(21)
        self.kc = KmerCounter(21, table_bytes=64 << 20)
        self.d_in = self.ctx.alloc(cap + 64)
        self.d_out = self.ctx.alloc(cap + 1 + PAD + 64)
        self.framers = {}

    def framer(self, max_in):
        if max_in not in self.framers:
            self.framers[max_in] = SqFramer(self.kc, max_in)
        return self.framers[max_in]

    def upload(self, data: np.ndarray, at=0):
        data = np.ascontiguousarray(data)
        hast_amd.lib().hast_memcpy_h2d(self.ctx._h, C.c_void_p(self.d_in + at), data.ctypes.data, data.size)

    def frame(self, max_in, in_at, n, flags, out_at=0):
        """frames d_in[in_at, in_at + n) into d_out + out_at; returns the result and d_out[out_at, out_at + n + 1 + PAD) as it stands after"""
        self.ctx.memset(self.d_out + out_at, CANARY, n + 1 + PAD)
        self.ctx.sync()
        res = self.framer(max_in).frame_fasta_device(self.d_in + in_at, n, self.d_out + out_at, n + 1, flags)
        return {f: getattr(res, f) for f in FIELDS}, self.ctx.to_host(self.d_out + out_at, (n + 1 + PAD,), np.uint8)

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
def test_corpus_view_by_view_equals_the_model(rig, model, max_in):
    """the input lies on the device once; a view is [pos, pos + max_in) and pos moves on by `consumed`: the carried bytes in front of the
    new ones, at whatever alignment that gives; a header seen opens the views behind it, the view that reaches the end is the last"""
    n_views = 0
    for name, files, longest in fc.corpus():
        if longest > max_in:
            continue
        arr = as_array(b"".join(files))
        rig.upload(arr)
        pos, opened = 0, False
        for _ in range(40):                              # (the first 40 views of an input say what the rest would)
            n = min(max_in, arr.size - pos)
            flags = (SQ_FA_OPEN if opened else 0) | (SQ_FA_LAST if pos + n == arr.size else 0)
            got, written = rig.frame(max_in, pos, n, flags)
            want, want_bytes = model(arr[pos:pos + n], flags)
            check(got, written, want, want_bytes, (name, max_in, pos))
            assert got["flags"] == 0 and (got["consumed"] > 0 or n == 0), (name, pos)
            n_views += 1
            opened = opened or got["records"] > 0
            pos += got["consumed"]
            if flags & SQ_FA_LAST:
                assert pos == arr.size
                break
    assert n_views > 50


def test_every_alignment_of_input_and_output(rig, model):
    inputs = [(fc.fasta(1, 9, 60, b"\n"), SQ_FA_LAST), (fc.fasta(2, 40, 7, b"\r\n", max_lines=5, last_newline=False), SQ_FA_LAST | SQ_FA_OPEN),
              (fc.fasta(3, 3, 4097, b"\r\r\n", max_lines=2), 0)]
    for i, (data, flags) in enumerate(inputs):
        arr = as_array(data)
        want, want_bytes = model(arr, flags)
        assert want["records"] > 0 and want["out_bytes"] > 100
        for a_in in range(16):
            rig.upload(arr, a_in)
            for a_out in range(16):
                got, written = rig.frame(65536, a_in, arr.size, flags, a_out)
                check(got, written, want, want_bytes, (i, a_in, a_out))


def test_every_cut_of_a_small_input(rig, model):
    """[0, s) first, then what it left + [s, end) as the last view: with the open state the first part leaves, the two streams together
    are the whole input's, for every s; with the other open state the second part still is the model's"""
    data = b">r0 x\r\nACGTACG\r\nTTGCA\r\n>r1\r\nNNACGTTGCAAC\r\n\r\n>r2 len=20\r\nGATTACAGATTACAGATTAC\r\nACGTTGCATG\r\nAC"
    arr = as_array(data)
    assert 80 <= arr.size <= 130
    whole, whole_bytes = model(arr, SQ_FA_LAST)
    assert whole["records"] == 3
    rig.upload(arr)
    nothing = 0
    for s in range(arr.size + 1):
        got1, w1 = rig.frame(700, 0, s, 0)
        want1, want1_bytes = model(arr[:s], 0)
        check(got1, w1, want1, want1_bytes, ("first", s))
        if b"\n" not in data[:s]:
            nothing += 1
            assert got1["consumed"] == 0 and got1["out_bytes"] == 0, s
        c, opened = got1["consumed"], got1["records"] > 0
        for open_in in (opened, not opened):
            flags = SQ_FA_LAST | (SQ_FA_OPEN if open_in else 0)
            got2, w2 = rig.frame(700, c, arr.size - c, flags)
            want2, want2_bytes = model(arr[c:], flags)
            check(got2, w2, want2, want2_bytes, ("second", s, open_in))
            if open_in == opened:
                both = np.concatenate([w1[:got1["out_bytes"]], w2[:got2["out_bytes"]]])
                assert np.array_equal(both, whole_bytes) and got1["records"] + got2["records"] == 3, s
    assert nothing >= 6


def test_an_empty_last_view(rig, model):
    """the end of an input that ended with a newline: one closing byte if a record is open, nothing if not"""
    for flags, n_out in ((SQ_FA_LAST | SQ_FA_OPEN, 1), (SQ_FA_LAST, 0), (SQ_FA_OPEN, 0), (0, 0)):
        got, written = rig.frame(700, 5, 0, flags, 3)
        assert got == dict(consumed=0, out_bytes=n_out, records=0, bases=0, flags=0, first_bad=0xFFFFFFFF), (flags, got)
        assert got == model(np.zeros(0, dtype=np.uint8), flags)[0]
        assert (written[:n_out] == 10).all() and (written[n_out:] == CANARY).all(), flags


def test_a_view_of_newlines_only(rig, model):
    """the most lines a view can have, one per byte: all of it consumed, nothing written"""
    n = 16 << 20
    arr = np.full(n, 10, dtype=np.uint8)
    rig.upload(arr)
    for flags in (0, SQ_FA_OPEN | SQ_FA_LAST):
        got, written = rig.frame(n, 0, n, flags)
        closing = 1 if flags else 0
        assert got == dict(consumed=n, out_bytes=closing, records=0, bases=0, flags=0, first_bad=0xFFFFFFFF), got
        assert (written[closing:] == CANARY).all() and got == model(arr, flags)[0]


def test_a_view_of_empty_headers_only(rig, model):
    """the most headers a view can have: every one but the input's first gives a separator"""
    n = 16 << 20
    arr = np.tile(as_array(b">\n"), n // 2)
    rig.upload(arr)
    for flags in (0, SQ_FA_OPEN):
        got, written = rig.frame(n, 0, n, flags)
        want, want_bytes = model(arr, flags)
        check(got, written, want, want_bytes, flags)
        assert got["records"] == n // 2 and got["out_bytes"] == n // 2 - (0 if flags else 1) and got["bases"] == 0
        assert (written[:got["out_bytes"]] == 10).all()


def folded(n_rows, width, seed):
    """n_rows lines of `width` bases, each with its '\\n'"""
    rng = np.random.default_rng(seed)
    rows = np.empty((n_rows, width + 1), dtype=np.uint8)
    rows[:, :width] = as_array(b"ACGTN")[rng.integers(0, 5, (n_rows, width))]
    rows[:, width] = 10
    return rows.reshape(-1)


def test_a_long_line_among_short_ones(rig, model):
    """one line of 1 MB inside a 16-MB view of 60-column lines: the copy is split by output bytes, not by lines"""
    parts = [as_array(b">chr1 folded\n"), folded(120_000, 60, 1), as_array(b">chr2 one line\r\n"), folded(1, 1 << 20, 2), as_array(b">chr3\n"),
             folded(140_000, 60, 3)]
    arr = np.concatenate(parts)
    arr = arr[:min(arr.size, (16 << 20) - 5)]             # (cut inside a line: not consumed)
    assert arr.size > 15 << 20
    rig.upload(arr, 3)
    got, written = rig.frame(16 << 20, 3, arr.size, 0, 7)
    want, want_bytes = model(arr, 0)
    check(got, written, want, want_bytes, "long line")
    assert got["records"] == 3 and got["bases"] > 15_000_000 and 0 < got["consumed"] < arr.size


def test_40_mb_in_16_mb_views(rig, model):
    n_records = 260_000
    rows = np.empty((n_records, 11 + 151), dtype=np.uint8)
    rows[:, :11] = as_array(b">r00000000\n")
    idx = np.arange(n_records)
    for d in range(8):
        rows[:, 9 - d] = ord("0") + (idx // 10 ** d) % 10
    rows[:, 11:] = folded(n_records, 150, 9).reshape(n_records, 151)
    arr = rows.reshape(-1)
    assert 40e6 < arr.size < 48 << 20
    rig.upload(arr)
    pos, records, bases, views, opened = 0, 0, 0, 0, False
    while True:
        n = min(16 << 20, arr.size - pos)
        flags = (SQ_FA_OPEN if opened else 0) | (SQ_FA_LAST if pos + n == arr.size else 0)
        got, written = rig.frame(16 << 20, pos, n, flags)
        want, want_bytes = model(arr[pos:pos + n], flags)
        check(got, written, want, want_bytes, pos)
        pos += got["consumed"]
        records += got["records"]
        bases += got["bases"]
        views += 1
        opened = True
        if flags & SQ_FA_LAST:
            break
    assert records == n_records and bases == 150 * n_records and views == 3 and pos == arr.size


# ---- the feed -------------------------------------------------------------------------------------------------------------------
def refold(data: bytes, width=7, brk=b"\r\n"):
    """the same records on `width`-column lines"""
    out = bytearray()
    for rec in data.split(b">")[1:]:
        header, _, rest = rec.partition(b"\n")
        seq = b"".join(l.rstrip(b"\r") for l in rest.split(b"\n"))
        out += b">" + header.rstrip(b"\r") + brk
        for at in range(0, len(seq), width):
            out += seq[at:at + width] + brk
    return bytes(out)


def feed_inputs():
    golden = {name: open(os.path.join(GOLDEN, "s00_fasta_k11", name), "rb").read() for name in ("p_crlf.fa", "p.fa")}
    inputs = dict(golden)
    inputs.update({name + ".7col": refold(data) for name, data in golden.items()})
    # long headers, no to two 7-column lines a record: most 64-byte views emit fewer bytes than K - 1
    inputs["headers"] = b"".join(b">record_%04d with a long description line\r\n" % i + b"ACGTTGA\r\n" * (i % 3) for i in range(90)) + b">end\nACGT"
    return inputs


def table_of(kc):
    kc.sync()
    histo, stats = kc.histo(0), kc.stats()
    n = kc.select(0, 1, 1000)
    kc.release_table()
    assert n == 0 or kc.selection_sort(0) == n
    return histo, stats["distinct"], stats["total"], kc.selection_text(0, 0, n) if n else b""


def same_table(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


@pytest.fixture(scope="module")
def parsed_tables(tmp_path_factory):
    """(input, K) -> the parser's stream and the table hast_kc_count makes of it, computed once"""
    d = tmp_path_factory.mktemp("sq_fasta_feed")
    driver = fc.build_parser_driver(d)
    out = {}
    for name, data in feed_inputs().items():
        stream = fc.parser_stream(driver, fc.write_case(d, name, [data]))
        for k in (11, 31):
            with KmerCounter(k, table_bytes=64 << 20) as kc:
                kc.count(0, as_array(stream))
                out[name, k] = (stream, table_of(kc))
    for name in ("p.fa", "p_crlf.fa"):
        for k in (11, 31):
            assert out[name, k][0] == out[name + ".7col", k][0] and same_table(out[name, k][1], out[name + ".7col", k][1])
    assert out["p_crlf.fa", 11][1][2][0] > 1000 and out["headers", 31][1][2][0] == 0  # (the headers input has no window of 31 at all)
    return out


@pytest.mark.parametrize("k", (11, 31))
@pytest.mark.parametrize("block", (64, 100, 4096))
@pytest.mark.parametrize("name", sorted(feed_inputs()))
def test_feed_counts_to_the_parsers_table(parsed_tables, name, block, k):
    data = feed_inputs()[name]
    stream, want = parsed_tables[name, k]
    fits = fc.longest_line([data]) <= block
    assert fits == (block == 4096 or name not in ("p.fa", "p_crlf.fa"))
    with KmerCounter(k, table_bytes=64 << 20) as kc:
        with SqFeed(kc, block, hast_amd.SQ_TAKE_FASTQ | hast_amd.SQ_TAKE_FASTA) as feed:
            assert feed.format == 0
            records = bases = out_bytes = short = views = 0
            too_long = False
            for at in range(0, len(data), block):
                feed.submit(data[at:at + block])
                res = feed.next(0)
                assert feed.format == 2
                if res.flags & hast_amd.SQ_TAIL_TOO_LONG:
                    too_long = True
                    break
                assert res.flags == 0
                views += 1
                short += res.out_bytes < k - 1
                records, bases, out_bytes = records + res.records, bases + res.bases, out_bytes + res.out_bytes
            assert too_long == (not fits), (name, block)
            if too_long:
                return
            res = feed.finish(0)
            assert res.flags == 0 and feed.format == 0
            records, bases, out_bytes = records + res.records, bases + res.bases, out_bytes + res.out_bytes
            assert (records, bases, out_bytes) == (data.count(b">"), len(stream) - stream.count(b"\n"), len(stream))
            if block == 64:
                assert views > 50
            if block == 64 and name == "headers":
                assert short > 10                            # the kept bytes lie in front of views that add fewer than K - 1 to them
            got = table_of(kc)
    assert same_table(got, want), (name, block, k)


def test_feed_api_misuse_and_fastq_through_a_feed_that_takes_both():
    both = hast_amd.SQ_TAKE_FASTQ | hast_amd.SQ_TAKE_FASTA
    fq = open(os.path.join(GOLDEN, "s00_trio_k21", "p1.fq"), "rb").read()[:4000]
    with KmerCounter(21, table_bytes=64 << 20) as kc:
        with SqFeed(kc, 4096) as feed:
            for mask in (0, hast_amd.SQ_TAKE_FASTA, 4, 7):
                with pytest.raises(hast_amd.HastError):
                    feed.set_formats(mask)
            feed.submit(b">a\nACGT\n>b\nAC\n")                # a feed that takes FASTQ only: FASTA is what it always was
            assert feed.next(0).flags & hast_amd.SQ_NOT_FOUR_LINE and feed.format == 1
            with pytest.raises(hast_amd.HastError):
                feed.finish(0)
        with SqFeed(kc, 4096, both) as feed:
            with pytest.raises(hast_amd.HastError):
                feed.finish(0)                               # undecided
            feed.submit(fq)
            with pytest.raises(hast_amd.HastError):
                feed.set_formats(hast_amd.SQ_TAKE_FASTQ)     # a block is submitted
            res = feed.next(0)
            assert res.flags == 0 and res.records > 5 and feed.format == 1
            with pytest.raises(hast_amd.HastError):
                feed.finish(0)                               # FASTQ ends through take_tail
            assert len(feed.take_tail()) == len(fq) - res.consumed and feed.format == 0
            feed.submit(b">a\nAC")                           # the next input decides anew
            assert feed.next(0).records == 1 and feed.format == 2
            res = feed.finish(0)
            assert (res.out_bytes, res.bases, res.records) == (3, 2, 0)
