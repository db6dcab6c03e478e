"""GPU tests of the shared record gather (hast_amd/csrc/record_gather.h: k_route_copy, k_rs_names, k_sq_copy) and of the shared newline
index kernels (nl_kernels.hip: k_nl_count, k_nl_index), each family through its public API against the host model its own tests use.

What the gather is asked: 1, 64, 65, 256 and 257 records (one, a whole wave, one more, a whole tile, one more), and gathered fields of 0
(where the format has one), 63, 64 and 65 bytes -- the 64 bytes a wave moves a step, one less, one more.
  routing   the field is the whole record: test_routed_records_at_the_wave_and_tile_borders
  rs        the field is the read name (a FASTA header of '>' alone and a FASTQ header of '@' alone name a read ""):
            test_read_names_at_the_wave_and_tile_borders; tests/rs_corpus.py has 0, 1, 255, 256 and 257 records and the bare header
            (fa_bare), not 64 or 65 records and no name of 63 to 65 bytes
  sq        the field is the sequence: tests/sq_corpus.py (COUNTS 0, 1, 63, 64, 65, 255, 256, 257, 1000 x READ_LENS 0, 1, 63, 64, 65, 150,
            4097) already runs all of it through tests/test_sq_gpu.py::test_corpus_block_by_block_equals_the_model; nothing is added here

What the newline kernels are asked: ranges of 1, 15, 16, 17, 4095, 4096 and 4097 bytes (a 16-byte piece and a 4-KB tile, one less, one
more) that start 0, 1 and 15 bytes past a 16-byte boundary, with newlines right in front of them and behind them that must not count.
One range a launch through the stage-00 framers (FASTQ and FASTA), two through the stLFR conversion, the sides of different lengths and
alignments.  The read stream (rs) launches the same two kernels on a range built by the same helper; its views start wherever the bytes
carried from the view before put them, which tests/test_rs_gpu.py runs at blocks of 64 to 65536 bytes."""
import ctypes as C
import random

import numpy as np
import pytest

import hast_amd
from hast_amd import ReadStream, SQ_FA_LAST
from tests import rs_corpus as rc
from tests import sq_corpus as sc
from tests import sq_fasta_corpus as fc
from tests import test_fq_gpu as fq_gpu
from tests import test_sq_fasta_gpu as sqfa_gpu
from tests import test_sq_gpu as sq_gpu
from tests import test_tx_gpu as tx_gpu

pytestmark = pytest.mark.gpu
COUNTS = (1, 64, 65, 256, 257)
FIELD_LENS = (63, 64, 65, 0, 1, 64, 150, 65, 63)       # taken in turn; no multiple of its length is 64, so every wave sees each of them
NL_SIZES = (1, 15, 16, 17, 4095, 4096, 4097)
NL_STARTS = (0, 1, 15)


# ---- routing: whole records -------------------------------------------------------------------------------------------------
def routed_record(i, total, barcode):
    """a four-line record of exactly `total` bytes whose header carries `barcode` (None: no field 2 at all)"""
    head = b"@r%d" % i + (b"" if barcode is None else b"#" + barcode + b"/1")
    rest = total - len(head) - 5                        # five line ends and the '+'
    assert rest >= 0
    head += b"x" * (rest % 2) if barcode is None else b""
    if barcode is not None and rest % 2:
        head = head[:-2] + b"/12"                       # (awk's field 2 ends at the '/')
    seq = rest // 2
    rec = head + b"\n" + (b"ACGT" * (seq // 4 + 1))[:seq] + b"\n+\n" + (b"FI:," * (seq // 4 + 1))[:seq] + b"\n"
    assert len(rec) == total, (len(rec), total)
    return rec


@pytest.mark.parametrize("n", COUNTS)
def test_routed_records_at_the_wave_and_tile_borders(n):
    cls_of = {b"1_2_%d" % j: 1 + j % 3 for j in range(30)}
    lens = [l for l in FIELD_LENS if l >= 32] + [300]
    barcodes = sorted(cls_of) + [b"0_0_0", None]
    data = b"".join(routed_record(i, lens[i % len(lens)], barcodes[(i * 7) % len(barcodes)]) for i in range(n))
    want, want_dropped = fq_gpu._awk_route(data, cls_of)
    block = 1 << 17
    assert len(data) <= block
    got, dropped, st = fq_gpu.route_through_abi(data, cls_of, block, block, 1, random.Random(n))
    assert dropped == [] == want_dropped and st == {"host_blocks": 0, "blocks": 1}          # the device routed every record itself
    for c in range(4):
        assert got[c] == want[c], (n, c, len(got[c]), len(want[c]))
    assert sum(g.count(b"\n") for g in got) == 4 * n
    assert all(want) or n < 64                           # every class has its run


# ---- rs: read names -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rs_ctx():
    ctx = hast_amd.Context(21)
    ctx.table_reserve(4)
    for hap, key in enumerate((b"ACGTACGTACGTACGTACGTA", b"TTGCATTGCATTGCATTGCAT")):
        assert ctx.table_insert_text(hap, key + b"\n") == 1
    yield ctx
    ctx.close()


def name_of_length(i, length):
    return (b"%d|" % i + b"n" * length)[:length]


@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
@pytest.mark.parametrize("n", COUNTS)
def test_read_names_at_the_wave_and_tile_borders(rs_ctx, n, fmt):
    recs = [(name_of_length(i, FIELD_LENS[i % len(FIELD_LENS)]), b"ACGTTGCA" * (1 + i % 5)) for i in range(n)]
    data = rc.fasta_text(random.Random(0), recs, 60) if fmt == rc.FASTA else rc.fastq_text(recs)
    want = rc.read_file(fmt, data)
    assert [w[0] for w in want] == [r[0] for r in recs] and {len(r[0]) for r in recs} >= set(FIELD_LENS[:min(n, 9)])
    names, flags = [], 0
    with ReadStream(rs_ctx, fmt, 1 << 17) as feed:
        feed.submit(data, device=True)
        feed.submit(b"", last=True)
        for _ in range(2):
            fl, _, _, nm, votes = feed.next()
            flags |= fl
            names.extend(nm)
            assert votes.shape == (len(nm), 2)
    assert flags == 0 and names == [w[0] for w in want], (n, fmt)


# ---- the newline kernels: one range a launch ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sq_rig():
    r = sq_gpu.Rig(1 << 16)
    yield r
    r.close()


@pytest.fixture(scope="module")
def sqfa_rig():
    r = sqfa_gpu.Rig(1 << 16)
    yield r
    r.close()


sq_model = sq_gpu.model
sqfa_model = sqfa_gpu.model
FENCE = np.full(32, 10, dtype=np.uint8)                 # newlines in front of a range and behind it


def fenced(arr, start):
    """(what to upload at 0, where the range starts): the range `start` bytes past the second 16-byte boundary, newlines all round"""
    at = 16 + start
    return np.concatenate([FENCE[:at], arr, FENCE]), at


@pytest.mark.parametrize("start", NL_STARTS)
def test_one_sided_fastq_ranges(sq_rig, sq_model, start):
    text = sq_gpu.as_array(sc.fastq(11, 400, (3, 0, 1, 9), b"\n"))
    assert text.size > NL_SIZES[-1]
    records = 0
    for n in NL_SIZES:
        arr = text[:n]
        buf, at = fenced(arr, start)
        sq_rig.upload(buf)
        got, written = sq_rig.frame(8192, at, n, 3)
        want, want_bytes = sq_model(arr)
        sq_gpu.check(got, written, want, want_bytes, (n, start))
        records += got["records"]
    assert records > 3 * 150                             # the three long ranges hold whole records, each counted to the last one


@pytest.mark.parametrize("start", NL_STARTS)
def test_one_sided_fasta_ranges(sqfa_rig, sqfa_model, start):
    text = sqfa_gpu.as_array(fc.fasta(5, 200, 7, b"\n", max_lines=9))
    assert text.size > NL_SIZES[-1]
    records = 0
    for n in NL_SIZES:
        arr = text[:n]
        buf, at = fenced(arr, start)
        sqfa_rig.upload(buf)
        got, written = sqfa_rig.frame(8192, at, n, SQ_FA_LAST, 5)
        want, want_bytes = sqfa_model(arr, SQ_FA_LAST)
        sqfa_gpu.check(got, written, want, want_bytes, (n, start))
        records += got["records"]
    assert records > 3 * 30


# ---- the newline kernels: two ranges a launch ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tx_rig():
    r = tx_gpu.Rig()
    yield r
    r.close()


@pytest.mark.parametrize("start1", NL_STARTS)
@pytest.mark.parametrize("start0", NL_STARTS)
def test_two_sided_ranges(tx_rig, start0, start1):
    """side 0 of every size against side 1 of the size three places on: the shorter side is now the first, now the second, and the
    launch's tile count is the longer one's; then the three long sizes against each other, where whole tiles of pairs come out"""
    r1, r2 = tx_gpu.records(200), tx_gpu.records(200, side=2, seq=lambda i: (i * 11) % 30 + 1)
    assert min(len(r1), len(r2)) > NL_SIZES[-1]
    fence = np.frombuffer(b"\n@x#k\n" * 8, dtype=np.uint8)
    pairs = 0
    sizes = [(n0, NL_SIZES[(i + 3) % len(NL_SIZES)]) for i, n0 in enumerate(NL_SIZES)] + [(4095, 4097), (4097, 4096), (4096, 4095)]
    for n0, n1 in sizes:
        in_at = (16 + start0, 16 + start1)
        for s, n in enumerate((n0, n1)):
            tx_rig.lib.hast_memcpy_h2d(tx_rig.ctx._h, C.c_void_p(tx_rig.d_in[s]), fence.ctypes.data, 32)
            tx_rig.lib.hast_memcpy_h2d(tx_rig.ctx._h, C.c_void_p(tx_rig.d_in[s] + in_at[s] + n), fence.ctypes.data, fence.size)
        _, _, res = tx_rig.run(tx_gpu.MAP, r1[:n0], r2[:n1], in_at=in_at)             # (compares every field and byte with the host's)
        assert tuple(res.lines) == (r1[:n0].count(b"\n"), r2[:n1].count(b"\n"))
        pairs += res.pairs
    assert pairs > 3 * 50
