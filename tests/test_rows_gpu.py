"""The output table made on the GPU (include/hast.h hast_rows_*, hast_amd/csrc/rows_kernels.hip) through the C ABI, on raw device
pointers (the context's allocator, as the other ABI tests of this suite: what a torch tensor's data_ptr() is to the library): for every case of tests/rows_corpus.py the table, the three lists, the list of every id, the order, any_sep, past_int and the sizes
are those of the independent model of tests/rows_model.py, byte for byte; hast_rows_read at odd offsets and lengths, across the
borders of its staging pieces.  The same for a table of a million rows (rows_corpus.big_case: past one pass of the capped grids, past
the size at which the library's radix sort leaves its merge sort, nine rounds of the scan with all four carries in use) and for tables of
whole tiles of one list at the edge of a scan round (rows_corpus.tile_case); tests/test_rows_caps_cpu.py holds those sizes to the
sources."""
import os

import numpy as np
import pytest

import hast_amd
from tests import rows_corpus as rc
from tests import rows_model as rm

pytestmark = pytest.mark.gpu

CASES = rc.cases()
STAGE = 8 << 20                                     # kStage of rows_api.cpp: a piece of hast_rows_read


@pytest.fixture(scope="module")
def ctx():
    if not os.path.exists(hast_amd.lib_path()):
        hast_amd.build()
    with hast_amd.Context(21) as c:
        yield c


class OnDevice:
    """the text records and the counters of a case in device memory"""

    def __init__(self, ctx, text, counts):
        self.ctx = ctx
        self.n = len(text)
        self.text = ctx.to_device(np.ascontiguousarray(text)) if self.n else 0
        self.counts = ctx.to_device(np.ascontiguousarray(counts)) if self.n else 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for p in (self.text, self.counts):
            if p:
                self.ctx.free(p)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_device_table_is_the_models(ctx, case):
    name, names, c0, c1, n0, n1, w0, w1 = case
    want = rm.build(names, c0, c1, n0, n1, w0, w1)
    n = len(names)
    with OnDevice(ctx, rc.text16(names), rc.counts4(c0, c1)) as dev, hast_amd.Rows(ctx, dev.text, dev.counts, n, n0, n1, w0, w1, with_lists=True) as rows:
        info = rows.info()
        assert info.n_rows == n and info.table_bytes == len(want.table), (info.table_bytes, len(want.table))
        assert list(info.list_bytes) == [len(x) for x in want.lists]
        assert (info.any_sep, info.past_int) == (int(want.any_sep), int(want.past_int))
        assert rows.read(0) == want.table
        for l in range(3):
            assert rows.read(l + 1) == want.lists[l], l
        assert rows.classes().tolist() == want.cls
        assert rows.order().tolist() == want.order
        # pieces at odd offsets and lengths
        for off, m in ((0, 1), (1, 60), (61, 1), (len(want.table) // 3, 4097), (max(0, len(want.table) - 7), 7)):
            m = min(m, len(want.table) - min(off, len(want.table)))
            if off <= len(want.table):
                assert rows.read(0, off, m) == want.table[off:off + m], (off, m)
        with pytest.raises(hast_amd.HastError):
            rows.read(0, len(want.table), 1)
        with pytest.raises(hast_amd.HastError):
            rows.read(4, 0, 0)
        # without the lists: the same table, no list text
        with hast_amd.Rows(ctx, dev.text, dev.counts, n, n0, n1, w0, w1, with_lists=False) as bare:
            assert bare.read(0) == want.table and list(bare.info().list_bytes) == [0, 0, 0]
            assert bare.classes().tolist() == want.cls


# ---- past one grid, past the library's merge sort, across the rounds of the scan ----------------------------------------------------
class Big:
    """a case of a million rows, its model and its arrays in device memory: made once, changed by nobody"""

    def __init__(self, ctx, case):
        self.name, self.names, c0, c1 = case[:4]
        self.weights = case[4:]
        self.n = len(self.names)
        self.want = rm.build(self.names, c0, c1, *self.weights)
        self.order = np.array(self.want.order, dtype=np.uint32)
        self.cls = np.array(self.want.cls, dtype=np.uint8)
        self.dev = OnDevice(ctx, rc.text16(self.names), rc.counts4(c0, c1))

    def rows(self, ctx, with_lists):
        return hast_amd.Rows(ctx, self.dev.text, self.dev.counts, self.n, *self.weights, with_lists=with_lists)


@pytest.fixture(scope="module")
def big(ctx):
    b = Big(ctx, rc.big_case())
    with b.dev:
        yield b


@pytest.fixture(scope="module", params=rc.TILE_SIZES)
def tiles(ctx, request):
    b = Big(ctx, rc.tile_case(request.param))
    with b.dev:
        yield b


def same_text(got, want, what, row_of_line=None):
    """got == want, without handing megabytes to an assert: the first offset that differs, the row (and so the tile of the sorted order,
    the walk of the tile loop and the round of the scan) it falls in, and 80 bytes around it from both sides"""
    same = len(got) == len(want) and got == want
    if same:
        return
    m = min(len(got), len(want))
    diff = np.flatnonzero(np.frombuffer(got, dtype=np.uint8, count=m) != np.frombuffer(want, dtype=np.uint8, count=m))
    at = int(diff[0]) if len(diff) else m
    line = want.count(b"\n", 0, at)                                             # (no text of the corpus holds a newline)
    row = line if row_of_line is None else int(row_of_line[line]) if line < len(row_of_line) else -1
    tile = row // rc.TILE
    pytest.fail("%s: %d bytes, the model has %d; %d bytes differ, the first at offset %d: line %d, row %d of the sorted order, tile %d (walk %d of its "
                "workgroup, scan round %d)\n got  %r\n want %r" % (what, len(got), len(want), len(diff), at, line, row, tile, tile // rc.GRID_CAP,
                                                                   tile // rc.SCAN_ROUND, got[max(0, at - 40):at + 40], want[max(0, at - 40):at + 40]))


def same_array(got, want, what):
    same = got.shape == want.shape and bool(np.array_equal(got, want))
    if same:
        return
    diff = np.flatnonzero(got != want) if got.shape == want.shape else np.zeros(0, dtype=np.int64)
    at = int(diff[0]) if len(diff) else -1
    pytest.fail("%s: shapes %s and %s; %d entries differ, the first at %d (tile %d): got %s, want %s" % (
        what, got.shape, want.shape, len(diff), at, at // rc.TILE, got[max(0, at - 4):at + 4].tolist(), want[max(0, at - 4):at + 4].tolist()))


def check_against_the_model(ctx, b):
    """sizes, flags, table, lists, classes and order with the lists; the same table and classes without them"""
    want = b.want
    cls_sorted = b.cls[b.order]
    with b.rows(ctx, True) as rows:
        info = rows.info()
        assert info.n_rows == b.n
        assert (info.table_bytes, list(info.list_bytes)) == (len(want.table), [len(x) for x in want.lists])
        assert (info.any_sep, info.past_int) == (int(want.any_sep), int(want.past_int))
        same_array(rows.order(), b.order, b.name + ": the order")
        same_array(rows.classes(), b.cls, b.name + ": the list of every id")
        same_text(rows.read(0), want.table, b.name + ": the table")
        for l in range(3):
            same_text(rows.read(l + 1), want.lists[l], b.name + ": list %d" % (l + 1), np.flatnonzero(cls_sorted == l + 1))
    with b.rows(ctx, False) as bare:
        info = bare.info()
        assert info.n_rows == b.n and info.table_bytes == len(want.table) and list(info.list_bytes) == [0, 0, 0]
        same_array(bare.classes(), b.cls, b.name + ", no lists: the list of every id")
        same_text(bare.read(0), want.table, b.name + ", no lists: the table")
        for l in range(3):
            assert bare.read(l + 1) == b""


def test_the_order_is_a_permutation_at_every_size(ctx, big):
    """before 28 MB of text are compared: every id once"""
    with big.rows(ctx, False) as rows:
        order = rows.order()
    assert order.shape == (big.n,)
    missing = np.flatnonzero(np.bincount(order[order < big.n], minlength=big.n) != 1)
    assert len(missing) == 0 and bool(np.array_equal(np.sort(order), np.arange(big.n, dtype=np.uint32))), \
        "%d ids are not once in the order, the first %s; %d entries are no id at all" % (len(missing), missing[:8].tolist(), int((order >= big.n).sum()))


def test_a_table_past_one_grid_and_past_the_merge_sort(ctx, big):
    """BIG_N rows: 2050 tiles (workgroups 0 and 1 of k_rows_tile_sums and k_rows_write walk their loop twice, k_rows_key and k_rows_gather
    three times), nine rounds of k_rows_scan with rows of every list in each, and two passes of the library's sort past its merge sort --
    the second must keep the first's order among the 440 000 rows that share a first key word"""
    with big.rows(ctx, False) as rows:
        n = rows.info().n_rows
    assert -(-n // rc.TILE) > rc.GRID_CAP and n > rc.SORT_MERGE_LIMIT and -(-n // 256) > 2 * rc.GRID_CAP and -(-n // rc.TILE) > 8 * rc.SCAN_ROUND
    check_against_the_model(ctx, big)


def test_list_offsets_across_scan_rounds(ctx, tiles):
    """256 and 257 tiles: whole tiles of one list (the staging of k_rows_write full: 512 rows of 61 bytes, 8192 bytes of lines that all go to
    list 3), a round of the scan that ends with the last tile, and one that leaves a second round of one tile of one row"""
    with tiles.rows(ctx, True) as rows:
        info = rows.info()
        assert -(-info.n_rows // rc.TILE) in (rc.SCAN_ROUND, rc.SCAN_ROUND + 1) and list(info.list_bytes) == [len(x) for x in tiles.want.lists]
    check_against_the_model(ctx, tiles)


def test_reads_across_the_staging_pieces(ctx):
    """a table longer than two staging pieces (every count 20 digits): reads that start in one piece and end in another"""
    n = 300000
    names = [b"%015d" % (i * 7919 % n) for i in range(n)]
    counts = np.full((n, 4), 2 ** 64 - 1, dtype=np.uint64)
    row = lambda i: b"%015d\t-1\t%d\t%d\n" % (i, 2 ** 64 - 1, 2 ** 64 - 1)          # equal weights, equal densities: no call
    assert len(row(0)) == 61
    with OnDevice(ctx, rc.text16(names), counts) as dev, hast_amd.Rows(ctx, dev.text, dev.counts, n, 5, 5, 1.0, 1.0, with_lists=False) as rows:
        total = rows.info().table_bytes
        assert total == 61 * n > 2 * STAGE
        for off, m in ((STAGE - 3, 7), (STAGE - 61, 2 * 61 + STAGE), (2 * STAGE - 1, 2), (1, total - 2), (0, total)):
            got = rows.read(0, off, m)
            r0, r1 = off // 61, (off + m + 60) // 61
            want = b"".join(row(i) for i in range(r0, r1))[off - 61 * r0:][:m]
            assert got == want, (off, m)
