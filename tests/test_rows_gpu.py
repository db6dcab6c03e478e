"""The output table made on the GPU (include/hast.h hast_rows_*, hast_amd/csrc/rows_kernels.hip) through the C ABI, on raw device
pointers (the context's allocator, as the other ABI tests of this suite: what a torch tensor's data_ptr() is to the library): for every case of tests/rows_corpus.py the table, the three lists, the list of every id, the order, any_sep, past_int and the sizes
are those of the independent model of tests/rows_model.py, byte for byte; hast_rows_read at odd offsets and lengths, across the
borders of its staging pieces."""
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
