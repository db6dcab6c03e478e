"""An overfull exact-entry filter on the GPU (K = 15, m = 8: 4^8 blocks for 600k filed strings; tests/native/test_tmer_order.cpp
counts thousands of sub-buckets that hold exactly 8 entries and thousands that turned one away and carry the overflow mark).
A window that lands in a full sub-bucket without a match goes to the exact table only when the mark is there: classification
must still equal the oracle and the exact table probed directly, before and after an erase (which rebuilds the filter)."""
import numpy as np
import pytest

import hast_amd
from hast_amd.binding import make_params
from tests.test_gpu_parity import built, oracle_counts, oracle_from_keys  # noqa: F401  (built: module fixture)


@pytest.mark.gpu
def test_overfull_exact_filter_vs_oracle_and_exact_table(built, oracle_lib):
    k, fm, L, n_keys, n_bc, n_reads = 15, 8, 150, 150_000, 64, 20000
    p = make_params(k, L, n_keys, n_bc)
    keys = [hast_amd.synth_keys_host(p, h, 0, n_keys) for h in (0, 1)]
    bases, ids = hast_amd.synth_reads_host(p, 3, n_reads)
    off = np.arange(n_reads + 1, dtype=np.uint64) * L

    def expect(k0, k1):
        oc = oracle_from_keys(oracle_lib, k, k0, k1)
        r = oracle_counts(oracle_lib, oc, bases, off, ids, n_bc)
        oracle_lib.ho_free(oc)
        return r

    gone = np.concatenate([keys[0][::3], keys[1][1::5]])
    want = [expect(keys[0], keys[1]), expect(keys[0][~np.isin(keys[0], gone)], keys[1][~np.isin(keys[1], gone)])]
    assert int(want[0][0].sum()) > 0 and int(want[0][1].sum()) > 0
    for enable in (1, 0):                       # the filter with exact entries / the table directly
        with hast_amd.Context(k) as ctx:
            ctx.set_filter(enable, fm if enable else 0)
            ctx.table_reserve(2 * n_keys)
            ctx.table_insert_keys(0, keys[0])
            ctx.table_insert_keys(1, keys[1])
            ctx.counts_resize(n_bc)
            d_b, d_i = ctx.to_device(bases), ctx.to_device(ids)
            for step in range(2):
                if step:
                    ctx.table_erase(gone)
                ctx.counts_zero()
                ctx.classify_device(d_b, bases.size, n_reads, L, d_barcode_ids=d_i)
                assert ctx.filter_mode() == (2 if enable else 0)
                if enable:
                    assert ctx.filter_info()[1] == fm
                for a, b in zip(ctx.counts_read(n_bc), want[step]):
                    assert np.array_equal(a, b), (enable, step)
