"""The searched t-mer levels on the GPU: k_filter_build files every key under the block the level table's order samples
(tmer_order, the table in constant memory), k_classify_f probes under the block it samples from its 2-KB LDS copy
(tmer_order_lvl).  Each read is its own barcode, so the counts are per-read votes; they must equal the oracle's at the
K = 21 geometry of the benchmark (m = 14, exact entries) and at the overfull K = 15 / m = 8 one, and equal the exact table probed
directly (no filter)."""
import numpy as np
import pytest

import hast_amd
from hast_amd.binding import make_params
from tests.test_gpu_parity import built, oracle_counts, oracle_from_keys  # noqa: F401  (built: module fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("k,fm,n_keys", [(21, 14, 200_000), (15, 8, 150_000)])   # C3's geometry (m = 14, t = 6, kp = 21); overfull
def test_per_read_votes_vs_oracle(built, oracle_lib, k, fm, n_keys):
    L, n_reads = 150, 20000
    p = make_params(k, L, n_keys, n_reads)
    keys = [hast_amd.synth_keys_host(p, h, 0, n_keys) for h in (0, 1)]
    bases, _ = hast_amd.synth_reads_host(p, 5, n_reads)
    ids = np.arange(n_reads, dtype=np.uint32)                 # one barcode per read: the counts are per-read votes
    off = np.arange(n_reads + 1, dtype=np.uint64) * L
    oc = oracle_from_keys(oracle_lib, k, keys[0], keys[1])
    want = oracle_counts(oracle_lib, oc, bases, off, ids, n_reads)
    oracle_lib.ho_free(oc)
    assert int(want[0].sum()) > 0 and int(want[1].sum()) > 0
    for enable in (1, 0):                       # the filter / the exact table directly
        with hast_amd.Context(k) as ctx:
            ctx.set_filter(enable, fm if enable else 0)
            ctx.table_reserve(2 * n_keys)
            ctx.table_insert_keys(0, keys[0])
            ctx.table_insert_keys(1, keys[1])
            ctx.counts_resize(n_reads)
            d_b, d_i = ctx.to_device(bases), ctx.to_device(ids)
            ctx.counts_zero()
            ctx.classify_device(d_b, bases.size, n_reads, L, d_barcode_ids=d_i)
            if enable:
                assert ctx.filter_mode() == 2 and ctx.filter_info()[1] == fm      # exact entries, the geometry under test
            for a, b in zip(ctx.counts_read(n_reads), want):
                assert np.array_equal(a, b), (k, enable)
