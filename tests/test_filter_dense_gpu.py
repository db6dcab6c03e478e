"""Dense filing on the GPU: one table classified through the dense filter (exact entries under every m-mer, k_classify_f's
DENSE instantiations), through the sampled exact filter (HAST_FILTER_EXACT=once) and through the exact table alone
(HAST_CLASSIFY=exact) gives identical per-barcode counters and per-read votes, and those of the oracle: 150-bp rows at the
benchmark's geometry (the kernel with geometry and row length compiled in; one read in 200 holds an 'N'), ragged reads of 0 to a
few thousand bases (empty, shorter than K, 'N', lower case, IUPAC), and a K = 15 table at m = 8 loaded to a mean of 3 entries per
sub-bucket, where marked sub-buckets send windows to the table (phase V).  Which filter a context really built is read from
hast_filter_dense / hast_ctx_options, not inferred."""
import random

import numpy as np
import pytest

import hast_amd
from hast_amd.binding import make_params
from tests.test_gpu_parity import built, oracle_counts, oracle_from_keys, oracle_votes, ragged_reads  # noqa: F401  (built: module fixture)

MODES = ("dense", "once", "table")


def _classify(monkeypatch, mode, k, fm, keys, bases, off, lens_max, ids, n_bc, fixed_len):
    monkeypatch.delenv("HAST_FILTER_EXACT", raising=False)
    monkeypatch.delenv("HAST_CLASSIFY", raising=False)
    if mode == "once":
        monkeypatch.setenv("HAST_FILTER_EXACT", "once")
    if mode == "table":
        monkeypatch.setenv("HAST_CLASSIFY", "exact")
    n = ids.size
    with hast_amd.Context(k) as ctx:
        if mode != "table":
            ctx.set_filter(1, fm)
        ctx.table_reserve(keys[0].size + keys[1].size)
        ctx.table_insert_keys(0, keys[0])
        ctx.table_insert_keys(1, keys[1])
        ctx.counts_resize(n_bc)
        d_b, d_i, d_v = ctx.to_device(bases), ctx.to_device(ids), ctx.alloc(n * 8)
        if fixed_len:
            ctx.classify_device(d_b, bases.size, n, fixed_len, d_barcode_ids=d_i, d_votes=d_v)
        else:
            d_o = ctx.to_device(off)
            ctx.classify_device(d_b, bases.size, n, lens_max, d_offsets=d_o, d_barcode_ids=d_i, d_votes=d_v)
        ctx.sync()
        counts = ctx.counts_read(n_bc)
        votes = ctx.to_host(d_v, (n, 2), np.uint32)
        # the filter this context really built
        if mode == "dense":
            assert ctx.filter_mode() == 2 and ctx.filter_info()[1] == fm and ctx.filter_dense()
            assert "filter_exact" not in ctx.options()
        elif mode == "once":
            assert ctx.filter_mode() == 2 and ctx.filter_info()[1] == fm and not ctx.filter_dense()
            assert "filter_exact_once=1" in ctx.options().split()
        else:
            assert ctx.filter_mode() == 0 and not ctx.filter_dense()
    return counts, votes


def _compare(monkeypatch, oracle_lib, k, fm, keys, bases, off, ids, n_bc, fixed_len):
    oc = oracle_from_keys(oracle_lib, k, keys[0], keys[1])
    want_counts = oracle_counts(oracle_lib, oc, bases, off, ids, n_bc)
    want_votes = oracle_votes(oracle_lib, oc, bases, off)
    oracle_lib.ho_free(oc)
    assert int(want_votes[:, 0].sum()) > 0 and int(want_votes[:, 1].sum()) > 0
    lens_max = int((off[1:] - off[:-1]).max())
    for mode in MODES:
        counts, votes = _classify(monkeypatch, mode, k, fm, keys, bases, off, lens_max, ids, n_bc, fixed_len)
        assert np.array_equal(votes, want_votes), (mode, int((votes != want_votes).any(axis=1).sum()))
        for got, want in zip(counts, want_counts):
            assert np.array_equal(got, want), mode


@pytest.mark.gpu
@pytest.mark.parametrize("L", [150, 100, 137])     # row length compiled in (150, 100) / the geometry alone
def test_dense_vs_once_vs_table_fixed_rows(built, oracle_lib, monkeypatch, L):
    k, fm, n_keys, n_bc, n_reads = 21, 14, 200_000, 211, 20000
    p = make_params(k, L, n_keys, n_bc)
    keys = [hast_amd.synth_keys_host(p, h, 0, n_keys) for h in (0, 1)]
    bases, ids = hast_amd.synth_reads_host(p, 7, n_reads)
    assert (bases.reshape(n_reads, L) == ord("N")).any(axis=1).sum() > 20          # reads with 'N' are there
    off = np.arange(n_reads + 1, dtype=np.uint64) * L
    _compare(monkeypatch, oracle_lib, k, fm, keys, bases, off, ids, n_bc, L)


@pytest.mark.gpu
@pytest.mark.parametrize("k,fm,max_len,clustered", [(21, 14, 180, False), (21, 14, 3000, False), (15, 8, 2500, False), (21, 14, 1200, True)])
def test_dense_vs_once_vs_table_ragged_reads(built, oracle_lib, monkeypatch, k, fm, max_len, clustered):
    rng = random.Random(77 * k + max_len)
    n_keys, n_bc = 20000, 50
    p = make_params(k, 100, n_keys, n_bc, clustered=clustered)
    keys = [hast_amd.synth_keys_host(p, h, 0, n_keys) for h in (0, 1)]
    seqs = ragged_reads(rng, k, np.concatenate(keys), 4000 if max_len < 1000 else 700, max_len)
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    assert lens.min() == 0 and (lens < k).sum() > 5
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    ids = np.array([rng.randrange(n_bc) for _ in seqs], dtype=np.uint32)
    _compare(monkeypatch, oracle_lib, k, fm, keys, bases, off, ids, n_bc, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("clustered", [False, True])
def test_dense_filter_loaded_to_three_per_sub_bucket(built, oracle_lib, monkeypatch, clustered):
    """K = 15 at m = 8: 4^8 blocks x 8 sub-buckets; 98 000 keys x 2 strands x 8 m-mers = 2.99 entries per sub-bucket on average, the
    load of the benchmark's table (2.98).  A Poisson variable of that mean passes 8 in 0.4 % of the sub-buckets: some 2000 of them
    carry the overflow mark, and about one window in 260 without a match lands in one and is verified against the table."""
    k, fm, L, n_keys, n_bc, n_reads = 15, 8, 150, 49_000, 97, 30000
    p = make_params(k, L, n_keys, n_bc, clustered=clustered)
    keys = [hast_amd.synth_keys_host(p, h, 0, n_keys) for h in (0, 1)]
    bases, ids = hast_amd.synth_reads_host(p, 3, n_reads)
    off = np.arange(n_reads + 1, dtype=np.uint64) * L
    _compare(monkeypatch, oracle_lib, k, fm, keys, bases, off, ids, n_bc, L)
