"""The dense filter's position sub-buckets and signed marks on the GPU (hast_common.h: filter_dense_code, filter_mark_sig,
filter_dense_file): the dense filter and the table-only kernel (HAST_CLASSIFY=exact) against the oracle, per-barcode counters
and per-read votes, where sub-buckets overflow -- K = 15 at m = 8 with 49 000 keys per haplotype (2.99 entries per sub-bucket,
some 2000 marks), random and clustered keys.  A host model of the filing (the layout only: which (string, position) pairs share a
sub-bucket) says which sub-buckets receive more than 8 entries; whatever order the build kernel files them in, slot 7 of such a
sub-bucket becomes a mark and all but 7 of its entries are turned away, so reads that show ALL of its strings at their grid positions
must send at least that many windows to the table, and every one of them must still be counted."""
import random

import numpy as np
import pytest

import hast_amd
from hast_amd.binding import make_params
from tests.test_gpu_parity import built, oracle_counts, oracle_from_keys, oracle_votes, ragged_reads  # noqa: F401  (built: module fixture)

U = np.uint64


def _revcomp(x, k):
    x = x ^ U(0xAAAAAAAAAAAAAAAA)
    for sh, mask in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x & U(mask)) << U(sh)) | ((x >> U(sh)) & U(mask))
    x = (x << U(32)) | (x >> U(32))
    return x >> U(64 - 2 * k)


def _dense_layout(strings, k, m):
    """every (string, pm) a dense build files for these strands: string, pm, sub-bucket index (block * 8 + sub-bucket), stored bits
    -- W = 8 only (the sub-bucket is pm, the stored bits are the 14 flank bits, rotated)"""
    assert k - m == 7
    out = []
    for pm in range(8):
        mm = (strings >> U(2 * (k - m - pm))) & U((1 << (2 * m)) - 1)
        blk = (mm ^ (mm >> U(m))) & U((1 << (2 * m)) - 1)
        rest = ((strings << U(2 * pm)) | (strings >> U(2 * (k - pm)))) & U(0x3FFF)
        out.append((strings, np.full(strings.size, pm), blk * U(8) + U(pm), rest))
    return [np.concatenate([o[i] for o in out]) for i in range(4)]


def _turned_away_plants(keys, k, m, L, rng, max_subs):
    """reads that show, each at a position whose grid m-mer is the filed one, ALL strings of up to max_subs sub-buckets that
    receive 9 or more entries -> (reads, the least number of windows the kernel must look up in the table)"""
    canon = np.unique(np.concatenate(keys))
    rc = _revcomp(canon, k)
    strands = np.concatenate([canon, rc[rc != canon]])
    s, pm, sub, rest = _dense_layout(strands, k, m)
    order = np.argsort(sub, kind="stable")
    s, pm, sub, rest = s[order], pm[order], sub[order], rest[order]
    uniq, start, count = np.unique(sub, return_index=True, return_counts=True)
    full = np.nonzero(count >= 9)[0]
    assert full.size > 500, full.size                      # the load the set-up is there for
    reads, least = [], 0
    for j in full[:max_subs]:
        least += int(count[j]) - 7
        for i in range(int(start[j]), int(start[j] + count[j])):
            p = (7 - int(pm[i])) + 8 * rng.randrange((L - k - 7) // 8)
            km = "".join("ACTG"[(int(s[i]) >> (2 * (k - 1 - b))) & 3] for b in range(k))
            r = [rng.choice("ACGT") for _ in range(L)]
            r[p:p + k] = km
            reads.append("".join(r).encode())
    return reads, least


def _run(monkeypatch, mode, k, fm, keys, bases, off, ids, n_bc, fixed_len):
    monkeypatch.delenv("HAST_FILTER_EXACT", raising=False)
    monkeypatch.delenv("HAST_CLASSIFY", raising=False)
    monkeypatch.setenv("HAST_COUNT_LOOKUPS", "1")
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
            ctx.classify_device(d_b, bases.size, n, int((off[1:] - off[:-1]).max()), d_offsets=ctx.to_device(off), d_barcode_ids=d_i, d_votes=d_v)
        ctx.sync()
        counts = ctx.counts_read(n_bc)
        votes = ctx.to_host(d_v, (n, 2), np.uint32)
        assert "count_lookups=1" in ctx.options().split()
        lookups = ctx.filter_lookups()
        if mode == "dense":
            assert ctx.filter_mode() == 2 and ctx.filter_info()[1] == fm and ctx.filter_dense()
        else:
            assert ctx.filter_mode() == 0 and lookups == 0          # (the table-only kernel has no filter to be sent on by)
    return counts, votes, lookups


def _compare(monkeypatch, oracle_lib, k, fm, keys, bases, off, ids, n_bc, fixed_len):
    """-> the oracle's votes and the dense filter's look-up count, after both kernels gave the oracle's counters and votes"""
    oc = oracle_from_keys(oracle_lib, k, keys[0], keys[1])
    want_counts = oracle_counts(oracle_lib, oc, bases, off, ids, n_bc)
    want_votes = oracle_votes(oracle_lib, oc, bases, off)
    oracle_lib.ho_free(oc)
    assert int(want_votes[:, 0].sum()) > 0 and int(want_votes[:, 1].sum()) > 0
    lookups = None
    for mode in ("dense", "table"):
        counts, votes, lk = _run(monkeypatch, mode, k, fm, keys, bases, off, ids, n_bc, fixed_len)
        assert np.array_equal(votes, want_votes), (mode, int((votes != want_votes).any(axis=1).sum()))
        for got, want in zip(counts, want_counts):
            assert np.array_equal(got, want), mode
        if mode == "dense":
            lookups = lk
    return want_votes, lookups


_SETUP = {}


def _setup(clustered):
    """K = 15 / m = 8, 49 000 keys per haplotype: made once per kind of keys"""
    if clustered not in _SETUP:
        k, n_keys, n_bc = 15, 49_000, 97
        p = make_params(k, 150, n_keys, n_bc, clustered=clustered)
        _SETUP[clustered] = (p, [hast_amd.synth_keys_host(p, h, 0, n_keys) for h in (0, 1)])
    return _SETUP[clustered]


@pytest.mark.gpu
@pytest.mark.parametrize("clustered", [False, True])
def test_lookups_happen_and_find_turned_away_keys(built, oracle_lib, monkeypatch, clustered):
    k, fm, L, n_bc, n_reads = 15, 8, 150, 97, 30000
    p, keys = _setup(clustered)
    rng = random.Random(5 + clustered)
    bases, ids = hast_amd.synth_reads_host(p, 3, n_reads)
    plants, least = _turned_away_plants(keys, k, fm, L, rng, 150)
    assert least >= 300 and len(plants) >= 9 * 150
    bases = np.concatenate([bases, np.frombuffer(b"".join(plants), dtype=np.uint8)])
    ids = np.concatenate([ids, np.array([rng.randrange(n_bc) for _ in plants], dtype=np.uint32)])
    n = n_reads + len(plants)
    off = np.arange(n + 1, dtype=np.uint64) * L
    want_votes, lookups = _compare(monkeypatch, oracle_lib, k, fm, keys, bases, off, ids, n_bc, L)
    # every planted read shows a key (so the turned-away ones among them were found in the table: the votes are the oracle's) ...
    assert (want_votes[n_reads:].sum(axis=1) >= 1).all()
    # ... and at least the entries those sub-buckets cannot hold went through the table; nowhere near every window did
    print("look-ups: %d (at least %d forced by %d planted reads), %.3f per read" % (lookups, least, len(plants), lookups / n))
    assert least <= lookups < n * (L - k + 1) // 20


@pytest.mark.gpu
@pytest.mark.parametrize("clustered", [False, True])
def test_ragged_reads_over_marked_sub_buckets(built, oracle_lib, monkeypatch, clustered):
    k, fm, n_bc = 15, 8, 97
    _, keys = _setup(clustered)
    rng = random.Random(91 + clustered)
    seqs = ragged_reads(rng, k, np.concatenate(keys), 700, 2500)
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    assert lens.min() == 0 and (lens < k).sum() > 5 and lens.max() > 2000
    assert any(b"N" in s for s in seqs) and any(s and s.islower() for s in seqs)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    ids = np.array([rng.randrange(n_bc) for _ in seqs], dtype=np.uint32)
    _, lookups = _compare(monkeypatch, oracle_lib, k, fm, keys, bases, off, ids, n_bc, 0)
    assert lookups > 0


@pytest.mark.gpu
def test_every_mark_bit_set_by_300_keys_in_one_sub_bucket(built, oracle_lib, monkeypatch):
    """K = 21 / m = 14: 300 keys that share one 14-mer at position 3 and differ only in their flanks land in ONE sub-bucket, far
    past its 8 slots: its mark collects the bits of 293 or more entries (all 14, in all likelihood), and every one of the 300 is
    still counted, through the table."""
    k, fm, L, n_bc, n_keys, n_special, pm = 21, 14, 150, 31, 200_000, 300, 3
    rng = random.Random(300)
    p = make_params(k, L, (n_keys - n_special) // 2, n_bc)
    keys = [hast_amd.synth_keys_host(p, h, 0, (n_keys - n_special) // 2) for h in (0, 1)]
    mmer = rng.getrandbits(2 * fm)
    flanks = rng.sample(range(1 << (2 * (k - fm))), n_special)
    strings = [((f >> (2 * (k - fm - pm))) << (2 * (k - pm))) | (mmer << (2 * (k - fm - pm))) | (f & ((1 << (2 * (k - fm - pm))) - 1)) for f in flanks]
    special = np.array(strings, dtype=np.uint64)
    s, pms, sub, rest = _dense_layout(special, k, fm)
    assert np.unique(sub[pms == pm]).size == 1 and np.unique(rest[pms == pm]).size == n_special      # one sub-bucket, 300 entries
    canon = np.minimum(special, _revcomp(special, k))
    assert np.unique(canon).size == n_special and not np.isin(canon, np.concatenate(keys)).any()
    keys = [np.concatenate([keys[h], canon[h::2]]) for h in (0, 1)]
    bases, ids = hast_amd.synth_reads_host(p, 11, 5000)
    plants = []
    for x in strings:
        km = "".join("ACTG"[(x >> (2 * (k - 1 - b))) & 3] for b in range(k))
        r = [rng.choice("ACGT") for _ in range(L)]
        o = (7 - pm) + 8 * rng.randrange((L - k - 7) // 8)        # the window there is probed under the m-mer at position pm
        r[o:o + k] = km
        plants.append("".join(r).encode())
    bases = np.concatenate([bases, np.frombuffer(b"".join(plants), dtype=np.uint8)])
    ids = np.concatenate([ids, np.array([rng.randrange(n_bc) for _ in plants], dtype=np.uint32)])
    n = 5000 + n_special
    off = np.arange(n + 1, dtype=np.uint64) * L
    want_votes, lookups = _compare(monkeypatch, oracle_lib, k, fm, keys, bases, off, ids, n_bc, L)
    assert (want_votes[5000:].sum(axis=1) >= 1).all()              # every one of the 300 is counted (the kernels gave these votes)
    assert lookups >= n_special - 7
