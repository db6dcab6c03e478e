"""GPU tests (-m gpu) of the partitioned commit's internal path: with barcode ids and no votes buffer of the caller's the probe kernel
hands a read's votes to k_commit_partition as 8 + 8 bits (ClassifyArgs::votes16), a bin's two counters have a 128-byte line of their
own, and the scratch is filled once and cleans itself afterwards (hast_amd/csrc/commit_plan.h).  Every leg classifies the same reads
through classify_device and is held, counter by counter, to the atomic commit and to the oracle."""
import os

import numpy as np
import pytest

import hast_amd
from hast_amd.binding import make_params
from tests.test_gpu_parity import oracle_counts, oracle_from_keys

pytestmark = pytest.mark.gpu

K, L, N_KEYS, N_BC, N_READS, N_SMALL = 21, 150, 5000, 1000, 40_000, 5_000     # 1000 barcodes = 4 bins of 256; 40 000 reads = 2.4
HOT = 300                                                                      # partition workgroups of 16 384, the last one ragged
BORDER_IDS = (0, 1, 254, 255, 256, 257, 510, 511, 512, 513, 766, 767, 768, 769, 998, 999)
PARTITION, ATOMIC = 2, 1


def periodic_read(rng):
    """one 21-mer repeated: every one of the read's 130 windows is a rotation of it"""
    unit = rng.choice(np.frombuffer(b"ACGT", np.uint8), K)
    return np.tile(unit, L // K + 1)[:L]


@pytest.fixture(scope="module")
def world(oracle_lib):
    if not os.path.exists(hast_amd.lib_path()):
        hast_amd.build()
    rng = np.random.default_rng(2024)
    p = make_params(K, L, N_KEYS, N_BC)
    keys = [hast_amd.synth_keys_host(p, h, 0, N_KEYS) for h in (0, 1)]
    bases, ids = hast_amd.synth_reads_host(p, 3, N_READS)
    bases = bases.copy().reshape(N_READS, L)
    ids = ids.copy()
    # reads whose every window hits: one planted key repeated, for either haplotype (vote 130 = the most a 150-bp read gives; bit 7 set)
    full = [periodic_read(rng) for _ in (0, 1)]
    for h in (0, 1):
        planted = np.array(hast_amd.chop_read(full[h].tobytes(), K), dtype=np.uint64)
        assert planted.size == L - K + 1
        keys[h] = np.unique(np.concatenate([keys[h], planted]))
    assert not np.intersect1d(keys[0], keys[1]).size
    # one barcode owns half the reads: its bin overflows into the list in the long launches and fits in the short one, which must
    # therefore find the overflow length of the launch before it reset
    ids[rng.random(N_READS) < 0.5] = HOT
    # ids on both sides of every bin border, the first and the last id: in the first reads (so the short launch has them too), in the
    # ragged last workgroup, and each with a read of every kind below
    at = np.concatenate([np.arange(100, 100 + 4 * len(BORDER_IDS)), np.arange(N_READS - 4 * len(BORDER_IDS), N_READS)])
    ids[at] = np.tile(np.repeat(np.array(BORDER_IDS, dtype=np.uint32), 4), 2)
    for j, i in enumerate(at):
        if j % 4 == 0:
            bases[i] = full[0]
        elif j % 4 == 1:
            bases[i] = full[1]
        elif j % 4 == 2:
            bases[i, (7 * j) % L] = ord("N")                                     # a read with an N: vote row 0, neg counted
    for i in rng.choice(N_READS, 400, replace=False):                            # and the same kinds anywhere, the hot barcode included
        kind = i % 3
        if kind == 2:
            bases[i, i % L] = ord("N")
        else:
            bases[i] = full[kind]
    bases = np.ascontiguousarray(bases.reshape(-1))
    oc = oracle_from_keys(oracle_lib, K, keys[0], keys[1])
    off = np.arange(N_READS + 1, dtype=np.uint64) * L
    exp = [a.astype(np.uint64) for a in oracle_counts(oracle_lib, oc, bases, off, ids, N_BC)]
    exp_small = [a.astype(np.uint64) for a in oracle_counts(oracle_lib, oc, bases[:N_SMALL * L], off[:N_SMALL + 1], ids[:N_SMALL], N_BC)]
    oracle_lib.ho_free(oc)
    # the cases are really there
    assert int(exp[2].sum()) > 0 and int(exp[0].sum()) > 0 and int(exp[1].sum()) > 0
    assert int((ids == HOT).sum()) > N_READS // 4 + N_READS // 8 + 2048           # more than a bin holds (commit_plan.h: mean * 1.5 + 2048)
    for b in BORDER_IDS:
        assert int(exp[0][b]) >= 130 and int(exp[1][b]) >= 130 and int(exp[2][b]) >= 1, b
    return {"keys": keys, "bases": bases, "ids": ids, "exp": exp, "exp_small": exp_small}


@pytest.fixture()
def ctx(world):
    with hast_amd.Context(K) as c:
        c.table_reserve(2 * (N_KEYS + L))
        c.table_insert_keys(0, world["keys"][0])
        c.table_insert_keys(1, world["keys"][1])
        c.counts_resize(N_BC)
        c.d_b, c.d_i = c.to_device(world["bases"]), c.to_device(world["ids"])
        yield c


def classify(c, world, n):
    c.classify_device(c.d_b, n * L, n, L, d_barcode_ids=c.d_i)


def equal(got, exp, what):
    for name, a, b in zip(("c0", "c1", "neg"), got, exp):
        bad = np.flatnonzero(a != b)
        assert not bad.size, (what, name, bad[:8], a[bad[:8]], b[bad[:8]])


@pytest.mark.parametrize("mode", [PARTITION, ATOMIC])
def test_three_launches_large_small_large_into_the_same_counters(ctx, world, mode):
    """40 000, then 5 000, then 40 000 reads: what a launch left in the scratch (lines, overflow lengths) must not reach the next one,
    after a larger and after a smaller batch; the hot barcode's bin overflows in both long launches.  Both commits == the oracle."""
    ctx.set_option("commit", mode)
    for n in (N_READS, N_SMALL, N_READS):
        classify(ctx, world, n)
    exp = [2 * a + b for a, b in zip(world["exp"], world["exp_small"])]
    equal(ctx.counts_read(N_BC), exp, "mode %d" % mode)
    # and once more after a read-back, alone: a single launch == the oracle
    ctx.counts_zero()
    classify(ctx, world, N_READS)
    equal(ctx.counts_read(N_BC), world["exp"], "mode %d, one launch" % mode)


def test_counters_resized_to_another_bin_count_between_launches(ctx, world):
    """4 bins, then 6 (1 500 barcodes), then 4 again: the scratch is laid out anew each time"""
    ctx.set_option("commit", PARTITION)
    classify(ctx, world, N_READS)
    equal(ctx.counts_read(N_BC), world["exp"], "4 bins")
    for n_bc in (1500, N_BC):
        ctx.counts_resize(n_bc)
        ctx.counts_zero()
        classify(ctx, world, N_READS)
        classify(ctx, world, N_SMALL)
        exp = [np.concatenate([a + b, np.zeros(n_bc - N_BC, np.uint64)]) for a, b in zip(world["exp"], world["exp_small"])]
        equal(ctx.counts_read(n_bc), exp, "%d barcodes" % n_bc)


def test_a_callers_votes_buffer_still_gets_u32_pairs_and_the_same_sums(ctx, world):
    """with a votes buffer the rows stay {vote0, vote1} as two u32 and the partitioned commit reads those; launches with and
    without the buffer alternate over one scratch"""
    ctx.set_option("commit", PARTITION)
    d_v = ctx.to_device(np.full((N_READS, 2), 0xA5A5A5A5, np.uint32))
    classify(ctx, world, N_READS)
    ctx.classify_device(ctx.d_b, N_READS * L, N_READS, L, d_barcode_ids=ctx.d_i, d_votes=d_v)
    classify(ctx, world, N_READS)
    equal(ctx.counts_read(N_BC), [3 * a for a in world["exp"]], "with and without a votes buffer")
    votes = ctx.to_host(d_v, (N_READS, 2), np.uint32)
    assert int(votes.max()) == L - K + 1
    got = [np.zeros(N_BC, np.uint64) for _ in range(3)]
    np.add.at(got[0], world["ids"], votes[:, 0].astype(np.uint64))
    np.add.at(got[1], world["ids"], votes[:, 1].astype(np.uint64))
    np.add.at(got[2], world["ids"], ((votes[:, 0] | votes[:, 1]) == 0).astype(np.uint64))
    equal(got, world["exp"], "the rows of the votes buffer")


@pytest.mark.parametrize("span", [13, 12, 0])
def test_bins_of_8192_barcodes_as_10M_barcodes_get_them(ctx, world, span):
    """20 000 barcodes at 8192 per bin (the option part_span; what 10M barcodes get by themselves): 3 bins, a thread of k_commit_bins
    adds the sums of 8 barcodes.  The 1000 ids are mapped onto ids on both sides of every bin border and of the borders inside a
    bin at which the thread's batch turns over, the first and the last one."""
    n_bc = 20_000
    rng = np.random.default_rng(span)
    fixed = np.array([0, 1, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 16383, 16384, 16385, n_bc - 2, n_bc - 1])
    rest = rng.choice(np.setdiff1d(np.arange(n_bc), fixed), N_BC - fixed.size, replace=False)
    to = np.sort(np.concatenate([fixed, rest])).astype(np.uint32)                # id i of the world -> barcode to[i]
    assert to[BORDER_IDS[0]] == 0 and to[BORDER_IDS[-1]] == n_bc - 1 and to[HOT] < 8192
    d_i = ctx.to_device(to[world["ids"]])
    ctx.counts_resize(n_bc)
    ctx.counts_zero()
    ctx.set_option("commit", PARTITION)
    ctx.set_option("part_span", span)
    assert ctx.options() == "commit=2" + (" part_span=%d" % span if span else "")
    for n in (N_READS, N_SMALL):
        ctx.classify_device(ctx.d_b, n * L, n, L, d_barcode_ids=d_i)
    exp = [np.zeros(n_bc, np.uint64) for _ in range(3)]
    for e, a, b in zip(exp, world["exp"], world["exp_small"]):
        e[to] = a + b
    equal(ctx.counts_read(n_bc), exp, "span %d" % span)
