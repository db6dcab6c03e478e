"""The device-side barcode DICTIONARY at and past its last id (-m gpu): k_fq_name_claim (fq_kernels.hip, the protocol of
name_claim.h) through the ABI, against a Python dict that restates BarcodeCache's first-sighting rule (classify.cpp:52-56: a barcode
gets its entry the first time it is seen, one entry per text).

The dictionary hands out hast_names_limit ids; what arrives after that is left to the caller, who numbers it in a range of its own
above.  Nothing merges the two ranges by text, so the dictionary must give ONE ANSWER PER TEXT: a device id for every record that
carries it, or none for any of them -- also in the block in which the last ids go, where hundreds of workgroups claim at once.

Input shape: short records (reads of K bases, ~60 bytes), one large block per launch -- 50 000 to 260 000 records.  The claim kernel
runs min(ceil(n / 256), 1024) workgroups of 256, record i is global lane i: records i and i + 256 c sit in different workgroups,
i and i + 64 in different waves.  The placements below put the occurrences of a text at those distances.

On every block: no record is left to the caller whose text (<= 15 bytes) has a device id, from an earlier block or from this one, and
no record gets a device id whose text the caller has had to name; device ids are dense from 0, below dict_ids, dict_ids never
decreases (one context) and equals min(limit, distinct short texts so far); nothing of <= 15 bytes is left to the caller before the
count has reached the limit; texts of >= 16 bytes always are.  At the end: hast_names_count, hast_names_texts for every id, and the
per-barcode counters against the oracle."""
import ctypes as C

import numpy as np
import pytest

import hast_amd
from hast_amd.binding import FqBlock, make_params

pytestmark = pytest.mark.gpu

K = 21
N_KEYS = 3000
NONE = 0xFFFFFFFF                          # HAST_NAME_NONE (include/hast.h)
HAST_ERR_INVALID, HAST_ERR_TABLE_FULL = 1, 5
N_LONG = 48                                # texts of >= 16 bytes in every input: always the caller's


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def short_texts(n):
    """n distinct texts of at most 15 bytes: the empty one (its text record is sixteen zero bytes), one byte, 14 and 15 bytes (a full
    record), and stLFR-like a_b_c in between; no '#', '/' or white space"""
    out = [b"", b"A", b"7", b"_", b"ABCDEFGHIJKLMNO", b"ABCDEFGHIJKLMN"]
    i = 0
    while len(out) < n:
        out.append((b"%014d" % i) if i % 4 == 0 else (b"%015d" % i) if i % 4 == 1 else b"%d_%d_%d" % (i % 1536, i // 1536, 1 + i % 3))
        i += 1
    out = out[:n]
    assert len(set(out)) == n and all(len(t) <= 15 for t in out)
    return out


def long_texts():
    """16 bytes and more; some equal to a short text in their first 15 bytes (the record keeps 15: they must not be taken for it)"""
    out = [b"ABCDEFGHIJKLMNOP", b"ABCDEFGHIJKLMNOQ", b"000000000000001x", b"000000000000001y", b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"]
    i = 0
    while len(out) < N_LONG:
        out.append(b"lib7_%d_222222_3333" % i if i % 2 else b"%016d" % i)
        i += 1
    assert len(set(out)) == N_LONG and all(len(t) >= 16 for t in out)
    return out


def place(n_short, spacing, n_min, rng, occ=4):
    """the text index of every record (>= n_short: a long text).  Every short text occurs `occ` times or more (at least occ - 1 after
    the sprinkle below), its occurrences `spacing` records apart (1: adjacent, one wave; 64: the next wave; 256: the next workgroup; 4096: sixteen workgroups on; 0:
    shuffled); at least n_min records.  Positions that no short text falls on carry long texts."""
    d = spacing if spacing > 1 else 1
    seq = []
    if spacing in (0, 1):
        reps = max(occ, -(-n_min // max(n_short, 1)))
        seq = np.repeat(np.arange(n_short, dtype=np.int64), reps)
        if spacing == 0:
            seq = seq[rng.permutation(seq.size)]
    else:
        groups = -(-n_short // d)
        reps = max(occ, -(-n_min // (groups * d)))
        pos = np.arange(d, dtype=np.int64)
        parts = []
        for g in range(groups):
            one = g * d + pos
            one = np.where(one < n_short, one, n_short + (one % N_LONG))
            parts.append(np.tile(one, reps))
        seq = np.concatenate(parts)
    # a sprinkle of long texts everywhere (1 in 64), in place: the distances above stay what they are
    seq = seq.copy()
    at = rng.choice(seq.size, size=seq.size // 64, replace=False)
    keep = np.ones(seq.size, bool)
    # ... but never on the first occ - 1 occurrences of a short text: find them and protect them
    order = np.argsort(seq, kind="stable")
    rank = np.empty(seq.size, np.int64)
    starts = np.r_[0, np.flatnonzero(np.diff(seq[order])) + 1]
    rank[order] = np.arange(seq.size) - np.repeat(starts, np.diff(np.r_[starts, seq.size]))
    keep[at] = False
    keep |= rank < occ - 1
    seq[~keep] = n_short + rng.integers(0, N_LONG, size=int((~keep).sum()))
    return seq


class Input:
    def __init__(self, n_short, seq, reads_pool, rng):
        self.shorts, self.longs = short_texts(n_short), long_texts()
        self.texts = self.shorts + self.longs
        self.n_short = n_short
        self.seq = np.asarray(seq, dtype=np.int64)
        # (which read a record carries: scattered over the pool, whatever the pattern of the texts -- every other pool entry is a key)
        self.read_of = (((np.arange(self.seq.size, dtype=np.int64) * 2654435761 + self.seq * 40503) % (1 << 32)) >> 13) % reads_pool.shape[0]
        self.pool = reads_pool
        rec = np.zeros((len(self.texts), 16), np.uint8)
        for j, t in enumerate(self.texts):
            if len(t) > 15:
                rec[j, 0] = 0xFF
            else:
                rec[j, 0] = len(t)
                rec[j, 1:1 + len(t)] = np.frombuffer(t, np.uint8)
        self.text_rec = rec
        self.text_len = np.array([len(t) for t in self.texts], np.int64)
        self.is_long = self.text_len > 15

    def bytes_of(self, lo, hi):
        pool = [self.pool[i].tobytes() for i in range(self.pool.shape[0])]
        qual = b"F" * K
        return b"".join(b"@r#" + self.texts[t] + b"/1\n" + pool[r] + b"\n+\n" + qual + b"\n" for t, r in zip(self.seq[lo:hi].tolist(), self.read_of[lo:hi].tolist()))


def first_sighting_model(inp, limit, blocks):
    """the Python dict: ids in order of first sighting; returns per block (ids left at its start, new short texts in it)"""
    seen, out = {}, []
    for lo, hi in blocks:
        left = max(0, limit - len(seen))
        new = 0
        for t in inp.seq[lo:hi].tolist():
            if t < inp.n_short and t not in seen:
                seen[t] = len(seen)
                new += 1
        out.append((left, new))
    return len(seen), out


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(oracle_lib):
    p = make_params(K, 100, N_KEYS, 1)
    keys = [hast_amd.synth_keys_host(p, h, 0, N_KEYS) for h in (0, 1)]
    rng = np.random.default_rng(20261017)
    pool = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(4096, K))]
    allk = np.concatenate(keys)
    for i in range(0, 4096, 2):                                   # every other read IS a key of one of the sets
        key = int(allk[(i * 2654435761) % allk.size])
        pool[i] = np.frombuffer("".join("ACTG"[(key >> (2 * (K - 1 - j))) & 3] for j in range(K)).encode(), np.uint8)
    return {"keys": keys, "pool": np.ascontiguousarray(pool), "oracle": oracle_lib}


def new_contexts(world, n):
    lib = hast_amd.lib()
    ctxs = [hast_amd.Context(K) for _ in range(n)]
    ctxs[0].table_reserve(2 * N_KEYS)
    ctxs[0].table_insert_keys(0, world["keys"][0])
    ctxs[0].table_insert_keys(1, world["keys"][1])
    for c in ctxs[1:]:
        assert lib.hast_table_clone(c._h, ctxs[0]._h) == 0, lib.hast_last_error()
    return ctxs


@pytest.fixture(scope="module")
def one_ctx(world):
    ctxs = new_contexts(world, 1)
    yield ctxs[0]
    ctxs[0].close()


def oracle_counts(world, inp, ids, n_ids):
    o = world["oracle"]
    oc = o.ho_new()
    for h in (0, 1):
        assert o.ho_load_keys(oc, world["keys"][h].ctypes.data, world["keys"][h].size, h, K) == 0
    bases = np.ascontiguousarray(world["pool"][inp.read_of]).reshape(-1)
    off = np.arange(inp.seq.size + 1, dtype=np.uint64) * K
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    e = [np.zeros(n_ids, np.uint32) for _ in range(3)]
    o.ho_classify_ids(oc, bases.ctypes.data, off.ctypes.data, ids.ctypes.data, ids.size, e[0].ctypes.data, e[1].ctypes.data, e[2].ctypes.data, None, 2)
    o.ho_free(oc)
    return e


# ---- the harness --------------------------------------------------------------------------------------------------------------------
class Checker:
    """what must hold block by block, in numpy (a block has 10^5 records)"""

    def __init__(self, inp, limit, one_context):
        self.inp, self.limit, self.one_context = inp, limit, one_context
        n = len(inp.texts)
        self.dev_id = np.full(n, -1, np.int64)                     # device id by text
        self.host_id = np.full(n, -1, np.int64)                    # the caller's id by text (order of first sighting)
        self.n_host = 0
        self.seen_short = np.zeros(n, bool)
        self.prev_dict_ids = 0
        self.at = 0                                                # records so far
        self.host_named = 0
        self.short_left = 0                                        # records of <= 15 bytes left to the caller
        self.final_ids = np.zeros(inp.seq.size, np.uint32)
        self.broken = []                                           # texts with two answers (reported, then asserted)

    def block(self, b):
        inp, limit = self.inp, self.limit
        n = int(b.n_records)
        tix = inp.seq[self.at:self.at + n]
        assert tix.size == n, (self.at, n, inp.seq.size)
        assert not b.short_read
        if b.bc_text:                                              # the framer's copy of the text: the record the dictionary keys on
            rec = np.ctypeslib.as_array(b.bc_text, shape=(n, 16))
            want = inp.text_rec[tix]
            assert np.array_equal(rec[:, 0], want[:, 0])
            short = ~inp.is_long[tix]
            assert np.array_equal(rec[short], want[short])         # (all sixteen bytes: the padding is zero -- the empty text is all zero)
        assert np.array_equal(np.ctypeslib.as_array(b.bc_len, shape=(n,)), inp.text_len[tix])
        assert b.unknown, "a stream over a dictionary always says which records it left"
        ids = np.ctypeslib.as_array(b.ids, shape=(n,))
        unk = np.zeros(n, bool)
        if b.n_unknown:
            unk[np.ctypeslib.as_array(b.unknown, shape=(int(b.n_unknown),))] = True
        assert int(unk.sum()) == int(b.n_unknown)
        dict_ids = int(b.dict_ids)
        assert dict_ids <= limit
        is_long = inp.is_long[tix]
        assert unk[is_long].all(), "a text of 16 bytes or more got a device id"
        # the dictionary's own ids: below dict_ids, one per text -- within the block and against every earlier block
        kt, kid = tix[~unk], ids[~unk].astype(np.int64)
        if kt.size:
            assert int(kid.max()) < dict_ids, (int(kid.max()), dict_ids)
            order = np.argsort(kt, kind="stable")
            st, sid = kt[order], kid[order]
            same = st[1:] == st[:-1]
            assert np.array_equal(sid[1:][same], sid[:-1][same]), "one text, two device ids in one block"
            ut, first = np.unique(st, return_index=True)
            uid = sid[first]
            old = self.dev_id[ut]
            assert np.array_equal(old[old >= 0], uid[old >= 0]), "a text changed its device id"
            self.dev_id[ut] = uid
        # ONE ANSWER PER TEXT: left to the caller <-> no device id, now or ever
        ushort = np.unique(tix[unk & ~is_long])
        both = ushort[self.dev_id[ushort] >= 0]                    # left to the caller although the device has numbered it (earlier, or in this block)
        known = np.unique(kt)
        late = known[self.host_id[known] >= 0]                     # numbered by the device after the caller had had to name it
        for t in np.concatenate([both, late]).tolist():
            self.broken.append((inp.texts[t], int(self.dev_id[t]), self.at))
        if ushort.size:
            assert dict_ids >= limit, "a text of <= 15 bytes left to the caller while the dictionary had ids"
        self.short_left += int((unk & ~is_long).sum())
        # density
        self.seen_short[tix[~is_long]] = True
        have = np.sort(self.dev_id[self.dev_id >= 0])
        if self.one_context:
            assert dict_ids >= self.prev_dict_ids
            assert dict_ids == min(limit, int(self.seen_short.sum())), (dict_ids, limit, int(self.seen_short.sum()))
            assert np.array_equal(have, np.arange(dict_ids)), "device ids not dense from 0"
        else:
            assert have.size == np.unique(have).size and (have.size == 0 or int(have[-1]) < limit)
        self.prev_dict_ids = dict_ids
        # the caller's part: its own range above the limit, ids in order of first sighting
        ut = tix[unk]
        if ut.size:
            new, first = np.unique(ut, return_index=True)
            fresh = self.host_id[new] < 0
            new = new[fresh][np.argsort(first[fresh])]
            self.host_id[new] = self.n_host + np.arange(new.size)
            self.n_host += new.size
            ids[unk] = (limit + self.host_id[ut]).astype(np.uint32)
        self.host_named += int(unk.sum())
        self.final_ids[self.at:self.at + n] = ids
        self.at += n

    def end(self, lib, nm):
        assert not self.broken, ("texts with a device id AND left to the caller", len(self.broken), self.broken[:5])
        assert self.at == self.inp.seq.size
        n = C.c_size_t()
        assert lib.hast_names_count(nm, C.byref(n)) == 0
        n_short_seen = int(self.seen_short.sum())
        assert n.value == min(self.limit, n_short_seen), (n.value, self.limit, n_short_seen)
        have = np.sort(self.dev_id[self.dev_id >= 0])
        assert np.array_equal(have, np.arange(n.value)), "device ids not dense from 0"
        txt = (C.c_uint8 * (16 * max(n.value, 1)))()
        assert lib.hast_names_texts(nm, 0, n.value, txt) == 0, lib.hast_last_error()
        raw = np.frombuffer(txt, np.uint8).reshape(-1, 16)[:n.value]
        t = np.flatnonzero(self.dev_id >= 0)
        assert np.array_equal(raw[self.dev_id[t]], self.inp.text_rec[t]), "hast_names_texts: not the text of the id"
        return n.value


def run_stream(world, ctxs, inp, cache, blocks, block_bytes, shared=True, n_buffers=2, counters=None):
    """the records of `inp` through hast_fq_* over a dictionary of `cache`.  One context: `blocks` = record ranges, one block each, opened
    as soon as it is submitted.  Several: a striped stream with the SAME dictionary in every lane, full blocks of block_bytes, as many
    in flight as the buffers allow -- their naming kernels run on the contexts' streams at the same time."""
    lib = hast_amd.lib()
    fq, nm = C.c_void_p(), C.c_void_p()
    assert lib.hast_names_create_dict(ctxs[0]._h, cache, C.byref(nm)) == 0, lib.hast_last_error()
    limit = lib.hast_names_limit(nm)
    n_counters = counters if counters is not None else limit + len(inp.texts) + 16
    for c in ctxs:
        c.counts_resize(n_counters)
    ck = Checker(inp, limit, len(ctxs) == 1)
    b = FqBlock()

    def drain():
        assert lib.hast_fq_next(fq, C.byref(b)) == 0, lib.hast_last_error()
        ck.block(b)
        assert lib.hast_fq_commit(fq) == 0, lib.hast_last_error()

    try:
        if len(ctxs) == 1:
            assert lib.hast_fq_create(ctxs[0]._h, block_bytes, n_buffers, nm, C.byref(fq)) == 0, lib.hast_last_error()
            for j, (lo, hi) in enumerate(blocks):
                data = inp.bytes_of(lo, hi)
                assert len(data) <= block_bytes, (len(data), block_bytes)
                buf = C.POINTER(C.c_uint8)()
                assert lib.hast_fq_acquire(fq, C.byref(buf)) == 0, lib.hast_last_error()
                C.memmove(buf, data, len(data))
                assert lib.hast_fq_submit(fq, len(data), 1 if j == len(blocks) - 1 else 0) == 0, lib.hast_last_error()
                drain()
                assert int(b.n_records) == hi - lo
        else:
            arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
            narr = (C.c_void_p * len(ctxs))(*[nm.value for _ in ctxs])
            assert lib.hast_fq_create_striped(arr, len(ctxs), block_bytes, n_buffers, narr, C.byref(fq)) == 0, lib.hast_last_error()
            data = inp.bytes_of(0, inp.seq.size)
            pos = pending = 0
            while True:
                n = min(len(data) - pos, block_bytes)
                buf = C.POINTER(C.c_uint8)()
                assert lib.hast_fq_acquire(fq, C.byref(buf)) == 0, lib.hast_last_error()
                C.memmove(buf, data[pos:pos + n], n)
                pos += n
                last = pos >= len(data)
                assert lib.hast_fq_submit(fq, n, 1 if last else 0) == 0, lib.hast_last_error()
                pending += 1
                while pending > (0 if last else n_buffers * len(ctxs) - 1):
                    drain()
                    pending -= 1
                if last:
                    break
            lanes = [lib.hast_fq_lane_records(fq, g) for g in range(len(ctxs))]
            assert sum(lanes) == inp.seq.size and all(x > 0 for x in lanes), lanes
        lib.hast_fq_destroy(fq)
        fq = C.c_void_p()
        count = ck.end(lib, nm)
        # the counters: the oracle's, under the ids the records ended up with
        n_ids = limit + ck.n_host
        if len(ctxs) > 1:
            assert lib.hast_counts_allreduce((C.c_void_p * len(ctxs))(*[c._h for c in ctxs]), len(ctxs)) == 0, lib.hast_last_error()
        got = ctxs[0].counts_read(n_ids)
        want = oracle_counts(world, inp, ck.final_ids, n_ids)
        for a, e in zip(got, want):
            assert np.array_equal(a, e)
        assert int(want[0].sum()) + int(want[1].sum()) > inp.seq.size // 4
    finally:
        if fq:
            lib.hast_fq_destroy(fq)
        lib.hast_names_destroy(nm)
    return ck, count, limit


def cut_blocks(n, size):
    """as few blocks of at most `size` records as hold n, all of (nearly) one size"""
    k = -(-n // size)
    each = -(-n // k)
    return [(lo, min(n, lo + each)) for lo in range(0, n, each)]


BLOCK_RECORDS = 260_000
BLOCK_BYTES = 20 << 20                     # 260 000 records of at most 78 bytes


# ---- the cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", [1, 64, 256, 4096, 0], ids=["adjacent", "64_apart", "256_apart", "4096_apart", "shuffled"])
@pytest.mark.parametrize("distinct", ["limit-1", "limit", "limit+1", "4xlimit"])
@pytest.mark.parametrize("cache", [16, 1024, 65536])
def test_dictionary_one_answer_per_text(world, one_ctx, monkeypatch, cache, distinct, spacing):
    """limits 32 (the smallest dictionary there is: 64 slots), 1 024 and 65 536; one id fewer texts than ids, as many, one more, four
    times as many; the occurrences of a text adjacent, 64, 256, 4 096 apart and shuffled"""
    monkeypatch.setenv("HAST_FQ_HOST_RECORDS", str(BLOCK_RECORDS + 1024))       # the per-record arrays hold a block: named behind its framing, as in production
    limit = max(2 * cache, 64) // 2
    n_short = {"limit-1": limit - 1, "limit": limit, "limit+1": limit + 1, "4xlimit": 4 * limit}[distinct]
    rng = np.random.default_rng(cache * 1000 + n_short % 997 + spacing)
    inp = Input(n_short, place(n_short, spacing, 50_000, rng), world["pool"], rng)
    blocks = cut_blocks(inp.seq.size, BLOCK_RECORDS)
    assert all(50_000 <= hi - lo <= BLOCK_RECORDS for lo, hi in blocks)
    # what the input claims to do, in plain Python
    n_seen, per_block = first_sighting_model(inp, limit, blocks)
    assert n_seen == n_short
    exhausts = n_short > limit
    crossing = [j for j, (left, new) in enumerate(per_block) if new > left]
    assert bool(crossing) == exhausts, (per_block, limit)
    if n_short >= 1000 and spacing not in (1, 64):
        wg = {}
        for i, t in enumerate(inp.seq[blocks[0][0]:blocks[0][1]].tolist()):
            if t < n_short:
                wg.setdefault(t, set()).add(i // 256)
        assert sum(1 for s in wg.values() if len(s) > 1) >= min(1000, n_short - 1)
    ck, count, got_limit = run_stream(world, [one_ctx], inp, cache, blocks, BLOCK_BYTES)
    assert got_limit == limit
    print("limit %d texts %d spacing %d: records %d blocks %d count %d host_named %d short_left %d" % (limit, n_short, spacing, inp.seq.size, len(blocks), count, ck.host_named, ck.short_left))
    n_long_records = int(inp.is_long[inp.seq].sum())
    if exhausts:
        assert count == limit and ck.host_named > n_long_records and ck.short_left > 0
    else:
        assert count == n_short and ck.host_named == n_long_records and ck.short_left == 0
    assert n_long_records > 0


def crossing_round(world, ctx, r, cache=1024, n_texts=4096, apart=4096, occ=4):
    """a fresh dictionary of 1 024 ids over one block: 4 096 texts, each four times, 4 096 records apart (sixteen workgroups), the start
    staggered by r; behind them long texts up to 50 000 records"""
    rng = np.random.default_rng(77000 + r)
    lead = (r * 37) % 256                                          # shifts every text against the wave and workgroup borders
    body = (np.arange(n_texts * occ, dtype=np.int64) + r * 61) % n_texts
    assert apart == n_texts
    fill = max(0, 50_000 - lead - body.size)
    seq = np.concatenate([n_texts + rng.integers(0, N_LONG, size=lead), body, n_texts + rng.integers(0, N_LONG, size=fill)])
    inp = Input(n_texts, seq, world["pool"], rng)
    limit = max(2 * cache, 64) // 2
    # the block crosses the limit, with most texts in several workgroups
    assert n_texts > limit
    pos = {}
    for i, t in enumerate(seq.tolist()):
        if t < n_texts:
            pos.setdefault(t, set()).add(i // 256)
    assert sum(1 for s in pos.values() if len(s) > 1) >= 1000
    lib = hast_amd.lib()
    fq, nm = C.c_void_p(), C.c_void_p()
    assert lib.hast_names_create_dict(ctx._h, cache, C.byref(nm)) == 0, lib.hast_last_error()
    assert lib.hast_names_limit(nm) == limit
    ck = Checker(inp, limit, True)
    try:
        assert lib.hast_fq_create(ctx._h, 4 << 20, 2, nm, C.byref(fq)) == 0, lib.hast_last_error()
        data = inp.bytes_of(0, seq.size)
        buf = C.POINTER(C.c_uint8)()
        assert lib.hast_fq_acquire(fq, C.byref(buf)) == 0, lib.hast_last_error()
        C.memmove(buf, data, len(data))
        assert lib.hast_fq_submit(fq, len(data), 1) == 0, lib.hast_last_error()
        b = FqBlock()
        assert lib.hast_fq_next(fq, C.byref(b)) == 0, lib.hast_last_error()
        ck.block(b)
        assert lib.hast_fq_commit(fq) == 0, lib.hast_last_error()
        lib.hast_fq_destroy(fq)
        fq = C.c_void_p()
        broken, ck.broken = ck.broken, []
        count = ck.end(lib, nm)
        assert count == limit and ck.short_left > 0
    finally:
        if fq:
            lib.hast_fq_destroy(fq)
        lib.hast_names_destroy(nm)
    return broken


N_CROSSING_ROUNDS = 200


def test_dictionary_crossing_the_limit_many_times(world, one_ctx, monkeypatch):
    """The block in which the last ids go, 200 times over, each time on a fresh dictionary: lanes of different workgroups meet the same
    new text while the counter passes the limit.  The order of rounds 6 to 10 (slot looked at, then the counter, no second look) lets
    one of them take the last id and publish while the other, having seen the slot empty a moment earlier, finds every id gone and
    leaves the text to the caller: two rows for one barcode.  Zero rounds may show that.
    Measured once with this harness on the kernel of round 10, on an MI355X: 28 of 200 rounds, 13 to 54 texts each; on this one: 0."""
    monkeypatch.setenv("HAST_FQ_HOST_RECORDS", "66000")
    one_ctx.counts_resize(1024 + 4096 + N_LONG + 16)
    bad = []
    for r in range(N_CROSSING_ROUNDS):
        broken = crossing_round(world, one_ctx, r)
        if broken:
            bad.append((r, len(broken), broken[:2]))
    print("crossing the limit: %d of %d rounds gave a text a device id AND left it to the caller" % (len(bad), N_CROSSING_ROUNDS), bad[:5])
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("placement", ["by_block", "shuffled"])
@pytest.mark.parametrize("n_ctx", [2, 3, 4])
def test_dictionary_shared_by_several_contexts(world, monkeypatch, n_ctx, placement):
    """ONE dictionary in every lane of a striped stream (what --devices 0,0 does): the naming kernels of as many blocks as there are
    buffers claim in it at the same time, on the contexts' streams, while it runs out.  16 384 ids, 65 536 texts six times: text t at
    records t, t + 65 536, ... -- about one block apart, so its occurrences sit at like places of neighbouring blocks, on different
    contexts -- or shuffled."""
    monkeypatch.setenv("HAST_FQ_HOST_RECORDS", "70000")
    cache, n_short, occ = 16384, 65536, 6
    rng = np.random.default_rng(4200 + n_ctx)
    seq = np.tile(np.arange(n_short, dtype=np.int64), occ)
    if placement == "shuffled":
        seq = seq[rng.permutation(seq.size)]
    seq = np.concatenate([seq[:1000], n_short + rng.integers(0, N_LONG, size=64), seq[1000:]])
    inp = Input(n_short, seq, world["pool"], rng)
    block_bytes = 3 << 20                                          # some 52 000 records
    ctxs = new_contexts(world, n_ctx)
    try:
        ck, count, limit = run_stream(world, ctxs, inp, cache, None, block_bytes, n_buffers=2)
    finally:
        for c in ctxs:
            c.close()
    print("shared by %d contexts, %s: count %d host_named %d short_left %d" % (n_ctx, placement, count, ck.host_named, ck.short_left))
    assert limit == 16384 and count == limit and ck.host_named > 64 and ck.short_left > 0


def fill_dictionary(world, ctx, cache, texts_idx, inp_texts_n):
    """a dictionary that has seen the short texts texts_idx (of short_texts(inp_texts_n)), in that order, through a stream"""
    rng = np.random.default_rng(5)
    inp = Input(inp_texts_n, np.asarray(texts_idx, dtype=np.int64), world["pool"], rng)
    lib = hast_amd.lib()
    fq, nm = C.c_void_p(), C.c_void_p()
    assert lib.hast_names_create_dict(ctx._h, cache, C.byref(nm)) == 0, lib.hast_last_error()
    ctx.counts_resize(lib.hast_names_limit(nm) + 64)
    assert lib.hast_fq_create(ctx._h, 1 << 20, 2, nm, C.byref(fq)) == 0, lib.hast_last_error()
    data = inp.bytes_of(0, inp.seq.size)
    buf = C.POINTER(C.c_uint8)()
    assert lib.hast_fq_acquire(fq, C.byref(buf)) == 0
    C.memmove(buf, data, len(data))
    assert lib.hast_fq_submit(fq, len(data), 1) == 0
    b = FqBlock()
    assert lib.hast_fq_next(fq, C.byref(b)) == 0, lib.hast_last_error()
    assert b.n_unknown == 0
    assert lib.hast_fq_commit(fq) == 0, lib.hast_last_error()
    lib.hast_fq_destroy(fq)
    return nm, inp


def texts_of(lib, nm, n):
    txt = (C.c_uint8 * (16 * max(n, 1)))()
    assert lib.hast_names_texts(nm, 0, n, txt) == 0, lib.hast_last_error()
    raw = bytes(txt)
    return [raw[16 * i + 1:16 * i + 1 + raw[16 * i]] for i in range(n)]


def test_names_merge_into_a_dictionary_that_runs_out(world, one_ctx):
    """hast_names_merge when the destination has fewer ids left than the source has new texts (include/hast.h): HAST_ERR_TABLE_FULL, and
    ids_out complete all the same -- the ids of the texts that were known or still fitted, right and dense, HAST_NAME_NONE for the rest;
    the same call again returns the same."""
    lib = hast_amd.lib()
    # dst: 32 ids, 20 of them taken (texts 0..19); src: texts 10..69 -- ten known to dst, fifty new, twelve ids left
    dst, _ = fill_dictionary(world, one_ctx, 16, list(range(20)), 80)
    src, inp = fill_dictionary(world, one_ctx, 128, list(range(10, 70)), 80)
    try:
        assert lib.hast_names_limit(dst) == 32
        n = C.c_size_t()
        assert lib.hast_names_count(src, C.byref(n)) == 0 and n.value == 60
        src_texts = texts_of(lib, src, 60)
        assert sorted(src_texts) == sorted(inp.shorts[10:70])
        before = texts_of(lib, dst, 20)
        # a piece that fits: ids [0, 8) of src -- whatever texts those are
        out0 = (C.c_uint32 * 8)()
        new0 = [t for t in src_texts[:8] if t not in before]
        assert lib.hast_names_merge(dst, src, 0, 8, out0) == 0, lib.hast_last_error()
        assert lib.hast_names_count(dst, C.byref(n)) == 0 and n.value == 20 + len(new0)
        mid = texts_of(lib, dst, n.value)
        assert mid[:20] == before and sorted(mid[20:]) == sorted(new0)
        assert [mid[i] for i in out0] == src_texts[:8]
        # all of it: more new texts than ids
        new_all = [t for t in src_texts if t not in mid]
        assert len(new_all) > 32 - len(mid)
        out1, out2 = (C.c_uint32 * 60)(), (C.c_uint32 * 60)()
        assert lib.hast_names_merge(dst, src, 0, 60, out1) == HAST_ERR_TABLE_FULL
        assert b"no id left" in lib.hast_last_error()
        assert lib.hast_names_count(dst, C.byref(n)) == 0 and n.value == 32
        full = texts_of(lib, dst, 32)
        assert full[:len(mid)] == mid and len(set(full)) == 32 and set(full[len(mid):]) <= set(new_all)
        ids = list(out1)
        for i, t in enumerate(src_texts):
            if t in full:
                assert ids[i] == full.index(t), (i, t, ids[i])         # what fitted: the right id
            else:
                assert ids[i] == NONE, (i, t, ids[i])                  # what did not: the marker
        assert sum(1 for x in ids if x == NONE) == len(new_all) - (32 - len(mid))
        assert sorted(set(x for x in ids if x != NONE) | set(range(len(mid)))) == list(range(32))       # dense
        assert lib.hast_names_merge(dst, src, 0, 60, out2) == HAST_ERR_TABLE_FULL
        assert list(out2) == ids
        assert texts_of(lib, dst, 32) == full
    finally:
        lib.hast_names_destroy(dst)
        lib.hast_names_destroy(src)


def test_commit_with_fewer_counters_than_dictionary_ids(world, one_ctx, monkeypatch):
    """A block the dictionary named completely is booked from its ids in device memory, unchecked: hast_fq_commit must refuse, on the host
    and before anything is queued, when the context's counters are fewer than hast_fq_block.dict_ids -- HAST_ERR_INVALID, the block
    still open -- and book it once they suffice."""
    lib = hast_amd.lib()
    rng = np.random.default_rng(9)
    n_short = 500
    inp = Input(n_short, np.tile(np.arange(n_short, dtype=np.int64), 3), world["pool"], rng)
    fq, nm = C.c_void_p(), C.c_void_p()
    assert lib.hast_names_create_dict(one_ctx._h, 1024, C.byref(nm)) == 0, lib.hast_last_error()
    one_ctx.counts_resize(8)
    try:
        assert lib.hast_fq_create(one_ctx._h, 1 << 20, 2, nm, C.byref(fq)) == 0, lib.hast_last_error()
        data = inp.bytes_of(0, inp.seq.size)
        buf = C.POINTER(C.c_uint8)()
        assert lib.hast_fq_acquire(fq, C.byref(buf)) == 0
        C.memmove(buf, data, len(data))
        assert lib.hast_fq_submit(fq, len(data), 1) == 0
        b = FqBlock()
        assert lib.hast_fq_next(fq, C.byref(b)) == 0, lib.hast_last_error()
        assert b.n_unknown == 0 and b.dict_ids == n_short and b.n_records == inp.seq.size
        ids = np.ctypeslib.as_array(b.ids, shape=(inp.seq.size,)).copy()
        assert lib.hast_fq_commit(fq) == HAST_ERR_INVALID
        assert b"dict_ids" in lib.hast_last_error()
        assert lib.hast_fq_commit(fq) == HAST_ERR_INVALID              # (still open, still refused)
        one_ctx.counts_resize(n_short - 1)
        assert lib.hast_fq_commit(fq) == HAST_ERR_INVALID
        one_ctx.counts_resize(n_short)                                 # the context is as usable as ever
        assert lib.hast_fq_commit(fq) == 0, lib.hast_last_error()
        lib.hast_fq_destroy(fq)
        fq = C.c_void_p()
        got = one_ctx.counts_read(n_short)
        for a, e in zip(got, oracle_counts(world, inp, ids, n_short)):
            assert np.array_equal(a, e)
        assert int(got[0].sum()) + int(got[1].sum()) > 100
    finally:
        if fq:
            lib.hast_fq_destroy(fq)
        lib.hast_names_destroy(nm)
