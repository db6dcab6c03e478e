"""GPU test of the read bins of stage 03's device ingest (hast_rs_set_bins / hast_rs_next_binned; rs_kernels.hip: k_rb_*; the
gzip job of dz_kernels.hip): files fed block by block, host and device blocks in turn, come back as three runs per view which,
concatenated over the views and with the FASTQ tail added, are the runs of tests/rb_model.py from the oracle's votes, byte for byte.
The two key sets differ in size (40 and 37 keys), so the denser haplotype is not the one with more votes."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import hast_amd
from hast_amd import ReadStream
from tests import rb_model as rb
from tests import rs_corpus as rc

pytestmark = pytest.mark.gpu
BLOCKS = (64, 700, 4096, 65536)
N0, N1 = 40, 37


def long_reads(keys, seed=11):
    """20 000-base reads on one line and over 60-column lines, keys planted back to back, small records in between"""
    rng = random.Random(seed)
    out = bytearray()
    for i in range(8):
        s = rc.seq_with_plants(rng, 20000, keys, dense=True)
        out += rc.fasta_text(rng, [(b"long%d" % i, s)], 1 << 20 if i % 2 == 0 else 60)
        out += rc.fasta_text(rng, rc.records(rng, 5, (150, 0, 61), keys, 60), 60)
    fq = rc.fastq_text([(b"long%d" % i, rc.seq_with_plants(rng, 20000, keys, dense=True)) for i in range(4)] + rc.records(rng, 9, (150, 0, 61), keys))
    return [("fa_long", rc.FASTA, bytes(out)), ("fq_long", rc.FASTQ, fq)]


def own_cases(keys, seed=23):
    """what the bins need beyond the corpus: records whose extents grow by one byte each, with a key of either set or none (every
    pair of source and destination alignment); reads with one key of each set (a tie in votes); files without any key"""
    rng = random.Random(seed)
    k = len(keys[0][0])

    def with_key(i, length):
        s = bytearray(b"N" * length)
        if i % 3 < 2 and length >= k:
            s[:k] = keys[i % 3][(i // 3) % len(keys[i % 3])]
        return bytes(s)
    grow = [(b"g%04d" % i, with_key(rng.randrange(3), k + i % 97)) for i in range(700)]
    tie = [(b"tie%d" % i, rng.choice(keys[0]) + b"N" + rng.choice(keys[1])) for i in range(40)] + rc.records(rng, 20, (150, 0, 61), keys)
    none = [(b"none%d" % i, b"N" * (i % 90)) for i in range(300)]
    big = 1 << 20
    return [("fa_grow", rc.FASTA, rc.fasta_text(rng, grow, big)), ("fq_grow", rc.FASTQ, rc.fastq_text(grow)),
            ("fa_tie", rc.FASTA, rc.fasta_text(rng, tie, 60)), ("fq_tie", rc.FASTQ, rc.fastq_text(tie)),
            ("fa_none", rc.FASTA, rc.fasta_text(rng, none, 60)), ("fq_none", rc.FASTQ, rc.fastq_text(none))]


def emitting_views(fmt, data, block):
    """from the file's lines alone: per record of rb_model.extents (the FASTQ tail left out) its file offset and the view that frames
    it, when view v is everything up to byte (v + 1) * block not framed before and the view behind the last block is the file's last"""
    ext = rb.extents(fmt, data)
    n_views = -(-len(data) // block) + 1
    out, at = [], 0
    if fmt == rc.FASTQ:
        for e in ext:
            if at + len(e) <= len(data) and e.count(b"\n") == 4:        # (not the tail)
                out.append((at, len(e), -(-(at + len(e)) // block) - 1))
            at += len(e)
        return out, n_views
    at = 0
    for line in data.split(b"\n")[:-1]:                                  # what lies in front of the first header line is nobody's
        if line[:1] == b">":
            break
        at += len(line) + 1
    for i, e in enumerate(ext):
        if i + 1 < len(ext):
            nxt = at + len(e)
            hdr_end = nxt + ext[i + 1].index(b"\n") + 1                   # a record is complete when the next header line is
            out.append((at, len(e), -(-hdr_end // block) - 1))
        else:
            out.append((at, len(e), n_views - 1))
        at += len(e)
    return out, n_views


class Cases:
    """the inputs with the oracle's votes and the model's runs; no GPU"""

    def __init__(self, k, oracle_lib):
        self.k = k
        keys = rc.make_keys(3, k)
        self.keys = [keys[0][:N0], keys[1][:N1]]
        self.o = oracle_lib
        self.s03 = oracle_lib.ho_s03_new()
        for hap in (0, 1):
            text = b"\n".join(self.keys[hap]) + b"\n"
            assert oracle_lib.ho_s03_load_text(self.s03, text, len(text), hap) == 0
        # the reference, once: name -> (format, bytes, records, votes, carry bound, (runs, counts, classes))
        self.cases = {}
        for name, fmt, data in rc.corpus(self.keys) + long_reads(self.keys) + own_cases(self.keys):
            want = rc.read_file(fmt, data)
            if want == rc.ERR:
                continue
            votes = self.hits([s for _, s in want])
            self.cases[name] = (fmt, data, want, votes, rc.carry_bound(fmt, data), rb.runs(fmt, data, votes, N0, N1))

    def hits(self, seqs):
        out = np.zeros((len(seqs), 2), dtype=np.uint32)
        h0, h1 = C.c_uint32(), C.c_uint32()
        for i, s in enumerate(seqs):
            self.o.ho_s03_read_hits(self.s03, s, len(s), C.byref(h0), C.byref(h1))
            out[i] = (h0.value, h1.value)
        return out



class Rig(Cases):
    def __init__(self, k, oracle_lib):
        super().__init__(k, oracle_lib)
        self.ctx = hast_amd.Context(k)
        self.ctx.table_reserve(N0 + N1 + 2)
        for hap in (0, 1):
            text = b"\n".join(self.keys[hap]) + b"\n"
            assert self.ctx.table_insert_text(hap, text) == len(self.keys[hap])
        self.feeds = {}
        self.results = {}

    def feed(self, fmt, block):
        if (fmt, block) not in self.feeds:
            self.feeds[(fmt, block)] = ReadStream(self.ctx, fmt, block)
        return self.feeds[(fmt, block)]

    def run(self, fmt, block, data, mode):
        """the file through the feed, a block ahead of the framer, host and device blocks in turn; mode None: hast_rs_next.
        Per view: (flags, consumed, names, votes, runs, raw_bytes, count); and the tail"""
        f = self.feed(fmt, block)
        views, pending = [], 0

        def step():
            if mode is None:
                fl, c, _, nm, v = f.next()
                views.append((fl, c, nm, v, None, None, None))
            else:
                fl, c, _, nm, v, runs, raw, cnt = f.next_binned()
                views.append((fl, c, nm, v, runs, raw, cnt))
        chunks = [data[i:i + block] for i in range(0, len(data), block)] + [b""]
        for i, chunk in enumerate(chunks):
            f.submit(chunk, last=i == len(chunks) - 1, device=i % 3 == 1)
            pending += 1
            if pending == 2:
                step()
                pending -= 1
        while pending:
            step()
            pending -= 1
        tail = f.take_tail() if fmt == rc.FASTQ else b""
        return views, tail

    def all_modes(self, fmt, block):
        """every case of the format that fits the block, through hast_rs_next, the plain bins and the gzip bins: computed once"""
        key = (fmt, block)
        if key not in self.results:
            f = self.feed(fmt, block)
            res = {}
            for name, c in self.cases.items():
                if c[0] != fmt or c[4] > block:
                    continue
                f.set_bins(0, 0, 0)
                plain = self.run(fmt, block, c[1], None)
                f.set_bins(1, N0, N1)
                m1 = self.run(fmt, block, c[1], 1)
                f.set_bins(2, N0, N1)
                m2 = self.run(fmt, block, c[1], 2)
                res[name] = (plain, m1, m2)
            f.set_bins(0, 0, 0)
            self.results[key] = res
        return self.results[key]

    def close(self):
        for f in self.feeds.values():
            f.close()
        self.o.ho_s03_free(self.s03)
        self.ctx.close()


@pytest.fixture(scope="module", params=[21, 31])
def rig(request, oracle_lib):
    r = Rig(request.param, oracle_lib)
    yield r
    r.close()


def tail_record(tail):
    """the bytes the FASTQ tail adds to its class's run"""
    if b"\n" not in tail:
        return b""
    return tail if tail.endswith(b"\n") else tail + b"\n"


def test_the_cases_hold_what_the_checks_rest_on(rig):
    check_cases(rig)


def check_cases(rig):
    """asserted from the models alone (no GPU is needed for it), before a pass below is trusted"""
    pairs = {b: set() for b in BLOCKS}
    one_class = {b: 0 for b in BLOCKS}
    no_record = {b: 0 for b in BLOCKS}
    classes = {b: [0, 0, 0] for b in BLOCKS}
    straddle = 0
    for name, (fmt, data, want, votes, bound, (runs, count, cls)) in rig.cases.items():
        for block in BLOCKS:
            if bound > block:
                continue
            recs, n_views = emitting_views(fmt, data, block)
            per_view = [[] for _ in range(n_views)]
            for i, (at, n, v) in enumerate(recs):
                per_view[v].append((i, at, n))
            for v, rs in enumerate(per_view):
                no_record[block] += not rs
                if len(rs) > 1 and len({cls[i] for i, _, _ in rs}) == 1:
                    one_class[block] += 1
                by = [sum(n for i, _, n in rs if cls[i] == c) for c in range(3)]
                dst = [0, by[0], by[0] + by[1]]
                for i, at, n in rs:
                    classes[block][cls[i]] += 1
                    pairs[block].add(((block + at - min(v * block, len(data))) % 16, dst[cls[i]] % 16))   # (new bytes lie at offset `block` of a 16-byte aligned buffer)
                    dst[cls[i]] += n
                    if block == 65536 and n > 3 * 4096 and at // block != (at + n - 1) // block:
                        straddle += 1
    for block in BLOCKS:
        assert min(classes[block]) > 0 and one_class[block] > 0 and no_record[block] > 0, (block, classes[block], one_class[block], no_record[block])
    assert len(pairs[4096]) == 256 and len(pairs[65536]) == 256, (len(pairs[4096]), len(pairs[65536]))
    assert straddle > 0
    differ = sum(1 for c in rig.cases.values() for (v0, v1), k in zip(c[3], c[5][2]) if k != (2 if v0 == v1 == 0 else 1 if v1 > v0 else 0))
    assert differ > 0
    for name in ("fa_grow", "fq_grow"):
        lens = sorted({len(e) for e in rb.extents(rig.cases[name][0], rig.cases[name][1])})
        assert len(lens) >= 90 and all(b - a in (1, 2) for a, b in zip(lens, lens[1:])), name


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_the_runs_are_the_models_runs(rig, fmt, block):
    res = rig.all_modes(fmt, block)
    assert len(res) >= (3 if block < 700 else 15)
    for name, (plain, m1, m2) in res.items():
        _, data, want, votes, _, (runs, count, cls) = rig.cases[name]
        views, tail = m1
        assert all(v[0] == 0 for v in views), (name, block)
        recs, n_views = emitting_views(fmt, data, block)
        assert len(views) == n_views and [len(v[2]) for v in views] == [sum(1 for r in recs if r[2] == i) for i in range(n_views)], (name, block)
        got = [b"".join(v[4][c] for v in views) for c in range(3)]
        got_count = [sum(v[6][c] for v in views) for c in range(3)]
        for v in views:
            assert [len(r) for r in v[4]] == v[5] and sum(v[6]) == len(v[2]), (name, block)
        if fmt == rc.FASTQ and tail_record(tail):
            got[cls[-1]] += tail_record(tail)
            got_count[cls[-1]] += 1
        for c in range(3):
            assert got[c] == runs[c], (name, block, c, len(got[c]), len(runs[c]))
        assert got_count == count, (name, block)
        raw = sum(sum(v[5]) for v in views)
        assert raw == sum(n for _, n, _ in recs) == sum(len(e) for e in rb.extents(fmt, data)) - len(tail_record(tail) if fmt == rc.FASTQ else b""), (name, block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_the_block_is_what_hast_rs_next_gives(rig, fmt, block):
    """names, votes and consumed of hast_rs_next_binned's view against hast_rs_next's on the same feed, and against the oracle's votes"""
    for name, (plain, m1, m2) in rig.all_modes(fmt, block).items():
        want, votes = rig.cases[name][2], rig.cases[name][3]
        for views, tail in (m1, m2):
            assert tail == plain[1] and len(views) == len(plain[0]), (name, block)
            for a, b in zip(plain[0], views):
                assert a[0] == b[0] == 0 and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3]), (name, block)
                assert a[4] is None and b[4] is not None
        names = [n for v in plain[0] for n in v[2]]
        got = np.concatenate([v[3] for v in plain[0]]) if plain[0] else np.zeros((0, 2), np.uint32)
        assert names == [w[0] for w in want[:len(names)]] and np.array_equal(got, votes[:len(names)]) and len(want) - len(names) <= 1, (name, block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_gzip_runs_are_one_member_each_of_the_plain_run(rig, fmt, block):
    members = 0
    for name, (plain, m1, m2) in rig.all_modes(fmt, block).items():
        for a, b in zip(m1[0], m2[0]):
            assert a[5] == b[5] and a[6] == b[6], (name, block)
            for c in range(3):
                if not a[4][c]:
                    assert b[4][c] == b"", (name, block, c)
                    continue
                z = zlib.decompressobj(16 + zlib.MAX_WBITS)
                raw = z.decompress(b[4][c])
                assert z.eof and z.unused_data == b"" and raw == a[4][c], (name, block, c, len(b[4][c]), len(a[4][c]))
                assert b[4][c][:4] == b"\x1f\x8b\x08\x00"
                members += 1
    assert members > 20


def test_switching_off_and_refusal(rig):
    f = rig.feed(rc.FASTA, 4096)
    fmt, data, want, votes, _, (runs, count, cls) = rig.cases["fa_tie"]
    f.set_bins(1, N0, N1)
    views, _ = rig.run(rc.FASTA, 4096, data, 1)
    assert [b"".join(v[4][c] for v in views) for c in range(3)] == runs
    f.set_bins(0, 0, 0)                                                      # off, between files: no bins, and the block as before
    views, _ = rig.run(rc.FASTA, 4096, data, 1)
    assert all(v[4] == [b"", b"", b""] and v[5] == [0, 0, 0] and v[6] == [0, 0, 0] for v in views)
    assert [n for v in views for n in v[2]] == [w[0] for w in want] and np.array_equal(np.concatenate([v[3] for v in views]), votes)
    views, _ = rig.run(rc.FASTA, 4096, data, None)
    assert [n for v in views for n in v[2]] == [w[0] for w in want] and np.array_equal(np.concatenate([v[3] for v in views]), votes)
    f.submit(data[:4096], last=False)
    with pytest.raises(hast_amd.HastError) as e:
        f.set_bins(1, N0, N1)
    assert e.value.status == 1                                               # HAST_ERR_INVALID: a block is pending
    f.next()
    f.submit(b"", last=True)
    f.next()
    f.set_bins(2, N0, N1)                                                    # ... and with none pending it is taken
    views, _ = rig.run(rc.FASTA, 4096, data, 2)
    assert [b"".join(zlib.decompress(v[4][c], 16 + zlib.MAX_WBITS) for v in views if v[4][c]) for c in range(3)] == runs
    f.set_bins(0, 0, 0)
