"""GPU test of stage 03's device ingest (hast_rs_*, hast_amd/csrc/rs_kernels.hip + rs_api.cpp): files fed block by block come back
as the reads of the reference's reader (tests/rs_corpus.py restates its two getline loops) -- names byte for byte, votes equal to the
oracle's hit counts on the sequences that reader frames.  K-mers are planted across FASTA line ends, so a hit needs the lines moved
together correctly; dense plants in 20 000-base reads cover the view boundaries and the 4-KB output tiles of the copy."""
import ctypes as C
import random

import numpy as np
import pytest

import hast_amd
from hast_amd import ReadStream
from tests import rs_corpus as rc

pytestmark = pytest.mark.gpu
BLOCKS = (64, 700, 4096, 65536)


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


class Rig:
    def __init__(self, k, oracle_lib):
        self.k = k
        self.keys = rc.make_keys(3, k)
        self.ctx = hast_amd.Context(k)
        self.ctx.table_reserve(2 * len(self.keys[0]) + 2)
        self.o = oracle_lib
        self.s03 = oracle_lib.ho_s03_new()
        for hap in (0, 1):
            text = b"\n".join(self.keys[hap]) + b"\n"
            assert self.ctx.table_insert_text(hap, text) == len(self.keys[hap])
            assert oracle_lib.ho_s03_load_text(self.s03, text, len(text), hap) == 0
        self.feeds = {}
        # the reference, once: (name, format, bytes, records or ERR, votes, carry bound)
        self.cases = []
        for name, fmt, data in rc.corpus(self.keys) + long_reads(self.keys):
            want = rc.read_file(fmt, data)
            self.cases.append((name, fmt, data, want, None if want == rc.ERR else self.hits([s for _, s in want]), rc.carry_bound(fmt, data)))

    def hits(self, seqs):
        out = np.zeros((len(seqs), 2), dtype=np.uint32)
        h0, h1 = C.c_uint32(), C.c_uint32()
        for i, s in enumerate(seqs):
            self.o.ho_s03_read_hits(self.s03, s, len(s), C.byref(h0), C.byref(h1))
            out[i] = (h0.value, h1.value)
        return out

    def feed(self, fmt, block):
        if (fmt, block) not in self.feeds:
            self.feeds[(fmt, block)] = ReadStream(self.ctx, fmt, block)
        return self.feeds[(fmt, block)]

    def run(self, fmt, block, data):
        """the file through the feed, a block ahead of the framer, host and device blocks in turn: (flags, names, votes, tail, views)"""
        f = self.feed(fmt, block)
        flags, names, votes, pending, consumed, views = 0, [], [], 0, 0, 0

        def step():
            nonlocal flags, consumed, views
            fl, c, _, nm, v = f.next()
            flags |= fl
            views += 1
            if not fl:
                names.extend(nm)
                votes.append(v)
                consumed += c
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
        tail = f.take_tail() if fmt == rc.FASTQ and not flags else b""
        return flags, names, np.concatenate(votes) if votes else np.zeros((0, 2), np.uint32), tail, views

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


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_fed_files_come_back_as_the_reference_readers_reads(rig, fmt, block):
    use = [c for c in rig.cases if c[1] == fmt and c[5] <= block]           # nothing to carry exceeds the block
    assert len(use) >= (3 if block < 700 else 15)
    hits = views = 0
    for name, _, data, want, want_votes, _ in use:
        flags, names, votes, tail, n_views = rig.run(fmt, block, data)
        views += n_views
        assert n_views == -(-len(data) // block) + 1, name
        if want == rc.ERR:                                                  # (a '>' header in the last, incomplete record is the host's to find)
            assert flags == hast_amd.RS_FORMAT_ERROR or (fmt == rc.FASTQ and flags == 0 and rc.read_file(fmt, tail) == rc.ERR), (name, block, flags)
            continue
        assert flags == 0, (name, block, flags)                             # never refused: the generator's condition
        n = len(names)
        if fmt == rc.FASTQ:                                                 # the end of the file is the host's: as the reader reads it
            assert tail == data[len(data) - len(tail):] and tail.count(b"\n") < 4, name
            assert rc.read_file(fmt, tail) == want[n:] and len(want) - n <= 1, name
        else:
            assert n == len(want), (name, block)
        assert names == [w[0] for w in want[:n]], (name, block)
        bad = np.nonzero((votes != want_votes[:n]).any(axis=1))[0]
        assert bad.size == 0, (name, block, int(bad[0]), votes[bad[0]].tolist(), want_votes[bad[0]].tolist(), len(want[bad[0]][1]))
        hits += int(votes.sum())
    # (a FASTQ record of 64 bytes has no room for a 31-mer: there the votes are all zero, on both sides)
    assert any(len(c[2]) > 2 * block for c in use) and views > len(use) and (hits > 100 or (block == 64 and hits > 0) or (block == 64 and fmt == rc.FASTQ and rig.k == 31))


def test_long_reads_straddle_views_and_copy_tiles(rig):
    """what the cases above rest on: the 20 000-base reads are in, they span views at 64-KB blocks, and their planted keys lie back
    to back, so every 4-KB boundary of the compacted bases and every view boundary falls inside a hit"""
    by = {c[0]: c for c in rig.cases}
    for name in ("fa_long", "fq_long"):
        _, _, data, want, votes, bound = by[name]
        longs = [i for i, (n, s) in enumerate(want) if len(s) == 20000]
        assert len(longs) >= 4 and len(data) > 2 * 65536 and bound <= 65536
        assert all(int(votes[i].sum()) >= 20000 // rig.k - 2 for i in longs)
    assert b"\n" not in by["fa_long"][2].split(b">long0\n")[1][:20000] and by["fa_long"][2].split(b">long1\n")[1][60:61] == b"\n"
    ends = [c for c in rig.cases if c[0] in ("fa_w63", "fa_w64", "fa_w65", "fa_n257", "fa_blank")]
    assert all(c[4].sum() > 20 for c in ends)                               # 60-, 70- and odd-column records: a key at every line end


@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_a_record_that_does_not_fit_is_refused_and_the_feed_goes_on(rig, fmt):
    rng = random.Random(5)
    recs = rc.records(rng, 20, (100,), rig.keys) + [(b"long one", rc.seq_with_plants(rng, 6000, rig.keys))] + rc.records(rng, 5, (100,), rig.keys)
    data = rc.fasta_text(rng, recs, 60) if fmt == rc.FASTA else rc.fastq_text(recs)
    flags, _, _, _, _ = rig.run(fmt, 2048, data)
    assert flags == hast_amd.RS_RECORD_TOO_LONG
    small = rc.fasta_text(rng, recs[:20], 60) if fmt == rc.FASTA else rc.fastq_text(recs[:20])
    flags, names, votes, _, _ = rig.run(fmt, 2048, small)                   # the same feed, the next file
    assert flags == 0 and names == [n for n, _ in recs[:20]] and np.array_equal(votes, rig.hits([s for _, s in recs[:20]]))
