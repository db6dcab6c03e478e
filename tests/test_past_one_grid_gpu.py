"""GPU tests of the tile loops past one grid and of the block scans past 1024 tiles (-m gpu).

The framing, routing, binning and conversion kernels walk tiles of 256 items with a grid the host caps at 2048 (1024 for the routing
class kernel and the name, insert and tally kernels), and one workgroup of 1024 scans the per-tile sums, each thread ceil(n / 1024) of
them.  At the block sizes the programs run with, most workgroups walk their loop many times and every scan thread takes a run of
tiles; the other GPU tests feed views so small that each loop body runs once per workgroup and each scan thread takes one value.  The
barriers that exist only for the second walk ("the sums of the tile before have been read"), the reuse of the LDS words, the clamped
lo / hi of the scans and the span copies' second lap over their output are what these tests are for.

Every family goes through its public API once with a view just past its caps (tests/past_grid_corpus.py: N2 = 524 609 items = 2050
tiles, N1 = 262 465 for the kernels capped at 1024; B = 8 388 608 output bytes for the span copies) and is compared, every output
byte and counter, with the host model its own tests use.  Each test asserts on what the API reports that the thresholds were passed;
tests/test_grid_caps_cpu.py pins the caps to the sources."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import hast_amd
from hast_amd import ReadStream, SQ_FA_LAST, TxConverter, TxMap, TxState
from tests import past_grid_corpus as pg
from tests import rb_model as rb
from tests import rs_corpus as rc
from tests import test_bf_gpu as bf_gpu
from tests import test_fq_gpu as fq_gpu
from tests import test_names_gpu as names_gpu
from tests import test_sq_fasta_gpu as sqfa_gpu
from tests import test_sq_gpu as sq_gpu
from tests import test_tx_gpu as tx_gpu
from tests import tx_model as tm
from tests.test_names_gpu import one_ctx, world  # noqa: F401  (module fixtures)

pytestmark = pytest.mark.gpu
N2, N1, B, TILE = pg.N2, pg.N1, pg.B, pg.TILE


def tiles(n, per=TILE):
    return -(-n // per)


def assert_past_one_grid(items, cap=pg.GRID_CAP, passes=2):
    """`items` (what the API reported) make some workgroup of a grid of `cap` walk its tile loop `passes` times, and the scan of the
    tile sums takes more than one value per thread"""
    assert tiles(items) > (passes - 1) * cap, (items, cap, passes)
    assert tiles(items) > pg.SCAN_THREADS


# ---- stage 03: the read stream and its bins (rs_kernels.hip) ------------------------------------------------------------------
class RsWorld:
    """keys in the table and in the oracle; the FASTQ and the FASTA input with the reference reader's records, the oracle's votes for
    every one of them and the bins' classes -- computed once"""

    def __init__(self, oracle_lib):
        self.keys = pg.keys()
        self.o = oracle_lib
        self.s03 = oracle_lib.ho_s03_new()
        self.ctx = hast_amd.Context(pg.K)
        self.ctx.table_reserve(sum(pg.N_KEYS) + 2)
        for hap in (0, 1):
            text = b"\n".join(self.keys[hap]) + b"\n"
            assert self.ctx.table_insert_text(hap, text) == len(self.keys[hap])
            assert oracle_lib.ho_s03_load_text(self.s03, text, len(text), hap) == 0
        self.memo = {}
        self.feeds = {}
        self.fq_recs, self.fq_tail = pg.rs_fastq(N2, self.keys)
        self.fq_want = rc.read_file(rc.FASTQ, b"".join(self.fq_recs))
        self.fq_votes = self.hits([s for _, s in self.fq_want])
        self.fa_data, self.fa_info = pg.rs_fasta(N2 + 1, self.keys)
        self.fa_want = rc.read_file(rc.FASTA, self.fa_data)
        self.fa_votes = self.hits([s for _, s in self.fa_want])

    def hits(self, seqs):
        """ho_s03_read_hits of every sequence (asked once per distinct sequence: the votes of a read are a function of its bases)"""
        h0, h1 = C.c_uint32(), C.c_uint32()
        memo, out = self.memo, []
        for s in seqs:
            v = memo.get(s)
            if v is None:
                self.o.ho_s03_read_hits(self.s03, s, len(s), C.byref(h0), C.byref(h1))
                v = memo[s] = (h0.value, h1.value)
            out.append(v)
        return np.array(out, dtype=np.uint32).reshape(-1, 2)

    def feed(self, fmt, block):
        if fmt not in self.feeds:
            self.feeds[fmt] = ReadStream(self.ctx, fmt, block)
        assert self.feeds[fmt].block == block
        return self.feeds[fmt]

    def run(self, fmt, block, data, mode=0):
        """the input as ONE block and the empty last block behind it -> the two views (next() or, mode 1 / 2, next_binned()), the tail"""
        f = self.feed(fmt, block)
        assert len(data) <= block
        f.set_bins(mode, *pg.N_KEYS)
        views = []
        for chunk, last in ((data, False), (b"", True)):
            f.submit(chunk, last=last)
            views.append(f.next_binned() if mode else f.next())
        tail = f.take_tail() if fmt == rc.FASTQ else b""
        f.set_bins(0, 0, 0)
        return views, tail

    def close(self):
        for f in self.feeds.values():
            f.close()
        self.o.ho_s03_free(self.s03)
        self.ctx.close()


@pytest.fixture(scope="module")
def rs_world(oracle_lib):
    w = RsWorld(oracle_lib)
    yield w
    w.close()


RS_FQ_BLOCK, RS_FA_BLOCK = 32 << 20, 20 << 20


def both_columns_in_every_tile(votes):
    whole = votes[:votes.shape[0] // TILE * TILE].reshape(-1, TILE, 2).sum(axis=1)
    return bool((whole > 0).all())


@pytest.mark.parametrize("n", pg.EDGES + (N2,))
def test_rs_fastq_view_past_one_grid(rs_world, n):
    """k_rs_records, k_rs_scan_names, k_rs_names: 2048 tiles exactly (no second walk), one record more, and 2050 tiles"""
    w = rs_world
    complete = b"".join(w.fq_recs[:n])
    (first, last), tail = w.run(rc.FASTQ, RS_FQ_BLOCK, complete + w.fq_tail)
    flags, consumed, bases, names, votes = first
    assert flags == 0 and last[0] == 0 and len(last[3]) == 0 and last[1] == 0
    assert len(names) == n == votes.shape[0]                                # what the API reports: the records of the view
    if n > pg.EDGES[0]:
        assert_past_one_grid(len(names))
    else:
        assert tiles(len(names)) == pg.GRID_CAP
    assert tiles(consumed, pg.NL_TILE) > pg.SCAN_THREADS                     # k_rs_scan over the newline tiles: more than one a thread
    assert consumed == len(complete) and tail == w.fq_tail and rc.read_file(rc.FASTQ, tail) == [(b"tail x", b"ACGTAC")]
    assert names == [nm for nm, _ in w.fq_want[:n]]
    bad = np.nonzero((votes != w.fq_votes[:n]).any(axis=1))[0]
    assert bad.size == 0, (int(bad[0]), votes[bad[0]].tolist(), w.fq_votes[bad[0]].tolist())
    assert bases == sum(len(s) for _, s in w.fq_want[:n])
    assert both_columns_in_every_tile(votes)
    assert sum(len(s) < pg.K for _, s in w.fq_want[:n]) > n // 4             # a third of the reads is too short for any vote


def test_rs_fasta_view_past_one_grid(rs_world):
    """k_rs_lines, k_rs_scan_lines, k_rs_line_dst over more than 4096 line tiles, k_rs_records / k_rs_names over 2050 record tiles,
    and k_rs_copy past B output bytes with bias != 0"""
    w = rs_world
    data, info = w.fa_data, w.fa_info
    (first, last), _ = w.run(rc.FASTA, RS_FA_BLOCK, data)
    assert first[0] == 0 and last[0] == 0
    names, votes = first[3] + last[3], np.concatenate([first[4], last[4]])
    n = len(first[3])
    assert n == N2 and len(last[3]) == 1                                    # the last record is complete only at the end of the file
    assert_past_one_grid(n)
    lines = data[:first[1]].count(b"\n")
    assert lines >= 2 * N2 and tiles(lines) > 2 * pg.GRID_CAP               # the line kernels: a third walk
    assert first[1] == data.rindex(b">") and first[1] + last[1] == len(data)
    assert names == [nm for nm, _ in w.fa_want]
    bad = np.nonzero((votes != w.fa_votes).any(axis=1))[0]
    assert bad.size == 0, (int(bad[0]), votes[bad[0]].tolist(), w.fa_votes[bad[0]].tolist(), len(w.fa_want[bad[0]][1]))
    assert first[2] == sum(len(s) for _, s in w.fa_want[:n]) and last[2] == len(w.fa_want[n][1])
    # the copy: more than one lap of 2048 tiles of 4 KB, the byte at B inside the long read's one line, sequence bytes in front of
    # the first header
    assert first[2] > B + pg.COPY_TILE
    assert 0 < B - info["long_at"] < info["long_len"] - 1
    at = next(i for i, (nm, _) in enumerate(w.fa_want) if nm.startswith(b"long read"))
    assert sum(len(s) for _, s in w.fa_want[:at]) == info["long_at"] and len(w.fa_want[at][1]) == info["long_len"]
    assert int(w.fa_votes[at].sum()) > info["long_len"] // (pg.K + 1)        # keys back to back: the 4-KB edges of the copy lie inside hits
    head = data[:data.index(b">")]
    assert sum(len(l) for l in head.split(b"\n")) > 0 and b"\n\n" in head
    # blank lines inside records; records whose lines reach over a tile edge, a key across every line end
    assert data.count(b"\n\n") > N2 // 200
    assert len(info["straddlers"]) >= N2 // 8191 - 1
    all_lines = data.split(b"\n")
    hdr = {l: j for j, l in enumerate(all_lines) if l.startswith(b">multi")}
    record_of = {nm: i for i, (nm, _) in enumerate(w.fa_want)}
    for r in info["straddlers"]:
        j = end = hdr[b">multi %d" % r]
        while not all_lines[end + 1].startswith(b">"):
            end += 1
        assert end - j >= 4 and j // TILE != end // TILE, r                  # header and last line in different tiles of 256 lines
        assert int(w.fa_votes[record_of[b"multi %d" % r]].sum()) >= end - j - 1, r    # a hit across every line end
    assert both_columns_in_every_tile(votes)


def bins_of(views):
    got = [b"".join(v[5][c] for v in views) for c in range(3)]
    raw = [sum(v[6][c] for v in views) for c in range(3)]
    count = [sum(v[7][c] for v in views) for c in range(3)]
    return got, raw, count


def classes_in_every_tile(cls):
    a = np.array(cls[:len(cls) // TILE * TILE]).reshape(-1, TILE)
    return all(bool((a == c).any(axis=1).all()) for c in range(3))


@pytest.mark.parametrize("mode", (1, 2), ids=("plain", "gzip"))
def test_rb_fastq_bins_past_one_grid(rs_world, mode):
    """k_rb_sums, k_rb_scan (over 3 x 2050 entries), k_rb_place over 2050 tiles; k_rb_copy past B routed bytes; mode 2: each run one
    gzip member of the plain run"""
    w = rs_world
    complete = b"".join(w.fq_recs)
    want_runs, want_count, cls = rb.runs(rc.FASTQ, complete, w.fq_votes, *pg.N_KEYS)
    views, tail = w.run(rc.FASTQ, RS_FQ_BLOCK, complete + w.fq_tail, mode)
    assert all(v[0] == 0 for v in views) and tail == w.fq_tail
    got, raw, count = bins_of(views)
    assert sum(count) == len(views[0][3]) == N2
    assert_past_one_grid(sum(count))
    assert tiles(3 * tiles(sum(count)), pg.SCAN_THREADS) >= 7                # k_rb_scan: seven entries a thread
    assert sum(raw) == len(complete) > B + pg.COPY_TILE                      # the copy's second lap
    assert count == want_count and raw == [len(r) for r in want_runs]
    assert min(count) > N2 // 4 and classes_in_every_tile(cls)
    if mode == 2:
        for c in range(3):
            z = zlib.decompressobj(16 + zlib.MAX_WBITS)
            plain = z.decompress(got[c])
            assert z.eof and z.unused_data == b"" and got[c][:4] == b"\x1f\x8b\x08\x00", c
            got[c] = plain
    for c in range(3):
        assert got[c] == want_runs[c], (c, len(got[c]), len(want_runs[c]))
    assert np.array_equal(views[0][4], w.fq_votes)


def test_rb_fasta_bins_past_one_grid(rs_world):
    w = rs_world
    want_runs, want_count, cls = rb.runs(rc.FASTA, w.fa_data, w.fa_votes, *pg.N_KEYS)
    views, _ = w.run(rc.FASTA, RS_FA_BLOCK, w.fa_data, 1)
    assert all(v[0] == 0 for v in views)
    got, raw, count = bins_of(views)
    assert views[0][7] and sum(views[0][7]) == len(views[0][3]) == N2
    assert_past_one_grid(sum(views[0][7]))
    assert sum(views[0][6]) > B + pg.COPY_TILE
    assert count == want_count and raw == [len(r) for r in want_runs] and sum(raw) == len(w.fa_data) - w.fa_data.index(b">")
    assert min(count) > N2 // 4 and classes_in_every_tile(cls)
    for c in range(3):
        assert got[c] == want_runs[c], (c, len(got[c]), len(want_runs[c]))


# ---- stage 02: stLFR pairs to 10x (tx_kernels.hip) ---------------------------------------------------------------------------
def test_tx_pairs_past_one_grid():
    """k_tx_keys, k_tx_sizes, k_tx_copy over 2050 tiles of pairs, k_tx_scan_kept / k_tx_scan_out with three tiles a thread, k_tx_scan
    over more than 1024 newline tiles a side; N passes from six to seven digits inside the step"""
    r1, r2 = pg.tx_pairs(N2)
    used = 999_000
    want1, want2, _, want_used, want_headers = tm.convert(tm.parse_map(tx_gpu.MAP), r1[:r1.rindex(b"@part")], r2[:r2.rindex(b"@part")], used=used, headers=used + 5)
    pad = tx_gpu.PAD
    ctx = hast_amd.Context(21)
    try:
        with TxMap(tx_gpu.MAP) as m, TxConverter(ctx, m, max(len(r1), len(r2))) as conv:
            st_h = TxState(used, used + 5)
            host = m.pair_host(r1, r2, False, st_h)
            d_in = [ctx.to_device(np.frombuffer(r, np.uint8)) for r in (r1, r2)]
            need = [len(want1), len(want2)]
            d_out = [ctx.alloc(n + pad + 64) for n in need]
            for s in range(2):
                ctx.memset(d_out[s], tx_gpu.CANARY, need[s] + pad)
            ctx.sync()
            st_d = TxState(used, used + 5)
            res = conv.pair_device(d_in[0], len(r1), d_in[1], len(r2), st_d, d_out[0], need[0] + pad, d_out[1], need[1] + pad)
            got = [ctx.to_host(d_out[s], (need[s] + pad,), np.uint8) for s in range(2)]
            for d in d_in + d_out:
                ctx.free(d)
    finally:
        ctx.close()
    assert res.pairs == N2 and tuple(res.lines) == (r1.count(b"\n"), r2.count(b"\n"))
    assert_past_one_grid(res.pairs)
    assert min(res.consumed1, res.consumed2) // pg.NL_TILE > pg.SCAN_THREADS
    assert tx_gpu.fields(res) == tx_gpu.fields(host[2]), (tx_gpu.fields(res), tx_gpu.fields(host[2]))
    assert (st_d.used, st_d.headers) == (st_h.used, st_h.headers) == (want_used, want_headers)
    assert (res.consumed1, res.consumed2) == (r1.rindex(b"@part"), r2.rindex(b"@part")) and tuple(res.out_bytes) == tuple(need)
    assert used < 999_999 < used + res.used and N2 // 3 < res.used < N2 - N2 // 4       # a decimal width is crossed; kept and dropped mix
    for s, want in enumerate((want1, want2)):
        w = np.frombuffer(want, np.uint8)
        assert np.array_equal(got[s][:need[s]], w), ("side", s, "first difference at", int(np.argmax(got[s][:need[s]] != w)))
        assert np.all(got[s][need[s]:] == tx_gpu.CANARY), ("side", s, "written behind its end")
        assert host[s] == want
    # whole tiles kept and whole tiles dropped, as the generator says
    in_map = tm.parse_map(tx_gpu.MAP)
    slot = np.array([tm.key_of(l) in in_map for l in r1.split(b"\n")[0:4 * N2:4]])
    per_tile = slot[:N2 // TILE * TILE].reshape(-1, TILE).sum(axis=1)
    assert (per_tile == TILE).sum() >= 100 and (per_tile == 0).sum() >= 100 and ((per_tile > 40) & (per_tile < 216)).sum() > 1500


# ---- stage 00: the framers (sq_kernels.hip, sq_fasta_kernels.hip) ---------------------------------------------------------
@pytest.fixture(scope="module")
def sq_rig():
    r = sq_gpu.Rig(24 << 20)
    yield r
    r.close()


sq_model = sq_gpu.model
sqfa_model = sqfa_gpu.model


@pytest.fixture(scope="module")
def sq_records():
    return pg.sq_fastq(N2)


@pytest.mark.parametrize("n", pg.EDGES + (N2,))
def test_sq_fastq_view_past_one_grid(sq_rig, sq_model, sq_records, n):
    """k_sq_records, k_sq_scan_out, k_sq_copy: 2048 tiles exactly, one record more, 2050 tiles; the start of a record behind them"""
    arr = sq_gpu.as_array(b"".join(sq_records[:n]) + b"@part\nAC")
    sq_rig.upload(arr, 5)
    got, written = sq_rig.frame(24 << 20, 5, arr.size, 3)
    want, want_bytes = sq_model(arr)
    sq_gpu.check(got, written, want, want_bytes, n)
    assert got["flags"] == 0 and got["records"] == n and got["consumed"] == arr.size - 8
    if n > pg.EDGES[0]:
        assert_past_one_grid(got["records"])
    else:
        assert tiles(got["records"]) == pg.GRID_CAP
    assert tiles(got["consumed"], pg.NL_TILE) > pg.SCAN_THREADS


def test_sq_fasta_view_past_one_grid(sq_model, sqfa_model):
    """k_sqfa_lines, k_sqfa_scan_lines, k_sqfa_line_dst over 2050 line tiles; k_sqfa_copy past B output bytes"""
    arr = sqfa_gpu.as_array(pg.sq_fasta(N2))
    rig = sqfa_gpu.Rig(24 << 20)
    try:
        rig.upload(arr, 9)
        got, written = rig.frame(24 << 20, 9, arr.size, SQ_FA_LAST, 6)
    finally:
        rig.close()
    want, want_bytes = sqfa_model(arr, SQ_FA_LAST)
    sqfa_gpu.check(got, written, want, want_bytes, "past one grid")
    lines = int((arr == 10).sum())
    assert got["flags"] == 0 and got["consumed"] == arr.size and lines >= N2 and lines < N2 + 16
    assert_past_one_grid(lines)
    assert got["out_bytes"] > B + pg.COPY_TILE and got["records"] > N2 // 8
    is_header = np.array([l[:1] == b">" for l in arr.tobytes().split(b"\n")[:lines]])
    assert got["records"] == int(is_header.sum())
    assert is_header[:lines // TILE * TILE].reshape(-1, TILE).any(axis=1).all()          # tile_h != 0 in every tile


# ---- stage 01: routing, names, tallies (fq_kernels.hip) ----------------------------------------------------------------------
def test_fq_routing_past_one_grid():
    """k_route_class (1024 workgroups: three walks), k_route_scan (four class rows a scan: nine entries a thread), k_route_copy and k_fq_records
    (2048 workgroups: two walks) on one block"""
    data, cls_of = pg.route_fastq(N2)
    want, want_dropped = fq_gpu._awk_route(data, cls_of)
    block = 16 << 20
    assert len(data) <= block
    got, dropped, st = fq_gpu.route_through_abi(data, cls_of, block, block, 1, random.Random(1))
    records = [g.count(b"\n") // 4 for g in got]                            # from the runs the device handed over
    assert sum(records) == N2
    assert_past_one_grid(sum(records), pg.NAME_GRID_CAP, 3)
    assert_past_one_grid(sum(records), pg.GRID_CAP, 2)
    assert min(records) > N2 // 5
    for c in range(4):
        assert got[c] == want[c], (c, len(got[c]), len(want[c]))
    assert dropped == [] == want_dropped and st == {"host_blocks": 0, "blocks": 1}
    heads = data.split(b"\n")[0:4 * (N2 // TILE * TILE):4]
    cls = np.array([0 if h.count(b"#") == 0 or b"#0_0_0/" in h else cls_of[h.split(b"#")[1].split(b"/")[0]] for h in heads]).reshape(-1, TILE)
    assert all(bool((cls == c).any(axis=1).all()) for c in range(4))


def test_names_insert_second_round():
    """k_names_insert with n_round = 2: barcode lists of N1 texts go into the routing table in one call; every record carries a barcode
    of its own, so one text the table did not learn hands the block to the host"""
    data, cls_of = pg.route_fastq_many_lists(N1)
    want, want_dropped = fq_gpu._awk_route(data, cls_of)
    block = 8 << 20
    assert len(data) <= block
    got, dropped, st = fq_gpu.route_through_abi(data, cls_of, block, block, 1, random.Random(2))
    assert dropped == [] == want_dropped and st == {"host_blocks": 0, "blocks": 1}
    for c in range(4):
        assert got[c] == want[c], (c, len(got[c]), len(want[c]))
    texts = {h.split(b"#")[1].split(b"/")[0] for g in got for h in g.split(b"\n")[0::4] if h}
    assert len(texts) == N1 and tiles(len(texts), 256) > pg.NAME_GRID_CAP     # as many listed texts found as the device routed records
    assert got[0] == b"" and min(len(g) for g in got[1:]) > len(data) // 4


def test_names_second_round_of_the_claim_kernel(world, one_ctx, monkeypatch):  # noqa: F811
    """k_fq_name_claim with n_round = 3 (1024 workgroups x 256 lanes a round) on one block of N2 records, k_fq_records over 2050 tiles:
    texts first met in round 0 come again in rounds 1 and 2 and must resolve to the same id; rounds 1 and 2 bring texts of their own,
    each several times"""
    monkeypatch.setenv("HAST_FQ_HOST_RECORDS", str(N2 + 1024))
    per_round = pg.NAME_GRID_CAP * 256
    rng = np.random.default_rng(20261020)
    n_a, n_b, n_c = 2000, 900, 40
    seq = np.concatenate([rng.integers(0, n_a, per_round), rng.integers(0, n_a + n_b, per_round), rng.integers(0, n_a + n_b + n_c, N2 - 2 * per_round)])
    seq[-n_c * 3:] = n_a + n_b + np.arange(n_c * 3) % n_c                    # every text of the last round is there, three times
    n_short = n_a + n_b + n_c
    seq[rng.choice(N2, N2 // 64, replace=False)] = n_short + rng.integers(0, names_gpu.N_LONG, N2 // 64)
    seq[-n_c * 3:] = n_a + n_b + np.arange(n_c * 3) % n_c
    inp = names_gpu.Input(n_short, seq, world["pool"], rng)
    rounds = [set(seq[r * per_round:(r + 1) * per_round].tolist()) - set(range(n_short, n_short + names_gpu.N_LONG)) for r in range(3)]
    assert len(rounds[0] & rounds[1]) > 1500 and len(rounds[1] - rounds[0]) > 500 and len(rounds[2] - rounds[1] - rounds[0]) == n_c
    assert len(rounds[2] & rounds[0]) > 50
    ck, count, limit = names_gpu.run_stream(world, [one_ctx], inp, 65536, [(0, N2)], 40 << 20)
    assert ck.at == N2                                                       # the records the stream reported, block by block
    assert tiles(ck.at, 256) > 2 * pg.NAME_GRID_CAP and tiles(ck.at) > pg.GRID_CAP
    assert limit == 65536 and count == n_short and ck.short_left == 0
    assert ck.host_named == int(inp.is_long[inp.seq].sum()) > 0


def test_tally_second_round(monkeypatch):
    """k_fq_field2, k_fq_name_claim and k_tally_add past 1024 workgroups x 256 lanes on one block of N1 records"""
    monkeypatch.setenv("HAST_FQ_HOST_RECORDS", str(N1 + 1024))
    data = pg.tally_fastq(N1)
    block = 8 << 20
    assert len(data) <= block
    run, on_device, st = bf_gpu.run_one(data, 1, block, block)
    assert run.st["blocks"] == 1 and st["records"] == N1
    assert tiles(st["records"], 256) > pg.NAME_GRID_CAP
    assert st["counted"] > N1 - N1 // 50 and st["left"] >= N1 // 4001 and st["nofield"] > N1 // 200
    assert on_device[0][b"0_0_0"] > N1 // 4 and len(on_device[0]) > 390
