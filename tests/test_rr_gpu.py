"""GPU test of stage 03's rows made on the device (rr_kernels.hip; rules: hast_amd/csrc/rr_core.h).  The direct entry
hast_rs_rows_device over crafted names and votes -- every tile boundary, more than 1024 tiles, names from nothing to kilobytes in one
call, votes and set sizes up to 2^32 - 1, and once more tiles than the capped grid has workgroups -- against the restatement of tests/rr_model.py, byte for byte; and the feed
(hast_rs_set_rows / hast_rs_next_rows) over every file of tests/rs_corpus.py against the model's rows of what hast_rs_next hands out
for the same file, with the views whose rows outgrow the feed's buffer coming back for the host."""
import random

import numpy as np
import pytest

import hast_amd
from hast_amd import ReadStream
from tests import past_grid_corpus as pg
from tests import rr_model as rr
from tests import rs_corpus as rc

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 256 * 1024 + 1)
NAME_LENS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 5000)
M32 = 2 ** 32 - 1
TOTALS = ((128, 37), (1, M32), (M32, 1))
BLOCKS = (64, 700, 4096)
N0, N1 = 40, 37
GUARD = 64


def crafted(n, seed):
    """names (lengths of NAME_LENS mixed; among many reads the kilobyte names are rare, so that the test stays small) and votes: zeros,
    ties, one-sided, odd votes (ties of the last digit over 128), the largest"""
    rng = random.Random(seed)
    alphabet = bytes(range(33, 127))
    names, votes = [], np.zeros((n, 2), dtype=np.uint32)
    for i in range(n):
        k = NAME_LENS[i % len(NAME_LENS)]
        if k == 5000 and n > 1000 and i % 4090 != 9:
            k = 7
        names.append(bytes(rng.choice(alphabet) for _ in range(min(k, 70))) * (k // 70 + 1))
        names[-1] = names[-1][:k]
        a = rng.randint(1, 300)
        votes[i] = ((0, 0), (a, a), (a, 0), (0, a), (2 * a + 1, 1), (1, 2 * a + 1), (M32, rng.randint(0, M32)), (rng.randint(0, M32), M32),
                    (rng.randint(0, M32), rng.randint(0, M32)), (a, max(0, a - 1)))[rng.randrange(10)]
    return names, votes


@pytest.fixture(scope="module")
def ctx():
    with hast_amd.Context(21) as c:
        yield c


@pytest.fixture(scope="module")
def inputs():
    """per size: names, votes and the packed arrays; the model's rows per pair of totals are worked out once, on first use"""
    out = {}
    for n in SIZES:
        names, votes = crafted(n, 100 + n)
        off = np.zeros(n + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
        out[n] = (names, votes, off, np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8), {})     # (never an empty upload)
    return out


def model(inputs, n, totals):
    names, votes, _, _, cache = inputs[n]
    if totals not in cache:
        cache[totals] = rr.rows(names, votes, *totals)
    return cache[totals]


def run_direct(ctx, inputs, n, totals, cap=None, fill=0xAA):
    """(bytes, count, what the output buffer holds: cap bytes and the guard behind them)"""
    names, votes, off, packed, _ = inputs[n]
    want = model(inputs, n, totals)[0]
    cap = len(want) if cap is None else cap
    d_names, d_off, d_votes = ctx.to_device(packed), ctx.to_device(off), ctx.to_device(votes if n else np.zeros((1, 2), np.uint32))
    d_out = ctx.alloc(cap + GUARD)
    ctx.memset(d_out, fill, cap + GUARD)
    ctx.sync()
    try:
        nbytes, count = hast_amd.rs_rows_device(ctx, d_names, d_off, d_votes, n, totals[0], totals[1], d_out, cap)
        return nbytes, count, ctx.to_host(d_out, (cap + GUARD,), np.uint8).tobytes()
    finally:
        for d in (d_names, d_off, d_votes, d_out):
            ctx.free(d)


def test_the_crafted_inputs_hold_what_the_checks_rest_on(inputs):
    for n in SIZES:
        names, votes, off, _, _ = inputs[n]
        if n >= 63:
            assert {len(x) for x in names} >= set(NAME_LENS), n
            for totals in TOTALS:
                assert min(model(inputs, n, totals)[1]) > 0, (n, totals)
    assert int(inputs[SIZES[-1]][1].max()) == M32 and -(-SIZES[-1] // 256) > 1024
    odd = [int(v0) for v0, v1 in inputs[257][1] if v0 % 2 and v0 < 600 and v1 <= 1]
    assert len(odd) > 10                                                          # odd votes over 128: exact halves of the sixth digit


@pytest.mark.parametrize("totals", TOTALS)
@pytest.mark.parametrize("n", SIZES)
def test_rows_of_crafted_arrays_are_the_models(ctx, inputs, n, totals):
    want, count, _ = model(inputs, n, totals)
    nbytes, got_count, buf = run_direct(ctx, inputs, n, totals)
    assert nbytes == len(want) and got_count == count, (n, totals, nbytes, len(want), got_count, count)
    if buf[:len(want)] != want:
        at = next(i for i in range(len(want)) if buf[i] != want[i])
        assert False, (n, totals, at, buf[max(0, at - 40):at + 40], want[max(0, at - 40):at + 40])
    assert buf[len(want):] == b"\xaa" * GUARD, (n, totals)


def sliced(n, seed):
    """names of 0 to 65 bytes cut out of one random buffer at random places (no byte of them drawn one by one: half a million names in
    a second), votes of crafted()'s ten kinds"""
    rng = np.random.default_rng(seed)
    soup = rng.integers(33, 127, size=1 << 16, dtype=np.uint8).tobytes()
    at, lens = rng.integers(0, len(soup) - 65, size=n).tolist(), rng.integers(0, 66, size=n).tolist()
    names = [soup[a:a + k] for a, k in zip(at, lens)]
    a, kind = rng.integers(1, 301, size=n), rng.integers(0, 10, size=n)
    r0, r1, zero, one, top = rng.integers(0, M32 + 1, size=n), rng.integers(0, M32 + 1, size=n), 0 * a, 0 * a + 1, 0 * a + M32
    votes = np.zeros((n, 2), dtype=np.uint32)
    votes[:, 0] = np.choose(kind, [zero, a, a, zero, 2 * a + 1, one, top, r0, r0, a])
    votes[:, 1] = np.choose(kind, [zero, a, zero, a, one, 2 * a + 1, r1, top, r1, a - 1])
    return names, votes


@pytest.fixture(scope="module")
def past_grid():
    """past_grid_corpus.N2 rows, in the layout of `inputs`"""
    n = pg.N2
    names, votes = sliced(n, 4100)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
    return {n: (names, votes, off, np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8), {})}


def test_rows_past_one_grid_are_the_models(ctx, past_grid):
    """2050 tiles of 256 rows: workgroups 0 and 1 of the capped grids walk a second tile, the last tile is partial; the block scan of the
    tiles' sums gives its threads three tiles each"""
    n, totals = pg.N2, TOTALS[0]
    names, votes = past_grid[n][:2]
    tiles = -(-n // pg.TILE)
    assert tiles > pg.GRID_CAP and tiles > 2 * pg.SCAN_THREADS and {len(x) for x in names} == set(range(66)) and len(set(names[:5000])) > 4900
    want, count, sizes = model(past_grid, n, totals)
    assert min(count) > 1000
    nbytes, got_count, buf = run_direct(ctx, past_grid, n, totals)
    assert nbytes == len(want) and got_count == count, (nbytes, len(want), got_count, count)
    same = buf[:len(want)] == want
    if not same:
        at = int(np.flatnonzero(np.frombuffer(buf, dtype=np.uint8, count=len(want)) != np.frombuffer(want, dtype=np.uint8))[0])
        row = int(np.searchsorted(np.cumsum(sizes), at, side="right"))
        pytest.fail("the rows differ at offset %d: row %d, tile %d\n got  %r\n want %r" % (at, row, row // pg.TILE, buf[max(0, at - 40):at + 40], want[max(0, at - 40):at + 40]))
    assert buf[len(want):] == b"\xaa" * GUARD


@pytest.mark.parametrize("n", (1, 257, 256 * 1024 + 1))
def test_a_cap_one_byte_short_writes_nothing_and_says_what_is_needed(ctx, inputs, n):
    want = model(inputs, n, TOTALS[0])[0]
    with pytest.raises(hast_amd.HastError) as e:
        run_direct(ctx, inputs, n, TOTALS[0], cap=len(want) - 1)
    assert e.value.status == 9 and e.value.needed == len(want)                   # HAST_ERR_UNSUPPORTED
    names, votes, off, packed, _ = inputs[n]
    d_names, d_off, d_votes = ctx.to_device(packed), ctx.to_device(off), ctx.to_device(votes)
    d_out = ctx.alloc(len(want) + GUARD)
    ctx.memset(d_out, 0x55, len(want) + GUARD)
    ctx.sync()
    with pytest.raises(hast_amd.HastError):
        hast_amd.rs_rows_device(ctx, d_names, d_off, d_votes, n, TOTALS[0][0], TOTALS[0][1], d_out, len(want) - 1)
    assert ctx.to_host(d_out, (len(want) + GUARD,), np.uint8).tobytes() == b"\x55" * (len(want) + GUARD)
    nbytes, _ = hast_amd.rs_rows_device(ctx, d_names, d_off, d_votes, n, TOTALS[0][0], TOTALS[0][1], d_out, len(want))     # ... and with the byte it fits
    assert nbytes == len(want) and ctx.to_host(d_out, (len(want),), np.uint8).tobytes() == want
    for d in (d_names, d_off, d_votes, d_out):
        ctx.free(d)


def test_a_set_size_of_zero_is_refused(ctx, inputs):
    names, votes, off, packed, _ = inputs[65]
    d_names, d_off, d_votes, d_out = ctx.to_device(packed), ctx.to_device(off), ctx.to_device(votes), ctx.alloc(8192)
    ctx.memset(d_out, 0x55, 8192)
    ctx.sync()
    for totals in ((0, 37), (40, 0), (0, 0)):
        with pytest.raises(hast_amd.HastError) as e:
            hast_amd.rs_rows_device(ctx, d_names, d_off, d_votes, 65, totals[0], totals[1], d_out, 8192)
        assert e.value.status == 1 and e.value.needed == 0                       # HAST_ERR_INVALID
    assert ctx.to_host(d_out, (8192,), np.uint8).tobytes() == b"\x55" * 8192
    for d in (d_names, d_off, d_votes, d_out):
        ctx.free(d)


# ---- the feed ---------------------------------------------------------------------------------------------------------------------
class Rig:
    def __init__(self):
        keys = rc.make_keys(3, 21)
        self.keys = [keys[0][:N0], keys[1][:N1]]
        self.ctx = hast_amd.Context(21)
        self.ctx.table_reserve(N0 + N1 + 2)
        for hap in (0, 1):
            assert self.ctx.table_insert_text(hap, b"\n".join(self.keys[hap]) + b"\n") == len(self.keys[hap])
        self.files = [(name, fmt, data, rc.carry_bound(fmt, data)) for name, fmt, data in rc.corpus(self.keys)]
        self.feeds, self.results = {}, {}

    def feed(self, fmt, block):
        if (fmt, block) not in self.feeds:
            self.feeds[(fmt, block)] = ReadStream(self.ctx, fmt, block)
        return self.feeds[(fmt, block)]

    def run(self, fmt, block, data, rows, binned):
        """the file through the feed, a block ahead of the framer, host and device blocks in turn.  Per view: (flags, consumed, names,
        votes, runs or None, text or None, count or None, on_host)"""
        f = self.feed(fmt, block)
        views, pending = [], 0

        def step():
            if rows:
                out = f.next_rows(binned=binned)
                fl, c, _, nm, v = out[:5]
                views.append((fl, c, nm, v, out[5] if binned else None) + tuple(out[-3:]))
            elif binned:
                fl, c, _, nm, v, runs, _, _ = f.next_binned()
                views.append((fl, c, nm, v, runs, None, None, False))
            else:
                fl, c, _, nm, v = f.next()
                views.append((fl, c, nm, v, None, None, None, False))
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

    def all_passes(self, fmt, block):
        """every file of the format that the block takes: hast_rs_next, hast_rs_next_rows, and both with the plain bins on; once"""
        key = (fmt, block)
        if key not in self.results:
            f = self.feed(fmt, block)
            res = {}
            for name, ffmt, data, bound in self.files:
                if ffmt != fmt or bound > block:
                    continue
                f.set_rows(0, 0, 0)
                f.set_bins(0, 0, 0)
                plain = self.run(fmt, block, data, False, False)
                f.set_bins(1, N0, N1)
                bins = self.run(fmt, block, data, False, True)
                f.set_rows(1, N0, N1)
                both = self.run(fmt, block, data, True, True)
                f.set_bins(0, 0, 0)
                rows = self.run(fmt, block, data, True, False)
                res[name] = (plain, rows, bins, both)
            f.set_rows(0, 0, 0)
            self.results[key] = res
        return self.results[key]

    def close(self):
        for f in self.feeds.values():
            f.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_the_feeds_rows_are_the_models_rows_of_what_hast_rs_next_gives(rig, fmt, block):
    res = rig.all_passes(fmt, block)
    assert len(res) >= (3 if block < 700 else 15)
    with_host, without_host, classes = set(), set(), [0, 0, 0]
    for name, (plain, rows, bins, both) in res.items():
        for got in (rows, both):
            assert got[1] == plain[1] and len(got[0]) == len(plain[0]), (name, block)
            joined, want_all = [], []
            for a, b in zip(plain[0], got[0]):
                assert a[0] == b[0] and a[1] == b[1], (name, block)                     # flags, consumed
                if a[0]:
                    assert b[5] in (b"", None) and b[6] == [0, 0, 0] and not b[7], (name, block)
                    continue
                want, count, _ = rr.rows(a[2], a[3], N0, N1)
                want_all.append(want)
                assert b[6] == count, (name, block)
                if b[7]:                                                                # the rows did not fit: names and votes, as ever
                    assert b[5] is None and len(want) > block and b[2] == a[2] and np.array_equal(b[3], a[3]), (name, block, len(want))
                    joined.append(rr.rows(b[2], b[3], N0, N1)[0])
                    with_host.add(name)
                else:
                    assert len(want) <= block and (b[2] is None or not a[2]) and (b[3] is None or not len(a[3])), (name, block, len(want))
                    joined.append(b[5])
                if got is rows:
                    for c in range(3):
                        classes[c] += count[c]
            assert b"".join(joined) == b"".join(want_all), (name, block)
        if name not in with_host:
            without_host.add(name)
        # with the bins on the runs are what they are without the rows
        for a, b in zip(bins[0], both[0]):
            assert a[4] == b[4], (name, block)
    assert without_host and min(classes) > 0, (block, classes)
    if block == 64:
        assert with_host, block


def test_some_file_has_a_view_for_the_host_and_some_file_has_none(rig):
    hosts = {b: {n for n, r in rig.all_passes(f, b).items() if any(v[7] for v in r[1][0])} for f in (rc.FASTA, rc.FASTQ) for b in (64,)}
    every = {n for f in (rc.FASTA, rc.FASTQ) for n in rig.all_passes(f, 64)}
    assert hosts[64] and every - hosts[64], (hosts, every)


def test_switching_the_rows_on_and_off(rig):
    f = rig.feed(rc.FASTA, 4096)
    data = next(d for n, _, d, _ in rig.files if n == "fa_n257")
    for totals in ((0, N1), (N0, 0)):
        with pytest.raises(hast_amd.HastError) as e:
            f.set_rows(1, *totals)
        assert e.value.status == 1
    f.set_bins(1, N0, N1)
    with pytest.raises(hast_amd.HastError) as e:                                 # the bins have other set sizes
        f.set_rows(1, N0 + 1, N1)
    assert e.value.status == 1
    f.set_bins(0, 0, 0)
    f.submit(data[:4096], last=False)
    with pytest.raises(hast_amd.HastError) as e:                                 # a block is pending
        f.set_rows(1, N0, N1)
    assert e.value.status == 1
    f.next()
    f.submit(b"", last=True)
    f.next()
    f.set_rows(0, 0, 0)                                                          # off: hast_rs_next_rows is hast_rs_next, no rows
    views, _ = rig.run(rc.FASTA, 4096, data, True, False)
    plain, _ = rig.run(rc.FASTA, 4096, data, False, False)
    assert all(v[5] == b"" and v[6] == [0, 0, 0] and not v[7] for v in views)
    assert [v[2] for v in views] == [v[2] for v in plain] and all(np.array_equal(a[3], b[3]) for a, b in zip(views, plain))
    f.set_rows(1, N0, N1)                                                        # on: hast_rs_next still hands out names and votes
    again, _ = rig.run(rc.FASTA, 4096, data, False, False)
    assert [v[2] for v in again] == [v[2] for v in plain] and all(np.array_equal(a[3], b[3]) for a, b in zip(again, plain))
    f.set_rows(0, 0, 0)
