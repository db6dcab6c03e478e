"""Stage 02's per-barcode read count on the GPU: tally streams through the C ABI (hast_tally_*, hast_fq_set_tally, hast_fq_next_tallied;
k_fq_field2 and k_tally_add around the unchanged naming kernel) and the `barcode_freq` program on the device route, checked against
the Python restatement of the rule (tests/bf_model.py) and the reference's rows (tests/golden/barcode_freq/)."""
import ctypes as C
import gzip
import os
import random
import subprocess

import pytest

import hast_amd
from hast_amd.binding import FqBlock, FqRouted, FqTallied
from tests import bf_model
from tests.test_bf_core_cpu import CASES, golden, stats_of

pytestmark = pytest.mark.gpu

INVALID = 1


def rec(head, i=0):
    return head + b"\n" + b"ACGTN"[:1 + i % 5] + b"\n+\n" + b"IIIII"[:1 + i % 5] + b"\n"


def fastq(n, keys, end="whole", seed=0):
    """n records whose keys are drawn by `keys` (a callable of the record's number), some without a field 2 when keys returns None"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        k = keys(i, rng)
        out.append(rec(b"@no barcode %d" % i if k is None else b"@V%d#%s/1" % (i, k), i))
    data = b"".join(out)
    data += {"whole": b"", "unterminated_header": b"@x#END_1/1", "in_line2": b"@x#END_2/1\nAC", "after_header": b"@x#END_3/1\n"}[end]
    return data


def one_key(i, rng):
    return b"0_0_0"


def distinct_keys(i, rng):
    return b"%d_%d" % (i, i * 7)


_MANY = [b"%d_%d_%d" % (a, b, c) for a, b, c in ((random.Random(3).randint(1, 1536), j, 7 * j % 1536) for j in range(396))] + \
        [b"1536_1536_1536_a", b"L" * 40, b"", None]


def many_mix(i, rng):
    """one key owns 30 % of the records, in runs longer than a wave; the rest over ~400 keys, some longer than a text record, some
    records without a field 2"""
    return b"0_0_0" if (i // 100) % 10 in (1, 4, 7) else rng.choice(_MANY)


class TallyRun:
    """one input through a tally stream, a block at a time: plain or striped over `ctxs` (contexts of one GPU), host blocks in pieces
    of lo..hi bytes or device blocks filled by the GPU inflate.  Collects what the device leaves to the caller."""

    def __init__(self, ctxs, tallies, data, lo, hi, seed=0, device_blocks=False, tmp_path=None):
        self.lib, self.ctxs, self.data, self.lo, self.hi = hast_amd.lib(), ctxs, data, lo, hi
        self.rng = random.Random(seed)
        self.striped, self.device_blocks = len(ctxs) > 1, device_blocks
        self.left = [dict() for _ in tallies]          # per tally: key -> count, from left_* (per lane of a striped stream)
        self.tail = {}
        self.st = {"records": 0, "counted": 0, "left": 0, "nofield": 0, "blocks": 0, "fetched": 0, "tails": 0}
        self.lane_of_block = 0
        lib, fq = self.lib, C.c_void_p()
        if self.striped:
            arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
            assert lib.hast_fq_create_striped_ex(arr, len(ctxs), hi, 2, None, 1 if device_blocks else 0, C.byref(fq)) == 0, lib.hast_last_error()
            self.n_buffers = 2 * len(ctxs)
        else:
            assert lib.hast_fq_create_ex(ctxs[0]._h, hi, 3, None, 1 if device_blocks else 0, C.byref(fq)) == 0, lib.hast_last_error()
            self.n_buffers = 3
        self.fq = fq
        self.block = lib.hast_fq_block_bytes(fq)
        tarr = (C.c_void_p * len(tallies))(*[t._h.value for t in tallies])
        assert lib.hast_fq_set_tally(fq, tarr, len(tallies)) == 0, lib.hast_last_error()
        self.pos, self.pending, self.done, self.opened = 0, 0, False, 0
        self.z = None
        if device_blocks:
            path = str(tmp_path / ("in%d.fq.gz" % id(self)))
            with open(path, "wb") as f:
                f.write(gzip.compress(data, 6, mtime=0))
            self.z = hast_amd.GzReader(ctxs[0], path, 4096, 7, ctxs=ctxs if self.striped else None)

    def drain(self):
        lib, b = self.lib, FqTallied()
        assert lib.hast_fq_next_tallied(self.fq, C.byref(b)) == 0, lib.hast_last_error()
        assert b.n_counted + b.n_left + b.n_nofield == b.n_records
        lane = self.opened % len(self.ctxs) if self.striped else 0
        self.opened += 1
        for name, v in (("records", b.n_records), ("counted", b.n_counted), ("left", b.n_left), ("nofield", b.n_nofield), ("blocks", 1)):
            self.st[name] += v
        if b.n_left:
            view = b.bytes
            if self.device_blocks:
                assert not view
                view = C.POINTER(C.c_uint8)()
                assert lib.hast_fq_block_host_bytes(self.fq, C.byref(view)) == 0, lib.hast_last_error()
                self.st["fetched"] += 1
            for i in range(b.n_left):
                k = bytes(view[b.left_pos[i]:b.left_pos[i] + b.left_len[i]])
                self.left[lane][k] = self.left[lane].get(k, 0) + 1
        if b.tail_bytes:
            self.st["tails"] += 1
            rest = bytes(b.tail[:b.tail_bytes])
            assert self.data.endswith(rest) and rest.count(b"\n") < 4
            for k, c in bf_model.barcode_freq(rest).items():
                self.tail[k] = self.tail.get(k, 0) + c
            self.st["tail_nofield"] = bf_model.no_field(rest)
        assert lib.hast_fq_commit(self.fq) == 0, lib.hast_last_error()

    def step(self):
        """one more block in, and out what may come out; False once the input is through"""
        if self.done:
            return False
        lib = self.lib
        buf = C.POINTER(C.c_uint8)()
        assert lib.hast_fq_acquire(self.fq, C.byref(buf)) == 0, lib.hast_last_error()
        if self.device_blocks:
            d, fs = C.c_void_p(), C.c_void_p()
            assert lib.hast_fq_device_block(self.fq, C.byref(d), C.byref(fs)) == 0, lib.hast_last_error()
            n = self.z.read_device(d.value, self.block, fs)
            last = n < self.block
            assert lib.hast_fq_submit_device(self.fq, n, 1 if last else 0) == 0, lib.hast_last_error()
        else:
            n = min(len(self.data) - self.pos, self.block if self.striped else self.rng.randint(self.lo, self.hi))
            C.memmove(buf, self.data[self.pos:self.pos + n], n)
            self.pos += n
            last = self.pos >= len(self.data)
            assert lib.hast_fq_submit(self.fq, n, 1 if last else 0) == 0, lib.hast_last_error()
        self.pending += 1
        while self.pending > (0 if last else 1):
            self.drain()
            self.pending -= 1
        self.done = last
        return not last

    def close(self):
        if self.z:
            self.z.close()
        self.lib.hast_fq_destroy(self.fq)


def merged(*dicts):
    out = {}
    for d in dicts:
        for k, c in d.items():
            out[k] = out.get(k, 0) + c
    return out


def check_against_model(runs, tallies, datas):
    """what the tallies hold + what every run was left with = the model over every input; the block sums add up; no tally reports a
    key that a stream over it was left with"""
    want = merged(*[bf_model.barcode_freq(d) for d in datas])
    on_device = [t.read() for t in tallies]
    assert all(0 < c for t in on_device for c in t.values()) and all(len(k) <= 15 for t in on_device for k in t)
    got = merged(*on_device, *[l for r in runs for l in r.left], *[r.tail for r in runs])
    assert got == want
    st = {k: sum(r.st[k] for r in runs) for k in ("records", "counted", "left", "nofield")}
    assert st["counted"] == sum(c for t in on_device for c in t.values())
    tail_lines = sum(sum(r.tail.values()) + r.st.get("tail_nofield", 0) for r in runs)
    assert st["records"] + tail_lines == sum(want.values()) + sum(bf_model.no_field(d) for d in datas)
    assert st["nofield"] + sum(r.st.get("tail_nofield", 0) for r in runs) == sum(bf_model.no_field(d) for d in datas)
    return on_device, st


def run_one(data, n_ctx, lo, hi, max_texts=4096, device_blocks=False, tmp_path=None, per_ctx_tally=False):
    ctxs = [hast_amd.Context(21) for _ in range(n_ctx)]
    tallies = [hast_amd.Tally(ctxs[i], max_texts) for i in range(n_ctx if per_ctx_tally else 1)]
    try:
        run = TallyRun(ctxs, tallies if per_ctx_tally else tallies * n_ctx, data, lo, hi, device_blocks=device_blocks, tmp_path=tmp_path)
        while run.step():
            pass
        run.close()
        if not per_ctx_tally:                      # one tally under every lane: what any lane was left with is that tally's
            run.left = [merged(*run.left)]
        on_device, st = check_against_model([run], tallies, [data])
        for t, l in zip(on_device, run.left):
            assert not set(t) & set(l)
        return run, on_device, st
    finally:
        for t in tallies:
            t.close()
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1200])
@pytest.mark.parametrize("keys", [one_key, distinct_keys, many_mix], ids=["one_key", "distinct", "many"])
def test_tally_record_counts_at_wave_and_tile_borders(n, keys):
    """a lane per record in k_fq_field2, the combining rounds of k_tally_add: whole waves of one id, 64 different ids, the mix"""
    data = fastq(n, keys, seed=n)
    run, on_device, st = run_one(data, 1, 65536, 65536)
    assert st["records"] == n
    if keys is one_key and n:
        assert on_device == [{b"0_0_0": n}] and st["left"] == 0
    if keys is distinct_keys:
        assert len(on_device[0]) == n and st["counted"] == n


@pytest.mark.parametrize("end", ["whole", "unterminated_header", "in_line2", "after_header"])
@pytest.mark.parametrize("chunk,n_ctx,device_blocks", [((700, 4096), 1, False), ((4096, 4096), 1, False), ((50_000, 65536), 1, False), ((4096, 4096), 2, False),
                                                       ((8192, 8192), 3, False), ((4096, 4096), 1, True), ((8192, 8192), 1, True), ((4096, 4096), 2, True),
                                                       ((8192, 8192), 3, True)])
def test_tally_streams_blocks_contexts_and_file_ends(tmp_path, end, chunk, n_ctx, device_blocks):
    """records straddle blocks of 700 B .. 64 KB; plain streams and streams striped over 1-3 contexts; host blocks and blocks the GPU
    inflate fills; a file that ends after a whole record, inside a header, inside line 2, right behind a header"""
    data = fastq(4000 if chunk[1] > 8192 else 1200, many_mix, end, seed=len(end))         # (more than one block at 64 KB too)
    run, on_device, st = run_one(data, n_ctx, chunk[0], chunk[1], device_blocks=device_blocks, tmp_path=tmp_path)
    assert run.st["blocks"] >= len(data) // chunk[1] and st["left"] > 0
    assert run.st["tails"] == (0 if end == "whole" else 1)
    assert (run.st["fetched"] > 0) == device_blocks


def often_long(i, rng):
    """every seventh key is longer than a text record, every eleventh record has no field 2"""
    return None if i % 11 == 5 else b"LONG_KEY_NUMBER_%d" % (i % 9) if i % 7 == 3 else b"%d_%d" % (i % 50, i % 50)


@pytest.mark.parametrize("chunk,n_ctx,device_blocks", [((700, 4096), 1, False), ((65536, 65536), 1, False), ((4096, 4096), 2, False), ((8192, 8192), 1, True)])
def test_tally_block_with_more_header_lines_than_the_pinned_arrays_hold(monkeypatch, tmp_path, chunk, n_ctx, device_blocks):
    """HAST_FQ_HOST_RECORDS=16: every slot's first block owns more header lines than its pinned arrays hold, so they grow before the
    block is named and the extents of what is left to the caller come by copy from the device; the slot's later blocks use the grown
    arrays"""
    monkeypatch.setenv("HAST_FQ_HOST_RECORDS", "16")
    data = fastq(3000, often_long, "in_line2", seed=4)
    run, on_device, st = run_one(data, n_ctx, chunk[0], chunk[1], device_blocks=device_blocks, tmp_path=tmp_path)
    assert st["records"] == 3000 and st["left"] == sum(1 for i in range(3000) if i % 11 != 5 and i % 7 == 3)
    assert st["nofield"] == sum(1 for i in range(3000) if i % 11 == 5) and run.st["tails"] == 1
    assert run.st["blocks"] >= 2 and set(merged(*run.left)) == {b"LONG_KEY_NUMBER_%d" % j for j in range(9)}


@pytest.mark.parametrize("per_ctx_tally", [False, True], ids=["shared_tally", "tally_per_context"])
def test_tally_full_dictionary_hands_over_without_double_counting(per_ctx_tally):
    """max_texts 8 under 40 texts in 1 200 records, blocks of 4 KB, two streams of two contexts each at once: the totals are exact, and
    a key is the device's in every block or the caller's in every block, per tally"""
    texts = [b"%d_%d" % (j, 3 * j) for j in range(40)]
    datas = [fastq(1200, lambda i, rng: rng.choice(texts), seed=s) for s in (1, 2)]
    ctxs = [hast_amd.Context(21) for _ in range(4)]
    tallies = [hast_amd.Tally(ctxs[i], 8) for i in range(4 if per_ctx_tally else 1)]
    try:
        assert all(t.limit() == 8 for t in tallies)
        lane_tallies = [[tallies[2 * s + g] if per_ctx_tally else tallies[0] for g in range(2)] for s in range(2)]
        runs = [TallyRun(ctxs[2 * s:2 * s + 2], lane_tallies[s], datas[s], 4096, 4096, seed=s) for s in range(2)]
        more = [True, True]
        while any(more):
            for s in range(2):
                more[s] = runs[s].step()
        for r in runs:
            r.close()
        on_device, st = check_against_model(runs, tallies, datas)
        assert all(t.size() == 8 for t in tallies) and st["left"] > 0 and st["counted"] > 0
        for ti, t in enumerate(tallies):
            lefts = [r.left[g] for s, r in enumerate(runs) for g in range(2) if lane_tallies[s][g] is t]
            assert len(on_device[ti]) == 8 and not set(on_device[ti]) & set(merged(*lefts))
    finally:
        for t in tallies:
            t.close()
        for c in ctxs:
            c.close()


def test_tally_mode_errors_change_nothing():
    lib = hast_amd.lib()
    data = fastq(300, many_mix, seed=9)
    with hast_amd.Context(21) as ctx, hast_amd.Tally(ctx, 1024) as tally:
        run = TallyRun([ctx], [tally], data, 4096, 4096)
        buf = C.POINTER(C.c_uint8)()
        assert lib.hast_fq_acquire(run.fq, C.byref(buf)) == 0
        tarr = (C.c_void_p * 1)(tally._h.value)
        assert lib.hast_fq_set_tally(run.fq, tarr, 1) == INVALID and b"in hand" in lib.hast_last_error()      # a block in hand
        assert lib.hast_fq_set_tally(run.fq, None, 0) == INVALID
        n = min(4096, len(data))
        C.memmove(buf, data[:n], n)
        assert lib.hast_fq_submit(run.fq, n, 0) == 0, lib.hast_last_error()
        assert lib.hast_fq_next(run.fq, C.byref(FqBlock())) == INVALID and b"tallies" in lib.hast_last_error()
        assert lib.hast_fq_next_routed(run.fq, C.byref(FqRouted())) == INVALID
        run.pos, run.pending = n, 1
        while run.step():                           # the stream is as usable as before
            pass
        run.close()
        check_against_model([run], [tally], [data])
        # a stream that does not tally (it routes, over an empty table: every barcode is in no list, the block is the caller's)
        fq, tab = C.c_void_p(), C.c_void_p()
        assert lib.hast_fq_create(ctx._h, 4096, 3, None, C.byref(fq)) == 0, lib.hast_last_error()
        assert lib.hast_fq_acquire(fq, C.byref(buf)) == 0
        C.memmove(buf, data[:n], n)
        assert lib.hast_fq_submit(fq, n, 1) == 0, lib.hast_last_error()
        assert lib.hast_fq_next_tallied(fq, C.byref(FqTallied())) == INVALID and b"does not tally" in lib.hast_last_error()
        blk = FqBlock()                                               # (reads shorter than K: framed, reported, not classified)
        assert lib.hast_fq_next(fq, C.byref(blk)) == 0 and blk.n_records > 0 and blk.short_read, lib.hast_last_error()
        assert lib.hast_fq_commit(fq) == 0, lib.hast_last_error()
        lib.hast_fq_destroy(fq)
        assert lib.hast_names_create(ctx._h, 64, C.byref(tab)) == 0, lib.hast_last_error()
        assert lib.hast_fq_create(ctx._h, 4096, 3, None, C.byref(fq)) == 0, lib.hast_last_error()
        assert lib.hast_fq_set_route(fq, (C.c_void_p * 1)(tab.value), 1) == 0, lib.hast_last_error()
        assert lib.hast_fq_set_tally(fq, tarr, 1) == INVALID and b"routes" in lib.hast_last_error()
        assert lib.hast_fq_acquire(fq, C.byref(buf)) == 0
        C.memmove(buf, data[:n], n)
        assert lib.hast_fq_submit(fq, n, 1) == 0, lib.hast_last_error()
        assert lib.hast_fq_next_tallied(fq, C.byref(FqTallied())) == INVALID and b"does not tally" in lib.hast_last_error()
        routed = FqRouted()
        assert lib.hast_fq_next_routed(fq, C.byref(routed)) == 0 and (routed.n_records or routed.host_block), lib.hast_last_error()
        assert lib.hast_fq_commit(fq) == 0
        lib.hast_fq_destroy(fq)
        lib.hast_names_destroy(tab)
        assert lib.hast_tally_read(tally._h, 1000, 100, None, None) == INVALID


# ---- the program ---------------------------------------------------------------------------------------------------------------
CONFIGS = {
    "plain": (False, (), None),
    "gz_inflate_device": (True, ("--inflate", "device"), None),
    "gz_inflate_host": (True, ("--inflate", "host"), None),
    "plain_small_blocks": (False, (), 4096),
    "gz_small_blocks": (True, (), 8192),
    "plain_three_lanes": (False, ("--devices", "0,0,0"), 4096),
    "gz_three_lanes": (True, ("--devices", "0,0,0"), 8192),
    "max_barcodes_8": (False, ("--max-barcodes", "8"), 4096),
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_program_device_route_reproduces_the_reference(tmp_path, config):
    hast_amd.build()
    gz, extra, block = CONFIGS[config]
    env = dict(os.environ)
    env.pop("HAST_BF_BLOCK", None)
    if block:
        env["HAST_BF_BLOCK"] = str(block)
    for case in CASES:
        data = golden(case, ".fq")
        name = case + (".fq.gz" if gz else ".fq")
        (tmp_path / name).write_bytes(gzip.compress(data, 6, mtime=0) if gz else data)
        r = subprocess.run([hast_amd.barcode_freq_exe(), "--stats", *extra, name], cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, (case, r.stderr)
        assert r.stdout == golden(case, ".txt"), case
        st = stats_of(r.stderr, b"device")
        want = bf_model.barcode_freq(data)
        assert st["counted_on_device"] + st["counted_on_host"] + st["no_field"] == st["header_lines"] == sum(want.values()) + bf_model.no_field(data)
        assert st["no_field"] == bf_model.no_field(data) and st["distinct"] == len(want)
        short = sum(1 for k in want if len(k) <= 15)
        assert st["dictionary_full"] == (1 if config == "max_barcodes_8" and short >= 8 else 0), (case, st)
        if data:
            assert st["counted_on_device"] > 0
        if config != "max_barcodes_8":             # only keys longer than a text record and the file's end are the host's
            assert st["counted_on_host"] <= sum(c for k, c in want.items() if len(k) > 15) + 1
