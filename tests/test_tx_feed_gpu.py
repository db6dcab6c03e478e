"""GPU tests of the paired feed behind `fake_10x --convert device --inflate device` (hast_tx_feed_*, hast_amd/csrc/tx_feed.cpp): driven
with the program's step sequence -- step n + 1 before collect n -- every step's result and the running state equal
hast_tx_pair_host(final = 0) over the same bytes, hast_tx_feed_wants equals the program's reading rule over the bytes, the collected
outputs (with gz_out: one gzip member per step and side that had bytes, inflated) are the host model's, and what the feed hands back at
the inputs' ends is what the host loop would hold.  Each case goes through device blocks and through host blocks."""
import ctypes as C
import zlib

import numpy as np
import pytest

import hast_amd
from hast_amd import TX_ENDS, TX_ON_HOST, TX_TAIL_TOO_LONG, TxConverter, TxFeed, TxMap, TxState
from tests import tx_model as tm

pytestmark = pytest.mark.gpu
FIELDS = ("consumed1", "consumed2", "pairs", "used")
MAX_IN = 1 << 20                   # the feed's room for every block used here (tx_feed_plan.h: at least 1 MB)
MAP16 = b"k\tACGTACGTACGTACGT\nq\tTTTT\n"


def fields(res):
    return tuple(getattr(res, f) for f in FIELDS) + tuple(res.out_bytes) + tuple(res.raw_bytes) + tuple(res.lines)


def members(data):
    out = []
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        assert d.eof
        data = d.unused_data
    return out


def uneven_case():
    """2000 pairs, read 1's records about four times the size of read 2's"""
    r1 = b"".join(b"@u%d#%s/1\n%s\n+\n%s\n" % (i, b"k" if i % 7 else b"absent", b"ACGT" * 30, b"IIH!" * 30) for i in range(2000))
    r2 = b"".join(b"@u%d#k/2\n%s\n+\n%s\n" % (i, b"TG" * 12, b"F!" * 12) for i in range(2000))
    return r1, r2, MAP16, 512


def case_inputs(case):
    if case == "uneven":
        return uneven_case()
    if case == "outgrow":                                           # 7 bytes become 78: every step's outputs outgrow 2 x input + 4 KB
        rec = b"@#k\n\n\n\n" * 3000
        return rec, rec, MAP16, 4096
    return tm.golden(case, "r1.fq"), tm.golden(case, "r2.fq"), tm.golden(case, "map.txt"), {"edge": 100, "widths": 4096, "long": 9000}[case]


@pytest.fixture(scope="module")
def ctx():
    with hast_amd.Context(21) as c:
        yield c


def drive(ctx, map_text, r1, r2, block, gz, via):
    """the program's loop over a feed, every step beside the host model -> dict of what happened"""
    lib = hast_amd.lib()
    src, at, eof, have = (r1, r2), [0, 0], [False, False], [b"", b""]
    st_d, st_h = TxState(0, 0), TxState(0, 0)
    want, got, flags_seen, skipped, steps = [], [], 0, 0, 0
    with TxMap(map_text) as m, TxConverter(ctx, m, MAX_IN) as conv, TxFeed(conv, block, gz) as feed:
        assert feed.room == MAX_IN
        waiting = False
        while True:
            for s in range(2):
                rule = not eof[s] and not (len(have[s]) > block and have[s].count(b"\n") >= 4)
                assert feed.wants(s) == rule, (steps, s)
                if not rule:
                    skipped += not eof[s]
                    continue
                piece = src[s][at[s]:at[s] + block]
                at[s] += len(piece)
                if via == "device":
                    d, _stream = feed.device_block(s)
                    if piece:
                        a = np.frombuffer(piece, dtype=np.uint8)
                        lib.hast_memcpy_h2d(ctx._h, C.c_void_p(d), a.ctypes.data, a.size)
                    feed.submit(s, len(piece))
                else:
                    feed.submit_host(s, piece)
                assert not feed.wants(s)
                have[s] += piece
                eof[s] = len(piece) < block
            mode = lib.hast_tx_step_mode(eof[0], eof[1], have[0], len(have[0]), have[1], len(have[1]))
            before = (st_d.used, st_d.headers)
            res, flags = feed.step(st_d)
            if mode != 0:
                assert flags == TX_ENDS and (st_d.used, st_d.headers) == before and res.pairs == 0
                break
            assert not flags & TX_ENDS
            o1, o2, hres = m.pair_host(have[0], have[1], 0, st_h)
            assert fields(res) == fields(hres), (steps, fields(res), fields(hres))
            assert (st_d.used, st_d.headers) == (st_h.used, st_h.headers)
            have = [have[0][hres.consumed1:], have[1][hres.consumed2:]]
            want.append((o1, o2))
            flags_seen |= flags
            steps += 1
            if waiting:
                got.append(feed.collect())
            waiting = True
            if flags & TX_TAIL_TOO_LONG:
                break
        if waiting:
            got.append(feed.collect())
        with pytest.raises(hast_amd.HastError):
            feed.collect()                                          # nothing is waiting
        for s in range(2):
            assert feed.take_tail(s) == have[s], ("tail of side", s)
        times, wait = feed.times()
        assert times.kernel_s > 0 and wait >= 0
    assert len(got) == len(want) == steps
    return dict(want=want, got=got, flags=flags_seen, skipped=skipped, steps=steps)


@pytest.mark.parametrize("via", ("device", "host"))
@pytest.mark.parametrize("gz", (0, 1), ids=("plain", "gz"))
@pytest.mark.parametrize("case", ("edge", "widths", "long", "uneven"))
def test_the_feed_is_the_host_model_step_by_step(ctx, case, gz, via):
    r1, r2, map_text, block = case_inputs(case)
    d = drive(ctx, map_text, r1, r2, block, gz, via)
    assert d["steps"] >= 1 and not d["flags"] & TX_TAIL_TOO_LONG
    if case in ("widths", "long", "uneven"):
        assert d["steps"] > 4
    if case == "uneven":
        assert d["skipped"] >= 1                                    # a condition of the test: a step in which a side reads nothing
    for (w1, w2), (g1, g2, raw) in zip(d["want"], d["got"]):
        assert raw == (len(w1), len(w2))
        for w, g in ((w1, g1), (w2, g2)):
            if gz:
                parts = members(g)
                assert len(parts) == (1 if w else 0) and b"".join(parts) == w      # one member per step and side that had bytes
            else:
                assert g == w


@pytest.mark.parametrize("gz", (0, 1), ids=("plain", "gz"))
def test_outputs_that_outgrow_their_room_are_the_host_models(ctx, gz):
    r1, r2, map_text, block = case_inputs("outgrow")
    d = drive(ctx, map_text, r1, r2, block, gz, "device")
    assert d["flags"] & TX_ON_HOST and d["steps"] > 4
    for (w1, w2), (g1, g2, raw) in zip(d["want"], d["got"]):
        assert raw == (len(w1), len(w2))
        for w, g in ((w1, g1), (w2, g2)):
            assert (b"".join(members(g)) if gz else g) == w


def test_what_the_feed_refuses(ctx):
    with TxMap(MAP16) as m, TxConverter(ctx, m, MAX_IN) as conv:
        with pytest.raises(hast_amd.HastError) as ei:
            TxFeed(conv, (MAX_IN // 2), 0)                          # 2 x block + 4 KB is more than the converter was created for
        assert ei.value.status == 9
        with TxFeed(conv, 4096, 1) as feed:
            with pytest.raises(hast_amd.HastError):
                feed.submit(0, 10)                                  # no block was handed out
            feed.submit_host(0, b"@a#k/1\nAC\n+\nII\n")
            with pytest.raises(hast_amd.HastError):
                feed.submit_host(0, b"x")                           # the side has read for this step
            feed.submit_host(1, b"@a#k/2\nGT\n+\nFF\n")
            st = TxState(0, 0)
            res, flags = feed.step(st)
            assert res.pairs == 1 and flags == 0
            res, flags = feed.step(st)                              # both inputs have ended and left nothing
            assert flags == TX_ENDS
            o1, o2, raw = feed.collect()
            w1, w2, _ = m.pair_host(b"@a#k/1\nAC\n+\nII\n", b"@a#k/2\nGT\n+\nFF\n", 0, TxState(0, 0))
            assert members(o1) == [w1] and members(o2) == [w2] and raw == (len(w1), len(w2))
