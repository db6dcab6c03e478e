"""GPU tests of the stLFR -> 10x conversion over device memory (hast_tx_create / hast_tx_pair_device, hast_amd/csrc/tx_kernels.hip):
every field of its result, the running state and every byte it writes equal hast_tx_pair_host(final = 0) on the same bytes; nothing is
written behind out_bytes, and nothing at all by a step whose outputs do not fit their room."""
import ctypes as C

import numpy as np
import pytest

import hast_amd
from hast_amd import TxConverter, TxMap, TxState
from tests import tx_model as tm

pytestmark = pytest.mark.gpu
CANARY, PAD = 0xEE, 64
ROOM = 1 << 20                     # bytes of each of the four device buffers' payload
MAX_IN = 1 << 18                   # what the converters are created for
FIELDS = ("consumed1", "consumed2", "pairs", "used")
UNSUPPORTED, INVALID = 9, 1
MAP = b"k\tACGT\nnone\t\none\tT\nsixteen\tACGTACGTACGTACGT\nA_1\tGG\nA_1\r\tCC\nA_1 \tTT\nK23456789012345\tAAAA\n"


def fields(res):
    return tuple(getattr(res, f) for f in FIELDS) + tuple(res.out_bytes) + tuple(res.raw_bytes) + tuple(res.lines)


class Rig:
    """a context, four device buffers (two inputs, two outputs) with slack for every alignment, and converters per map text"""

    def __init__(self):
        self.ctx = hast_amd.Context(21)
        self.lib = hast_amd.lib()
        self.d_in = [self.ctx.alloc(ROOM + 64) for _ in range(2)]
        self.d_out = [self.ctx.alloc(ROOM + PAD + 64) for _ in range(2)]
        self.maps = {}

    def conv(self, map_text):
        if map_text not in self.maps:
            m = TxMap(map_text)
            self.maps[map_text] = (m, TxConverter(self.ctx, m, MAX_IN))
        return self.maps[map_text]

    def run(self, map_text, r1, r2, used=0, in_at=(0, 0), out_at=(0, 0), short=None):
        """one step on the device and on the host over the same bytes, compared.  short = 0 / 1: that side's room is one byte less than
        it needs, the step must be refused whole.  Returns the host's (out1, out2, result)."""
        m, conv = self.conv(map_text)
        st_h = TxState(used, used + 5)
        want = m.pair_host(r1, r2, False, st_h)
        for s, data in enumerate((r1, r2)):
            if data:
                a = np.frombuffer(data, dtype=np.uint8)
                self.lib.hast_memcpy_h2d(self.ctx._h, C.c_void_p(self.d_in[s] + in_at[s]), a.ctypes.data, a.size)
        need = [len(want[0]), len(want[1])]
        assert max(need) + PAD <= ROOM
        for s in range(2):
            self.ctx.memset(self.d_out[s] + out_at[s], CANARY, need[s] + PAD)
        self.ctx.sync()
        caps = [need[s] + PAD - (PAD + 1 if short == s else 0) for s in range(2)]
        st_d = TxState(used, used + 5)
        args = (self.d_in[0] + in_at[0], len(r1), self.d_in[1] + in_at[1], len(r2), st_d, self.d_out[0] + out_at[0], caps[0], self.d_out[1] + out_at[1], caps[1])
        if short is None:
            res = conv.pair_device(*args)
            assert fields(res) == fields(want[2]), (fields(res), fields(want[2]))
            assert (st_d.used, st_d.headers) == (st_h.used, st_h.headers)
        else:
            with pytest.raises(hast_amd.HastError) as ei:
                conv.pair_device(*args)
            assert ei.value.status == UNSUPPORTED
            assert tuple(ei.value.result.out_bytes) == tuple(need)
            assert (st_d.used, st_d.headers) == (used, used + 5)
        for s in range(2):
            got = self.ctx.to_host(self.d_out[s] + out_at[s], (need[s] + PAD,), np.uint8)
            n = need[s] if short is None else 0
            assert got[:n].tobytes() == want[s][:n], ("side", s, "first difference at", int(np.argmax(got[:n] != np.frombuffer(want[s], np.uint8)[:n])))
            assert np.all(got[n:] == CANARY), ("side", s, "written behind its end")
        return want

    def close(self):
        for m, conv in self.maps.values():
            conv.close()
            m.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def records(n, key=lambda i: b"k", side=1, seq=lambda i: (i * 7) % 40 + 1):
    out = []
    for i in range(n):
        L = seq(i)
        out.append(b"@r%d#%s/%d\n%s\n+\n%s\n" % (i, key(i), side, (b"ACGTN" * (L // 5 + 1))[:L], (b"FI!,:" * (L // 5 + 1))[:L]))
    return b"".join(out)


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257, 513))
def test_pairs_per_call_at_the_wave_and_tile_borders(rig, n):
    for what, key in (("kept", lambda i: b"k"), ("dropped", lambda i: b"absent"), ("alternating", lambda i: b"k" if i % 2 else b"x")):
        o1, o2, res = rig.run(MAP, records(n, key), records(n, key, side=2, seq=lambda i: (i * 11) % 30 + 1))
        assert res.pairs == n and res.used == {"kept": n, "dropped": 0, "alternating": n // 2}[what]


def test_no_whole_pair(rig):
    for r1, r2 in ((b"", b""), (b"@a#k/1\nAC\n+\n", b"@a#k/2\nAC\n+\nII\n"), (b"@a#k/1\nAC\n+\nII\n", b"@a#k/2"), (b"no newline at all", b"\n\n\n")):
        o1, o2, res = rig.run(MAP, r1, r2)
        assert fields(res)[:8] == (0,) * 8 and tuple(res.lines) == (r1.count(b"\n"), r2.count(b"\n"))


def test_sides_of_different_lengths(rig):
    """the side with more whole records keeps them for the next step; a partial record lies behind each"""
    for n1, n2 in ((70, 9), (9, 70), (300, 257)):
        r1, r2 = records(n1) + b"@part#k/1\nAC", records(n2, side=2) + b"@part#k/2\nACGT\n+"
        o1, o2, res = rig.run(MAP, r1, r2)
        assert res.pairs == min(n1, n2) and res.consumed1 == len(records(min(n1, n2))) and res.consumed2 == len(records(min(n1, n2), side=2))


@pytest.mark.parametrize("used", (8, 98, 999998, 4294967290, 9999999995))
def test_n_crosses_a_width_and_two_to_the_32(rig, used):
    o1, o2, res = rig.run(MAP, records(12), records(12, side=2), used=used)
    want1, want2, _, _, _ = tm.convert(tm.parse_map(MAP), records(12), records(12, side=2), used=used)
    assert (o1, o2) == (want1, want2) and res.used == 12
    assert b"0:0:%d 1:N" % (used + 1) in o1 and b"0:0:%d 2:N" % (used + 12) in o2


def test_values_of_every_length_and_the_key_rules(rig):
    keys = (b"none", b"one", b"sixteen", b"k")
    o1, o2, res = rig.run(MAP, records(40, lambda i: keys[i % 4]), records(40, side=2))
    assert res.used == 40 and b"\nATCGAGN" in o1 and b"\nTATCGAGN" in o1 and b"\nACGTACGTACGTACGTATCGAGN" in o1
    heads = (b"@r#A_1/1\tx", b"@r#A_1#zz/1", b"@r/1#A_1", b"@r\t#A_1/1", b"@r#A_1\r", b"@r#A_1 /1", b"@r#/1", b"@r#", b"@r", b"", b"#k", b"#k#", b"#", b"\t",
             b"@r#K23456789012345/1", b"@r#K234567890123456/1", b"@r#K2345678901234/1", b"@r#K23456789012345")
    r1 = b"".join(h + b"\nAC\n+\n!I\n" for h in heads)
    o1, o2, res = rig.run(MAP, r1, records(len(heads), side=2))
    assert res.used == sum(tm.key_of(h) in tm.parse_map(MAP) for h in heads) == 9
    assert b"\nCCATCGAGNAC\n" in o1 and b"\nTTATCGAGNAC\n" in o1 and o1.count(b"\nAAAAATCGAGNAC\n") == 2


def test_line_lengths_and_bangs(rig):
    """empty lines, lines around the 64 bytes a wave copies at a time, and '!' in every line: only line 4's change"""
    r1 = b"\n\n\n\n" + b"@#k\n\n\n\n" + b"#k\n!\n!\n!\n"
    r2 = b"\n\n\n\n" * 2 + b"!\n!\n!\n!\n"
    for L in (1, 63, 64, 65, 300):
        r1 += b"@a!#k/1\n" + b"A!" * (L // 2) + b"C" * (L % 2) + b"\n+!" + b"x" * (L - 1) + b"\n" + b"!I" * (L // 2) + b"!" * (L % 2) + b"\n"
        r2 += b"@a!#k/2\n" + b"!" * L + b"\n+\n" + b"!" * L + b"\n"
    o1, o2, res = rig.run(MAP, r1, r2)
    assert (res.pairs, res.used) == (8, 7)
    assert b"NAAGTGCT\nACGTATCGAGN!\n!\n" + b"F" * 22 + b"##\n" in o1 and b"NAAGTGCT\n!\n!\n#\n" in o2
    assert b"\n" + b"!" * 300 + b"\n+\n" + b"#" * 300 + b"\n" in o2
    rig.run(tm.golden("long", "map.txt"), tm.golden("long", "r1.fq"), tm.golden("long", "r2.fq"))


@pytest.mark.parametrize("which", ("d_r1", "d_r2", "d_out1", "d_out2"))
def test_every_alignment_of_every_buffer(rig, which):
    r1, r2 = records(70), records(70, side=2)
    for a in range(16):
        in_at = (a if which == "d_r1" else 0, a if which == "d_r2" else 0)
        out_at = (a if which == "d_out1" else 0, a if which == "d_out2" else 0)
        # the bytes in front of and behind an input are other text with newlines of its own: nothing outside [d, d + n) may count
        for s in range(2):
            junk = np.frombuffer(b"\n@x#k\n" * 40, dtype=np.uint8)
            rig.lib.hast_memcpy_h2d(rig.ctx._h, C.c_void_p(rig.d_in[s]), junk.ctypes.data, 16)
            rig.lib.hast_memcpy_h2d(rig.ctx._h, C.c_void_p(rig.d_in[s] + in_at[s] + len((r1, r2)[s])), junk.ctypes.data, junk.size)
        rig.run(MAP, r1, r2, in_at=in_at, out_at=out_at)


def test_a_room_one_byte_short_is_refused_whole(rig):
    r1, r2 = records(300), records(300, side=2)
    for short in (0, 1):
        rig.run(MAP, r1, r2, used=7, short=short)
    rig.run(MAP, r1, r2, used=7)


def test_larger_than_created_for_is_invalid(rig):
    m, conv = rig.conv(MAP)
    st = TxState(0, 0)
    for n1, n2 in ((MAX_IN + 1, 16), (16, MAX_IN + 1)):
        with pytest.raises(hast_amd.HastError) as ei:
            conv.pair_device(rig.d_in[0], n1, rig.d_in[1], n2, st, rig.d_out[0], ROOM, rig.d_out[1], ROOM)
        assert ei.value.status == INVALID and (st.used, st.headers) == (0, 0)
    with pytest.raises(hast_amd.HastError) as ei:
        TxConverter(rig.ctx, m, (128 << 20) + 1)
    assert ei.value.status == INVALID


def test_a_map_of_5000_keys_and_5000_near_misses(rig):
    keys = [b"%d_%d_%d" % (i % 97, i // 97, i * 7919 % 1537) for i in range(5000)]
    assert len(set(keys)) == 5000 and max(len(k) for k in keys) <= 15
    values = [(b"ACGT" * 4)[i % 4:i % 4 + i % 17] for i in range(5000)]
    text = b"".join(k + b"\t" + v + b"\n" for k, v in zip(keys, values))
    misses = [k[:-1] + bytes([k[-1] ^ 1]) if i % 2 else k + b"_" for i, k in enumerate(keys)]
    misses = [k for k in misses if k not in set(keys)]
    assert len(misses) == 5000
    mix = [k for pair in zip(keys, misses) for k in pair]
    r1 = b"".join(b"@r#%s/1\nAC\n+\nII\n" % k for k in mix)
    o1, o2, res = rig.run(text, r1, records(len(mix), side=2, seq=lambda i: 3))
    assert res.pairs == 10000 and res.used == 5000                # every key kept, every near miss dropped
    lines = o1.split(b"\n")
    assert [lines[4 * i + 1] for i in range(5000)] == [v + b"ATCGAGNAC" for v in values]     # every key with its own value


def test_a_step_from_host_bytes_to_host_bytes(rig):
    """hast_tx_pair_staged: the runs as they are, and as one gzip member each; what it cannot take is UNSUPPORTED and changes nothing"""
    import gzip
    m, conv = rig.conv(MAP)
    r1, r2 = records(300) + b"@part", records(300, side=2)
    for gz in (0, 1):
        st_h, st_d = TxState(3, 4), TxState(3, 4)
        w1, w2, want = m.pair_host(r1, r2, False, st_h)
        times = hast_amd.TxTimes()
        o1, o2, res = conv.pair_staged(r1, r2, st_d, gz, times)
        assert (gzip.decompress(o1), gzip.decompress(o2)) == (w1, w2) if gz else (o1, o2) == (w1, w2)
        assert fields(res)[:4] == fields(want)[:4] and tuple(res.raw_bytes) == (len(w1), len(w2)) and tuple(res.lines) == tuple(want.lines)
        assert (st_d.used, st_d.headers) == (st_h.used, st_h.headers) and times.kernel_s > 0
    st = TxState(3, 4)
    short = b"@#k\n\n\n\n" * 2000                              # 7 bytes become 78: more than twice the bytes and 4 KB
    for a, b in ((short, short), (b"x" * (MAX_IN + 1), r2)):
        with pytest.raises(hast_amd.HastError) as ei:
            conv.pair_staged(a, b, st, 0)
        assert ei.value.status == UNSUPPORTED and (st.used, st.headers) == (3, 4)


def drive_as_the_program(rig, case, block):
    """the steps of fake_10x --convert device: mode 0 on the device with room for twice the bytes given and 4 KB, the rest on the host"""
    text = tm.golden(case, "map.txt")
    m, conv = rig.conv(text)
    src = [tm.golden(case, "r1.fq"), tm.golden(case, "r2.fq")]
    have, at, out, st = [b"", b""], [0, 0], [[], []], TxState(0, 0)
    on_device = on_host = steps = 0
    mode = 0
    while mode != 1:
        for s in range(2):
            have[s] += src[s][at[s]:at[s] + block]
            at[s] = min(at[s] + block, len(src[s]))
        mode = rig.lib.hast_tx_step_mode(at[0] == len(src[0]), at[1] == len(src[1]), have[0], len(have[0]), have[1], len(have[1]))
        caps = [2 * len(have[s]) + 4096 for s in range(2)]
        res = None
        if mode == 0 and max(caps) + 64 <= ROOM:
            for s in range(2):
                if have[s]:
                    a = np.frombuffer(have[s], dtype=np.uint8)
                    rig.lib.hast_memcpy_h2d(rig.ctx._h, C.c_void_p(rig.d_in[s]), a.ctypes.data, a.size)
            try:
                res = conv.pair_device(rig.d_in[0], len(have[0]), rig.d_in[1], len(have[1]), st, rig.d_out[0], caps[0], rig.d_out[1], caps[1])
                o = [rig.ctx.to_host(rig.d_out[s], (res.out_bytes[s],), np.uint8).tobytes() if res.out_bytes[s] else b"" for s in range(2)]
                on_device += res.pairs
            except hast_amd.HastError as e:
                assert e.status == UNSUPPORTED
                res = None
        if res is None:
            o1, o2, res = m.pair_host(have[0], have[1], mode, st)
            o = [o1, o2]
            on_host += res.pairs
        steps += 1
        for s in range(2):
            out[s].append(o[s])
        have = [have[0][res.consumed1:], have[1][res.consumed2:]]
    return b"".join(out[0]), b"".join(out[1]), st, on_device, on_host, steps


@pytest.mark.parametrize("block", (700, 4096))
@pytest.mark.parametrize("case", ("edge", "widths", "long"))
def test_goldens_driven_as_the_program_drives_them(rig, case, block):
    o1, o2, st, on_device, on_host, steps = drive_as_the_program(rig, case, block)
    assert o1 == tm.golden(case, "out1.fq") and o2 == tm.golden(case, "out2.fq")
    assert b"Total %d pair reads and used %d pairs.\n" % (st.headers, st.used) in tm.golden(case, "stdout.txt")
    assert on_device + on_host == st.headers and on_device >= 1
    if case != "edge":
        assert on_host <= 1 and steps > 4


@pytest.mark.parametrize("case", ("fb_value17", "fb_key16", "fb_emptykey"))
def test_a_map_the_device_cannot_take_is_unsupported(rig, case):
    with TxMap(tm.golden(case, "map.txt")) as m:
        assert not m.device_ok
        with pytest.raises(hast_amd.HastError) as ei:
            TxConverter(rig.ctx, m, MAX_IN)
        assert ei.value.status == UNSUPPORTED and tm.FALLBACK[case][1] in str(ei.value)
        assert tm.FALLBACK[case][1] in hast_amd.lib().hast_last_error().decode()
