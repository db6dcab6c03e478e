"""Blocked-gzip (BGZF) files for the tests of the per-member device inflate (a helper, not a test): built in memory from the helpers
of tests/test_inflate_cpu.py (bgzf, fastq, member) and the deflate assembler (tests/deflate_asm.py).

GOOD[name] = (file bytes, what it inflates to); BAD[name] = (file bytes, the bytes of the members in front of the bad one, kind,
index of the bad member, reason) with kind "io" | "unsupported" and reason one of the names below (bz_core.h: plan stops and kBad*).
reference() is the verdict of Python's zlib on a file, member by member, by the same rules.

One case of the issue's list cannot exist: a level-0 member of 65 536 bytes needs 65 536 + 2 x 5 + 26 bytes and BSIZE holds at most
65 535 (total - 1).  The level-0 member here has two stored blocks of 40 000 + 25 000 bytes."""
import random
import struct
import zlib

from tests import deflate_asm as da
from tests.test_inflate_cpu import bgzf, fastq, member

BLOCK = 65280


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def blk(raw, data, extra_pre=b"", crc=None, isize=None, bsize=None, slack=b""):
    """one BGZF member around the raw deflate stream `raw` of `data`; crc / isize / bsize: forged values"""
    extra = extra_pre + b"BC\x02\x00"
    xlen = len(extra) + 2
    total = 12 + xlen + len(raw) + len(slack) + 8
    assert total <= 65536, total
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra + struct.pack("<H", total - 1 if bsize is None else bsize) +
            raw + slack + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc, len(data) if isize is None else isize))


def zblk(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw):
    return blk(raw_deflate(data, level, strategy), data, **kw)


EOF_MARKER = zblk(b"")


def blocked(data, level=6, sizes=None, rng=None, strategy=zlib.Z_DEFAULT_STRATEGY):
    out, i = [], 0
    while i < len(data):
        n = BLOCK if sizes is None else rng.randint(*sizes)
        out.append(zblk(data[i:i + n], level, strategy))
        i += n
    return b"".join(out) + EOF_MARKER


def flushed(rng, n):
    """a member with sync and full flush points inside: empty stored blocks in mid-member"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    data, raw = b"", b""
    for _ in range(n):
        d = bytes(rng.choice(b"ACGTN\n") for _ in range(rng.randint(0, 900)))
        data += d
        raw += c.compress(d) + c.flush(rng.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH]))
    raw += c.flush()
    return blk(raw, data), data


def asm_blk(blocks, history=None, **kw):
    return blk(da.deflate(blocks), da.simulate(blocks, history), **kw)


def build():
    rng = random.Random(17)
    fq = fastq(rng, 3000)
    good, bad = {}, {}
    for lv in (1, 6, 9):
        good["fastq_l%d" % lv] = (blocked(fq, lv), fq)
    good["fastq_tiny_members"] = (blocked(fq, 6, (1, 400), rng), fq)
    good["bgzf_helper"] = (bgzf(fq[:200_000]), fq[:200_000])
    good["empty_members"] = (EOF_MARKER + zblk(fq[:5000]) + EOF_MARKER + EOF_MARKER + zblk(fq[5000:9000]) + EOF_MARKER, fq[:9000])
    sized = [fq[:1], fq[1000:1000 + 65280], fq[:65536], fq[7:8]]
    good["sizes_1_65280_65536"] = (b"".join(zblk(d) for d in sized) + EOF_MARKER, b"".join(sized))
    st = [fq[:40000], fq[40000:65000]]
    good["stored_two_blocks"] = (zblk(fq[:3000]) + asm_blk([da.stored(st[0]), da.stored(st[1])]) + zblk(fq[3000:4000], 0) + EOF_MARKER,
                                 fq[:3000] + st[0] + st[1] + fq[3000:4000])
    good["fixed"] = (blocked(fq[:300_000], 6, (1, 65280), rng, zlib.Z_FIXED), fq[:300_000])
    fl = [flushed(rng, rng.randint(1, 40)) for _ in range(12)]
    good["flush_points"] = (b"".join(m for m, _ in fl) + EOF_MARKER, b"".join(d for _, d in fl))
    rnd = bytes(rng.getrandbits(8) for _ in range(100_000))
    good["random_l9"] = (blocked(rnd, 9, (20000, 60000), rng), rnd)
    # (uniform bytes are stored by zlib; a steep distribution over 256 values gives codes of up to 15 bits and second-level tables)
    skew = bytes(rng.choices(range(256), weights=[1.0 / (i + 1) ** 2.2 for i in range(256)], k=100_000))
    good["skewed_l9"] = (blocked(skew, 9, (20000, 65280), rng), skew)
    runs, run_data = [], b""
    for alt in (False, True):
        for kind in (da.dynamic, da.fixed):
            toks = [("L", 65 + len(runs))] + [("M", 258, 1)] * 40 + [("M", 3 + len(runs), 1)]
            b = [kind(toks, alt258=alt)]
            runs.append(asm_blk(b))
            run_data += da.simulate(b)
    good["one_byte_runs"] = (b"".join(runs) + EOF_MARKER, run_data)
    far_toks = [("L", rng.choice(b"ACGT")) for _ in range(32768)] + [("M", 258, 32768)] * 100 + [("M", 77, 32768), ("M", 258, 32767), ("M", 64, 1025), ("M", 65, 1024)]
    far = [da.dynamic(far_toks)]
    good["reach_back_32768"] = (zblk(fq[:2000]) + asm_blk(far) + zblk(fq[2000:3000]) + EOF_MARKER, fq[:2000] + da.simulate(far) + fq[2000:3000])
    good["other_subfield_first"] = (b"".join(zblk(fq[i:i + 30000], extra_pre=b"XY\x05\x00hello" + b"ab\x00\x00") for i in range(0, 120000, 30000)), fq[:120000])
    good["slack_in_front_of_trailer"] = (zblk(fq[:20000]) + zblk(fq[20000:30000], slack=b"\x00\x00\x00") + zblk(fq[30000:50000]) + EOF_MARKER, fq[:50000])
    good["trailing_bytes"] = (blocked(fq[:100_000]) + b"\x00\x00\x00bytes that are no gzip member" * 3, fq[:100_000])

    # ---- bad files: F1 | F2 | s1 | BAD | s2 | s3 | tail: at 64 KB of output a batch the bad member shares its batch with s2 and s3
    F1, F2, s1, s2, s3, T = fq[:40000], fq[40000:80000], fq[80000:81000], fq[81000:82000], fq[82000:83000], fq[83000:200_000]
    victim = fq[200_000:201_500]

    def around(bad_member, lead=True):
        front = [F1, F2] + ([s1] if lead else [])
        return (b"".join(zblk(d) for d in front) + bad_member + zblk(s2) + zblk(s3) + blocked(T), b"".join(front), len(front))

    def add(name, bad_member, kind, reason, lead=True):
        f, head, idx = around(bad_member, lead)
        bad[name] = (f, head, kind, idx, reason)

    ok = zblk(victim)
    flipped = bytearray(ok)
    flipped[18 + (len(ok) - 26) // 2] ^= 0x10
    add("flipped_bit", bytes(flipped), "io", "any")
    add("wrong_crc", zblk(victim, crc=zlib.crc32(victim) ^ 1), "io", "crc")
    add("isize_one_small", zblk(victim, isize=len(victim) - 1), "io", "too_long")
    add("isize_one_large", zblk(victim, isize=len(victim) + 1), "io", "too_short")
    add("bsize_cuts_data", zblk(victim, bsize=len(ok) - 1 - 40), "io", "any")
    add("isize_65537", zblk(victim, isize=65537), "io", "too_large")
    hist = F2[-32768:]
    forged = [da.dynamic([("L", c) for c in b"hello"] + [("M", 20, 15)] + [("L", c) for c in victim[:300]])]
    add("too_far", asm_blk(forged, history=hist), "io", "too_far", lead=False)
    assert da.simulate(forged, hist)[5:15] == hist[-10:]               # (what a decoder that read the previous member's tail would produce)
    add("plain_gzip_member", member(victim), "unsupported", "not_bgzf")
    # BSIZE past the end of the file (the bad member near the end, good ones behind it); a file cut inside a member
    front = [F1, F2, s1]
    f = b"".join(zblk(d) for d in front) + zblk(victim, bsize=65535) + zblk(s2) + zblk(s3) + EOF_MARKER
    bad["bsize_past_eof"] = (f, b"".join(front), "io", 3, "truncated")
    whole = b"".join(zblk(d) for d in front) + ok
    bad["cut_inside_member"] = (whole[:-300], b"".join(front), "io", 3, "truncated")
    return good, bad


GOOD, BAD = build()
SMALL = {n for n, (f, d) in GOOD.items() if len(d) <= 70_000}         # read 13 bytes a call on these only


def unsupported_offset(name):
    f, head, kind, idx, _ = BAD[name]
    assert kind == "unsupported"
    at = 0
    for _ in range(idx):
        at += walk_header(f, at)[1]
    return at


def walk_header(f, at):
    """bz_core.h parse_header on f[at:]: (header bytes, total bytes) or None"""
    h = f[at:]
    if len(h) < 18 or h[:3] != b"\x1f\x8b\x08" or h[3] != 4:
        return None
    xlen = h[10] | h[11] << 8
    p = 12
    while p + 4 <= min(len(h), 12 + xlen):
        slen = h[p + 2] | h[p + 3] << 8
        if h[p:p + 2] == b"BC" and slen == 2 and p + 6 <= len(h):
            total = (h[p + 4] | h[p + 5] << 8) + 1
            return (12 + xlen, total) if total >= 12 + xlen + 10 else None
        p += 4 + slen
    return None


def reference(f):
    """Python's zlib on the file, member by member: (bytes of the members in front of the first bad one, None) for a good file,
    (those bytes, (member index, reason)) for a bad one"""
    out, at, idx = [], 0, 0
    while at < len(f):
        if f[at] != 0x1f or (at + 1 < len(f) and f[at + 1] != 0x8b):
            break                                                       # not gzip: the end of the stream
        if len(f) - at < 18:
            return b"".join(out), (idx, "truncated")
        ht = walk_header(f, at)
        if ht is None:
            return b"".join(out), (idx, "not_bgzf")
        hdr, total = ht
        if at + total > len(f):
            return b"".join(out), (idx, "truncated")
        crc, isize = struct.unpack("<II", f[at + total - 8:at + total])
        if isize > 65536:
            return b"".join(out), (idx, "too_large")
        d = zlib.decompressobj(-15)
        try:
            data = d.decompress(f[at + hdr:at + total - 8], isize + 1)
        except zlib.error as e:
            return b"".join(out), (idx, "too_far" if "too far" in str(e) else "deflate")
        if len(data) > isize:
            return b"".join(out), (idx, "too_long")
        if not d.eof:
            return b"".join(out), (idx, "cut_short")
        if len(data) < isize:
            return b"".join(out), (idx, "too_short")
        if zlib.crc32(data) & 0xFFFFFFFF != crc:
            return b"".join(out), (idx, "crc")
        out.append(data)
        at += total
        idx += 1
    return b"".join(out), None
