"""gzip files no zlib deflate would write (a helper, not a test), assembled token by token with tests/deflate_asm.py:

    VALID      {name: (file, bytes)}   legal deflate; zlib's inflate gives exactly the simulated bytes (asserted here, at import)
    MUST_FAIL  {name: (file, prefix)}  zlib raises (asserted here); the trailer is right for what a lenient decoder would produce, so
                                       only the decoder's own checks can refuse the file; prefix = the valid bytes in front of the damage
    LENIENT    {name: (file, bytes)}   zlib raises, yet the bytes are well defined (codes that are incomplete but never miss)

What zlib's encoder never does and these do: distances above 32 506 up to the full 32 768 (behind ~35 000 literals, so that every
match has a whole window behind it), blocks that start with such a match (a chunk of the parallel decoders that starts there holds
nothing but markers for the OLDEST bytes of its window), 15-bit codes and 48-bit tokens, blocks without distance codes, a lone
distance code, length 258 as code 284 + 31, far matches right behind stored and fixed blocks, code-length runs over the
literal/distance border; members whose matches reach in front of their own first byte.  Deterministic: fixed seeds."""
import random
import struct
import zlib

from tests import deflate_asm as da
from tests.deflate_asm import canonical, dynamic, fixed, lens_from, member, raw, simulate, stored, write_dynamic_header, write_tokens

_POP = b"ACGT" + b"\n" + b"F:,#@" + b"0123456789"
_WEIGHTS = [20, 20, 20, 20, 3, 8, 3, 3, 1, 1] + [1] * 10


def lits(rng, n, pop=_POP, weights=_WEIGHTS):
    return [("L", b) for b in rng.choices(pop, weights, k=n)]


def opening(rng, n=35_000):
    """~n literals in dynamic blocks of 300 to 700 tokens: behind them every match has 32 768 bytes to reach into"""
    blocks = []
    while n > 0:
        k = min(n, rng.randint(300, 700))
        blocks.append(dynamic(lits(rng, k), header=rng.choice(["plain", "rle"])))
        n -= k
    return blocks


def zlib_inflate(blob):
    out, rest = b"", blob
    while rest[:2] == b"\x1f\x8b":
        d = zlib.decompressobj(31)
        out += d.decompress(rest)
        assert d.eof
        rest = d.unused_data
    return out


def zlib_refuses(blob):
    try:
        zlib_inflate(blob)
    except zlib.error:
        return True
    return False


def block_bytes(blocks):
    """compressed size of every block, in bytes (rounded up)"""
    bw, sizes = da.BitWriter(), []
    for i, b in enumerate(blocks):
        at = bw.bit_length()
        da.write_block(bw, b, i == len(blocks) - 1)
        sizes.append((bw.bit_length() - at + 7) // 8)
    return sizes


VALID, MUST_FAIL, LENIENT = {}, {}, {}
FAR = 32768


def _valid(name, blocks):
    blob, want = member(blocks), simulate(blocks)
    assert zlib_inflate(blob) == want, name                             # zlib is the reference: the assembler's own simulation must agree with it
    assert len(blob) < 150_000, (name, len(blob))
    VALID[name] = (blob, want)


def far_blocks(rng, n, pop=_POP, weights=_WEIGHTS):
    blocks = []
    for i in range(n):
        toks = [("M", (3, 4, 63, 64, 65, 66, 129, 258)[i % 8], FAR)] + lits(rng, rng.randint(150, 400), pop, weights)
        for _ in range(rng.randint(1, 6)):
            toks.append(("M", rng.choice([3, 64, 65, 200, 258]), rng.choice([FAR, 32767, 32507, 32506, 24577, 16385, 513, 512, 1])))
            toks += lits(rng, rng.randint(0, 2), pop, weights)
        blocks.append(dynamic(toks, header=("plain", "rle")[i & 1]))
    return blocks


def _far():
    rng = random.Random(101)
    _valid("far", opening(rng) + far_blocks(rng, 84))


def far_for_a_ring(min_bytes):
    """A far-match stream of its own (seed 102, not the `far` case's 101), built like `far` and padded with further far-match blocks
    (literals of all 256 byte values: ~a byte of deflate each) until the file is larger than min_bytes -- for the ring of compressed
    bytes on the device, which smaller files do not go round"""
    rng = random.Random(102)
    blocks = opening(rng) + far_blocks(rng, 84)
    every = bytes(range(256))
    size = sum(block_bytes(blocks))
    while size <= min_bytes + 64:
        more = far_blocks(rng, 40, every, [1] * 256)
        size += sum(block_bytes(more))
        blocks += more
    blob, want = member(blocks), simulate(blocks)
    assert zlib_inflate(blob) == want and len(blob) > min_bytes
    return blob, want


def _far_small_blocks():
    rng = random.Random(103)
    blocks = opening(rng)
    n0 = len(blocks)
    for i in range(340):
        blocks.append(dynamic([("M", (3, 4, 63, 64, 65, 66, 129, 258)[i % 8], FAR)] + lits(rng, rng.randint(300, 480))))
    blocks.append(dynamic(lits(rng, 10)))                               # (the final block: the 340 in front of it are non-final)
    sizes = block_bytes(blocks)[n0:]
    assert len(sizes) >= 300 and max(sizes) <= 260, max(sizes)
    _valid("far_small_blocks", blocks)


# literal/length and distance codes over 16 symbols each, lengths 1, 2, ..., 14, 15, 15
LADDER_LL = [ord(c) for c in "ACGT\nF:"] + [256, 257, 264, 269, ord("N"), 277, 285, 284, ord("Z")]
LADDER_D = [0, 1, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 24, 27, 29, 28]
_LADDER_LENS = list(range(1, 16)) + [15]


def _ladder15():
    rng = random.Random(104)
    ll = dict(zip(LADDER_LL, _LADDER_LENS))
    d = dict(zip(LADDER_D, _LADDER_LENS))
    pop, w = b"ACGT\nF:NZ", [30, 20, 12, 8, 5, 3, 2, 2, 2]
    reach = {0: [1], 1: [2], 2: [3], 4: [5, 6], 6: [9, 12], 8: [17, 24], 10: [33, 48], 12: [65, 96], 14: [129, 192], 16: [257, 384],
             18: [513, 768], 20: [1025, 1536], 24: [4097, 6144], 27: [12289, 16384], 28: [16385, 24576], 29: [24577, 30000, 32767, FAR]}
    assert sorted(reach) == sorted(LADDER_D)
    blocks = opening(rng)
    for i in range(124):
        toks = [("M", 257, FAR)]                                        # 15 + 5 + 15 + 13 = 48 bits
        for _ in range(rng.randint(8, 20)):
            toks += lits(rng, rng.randint(1, 30), pop, w)
            toks.append(("M", rng.choice([3, 10, 19, 22, 67, 82, 227, 240, 257, 258]), rng.choice(reach[rng.choice(LADDER_D)])))
        # long codes back to back, then the widest token at whatever bit offset of the step that leaves it at
        toks += lits(rng, rng.randint(1, 4), b"NZ", [1, 1]) + [("M", 257, rng.choice([FAR, 32767, 24577 + 8191]))]
        toks += lits(rng, rng.randint(0, 5), pop, w)
        blocks.append(dynamic(toks, ll_lens=ll, d_lens=d, header=("plain", "rle")[i & 1]))
    _valid("ladder15", blocks)


def _no_dist_codes():
    rng = random.Random(105)
    blocks = opening(rng)
    for i in range(30):
        blocks.append(dynamic(lits(rng, rng.randint(50, 900)), d_lens=[0], header=("plain", "rle")[i & 1]))      # HDIST = 1, that one length 0
    _valid("no_dist_codes", blocks)


def _lone_far_dist():
    rng = random.Random(106)
    blocks = opening(rng)
    for i in range(60):
        toks = []
        for _ in range(rng.randint(1, 8)):
            toks.append(("M", rng.choice([3, 5, 64, 65, 130, 258]), rng.choice([24577, 30000, FAR])))
            toks += lits(rng, rng.randint(0, 120))
        blocks.append(dynamic(toks, d_lens={29: 1}))
    _valid("lone_far_dist", blocks)


def _len258_as_284():
    rng = random.Random(107)
    blocks = opening(rng)
    for i in range(60):
        toks = []
        for _ in range(rng.randint(1, 6)):
            toks.append(("M", 258, rng.choice([1, 300, 32767, FAR])))
            toks += lits(rng, rng.randint(0, 150))
        blocks.append((dynamic if i % 3 else fixed)(toks, alt258=True))
    _valid("len258_as_284", blocks)


def _far_after_stored_and_fixed():
    rng = random.Random(108)
    blocks = opening(rng)
    for i in range(48):
        n = (0, 1, 300, 5000)[i % 4]
        blocks.append(stored(bytes(rng.choices(_POP, _WEIGHTS, k=n))))
        toks = [("M", rng.choice([3, 64, 65, 129, 258]), FAR)] + lits(rng, rng.randint(20, 300))
        if i % 3 != 2:                                                  # two Huffman blocks in three are fixed ones, with far matches inside as well
            toks += [("M", rng.choice([4, 70, 258]), FAR)] + lits(rng, rng.randint(0, 40)) + [("M", 3, 32767)]
            blocks.append(fixed(toks))
            if i % 3 == 1:
                blocks.append(dynamic([("M", 66, FAR)] + lits(rng, rng.randint(100, 400))))
        else:
            blocks.append(dynamic(toks, header="plain"))
    _valid("far_after_stored_and_fixed", blocks)


def _rle_header():
    rng = random.Random(109)
    # ten 4-bit literal/length codes, '\n' 3 bits, end of block 2 bits; sixteen 4-bit distance codes: the lengths of 282 .. 285 and of
    # distance codes 0 .. 15 are one run of twenty 4s over the border between the two alphabets
    ll = {256: 2, ord("\n"): 3}
    for s in [ord(c) for c in "ACGTF:"] + [282, 283, 284, 285]:
        ll[s] = 4
    d = dict((s, 4) for s in range(16))
    seq = lens_from(ll, 286) + lens_from(d, 16)
    syms = da.code_length_symbols(seq, True)
    at, spans = 0, False
    for s, extra, _ in syms:                                            # (where every symbol's run lies: one must hold lengths of both alphabets)
        n = 1 if s < 16 else extra + (3 if s < 18 else 11)
        spans = spans or (s == 16 and at < 286 < at + n)
        at += n
    assert spans and set(s for s, _, _ in syms) >= {16, 17, 18}
    blocks = opening(rng)
    for i in range(40):
        toks = lits(rng, rng.randint(5, 60), b"ACGTF:\n", [5, 5, 5, 5, 2, 2, 1])
        for _ in range(rng.randint(1, 5)):
            toks.append(("M", rng.choice([163, 194, 195, 226, 227, 257, 258]), rng.randint(1, 256)))
            toks += lits(rng, rng.randint(0, 60), b"ACGTF:\n", [5, 5, 5, 5, 2, 2, 1])
        blocks.append(dynamic(toks, ll_lens=ll, d_lens=d, header="rle"))
    _valid("rle_header", blocks)


def _zero_codes_are_a_far_match():
    """In these blocks the all-zero bit string is a TOKEN: literal/length code 0 is 257 (length 3), the lone distance code is 29, so
    zeros decode to a match at distance 24 577.  A decoder that reads a block on into the zero padding behind its input buffer (the
    threaded decoder, when a block straddles the end of what it has read) decodes such tokens before it rolls the block back -- they
    are no stream data and must not count as a reach in front of the member, which begins less than 24 577 bytes back.  Blocks of
    1500 'A' (375 bytes) behind literal blocks of many sizes, so that some straddle the buffer end at every small chunk size."""
    rng = random.Random(113)
    ll, d = {257: 1, ord("A"): 2, ord("C"): 3, 256: 3}, {29: 1}
    blocks = []
    for size in (120, 150, 210, 260, 300, 330, 390):
        blocks.append(dynamic(lits(rng, size)))
        blocks.append(dynamic([("L", ord(c)) for c in "CAC"], ll_lens=ll, d_lens=d))
        blocks.append(dynamic([("L", ord("A"))] * 1500, ll_lens=ll, d_lens=d))
    blocks.append(dynamic(lits(rng, 200)))
    assert len(simulate(blocks)) < 24577
    _valid("zero_codes_are_a_far_match", blocks)


# ---- files that must be refused ----------------------------------------------------------------------------------------------------
def _must_fail(name, blob, prefix):
    assert zlib_refuses(blob), name
    assert len(blob) < 150_000, (name, len(blob))
    MUST_FAIL[name] = (blob, prefix)


def _forged_members():
    rng = random.Random(110)
    first = opening(rng)
    m1, out1 = member(first), simulate(first)
    assert len(out1) >= 32768
    tail = lits(rng, 500)
    # member 2's first token reaches 32 768 bytes in front of the member's first byte
    # (a non-final block: the parallel decoders' searches look for those, and one that finds it arrives at the member's start as a candidate)
    second = [dynamic([("M", 100, FAR)] + tail), dynamic(lits(rng, 300))]
    # ... and the same reach behind 20 000 literals of the member's own: 12 768 bytes in front of its first byte
    late = opening(rng, 20_000)
    late_prefix = simulate(late)
    late = late + [dynamic([("M", 100, FAR)] + tail), dynamic(lits(rng, 300))]
    for hist_name, hist in (("prev", out1[-32768:]), ("zeros", bytes(32768))):
        _must_fail("cross_member_" + hist_name, m1 + member(second, history=hist), out1)
        _must_fail("cross_member_late_" + hist_name, m1 + member(late, history=hist), out1 + late_prefix)
    _must_fail("too_far_first", member([dynamic([("M", 10, 1)] + tail), dynamic(lits(rng, 300))], history=bytes(32768)), b"")


def _raw_dynamic(tokens, ll, d, eob=True, written=None, **hdr):
    """a dynamic block whose header is written without the assembler's checks; written: the tokens to put into the stream (default: all)"""
    ll, d = lens_from(ll, 286) if isinstance(ll, dict) else ll, lens_from(d, 30) if isinstance(d, dict) else d

    def fn(bw, final):
        bw.put(1 if final else 0, 1)
        bw.put(2, 2)
        write_dynamic_header(bw, ll, d, check=False, **hdr)
        write_tokens(bw, tokens if written is None else written, canonical(ll), canonical(d), eob=eob)
    return raw(fn, tokens)


def _trailer_for(blocks):
    """a member with the trailer of ALL the blocks' simulated bytes -- what a decoder lenient enough to get through them would check"""
    return member(blocks)


def _structural():
    rng = random.Random(111)
    good = [dynamic(lits(rng, 600)), dynamic([("M", 20, 7)] + lits(rng, 300))]
    prefix = simulate(good)
    ten = lits(rng, 10)
    ll_plain, d_plain = da.token_lengths(ten, False)

    def typed(btype):
        def fn(bw, final):
            bw.put(1 if final else 0, 1)
            bw.put(btype, 2)
        return fn
    _must_fail("block_type_3", _trailer_for(good + [raw(typed(3))]), prefix)

    def bad_stored(bw, final):
        typed(0)(bw, final)
        bw.align()
        bw.put_bytes(struct.pack("<HH", 10, (10 ^ 0xFFFF) ^ 0x0100) + bytes(t[1] for t in ten))
    _must_fail("stored_len_nlen", _trailer_for(good + [raw(bad_stored, ten)]), prefix)

    seq = ll_plain[:257] + d_plain[:1]
    normal = da.code_length_symbols(seq, True)
    _must_fail("repeat_first", _trailer_for(good + [_raw_dynamic(ten, ll_plain, d_plain, cl_syms=[(16, 0, 2)] + normal)]), prefix)
    _must_fail("too_many_lengths", _trailer_for(good + [_raw_dynamic(ten, ll_plain, d_plain, cl_syms=normal[:-1] + [(18, 127, 7)])]), prefix)
    no_eob = {ord("A"): 1, ord("C"): 2, ord("G"): 2}                     # complete, and nothing for 256
    acg = lits(rng, 20, b"ACG", [1, 1, 1])
    _must_fail("no_end_of_block_code", _trailer_for(good + [_raw_dynamic(acg, no_eob, [0], eob=False, hlit=257)]), prefix)
    over = {ord("A"): 1, ord("C"): 1, 256: 1}
    _must_fail("oversubscribed", _trailer_for(good + [_raw_dynamic(lits(rng, 20, b"AC", [1, 1]), over, [0])]), prefix)

    fx_ll, fx_d = canonical(da.FIXED_LL), canonical(da.FIXED_D)

    def fixed_286(bw, final):
        typed(1)(bw, final)
        write_tokens(bw, ten, fx_ll, fx_d, eob=False)
        bw.put_code(*fx_ll[286])
        bw.put_code(*fx_ll[256])
    _must_fail("fixed_symbol_286", _trailer_for(good + [raw(fixed_286, ten)]), prefix + bytes(t[1] for t in ten))

    def fixed_dist_30(bw, final):
        typed(1)(bw, final)
        write_tokens(bw, ten, fx_ll, fx_d, eob=False)
        bw.put_code(*fx_ll[257])                                        # a match of length 3 ...
        bw.put_code(*fx_d[30])                                          # ... at a distance code that stands for nothing
        bw.put_code(*fx_ll[256])
    _must_fail("fixed_distance_30", _trailer_for(good + [raw(fixed_dist_30, ten)]), prefix + bytes(t[1] for t in ten))


def _lenient():
    rng = random.Random(112)
    good = [dynamic(lits(rng, 600))]
    toks = lits(rng, 400) + [("M", 30, 100)] + lits(rng, 50)
    ll, d = da.token_lengths(toks, False)

    def add(name, block):
        blocks = good + [block, dynamic(lits(rng, 100))]
        blob, want = member(blocks), simulate(blocks)
        assert zlib_refuses(blob), name
        LENIENT[name] = (blob, want)

    # an incomplete code-length code: one of its codes a bit longer than the Huffman build made it (still prefix-free, never misses)
    seq = ll[:max(s for s, l in enumerate(ll) if l) + 1] + d[:max(s for s, l in enumerate(d) if l) + 1]
    syms = da.code_length_symbols(seq, True)
    freq = {}
    for s, _, _ in syms:
        freq[s] = freq.get(s, 0) + 1
    cl = da.huffman_lengths(freq, 19, 7)
    s = max((s for s in range(19) if 0 < cl[s] < 7), key=lambda s: cl[s])
    cl[s] += 1
    assert da.kraft(cl, 7) < 128
    add("incomplete_code_length_code", _raw_dynamic(toks, ll, d, cl_syms=syms, cl_lens=cl))
    # an incomplete literal/length code whose missing codes are never used
    ll2 = list(ll)
    s = max((s for s in range(286) if 0 < ll2[s] < 15), key=lambda s: ll2[s])
    ll2[s] += 1
    assert da.kraft(ll2) < 1 << 15
    add("incomplete_literal_length_code", _raw_dynamic(toks, ll2, d))


_far()
_far_small_blocks()
_ladder15()
_no_dist_codes()
_lone_far_dist()
_len258_as_284()
_far_after_stored_and_fixed()
_rle_header()
_zero_codes_are_a_far_match()
_forged_members()
_structural()
_lenient()
