"""A deflate ASSEMBLER for tests (a helper, not a test): gzip members written token by token, so that a stream can hold what zlib's
deflate never emits -- distances up to 32 768, chosen code lengths (15-bit codes, 48-bit tokens), blocks without distance codes, a
lone distance code, length 258 as code 284 + 31, code-length runs that span the literal/distance border -- and, through the raw
escape, structures that are not deflate at all.  Standard library and zlib (for crc32) only; what the streams inflate to is
simulated here (apply) and compared with zlib's inflate by the corpus that uses this (tests/gz_crafted_corpus.py).

    tokens  ('L', byte) | ('M', length 3..258, distance 1..32768)
    blocks  dynamic(tokens, ...) | fixed(tokens, ...) | stored(data) | raw(fn, tokens)
    member(blocks, history=None) -> bytes of one gzip member
"""
import heapq
import struct
import zlib

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
EOB = 256
WINDOW = 32768
_REVERSED = {}                          # (code, length) -> the code's bits in the order they are written


class BitWriter:
    """bits go out LSB first, as RFC 1951 packs them"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, bits, n):
        """the raw escape: the low n bits of `bits`, lowest first"""
        assert 0 <= bits < (1 << n) or n == 0
        self.acc |= bits << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, n):
        """a Huffman code: its most significant bit goes first"""
        rev = _REVERSED.get((code, n))
        if rev is None:
            rev = _REVERSED[(code, n)] = int(format(code, "0%db" % n)[::-1], 2) if n else 0
        self.put(rev, n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def put_bytes(self, data):
        assert self.n == 0
        self.out += data

    def bit_length(self):
        return len(self.out) * 8 + self.n

    def bytes(self):
        assert self.n == 0
        return bytes(self.out)


def kraft(lens, unit=15):
    """sum of 2^(unit - len) over the used codes: 2^unit for a complete code"""
    return sum(1 << (unit - l) for l in lens if l)


def canonical(lens):
    """{symbol: (code, length)} for code lengths given per symbol (0 = unused), RFC 1951 3.2.2"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = {}
    for s, l in enumerate(lens):
        if l:
            codes[s] = (nxt[l], l)
            nxt[l] += 1
    return codes


def huffman_lengths(freq, n_syms, max_len):
    """a plain Huffman build: code lengths for the symbols with freq > 0 (at least two get a code, so the code is complete)"""
    freq = dict((s, f) for s, f in freq.items() if f > 0)
    for filler in range(n_syms):
        if len(freq) >= 2:
            break
        freq.setdefault(filler, 1)
    while True:
        heap = [(f, s, (s,)) for s, f in sorted(freq.items())]
        heapq.heapify(heap)
        depth = dict((s, 0) for s in freq)
        while len(heap) > 1:
            fa, ka, a = heapq.heappop(heap)
            fb, kb, b = heapq.heappop(heap)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
        if max(depth.values()) <= max_len:
            break
        freq = dict((s, (f + 1) // 2 + 1) for s, f in freq.items())      # flatter, until the tree is shallow enough
    lens = [0] * n_syms
    for s, d in depth.items():
        lens[s] = d
    assert kraft(lens) == 1 << 15
    return lens


def length_symbol(length, alt258=False):
    """(literal/length symbol, extra bits, number of extra bits)"""
    assert 3 <= length <= 258
    if length == 258 and alt258:
        return 284, 31, 5                                                # 227 + 31: legal, and no encoder writes it
    i = max(k for k in range(29) if LEN_BASE[k] <= length)
    if length == 258:
        i = 28
    assert length - LEN_BASE[i] < (1 << LEN_EXTRA[i]) or LEN_EXTRA[i] == 0 and length == LEN_BASE[i]
    return 257 + i, length - LEN_BASE[i], LEN_EXTRA[i]


def distance_symbol(distance):
    assert 1 <= distance <= WINDOW
    i = max(k for k in range(30) if DIST_BASE[k] <= distance)
    return i, distance - DIST_BASE[i], DIST_EXTRA[i]


def apply(out, tokens):
    """what the tokens inflate to, appended to bytearray `out` (which holds whatever history they may copy from)"""
    for t in tokens:
        if t[0] == "L":
            out.append(t[1])
        else:
            _, length, distance = t
            assert 3 <= length <= 258 and 1 <= distance <= len(out), t
            for _ in range(length):
                out.append(out[-distance])
    return out


def lens_from(table, n):
    """code lengths as a list of n from {symbol: length}"""
    lens = [0] * n
    for s, l in table.items():
        lens[s if isinstance(s, int) else ord(s)] = l
    return lens


# ---- blocks --------------------------------------------------------------------------------------------------------------------
def dynamic(tokens, ll_lens=None, d_lens=None, alt258=False, header="rle"):
    """ll_lens / d_lens: explicit code lengths ({symbol: length} or lists), else a plain Huffman build over what the tokens use.
    header: "plain" = every code length sent on its own, "rle" = runs sent with symbols 16, 17 and 18 (a run goes on from the
    literal/length lengths into the distance lengths where the values allow it)"""
    return ("dynamic", list(tokens), dict(ll_lens=ll_lens, d_lens=d_lens, alt258=alt258, header=header))


def fixed(tokens, alt258=False):
    return ("fixed", list(tokens), dict(alt258=alt258))


def stored(data):
    data = bytes(data)
    assert len(data) <= 0xFFFF
    return ("stored", [("L", b) for b in data], dict(data=data))


def raw(fn, tokens=()):
    """fn(bw, final) writes the block's bits itself (put / put_code); `tokens`: what a decoder that got through it would produce"""
    return ("raw", list(tokens), dict(fn=fn))


def code_length_symbols(seq, rle):
    """the code-length alphabet's symbols for the sequence of lengths: [(symbol, extra bits, number of extra bits)]"""
    if not rle:
        return [(v, 0, 0) for v in seq]
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                out.append((18, n - 11, 7))
                run -= n
            if run >= 3:
                out.append((17, run - 3, 3))
                run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                n = min(run, 6)
                out.append((16, n - 3, 2))
                run -= n
            out += [(v, 0, 0)] * run
    return out


def write_dynamic_header(bw, ll_lens, d_lens, header="rle", cl_syms=None, cl_lens=None, check=True, hlit=None, hdist=None):
    """HLIT, HDIST, HCLEN, the code-length code, the code lengths.  cl_syms / cl_lens / check=False: for streams that are meant to
    be wrong (explicit code-length symbols, an explicit code-length code, no completeness checks)"""
    ll_lens, d_lens = list(ll_lens), list(d_lens)
    if hlit is None:
        hlit = max([257] + [s + 1 for s, l in enumerate(ll_lens) if l])
    if hdist is None:
        hdist = max([1] + [s + 1 for s, l in enumerate(d_lens) if l])
    ll_lens += [0] * (hlit - len(ll_lens))
    d_lens += [0] * (hdist - len(d_lens))
    if check:
        assert hlit <= 286 and hdist <= 30 and ll_lens[EOB]
        assert kraft(ll_lens[:hlit]) == 1 << 15, "the literal/length code must be complete"
        used = [l for l in d_lens[:hdist] if l]
        assert not used or used == [1] or kraft(used) == 1 << 15, "distance code: complete, one lone code, or none"
    seq = ll_lens[:hlit] + d_lens[:hdist]
    if cl_syms is None:
        cl_syms = code_length_symbols(seq, header == "rle")
    if cl_lens is None:
        freq = {}
        for s, _, _ in cl_syms:
            freq[s] = freq.get(s, 0) + 1
        cl_lens = huffman_lengths(freq, 19, 7)
    codes = canonical(cl_lens)
    hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
    bw.put(hlit - 257, 5)
    bw.put(hdist - 1, 5)
    bw.put(hclen - 4, 4)
    for i in range(hclen):
        bw.put(cl_lens[CL_ORDER[i]], 3)
    for s, extra, nbits in cl_syms:
        bw.put_code(*codes[s])
        bw.put(extra, nbits)


def write_tokens(bw, tokens, ll_codes, d_codes, alt258=False, eob=True):
    for t in tokens:
        if t[0] == "L":
            bw.put_code(*ll_codes[t[1]])
        else:
            s, extra, nbits = length_symbol(t[1], alt258)
            bw.put_code(*ll_codes[s])
            bw.put(extra, nbits)
            s, extra, nbits = distance_symbol(t[2])
            bw.put_code(*d_codes[s])
            bw.put(extra, nbits)
    if eob:
        bw.put_code(*ll_codes[EOB])


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def token_lengths(tokens, alt258):
    """code lengths by a plain Huffman build over the symbols the tokens (and the end-of-block code) use"""
    lf, df = {EOB: 1}, {}
    for t in tokens:
        if t[0] == "L":
            lf[t[1]] = lf.get(t[1], 0) + 1
        else:
            s = length_symbol(t[1], alt258)[0]
            lf[s] = lf.get(s, 0) + 1
            s = distance_symbol(t[2])[0]
            df[s] = df.get(s, 0) + 1
    ll = huffman_lengths(lf, 286, 15)
    if not df:
        d = [0]
    elif len(df) == 1:
        d = lens_from({list(df)[0]: 1}, 30)                              # one lone code of one bit
    else:
        d = huffman_lengths(df, 30, 15)
    return ll, d


def write_block(bw, block, final):
    kind, tokens, opt = block
    if kind == "raw":
        opt["fn"](bw, final)
        return
    bw.put(1 if final else 0, 1)
    if kind == "stored":
        bw.put(0, 2)
        bw.align()
        bw.put_bytes(struct.pack("<HH", len(opt["data"]), len(opt["data"]) ^ 0xFFFF) + opt["data"])
    elif kind == "fixed":
        bw.put(1, 2)
        write_tokens(bw, tokens, canonical(FIXED_LL), canonical(FIXED_D), opt["alt258"])
    else:
        bw.put(2, 2)
        ll, d = opt["ll_lens"], opt["d_lens"]
        if ll is None:
            ll, d0 = token_lengths(tokens, opt["alt258"])
            d = d0 if d is None else d
        if d is None:
            d = [0]
        ll = lens_from(ll, 286) if isinstance(ll, dict) else list(ll)
        d = lens_from(d, 30) if isinstance(d, dict) else list(d)
        write_dynamic_header(bw, ll, d, opt["header"])
        write_tokens(bw, tokens, canonical(ll), canonical(d), opt["alt258"])


def deflate(blocks):
    """the raw deflate stream of the blocks; the last one is the final block"""
    bw = BitWriter()
    for i, b in enumerate(blocks):
        write_block(bw, b, i == len(blocks) - 1)
    bw.align()
    return bw.bytes()


def simulate(blocks, history=None):
    """the bytes the blocks' tokens stand for, simulated on top of `history`"""
    out = bytearray(history or b"")
    for _, tokens, _ in blocks:
        apply(out, tokens)
    return bytes(out[len(history or b""):])


GZ_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"


def member(blocks, history=None):
    """One gzip member.  history (32 768 bytes): the tokens are simulated on top of it, so matches may reach in front of the member's
    first byte, and CRC-32 and ISIZE cover only the member's own simulated bytes -- a FORGERY: a file no inflate may accept, with the
    trailer a decoder that did resolve those matches (against the bytes in front of the member) would find correct."""
    assert history is None or len(history) == WINDOW
    data = simulate(blocks, history)
    return GZ_HEADER + deflate(blocks) + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)
