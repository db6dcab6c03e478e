"""route_gz.sh's ratio line for one routed .fastq.gz: the file's leading members (up to ~64 MB of plain bytes) as the GPU's encoder
wrote them against zlib on the same plain bytes -- cut into the encoder's 16-KB pieces (levels 1 and 6, each piece a raw deflate
stream: what a piece-wise encoder can reach) and whole (levels 1 and 6).  The comparison is zlib, never the encoder's earlier output."""
import os
import sys
import zlib

PIECE, LIMIT = 16384, 64 << 20


def main(path):
    blob = open(path, "rb").read(LIMIT)                     # (at least as many compressed bytes as the sample needs)
    plain, used, rest = [], 0, blob
    while rest[:2] == b"\x1f\x8b" and sum(map(len, plain)) < LIMIT:
        d = zlib.decompressobj(31)
        try:
            out = d.decompress(rest)
        except zlib.error:
            break
        if not d.eof:                                       # (a member cut by the read limit)
            break
        plain.append(out)
        used += len(rest) - len(d.unused_data)
        rest = d.unused_data
    data = b"".join(plain)
    if not data:
        print("   %s: no complete member in the first %d bytes" % (os.path.basename(path), LIMIT))
        return 1

    def pieces(level):
        n = 0
        for i in range(0, len(data), PIECE):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            n += len(c.compress(data[i:i + PIECE])) + len(c.flush())
        return n

    row = {"encoder": used, "zlib1_pieces": pieces(1), "zlib6_pieces": pieces(6), "zlib1_whole": len(zlib.compress(data, 1)), "zlib6_whole": len(zlib.compress(data, 6))}
    print("   %s: %d members, %d plain bytes: " % (os.path.basename(path), len(plain), len(data)) +
          " ".join("%s=%d (%.4f)" % (k, v, v / len(data)) for k, v in row.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
