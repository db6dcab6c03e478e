#!/usr/bin/env python3
"""Writes tests/golden/fake10x/: small inputs for HAST's 02.assemble_by_supernova/fake_10x.pl and what the script itself made of
them (its stdout and both outputs, decompressed; the `widths` and `long` cases gzipped again to keep them small, the fallback
cases keep only what differs from `edge`: tests/tx_model.py).  Needs perl, gzip and the script:

    python tests/golden/gen_fake10x_golden.py /path/to/HAST/02.assemble_by_supernova/fake_10x.pl

The tests read the files only; they never run this."""
import gzip
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.tx_model import FALLBACK  # noqa: E402
OUT = os.path.join(HERE, "fake10x")


def rec(head, seq, plus=b"+", qual=None):
    return head + b"\n" + seq + b"\n" + plus + b"\n" + (qual if qual is not None else b"I" * len(seq)) + b"\n"


def edge():
    heads = [b"@r#A_1/1\tx", b"@r#A_1#zz/1", b"@r/1#A_1", b"@r\t#A_1/1", b"@r#A_1\r", b"@r#A_1 /1", b"@r#/1", b"@r#", b"@r",
             b"@x#DUP/1", b"@x#NOTAB/1", b"@x#ZZ/1"]
    r1 = b"".join(rec(h, b"ACGTN"[:1 + i % 5] * 3, b"+" if i % 2 else b"+r1 text", b"!I!FF,:!"[:3 * (1 + i % 5)].ljust(3 * (1 + i % 5), b"!"))
                  for i, h in enumerate(heads))
    r1 += b"@x#A_1/1 the file ends inside this record\nACGT"
    r2 = b"".join(rec(b"@whatever %d" % i, b"TTGCA" * (1 + i % 3), b"+", b"!" + b"F" * (5 * (1 + i % 3) - 2) + b"!") for i in range(len(heads)))
    r2 += b"@x#A_1/2\nGG"
    m = b"A_1\tAAACCCGGGTTTAAAC\nA_1 \tTTTT\nDUP\tCCCCCCCCCCCCCCCC\nNOTAB\nDUP\tACG\nUNUSED\tGGGGGGGGGGGGGGGG\textra field\n"
    return r1, r2, m


def widths():
    rng = random.Random(2)
    keys = [b"%d_%d_%d" % (rng.randint(1, 1536), rng.randint(1, 1536), rng.randint(1, 1536)) for _ in range(24)]
    m = b"".join(k + b"\t" + bytes(rng.choice(b"ACGT") for _ in range(rng.choice((4, 4, 4, 16)))) + b"\n" for k in keys[:22])
    r1, r2 = [], []
    for i in range(1200):
        k = keys[23] if i in (3, 50, 97, 600) else rng.choice(keys[:23] if rng.random() < 0.1 else keys[:22])
        s1, s2 = (bytes(rng.choice(b"ACGT") for _ in range(6)) for _ in range(2))
        r1.append(rec(b"@r%d#%s/1" % (i, k), s1, b"+", bytes(rng.choice(b"!FF,:I") for _ in range(6))))
        r2.append(rec(b"@r%d#%s/2" % (i, k), s2, b"+", bytes(rng.choice(b"!FF,:I") for _ in range(6))))
    return b"".join(r1), b"".join(r2), m


def long_reads():
    rng = random.Random(3)
    lens = (0, 1, 63, 64, 65, 150, 300, 20000, 20000, 64, 20000)         # (three long ones: a run in blocks of one record takes several steps)
    r1, r2 = [], []
    for i, n in enumerate(lens):
        n2 = lens[len(lens) - 1 - i]
        for n_, out, side in ((n, r1, 1), (n2, r2, 2)):
            # motifs of 61 and 67 bytes repeated (coprime with the 64 bytes of a copy step; the files gzip to a few KB)
            motif, qmotif = bytes(rng.choice(b"ACGTN") for _ in range(61)), bytes(rng.choice(b"FF,:I!") for _ in range(67))
            q = bytearray((qmotif * (n_ // 67 + 1))[:n_])
            if n_:
                q[0] = q[-1] = ord("!")
            out.append(rec(b"@long%d#%s/%d" % (i, b"7_8_9" if i != 2 else b"none", side), (motif * (n_ // 61 + 1))[:n_],
                           b"+long%d with text" % i, bytes(q)))
    return b"".join(r1), b"".join(r2), b"7_8_9\tACGTACGTACGTACGT\n"


def main():
    script = os.path.abspath(sys.argv[1])
    e = edge()
    cases = {"edge": e, "widths": widths(), "long": long_reads()}
    cases.update({name: (e[0], e[1], e[2] + line) for name, (line, _) in FALLBACK.items()})
    kept = {}
    for name, (r1, r2, m) in cases.items():
        d = os.path.join(OUT, name)
        with tempfile.TemporaryDirectory() as tmp:
            for fn, data in (("r1.fq.gz", r1), ("r2.fq.gz", r2)):
                with gzip.open(os.path.join(tmp, fn), "wb") as f:
                    f.write(data)
            with open(os.path.join(tmp, "map.txt"), "wb") as f:
                f.write(m)
            res = subprocess.run(["perl", script, "r1.fq.gz", "r2.fq.gz", "map.txt"], cwd=tmp, stdout=subprocess.PIPE, check=True)
            outs = [gzip.open(os.path.join(tmp, "SampleName_S1_L001_R%d_001.fastq.gz" % s)).read() for s in (1, 2)]
        kept[name] = (res.stdout, outs)
        if name in FALLBACK and kept[name] == kept["edge"]:      # nothing of its own to keep: the tests read edge's files
            print(name, "as edge")
            continue
        files = [("stdout.txt", res.stdout), ("out1.fq", outs[0]), ("out2.fq", outs[1])]
        if name not in FALLBACK:
            files += [("map.txt", m), ("r1.fq", r1), ("r2.fq", r2)]
        os.makedirs(d, exist_ok=True)
        for fn, data in files:
            if fn.endswith(".fq") and name in ("widths", "long"):        # the larger cases are kept gzipped
                fn, data = fn + ".gz", gzip.compress(data, 9, mtime=0)
            with open(os.path.join(d, fn), "wb") as f:
                f.write(data)
        print(name, res.stdout.decode().splitlines()[-1])


if __name__ == "__main__":
    main()
