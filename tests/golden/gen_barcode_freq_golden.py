#!/usr/bin/env python3
"""Writes tests/golden/barcode_freq/: small read-1 files and what the line of HAST's 02.assemble_by_supernova/assemble_by_supernova.sh
that writes barcode_freq.txt made of them, its rows sorted with LC_ALL=C (awk prints them in its hash order).  Needs bash, gzip,
awk, sort and the script, out of which the line is taken when this runs:

    python tests/golden/gen_barcode_freq_golden.py /path/to/HAST/02.assemble_by_supernova/assemble_by_supernova.sh

<case>.fq is the input, <case>.txt the sorted rows.  The tests read the files only; they never run this."""
import gzip
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "barcode_freq")


def rec(head, seq=b"ACGT", plus=b"+", qual=None):
    return head + b"\n" + seq + b"\n" + plus + b"\n" + (qual if qual is not None else b"I" * len(seq)) + b"\n"


def edge_body():
    """every branch of the rule; fields of 0, 1, 15, 16 and 40 bytes; an empty header line; separators in lines that do not count"""
    heads = [b"@r#1_2_3/1", b"@r#1_2_3/1\tx y", b"@r/1", b"@r/1#A_1", b"@r#", b"@r##x", b"@r#ab\r", b"@r", b"", b"r#K1/1", b"@r#0_0_0/1",
             b"@r#0_0_0/1", b"@r#Z/1", b"@r#123456789012345/1", b"@r#1234567890123456/1", b"@r#" + b"L" * 40 + b"/1", b"@r#n\0ul/1",
             b"@r#a b/1", b"@r#ta\tb", b"#", b"/", b"@r#1234567890123456/2", b"@no separator at all", b"@r#1_2_3#zz/1"]
    return b"".join(rec(h, b"AC#GT/"[:2 + i % 5], b"+" if i % 2 else b"+r#NOT_A_KEY/1", b"#/I#/!"[:2 + i % 5]) for i, h in enumerate(heads))


HEAVY_RUNS = (65, 150, 100, 128, 70, 90, 149, 148)      # 900 of 3 000 records: each run longer than a wave of 64


def many():
    """3 000 records over about 400 barcodes; one barcode (0_0_0) owns 30 % of them, in runs of 65 to 150 records between
    stretches of the others"""
    rng = random.Random(5)
    keys = sorted({b"%d_%d_%d" % (rng.randint(1, 1536), rng.randint(1, 1536), rng.randint(1, 1536)) for _ in range(396)})
    keys += [b"1536_1536_1536_a", b"1536_1536_1536_bb", b""]          # two longer than a text record, and the empty key
    n_other = 3000 - sum(HEAVY_RUNS)
    stretch = [n_other // (len(HEAVY_RUNS) + 1)] * (len(HEAVY_RUNS) + 1)
    stretch[-1] += n_other - sum(stretch)
    heads = []
    for g, n in enumerate(stretch):
        heads += [rng.choice(keys) for _ in range(n)]
        if g < len(HEAVY_RUNS):
            heads += [b"0_0_0"] * HEAVY_RUNS[g]
    check_many(heads)
    return b"".join(rec(b"@V%d#%s/1" % (i, k), b"ACGTN"[:1 + i % 5]) for i, k in enumerate(heads))


def check_many(heads):
    """what the case is for: the heavy key's share and the lengths of its runs"""
    runs, n = [], 0
    for k in heads + [None]:
        if k == b"0_0_0":
            n += 1
        elif n:
            runs.append(n)
            n = 0
    assert len(heads) == 3000 and sum(runs) == 900 and tuple(runs) == HEAVY_RUNS and min(runs) > 64, (len(heads), runs)
    assert 390 <= len(set(heads)) <= 400, len(set(heads))


def cases():
    body = edge_body()
    return {"edge_whole": body, "edge_unterminated_header": body + b"@x#END_1/1", "edge_in_line2": body + b"@x#END_2/1\nAC",
            "edge_after_header": body + b"@x#END_3/1\n", "empty": b"", "many": many()}


def the_line(script):
    """the one uncommented line of the script that writes barcode_freq.txt"""
    found = [ln for ln in open(script).read().splitlines() if not ln.lstrip().startswith("#") and "> barcode_freq.txt" in ln.replace(">barcode", "> barcode")]
    assert len(found) == 1 and "split_reads.1.fq.gz" in found[0], found
    return found[0]


def main():
    line = the_line(os.path.abspath(sys.argv[1]))
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ, LC_ALL="C")
    for name, data in cases().items():
        with tempfile.TemporaryDirectory() as tmp:
            with gzip.open(os.path.join(tmp, name + ".fq.gz"), "wb") as f:
                f.write(data)
            subprocess.run(["bash", "-c", line.replace("split_reads.1.fq.gz", name + ".fq.gz")], cwd=tmp, check=True, env=env)
            rows = subprocess.run(["sort", "barcode_freq.txt"], cwd=tmp, check=True, env=env, stdout=subprocess.PIPE).stdout
        # the order of whole lines is the order of the keys here: no key is another one followed by a byte below the tab
        keys = [r.rsplit(b"\t", 1)[0] for r in rows.split(b"\n")[:-1]]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), name
        for fn, blob in ((name + ".fq", data), (name + ".txt", rows)):
            with open(os.path.join(OUT, fn), "wb") as f:
                f.write(blob)
        print(name, len(data), "bytes,", len(keys), "keys")


if __name__ == "__main__":
    main()
