"""Inputs for the tests of the stage-00 device ingest (sq_core.h, hast_sq_*): strict four-line FASTQ on which the framer and the
host parser must agree, and seeded mutants of it that the framer must refuse unless the parser reads them the same way."""
import os
import random
import subprocess

from tests.conftest import ROOT

READ_LENS = (0, 1, 63, 64, 65, 150, 4097)
BREAKS = (b"\n", b"\r\n", b"\r\r\n")
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
BASES = b"ACGTacgtN"
QUALS = b"@+#>FI5"          # quality lines may start with '@' or '+'


def record(rng, i, length, brk, qual_first=None):
    seq = bytes(rng.choice(BASES) for _ in range(length))
    if seq[:1] == b"+":     # (never: '+' is no base; the generator's condition)
        raise AssertionError
    qual = bytearray(rng.choice(QUALS) for _ in range(length))
    if length and qual_first is not None:
        qual[0] = qual_first
    third = b"+" if i % 3 else b"+r%d" % i
    return b"@r%d/1" % i + brk + seq + brk + third + brk + bytes(qual) + brk


def fastq(seed, n_records, lens, brk, last_newline=True):
    """n_records strict four-line records, their lengths taken in turn from `lens`; the last line with or without its line break"""
    rng = random.Random(seed)
    out = bytearray()
    for i in range(n_records):
        out += record(rng, i, lens[i % len(lens)], brk, qual_first=(ord("@"), ord("+"), None)[i % 3])
    if n_records and not last_newline:
        del out[len(out) - len(brk):]
    return bytes(out)


def valid_corpus():
    """(name, bytes, longest record in bytes): every read length, line break, record count, with and without the last newline"""
    out = []
    for b, brk in enumerate(BREAKS):
        for length in READ_LENS:
            data = fastq(100 + length, 65 if length < 4097 else 5, (length,), brk)
            out.append(("len%d_b%d" % (length, b), data, 2 * length + 40))
        for n in COUNTS:
            for last in (True, False):
                lens = (150, 0, 1, 63, 64, 65) if n < 1000 else (150, 64, 1, 0, 65, 63, 150, 150)
                out.append(("n%d_b%d_%s" % (n, b, "nl" if last else "nonl"), fastq(7 * n + b, n, lens, brk, last), 2 * 150 + 40))
        out.append(("short_b%d" % b, fastq(5 + b, 257, (0, 1, 1, 0, 1), brk), 2 * 1 + 28))
        out.append(("long_b%d" % b, fastq(9 + b, 9, (4097, 150, 4097, 0), brk, False), 2 * 4097 + 40))
    return out


MUTANTS = ("blank_line", "split_seq", "split_qual", "seq_plus", "qual_short", "qual_long", "no_at", "fasta_header")


def mutate(data: bytes, kind: str, seed: int) -> bytes:
    """one seeded damage to a strict four-line input with '\\n' line breaks"""
    rng = random.Random(seed)
    lines = data.split(b"\n")
    tail = lines.pop()                      # b"" when the input ends with '\n'
    n_rec = len(lines) // 4
    r = rng.randrange(n_rec)
    h, s, p, q = 4 * r, 4 * r + 1, 4 * r + 2, 4 * r + 3
    if kind == "blank_line":
        lines.insert(rng.randrange(4 * r, 4 * r + 5), b"")
    elif kind in ("split_seq", "split_qual"):
        at = s if kind == "split_seq" else q
        while len(lines[at]) < 2:           # a line with something to split
            r = (r + 1) % n_rec
            at = 4 * r + (1 if kind == "split_seq" else 3)
        cut = rng.randrange(1, len(lines[at]))
        lines[at:at + 1] = [lines[at][:cut], lines[at][cut:]]
    elif kind == "seq_plus":
        lines[s] = b"+" + lines[s][1:]
    elif kind == "qual_short":
        while not lines[q]:
            r = (r + 1) % n_rec
            q = 4 * r + 3
        lines[q] = lines[q][1:]
    elif kind == "qual_long":
        lines[q] = lines[q] + b"I"
    elif kind == "no_at":
        lines[h] = b"r" + lines[h][1:]
    elif kind == "fasta_header":
        lines[h] = b">" + lines[h][1:]
    else:
        raise ValueError(kind)
    return b"\n".join(lines + [tail])


def build_native(out_dir, sanitize=False, shared=False):
    """tests/native/test_sq_core.cpp as a program (optionally under ASan + UBSan) or, shared=True, as the model's library"""
    src = os.path.join(ROOT, "tests", "native", "test_sq_core.cpp")
    if shared:
        out = os.path.join(str(out_dir), "libsq_model.so")
        cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DSQ_MODEL_LIB", "-o", out, src]
    else:
        out = os.path.join(str(out_dir), "test_sq_core_san" if sanitize else "test_sq_core")
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + ["-o", out, src]
    subprocess.run(cmd, check=True)
    return out


def build_parser_driver(out_dir):
    out = os.path.join(str(out_dir), "test_seqstream")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "native", "test_seqstream.cpp")], check=True)
    return out
