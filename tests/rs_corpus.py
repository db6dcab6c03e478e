"""Inputs for the tests of stage 03's device ingest (rs_core.h, hast_rs_*, `classify_read --ingest device`): FASTA and FASTQ files
over the edge cases of the reference's two getline loops, an independent restatement of those loops (`read_file`), and the bound on
what a feed has to carry (`carry_bound`), the generator's condition under which no block size may refuse a file."""
import os
import random
import subprocess

from tests.conftest import ROOT

FASTA, FASTQ = 0, 1
WIDTHS = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097)           # FASTA line widths and FASTQ read lengths (0: the empty-line cases)
COUNTS = (0, 1, 255, 256, 257)
ERR = "format_error"


def make_keys(seed, k, n=40):
    rng = random.Random(seed)
    return [[bytes(rng.choice(b"ACGT") for _ in range(k)) for _ in range(n)] for _ in (0, 1)]


def rand_seq(rng, length, dirty=True):
    s = bytearray(rng.choice(b"ACGT") for _ in range(length))
    if dirty and length and rng.random() < 0.2:
        s[rng.randrange(length)] = rng.choice(b"Nnacgt")
    return s


def plant(rng, s, keys, at):
    key = rng.choice(keys[rng.randrange(2)])
    if 0 <= at and at + len(key) <= len(s):
        s[at:at + len(key)] = key


def seq_with_plants(rng, length, keys, width=None, dense=False):
    """random bases with planted keys: a few anywhere; width: one across every line end of a `width`-column layout; dense: back to back"""
    k = len(keys[0][0])
    s = rand_seq(rng, length, dirty=not dense)
    if dense:
        for at in range(rng.randrange(k), length - k, k):
            plant(rng, s, keys, at)
    elif width and width >= 2 * k:
        for e in range(width, length, width):
            plant(rng, s, keys, e - k // 2)
    else:
        for _ in range(rng.randint(0, 1 + length // 100)):
            plant(rng, s, keys, rng.randint(0, max(0, length - k)))
    return bytes(s)


def fasta_text(rng, records, width, brk=b"\n", blank=0.0):
    out = bytearray()
    for name, s in records:
        out += b">" + name + brk
        for j in range(0, len(s), width):
            out += s[j:j + width] + brk
            if rng.random() < blank:
                out += brk if rng.random() < 0.5 else b"\n"
        if rng.random() < blank:
            out += b"\n"
    return bytes(out)


def fastq_text(records, brk=b"\n"):
    return b"".join(b"@" + n + brk + s + brk + (b"+" if i % 2 else b"+" + n) + brk + b"I" * len(s) + brk for i, (n, s) in enumerate(records))


def records(rng, n, lens, keys, width=None):
    return [(b"r%d some/desc %d" % (i, i), seq_with_plants(rng, lens[i % len(lens)], keys, width)) for i in range(n)]


def corpus(keys, seed=1):
    """[(name, format, bytes)]"""
    rng = random.Random(seed)
    out = []
    mixed = (150, 0, 1, 63, 64, 65, 300)
    for w in WIDTHS:
        n = 40 if w < 4095 else 4
        out.append(("fa_w%d" % w, FASTA, fasta_text(rng, records(rng, n, (3 * w + 1, w, 2 * w, 0, w - 1, 1), keys, w), w)))
        out.append(("fq_l%d" % w, FASTQ, fastq_text(records(rng, n, (w,), keys))))
    out.append(("fq_l0", FASTQ, fastq_text(records(rng, 40, (0,), keys))))
    for n in COUNTS:
        out.append(("fa_n%d" % n, FASTA, fasta_text(rng, records(rng, n, mixed, keys, 60), 60)))
        out.append(("fq_n%d" % n, FASTQ, fastq_text(records(rng, n, mixed, keys))))
    # files that blocks of 64 bytes take: a FASTA record and the next header, a whole FASTQ record within 64 bytes
    tiny = [(b"t%d" % i, seq_with_plants(rng, (0, 1, 5, 12, 38)[i % 5], keys)) for i in range(300)]
    out.append(("fa_tiny", FASTA, b"junk\n\n" + fasta_text(rng, tiny, 7, blank=0.1) + b">t\nAC"))
    out.append(("fa_tiny_crlf", FASTA, fasta_text(rng, tiny, 16, b"\r\n")))
    tiny = [(b"t%d" % i, seq_with_plants(rng, (0, 1, 5, 12, 22)[i % 5], keys)) for i in range(300)]
    out.append(("fq_tiny", FASTQ, fastq_text(tiny) + b"@t\nACGT"))
    out.append(("fq_tiny_crlf", FASTQ, fastq_text(tiny[:100], b"\r\n")))
    out.append(("fa_crlf", FASTA, fasta_text(rng, records(rng, 50, mixed, keys, 60), 60, b"\r\n")))
    out.append(("fq_crlf", FASTQ, fastq_text(records(rng, 50, mixed, keys), b"\r\n")))
    out.append(("fa_blank", FASTA, b"\n\n" + fasta_text(rng, records(rng, 120, mixed, keys, 70), 70, blank=0.3)))
    junk = b"junk line before any header\nACGT\n\nmore junk " + b"x" * 50 + b"\n"
    body = fasta_text(rng, records(rng, 60, mixed, keys, 60), 60)
    out.append(("fa_junk", FASTA, junk + body))
    out.append(("fa_junk_only", FASTA, junk * 5))                                       # a file without any header
    out.append(("fa_junk_unterminated", FASTA, junk * 5 + b"ACGT"))
    out.append(("fa_header_only", FASTA, b">lonely\n" + body + b">also lonely\n>and a third\n" + body + b">at the end\n"))
    out.append(("fa_bare", FASTA, b">\n" + b"ACGTACGTAC" * 5 + b"\n>\n>\n" + body + b">\n"))
    out.append(("fa_unterminated_seq", FASTA, body + b">last\nACGTACGTACGTACGTACGTACGT\nTTTT"))      # the last line is dropped
    out.append(("fa_unterminated_header", FASTA, body + b">never seen"))
    out.append(("fa_one_unterminated", FASTA, b">only"))
    out.append(("empty_fa", FASTA, b""))
    out.append(("empty_fq", FASTQ, b""))
    out.append(("newline_fa", FASTA, b"\n"))
    out.append(("newline_fq", FASTQ, b"\n"))
    fq = fastq_text(records(rng, 30, mixed, keys))
    tail = [b"@tail x", seq_with_plants(rng, 45, keys), b"+", b"IIII"]
    for lines in (1, 2, 3):
        for terminated in (True, False):
            out.append(("fq_tail%d_%s" % (lines, "nl" if terminated else "nonl"), FASTQ,
                        fq + b"\n".join(tail[:lines]) + (b"\n" if terminated else b"")))
    out.append(("fq_empty_header", FASTQ, b"\nACGT\n+\nIIII\n" + fq + b"\n"))
    # each format error at the first, a middle and the last line
    fa_lines = fasta_text(rng, records(rng, 30, mixed, keys, 60), 60).split(b"\n")[:-1]
    fq_lines = fq.split(b"\n")[:-1]
    for where, pick in (("first", lambda n: 0), ("middle", lambda n: n // 2), ("last", lambda n: n - 1)):
        for c in (b"@", b"+"):
            ls = list(fa_lines)
            ls[pick(len(ls))] = c + ls[pick(len(ls))][1:]
            out.append(("fa_err_%s_%s" % (where, "at" if c == b"@" else "plus"), FASTA, b"\n".join(ls) + b"\n"))
        ls = list(fq_lines)
        i = pick(len(ls)) // 4 * 4
        ls[i] = b">" + ls[i][1:]
        out.append(("fq_err_%s" % where, FASTQ, b"\n".join(ls) + b"\n"))
    out.append(("fq_err_tail", FASTQ, fq + b">tail\nACGT"))
    return out


def read_file(fmt, data):
    """the reference's reader (processFasta / processFastq, restated line by line): [(name, sequence)] or ERR"""
    lines = data.split(b"\n")
    rest = lines.pop()                                  # what getline returns together with eof
    recs = []
    if fmt == FASTQ:
        pieces = lines + [rest]
        for i in range(0, len(lines), 4):               # `while(!getline(head).eof())`: a header needs its newline
            if lines[i][:1] == b">":
                return ERR
            recs.append((lines[i][1:], pieces[i + 1] if i + 1 < len(pieces) else b""))
        return recs
    cur = None
    for line in lines:                                  # the unterminated last line ends the loop unread
        if not line:
            continue
        if line[:1] in (b"@", b"+"):
            return ERR
        if line[:1] == b">":
            cur = [line[1:], bytearray()]
            recs.append(cur)
        elif cur is not None:
            cur[1] += line
    return [(n, bytes(s)) for n, s in recs]


def carry_bound(fmt, data):
    """the most bytes a feed has to carry from one view of this file to the next, wherever the views end"""
    if fmt == FASTQ:
        pieces = data.split(b"\n")
        return max([sum(len(p) + 1 for p in pieces[i:i + 4]) for i in range(0, len(pieces), 4)] + [1])
    bound, cur, seen = 1, 0, False
    for line in data.split(b"\n"):
        if line[:1] == b">":
            bound = max(bound, cur + len(line) + 1)     # the open record and the next header up to its newline
            cur, seen = 0, True
        if seen:
            cur += len(line) + 1
        bound = max(bound, cur, len(line) + 1)
    return bound


def rows_of(recs):
    return b"".join(n + b"\t" + s + b"\n" for n, s in recs)


def build_native(out_dir, sanitize=False):
    """tests/native/test_rs_core.cpp as a program, optionally under ASan + UBSan"""
    out = os.path.join(str(out_dir), "test_rs_core_san" if sanitize else "test_rs_core")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_rs_core.cpp")]
    subprocess.run(cmd, check=True)
    return out
